"""The train/valid split cases shared by tests/golden/make_split_golden.py (which runs the
reference's train_valid_split on them and writes tests/golden/split_*.npz) and by the CPU and
GPU tests that compare gnnrec.sampling.train_valid_split with those fixtures."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

BUYS, BOUGHT = ("user", "buys", "item"), ("item", "bought-by", "user")
CLICKS, CLICKED = ("user", "clicks", "item"), ("item", "clicked-by", "user")
RELS = [BUYS, BOUGHT, CLICKS, CLICKED]  # fixtures name a relation by its index here
REVERSE = {BUYS: BOUGHT, BOUGHT: BUYS, CLICKS: CLICKED, CLICKED: CLICKS}
ETYPES = [BUYS, CLICKS]
N_USER, N_ITEM, N_BUYS, N_CLICKS = 300, 200, 3000, 5000
SUBTRAIN_SIZE, VALID_SIZE = 0.1, 0.2

# name -> (train_on_clicks, remove_train_eids, purchases_sample, clicks_sample)
CASES = {"clicks_full": (True, False, 1, 1),
         "clicks_removed_sampled": (True, True, 0.5, 0.3),
         "buys_sampled": (False, False, 0.7, 1)}
RAISING = (False, True, 1, 1)  # the last relation (clicks) is not trained: KeyError


def make_inputs():
    """The seeded graph (relation -> (src, dst), reverses sharing the edge order) and the
    test ground truth."""
    rng = np.random.default_rng(2024)
    bu, bi = rng.integers(0, N_USER, N_BUYS), rng.integers(0, N_ITEM, N_BUYS)
    cu, ci = rng.integers(0, N_USER, N_CLICKS), rng.integers(0, N_ITEM, N_CLICKS)
    edges = {BUYS: (bu, bi), BOUGHT: (bi, bu), CLICKS: (cu, ci), CLICKED: (ci, cu)}
    gt_test = (rng.integers(0, N_USER, 400), rng.integers(0, N_ITEM, 400))
    return {ce: (s.astype(np.int64), d.astype(np.int64)) for ce, (s, d) in edges.items()}, gt_test


def split_kwargs(case):
    toc, rte, ps, cs = case
    return dict(etypes=list(ETYPES), subtrain_size=SUBTRAIN_SIZE, valid_size=VALID_SIZE,
                reverse_etype=dict(REVERSE), train_on_clicks=toc, remove_train_eids=rte,
                clicks_sample=cs, purchases_sample=ps)


def flatten(result, coo_of):
    """The ten return values as {name: int64 array}; coo_of(train_graph, relation) -> (src,
    dst) numpy arrays.  Dict orders are kept as relation indices."""
    (train_graph, train_eids, valid_eids, subtrain_uids, valid_uids, test_uids, all_iids,
     gt_subtrain, gt_valid, all_eids) = result
    a = lambda x: np.asarray(x, dtype=np.int64)  # noqa: E731
    out = {"subtrain_uids": a(subtrain_uids), "valid_uids": a(valid_uids),
           "test_uids": a(test_uids), "all_iids": a(all_iids),
           "gt_subtrain_u": a(gt_subtrain[0]), "gt_subtrain_i": a(gt_subtrain[1]),
           "gt_valid_u": a(gt_valid[0]), "gt_valid_i": a(gt_valid[1])}
    for name, d in (("train_eids", train_eids), ("valid_eids", valid_eids),
                    ("all_eids", all_eids)):
        out[name + "_order"] = a([RELS.index(tuple(k)) for k in d])
        for k, v in d.items():
            out[f"{name}_{RELS.index(tuple(k))}"] = a(v)
    for r, ce in enumerate(RELS):
        s, d = coo_of(train_graph, ce)
        out[f"train_src_{r}"], out[f"train_dst_{r}"] = a(s), a(d)
    return out


def load_golden(name):
    with np.load(os.path.join(GOLDEN, f"split_{name}.npz")) as z:
        return {k: z[k] for k in z.files}


def assert_matches(got, want):
    assert sorted(got) == sorted(want), (sorted(got), sorted(want))
    for k in want:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)
