"""Pins tests/train_reference.py, the fp64 yardstick of the training gradients, without a GPU:
its forward against oracle/oracle.py (which the goldens pin to the reference model), its
gradients against central finite differences of its own fp64 loss, every committed seed's
empty fragility report, and its fp32 run taking the same side of every kink."""
import functools

import numpy as np
import pytest
import torch

import train_grad_cases as tc
import train_reference as tr
from oracle import oracle

IDS = [c.name for c in tc.CASES]


@functools.lru_cache(maxsize=None)
def _data(name):
    return tc.with_parameters(next(c for c in tc.CASES if c.name == name))


@functools.lru_cache(maxsize=None)
def _ref64(name):
    return tr.train_step(_data(name))


def test_case_table_covers_what_the_gradient_comparison_needs():
    """Every aggregator with hetero sum at d 64, and the special rows of block 0."""
    have = {(c.aggregator, c.hetero, c.hidden) for c in tc.CASES}
    for agg in tr.AGGREGATORS:
        assert (agg, "sum", 64) in have, agg
    assert len(set(IDS)) == len(IDS)
    for case in tc.CASES:
        data = _data(case.name)
        b0 = data["blocks"][0]
        for b in data["blocks"]:
            assert all(n % 32 for n in b["num_dst"].values())
        for a, b in zip(data["blocks"], data["blocks"][1:]):
            assert a["num_dst"] == b["num_src"]  # the next block's sources are these dst rows
        deg = {ce: np.diff(r[0]) for ce, r in b0["rels"].items()}
        used = {nt: np.zeros(n, bool) for nt, n in b0["num_src"].items()}
        for ce, (ip, ix, eids) in b0["rels"].items():
            assert ix.max() < b0["num_src"][ce[0]] and ip[-1] == ix.size == eids.size
            assert np.unique(eids).size == eids.size
            used[ce[0]][ix] = True
            assert deg[ce][1] == 1
            row3 = ix[ip[3]:ip[4]]
            assert np.unique(row3).size < row3.size  # repeated sources
        assert deg[tc.BUYS][0] == 0 and deg[tc.BOUGHT][0] == 0
        if case.relations != "single":
            assert deg[tc.CLICKS][0] > 0 and deg[tc.CLICKED][0] > 0
        heavy = (tc.BUYS, tc.BOUGHT) if case.relations == "single" else (tc.CLICKS, tc.CLICKED)
        assert all(deg[ce][2] >= 150 for ce in heavy)
        for nt, u in used.items():
            assert not u[-1] and b0["num_src"][nt] - 1 >= b0["num_dst"][nt]
        for ce, occ in data["occurrence"].items():
            assert occ.min() >= 1 and occ.max() <= 8
        assert all(s.size == tc.N_POS for s, _ in data["pos"].values())


@pytest.mark.parametrize("name", IDS)
def test_forward_matches_oracle(name):
    """The reference's forward, cast to fp32, is oracle.model_blocks + the head + the loss."""
    data, ref = _data(name), _ref64(name)
    blocks = [oracle.BlockGraph(b["rels"], b["num_dst"], data["occurrence"]) for b in data["blocks"]]
    h = oracle.model_blocks(blocks, data["feats"], data["sd"], data["aggregator"], data["hetero"],
                            data["norm"], data["embed"])
    assert h.keys() == ref["h"].keys()
    for nt in h:
        np.testing.assert_allclose(ref["h"][nt].astype(np.float32), h[nt], rtol=1e-4, atol=1e-5,
                                   err_msg=nt)
    if data["pred"] == "cos":
        ps, ns = oracle.cosine_prediction(data["pos"], h), oracle.cosine_prediction(data["neg"], h)
    else:
        p = {k[len("layer_nn."):]: v for k, v in oracle.split_state_dict(data["sd"])[2].items()}
        ps = oracle.predicting_module(data["pos"], h, p)
        ns = oracle.predicting_module(data["neg"], h, p)
    for got, want in ((ref["pos"], ps), (ref["neg"], ns)):
        assert got.keys() == want.keys()
        for ce in want:
            np.testing.assert_allclose(got[ce].astype(np.float32), want[ce], rtol=1e-4, atol=1e-5,
                                       err_msg=str(ce))
    loss = oracle.max_margin_loss(ps, ns, data["delta"], data["K"], data["recency"] is not None,
                                  data["recency"], data["mask"] is not None, data["mask"])
    np.testing.assert_allclose(np.float32(ref["loss"]), loss, rtol=1e-4, atol=1e-5)


@pytest.mark.parametrize("name", IDS)
def test_committed_seed_has_an_empty_fragility_report(name):
    """The cap on fragile entries is zero: a condition on the case, not a tolerance."""
    ref = _ref64(name)
    assert ref["report"].empty(), ref["report"].where
    assert ref["hinge_active"] >= 0.1


@pytest.mark.parametrize("name", IDS)
def test_gradients_match_central_finite_differences(name):
    """(L(θ + εv) − L(θ − εv)) / 2ε = <∇L, v> to relative 1e-6, ε = 1e-6, fp64 against fp64,
    along three seeded random directions over every parameter and both feature tables at once.

    v has unit norm per tensor: an entry of a tensor with n elements moves by about ε/√n, so
    a pre-activation moves by some 1e-6 at most — inside tau = 1e-5, the distance that the
    empty fragility report keeps every kink away.  Its magnitudes are random; where the
    gradient is not 0 its signs are the gradient's, and where the gradient is exactly 0 (dead
    ReLU units, max losers, unreferenced rows) the component keeps its random sign, so a
    gradient that is wrongly 0 somewhere still moves the loss and shows in the quotient.  Pure
    random signs do not reach the bound: fp64 rounding of L leaves about 4e-11 in the quotient
    (measured), and a direction of random signs over 10^5 elements is so nearly orthogonal to
    the gradient (<∇L, v> of a few 1e-5) that this floor alone is 1e-6 of it (3 of 69 trials
    miss, at 1.2e-6 to 7.8e-6).  With the non-zero terms all of one sign <∇L, v> is about half
    the gradient's norm per tensor."""
    data, ref = _data(name), _ref64(name)
    eps = 1e-6
    g = {**{"sd:" + k: v for k, v in ref["grads"].items()},
         **{"feats:" + k: v for k, v in ref["feat_grads"].items()}}
    assert all(v is None or np.isfinite(v).all() for v in g.values())
    for trial in range(3):
        rng = np.random.default_rng(1000 + trial)
        v = {}
        for k, t in g.items():
            d = rng.standard_normal(np.shape(data[k.split(":")[0]][k.split(":", 1)[1]]))
            if t is not None:
                d = np.where(t != 0, np.abs(d) * np.sign(t), d)
            v[k] = d / max(np.linalg.norm(d), 1e-300)

        def moved(sign):
            out = dict(data)
            for part in ("sd", "feats"):
                out[part] = {k: np.asarray(t, np.float64) + sign * eps * v[f"{part}:{k}"]
                             for k, t in data[part].items()}
            return out
        fd = (tr.loss_only(moved(+1)) - tr.loss_only(moved(-1))) / (2 * eps)
        dot = sum(float((g[k] * v[k]).sum()) for k in g if g[k] is not None)
        assert abs(fd - dot) <= 1e-6 * abs(dot), (trial, fd, dot)


@pytest.mark.parametrize("name", IDS)
def test_fp32_run_takes_the_same_side_of_every_kink(name):
    """The fp32 run of the reference — the yardstick of the GPU test's measured tolerances —
    has the ReLU masks and arg-max choices of the fp64 run."""
    ref32 = tr.train_step(_data(name), dtype=torch.float32, grad=False)
    assert _ref64(name)["report"].same_choices(ref32["report"]) is None
