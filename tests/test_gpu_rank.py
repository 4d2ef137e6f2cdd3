"""GPU checks of the full-ranking evaluation (gnnrec.recs.rank_items / rank_for_graph /
ranks_to_metrics and the kernels of csrc/rank.hip): every rank must be the definition's
(tests/rank_cases.py) applied to the device's own ops.sddmm_cos matrix, exactly, whatever the
count pass put into the band.  tests/test_rank_cases_cpu.py shows on the CPU that the base
inputs keep every band under the cap, which the tests here assert as overflow_rows == 0."""
import functools

import numpy as np
import pytest
import torch

import golden_io
import rank_cases as rk
import recommend_cases as rc

pytestmark = pytest.mark.gpu


def _cu(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _scores(hu, hi):
    """score(u, v) for every pair: ops.sddmm_cos, the definition."""
    from gnnrec import ops
    U, n = hu.shape[0], hi.shape[0]
    src = torch.arange(U, device="cuda").repeat_interleave(n)
    dst = torch.arange(n, device="cuda").repeat(U)
    return ops.sddmm_cos(src, dst, _cu(hu), _cu(hi)).view(U, n).cpu().numpy()


@functools.lru_cache(maxsize=None)
def _case(kind, d):
    """Base tables, the device's score matrix, the exclusions, the pairs and their ranks by
    the definition with and without the exclusions: computed once, shared, never written."""
    hu, hi = rc.tables(kind, d)
    S = _scores(hu, hi)
    excl = rc.exclusions()
    us, gs = rk.pairs(S, excl)
    return hu, hi, S, excl, us, gs, rk.ranks(S, us, gs, *excl), rk.ranks(S, us, gs)


def _rank(hu, hi, us, gs, excl=None, **kw):
    from gnnrec import recs
    kw.setdefault("cand_cap", rk.CAND_CAP)
    ex = None if excl is None else (_cu(excl[0]), _cu(excl[1]))
    rank, vals, stats = recs.rank_items(_cu(hu), _cu(hi), _cu(np.asarray(us, np.int64)),
                                        _cu(np.asarray(gs, np.int64)), ex, return_stats=True, **kw)
    assert rank.dtype == torch.int64 and vals.dtype == torch.float32 and rank.is_cuda
    return rank.cpu().numpy(), vals.cpu().numpy(), stats


def _assert_definition(hu, hi, us, gs, excl=None, S=None, **kw):
    S = _scores(hu, hi) if S is None else S
    rank, vals, stats = _rank(hu, hi, us, gs, excl, **kw)
    ip, ix = excl if excl is not None else (None, None)
    np.testing.assert_array_equal(rank, rk.ranks(S, us, gs, ip, ix))
    np.testing.assert_array_equal(vals.view(np.int32),
                                  S[np.asarray(us), np.asarray(gs)].view(np.int32))   # bitwise
    return rank, stats


# ---------------------------------------------------------------- 1. the bound
@pytest.mark.parametrize("d,scale", [(d, 1.0) for d in rc.BOUND_DIMS] + list(rc.BOUND_SCALED))
def test_bound(d, scale):
    """|a - sddmm_cos| <= eps(d) and |a - cosine64| <= eps(d) + sddmm_cos's tolerance, a the
    stored scores of the loop the count pass runs."""
    from gnnrec import ops
    for kind in rc.KINDS:
        hu, hi = rc.bound_tables(kind, d, scale)
        a = ops.cos_scores_f32(ops.normalize_rows_f32(_cu(hu)),
                               ops.normalize_rows_f32(_cu(hi))).cpu().numpy().astype(np.float64)
        e_s = np.abs(a - _scores(hu, hi)).max()
        e_c = np.abs(a - rc.cosine64(hu, hi)).max()
        print(f"rank bound d={d} scale={scale:g} {kind}: max|a - sddmm_cos| = {e_s:.3e} "
              f"max|a - cosine64| = {e_c:.3e} eps = {rk.eps(d):.3e}")
        assert e_s <= rk.eps(d), (kind, e_s)
        assert e_c <= rk.eps(d) + rk.COS_TOL, (kind, e_c)


# ---------------------------------------------------------------- 2. the definition
@pytest.mark.parametrize("d", rk.DIMS)
@pytest.mark.parametrize("kind", rk.KINDS)
def test_ranks_are_the_definition(kind, d):
    hu, hi, S, excl, us, gs, want_ex, want_plain = _case(kind, d)
    for ex, want in ((excl, want_ex), (None, want_plain)):
        for bs in (7, 128, 8192):
            rank, vals, stats = _rank(hu, hi, us, gs, ex, batch_size=bs)
            np.testing.assert_array_equal(rank, want, err_msg=f"batch_size {bs}")
            np.testing.assert_array_equal(vals.view(np.int32), S[us, gs].view(np.int32))
            assert stats["fast_path"] and stats["overflow_rows"] == 0
            assert stats["eps"] == rk.eps(d) and stats["cand_cap"] == rk.CAND_CAP
            assert 1 <= stats["band_max"] < rk.CAND_CAP     # the held-out item itself is in it


# ---------------------------------------------------------------- 3. against recommend
@pytest.mark.parametrize("kind,d", [("normal", 16), ("relu", 64), ("lowrank", 128),
                                    ("midpoint", 160)])
def test_ranks_agree_with_recommend(kind, d):
    from gnnrec import recs
    hu, hi, S, excl, us, gs, want_ex, _ = _case(kind, d)
    k = 10
    ex = (_cu(excl[0]), _cu(excl[1]))
    idx, _ = recs.recommend(_cu(hu), _cu(hi), k, None, ex, sample=rc.SAMPLE, cand_cap=rc.CAND_CAP)
    idx = idx.cpu().numpy()
    assert (idx >= 0).all()
    lu = np.repeat(np.arange(rc.N_USERS), k)
    rank, _, stats = _rank(hu, hi, lu, idx.reshape(-1), excl)
    np.testing.assert_array_equal(rank.reshape(rc.N_USERS, k),
                                  np.tile(np.arange(1, k + 1), (rc.N_USERS, 1)))
    assert stats["overflow_rows"] == 0
    rank, _, _ = _rank(hu, hi, us, gs, excl)
    top = (rank >= 1) & (rank <= k)
    assert top.sum() >= 5 * rc.N_USERS
    np.testing.assert_array_equal(idx[us[top], rank[top] - 1], gs[top])


# ---------------------------------------------------------------- 4. tails
@pytest.mark.parametrize("n_items", [1, 31, 33, 1025])
def test_tails(n_items):
    hu, hi = rc.tables("normal", 16, 40, n_items, seed=4)
    S = _scores(hu, hi)
    excl = rc.exclusions(40, n_items, 0, min(6, n_items), seed=5)
    rng = np.random.default_rng(n_items)
    for P in (1, 127, 129):
        us, gs = rng.integers(0, 40, P), rng.integers(0, n_items, P)
        for ex in (None, excl):
            _, stats = _assert_definition(hu, hi, us, gs, ex, S=S)
            assert stats["fast_path"]


def test_empty_pair_set_and_empty_item_table():
    from gnnrec import recs
    hu, hi = rc.tables("normal", 16, 8, 20)
    none = torch.zeros(0, dtype=torch.int64, device="cuda")
    for table in (_cu(hi), _cu(hi[:0])):
        rank, vals, stats = recs.rank_items(_cu(hu), table, none, none, return_stats=True)
        assert tuple(rank.shape) == (0,) and tuple(vals.shape) == (0,)
        assert rank.dtype == torch.int64 and vals.dtype == torch.float32
        assert stats["overflow_rows"] == 0 and not stats["fast_path"]
    one = torch.zeros(1, dtype=torch.int64, device="cuda")
    with pytest.raises(ValueError, match="out of range"):
        recs.rank_items(_cu(hu), _cu(hi[:0]), one, one)
    with pytest.raises(ValueError, match="out of range"):
        recs.rank_items(_cu(hu), _cu(hi), one + 8, one)
    with pytest.raises(ValueError, match="out of range"):
        recs.rank_items(_cu(hu), _cu(hi), one, one - 1)


def test_zero_rows():
    """A zero user row scores 0 against every item (all tied: ranked by id); a zero item row
    scores 0 for every user."""
    hu, hi = rc.tables("normal", 16, 12, 300, seed=6)
    hu[3] = 0
    hi[5] = 0
    us = np.array([3, 3, 3, 0, 1, 7], np.int64)
    gs = np.array([0, 5, 299, 5, 5, 200], np.int64)
    rank, stats = _assert_definition(hu, hi, us, gs, cand_cap=512)
    np.testing.assert_array_equal(rank[:3], [1, 6, 300])
    assert stats["overflow_rows"] == 0 and stats["band_max"] == 300


# ---------------------------------------------------------------- 5. ties
def _tied(n_copies):
    hu, hi = rc.tables("normal", 64, 24, 5000, seed=7)
    hi = hi.copy()
    hi[1000:1000 + n_copies] = hi[1000]
    us = np.repeat(np.arange(24), 3).astype(np.int64)
    gs = np.tile(np.array([1000, 1000 + n_copies // 2, 1000 + n_copies - 1], np.int64), 24)
    return hu, hi, us, gs


def test_ties_are_resolved_by_id():
    hu, hi, _, _ = _tied(40)
    us = np.repeat(np.arange(24), 40).astype(np.int64)
    gs = np.tile(np.arange(1000, 1040, dtype=np.int64), 24)
    rank, stats = _assert_definition(hu, hi, us, gs)
    r = rank.reshape(24, 40)
    np.testing.assert_array_equal(r, r[:, :1] + np.arange(40))     # consecutive, in id order
    assert stats["overflow_rows"] == 0 and stats["band_max"] >= 40


@pytest.mark.parametrize("n_copies,cap", [(3000, 1024), (3000, 8), (40, 8)])
def test_ties_past_the_cap_take_the_exhaustive_path(n_copies, cap):
    hu, hi, us, gs = _tied(n_copies)
    excl = rc.exclusions(24, 5000, 0, 60, seed=8)
    for ex in (None, excl):
        rank, stats = _assert_definition(hu, hi, us, gs, ex, cand_cap=cap)
        assert stats["fast_path"] and stats["overflow_rows"] == us.size
        assert stats["band_max"] >= n_copies


# ---------------------------------------------------------------- 6. exclusion
def test_exclusion_lists():
    hu, hi = rc.tables("relu", 16, 6, 400, seed=9)
    S = _scores(hu, hi)
    order = np.argsort(-S[2], kind="stable")
    lists = [[], [7, 7, 3, 7, 399, 3], list(order[:50]) + list(order[:50][::-1]),
             [i for i in range(400) if i != 123], [0], list(range(400))]
    excl = rc.csr(lists)
    us = np.array([0, 1, 1, 1, 2, 2, 3, 4, 4, 5], np.int64)
    gs = np.array([9, 7, 3, 50, order[50], order[10], 123, 0, 1, 17], np.int64)
    rank, stats = _assert_definition(hu, hi, us, gs, excl, S=S)
    assert rank[1] == 0 and rank[2] == 0          # an excluded held-out item, listed repeatedly
    assert rank[4] == 1 and rank[5] == 0          # the 50 items ahead excluded, each twice
    assert rank[6] == 1                           # every other item excluded
    assert rank[7] == 0 and rank[9] == 0
    assert stats["overflow_rows"] == 0


def test_rank_for_graph_takes_the_graph_lists():
    """A multigraph: repeated purchases put duplicate ids into the bought-by CSR."""
    from gnnrec import recs
    from gnnrec.graph import HeteroGraph
    rng = np.random.default_rng(3)
    n_u, n_i, E = 60, 80, 500
    u, i = rng.integers(0, n_u, E), rng.integers(0, n_i, E)
    u, i = np.concatenate([u, u[:100]]), np.concatenate([i, i[:100]])
    edges = {("user", "buys", "item"): (u, i), ("item", "bought-by", "user"): (i, u)}
    g = HeteroGraph({ce: (torch.from_numpy(s), torch.from_numpy(d))
                     for ce, (s, d) in edges.items()}, {"user": n_u, "item": n_i}).to("cuda")
    hu, hi = rc.tables("normal", 16, n_u, n_i, seed=10)
    gu, gi = rng.integers(0, n_u, 200), rng.integers(0, n_i, 200)
    rank, vals = recs.rank_for_graph(g, {"user": _cu(hu), "item": _cu(hi)}, (gu, gi))
    lists = [[] for _ in range(n_u)]
    for a, b in zip(u.tolist(), i.tolist()):
        lists[a].append(b)
    np.testing.assert_array_equal(rank.cpu().numpy(),
                                  rk.ranks(_scores(hu, hi), gu, gi, *rc.csr(lists)))
    assert (rank == 0).any() and (rank > 0).any()


# ---------------------------------------------------------------- 7. widths
@pytest.mark.parametrize("d,fast", [(6, False), (100, True)])
def test_widths(d, fast):
    hu, hi = rc.tables("normal", d, 16, 600, seed=2)
    excl = rc.exclusions(16, 600, 0, 20, seed=3)
    rng = np.random.default_rng(d)
    us, gs = rng.integers(0, 16, 90), rng.integers(0, 600, 90)
    for ex in (None, excl):
        _, stats = _assert_definition(hu, hi, us, gs, ex)
        assert stats["fast_path"] == fast and stats["overflow_rows"] == 0


# ---------------------------------------------------------------- 8. the reference's data
def _lists(users, items, n_users):
    out = [[] for _ in range(n_users)]
    for u, i in zip(np.asarray(users).tolist(), np.asarray(items).tolist()):
        out[u].append(i)
    return out


@pytest.mark.parametrize("name", sorted(k for k, v in golden_io.manifest().items()
                                        if v["kind"] == "recs" and v["pred"] == "cos"
                                        and not v["use_popularity"]))
def test_reference_lists_and_ground_truth(name):
    meta = golden_io.manifest()[name]
    a = golden_io.load(name)
    hu, hi = a["h/user"], a["h/item"]
    bought = _lists(a["bought/u"], a["bought/i"], hu.shape[0])
    excl = rc.csr(bought)
    k = a["recs"].shape[1]
    ok = a["recs"] >= 0
    lu = np.repeat(a["user_ids"], k).reshape(-1, k)[ok]
    rank, _, stats = _rank(hu, hi, lu, a["recs"][ok], excl)
    np.testing.assert_array_equal(rank, np.tile(np.arange(1, k + 1), (len(a["user_ids"]), 1))[ok])
    assert stats["fast_path"]
    # the ground truth: within the reference's own near-ties of its stored position
    row_of = {int(u): r for r, u in enumerate(a["user_ids"])}
    keep = np.array([int(u) in row_of for u in a["gt/u"]])
    gu, gi = a["gt/u"][keep].astype(np.int64), a["gt/i"][keep].astype(np.int64)
    rank, _, _ = _rank(hu, hi, gu, gi, excl)
    tol = meta["min_rel_gap_required"]
    for u, g, q in zip(gu.tolist(), gi.tolist(), rank.tolist()):
        s = a["scores"][row_of[u]].astype(np.float64)
        if g in bought[u]:
            assert q == 0
            continue
        free = np.setdiff1d(np.arange(s.size), bought[u])
        ref = 1 + int(((s[free] > s[g]) | ((s[free] == s[g]) & (free < g))).sum())
        near = np.abs(s[free] - s[g]) <= tol * np.maximum(np.abs(s[free]), abs(s[g]))
        assert abs(q - ref) <= int(near.sum()) - 1, (u, g, q, ref)   # near holds g itself


# ---------------------------------------------------------------- 9. the metrics
def _assert_metrics(got, want):
    assert set(got) == set(want)
    for key, w in want.items():
        if isinstance(w, float) and np.isnan(w):
            assert np.isnan(got[key]), key
        else:
            assert got[key] == pytest.approx(w, rel=1e-12, abs=0), key


def test_metrics_match_the_restatement():
    from gnnrec import recs
    hu, hi, S, excl, us, gs, want_ex, _ = _case("normal", 64)
    m = recs.ranks_to_metrics(_cu(want_ex), _cu(us), rk.KS)
    _assert_metrics(m, rk.metrics(want_ex, us, rk.KS))
    assert m["unranked"] > 0 and 0 < m["recall@10"] < 1
    rank = np.array([1, 3, 3, 0, 12, 0], np.int64)
    users = np.array([4, 4, 4, 4, 9, 2], np.int64)
    _assert_metrics(recs.ranks_to_metrics(_cu(rank), _cu(users), (1, 3, 20)),
                    rk.metrics(rank, users, (1, 3, 20)))
    none = torch.zeros(0, dtype=torch.int64, device="cuda")
    _assert_metrics(recs.ranks_to_metrics(none, none, (10,)), rk.metrics([], [], (10,)))
    zeros = np.zeros(3, np.int64)
    _assert_metrics(recs.ranks_to_metrics(_cu(zeros), _cu(zeros), (10,)),
                    rk.metrics(zeros, zeros, (10,)))


def test_recall_is_recs_to_metrics_device_s():
    from gnnrec import recs
    hu, hi, S, excl, us, gs, _, _ = _case("relu", 16)
    k = 10
    ex = (_cu(excl[0]), _cu(excl[1]))
    rank, _ = recs.rank_items(_cu(hu), _cu(hi), _cu(us), _cu(gs), ex)
    m = recs.ranks_to_metrics(rank, _cu(us), (k,))
    rows = torch.arange(rc.N_USERS, device="cuda")
    idx, _ = recs.recommend(_cu(hu), _cu(hi), k, rows, ex, sample=rc.SAMPLE, cand_cap=rc.CAND_CAP)
    ip, ix = rc.csr(_lists(us, gs, rc.N_USERS))
    _, recall, _ = recs.recs_to_metrics_device(idx, rows, _cu(ip), _cu(ix), rc.N_ITEMS)
    hits = int(((rank >= 1) & (rank <= k)).sum())
    assert recall == hits / us.size == m[f"recall@{k}"]
