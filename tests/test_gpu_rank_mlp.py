"""GPU checks of the full-ranking evaluation for the MLP head (gnnrec.recs.rank_items(head=) /
rank_for_graph, the counting epilogues of the dense MLP kernel and its resolve kernel in
csrc/heads.hip with every pair a one-slot row).  The reference for
every value is ops.edge_mlp over the expanded pair list — the per-edge kernel, not the code under test — and for every rank the
definition of tests/rank_cases.py applied to that matrix (to ops.rating_rows_ of it for the
popularity-weighted form).  Everything is exact: ranks are compared with assert_array_equal,
values bit for bit.  tests/test_rank_mlp_cpu.py shows on the host that the saturated head and
the popularity vector used here really produce the exact ties the tie rule is tested on."""
import functools

import numpy as np
import pytest
import torch

import golden_io
import rank_cases as rk
import rank_mlp_cases as rm
import recommend_cases as rc
import recommend_mlp_cases as mc

pytestmark = pytest.mark.gpu

STATS_KEYS = {"band_mean", "band_max", "overflow_rows", "fast_path", "eps", "cand_cap"}


def _cu(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _bits(x):
    return np.ascontiguousarray(x).view(np.int32)


@functools.lru_cache(maxsize=None)
def _head(d, saturated=False):
    return (mc.saturated_head(d) if saturated else mc.head(d)).cuda()


def _tail(pl):
    return (pl.hidden_2.weight, pl.hidden_2.bias, pl.output.weight.reshape(-1), pl.output.bias)


def _PQ(pl, hu, hi):
    from gnnrec import ops
    d = hu.shape[1]
    W1 = pl.hidden_1.weight
    return (ops.gemm(_cu(hu), W1[:, :d], bias=pl.hidden_1.bias), ops.gemm(_cu(hi), W1[:, d:]))


def _edge_mlp_matrix(pl, P, Q):
    """score(u, v) for every pair: ops.edge_mlp over the expanded pair list, the definition."""
    from gnnrec import ops
    U, n = P.shape[0], Q.shape[0]
    src = torch.arange(U, device="cuda").repeat_interleave(n)
    dst = torch.arange(n, device="cuda").repeat(U)
    return ops.edge_mlp(src, dst, P, Q, *_tail(pl)).view(U, n)


def _matrix(pl, hu, hi):
    S = _edge_mlp_matrix(pl, *_PQ(pl, hu, hi)).cpu().numpy()
    S.setflags(write=False)
    return S


@functools.lru_cache(maxsize=None)
def _case(kind, d, saturated=False):
    """Base tables, the device's edge_mlp matrix, the exclusions, rank_cases' pairs and their
    ranks by the definition with and without the exclusions: computed once, never written."""
    hu, hi = rc.tables(kind, d)
    pl = _head(d, saturated)
    S = _matrix(pl, hu, hi)
    excl = rc.exclusions()
    us, gs = rk.pairs(S, excl)
    return hu, hi, pl, S, excl, us, gs, rk.ranks(S, us, gs, *excl), rk.ranks(S, us, gs)


def _rank(pl, hu, hi, us, gs, excl=None, **kw):
    from gnnrec import recs
    ex = None if excl is None else (_cu(excl[0]), _cu(excl[1]))
    rank, vals, stats = recs.rank_items(_cu(hu), _cu(hi), _cu(np.asarray(us, np.int64)),
                                        _cu(np.asarray(gs, np.int64)), ex, return_stats=True,
                                        head=pl, **kw)
    assert rank.dtype == torch.int64 and vals.dtype == torch.float32 and rank.is_cuda
    return rank.cpu().numpy(), vals.cpu().numpy(), stats


def _assert_stats(stats, cand_cap=1024):
    assert set(stats) == STATS_KEYS
    assert stats["fast_path"] is True and stats["overflow_rows"] == 0
    assert stats["band_mean"] == 0.0 and stats["band_max"] == 0 and stats["eps"] == 0.0
    assert stats["cand_cap"] == cand_cap


def _assert_definition(pl, hu, hi, us, gs, excl=None, S=None, **kw):
    S = _matrix(pl, hu, hi) if S is None else S
    rank, vals, stats = _rank(pl, hu, hi, us, gs, excl, **kw)
    ip, ix = excl if excl is not None else (None, None)
    np.testing.assert_array_equal(rank, rk.ranks(S, us, gs, ip, ix))
    np.testing.assert_array_equal(_bits(vals), _bits(S[np.asarray(us), np.asarray(gs)]))
    _assert_stats(stats, kw.get("cand_cap", 1024))
    return rank


# ---------------------------------------------------------------- 1. the count kernel alone
@functools.lru_cache(maxsize=None)
def _kernel_case(saturated):
    """P, Q of the 130 x 5000 'normal' tables (d = 64; the saturated head's d = 16) and their
    edge_mlp matrix, on the device."""
    d = rm.SATURATED_D if saturated else 64
    hu, hi = rc.tables("normal", d)
    pl = _head(d, saturated)
    P, Q = _PQ(pl, hu, hi)
    return pl, P.detach(), Q.detach(), _edge_mlp_matrix(pl, P, Q)


def _count_with_guard(op, lead, s, gid, n_rows, n_items):
    """The torch op itself with every row a single slot (lptr = 0 .. n_rows), its parts a view
    into a guarded buffer -> ahead."""
    from gnnrec import ops
    n_part = ops.denominator_parts(n_items)
    assert n_part == (n_items + 1023) // 1024
    guard = 1024
    buf = torch.full((n_part * n_rows + guard,), -7, dtype=torch.int32, device="cuda")
    parts = buf[:n_part * n_rows].view(n_part, n_rows)
    ahead = torch.full((n_rows,), -7, dtype=torch.int32, device="cuda")
    op(*lead, torch.arange(n_rows + 1, device="cuda"), s, gid, parts, ahead)
    torch.cuda.synchronize()
    assert (buf[n_part * n_rows:] == -7).all()          # nothing past the last chunk's row
    assert (parts >= 0).all()                            # every (chunk, row) slot written
    assert torch.equal(parts.sum(0, dtype=torch.int32), ahead)
    return ahead.cpu().numpy()


@pytest.mark.parametrize("saturated", [False, True])
@pytest.mark.parametrize("n_rows", rm.COUNT_ROWS)
def test_count_is_the_definition_without_exclusions(n_rows, saturated):
    """Every ragged edge of the 32-item tile, the 1024-item chunk and the 64-row group; with
    the saturated head nearly every compare is a tie decided by ids."""
    from gnnrec import _lib
    T = _lib.torch_ops()
    pl, P, Q, S = _kernel_case(saturated)
    tail = tuple(t.detach().contiguous() for t in _tail(pl))
    rows = np.arange(n_rows)
    for n_items in rm.COUNT_ITEMS:
        rng = np.random.default_rng([n_rows, n_items])
        g = rng.integers(0, n_items, n_rows)
        g[0], g[-1] = n_items - 1, 0                    # the last item (a partial tile) and the first
        Sn = S[:n_rows, :n_items].cpu().numpy()
        gid = _cu(g.astype(np.int32))
        thr = S[:n_rows, :n_items][torch.arange(n_rows, device="cuda"), _cu(g)].contiguous()
        lead = (P[:n_rows].contiguous(), Q[:n_items].contiguous(), *tail)
        ahead = _count_with_guard(T.edge_mlp_dense_count_lists_f32, lead, thr, gid, n_rows,
                                  n_items)
        np.testing.assert_array_equal(ahead, rk.ranks(Sn, rows, g) - 1, err_msg=f"{n_items} items")


@pytest.mark.parametrize("n_rows,n_items", [(1, 33), (65, 1025), (130, 5000)])
def test_count_rating_is_the_definition_without_exclusions(n_rows, n_items):
    """The rating form against the definition on ops.rating_rows_ of the edge_mlp matrix with
    the denominators recommend uses; the row's threshold is formed in the kernel from the raw
    score."""
    from gnnrec import _lib, ops
    T = _lib.torch_ops()
    pl, P, Q, S = _kernel_case(False)
    tail = tuple(t.detach().contiguous() for t in _tail(pl))
    Pn, Qn = P[:n_rows].contiguous(), Q[:n_items].contiguous()
    Z = ops.edge_mlp_dense_denominators(Pn, Qn, *tail)
    p = _cu(rm.popularity(n_items)) * 0.5
    R = ops.rating_rows_(S[:n_rows, :n_items].contiguous().clone(), Z, p).cpu().numpy()
    g = np.random.default_rng([7, n_rows, n_items]).integers(0, n_items, n_rows)
    s = S[:n_rows, :n_items][torch.arange(n_rows, device="cuda"), _cu(g)].contiguous()
    ahead = _count_with_guard(T.edge_mlp_dense_count_lists_rating_f32, (Pn, Qn, *tail, Z, p), s,
                              _cu(g.astype(np.int32)), n_rows, n_items)
    np.testing.assert_array_equal(ahead, rk.ranks(R, np.arange(n_rows), g) - 1)


def test_count_of_nothing():
    """No rows: nothing written.  No items: ahead = 0, no launch."""
    from gnnrec import ops
    pl, P, Q, _ = _kernel_case(False)
    none_f, none_i = torch.zeros(0, device="cuda"), torch.zeros(0, dtype=torch.int32, device="cuda")
    lptr = torch.arange(6, device="cuda")
    assert ops.edge_mlp_dense_count_lists(P[:0], Q, *_tail(pl), lptr[:1], none_f,
                                          none_i).numel() == 0
    thr, gid = torch.zeros(5, device="cuda"), torch.zeros(5, dtype=torch.int32, device="cuda")
    assert (ops.edge_mlp_dense_count_lists(P[:5], Q[:0], *_tail(pl), lptr, thr, gid) == 0).all()
    Z = torch.ones(5, device="cuda")
    assert (ops.edge_mlp_dense_count_lists_rating(P[:5], Q[:0], *_tail(pl), Z, none_f, lptr, thr,
                                                  gid) == 0).all()


# ---------------------------------------------------------------- 2. the definition
@pytest.mark.parametrize("d", mc.DIMS)
@pytest.mark.parametrize("kind", mc.KINDS)
def test_ranks_are_the_definition(kind, d):
    hu, hi, pl, S, excl, us, gs, want_ex, want_plain = _case(kind, d)
    for ex, want in ((excl, want_ex), (None, want_plain)):
        rank, vals, stats = _rank(pl, hu, hi, us, gs, ex)
        np.testing.assert_array_equal(rank, want)
        np.testing.assert_array_equal(_bits(vals), _bits(S[us, gs]))
        _assert_stats(stats)
    assert (want_ex == 0).sum() > 100 and (want_ex[5::8] > 4000).all()   # excluded; the worst item


def test_cand_cap_is_accepted_and_unused():
    hu, hi, pl, S, excl, us, gs, want_ex, _ = _case("relu", 64)
    for cap in (1, 4096):
        rank, _, stats = _rank(pl, hu, hi, us, gs, excl, cand_cap=cap)
        np.testing.assert_array_equal(rank, want_ex)
        _assert_stats(stats, cap)


# ---------------------------------------------------------------- 3. against recommend
@pytest.mark.parametrize("kind,d", [("normal", 16), ("relu", 64), ("lowrank", 128)])
def test_ranks_agree_with_recommend(kind, d):
    from gnnrec import recs
    hu, hi, pl, S, excl, us, gs, want_ex, _ = _case(kind, d)
    k = 10
    ex = (_cu(excl[0]), _cu(excl[1]))
    idx, _ = recs.recommend(_cu(hu), _cu(hi), k, None, ex, sample=rc.SAMPLE, cand_cap=rc.CAND_CAP,
                            head=pl)
    idx = idx.cpu().numpy()
    assert (idx >= 0).all()
    lu = np.repeat(np.arange(rc.N_USERS), k)
    rank, _, stats = _rank(pl, hu, hi, lu, idx.reshape(-1), excl)
    np.testing.assert_array_equal(rank.reshape(rc.N_USERS, k),
                                  np.tile(np.arange(1, k + 1), (rc.N_USERS, 1)))
    _assert_stats(stats)


# ---------------------------------------------------------------- 4. ties
def test_saturated_head_ranks_by_id():
    """~99.7 % of the scores are exactly 1.0f: the rank of most pairs is decided by ids."""
    hu, hi, pl, S, excl, us, gs, want_ex, want_plain = _case("normal", rm.SATURATED_D, True)
    assert (S == 1.0).mean() > 0.99
    assert rm.tied_both_sides(S, us, gs).mean() >= rm.TIED_BOTH_SIDES_MIN
    for ex, want in ((excl, want_ex), (None, want_plain)):
        rank, vals, stats = _rank(pl, hu, hi, us, gs, ex, batch_size=300)
        np.testing.assert_array_equal(rank, want)
        np.testing.assert_array_equal(_bits(vals), _bits(S[us, gs]))
        _assert_stats(stats)


def test_copied_rows_rank_in_id_order():
    """The held-out item's row copied to two lower and two higher ids (in other tiles and
    chunks): five bitwise equal scores per user, consecutive ranks in id order."""
    hu, hi = rc.tables("normal", 64, 24, 5000, seed=7)
    hi = hi.copy()
    copies = np.array([3, 999, 1000, 1024, 4999], np.int64)
    hi[copies] = hi[1000]
    pl = _head(64)
    S = _matrix(pl, hu, hi)
    assert (S[:, copies] == S[:, 1000:1001]).all()
    us = np.repeat(np.arange(24), copies.size).astype(np.int64)
    gs = np.tile(copies, 24)
    rank = _assert_definition(pl, hu, hi, us, gs, S=S)
    r = rank.reshape(24, copies.size)
    np.testing.assert_array_equal(r, r[:, :1] + np.arange(copies.size))


# ---------------------------------------------------------------- 5. exclusion
def test_exclusion_lists():
    hu, hi = rc.tables("relu", 16, 8, 400, seed=9)
    pl = _head(16)
    S = _matrix(pl, hu, hi)
    order = np.argsort(-S[2], kind="stable")
    best6 = np.argsort(-S[6], kind="stable")
    lists = [[], [7, 7, 3, 7, 399, 3],
             list(order[:50]) + list(order[:50][::-1]),          # 100 entries, 50 distinct
             [i for i in range(400) if i != 123], [0], list(range(400)),
             list(best6[:32]),                                    # exactly one resolve tile
             [400, 10 ** 6, 5, 401, 5], ]                         # ids past the table, a repeat
    assert len(lists[6]) == 32 and len(lists[2]) > 32
    excl = rc.csr(lists)
    us = np.array([0, 1, 1, 1, 2, 2, 3, 4, 4, 5, 6, 6, 7, 7, 0, 1], np.int64)
    gs = np.array([9, 7, 3, 50, order[50], order[10], 123, 0, 1, 17, best6[32], best6[31], 5,
                   399, 9, 50], np.int64)
    for bs in (8192, 5, 1):          # users repeated across pairs, within and across batches
        rank = _assert_definition(pl, hu, hi, us, gs, excl, S=S, batch_size=bs)
        assert rank[1] == 0 and rank[2] == 0          # an excluded held-out item, listed repeatedly
        assert rank[4] == 1 and rank[5] == 0          # the 50 items ahead excluded, each twice
        assert rank[6] == 1                           # every other item excluded
        assert rank[7] == 0 and rank[9] == 0
        assert rank[10] == 1 and rank[11] == 0        # the 32 best excluded
        assert rank[12] == 0                          # listed twice, among ids past the table
        assert rank[13] >= 1                          # 400, 401 and 10^6 name no item
        assert rank[14] == rank[0] and rank[15] == rank[3]


# ---------------------------------------------------------------- 6. empty and degenerate
def test_empty_pair_set_and_empty_item_table():
    from gnnrec import recs
    hu, hi = rc.tables("normal", 16, 8, 20)
    pl = _head(16)
    none = torch.zeros(0, dtype=torch.int64, device="cuda")
    for table in (_cu(hi), _cu(hi[:0])):
        rank, vals, stats = recs.rank_items(_cu(hu), table, none, none, return_stats=True, head=pl)
        assert tuple(rank.shape) == (0,) and tuple(vals.shape) == (0,)
        assert rank.dtype == torch.int64 and vals.dtype == torch.float32
        assert set(stats) == STATS_KEYS and stats["overflow_rows"] == 0 and stats["eps"] == 0.0
    one = torch.zeros(1, dtype=torch.int64, device="cuda")
    with pytest.raises(ValueError, match="out of range"):
        recs.rank_items(_cu(hu), _cu(hi[:0]), one, one, head=pl)
    with pytest.raises(ValueError, match="out of range"):
        recs.rank_items(_cu(hu), _cu(hi), one + 8, one, head=pl)
    with pytest.raises(ValueError, match="out of range"):
        recs.rank_items(_cu(hu), _cu(hi), one, one - 1, head=pl)
    with pytest.raises(ValueError, match="out of range"):
        recs.rank_items(_cu(hu), _cu(hi), one, one + 20, head=pl,
                        popularity=torch.zeros(20, device="cuda"))
    with pytest.raises(ValueError, match="hidden_1 must be"):
        recs.rank_items(_cu(hu), _cu(hi), one, one, head=_head(64))


def test_zero_rows():
    """A zero embedding row is a row like any other for this head."""
    hu, hi = rc.tables("normal", 16, 12, 300, seed=6)
    hu[3] = 0
    hi[5] = 0
    hi[77] = 0                       # two zero item rows: tied for every user
    us = np.array([3, 3, 3, 0, 1, 7, 2], np.int64)
    gs = np.array([0, 5, 299, 5, 77, 200, 77], np.int64)
    pl = _head(16)
    S = _matrix(pl, hu, hi)
    assert (S[:, 5] == S[:, 77]).all()
    rank = _assert_definition(pl, hu, hi, us, gs, S=S)
    assert rank[4] > rk.ranks(S, [1], [5])[0]         # 77 ranks behind its twin 5


# ---------------------------------------------------------------- 7. popularity
@functools.lru_cache(maxsize=None)
def _pop_case(weight):
    """The 'normal' d = 64 case with the popularity of rank_mlp_cases: the R matrix built by
    ops.rating_rows_ on the edge_mlp matrix with recommend's Z, rank_cases' pairs on it plus,
    per user, the two lowest ids of an exact R tie where the row has one."""
    from gnnrec import ops
    hu, hi = rc.tables("normal", 64)
    pl = _head(64)
    P, Q = _PQ(pl, hu, hi)
    pop = rm.popularity()
    p = _cu(pop) * float(weight)
    Z = ops.edge_mlp_dense_denominators(P, Q, *_tail(pl))
    R = ops.rating_rows_(_edge_mlp_matrix(pl, P, Q).clone(), Z, p).cpu().numpy()
    R.setflags(write=False)
    excl = rc.exclusions()
    us, gs = rk.pairs(R, excl)
    tu, tg = [], []
    for u in range(rc.N_USERS):
        vals, first, cnt = np.unique(R[u], return_index=True, return_counts=True)
        if (cnt > 1).any():
            v = vals[cnt > 1][-1]                       # the largest tied rating of the row
            ids = np.nonzero(R[u] == v)[0][:2]
            tu += [u, u]
            tg += ids.tolist()
    us = np.concatenate([us, np.asarray(tu, np.int64)])
    gs = np.concatenate([gs, np.asarray(tg, np.int64)])
    return hu, hi, pl, pop, R, excl, us, gs, len(tu)


@pytest.mark.parametrize("weight", rm.POP_WEIGHTS)
def test_popularity_ranks_are_the_definition_on_ratings(weight):
    from gnnrec import recs
    hu, hi, pl, pop, R, excl, us, gs, n_tied = _pop_case(weight)
    assert n_tied >= rc.N_USERS                         # at least half the rows hold an exact tie
    for ex in (excl, None):
        ip, ix = ex if ex is not None else (None, None)
        for bs in (8192, 500):
            rank, vals, stats = _rank(pl, hu, hi, us, gs, ex, popularity=_cu(pop),
                                      weight_popularity=weight, batch_size=bs)
            np.testing.assert_array_equal(rank, rk.ranks(R, us, gs, ip, ix))
            np.testing.assert_array_equal(_bits(vals), _bits(R[us, gs]))
            _assert_stats(stats)
    # recommend(head=, popularity=): position j of a user's list has rank j + 1
    k = 10
    exc = (_cu(excl[0]), _cu(excl[1]))
    idx, rv = recs.recommend(_cu(hu), _cu(hi), k, None, exc, sample=rc.SAMPLE, cand_cap=2048,
                             head=pl, popularity=_cu(pop), weight_popularity=weight)
    idx = idx.cpu().numpy()
    assert (idx >= 0).all()
    lu = np.repeat(np.arange(rc.N_USERS), k)
    rank, vals, _ = _rank(pl, hu, hi, lu, idx.reshape(-1), excl, popularity=_cu(pop),
                          weight_popularity=weight)
    np.testing.assert_array_equal(rank.reshape(rc.N_USERS, k),
                                  np.tile(np.arange(1, k + 1), (rc.N_USERS, 1)))
    np.testing.assert_array_equal(_bits(vals), _bits(rv.cpu().numpy().reshape(-1)))


def test_popularity_column_shape_and_refusals():
    from gnnrec import recs
    hu, hi, pl, pop, R, excl, us, gs, _ = _pop_case(0.5)
    a = recs.rank_items(_cu(hu), _cu(hi), _cu(us[:64]), _cu(gs[:64]), head=pl,
                        popularity=_cu(pop), weight_popularity=0.5)
    b = recs.rank_items(_cu(hu), _cu(hi), _cu(us[:64]), _cu(gs[:64]), head=pl,
                        popularity=_cu(pop.reshape(-1, 1)), weight_popularity=0.5)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    with pytest.raises(ValueError, match="popularity must be"):
        recs.rank_items(_cu(hu), _cu(hi), _cu(us[:4]), _cu(gs[:4]), head=pl,
                        popularity=_cu(pop[:-1]))
    with pytest.raises(NotImplementedError, match="needs head="):
        recs.rank_items(_cu(hu), _cu(hi), _cu(us[:4]), _cu(gs[:4]), popularity=_cu(pop))


# ---------------------------------------------------------------- 8. the graph entry
def test_rank_for_graph_takes_the_graph_lists_and_popularity():
    """A multigraph: repeated purchases put duplicate ids into the bought-by CSR."""
    from gnnrec import ops, recs
    from gnnrec.graph import HeteroGraph
    rng = np.random.default_rng(3)
    n_u, n_i, E = 60, 80, 500
    u, i = rng.integers(0, n_u, E), rng.integers(0, n_i, E)
    u, i = np.concatenate([u, u[:100]]), np.concatenate([i, i[:100]])
    edges = {("user", "buys", "item"): (u, i), ("item", "bought-by", "user"): (i, u)}
    g = HeteroGraph({ce: (torch.from_numpy(s), torch.from_numpy(d))
                     for ce, (s, d) in edges.items()}, {"user": n_u, "item": n_i}).to("cuda")
    hu, hi = rc.tables("normal", 16, n_u, n_i, seed=10)
    h = {"user": _cu(hu), "item": _cu(hi)}
    pl = _head(16)
    gu, gi = rng.integers(0, n_u, 200), rng.integers(0, n_i, 200)
    lists = [[] for _ in range(n_u)]
    for a, b in zip(u.tolist(), i.tolist()):
        lists[a].append(b)
    excl = rc.csr(lists)
    P, Q = _PQ(pl, hu, hi)
    Sd = _edge_mlp_matrix(pl, P, Q)
    S = Sd.cpu().numpy()
    rank, vals = recs.rank_for_graph(g, h, (gu, gi), head=pl)
    np.testing.assert_array_equal(rank.cpu().numpy(), rk.ranks(S, gu, gi, *excl))
    np.testing.assert_array_equal(_bits(vals.cpu().numpy()), _bits(S[gu, gi]))
    assert (rank == 0).any() and (rank > 0).any()
    with pytest.raises(KeyError, match="popularity"):
        recs.rank_for_graph(g, h, (gu, gi), head=pl, use_popularity=True)
    with pytest.raises(NotImplementedError, match="needs head="):
        recs.rank_for_graph(g, h, (gu, gi), use_popularity=True)
    pop = (rng.integers(0, 4, (n_i, 1)) / 4).astype(np.float32)   # a column, as the reference's
    g.nodes["item"].data["popularity"] = _cu(pop)
    wgt = 0.25
    Z = ops.edge_mlp_dense_denominators(P, Q, *_tail(pl))
    R = ops.rating_rows_(Sd.clone(), Z, _cu(pop.reshape(-1)) * wgt).cpu().numpy()
    rank, vals = recs.rank_for_graph(g, h, (gu, gi), head=pl, use_popularity=True,
                                     weight_popularity=wgt)
    np.testing.assert_array_equal(rank.cpu().numpy(), rk.ranks(R, gu, gi, *excl))
    np.testing.assert_array_equal(_bits(vals.cpu().numpy()), _bits(R[gu, gi]))


# ---------------------------------------------------------------- 9. the reference's data
def _lists(users, items, n_users):
    out = [[] for _ in range(n_users)]
    for u, i in zip(np.asarray(users).tolist(), np.asarray(items).tolist()):
        out[u].append(i)
    return out


@pytest.mark.parametrize("name", ["recs_nn", "recs_nn_k100"])
def test_reference_lists_and_ground_truth(name):
    from gnnrec.nn import PredictingLayer
    meta = golden_io.manifest()[name]
    a = golden_io.load(name)
    assert meta["pred"] == "nn" and not meta["use_popularity"]
    pl = PredictingLayer(meta["embed_dim"])
    pl.load_state_dict({k[2:]: torch.from_numpy(v) for k, v in a.items() if k.startswith("w/")})
    pl = pl.cuda().eval()
    hu, hi = a["h/user"], a["h/item"]
    bought = _lists(a["bought/u"], a["bought/i"], hu.shape[0])
    excl = rc.csr(bought)
    k = a["recs"].shape[1]
    ok = a["recs"] >= 0
    lu = np.repeat(a["user_ids"], k).reshape(-1, k)[ok]
    rank, _, stats = _rank(pl, hu, hi, lu, a["recs"][ok], excl)
    np.testing.assert_array_equal(rank, np.tile(np.arange(1, k + 1), (len(a["user_ids"]), 1))[ok])
    _assert_stats(stats)
    # the ground truth: within the reference's own near-ties of its stored position
    row_of = {int(u): r for r, u in enumerate(a["user_ids"])}
    keep = np.array([int(u) in row_of for u in a["gt/u"]])
    gu, gi = a["gt/u"][keep].astype(np.int64), a["gt/i"][keep].astype(np.int64)
    rank, _, _ = _rank(pl, hu, hi, gu, gi, excl)
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


# ---------------------------------------------------------------- 10. the cosine path
def test_cosine_path_is_unchanged():
    """rank_items without head= (and with head=None spelled out): the ranks of the definition
    on ops.sddmm_cos, its values bit for bit, the same stats keys and values as before."""
    from gnnrec import ops, recs
    hu, hi = rc.tables("relu", 64)
    U, n = hu.shape[0], hi.shape[0]
    src = torch.arange(U, device="cuda").repeat_interleave(n)
    dst = torch.arange(n, device="cuda").repeat(U)
    S = ops.sddmm_cos(src, dst, _cu(hu), _cu(hi)).view(U, n).cpu().numpy()
    excl = rc.exclusions()
    us, gs = rk.pairs(S, excl)
    ex = (_cu(excl[0]), _cu(excl[1]))
    a = recs.rank_items(_cu(hu), _cu(hi), _cu(us), _cu(gs), ex, return_stats=True)
    b = recs.rank_items(_cu(hu), _cu(hi), _cu(us), _cu(gs), ex, return_stats=True, head=None,
                        popularity=None)
    np.testing.assert_array_equal(a[0].cpu().numpy(), rk.ranks(S, us, gs, *excl))
    np.testing.assert_array_equal(_bits(a[1].cpu().numpy()), _bits(S[us, gs]))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and a[2] == b[2]
    assert set(a[2]) == STATS_KEYS
    assert a[2]["fast_path"] and a[2]["eps"] == rk.eps(64) and a[2]["band_max"] >= 1
    assert a[2]["overflow_rows"] == 0 and a[2]["cand_cap"] == 1024
