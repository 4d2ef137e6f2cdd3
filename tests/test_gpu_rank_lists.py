"""GPU checks of the list-shaped full-ranking evaluation (gnnrec.recs.rank_lists / list_pairs /
rank_lists_for_graph, the list forms of the dense MLP kernel's counting epilogue and
rank_resolve_mlp_lists in csrc/heads.hip).  The reference for every value is
ops.edge_mlp over the expanded pair list — the per-edge kernel, never the code under test — and
for every rank the definition of tests/rank_cases.py applied to that matrix (to ops.rating_rows_
of it for the popularity-weighted form); the lists' pairs and the row plan of the kernel tests
are the numpy restatements of tests/rank_lists_cases.py.  Everything is exact: ranks are
compared with assert_array_equal, values bit for bit.  The cases (tables, heads, matrices) are
test_gpu_rank_mlp's, computed once for both files."""
import functools

import numpy as np
import pytest
import torch

import rank_cases as rk
import rank_lists_cases as rl
import rank_mlp_cases as rm
import recommend_cases as rc
import recommend_mlp_cases as mc
from test_gpu_rank_mlp import (STATS_KEYS, _bits, _case, _cu, _edge_mlp_matrix, _head,
                               _kernel_case, _pop_case, _PQ, _tail)

pytestmark = pytest.mark.gpu

LIST_STATS_KEYS = STATS_KEYS | {"rows", "pairs"}


def _plan_rows(lens):
    return int((-(-np.asarray(lens) // rl.BUDGET)).sum())


# ---------------------------------------------------------------- 1. the count kernel alone
def _count_lists_with_guard(op, lead, lptr, s, gid, n_items):
    """The torch op itself, its parts a view into a guarded buffer -> ahead."""
    from gnnrec import ops
    E = s.numel()
    n_part = ops.denominator_parts(n_items)
    assert n_part == (n_items + 1023) // 1024
    guard = 1024
    buf = torch.full((n_part * E + guard,), -7, dtype=torch.int32, device="cuda")
    parts = buf[:n_part * E].view(n_part, E)
    ahead = torch.full((E,), -7, dtype=torch.int32, device="cuda")
    op(*lead, lptr, s, gid, parts, ahead)
    torch.cuda.synchronize()
    assert (buf[n_part * E:] == -7).all()               # nothing past the last chunk's slots
    assert (parts >= 0).all()                            # every (chunk, slot) written
    assert torch.equal(parts.sum(0, dtype=torch.int32), ahead)
    return ahead.cpu().numpy()


def _kernel_inputs(S, P, n_users, n_items):
    """rank_lists_cases' lists for the shape: their pairs, the plan's P rows and lptr, the
    entries' own scores (gathered from the edge_mlp matrix) and items."""
    ip, ix = rl.kernel_lists(n_users, n_items)
    us, gs = rl.list_pairs(None, ip, ix)
    owner, lptr = rl.row_plan(np.diff(ip))
    assert owner.size == _plan_rows(np.diff(ip)) and np.diff(lptr).max() == rl.BUDGET
    thr = S[_cu(us), _cu(gs)].contiguous()
    return us, gs, owner, P[:n_users][_cu(owner)].contiguous(), _cu(lptr), thr, \
        _cu(gs.astype(np.int32))


@pytest.mark.parametrize("saturated", [False, True])
@pytest.mark.parametrize("n_users", rl.COUNT_ROWS)
def test_count_lists_is_the_definition_without_exclusions(n_users, saturated):
    """Every ragged edge of the 32-item tile, the 1024-item chunk, the 64-row group and the
    16-slot row (lists of 0, 1, 2, 15, 16, 17 and 200 entries).  Condition on the inputs, shown
    on the host by test_rank_lists_cpu.py and asserted here on the device's own matrix: with
    the saturated head at least rl.TIED_BOTH_SIDES_MIN of the entries have an exactly tied item
    on both sides of their id, so their count is decided by the id rule."""
    from gnnrec import _lib
    T = _lib.torch_ops()
    pl, P, Q, S = _kernel_case(saturated)
    tail = tuple(t.detach().contiguous() for t in _tail(pl))
    for n_items in rl.COUNT_ITEMS:
        us, gs, owner, Pr, lptr, thr, gid = _kernel_inputs(S, P, n_users, n_items)
        Sn = S[:n_users, :n_items].cpu().numpy()
        ahead = _count_lists_with_guard(T.edge_mlp_dense_count_lists_f32,
                                        (Pr, Q[:n_items].contiguous(), *tail), lptr, thr, gid,
                                        n_items)
        np.testing.assert_array_equal(ahead, rk.ranks(Sn, us, gs) - 1, err_msg=f"{n_items} items")
    if saturated:
        both = rm.tied_both_sides(Sn, us, gs).mean()
        print(f"{n_users} users x {n_items} items: tied on both sides {both:.4f}")
        assert both >= rl.TIED_BOTH_SIDES_MIN


@pytest.mark.parametrize("saturated,weight", [(False, 0.5), (False, 0.0), (True, 0.5)])
@pytest.mark.parametrize("n_users", rl.COUNT_ROWS)
def test_count_lists_rating_is_the_definition_without_exclusions(n_users, saturated, weight):
    """The rating form over the plain form's whole grid, against the definition on
    ops.rating_rows_ of the edge_mlp matrix with the denominators recommend uses (per USER,
    gathered to the plan's rows); a slot's threshold is formed in the kernel from its raw score.
    rank_mlp_cases' popularity has 8 levels: with weight 0.0 equal softmax terms tie exactly,
    and with the saturated head (every softmax term of a row nearly the same) the ratings of a
    row fall on the popularity's levels, so — the same condition as for the plain form — at
    least rl.TIED_BOTH_SIDES_MIN of the entries have an exactly tied rating on both sides of
    their id."""
    from gnnrec import _lib, ops
    T = _lib.torch_ops()
    pl, P, Q, S = _kernel_case(saturated)
    tail = tuple(t.detach().contiguous() for t in _tail(pl))
    for n_items in rl.COUNT_ITEMS:
        Qn = Q[:n_items].contiguous()
        Z = ops.edge_mlp_dense_denominators(P[:n_users].contiguous(), Qn, *tail)
        p = _cu(rm.popularity(n_items)) * float(weight)
        R = ops.rating_rows_(S[:n_users, :n_items].contiguous().clone(), Z, p).cpu().numpy()
        us, gs, owner, Pr, lptr, s, gid = _kernel_inputs(S, P, n_users, n_items)
        ahead = _count_lists_with_guard(T.edge_mlp_dense_count_lists_rating_f32,
                                        (Pr, Qn, *tail, Z[_cu(owner)].contiguous(), p), lptr, s,
                                        gid, n_items)
        np.testing.assert_array_equal(ahead, rk.ranks(R, us, gs) - 1, err_msg=f"{n_items} items")
    if saturated:
        both = rm.tied_both_sides(R, us, gs).mean()
        print(f"{n_users} users x {n_items} items: ratings tied on both sides {both:.4f}")
        assert both >= rl.TIED_BOTH_SIDES_MIN


def test_count_lists_ids_that_name_no_item():
    """gid -1 and gid >= n_items read nothing: the compare runs on the id as it is (no item
    equals it; every item is above -1 and below n_items) and the rating form's threshold takes
    popularity 0."""
    from gnnrec import ops
    pl, P, Q, S = _kernel_case(False)
    n_users, n_items = 3, 1025
    Sn = S[:n_users, :n_items].cpu().numpy()
    Pn, Qn = P[:n_users].contiguous(), Q[:n_items].contiguous()
    lptr = _cu(np.array([0, 2, 4, 6], np.int64))
    gid = _cu(np.array([-1, n_items, -1, 10 ** 6, n_items, -1], np.int32))
    thr = _cu(np.ascontiguousarray(Sn[[0, 0, 1, 1, 2, 2], [5, 5, 6, 6, 7, 7]]))
    ahead = ops.edge_mlp_dense_count_lists(Pn, Qn, *_tail(pl), lptr, thr, gid).cpu().numpy()
    rows, t = Sn[[0, 0, 1, 1, 2, 2]], thr.cpu().numpy()[:, None]
    want = np.where(gid.cpu().numpy() < 0, (rows > t).sum(1), (rows >= t).sum(1))
    np.testing.assert_array_equal(ahead, want)
    Z = ops.edge_mlp_dense_denominators(Pn, Qn, *_tail(pl))
    p = _cu(rm.popularity(n_items)) * 0.5
    R = ops.rating_rows_(S[:n_users, :n_items].contiguous().clone(), Z, p).cpu().numpy()
    t = ops.rating_rows_(thr.view(n_users, 2).clone(), Z, torch.zeros(2, device="cuda"))
    ahead = ops.edge_mlp_dense_count_lists_rating(Pn, Qn, *_tail(pl), Z, p, lptr, thr,
                                                  gid).cpu().numpy()
    rows, t = R[[0, 0, 1, 1, 2, 2]], t.cpu().numpy().reshape(-1, 1)
    want = np.where(gid.cpu().numpy() < 0, (rows > t).sum(1), (rows >= t).sum(1))
    np.testing.assert_array_equal(ahead, want)


def test_count_lists_of_nothing():
    """No slots: nothing written.  No items: ahead = 0, no launch."""
    from gnnrec import ops
    pl, P, Q, _ = _kernel_case(False)
    none_f, none_i = torch.zeros(0, device="cuda"), torch.zeros(0, dtype=torch.int32, device="cuda")
    one = torch.zeros(1, dtype=torch.int64, device="cuda")
    assert ops.edge_mlp_dense_count_lists(P[:0], Q, *_tail(pl), one, none_f, none_i).numel() == 0
    lptr = _cu(np.array([0, 2, 2, 5], np.int64))
    thr, gid = torch.zeros(5, device="cuda"), torch.zeros(5, dtype=torch.int32, device="cuda")
    assert (ops.edge_mlp_dense_count_lists(P[:3], Q[:0], *_tail(pl), lptr, thr, gid) == 0).all()
    Z = torch.ones(3, device="cuda")
    assert (ops.edge_mlp_dense_count_lists_rating(P[:3], Q[:0], *_tail(pl), Z, none_f, lptr, thr,
                                                  gid) == 0).all()


# ---------------------------------------------------------------- 2. the resolve kernel alone
def test_resolve_lists_subtracts_each_rows_exclusions_once():
    """Rows with 0, 1, 31, 32, 33 and 60 excluded entries (the resolve's 32-entry tile), struck
    entries (-1) and an id past the table among them; every user's list holds an excluded item
    (rank 0) between ranked ones, one list is long enough for two rows, and the rows are served
    in descending user order.  ahead is the definition's count without exclusions."""
    from gnnrec import ops
    n_users, n_items = 6, 400
    hu, hi = rc.tables("relu", 16, n_users, n_items, seed=9)
    pl = _head(16)
    P, Q = _PQ(pl, hu, hi)
    Sd = _edge_mlp_matrix(pl, P, Q)
    S = Sd.cpu().numpy()
    rng = np.random.default_rng(5)
    sizes = (0, 1, 31, 32, 33, 60)
    excl_lists, held, first = [], [], []
    for u, n in enumerate(sizes):
        best = np.argsort(-S[u], kind="stable")
        x = best[:n].astype(np.int64)                   # the n best: every one is ahead of the rest
        if n >= 33:
            x[[3, n - 1]] = -1                          # struck repeats, one in the last tile
        if n == 60:
            x[40] = n_items + 7                         # an id past the table: no item
        kept = x[(x >= 0) & (x < n_items)]
        mine = [int(best[n]), int(best[-1])] + rng.integers(0, n_items, 3).tolist()
        if kept.size:
            mine.insert(1, int(kept[0]))                # an excluded item: rank 0
        if u == 5:
            mine += rng.integers(0, n_items, 20).tolist() + [int(kept[-1]), mine[0]]
        excl_lists.append(x)
        held.append(mine)
        first.append(1 + n - kept.size)                 # the struck entries' items stay ahead
    ex = rc.csr(excl_lists)
    gt = rc.csr(held)
    assert np.diff(gt[0]).max() > rl.BUDGET
    rows = np.arange(n_users)[::-1].copy()
    us, gs = rl.list_pairs(rows, *gt)
    owner, lptr = rl.row_plan(np.diff(gt[0])[rows])
    row_user = _cu(rows[owner])
    Pr = P[row_user].contiguous()
    gid, lp = _cu(gs.astype(np.int32)), _cu(lptr)
    s = Sd[_cu(us), _cu(gs)].contiguous()
    Z = ops.edge_mlp_dense_denominators(P, Q, *_tail(pl))
    p = _cu(rm.popularity(n_items)) * 0.5
    R = ops.rating_rows_(Sd.clone(), Z, p).cpu().numpy()
    for M, rated in ((S, False), (R, True)):
        ahead = _cu((rk.ranks(M, us, gs) - 1).astype(np.int32))
        rank = torch.full((us.size,), -7, dtype=torch.int64, device="cuda")
        vals = torch.full((us.size,), -7.0, device="cuda")
        ops.rank_resolve_mlp_lists(row_user, lp, s, gid, ahead, n_users, Pr, Q, *_tail(pl),
                                   _cu(ex[0]), _cu(ex[1]), Z[row_user].contiguous() if rated
                                   else None, p if rated else None, rank, vals)
        rank = rank.cpu().numpy()
        np.testing.assert_array_equal(rank, rk.ranks(M, us, gs, *ex))
        np.testing.assert_array_equal(_bits(vals.cpu().numpy()), _bits(M[us, gs]))
        for u in range(1, n_users):                     # an excluded slot, the others ranked
            mine = rank[us == u]
            assert mine[1] == 0 and mine[2] > 0 and (rated or mine[0] == first[u])
        assert (rank[us == 0] > 0).all()
        # without exclusions: 1 + ahead
        rank, _ = ops.rank_resolve_mlp_lists(row_user, lp, s, gid, ahead, n_users, Pr, Q,
                                             *_tail(pl), None, None,
                                             Z[row_user].contiguous() if rated else None,
                                             p if rated else None)
        np.testing.assert_array_equal(rank.cpu().numpy(), ahead.cpu().numpy() + 1)


# ---------------------------------------------------------------- 3. + 5. end to end, the contract
@functools.lru_cache(maxsize=None)
def _lists_case(kind, d):
    """test_gpu_rank_mlp's case with rank_cases' pairs regrouped into lists (plus users with 0,
    1 and 200 entries), the lists' pairs and their ranks by the definition: computed once."""
    hu, hi, pl, S, excl, us, gs, _, _ = _case(kind, d)
    ip, ix = rl.grouped(us, gs, S.shape[1])
    lu, lg = rl.list_pairs(None, ip, ix)
    return hu, hi, pl, S, excl, ip, ix, lu, lg, rk.ranks(S, lu, lg, *excl), rk.ranks(S, lu, lg)


def _rank_lists(pl, hu, hi, ip, ix, rows=None, excl=None, **kw):
    from gnnrec import recs
    ex = None if excl is None else (_cu(excl[0]), _cu(excl[1]))
    rank, vals, stats = recs.rank_lists(_cu(hu), _cu(hi), None if rows is None else _cu(rows),
                                        _cu(ip), _cu(ix), ex, return_stats=True, head=pl, **kw)
    assert rank.dtype == torch.int64 and vals.dtype == torch.float32 and rank.is_cuda
    return rank.cpu().numpy(), vals.cpu().numpy(), stats


def _rank_items_on_list_pairs(pl, hu, hi, ip, ix, rows=None, excl=None, **kw):
    """The contract's right-hand side: rank_items on recs.list_pairs of the same lists."""
    from gnnrec import recs
    ex = None if excl is None else (_cu(excl[0]), _cu(excl[1]))
    us, gs = recs.list_pairs(None if rows is None else _cu(rows), _cu(ip), _cu(ix))
    rank, vals, stats = recs.rank_items(_cu(hu), _cu(hi), us, gs, ex, return_stats=True, head=pl,
                                        **kw)
    return rank.cpu().numpy(), vals.cpu().numpy(), stats, us.cpu().numpy(), gs.cpu().numpy()


def _assert_list_stats(stats, lens, cand_cap=1024):
    assert set(stats) == LIST_STATS_KEYS
    assert stats["fast_path"] is True and stats["overflow_rows"] == 0
    assert stats["band_mean"] == 0.0 and stats["band_max"] == 0 and stats["eps"] == 0.0
    assert stats["cand_cap"] == cand_cap
    assert stats["pairs"] == int(np.sum(lens)) and stats["rows"] == _plan_rows(lens)


def _by_user(users):
    """Entries in (user, list position) order: aligns two calls that serve the same users in
    another order."""
    return np.argsort(users, kind="stable")


@pytest.mark.parametrize("d", mc.DIMS)
@pytest.mark.parametrize("kind", mc.KINDS)
def test_rank_lists_is_the_definition_and_rank_items(kind, d):
    """rank_items(head=) now runs the same kernels on the expanded pairs, one slot a row, so its
    half is no longer independent evidence: the definition half carries the proof."""
    hu, hi, pl, S, excl, ip, ix, lu, lg, want_ex, want_plain = _lists_case(kind, d)
    lens = np.diff(ip)
    assert lens[rl.EMPTY_USER] == 0 and lens[rl.SINGLE_USER] == 1 and lens[rl.LONG_USER] == rl.LONG
    for ex, want in ((excl, want_ex), (None, want_plain)):
        rank, vals, stats = _rank_lists(pl, hu, hi, ip, ix, None, ex)
        np.testing.assert_array_equal(rank, want)
        np.testing.assert_array_equal(_bits(vals), _bits(S[lu, lg]))
        _assert_list_stats(stats, lens)
        assert stats["rows"] == rc.N_USERS - 1 + 12        # one row a user, 13 for the long list
        r2, v2, s2, us, gs = _rank_items_on_list_pairs(pl, hu, hi, ip, ix, None, ex)
        np.testing.assert_array_equal(us, lu)
        np.testing.assert_array_equal(gs, lg)
        np.testing.assert_array_equal(rank, r2)
        np.testing.assert_array_equal(_bits(vals), _bits(v2))
        assert {k: stats[k] for k in STATS_KEYS} == s2
    assert (want_ex == 0).sum() > 100
    # the same entries whatever the batch and the order of the users
    rank, vals, _ = _rank_lists(pl, hu, hi, ip, ix, None, excl)
    for bs in rl.BATCHES:
        r, v, stats = _rank_lists(pl, hu, hi, ip, ix, None, excl, batch_size=bs)
        np.testing.assert_array_equal(r, rank)
        np.testing.assert_array_equal(_bits(v), _bits(vals))
        _assert_list_stats(stats, lens)
    rows = np.arange(rc.N_USERS)[::-1].copy()
    r, v, _ = _rank_lists(pl, hu, hi, ip, ix, rows, excl, batch_size=50)
    ru, rg = rl.list_pairs(rows, ip, ix)
    a, b = _by_user(lu), _by_user(ru)
    np.testing.assert_array_equal(rg[b], lg[a])
    np.testing.assert_array_equal(r[b], rank[a])
    np.testing.assert_array_equal(_bits(v[b]), _bits(vals[a]))


def test_rank_lists_serves_a_subset_with_the_saturated_head():
    """An unsorted subset of the users (the empty, the single and the long list among them), the
    head whose scores are nearly all 1.0f: ranks by ids; cand_cap accepted and unused."""
    hu, hi, pl, S, excl, us, gs, _, _ = _case("normal", rm.SATURATED_D, True)
    ip, ix = rl.grouped(us, gs, S.shape[1])
    rows = np.array([129, 7, 3, 64, 5, 0, 63, 100], np.int64)
    lu, lg = rl.list_pairs(rows, ip, ix)
    assert rm.tied_both_sides(S, lu, lg).mean() >= rl.TIED_BOTH_SIDES_MIN
    for bs in (8192, 3):
        rank, vals, stats = _rank_lists(pl, hu, hi, ip, ix, rows, excl, batch_size=bs, cand_cap=1)
        np.testing.assert_array_equal(rank, rk.ranks(S, lu, lg, *excl))
        np.testing.assert_array_equal(_bits(vals), _bits(S[lu, lg]))
        _assert_list_stats(stats, np.diff(ip)[rows], 1)


def test_cosine_lists_are_rank_items_on_the_expanded_pairs():
    """head=None: no new kernel — rank_items' ranks, values and stats for list_pairs."""
    from gnnrec import recs
    hu, hi = rc.tables("relu", 64)
    _, _, _, _, excl, us, gs, _, _ = _case("relu", 64)
    ip, ix = rl.grouped(us, gs, hi.shape[0])
    ex = (_cu(excl[0]), _cu(excl[1]))
    rows = _cu(np.arange(rc.N_USERS)[::-1].copy())
    for ur in (None, rows):
        a = recs.rank_lists(_cu(hu), _cu(hi), ur, _cu(ip), _cu(ix), ex, return_stats=True)
        pu, pg = recs.list_pairs(ur, _cu(ip), _cu(ix))
        b = recs.rank_items(_cu(hu), _cu(hi), pu, pg, ex, return_stats=True)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and a[2] == b[2]
        assert set(a[2]) == STATS_KEYS and a[2]["eps"] == rk.eps(64)
    with pytest.raises(NotImplementedError, match="needs head="):
        recs.rank_lists(_cu(hu), _cu(hi), None, _cu(ip), _cu(ix),
                        popularity=torch.zeros(hi.shape[0], device="cuda"))


# ---------------------------------------------------------------- 4. + 5. the rating form
@pytest.mark.parametrize("weight", rm.POP_WEIGHTS)
def test_popularity_lists_are_the_definition_on_ratings(weight):
    from gnnrec import recs
    hu, hi, pl, pop, R, excl, us, gs, n_tied = _pop_case(weight)
    assert n_tied >= rc.N_USERS                          # at least half the rows hold an exact tie
    lists = rl.regroup(us, gs)
    lists[rl.LONG_USER] = (lists[rl.LONG_USER] * 25)[:rl.LONG]     # a list of several rows
    ip, ix = rc.csr(lists)
    lu, lg = rl.list_pairs(None, ip, ix)
    kw = dict(popularity=_cu(pop), weight_popularity=weight)
    for ex in (excl, None):
        ipx, ixx = ex if ex is not None else (None, None)
        want = rk.ranks(R, lu, lg, ipx, ixx)
        for bs in (8192, 50):
            rank, vals, stats = _rank_lists(pl, hu, hi, ip, ix, None, ex, batch_size=bs, **kw)
            np.testing.assert_array_equal(rank, want)
            np.testing.assert_array_equal(_bits(vals), _bits(R[lu, lg]))
            _assert_list_stats(stats, np.diff(ip))
        r2, v2, s2, _, _ = _rank_items_on_list_pairs(pl, hu, hi, ip, ix, None, ex, **kw)
        np.testing.assert_array_equal(rank, r2)
        np.testing.assert_array_equal(_bits(vals), _bits(v2))
        assert {k: stats[k] for k in STATS_KEYS} == s2
    # a column popularity is the flat one
    b = recs.rank_lists(_cu(hu), _cu(hi), None, _cu(ip), _cu(ix), (_cu(excl[0]), _cu(excl[1])),
                        head=pl, popularity=_cu(pop.reshape(-1, 1)), weight_popularity=weight)
    rank, vals, _ = _rank_lists(pl, hu, hi, ip, ix, None, excl, **kw)
    np.testing.assert_array_equal(b[0].cpu().numpy(), rank)
    np.testing.assert_array_equal(_bits(b[1].cpu().numpy()), _bits(vals))
    # recommend(head=, popularity=)'s values for the same users, where an item is in both
    k = 10
    idx, rv = recs.recommend(_cu(hu), _cu(hi), k, None, (_cu(excl[0]), _cu(excl[1])),
                             sample=rc.SAMPLE, cand_cap=2048, head=pl, **kw)
    idx, rv = idx.cpu().numpy(), rv.cpu().numpy()
    pos = {(u, int(g)): j for u in range(rc.N_USERS) for j, g in enumerate(idx[u])}
    hit = [(e, pos[(u, g)]) for e, (u, g) in enumerate(zip(lu.tolist(), lg.tolist()))
           if (u, g) in pos]
    assert len(hit) >= 5 * rc.N_USERS                    # rank_cases' five list positions a user
    for e, j in hit:
        assert _bits(vals[e:e + 1])[0] == _bits(rv[lu[e], j:j + 1])[0] and rank[e] == j + 1


# ---------------------------------------------------------------- 6. the graph entry
def test_rank_lists_for_graph_agrees_with_rank_for_graph():
    """A multigraph, ground-truth pairs with repeated users, repeated pairs and users without
    any: the pairs come back permuted, each with rank_for_graph's rank and value."""
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
    h = {"user": _cu(hu), "item": _cu(hi)}
    pl = _head(16)
    gu, gi = rng.integers(0, n_u - 5, 300), rng.integers(0, n_i, 300)     # users 55.. have none
    gu[:40] = 11                                                          # a list of three rows
    gu[-3:], gi[-3:] = gu[0], gi[0]                                       # a repeated pair
    pop = (rng.integers(0, 4, (n_i, 1)) / 4).astype(np.float32)
    g.nodes["item"].data["popularity"] = _cu(pop)
    for kw in (dict(), dict(use_popularity=True, weight_popularity=0.25)):
        rank, vals, us, gs, stats = recs.rank_lists_for_graph(g, h, (gu, gi), head=pl,
                                                              return_stats=True, **kw)
        assert len(recs.rank_lists_for_graph(g, h, (gu, gi), head=pl, **kw)) == 4
        r0, v0 = recs.rank_for_graph(g, h, (gu, gi), head=pl, **kw)
        key = lambda a, b: np.lexsort((np.asarray(b), np.asarray(a)))     # noqa: E731
        a, b = key(us.cpu().numpy(), gs.cpu().numpy()), key(gu, gi)
        np.testing.assert_array_equal(us.cpu().numpy()[a], gu[b])         # a permutation
        np.testing.assert_array_equal(gs.cpu().numpy()[a], gi[b])
        np.testing.assert_array_equal(rank.cpu().numpy()[a], r0.cpu().numpy()[b])
        np.testing.assert_array_equal(_bits(vals.cpu().numpy()[a]), _bits(v0.cpu().numpy()[b]))
        assert (rank == 0).any() and (rank > 0).any()
        assert stats["pairs"] == 300 and stats["rows"] < 60 + 3
        # the returned pairs feed ranks_to_metrics; rank_for_graph on them in that order
        # (sums taken in one order) gives the same dict
        r1, _ = recs.rank_for_graph(g, h, (us, gs), head=pl, **kw)
        m = recs.ranks_to_metrics(rank, us, rk.KS)
        assert m == recs.ranks_to_metrics(r1, us, rk.KS) and m["unranked"] == int((r0 == 0).sum())
    with pytest.raises(NotImplementedError, match="needs head="):
        recs.rank_lists_for_graph(g, h, (gu, gi), use_popularity=True)
    with pytest.raises(ValueError, match="out of range"):
        recs.rank_lists_for_graph(g, h, (gu, gi + n_i), head=pl)


# ---------------------------------------------------------------- 7. errors, empty sets
def test_bad_ids_and_empty_sets():
    from gnnrec import recs
    hu, hi = rc.tables("normal", 16, 8, 20)
    pl = _head(16)
    ip, ix = rc.csr([[1, 2], [], [19, 0, 19], [], [], [5], [], [20]])     # user 7 lists item 20
    H = (_cu(hu), _cu(hi))
    ok = _cu(np.array([2, 0, 5, 1], np.int64))
    for head in (pl, None):
        rank, vals = recs.rank_lists(*H, ok, _cu(ip), _cu(ix), head=head)
        assert tuple(rank.shape) == (6,) and (rank > 0).all()
        with pytest.raises(ValueError, match="out of range"):
            recs.rank_lists(*H, None, _cu(ip), _cu(ix), head=head)        # a served list's item
        with pytest.raises(ValueError, match="out of range"):
            recs.rank_lists(*H, _cu(np.array([2, 8], np.int64)), _cu(ip), _cu(ix), head=head)
        with pytest.raises(ValueError, match="out of range"):
            recs.rank_lists(*H, _cu(np.array([-1, 2], np.int64)), _cu(ip), _cu(ix), head=head)
        with pytest.raises(ValueError, match="repeated user"):
            recs.rank_lists(*H, _cu(np.array([2, 0, 2], np.int64)), _cu(ip), _cu(ix), head=head)
        neg = ix.copy()
        neg[2] = -1                                                       # user 2's first entry
        with pytest.raises(ValueError, match="out of range"):
            recs.rank_lists(*H, ok, _cu(ip), _cu(neg), head=head)
        # nothing to rank: no users, or users whose lists are empty
        for rows in (ok[:0], _cu(np.array([1, 3, 6], np.int64))):
            rank, vals, stats = recs.rank_lists(*H, rows, _cu(ip), _cu(ix), head=head,
                                                return_stats=True)
            assert tuple(rank.shape) == (0,) and tuple(vals.shape) == (0,)
            assert rank.dtype == torch.int64 and vals.dtype == torch.float32
            assert set(stats) == (LIST_STATS_KEYS if head is not None else STATS_KEYS)
    with pytest.raises(ValueError, match="hidden_1 must be"):
        recs.rank_lists(*H, ok, _cu(ip), _cu(ix), head=_head(64))
    a = recs.rank_lists(*H, ok, _cu(ip), _cu(ix.astype(np.int64)), head=pl)   # int64 lists
    b = recs.rank_lists(*H, ok, _cu(ip), _cu(ix), head=pl)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
