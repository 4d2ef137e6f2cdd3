"""Cached top-k lists kept current after a refresh, on the device:
gnnrec.recs.update_recommendations (the bf16 filter over the dirty items, gnnrec_topk_update_f32,
the re-rank of what it hands back) and recs.LiveRecommendations over an
IncrementalEmbeddings.  The reference in every test is recs.recommend on the refreshed tables
(in one small case the definition itself: ops.sddmm_cos over all pairs + topk_rows), and
every comparison is torch.equal on both idx and vals.  The shapes are 300 users x 700 items
(three 128-row tiles, the last partial; six item tiles) with batch_size = 128, so every call
runs several batches."""
import functools

import numpy as np
import pytest
import torch

import live_recs_cases as lc
import recommend_cases as rc
from incremental_cases import (BUYS, COLD_I, COLD_U, HostTwin, cold_batch, dirty_sets,
                               reverse_of, route_graph)

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
NU, NI = lc.N_USERS, lc.N_ITEMS
NONE = np.empty(0, np.int64)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def entry(n, ids):
    """A final_dirty entry: (marks int32 [n], ascending int64 ids)."""
    return dev(lc.marks(n, ids)), dev(np.asarray(ids, np.int64))


def excl_dev(excl):
    return dev(excl[0]), dev(excl[1])


@functools.lru_cache(maxsize=None)
def old_lists(d, k):
    """recommend() on the shared tables of width d before any change: computed once per
    (d, k), cloned by every test that updates them."""
    from gnnrec import recs
    hu, hi = lc.tables(d)
    return recs.recommend(dev(hu), dev(hi), k, None, excl_dev(lc.exclusions()))


def update(hu1, hi1, excl, k, du, di, idx, vals, n_users=NU, n_items=NI, check=True, **kw):
    """update_recommendations on clones of (idx, vals), compared with recommend on the
    refreshed tables -> (stats, idx, vals)."""
    from gnnrec import recs
    idx, vals = idx.clone(), vals.clone()
    hu1, hi1, ex = dev(hu1), dev(hi1), excl_dev(excl)
    kw.setdefault("batch_size", 128)
    stats = recs.update_recommendations(
        idx, vals, hu1, hi1, None if du is None else entry(n_users, du),
        None if di is None else entry(n_items, di), ex, return_stats=True, **kw)
    if check:
        want_i, want_v = recs.recommend(hu1, hi1, k, None, ex)
        assert torch.equal(idx, want_i), stats
        assert torch.equal(vals, want_v), stats
    return stats, idx, vals


# ---------------------------------------------------------------- 1. widths and lengths
@pytest.mark.parametrize("d,k,n_di,n_du", lc.GRID)
def test_small_perturbation_equals_recommend(d, k, n_di, n_du):
    """Every grid case equals recommend, and the merge really settles what the rule can
    settle: redo_rows is at most the unsettled count of the numpy restatement (lc.rule) on the
    same tables plus the rows that restatement calls undecided between fp32 and float64 scores
    (lc.DECIDE_TOL) — so a merge that hands rows back without need fails at every k and width.
    Where the restatement stays at 5 % of the clean rows or under (tests/test_live_recs_cpu.py
    asserts that for the small perturbation: 5 % of the items or fewer, k <= 10) the device is
    also held to 10 %.  With 129 of 700 items dirty, or k = 64 and 35 dirty, the rule itself
    leaves 8 - 22 %, so 10 % cannot hold there; the restatement's own count does."""
    c = lc.grid_case(d, k, n_di, n_du)
    i0, v0 = old_lists(d, k)
    stats, _i, _v = update(c["hu1"], c["hi1"], c["excl"], k, c["du"], c["di"], i0, v0)
    n_clean = NU - n_du
    assert not stats["full"] and stats["overflow_rows"] == 0
    assert (stats["clean_rows"], stats["dirty_users"], stats["dirty_items"]) == (n_clean, n_du, n_di)
    s0 = rc.cosine64(c["hu0"], c["hi0"])
    s1 = lc.refreshed_scores(s0, c["hu1"], c["hi1"], c["du"], c["di"])
    _ri, _rv, settled, _kept, undecided = lc.rule(s0, s1, lc.approx(c["hu1"], c["hi1"]),
                                                  c["excl"], k, c["du"], c["di"])
    unsettled = n_clean - int(settled.sum())
    print(f"d {d} k {k}: redo {stats['redo_rows']} of {n_clean} clean rows, restated "
          f"{unsettled} (+{int(undecided.sum())} undecided), candidates_max "
          f"{stats['candidates_max']}")
    assert stats["redo_rows"] <= unsettled + int(undecided.sum()), stats
    if unsettled <= lc.UNSETTLED_CPU * n_clean:
        assert stats["redo_rows"] <= lc.UNSETTLED_GPU * n_clean, stats
    if n_di <= lc.SMALL and k <= 10:     # the issue's small perturbation: always capped
        assert stats["redo_rows"] <= lc.UNSETTLED_GPU * n_clean, stats


def test_marks_are_dirty_where_non_zero():
    """Marks of 7 instead of 1 (a row is dirty where its mark is non-zero) give the same
    lists and the same statistics."""
    from gnnrec import recs
    d, k = 128, 10
    c = lc.grid_case(d, k, 35, 40)
    want, _i, _v = update(c["hu1"], c["hi1"], c["excl"], k, c["du"], c["di"], *old_lists(d, k))
    idx, vals = (t.clone() for t in old_lists(d, k))
    hu1, hi1, ex = dev(c["hu1"]), dev(c["hi1"]), excl_dev(c["excl"])
    (um, ui), (im, ii) = entry(NU, c["du"]), entry(NI, c["di"])
    stats = recs.update_recommendations(idx, vals, hu1, hi1, (um * 7, ui), (im * 7, ii), ex,
                                        batch_size=128, return_stats=True)
    assert stats == want and want["redo_rows"] > 0
    assert torch.equal(idx, _i) and torch.equal(vals, _v)


def test_equals_the_definition():
    """The same against the definition itself: ops.sddmm_cos over all pairs, topk_rows."""
    from gnnrec import ops, recs
    d, k = 64, 10
    c = lc.grid_case(d, k, 35, 1)
    _stats, idx, vals = update(c["hu1"], c["hi1"], c["excl"], k, c["du"], c["di"],
                               *old_lists(d, k), check=False)
    hu1, hi1 = dev(c["hu1"]), dev(c["hi1"])
    src = torch.arange(NU, device=DEV).repeat_interleave(NI)
    dst = torch.arange(NI, device=DEV).repeat(NU)
    sc = ops.sddmm_cos(src, dst, hu1, hi1).view(NU, NI)
    want_v, want_i = recs.topk_rows(sc, k, dev(c["excl"][0]), dev(c["excl"][1].astype(np.int64)))
    assert torch.equal(idx, want_i) and torch.equal(vals, want_v)


# ---------------------------------------------------------------- 2. - 5. single items
def _free_item(u, excl, taken):
    """An item that is neither excluded for user u nor in `taken`."""
    ex = set(excl[1][excl[0][u]:excl[0][u + 1]].tolist()) | set(int(t) for t in taken)
    return next(v for v in range(NI - 1, -1, -1) if v not in ex)


def test_an_item_that_enters():
    """A dirty item's new row is a bit-copy of a clean user's row: it enters at rank 0."""
    d, k, u = 128, 10, 130
    hu, hi = lc.tables(d)
    excl = lc.exclusions()
    i0, v0 = old_lists(d, k)
    v = _free_item(u, excl, i0[u].tolist())
    hi1 = hi.copy()
    hi1[v] = hu[u]
    _stats, idx, _vals = update(hu, hi1, excl, k, NONE, [v], i0, v0)
    assert idx[u, 0].item() == v


def test_an_item_that_leaves():
    """A dirty item of a clean user's list gets the negated user row: the merged set holds
    k - 1 entries, the row must come back through redo."""
    d, k, u = 128, 10, 7
    hu, hi = lc.tables(d)
    i0, v0 = old_lists(d, k)
    v = i0[u, 3].item()
    hi1 = hi.copy()
    hi1[v] = -hu[u]
    stats, idx, _vals = update(hu, hi1, lc.exclusions(), k, NONE, [v], i0, v0)
    assert stats["redo_rows"] >= 1
    assert v not in idx[u].tolist()


def test_unchanged_bits_leave_the_lists_alone():
    """Dirty rows times 2 (exact in fp32) normalise to the same bits: no list changes, no row
    is handed back, and a row with no dirty entry and no candidate is not written at all —
    a sentinel in its vals survives."""
    d, k = 64, 10
    hu, hi = lc.tables(d)
    excl = lc.exclusions()
    di = lc.pick(NI, 35, 3)
    hi1 = hi.copy()
    hi1[di] *= 2
    i0, v0 = old_lists(d, k)
    # a row the kernel must leave: no dirty entry, and every dirty item's approximate score
    # below the threshold by more than the band of the filter's own rounding
    a = lc.approx(hu, hi1[di]).astype(np.float64)
    thr = v0[:, k - 1].cpu().numpy().astype(np.float64) - 2 * lc.EPS
    quiet = (a.max(1) < thr - rc.FILTER_BAND) & ~np.isin(i0.cpu().numpy(), di).any(1)
    assert quiet.any() and not quiet.all()
    u = int(np.nonzero(quiet)[0][0])
    v0 = v0.clone()
    v0[u, 0] = 12345.0
    stats, idx, vals = update(hu, hi1, excl, k, NONE, di, i0, v0, check=False)
    assert stats["redo_rows"] == 0 and not stats["full"]
    assert torch.equal(idx, i0) and torch.equal(vals, v0)
    assert vals[u, 0].item() == 12345.0


def _tie_setup(d, k):
    hu, hi = lc.tables(d)
    excl = lc.exclusions()
    i0, v0 = old_lists(d, k)
    last = i0[:, k - 1].cpu().numpy()
    u = int(np.nonzero((last > 50) & (last < NI - 50))[0][0])
    return hu, hi, excl, i0, v0, u, int(last[u])


@pytest.mark.parametrize("above", [True, False])
def test_a_tie_with_the_last_entry(above):
    """A dirty item becomes a bit-copy of user u's last list entry: the same score bits.  With
    a higher id it stays out; with a lower id it takes the entry's place."""
    d, k = 128, 10
    hu, hi, excl, i0, v0, u, last = _tie_setup(d, k)
    ex = set(excl[1][excl[0][u]:excl[0][u + 1]].tolist()) | set(i0[u].tolist())
    ids = range(last + 1, NI) if above else range(last - 1, -1, -1)
    v = next(x for x in ids if x not in ex)
    hi1 = hi.copy()
    hi1[v] = hi[last]
    _stats, idx, vals = update(hu, hi1, excl, k, NONE, [v], i0, v0)
    if above:
        assert torch.equal(idx[u], i0[u]) and torch.equal(vals[u], v0[u])
    else:
        assert idx[u, k - 1].item() == v and vals[u, k - 1].item() == v0[u, k - 1].item()
        assert torch.equal(idx[u, :k - 1], i0[u, :k - 1])


def test_two_dirty_copies_rank_in_id_order():
    d, k, u = 64, 5, 200
    hu, hi = lc.tables(d)
    excl = lc.exclusions()
    i0, v0 = old_lists(d, k)
    v2 = _free_item(u, excl, i0[u].tolist())
    v1 = _free_item(u, excl, i0[u].tolist() + [v2])
    assert v1 < v2
    hi1 = hi.copy()
    hi1[v1] = hi1[v2] = hu[u]
    _stats, idx, vals = update(hu, hi1, excl, k, NONE, [v1, v2], i0, v0)
    assert idx[u, :2].tolist() == [v1, v2] and vals[u, 0].item() == vals[u, 1].item()


# ---------------------------------------------------------------- 6. padded lists
def test_padded_lists():
    """12 items, k = 10, users with 0, 3 and 11 excluded items: lists of 10, 9 and 1 entries.
    Dirty items leave and re-enter the padded lists (tau = -inf keeps every dirty item)."""
    from gnnrec import recs
    d, k, n_u, n_i = 64, 10, 9, 12
    hu, hi = lc.tables(d, n_u, n_i)
    rng = np.random.default_rng(4)
    excl = rc.csr([rng.permutation(n_i)[:(0, 3, 11)[u % 3]] for u in range(n_u)])
    ex = excl_dev(excl)
    i0, v0 = recs.recommend(dev(hu), dev(hi), k, None, ex)
    assert sorted(set((i0 >= 0).sum(1).tolist())) == [1, 9, 10]
    for di in ([5], [0, 3, 4, 8, 11], list(range(n_i))):
        hi1 = hi.copy()
        hi1[di] = rng.standard_normal((len(di), d)).astype(np.float32)
        stats, _i, _v = update(hu, hi1, excl, k, NONE, di, i0, v0, n_u, n_i, max_dirty_frac=1.0)
        assert not stats["full"]
    # a dirty user beside them, and the items of one padded list all dirty
    hi1 = hi.copy()
    hi1[[1, 2]] *= -1
    hu1 = hu.copy()
    hu1[4] = rng.standard_normal(d).astype(np.float32)
    update(hu1, hi1, excl, k, [4], [1, 2], i0, v0, n_u, n_i)


# ---------------------------------------------------------------- 7. exclusion
def test_an_excluded_dirty_item_stays_out():
    """A dirty item that would rank first for user u but sits in u's exclusion row — 5,000
    entries (no staging buffer holds them), unsorted, with duplicates and ids outside
    [0, n_items), the item near the end — must not appear; for another user it ranks first."""
    d, k, u, w = 128, 10, 150, 151
    hu, hi = lc.tables(d)
    indptr, indices = lc.exclusions()
    i0, v0 = old_lists(d, k)
    v = _free_item(u, (indptr, indices), i0[u].tolist() + i0[w].tolist() +
                   indices[indptr[w]:indptr[w + 1]].tolist())
    rng = np.random.default_rng(6)
    own = indices[indptr[u]:indptr[u + 1]]
    noise = np.concatenate([rng.choice(own, 4000), np.full(500, -3), np.full(200, NI),
                            np.full(299 - own.size, 1 << 30), own]).astype(np.int32)
    row = np.concatenate([rng.permutation(noise)[:4900], [v], rng.permutation(noise)[:99]])
    assert row.size == 5000 and set(own.tolist()) <= set(row.tolist())
    lists = [indices[indptr[r]:indptr[r + 1]] if r != u else row for r in range(NU)]
    excl = rc.csr(lists)
    hi1 = hi.copy()
    hi1[v] = hu[u]
    hu1 = hu.copy()
    hu1[w] = hu[u]            # user w (dirty) has u's row: the item ranks first there
    _stats, idx, _vals = update(hu1, hi1, excl, k, [w], [v], i0, v0)
    assert v not in idx[u].tolist() and idx[w, 0].item() == v
    assert torch.equal(idx[u], i0[u])
    # a clean user with the same long row and the item NOT in it: it enters
    row2 = np.where(row == v, -3, row).astype(np.int32)
    excl2 = rc.csr([lists[r] if r != u else row2 for r in range(NU)])
    _stats, idx, _vals = update(hu, hi1, excl2, k, NONE, [v], i0, v0)
    assert idx[u, 0].item() == v


# ---------------------------------------------------------------- 8. the slot boundary
@pytest.mark.parametrize("over", [0, 1])
def test_the_slot_boundary(over):
    """cap = 256 - k dirty items, all bit-copies of user u's best item, fill u's slots exactly
    and the merge settles the row; one more and the row goes to redo.  Every other user is
    passed as dirty, so redo_rows speaks of u alone."""
    from gnnrec import ops
    d, k, u = 64, 10, 33
    cap = ops.UPDATE_SLOTS - k
    hu, hi = lc.tables(d)
    excl = lc.exclusions()
    i0, v0 = old_lists(d, k)
    best = i0[u, 0].item()
    ex = set(excl[1][excl[0][u]:excl[0][u + 1]].tolist()) | set(i0[u].tolist())
    di = np.asarray([x for x in range(NI) if x not in ex][:cap + over], np.int64)
    hi1 = hi.copy()
    hi1[di] = hi[best]
    others = np.setdiff1d(np.arange(NU), [u])
    stats, idx, _vals = update(hu, hi1, excl, k, others, di, i0, v0, max_dirty_frac=1.0)
    assert stats["clean_rows"] == 1 and stats["candidates_max"] == cap + over
    assert stats["redo_rows"] == over and stats["overflow_rows"] == over
    assert idx[u].tolist() == sorted([best] + di.tolist())[:k]


# ---------------------------------------------------------------- 9. fallbacks
@pytest.mark.parametrize("case", ["items None", "users None", "share", "d6", "k65"])
def test_fallbacks_take_the_full_path(case):
    from gnnrec import recs
    d, k = (6, 10) if case == "d6" else (64, 65) if case == "k65" else (64, 10)
    hu, hi = lc.tables(d)
    excl = lc.exclusions()
    i0, v0 = recs.recommend(dev(hu), dev(hi), k, None, excl_dev(excl))
    di, du = lc.pick(NI, 35, 1), lc.pick(NU, 3, 2)
    hi1, hu1 = lc.perturbed(hi, di, 1), lc.perturbed(hu, du, 2)
    kw = {}
    if case == "items None":     # every item row may differ
        di, hi1 = None, lc.perturbed(hi, np.arange(NI), 3)
    elif case == "users None":
        du, hu1 = None, lc.perturbed(hu, np.arange(NU), 4)
    elif case == "share":
        kw["max_dirty_frac"] = 34 / NI
    stats, _i, _v = update(hu1, hi1, excl, k, du, di, i0, v0, **kw)
    assert stats["full"]
    if case == "share":          # and at the threshold itself the merge runs
        stats, _i, _v = update(hu1, hi1, excl, k, du, di, i0, v0, max_dirty_frac=35 / NI)
        assert not stats["full"]


def test_nothing_dirty_changes_nothing():
    d, k = 64, 10
    hu, hi = lc.tables(d)
    i0, v0 = old_lists(d, k)
    v0 = v0.clone()
    v0[5, 2] = 12345.0     # nothing is launched: nothing rewrites it
    stats, idx, vals = update(hu, hi, lc.exclusions(), k, NONE, NONE, i0, v0, check=False)
    assert torch.equal(idx, i0) and torch.equal(vals, v0)
    assert not stats["full"] and stats["redo_rows"] == 0 and stats["clean_rows"] == NU


def test_refusals():
    from gnnrec import recs
    d, k = 64, 10
    hu, hi = lc.tables(d)
    i0, v0 = old_lists(d, k)
    hu, hi = dev(hu), dev(hi)
    with pytest.raises(ValueError, match="refused"):
        recs.update_recommendations(i0.clone(), v0.clone(), hu, hi, None, None,
                                    popularity=torch.ones(NI, device=DEV))
    with pytest.raises(ValueError, match="marks must have"):
        recs.update_recommendations(i0.clone(), v0.clone(), hu, hi, entry(NU + 1, NONE),
                                    entry(NI, NONE))
    with pytest.raises(ValueError, match="idx / vals"):
        recs.update_recommendations(i0[:10].clone(), v0[:10].clone(), hu, hi, None, None)


# ---------------------------------------------------------------- 10. - 11. end to end
def _graph(num_nodes, edges, feats):
    from gnnrec.graph import HeteroGraph
    g = HeteroGraph({ce: (dev(s), dev(d)) for ce, (s, d) in edges.items()}, dict(num_nodes),
                    device=DEV)
    g.ndata["features"] = {nt: dev(f) for nt, f in feats.items()}
    return g


class Rig:
    """route_graph("a_valu") under IncrementalEmbeddings and LiveRecommendations, with its
    host twin; check() compares the live lists with recommend_for_graph over a freshly built
    graph and a fresh full pass."""
    K = 10

    def __init__(self):
        from gnnrec import nn as gnn
        from gnnrec import recs
        from gnnrec.inference import IncrementalEmbeddings
        c = route_graph("a_valu")
        d = c["d"]
        self.tw = HostTwin(c["num_nodes"], c["edges"], c["feats"])
        self.g = _graph(c["num_nodes"], c["edges"], c["feats"])
        torch.manual_seed(11)
        self.model = gnn.ConvModel(self.g, 3, {"user": d, "item": d, "hidden": d, "out": d}, True,
                                   0.0, c["agg"], "cos", c["hetero"], True).to(DEV).eval()
        self.rng = np.random.default_rng(5)
        with torch.no_grad():
            self.inc = IncrementalEmbeddings(self.g, self.model, max_dirty_frac=1.0)
        self.live = recs.LiveRecommendations(self.inc, self.K, batch_size=512)

    def add_pairs(self, u, i):
        for ce, (s, t) in ((BUYS, (u, i)), (reverse_of(BUYS), (i, u))):
            self.inc.add_edges(dev(s), dev(t), etype=ce)
            self.tw.add_edges(ce, s, t)

    def remove_cold(self, n):
        lim = {"user": COLD_U, "item": COLD_I}
        for ce in self.tw.edges:
            s, t = self.tw.edges[ce]
            cold = np.nonzero((s < lim[ce[0]]) & (t < lim[ce[2]]))[0]
            e = cold[self.rng.permutation(cold.size)[:n]]
            self.inc.remove_edges(dev(e), etype=ce)
            self.tw.remove_edges(ce, e)

    def add_nodes(self):
        d = self.tw.feats["user"].shape[1]
        n_u, n_i = self.tw.num_nodes["user"], self.tw.num_nodes["item"]
        fu = self.rng.standard_normal((3, d)).astype(np.float32)
        fi = self.rng.standard_normal((2, d)).astype(np.float32)
        self.inc.add_nodes(3, {"features": dev(fu)}, ntype="user")
        self.inc.add_nodes(2, {"features": dev(fi)}, ntype="item")
        self.tw.add_nodes("user", fu)
        self.tw.add_nodes("item", fi)
        self.add_pairs(np.asarray([n_u, n_u + 1, n_u + 2, n_u], np.int64),
                       np.asarray([0, 1, 2, 2], np.int64))
        self.add_pairs(np.asarray([4, 9, 9], np.int64), np.asarray([n_i, n_i + 1, n_i], np.int64))

    def set_features(self):
        d = self.tw.feats["item"].shape[1]
        ids = np.asarray([2, 7, 11], np.int64)
        rows = self.rng.standard_normal((3, d)).astype(np.float32)
        self.inc.set_features("item", dev(ids), dev(rows))
        self.tw.set_features("item", ids, rows)

    def want(self):
        from gnnrec import recs
        from gnnrec.inference import full_graph_embeddings
        with torch.no_grad():
            fresh = _graph(self.tw.num_nodes, self.tw.edges, self.tw.feats)
            h = full_graph_embeddings(fresh, self.model)
        return recs.recommend_for_graph(fresh, h, self.K)

    def check(self, what, refresh=True):
        S, E = self.tw.take()
        D = dirty_sets(self.tw.num_nodes, self.tw.edges, S, E, 2)
        out = None
        if refresh:
            with torch.no_grad():
                out = self.live.refresh()
        want_i, want_v = self.want()
        assert torch.equal(self.live.idx, want_i), (what, out)
        assert torch.equal(self.live.vals, want_v), (what, out)
        return out, D


def test_live_recommendations_end_to_end():
    r = Rig()
    r.check("creation", refresh=False)
    held = r.live.idx
    gen = r.inc.generation
    for n in (1, 33):
        r.add_pairs(*cold_batch(r.rng, n, r.tw.num_nodes))
        (rs, us), D = r.check(f"add {n}")
        assert not us["full"] and not rs.whole_pass
        # 11. final_dirty is the restated D_L on the row path
        for nt in ("user", "item"):
            mark, ids = rs.final_dirty[nt]
            assert np.array_equal(ids.cpu().numpy(), D[2][nt]), (n, nt)
            assert np.array_equal(mark.cpu().numpy(), lc.marks(r.tw.num_nodes[nt], D[2][nt]))
        assert (us["dirty_users"], us["dirty_items"]) == (D[2]["user"].size, D[2]["item"].size)
        assert us["clean_rows"] == r.tw.num_nodes["user"] - D[2]["user"].size
    assert r.inc.generation == gen + 2
    r.remove_cold(20)
    (rs, us), _D = r.check("remove")
    assert not us["full"]
    assert r.live.idx is held                       # updated in place all along
    r.add_nodes()
    (rs, us), D = r.check("new nodes")
    assert not us["full"] and r.live.idx is not held
    assert r.live.idx.shape[0] == r.tw.num_nodes["user"]
    held = r.live.idx
    r.set_features()
    (rs, us), D = r.check("features")
    assert not us["full"] and r.live.idx is held
    # nothing recorded: nothing runs, final_dirty is empty
    rs, us = r.live.refresh()
    assert rs.final_dirty == {} and not us["full"] and us["dirty_items"] == 0
    assert r.inc.generation == gen + 5
    # a refresh behind the object's back: the next one re-ranks everyone
    r.add_pairs(*cold_batch(r.rng, 5, r.tw.num_nodes))
    with torch.no_grad():
        r.inc.refresh()
    r.add_pairs(*cold_batch(r.rng, 2, r.tw.num_nodes))
    (rs, us), _D = r.check("skipped update")
    assert us["full"] and r.live.idx is held
    # a weight edit runs the whole pass: every row of both types
    with torch.no_grad():
        r.model.layers[0].mods["buys"].fc_self.weight.mul_(1.01)
    (rs, us), _D = r.check("weight edit")
    assert rs.whole_pass and rs.final_dirty == {"user": None, "item": None} and us["full"]


def test_live_recommendations_refuse_other_heads():
    from gnnrec import recs
    with pytest.raises(ValueError, match="refused"):
        recs.LiveRecommendations(object(), 10, use_popularity=True)
    with pytest.raises(ValueError, match="refused"):
        recs.LiveRecommendations(object(), 10, head=object())
