"""Incremental embedding refresh on the device: csrc/frontier.hip against the
numpy restatement of the frontier, gnnrec_scatter_rows against index_copy_, and
gnnrec.inference.IncrementalEmbeddings against a fresh full pass over a freshly built graph
— every layer's table, torch.equal — on one graph per kernel route, under added and removed
batches, new nodes, a feature change and several refreshes in a row.  The restated dirty
sets (tests/incremental_cases.py) say how many rows each refresh may touch: the statistics
must equal them with no whole-layer flag, so a fallback cannot make these tests pass."""
import numpy as np
import pytest
import torch

from incremental_cases import (BOUGHT, BUYS, CLICKS, COLD_I, COLD_U, HostTwin, ROUTES, cold_batch,
                               dirty_sets, reverse_of, route_graph)

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
TILE = 512  # slots per wave-tile of the mark kernel (frontier.hip kFTile)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ---- frontier_mark --------------------------------------------------------------------
N_SRC, N_DST = 1500, 1700
DEGREES = {
    "one edge per row": lambda rng: np.ones(N_SRC, np.int64),              # total = rows listed
    "seven": lambda rng: np.full(N_SRC, 7, np.int64),                      # several tiles
    "mixed with empty rows": lambda rng: rng.integers(0, 21, N_SRC) * (rng.random(N_SRC) < .6),
    "every row empty": lambda rng: np.zeros(N_SRC, np.int64),
}


def _csr(deg, rng):
    indptr = np.zeros(deg.size + 1, np.int64)
    np.cumsum(deg, out=indptr[1:])
    return indptr, rng.integers(0, N_DST, int(indptr[-1])).astype(np.int32)


def _want(indptr, indices, rows, mark0):
    want = mark0.copy()
    for r in rows:
        want[indices[indptr[r]:indptr[r + 1]]] = 1
    return want


@pytest.mark.parametrize("n_rows", [0, 1, 63, 64, 65, 513])
def test_frontier_mark_equals_the_restatement(n_rows):
    from gnnrec import ops
    rng = np.random.default_rng(n_rows)
    for name, make in DEGREES.items():
        indptr, indices = _csr(np.asarray(make(rng), np.int64), rng)
        rows = np.sort(rng.permutation(N_SRC)[:n_rows]).astype(np.int64)
        mark0 = (rng.random(N_DST) < 0.05).astype(np.int32)  # marks already set are kept
        mark = dev(mark0)
        ops.frontier_mark(dev(rows), dev(indptr), dev(indices), mark)
        assert torch.equal(mark.cpu(), torch.from_numpy(_want(indptr, indices, rows, mark0))), name
        if n_rows > 1:  # a device count below the list's length: only that prefix counts
            mark = dev(mark0)
            ops.frontier_mark(dev(rows), dev(indptr), dev(indices), mark,
                              n_rows=torch.tensor([n_rows - 1], device=DEV))
            assert torch.equal(mark.cpu(),
                               torch.from_numpy(_want(indptr, indices, rows[:-1], mark0))), name


@pytest.mark.parametrize("total", [TILE - 1, TILE, TILE + 1, 3 * TILE + 5])
def test_frontier_mark_at_the_tile_boundaries(total):
    """The listed ranges add up to `total` slots: a last tile that is short, exact, one over."""
    from gnnrec import ops
    rng = np.random.default_rng(total)
    deg = np.zeros(N_SRC, np.int64)
    rows = np.sort(rng.permutation(N_SRC)[:40]).astype(np.int64)
    deg[rows] = total // 40
    deg[rows[:total % 40]] += 1
    deg[np.setdiff1d(np.arange(N_SRC), rows)] = rng.integers(0, 9, N_SRC - 40)  # not listed
    assert deg[rows].sum() == total
    indptr, indices = _csr(deg, rng)
    mark = torch.zeros(N_DST, dtype=torch.int32, device=DEV)
    ops.frontier_mark(dev(rows), dev(indptr), dev(indices), mark)
    want = _want(indptr, indices, rows, np.zeros(N_DST, np.int32))
    assert torch.equal(mark.cpu(), torch.from_numpy(want))


def test_frontier_mark_one_heavy_row_among_empty_rows():
    from gnnrec import ops
    rng = np.random.default_rng(7)
    deg = np.zeros(N_SRC, np.int64)
    deg[700] = 5000
    indptr = np.zeros(N_SRC + 1, np.int64)
    np.cumsum(deg, out=indptr[1:])
    indices = rng.integers(0, 6000, 5000).astype(np.int32)
    rows = np.asarray([3, 699, 700, 701, 1499], np.int64)
    mark = torch.zeros(6000, dtype=torch.int32, device=DEV)
    ops.frontier_mark(dev(rows), dev(indptr), dev(indices), mark)
    want = np.zeros(6000, np.int32)
    want[indices] = 1
    assert torch.equal(mark.cpu(), torch.from_numpy(want))


@pytest.mark.parametrize("bad", [-1, N_SRC, 1 << 40])
def test_frontier_mark_bad_row_raises_and_writes_nothing(bad):
    # safe to run: the degree kernel validates every listed id before it indexes indptr, a
    # bad row gets degree 0, and the mark kernel returns at once when the flag is set
    from gnnrec import ops
    rng = np.random.default_rng(1)
    indptr, indices = _csr(np.full(N_SRC, 3, np.int64), rng)
    rows = np.sort(np.asarray([5, 9, bad, 77], np.int64))
    mark0 = (rng.random(N_DST) < 0.05).astype(np.int32)
    mark = dev(mark0)
    with pytest.raises(ValueError, match="listed row"):
        ops.frontier_mark(dev(rows), dev(indptr), dev(indices), mark)
    assert torch.equal(mark.cpu(), torch.from_numpy(mark0))


def test_frontier_mark_bad_neighbour_is_skipped_and_flagged():
    # safe to run: the neighbour id is compared with n_dst before it indexes mark
    from gnnrec import ops
    indptr = np.asarray([0, 2, 4], np.int64)
    indices = np.asarray([1, 9, -3, 2], np.int32)  # 9 and -3 lie outside [0, 4)
    mark = torch.zeros(4, dtype=torch.int32, device=DEV)
    with pytest.raises(ValueError, match="neighbour id"):
        ops.frontier_mark(dev(np.asarray([0, 1], np.int64)), dev(indptr), dev(indices), mark)
    assert mark.tolist() == [0, 1, 1, 0]


# ---- scatter_rows -----------------------------------------------------------------------
@pytest.mark.parametrize("width", [4, 128, 200])
@pytest.mark.parametrize("n", [1, 2, 1025])
def test_scatter_rows_equals_index_copy(width, n):
    from gnnrec import ops
    rng = np.random.default_rng(width * n)
    dst0 = torch.from_numpy(rng.standard_normal((3000, width)).astype(np.float32))
    idx = torch.from_numpy(np.sort(rng.permutation(3000)[:n]).astype(np.int64))
    src = torch.from_numpy(rng.standard_normal((n, width)).astype(np.float32))
    want = dst0.clone().index_copy_(0, idx, src)
    got = dst0.to(DEV)
    assert ops.scatter_rows(got, idx.to(DEV), src.to(DEV)) is got
    assert torch.equal(got.cpu(), want)
    # and it undoes gather_rows
    assert torch.equal(ops.gather_rows(got, idx.to(DEV)).cpu(), src)


def test_scatter_rows_other_dtypes_and_ids_out_of_range():
    from gnnrec import ops
    dst = torch.arange(10, dtype=torch.int64, device=DEV)          # 8-B rows
    ops.scatter_rows(dst, torch.tensor([2, 7], device=DEV), torch.tensor([-1, -2], device=DEV))
    assert dst.tolist() == [0, 1, -1, 3, 4, 5, 6, -2, 8, 9]
    d3 = torch.zeros(5, 3, dtype=torch.float32, device=DEV)        # 12-B rows: 4-B units
    # safe to run: an id outside [0, rows) is compared before it is used, and skipped
    ops.scatter_rows(d3, torch.tensor([1, 5, 99], device=DEV), torch.ones(3, 3, device=DEV))
    assert d3.sum().item() == 3 and d3[1].tolist() == [1, 1, 1]


# ---- refresh equals recompute -------------------------------------------------------------
def _graph(num_nodes, edges, feats, occurrence):
    from gnnrec.graph import HeteroGraph
    g = HeteroGraph({ce: (dev(s), dev(d)) for ce, (s, d) in edges.items()}, dict(num_nodes),
                    device=DEV)
    g.ndata["features"] = {nt: dev(f) for nt, f in feats.items()}
    for ce, o in occurrence.items():
        g.edges[ce].data["occurrence"] = dev(o)
    return g


def _layers(g, model):
    """full_graph_embeddings, keeping every layer's tables."""
    h = model.embed(g.ndata["features"])
    out = [h]
    for layer in model.layers:
        h = layer(g, h)
        out.append(h)
    return out


class Rig:
    """One route case: the device graph under IncrementalEmbeddings, its host twin, and the
    comparison of every table with a fresh pass over a freshly built graph."""

    def __init__(self, name, max_dirty_frac=1.0):
        from gnnrec import nn as gnn
        from gnnrec.inference import IncrementalEmbeddings
        c = route_graph(name)
        self.name, d = name, c["d"]
        self.tw = HostTwin(c["num_nodes"], c["edges"], c["feats"], c["occurrence"])
        self.g = _graph(c["num_nodes"], c["edges"], c["feats"], c["occurrence"])
        torch.manual_seed(11)
        self.model = gnn.ConvModel(self.g, 3, {"user": d, "item": d, "hidden": d, "out": d}, True,
                                   0.0, c["agg"], "cos", c["hetero"], True).to(DEV).eval()
        self.rng = np.random.default_rng(5)
        with torch.no_grad():
            self.inc = IncrementalEmbeddings(self.g, self.model, max_dirty_frac=max_dirty_frac)
        self.weighted = bool(c["occurrence"])
        self.frac = max_dirty_frac

    # the edits, applied to the device graph and the twin alike
    def add(self, ce, u, v):
        occ = self.rng.integers(1, 5, len(u)).astype(np.float32) if self.weighted else None
        self.inc.add_edges(dev(u), dev(v), None if occ is None else {"occurrence": dev(occ)},
                           etype=ce)
        self.tw.add_edges(ce, u, v, occ)

    def add_pairs(self, u, i, rels=(BUYS,)):
        for ce in rels:
            self.add(ce, u, i)
            self.add(reverse_of(ce), i, u)

    def remove_cold(self, n):
        lim = {"user": COLD_U, "item": COLD_I}
        for ce in self.tw.edges:
            s, d = self.tw.edges[ce]
            cold = np.nonzero((s < lim[ce[0]]) & (d < lim[ce[2]]))[0]  # both ends cold
            e = cold[self.rng.permutation(cold.size)[:n]]
            assert e.size
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
        # edges to the new nodes: new users buy cold items, cold users buy the new items
        self.add_pairs(np.asarray([n_u, n_u + 1, n_u + 2, n_u], np.int64),
                       np.asarray([0, 1, 2, 2], np.int64))
        self.add_pairs(np.asarray([4, 9, 9], np.int64), np.asarray([n_i, n_i + 1, n_i], np.int64))

    def set_features(self):
        d = self.tw.feats["item"].shape[1]
        ids = np.asarray([2, 7, 11], np.int64)
        rows = self.rng.standard_normal((3, d)).astype(np.float32)
        self.inc.set_features("item", dev(ids), dev(rows))
        self.tw.set_features("item", ids, rows)

    def check(self, what, row_path=True):
        """refresh(), then every table against a fresh pass; -> (stats, D)."""
        S, E = self.tw.take()
        D = dirty_sets(self.tw.num_nodes, self.tw.edges, S, E, 2, self.frac)
        with torch.no_grad():
            stats = self.inc.refresh()
            fresh = _graph(self.tw.num_nodes, self.tw.edges, self.tw.feats, self.tw.occurrence)
            want = _layers(fresh, self.model)
        for l, tables in enumerate(want):
            assert set(tables) == set(self.inc.layers[l]), (self.name, what, l)
            for nt, t in tables.items():
                assert torch.equal(self.inc.layers[l][nt], t), (self.name, what, l, nt)
        assert self.inc.h is self.inc.layers[-1]
        if row_path:
            assert not stats.whole_pass, (self.name, what)
            for l in range(3):
                for nt, n in self.tw.num_nodes.items():
                    # the row path really ran: exactly the restated rows, no whole layer
                    assert stats.rows[l].get(nt, 0) == D[l][nt].size, (self.name, what, l, nt, stats)
                    assert not stats.whole_layer[l].get(nt, False), (self.name, what, l, nt)
                    assert D[l][nt].size <= n / 2, (self.name, what, l, nt)
        return stats, D


ROW_PATH = [n for n in ROUTES if n != "h_lstm"]


@pytest.mark.parametrize("name", ROW_PATH)
def test_refresh_equals_recompute_on_the_row_path(name):
    r = Rig(name)
    rels = (BUYS, CLICKS) if CLICKS in r.tw.edges else (BUYS,)
    held = r.inc.h["user"]
    for n in (1, 31, 33, 257):  # dirty-row counts around the 2-row and 32-row tiles
        r.add_pairs(*cold_batch(r.rng, n, r.tw.num_nodes), rels=rels if n == 33 else (BUYS,))
        stats, D = r.check(f"add {n}")
        assert D[2]["user"].size >= min(n, COLD_U)
    assert held is r.inc.h["user"]  # updated in place: a consumer's table sees the new rows
    r.remove_cold(20)
    r.check("remove")
    r.add_nodes()
    stats, D = r.check("new nodes")
    assert held is not r.inc.h["user"]  # add_nodes replaces the tables of its type
    r.set_features()
    stats, D = r.check("features")
    assert stats.rows[0] == {"item": 3}
    # a relation whose dirty rows have no in-edge still contributes its self term: fresh
    # nodes named by mark, and one direction edited alone
    r.inc.add_nodes(2, ntype="user")
    r.tw.add_nodes("user", np.zeros((2, r.tw.feats["user"].shape[1]), np.float32))
    r.add(BOUGHT, np.asarray([1], np.int64), np.asarray([3], np.int64))
    r.check("isolated nodes, one direction")
    # nothing recorded: nothing runs
    stats = r.inc.refresh()
    assert not stats.whole_pass and not any(stats.rows)


def test_heavy_row_dirty_and_clean():
    """Route (d): the relation with a row above DEFAULT_SPLIT takes spmm + gemm whether or
    not the subset holds the heavy row, and a heavy row in the subset is chunked as in the
    whole relation."""
    from gnnrec import ops
    from incremental_cases import SPLIT
    r = Rig("d_heavy")
    heavy = r.tw.num_nodes["item"] - 1
    assert ops.split_plan(r.g.in_csr(BUYS)[0]) is not None
    assert np.bincount(r.tw.edges[BUYS][1]).max() > SPLIT
    r.add(BUYS, np.asarray([3, 8], np.int64), np.asarray([heavy, heavy], np.int64))
    _s, D = r.check("heavy row dirty")
    assert heavy in D[1]["item"]
    r.add_pairs(*cold_batch(r.rng, 5, r.tw.num_nodes))
    _s, D = r.check("heavy row clean")
    assert heavy not in D[2]["item"]


def test_a_dirty_row_above_the_extraction_cap_takes_the_whole_layer(monkeypatch):
    """ROW_PATH_MAX_DEG (2^18 in-edges by default; 2,000 here, below the heavy row's 2,500):
    the item layers with the heavy row dirty run whole, the users' stay on the row path, and
    the dirty sets do not grow."""
    from gnnrec import inference
    monkeypatch.setattr(inference, "ROW_PATH_MAX_DEG", 2000)
    r = Rig("d_heavy")
    heavy = r.tw.num_nodes["item"] - 1
    r.add(BUYS, np.asarray([3, 8], np.int64), np.asarray([heavy, heavy], np.int64))
    stats, D = r.check("above the cap", row_path=False)
    for l in (1, 2):
        assert stats.whole_layer[l]["item"] and stats.rows[l]["item"] == r.tw.num_nodes["item"]
    assert not stats.whole_layer[2]["user"] and stats.rows[2]["user"] == D[2]["user"].size > 0
    r.add_pairs(*cold_batch(r.rng, 5, r.tw.num_nodes))  # the heavy row clean: rows again
    r.check("below the cap")


def test_lstm_takes_the_whole_layer():
    r = Rig("h_lstm")
    r.add_pairs(*cold_batch(r.rng, 4, r.tw.num_nodes))
    stats, D = r.check("lstm add", row_path=False)
    assert not stats.whole_pass
    for l in (1, 2):
        for nt in ("user", "item"):
            assert D[l][nt].size and stats.whole_layer[l][nt], (l, nt, stats)
            assert stats.rows[l][nt] == r.tw.num_nodes[nt]


def test_max_dirty_frac_zero_runs_every_layer_whole():
    r = Rig("b_mfma", max_dirty_frac=0.0)
    r.add_pairs(*cold_batch(r.rng, 9, r.tw.num_nodes))
    stats, D = r.check("frac 0", row_path=False)
    assert not stats.whole_pass
    for l in (1, 2):
        assert stats.whole_layer[l] == {"user": True, "item": True}
        assert stats.rows[l] == r.tw.num_nodes


def test_size_fallback_above_the_threshold():
    """257 dirty users of 2,000 exceed max_dirty_frac = 0.05: the whole layer runs for users
    and every user counts as dirty from there on, as the restatement says."""
    r = Rig("a_valu", max_dirty_frac=0.05)
    r.add_pairs(*cold_batch(r.rng, 257, r.tw.num_nodes))
    stats, D = r.check("frac 0.05", row_path=False)
    assert stats.whole_layer[1]["user"] and not stats.whole_layer[1]["item"]
    assert stats.rows[1]["item"] == D[1]["item"].size == 3
    assert stats.rows[2] == r.tw.num_nodes  # every user dirty: every item one layer on


def test_weight_edit_and_invalidate_run_the_whole_pass():
    r = Rig("c_preprojected")
    with torch.no_grad():
        r.model.layers[0].mods["buys"].fc_self.weight.mul_(1.01)
    stats, _ = r.check("weight edit", row_path=False)
    assert stats.whole_pass
    assert not r.inc.refresh().whole_pass
    r.inc.invalidate()
    assert r.inc.refresh().whole_pass
    # a bad call records nothing and leaves graph and tables as they were
    with pytest.raises(ValueError):
        r.inc.add_edges(dev(np.asarray([10 ** 6], np.int64)), dev(np.asarray([0], np.int64)),
                        etype=BUYS)
    with pytest.raises(ValueError):
        r.inc.remove_edges(dev(np.asarray([10 ** 7], np.int64)), etype=BUYS)
    with pytest.raises(ValueError):
        r.inc.mark("user", [10 ** 6])
    stats = r.inc.refresh()
    assert not any(stats.rows) and not stats.whole_pass
    # mark(): the caller edited the graph directly
    u, i = np.asarray([6], np.int64), np.asarray([1], np.int64)
    r.g.add_edges(dev(u), dev(i), etype=BUYS)
    r.inc.mark("item", [1])
    r.tw.add_edges(BUYS, u, i)
    r.check("mark")


def test_recommendations_follow_the_refreshed_tables():
    from gnnrec import recs
    from gnnrec.inference import full_graph_embeddings
    r = Rig("a_valu")
    r.add_pairs(*cold_batch(r.rng, 33, r.tw.num_nodes))
    r.check("add 33")
    with torch.no_grad():
        fresh = _graph(r.tw.num_nodes, r.tw.edges, r.tw.feats, r.tw.occurrence)
        h = full_graph_embeddings(fresh, r.model)
    rows = torch.arange(0, 400, device=DEV)
    got = recs.recommend(r.inc.h["user"], r.inc.h["item"], 10, rows, r.g.in_csr(BOUGHT)[:2])
    want = recs.recommend(h["user"], h["item"], 10, rows, fresh.in_csr(BOUGHT)[:2])
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
