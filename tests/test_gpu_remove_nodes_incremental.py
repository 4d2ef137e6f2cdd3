"""IncrementalEmbeddings.remove_nodes and LiveRecommendations under it: after
refresh() every layer's table is torch.equal to a fresh full pass over a freshly built graph
with the filtered, relabelled edges and the kept feature rows — for a handful of items, a
handful of users, a removal together with add_edges in one refresh, and a share above
max_dirty_frac.  The dirty sets restated on the host (incremental_cases.py, extended here by
the removal: the destinations of the removed nodes' out-edges, then every recorded id
relabelled) say how many rows the row path may touch."""
import numpy as np
import pytest
import torch

from incremental_cases import BOUGHT, BUYS, COLD_I, COLD_U, HostTwin, dirty_sets, route_graph

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


class Twin(HostTwin):
    def remove_nodes(self, nt, ids):
        n = self.num_nodes[nt]
        keep = np.ones(n, bool)
        keep[ids] = False
        new_id = np.cumsum(keep) - 1
        for ce, (s, d) in self.edges.items():  # E: where the removed nodes' out-edges end
            if ce[0] == nt:
                self.E[ce[2]].append(np.unique(d[~keep[s]]))
        for ce, (s, d) in list(self.edges.items()):
            ok = np.ones(s.size, bool)
            if ce[0] == nt:
                ok &= keep[s]
            if ce[2] == nt:
                ok &= keep[d]
            s, d = s[ok], d[ok]
            self.edges[ce] = (new_id[s] if ce[0] == nt else s, new_id[d] if ce[2] == nt else d)
        for store in (self.S, self.E):  # what was recorded before, in the new numbering
            store[nt] = [new_id[a[keep[a]]] for a in store[nt]]
        self.feats[nt] = self.feats[nt][keep]
        self.num_nodes[nt] = int(keep.sum())


def _graph(num_nodes, edges, feats):
    from gnnrec.graph import HeteroGraph
    g = HeteroGraph({ce: (dev(s), dev(d)) for ce, (s, d) in edges.items()}, dict(num_nodes),
                    device=DEV)
    g.ndata["features"] = {nt: dev(f) for nt, f in feats.items()}
    return g


def _layers(g, model):
    h = model.embed(g.ndata["features"])
    out = [h]
    for layer in model.layers:
        h = layer(g, h)
        out.append(h)
    return out


class Rig:
    """One route case of incremental_cases.py (2 ConvLayers, d = 128) under
    IncrementalEmbeddings, with its host twin."""

    def __init__(self, name="a_valu", max_dirty_frac=1.0, own_feats=False):
        from gnnrec import nn as gnn
        from gnnrec.inference import IncrementalEmbeddings
        c = route_graph(name)
        d = c["d"]
        self.tw = Twin(c["num_nodes"], c["edges"], c["feats"])
        self.g = _graph(c["num_nodes"], c["edges"], c["feats"])
        torch.manual_seed(11)
        self.model = gnn.ConvModel(self.g, 3, {"user": d, "item": d, "hidden": d, "out": d}, True,
                                   0.0, c["agg"], "cos", c["hetero"], True).to(DEV).eval()
        assert len(self.model.layers) == 2
        self.frac = max_dirty_frac
        feats = {nt: dev(f) for nt, f in c["feats"].items()} if own_feats else None
        with torch.no_grad():
            self.inc = IncrementalEmbeddings(self.g, self.model, feats,
                                             max_dirty_frac=max_dirty_frac)

    def remove(self, nt, ids):
        ids = np.asarray(ids, np.int64)
        self.inc.remove_nodes(dev(ids), ntype=nt)
        self.tw.remove_nodes(nt, ids)

    def add_pairs(self, u, i):
        u, i = np.asarray(u, np.int64), np.asarray(i, np.int64)
        for ce, (s, t) in ((BUYS, (u, i)), (BOUGHT, (i, u))):
            self.inc.add_edges(dev(s), dev(t), etype=ce)
            self.tw.add_edges(ce, s, t)

    def check(self, what, row_path):
        S, E = self.tw.take()
        D = dirty_sets(self.tw.num_nodes, self.tw.edges, S, E, 2, self.frac)
        with torch.no_grad():
            stats = self.inc.refresh()
            fresh = _graph(self.tw.num_nodes, self.tw.edges, self.tw.feats)
            want = _layers(fresh, self.model)
        for l, tables in enumerate(want):
            assert set(tables) == set(self.inc.layers[l]), (what, l)
            for nt, t in tables.items():
                got = self.inc.layers[l][nt]
                assert got.shape == t.shape, (what, l, nt, got.shape, t.shape)
                assert torch.equal(got, t), (what, l, nt)
        for nt, n in self.tw.num_nodes.items():
            assert self.g.num_nodes(nt) == n
            fd = stats.final_dirty.get(nt)
            if fd is not None:  # the marks of the NEW numbering
                assert fd[0].shape == (n,) and int(fd[0].sum()) == fd[1].numel(), (what, nt)
                if fd[1].numel():
                    assert 0 <= int(fd[1].min()) and int(fd[1].max()) < n
        print(what, stats)
        if row_path:
            assert not stats.whole_pass, (what, stats)
            for l in range(3):
                for nt in self.tw.num_nodes:
                    assert stats.rows[l].get(nt, 0) == D[l][nt].size, (what, l, nt, stats)
            for nt in self.tw.num_nodes:
                fd = stats.final_dirty.get(nt)
                if D[2][nt].size and not stats.whole_layer[2].get(nt, False):
                    np.testing.assert_array_equal(fd[1].cpu().numpy(), D[2][nt])
        return stats, D


def test_remove_a_handful_of_items_then_users():
    r = Rig()
    held_u, held_i = r.inc.h["user"], r.inc.h["item"]
    n0 = r.inc.numbering
    # cold items: their buyers are cold users, so the dirty sets stay small (the row path)
    r.remove("item", [3, 0, 17, 3, COLD_I - 1])
    assert r.inc.numbering == n0 + 1
    assert r.inc.h["item"] is not held_i and r.inc.h["user"] is held_u  # item tables replaced
    assert r.inc.h["item"].shape[0] == r.tw.num_nodes["item"] == 396
    stats, D = r.check("items", row_path=True)
    assert D[1]["user"].size > 0 and D[0]["user"].size == 0
    assert D[1]["item"].size == 0 < D[2]["item"].size  # a removed row needs no mark of its own
    # users, the last one and some cold ones, repeated and unsorted
    n_u = r.tw.num_nodes["user"]
    r.remove("user", [n_u - 1, 5, 0, 77, 5, COLD_U - 1])
    assert r.inc.numbering == n0 + 2 and r.inc.h["user"].shape[0] == n_u - 5
    stats, D = r.check("users", row_path=True)
    assert D[1]["item"].size > 0
    # nothing recorded: nothing runs; the empty list is a no-op
    r.inc.remove_nodes([], ntype="user")
    assert r.inc.numbering == n0 + 2
    stats = r.inc.refresh()
    assert not stats.whole_pass and not any(stats.rows)


def test_remove_nodes_and_add_edges_in_one_refresh():
    r = Rig(own_feats=True)
    r.add_pairs([2, 9, 11], [1, 2, 5])       # recorded in the OLD numbering: item 1, 2, 5
    r.remove("item", [2, 7, 4])              # item 2 goes, 5 becomes 3
    r.add_pairs([4, 150], [3, 0])            # the NEW numbering
    r.remove("user", [9, 199])
    r.add_pairs([9], [6])
    r.check("mixed", row_path=True)
    assert r.inc._feats["item"].shape[0] == r.tw.num_nodes["item"]
    with pytest.raises(ValueError, match="outside"):
        r.inc.remove_nodes([r.tw.num_nodes["item"]], ntype="item")
    with pytest.raises(ValueError, match="ntype"):
        r.inc.remove_nodes([0])
    with pytest.raises(ValueError, match="no node type"):
        r.inc.remove_nodes([0], ntype="sport")
    stats = r.inc.refresh()  # a call that raises records nothing
    assert not stats.whole_pass and not any(stats.rows)


def test_remove_a_share_above_max_dirty_frac():
    # (c_preprojected: no routing threshold near, so the first removal stays off the whole
    # pass — bought-by keeps 2 * items <= users and 8 edges per row, buys about 30)
    r = Rig("c_preprojected", max_dirty_frac=0.25)
    rng = np.random.default_rng(3)
    n_i = r.tw.num_nodes["item"]
    r.remove("item", rng.permutation(n_i)[:n_i // 3])  # hot items: most users turn dirty
    stats, D = r.check("a third of the items", row_path=False)
    n_u = r.tw.num_nodes["user"]
    assert D[1]["user"].size == n_u  # the restatement took every row too
    assert not stats.whole_pass, stats
    assert stats.whole_layer[1]["user"] and stats.rows[1]["user"] == n_u
    assert stats.final_dirty["user"] is None
    r.remove("user", rng.permutation(n_u)[:n_u // 2])
    r.check("half of the users", row_path=False)


def test_live_recommendations_rerank_after_a_removal():
    from gnnrec import recs
    from gnnrec.inference import full_graph_embeddings
    r = Rig()
    K = 10
    live = recs.LiveRecommendations(r.inc, K, batch_size=512)
    held = live.idx

    def want():
        with torch.no_grad():
            fresh = _graph(r.tw.num_nodes, r.tw.edges, r.tw.feats)
            return recs.recommend_for_graph(fresh, full_graph_embeddings(fresh, r.model), K)

    r.remove("item", [0, 5, 399])
    with torch.no_grad():
        rs, us = live.refresh()
    assert us["full"] and live.idx is not held and not rs.whole_pass
    wi, wv = want()
    assert torch.equal(live.idx, wi) and torch.equal(live.vals, wv)
    assert int(live.idx.max()) < r.tw.num_nodes["item"]
    r.remove("user", [1, 1999])
    with torch.no_grad():
        rs, us = live.refresh()
    assert us["full"] and live.idx.shape == (r.tw.num_nodes["user"], K)
    wi, wv = want()
    assert torch.equal(live.idx, wi) and torch.equal(live.vals, wv)
    # an edit that renumbers nothing goes back to the row path of the lists
    held = live.idx
    r.add_pairs([3], [1])
    with torch.no_grad():
        rs, us = live.refresh()
    assert not us["full"] and live.idx is held
    wi, wv = want()
    assert torch.equal(live.idx, wi) and torch.equal(live.vals, wv)
