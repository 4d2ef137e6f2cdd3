"""CPU-side checks of the incremental embedding refresh (gnnrec.inference.
IncrementalEmbeddings): the dirty-set definition is SOUND — after every kind of
edit, every row of the oracle's full-graph pass outside the restated D_L keeps its bits — the
restatement gives the sets worked out by hand on three- and four-node graphs, and a host
graph or a CPU tensor is refused (there is no CPU path).  The device tests are in
tests/test_gpu_incremental.py."""
import numpy as np
import pytest
import torch

from incremental_cases import (BOUGHT, BUYS, HostTwin, dirty_sets, out_neighbours, route_graph,
                               ROUTES)
from oracle import oracle

I64 = np.int64


def ids(*v):
    return np.asarray(v, I64)


def as_lists(D):
    return [{nt: v.tolist() for nt, v in d.items()} for d in D]


# ---- the restatement on hand-made graphs ---------------------------------------------------
def test_three_node_chain():
    """u0 -buys-> i0 -bought-by-> u1: a feature change of u0 reaches i0 after one layer and u1
    after two; nothing flows against the edges."""
    nn_ = {"user": 2, "item": 1}
    edges = {BUYS: (ids(0), ids(0)), BOUGHT: (ids(0), ids(1))}
    D = dirty_sets(nn_, edges, {"user": ids(0)}, {}, 2)
    assert as_lists(D) == [{"user": [0], "item": []}, {"user": [0], "item": [0]},
                           {"user": [0, 1], "item": [0]}]
    # an edge INTO u1 (E): u1 from layer 1 on, and no one else — u1 has no out-edge
    D = dirty_sets(nn_, edges, {}, {"user": ids(1)}, 2)
    assert as_lists(D) == [{"user": [], "item": []}, {"user": [1], "item": []},
                           {"user": [1], "item": []}]


def test_four_node_pair():
    """users 0, 1 and items 0, 1 with buys = {0->0, 1->0, 1->1} and its reverse: the new
    edge 0->1 (both directions) dirties its endpoints at layer 1 and their out-neighbours —
    on the EDITED graph — at layer 2."""
    nn_ = {"user": 2, "item": 2}
    u, i = ids(0, 1, 1, 0), ids(0, 0, 1, 1)  # the last pair is the new edge
    edges = {BUYS: (u, i), BOUGHT: (i, u)}
    assert out_neighbours(edges, BUYS, ids(0)).tolist() == [0, 1]
    D = dirty_sets(nn_, edges, {}, {"item": ids(1), "user": ids(0)}, 2)
    assert as_lists(D)[1] == {"user": [0], "item": [1]}
    assert as_lists(D)[2] == {"user": [0, 1], "item": [0, 1]}
    # the size cut: above half of a type's rows the set becomes every row; 0 cuts any set
    D = dirty_sets({"user": 4, "item": 2}, edges, {}, {"user": ids(0, 1, 2)}, 1, 0.5)
    assert as_lists(D)[1] == {"user": [0, 1, 2, 3], "item": []}
    D = dirty_sets({"user": 4, "item": 2}, edges, {}, {"user": ids(3)}, 1, 0.0)
    assert as_lists(D)[1]["user"] == [0, 1, 2, 3] and as_lists(D)[0]["user"] == []


def test_route_cases_stay_within_the_sizes_the_issue_names():
    for name in ROUTES:
        c = route_graph(name)
        assert c["num_nodes"]["user"] <= 3000 and c["num_nodes"]["item"] <= 1010
        assert all(s.size <= 60000 for s, _ in c["edges"].values())


# ---- soundness against the oracle's full-graph pass --------------------------------------
def _model(agg, d, hetero="sum"):
    from gnnrec import nn as gnn
    from gnnrec.synth import GraphMeta
    meta = GraphMeta([BUYS, BOUGHT], ["item", "user"])
    torch.manual_seed(3)
    m = gnn.ConvModel(meta, 3, {"user": d, "item": d, "hidden": d, "out": d}, True, 0.0, agg,
                      "cos", hetero, True)
    return {k: v.detach().numpy() for k, v in m.state_dict().items()}


def _pass(tw, sd, agg):
    g = oracle.Graph(tw.num_nodes, tw.edges, tw.occurrence)
    return oracle.model_full_graph(g, tw.feats, sd, agg, "sum", True, True)


def _edits(tw, rng):
    """name -> a function applying one edit kind to the twin."""
    n_u, n_i = tw.num_nodes["user"], tw.num_nodes["item"]
    d = tw.feats["user"].shape[1]

    def add():
        u, i = rng.integers(0, n_u, 3), rng.integers(0, n_i, 3)
        tw.add_edges(BUYS, u, i)
        tw.add_edges(BOUGHT, i, u)

    def remove():
        e = rng.permutation(tw.edges[BUYS][0].size)[:3]
        tw.remove_edges(BUYS, e)
        tw.remove_edges(BOUGHT, e)

    def nodes():
        tw.add_nodes("user", rng.standard_normal((2, d)).astype(np.float32))
        tw.add_edges(BUYS, ids(n_u, n_u + 1), rng.integers(0, n_i, 2))
        tw.add_edges(BOUGHT, rng.integers(0, n_i, 2), ids(n_u, n_u + 1))

    def features():
        tw.set_features("item", ids(1, 5), rng.standard_normal((2, d)).astype(np.float32))

    def one_direction():
        tw.add_edges(BOUGHT, rng.integers(0, n_i, 2), rng.integers(0, n_u, 2))

    return {"add": add, "remove": remove, "nodes": nodes, "features": features,
            "one direction": one_direction}


@pytest.mark.parametrize("agg", ["mean", "pool_nn"])
@pytest.mark.parametrize("seed", [0, 1])
def test_rows_outside_the_dirty_set_keep_their_bits(agg, seed):
    rng = np.random.default_rng(seed)
    n_u, n_i, d, E = 240, 90, 16, 500  # sparse: two hops reach a small part of the graph
    u, i = rng.integers(0, n_u, E), rng.integers(0, n_i, E)
    feats = {"user": rng.standard_normal((n_u, d)).astype(np.float32),
             "item": rng.standard_normal((n_i, d)).astype(np.float32)}
    tw = HostTwin({"user": n_u, "item": n_i}, {BUYS: (u, i), BOUGHT: (i, u)}, feats)
    sd = _model(agg, d)
    before = _pass(tw, sd, agg)
    for name in ("add", "remove", "nodes", "features", "one direction"):
        _edits(tw, rng)[name]()
        S, E_ = tw.take()
        D = dirty_sets(tw.num_nodes, tw.edges, S, E_, 2)[-1]
        after = _pass(tw, sd, agg)
        spared = 0
        for nt, old in before.items():
            clean = np.setdiff1d(np.arange(old.shape[0]), D[nt])
            assert clean.size, (name, nt)  # the check must have rows to look at
            spared += clean.size
            assert np.array_equal(after[nt][clean].view(np.uint32), old[clean].view(np.uint32)), \
                (name, nt)
        # and the sets are not vacuous the other way: some dirty row did change
        changed = sum(int((after[nt][:old.shape[0]] != old).any(1).sum())
                      for nt, old in before.items())
        assert changed > 0 and spared > 0, name
        before = after


# ---- no CPU path ---------------------------------------------------------------------------
def test_host_graph_and_cpu_tensors_are_refused():
    from gnnrec import nn as gnn
    from gnnrec import ops
    from gnnrec.graph import HeteroGraph
    from gnnrec.inference import IncrementalEmbeddings
    g = HeteroGraph({BUYS: (torch.tensor([0, 1]), torch.tensor([1, 0])),
                     BOUGHT: (torch.tensor([1, 0]), torch.tensor([0, 1]))},
                    {"user": 2, "item": 2})
    g.ndata["features"] = {"user": torch.zeros(2, 8), "item": torch.zeros(2, 8)}
    model = gnn.ConvModel(g, 3, {"user": 8, "item": 8, "hidden": 8, "out": 8}).eval()
    with pytest.raises(ValueError, match="no CPU path"):
        IncrementalEmbeddings(g, model)
    i64, i32 = torch.int64, torch.int32
    with pytest.raises(ValueError, match="no CPU path"):
        ops.frontier_mark(torch.zeros(1, dtype=i64), torch.zeros(3, dtype=i64),
                          torch.zeros(2, dtype=i32), torch.zeros(2, dtype=i32))
    with pytest.raises(ValueError, match="no CPU path"):
        ops.scatter_rows(torch.zeros(4, 8), torch.zeros(1, dtype=i64), torch.zeros(1, 8))


def test_meta_kernels_check_the_new_ops():
    from gnnrec import _lib
    T = _lib.torch_ops()

    def meta(*shape, dtype=torch.float32):
        return torch.empty(*shape, dtype=dtype, device="meta")

    i64, i32, u8 = torch.int64, torch.int32, torch.uint8
    T.frontier_mark(meta(5, dtype=i64), None, meta(9, dtype=i64), meta(20, dtype=i32),
                    meta(7, dtype=i32), meta(64, dtype=u8), meta(2, dtype=i64))
    with pytest.raises(ValueError, match="status"):
        T.frontier_mark(meta(5, dtype=i64), None, meta(9, dtype=i64), meta(20, dtype=i32),
                        meta(7, dtype=i32), meta(64, dtype=u8), meta(3, dtype=i64))
    with pytest.raises(ValueError, match="indices must be Int"):
        T.frontier_mark(meta(5, dtype=i64), None, meta(9, dtype=i64), meta(20, dtype=i64),
                        meta(7, dtype=i32), meta(64, dtype=u8), meta(2, dtype=i64))
    T.scatter_rows(meta(3, 8), meta(3, dtype=i64), meta(10, 8))
    with pytest.raises(ValueError, match="row shapes differ"):
        T.scatter_rows(meta(3, 4), meta(3, dtype=i64), meta(10, 8))
    with pytest.raises(ValueError, match="scatter_rows"):
        T.scatter_rows(meta(2, 8), meta(3, dtype=i64), meta(10, 8))
    assert T.frontier_mark_workspace_bytes(0) > 0
    assert T.frontier_mark_workspace_bytes(1000) >= 8 * 1001


def test_route_pin_overrides_the_subsets_own_figures():
    """A CSR with `_gnnrec_route` routes by the whole relation's figures; one without it is
    untouched (every existing caller)."""
    from gnnrec import ops
    ip = torch.tensor([0, 1, 2, 3], dtype=torch.int64)  # 1 edge per row: 'mfma' by itself
    ip._gnnrec_nnz = 3
    assert ops.fused_variant(ip) == "mfma" and ops.routed_n_dst(ip, 3) == 3
    ops.pin_route(ip, ops.Route(30.0, 1000, False), 3)
    assert ops.fused_variant(ip) == "valu" and ops.routed_n_dst(ip, 3) == 1000
    assert ops.fused_variant(ip, avg_deg=2.0) == "mfma"  # an explicit figure still wins
    r = ops.relation_route(torch.tensor([0, 3000, 3001], dtype=torch.int64))
    assert r.has_split and r.n_dst == 2 and r.avg_deg == 3001 / 2
