"""HeteroGraph.remove_nodes on a graph in host memory against a numpy restatement written in
remove_nodes_cases.py (mask, cumsum relabel, stable-argsort CSR), and the CPU-side checks of
torch.ops.gnnrec.node_rank_table / csr_remove_nodes (csrc/torch_ops.cpp over
csrc/csr_remove_nodes.hip): schemas with every output mutable, Meta kernels that stop after
the shape and dtype checks.  Nothing here touches a device."""
import numpy as np
import pytest
import torch

import remove_nodes_cases as rc
from remove_nodes_cases import BOUGHT, BUYS, FOLLOWS, SIMILAR

N_U, N_I, E = 41, 19, 301
NUM = {"user": N_U, "item": N_I}
# unsorted, repeated; node 0, the last node, a node without edges (N - 2), a node with many
RM = {"item": [5, 0, N_I - 1, 5, N_I - 2, 1, 5], "user": [7, 0, N_U - 1, N_U - 2, 7, 12, 0]}
UNTOUCHED = {"item": FOLLOWS, "user": SIMILAR}


def _setup(cached):
    edges = rc.make_edges(N_U, N_I, E)
    nd, ed = rc.make_data(edges, NUM)
    g = rc.build_graph(edges, NUM, nd, ed)
    if cached:
        for ce in rc.RELS:
            g.in_csr(ce)
        g.rel_graph(BUYS)  # edge data in CSR order
        g.out_csr(BUYS)
        g.edge_records(BUYS)
    return g, edges, nd, ed


@pytest.mark.parametrize("ntype", ["item", "user"])
@pytest.mark.parametrize("cached", [False, True])
def test_remove_nodes_matches_the_filtered_relabelled_graph(cached, ntype):
    g, edges, nd, ed = _setup(cached)
    deg = np.bincount(edges[BUYS][1 if ntype == "item" else 0], minlength=NUM[ntype])
    assert deg[NUM[ntype] - 2] == 0 and deg[RM[ntype]].max() >= 4  # no edges / many edges
    before = g.clone()
    free = UNTOUCHED[ntype]
    free_coo, free_csr = g._coo[free], g._csr.get(free)
    assert g.remove_nodes(torch.tensor(RM[ntype]), ntype=ntype) is None
    e2, n2, nd2, ed2, _ = rc.np_remove(edges, NUM, nd, ed, ntype, RM[ntype])
    assert n2[ntype] == NUM[ntype] - len(set(RM[ntype]))
    assert len(e2[BUYS][0]) < E and len(e2[BUYS][0]) == len(e2[BOUGHT][0])
    other = FOLLOWS if ntype == "user" else SIMILAR
    assert len(e2[other][0]) <= len(edges[other][0])
    rc.assert_graph(g, e2, n2, nd2, ed2, csr_cached=cached)
    # the relation that does not touch the type keeps the very same tensors
    assert g._coo[free][0] is free_coo[0] and g._coo[free][1] is free_coo[1]
    if cached:
        assert g._csr[free] is free_csr
    # what is dropped is rebuilt for the new numbering on next use
    assert BUYS not in g._out_csr and BUYS not in g._edge_rec
    rel = g.rel_graph(BUYS)
    np.testing.assert_array_equal(rel.edata["t"].numpy(), ed2[BUYS]["t"][rel.eids.numpy()])
    want = rc.np_csr(e2[BUYS][1], e2[BUYS][0], n2["user"])
    for got, w in zip(g.out_csr(BUYS), want):
        np.testing.assert_array_equal(got.numpy(), w)
    # the clone taken before is unaffected
    rc.assert_graph(before, edges, NUM, nd, ed, csr_cached=cached)
    # a second removal, in the NEW numbering
    rm2 = [2, n2[ntype] - 1, 2]
    g.remove_nodes(rm2, ntype=ntype)
    e3, n3, nd3, ed3, _ = rc.np_remove(e2, n2, nd2, ed2, ntype, rm2)
    rc.assert_graph(g, e3, n3, nd3, ed3)
    # the empty list: a no-op that replaces nothing
    coo = g._coo[BUYS]
    g.remove_nodes([], ntype=ntype)
    g.remove_nodes(torch.empty(0, dtype=torch.int64), ntype=ntype)
    assert g._coo[BUYS] is coo and g.num_nodes(ntype) == n3[ntype]
    # every node of the type
    g.remove_nodes(np.arange(n3[ntype]), ntype=ntype)
    e4, n4, nd4, ed4, _ = rc.np_remove(e3, n3, nd3, ed3, ntype, np.arange(n3[ntype]))
    assert n4[ntype] == 0 and len(e4[BUYS][0]) == 0
    rc.assert_graph(g, e4, n4, nd4, ed4)
    assert g.edges[BUYS].data["t"].shape == (0, 2) and g.nodes[ntype].data["f"].shape == (0, 3)
    g.remove_nodes([], ntype=ntype)


@pytest.mark.parametrize("bad", [[3, N_I], [-1], [2 ** 40]])
def test_a_bad_id_raises_and_changes_nothing(bad):
    g, edges, nd, ed = _setup(True)
    coo = dict(g._coo)
    csr = dict(g._csr)
    f = g.nodes["item"].data["f"]
    w = g.edges[BUYS].data["w"]
    with pytest.raises(ValueError, match="outside"):
        g.remove_nodes(bad, ntype="item")
    for ce in rc.RELS:
        assert g._coo[ce] is coo[ce] and g._csr[ce] is csr[ce]
    assert g.nodes["item"].data["f"] is f and g.edges[BUYS].data["w"] is w
    assert BUYS in g._out_csr and BUYS in g._edge_rec
    rc.assert_graph(g, edges, NUM, nd, ed, csr_cached=True)


def test_ntype_is_needed_and_must_exist():
    g, *_ = _setup(False)
    with pytest.raises(ValueError, match="ntype"):
        g.remove_nodes([0])  # two types: which one?
    with pytest.raises(ValueError, match="no node type"):
        g.remove_nodes([0], ntype="sport")
    one = rc.HeteroGraph({FOLLOWS: (torch.tensor([0, 1, 2]), torch.tensor([1, 2, 0]))},
                         {"user": 4})
    one.remove_nodes([1])  # one type: no ntype needed
    assert one.num_nodes("user") == 3
    assert [t.tolist() for t in one.all_edges(etype=FOLLOWS)] == [[1], [0]]


# ---- torch.ops.gnnrec.node_rank_table / csr_remove_nodes on meta tensors -------------------
def _T():
    from gnnrec import _lib
    return _lib.torch_ops()


def _meta(*shape, dtype=torch.int64):
    return torch.empty(*shape, dtype=dtype, device="meta")


def _args(E=20, n_src=40, n_dst=5, n_new=3, dev="meta", **over):
    i64, i32 = torch.int64, torch.int32
    mk = lambda n, dt=i64: torch.zeros(n, dtype=dt, device=dev)  # noqa: E731
    a = dict(src=mk(E), dst=mk(E), indptr=mk(n_dst + 1), indices=mk(E, i32), eids=mk(E),
             src_table=mk((n_src + 31) // 32 + 1), dst_table=mk((n_dst + 31) // 32 + 1),
             n_src=n_src, n_dst=n_dst, n_dst_new=n_new, workspace=mk(4096, torch.uint8),
             src_out=mk(E), dst_out=mk(E), kept_eids=mk(E), indptr_out=mk(n_new + 1),
             indices_out=mk(E, i32), eids_out=mk(E), status=mk(2))
    a.update(over)
    return list(a.values())


def _table_args(R=3, N=70, dev="meta", **over):
    mk = lambda n, dt=torch.int64: torch.zeros(n, dtype=dt, device=dev)  # noqa: E731
    W = (N + 31) // 32
    a = dict(nids=mk(R), n_nodes=N, workspace=mk(4096, torch.uint8), removed=mk(W, torch.int32),
             table=mk(W + 1), kept=mk(N), status=mk(2))
    a.update(over)
    return list(a.values())


def test_schemas_declare_the_outputs_mutable():
    T = _T()
    s = str(T.csr_remove_nodes.default._schema)
    for out in ("workspace", "src_out", "dst_out", "kept_eids", "indptr_out", "indices_out",
                "eids_out", "status"):
        assert f"!) {out}" in s, s
    assert s.endswith("-> ()")
    assert "!) src," not in s and "!) src_table" not in s and "!) dst_table" not in s
    assert "Tensor? src_table" in s and "Tensor? dst_table" in s
    s = str(T.node_rank_table.default._schema)
    for out in ("workspace", "removed", "table", "kept", "status"):
        assert f"!) {out}" in s, s
    assert s.endswith("-> ()") and "!) nids" not in s
    assert int(T.csr_remove_nodes_workspace_bytes(0, 0)) > 0
    assert int(T.node_rank_table_workspace_bytes(0)) > 0
    small, large = (int(T.csr_remove_nodes_workspace_bytes(e, 7)) for e in (1000, 10 ** 6))
    assert small < large < 10 ** 6  # well under a byte per edge
    assert int(T.node_rank_table_workspace_bytes(10 ** 6)) < 10 ** 6


def test_meta_kernels_check_shapes_and_dtypes():
    T = _T()
    T.csr_remove_nodes(*_args())  # fine: nothing launches on meta
    T.csr_remove_nodes(*_args(E=0))
    T.csr_remove_nodes(*_args(src_table=None))
    T.csr_remove_nodes(*_args(dst_table=None, n_new=5))
    # the COO alone: every CSR operand empty
    T.csr_remove_nodes(*_args(indptr=_meta(0), indices=_meta(0, dtype=torch.int32),
                              eids=_meta(0), indptr_out=_meta(0),
                              indices_out=_meta(0, dtype=torch.int32), eids_out=_meta(0)))
    with pytest.raises(ValueError, match="one length"):
        T.csr_remove_nodes(*_args(src=_meta(19)))
    with pytest.raises(ValueError, match="the CSR must be"):
        T.csr_remove_nodes(*_args(eids=_meta(19)))
    with pytest.raises(ValueError, match="the CSR must be"):
        T.csr_remove_nodes(*_args(indptr=_meta(5)))
    with pytest.raises(ValueError, match="output sizes"):
        T.csr_remove_nodes(*_args(indptr_out=_meta(6)))  # the OLD row count
    with pytest.raises(ValueError, match="output sizes"):
        T.csr_remove_nodes(*_args(kept_eids=_meta(21)))
    with pytest.raises(ValueError, match="output sizes"):
        T.csr_remove_nodes(*_args(status=_meta(1)))
    with pytest.raises(ValueError, match="indices must be Int"):
        T.csr_remove_nodes(*_args(indices=_meta(20)))
    with pytest.raises(ValueError, match="src_table must be Long"):
        T.csr_remove_nodes(*_args(src_table=_meta(3, dtype=torch.int32)))
    with pytest.raises(ValueError, match="rank table"):
        T.csr_remove_nodes(*_args(dst_table=_meta(3)))
    with pytest.raises(ValueError, match="a source table, a destination table or both"):
        T.csr_remove_nodes(*_args(src_table=None, dst_table=None, n_new=5))
    with pytest.raises(ValueError, match="n_dst_new"):
        T.csr_remove_nodes(*_args(dst_table=None, n_new=3))  # no table: the rows stay
    with pytest.raises(ValueError, match="n_dst_new"):
        T.csr_remove_nodes(*_args(n_new=6))
    T.node_rank_table(*_table_args())
    T.node_rank_table(*_table_args(R=0, N=0))
    with pytest.raises(ValueError, match="output sizes"):
        T.node_rank_table(*_table_args(table=_meta(3)))
    with pytest.raises(ValueError, match="output sizes"):
        T.node_rank_table(*_table_args(kept=_meta(69)))
    with pytest.raises(ValueError, match="removed must be Int"):
        T.node_rank_table(*_table_args(removed=_meta(3)))
    with pytest.raises(ValueError, match="nids must be Long"):
        T.node_rank_table(*_table_args(nids=_meta(3, dtype=torch.int32)))
    with pytest.raises(ValueError, match="contiguous 1-D"):
        T.node_rank_table(*_table_args(nids=_meta(3, 2)))
    with pytest.raises(ValueError, match="negative"):
        T.node_rank_table(*_table_args(n_nodes=-1))


def test_cpu_tensors_are_refused():
    from gnnrec import ops
    with pytest.raises(ValueError, match="HIP device tensor"):
        _T().csr_remove_nodes(*_args(dev="cpu"))
    with pytest.raises(ValueError, match="HIP device tensor"):
        _T().node_rank_table(*_table_args(dev="cpu"))
    z = torch.zeros(4, dtype=torch.int64)
    with pytest.raises(ValueError, match="HIP device tensor"):
        ops.node_rank_table(z, 9)
    with pytest.raises(ValueError, match="HIP device tensor"):
        ops.csr_remove_nodes(z, z, None, z[:2], None, 9, 9, 9)


def test_ops_wrappers_trace_on_meta():
    from gnnrec import ops
    removed, table, kept = ops.node_rank_table(_meta(3), 70)
    assert removed.shape == (3,) and removed.dtype == torch.int32
    assert table.shape == (4,) and kept.shape == (70,)
    s, d, csr = _meta(20), _meta(20), (_meta(6), _meta(20, dtype=torch.int32), _meta(20))
    s2, d2, kept_e, csr2 = ops.csr_remove_nodes(s, d, csr, table, _meta(2), 70, 5, 3)
    assert s2.shape == d2.shape == kept_e.shape == (20,) and csr2[0].shape == (4,)
    assert csr2[1].dtype == torch.int32 and csr2[2].shape == (20,)
    assert ops.csr_remove_nodes(s, d, None, table, None, 70, 5, 5)[3] is None
    pending, status = ops.csr_remove_nodes(s, d, csr, None, _meta(2), 70, 5, 3, sync=False)
    assert status.shape == (2,)
    assert ops.csr_remove_nodes_finish(pending, 7, 0)[0].shape == (7,)
    with pytest.raises(ValueError, match="outside"):
        ops.csr_remove_nodes_finish(pending, 20, 1)
    with pytest.raises(ValueError, match="rank table"):
        ops.csr_remove_nodes(s, d, csr, _meta(9), None, 70, 5, 5)
    with pytest.raises(ValueError, match="new rows"):
        ops.csr_remove_nodes(s, d, csr, table, None, 70, 5, 3)
    with pytest.raises(ValueError, match="n_dst \\+ 1"):
        ops.csr_remove_nodes(s, d, (_meta(5), csr[1], csr[2]), table, None, 70, 5, 5)
