"""HeteroGraph.add_edges / add_nodes on a graph in host memory, and the CPU side of
torch.ops.gnnrec.csr_add_edges (csrc/torch_ops.cpp over csrc/csr_merge.hip): the host path of
both methods against a fresh host graph built from the concatenated COO, the frame rules, and
the ops' schemas and Meta kernels (nothing launches here)."""
import numpy as np
import pytest
import torch

BUYS, BOUGHT = ("user", "buys", "item"), ("item", "bought-by", "user")
N_U, N_I = 30, 11


def _graph(E=200, seed=0, n_u=N_U, n_i=N_I):
    from gnnrec.graph import HeteroGraph
    rng = np.random.default_rng(seed)
    # items n_i - 3 .. n_i - 1 start without edges
    u = torch.from_numpy(rng.integers(0, n_u, E))
    i = torch.from_numpy(rng.integers(0, max(n_i - 3, 1), E))
    g = HeteroGraph({BUYS: (u, i), BOUGHT: (i, u)}, {"user": n_u, "item": n_i})
    for ce in (BUYS, BOUGHT):
        g.edges[ce].data["occurrence"] = torch.from_numpy(rng.integers(1, 9, E))
        g.edges[ce].data["w"] = torch.from_numpy(rng.standard_normal((E, 3)).astype(np.float32))
    g.nodes["user"].data["features"] = torch.from_numpy(
        rng.standard_normal((n_u, 5)).astype(np.float32))
    g.nodes["item"].data["features"] = torch.from_numpy(
        rng.standard_normal((n_i, 6)).astype(np.float32))
    return g


def _fresh(g):
    from gnnrec.graph import HeteroGraph
    return HeteroGraph({ce: g.all_edges(etype=ce) for ce in g.canonical_etypes},
                       {nt: g.num_nodes(nt) for nt in g.ntypes})


def _same_structure(g, what=""):
    f = _fresh(g)
    for ce in g.canonical_etypes:
        for a, b in zip(g.in_csr(ce), f.in_csr(ce)):
            assert a.dtype == b.dtype and torch.equal(a, b), (what, ce, "in")
        for a, b in zip(g.out_csr(ce), f.out_csr(ce)):
            assert a.dtype == b.dtype and torch.equal(a, b), (what, ce, "out")
        E = g.num_edges(ce)
        for k, v in g._edata[ce].items():
            assert v.shape[0] == E, (what, ce, k)


def _batches(E, n_u, n_i, rng):
    s, d = rng.integers(0, n_u, max(E, 1)), rng.integers(0, max(n_i - 3, 1), max(E, 1))
    return {"row 0": (rng.integers(0, n_u, 9), np.zeros(9, dtype=np.int64)),
            "last row": (rng.integers(0, n_u, 9), np.full(9, n_i - 1)),
            "empty rows": (rng.integers(0, n_u, 6), np.repeat(np.arange(max(n_i - 3, 0), n_i), 2)),
            "every row once": (rng.integers(0, n_u, n_i), rng.permutation(n_i)),
            "random": (rng.integers(0, n_u, 50), rng.integers(0, n_i, 50)),
            "one": (np.array([n_u - 1]), np.array([n_i // 2])),
            "duplicates": (s[:7], d[:7])}


@pytest.mark.parametrize("E", [0, 1, 200])
@pytest.mark.parametrize("cached", [True, False])
def test_host_add_edges_equals_a_fresh_graph(E, cached):
    rng = np.random.default_rng(E + 5)
    ref = _graph(E)
    s0, d0 = ref.all_edges(etype=BUYS)
    for name, (u, v) in _batches(E, N_U, N_I, rng).items():
        if name == "duplicates" and E:
            u, v = s0[:7].numpy(), d0[:7].numpy()
        g = _graph(E)
        if cached:
            g.in_csr(BUYS), g.out_csr(BUYS), g.in_csr(BOUGHT)
        csr_before = g._csr.get(BUYS)
        assert g.add_edges(u, v, etype=BUYS) is None
        g.add_edges(torch.from_numpy(v), torch.from_numpy(u), etype="bought-by")
        assert g.num_edges(BUYS) == E + len(u) == g.num_edges(BOUGHT)
        s, d = g.all_edges(etype=BUYS)
        assert torch.equal(s, torch.cat([s0, torch.from_numpy(u)])), name
        assert torch.equal(d, torch.cat([d0, torch.from_numpy(v)])), name
        if cached:
            assert g._csr[BUYS] is not csr_before and BUYS in g._out_csr
            assert BOUGHT not in g._out_csr  # a CSR that was not cached stays unbuilt
        else:
            assert not g._csr and not g._out_csr
        _same_structure(g, name)
        assert bool(g.has_edges_between(u, v, etype=BUYS).all()), name
        # the old frame rows are kept, the new ones are zero
        for k in ("occurrence", "w"):
            assert torch.equal(g.edges[BUYS].data[k][:E], ref.edges[BUYS].data[k])
            assert not bool(g.edges[BUYS].data[k][E:].any())


def test_host_add_nodes_then_edges_to_them():
    g = _graph()
    g.in_csr(BUYS), g.out_csr(BUYS), g.in_csr(BOUGHT)
    feats = torch.arange(12, dtype=torch.float32).reshape(2, 6)
    assert g.add_nodes(2, {"features": feats}, ntype="item") is None
    g.add_nodes(3, ntype="user")
    assert g.num_nodes("item") == N_I + 2 and g.num_nodes("user") == N_U + 3
    assert torch.equal(g.nodes["item"].data["features"][N_I:], feats)
    assert g.nodes["user"].data["features"].shape == (N_U + 3, 5)
    assert not bool(g.nodes["user"].data["features"][N_U:].any())
    assert g.in_csr(BUYS)[0].numel() == N_I + 3 and g.out_csr(BUYS)[0].numel() == N_U + 4
    _same_structure(g, "after add_nodes")
    g.add_edges([N_U + 2, 0], [N_I + 1, N_I + 1], etype=BUYS)
    _same_structure(g, "edges to the new nodes")
    assert g.has_edges_between([N_U + 2, N_U + 1], [N_I + 1, N_I + 1], etype=BUYS).tolist() == \
        [True, False]
    u, v = g.out_edges([N_U + 2], etype=BUYS)
    assert u.tolist() == [N_U + 2] and v.tolist() == [N_I + 1]


def test_frame_rules():
    g = _graph()
    E = g.num_edges(BUYS)
    occ = torch.tensor([4, 5])
    g.add_edges([1, 2], [3, 4], {"occurrence": occ, "fresh": torch.tensor([1.5, 2.5])}, etype=BUYS)
    d = g.edges[BUYS].data
    assert torch.equal(d["occurrence"][E:], occ) and d["occurrence"].dtype == torch.int64
    assert d["w"].shape == (E + 2, 3) and not bool(d["w"][E:].any())  # zero fill
    assert d["fresh"].shape == (E + 2,) and not bool(d["fresh"][:E].any())  # a new field
    assert d["fresh"][E:].tolist() == [1.5, 2.5]
    assert "fresh" not in g.edges[BOUGHT].data
    for bad, match in (({"occurrence": torch.tensor([1, 2, 3])}, "rows"),
                       ({"occurrence": torch.tensor([1.0, 2.0])}, "float32"),
                       ({"w": torch.zeros(2, 4)}, "trailing shape"),
                       ({"w": torch.zeros(2)}, "trailing shape")):
        with pytest.raises(ValueError, match=match):
            g.add_edges([1, 2], [3, 4], bad, etype=BUYS)
        assert g.num_edges(BUYS) == E + 2 and d["w"].shape[0] == E + 2
    with pytest.raises(ValueError, match="rows"):
        g.add_nodes(2, {"features": torch.zeros(3, 6)}, ntype="item")
    with pytest.raises(ValueError, match="trailing shape"):
        g.add_nodes(2, {"features": torch.zeros(2, 5)}, ntype="item")
    with pytest.raises(ValueError, match="float64"):
        g.add_nodes(2, {"features": torch.zeros(2, 6, dtype=torch.float64)}, ntype="item")
    assert g.num_nodes("item") == N_I
    g.add_nodes(1, {"age": torch.tensor([7])}, ntype="user")
    assert g.nodes["user"].data["age"].tolist() == [0] * N_U + [7]
    with pytest.raises(ValueError, match="source ids"):
        g.add_edges([1, 2], [3], etype=BUYS)


@pytest.mark.parametrize("cached", [True, False])
@pytest.mark.parametrize("u,v", [([0, N_U], [0, 0]), ([0], [N_I]), ([-1], [0]), ([0], [1 << 40])])
def test_out_of_range_id_leaves_the_graph_unchanged(cached, u, v):
    g = _graph()
    if cached:
        g.in_csr(BUYS), g.out_csr(BUYS)
    coo, csr = g.all_edges(etype=BUYS), g._csr.get(BUYS)
    frames = dict(g.edges[BUYS].data.lazy_items())
    with pytest.raises(ValueError, match="outside"):
        g.add_edges(u, v, etype=BUYS)
    assert all(a is b for a, b in zip(g.all_edges(etype=BUYS), coo)) and g._csr.get(BUYS) is csr
    assert all(g.edges[BUYS].data[k] is t for k, t in frames.items())
    assert g.num_nodes("user") == N_U and g.num_nodes("item") == N_I


def test_etype_and_ntype_are_required_on_a_graph_with_several():
    from gnnrec.graph import HeteroGraph
    g = _graph()
    with pytest.raises(ValueError, match="etype"):
        g.add_edges([0], [0])
    with pytest.raises(ValueError, match="ntype"):
        g.add_nodes(1)
    with pytest.raises(ValueError, match="node type"):
        g.add_nodes(1, ntype="sport")
    one = HeteroGraph({("n", "e", "n"): (torch.tensor([0, 1]), torch.tensor([1, 2]))}, {"n": 3})
    one.in_csr("e")
    one.add_nodes(1)
    one.add_edges([3], [0])
    assert one.num_nodes("n") == 4 and one.num_edges("e") == 3
    _same_structure(one)


def test_empty_batch_is_a_no_op():
    g = _graph()
    g.in_csr(BUYS)
    coo, csr, w = g.all_edges(etype=BUYS), g._csr[BUYS], g.edges[BUYS].data["w"]
    g.add_edges([], [], etype=BUYS)
    g.add_edges(torch.empty(0, dtype=torch.int64), np.empty(0, dtype=np.int64), etype=BUYS)
    g.add_nodes(0, ntype="user")
    assert all(a is b for a, b in zip(g.all_edges(etype=BUYS), coo))
    assert g._csr[BUYS] is csr and g.edges[BUYS].data["w"] is w and g.num_nodes("user") == N_U


def test_clone_taken_before_is_unaffected():
    g = _graph()
    g.in_csr(BUYS), g.out_csr(BUYS)
    c = g.clone()
    E = g.num_edges(BUYS)
    g.add_nodes(2, ntype="item")
    g.add_edges([0, 1], [N_I + 1, 0], {"occurrence": torch.tensor([3, 3])}, etype=BUYS)
    assert c.num_edges(BUYS) == E and c.num_nodes("item") == N_I
    assert c.in_csr(BUYS)[0].numel() == N_I + 1 and c.in_csr(BUYS)[1].numel() == E
    assert c.edges[BUYS].data["occurrence"].shape[0] == E
    assert c.nodes["item"].data["features"].shape[0] == N_I
    _same_structure(c)
    _same_structure(g)


# ---- the torch ops (Meta kernels: nothing launches) -------------------------------------------
def _T():
    from gnnrec import _lib
    return _lib.torch_ops()


def _meta(*shape, dtype=torch.int64):
    return torch.empty(*shape, dtype=dtype, device="meta")


def _args(E=20, n=4, n_src=9, n_dst=5, dev="meta", **over):
    i64, i32 = torch.int64, torch.int32
    mk = lambda k, dt=i64: torch.zeros(k, dtype=dt, device=dev)  # noqa: E731
    a = dict(indptr=mk(n_dst + 1), indices=mk(E, i32), eids=mk(E), src_new=mk(n), dst_new=mk(n),
             n_src=n_src, n_dst=n_dst, workspace=mk(4096, torch.uint8), indptr_out=mk(n_dst + 1),
             indices_out=mk(E + n, i32), eids_out=mk(E + n), status=mk(2))
    a.update(over)
    return list(a.values())


def test_schema_declares_the_outputs_mutable():
    T = _T()
    s = str(T.csr_add_edges.default._schema)
    for out in ("workspace", "indptr_out", "indices_out", "eids_out", "status"):
        assert f"!) {out}" in s, s
    assert s.endswith("-> ()")
    for inp in ("indptr,", "indices,", "eids,", "src_new", "dst_new"):
        assert f"!) {inp}" not in s, s
    assert "int n_src, int n_dst" in s
    assert "-> int" in str(T.csr_add_edges_workspace_bytes.default._schema)
    assert int(T.csr_add_edges_workspace_bytes(0, 0)) > 0
    assert int(T.csr_add_edges_workspace_bytes(-3, 7)) == int(T.csr_add_edges_workspace_bytes(0, 7))
    small, large = (int(T.csr_add_edges_workspace_bytes(n, 7)) for n in (1000, 10 ** 6))
    assert small < large < 100 * 10 ** 6  # a function of the BATCH, not of the relation


def test_meta_kernel_checks_shapes_and_dtypes():
    T = _T()
    T.csr_add_edges(*_args())  # fine: nothing launches on meta
    T.csr_add_edges(*_args(E=0))
    T.csr_add_edges(*_args(n=0))
    T.csr_add_edges(*_args(E=0, n=0, n_dst=0, n_src=0))
    with pytest.raises(ValueError, match="the CSR must be"):
        T.csr_add_edges(*_args(indptr=_meta(5)))
    with pytest.raises(ValueError, match="the CSR must be"):
        T.csr_add_edges(*_args(indices=_meta(19, dtype=torch.int32)))
    with pytest.raises(ValueError, match="one length"):
        T.csr_add_edges(*_args(src_new=_meta(3)))
    with pytest.raises(ValueError, match="one length"):
        T.csr_add_edges(*_args(src_new=_meta(2, 2)))
    with pytest.raises(ValueError, match="output sizes"):
        T.csr_add_edges(*_args(indices_out=_meta(20, dtype=torch.int32)))
    with pytest.raises(ValueError, match="output sizes"):
        T.csr_add_edges(*_args(eids_out=_meta(25)))
    with pytest.raises(ValueError, match="output sizes"):
        T.csr_add_edges(*_args(indptr_out=_meta(5)))
    with pytest.raises(ValueError, match="output sizes"):
        T.csr_add_edges(*_args(status=_meta(1)))
    with pytest.raises(ValueError, match="indices must be Int"):
        T.csr_add_edges(*_args(indices=_meta(20)))
    with pytest.raises(ValueError, match="dst_new must be Long"):
        T.csr_add_edges(*_args(dst_new=_meta(4, dtype=torch.int32)))
    with pytest.raises(ValueError, match="indices_out must be Int"):
        T.csr_add_edges(*_args(indices_out=_meta(24)))
    with pytest.raises(ValueError, match="negative"):
        T.csr_add_edges(*_args(n_src=-1))
    with pytest.raises(ValueError, match="HIP device tensor"):
        T.csr_add_edges(*_args(dev="cpu"))


def test_ops_wrapper_traces_on_meta():
    from gnnrec import ops
    csr = (_meta(6), _meta(20, dtype=torch.int32), _meta(20))
    ip, ix, eid = ops.csr_add_edges(csr, _meta(4), _meta(4), 9, 5)
    assert ip.shape == (6,) and ix.shape == eid.shape == (24,)
    assert ix.dtype == torch.int32 and eid.dtype == ip.dtype == torch.int64
    assert ip._gnnrec_nnz == 24
    with pytest.raises(ValueError, match="one length"):
        ops.csr_add_edges(csr, _meta(4), _meta(3), 9, 5)
    with pytest.raises(ValueError, match="indptr"):
        ops.csr_add_edges(csr, _meta(4), _meta(4), 9, 6)
    z = torch.zeros(4, dtype=torch.int64)
    with pytest.raises(ValueError, match="HIP device tensor"):
        ops.csr_add_edges((z, z.to(torch.int32), z), z, z, 9, 3)
