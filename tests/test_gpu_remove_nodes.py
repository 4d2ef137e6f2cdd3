"""HeteroGraph.remove_nodes on the device (csrc/csr_remove_nodes.hip): every array — COO,
kept edge ids, the three CSR arrays with their dtypes, node and edge data — equals that of a
HeteroGraph built from the filtered, relabelled COO with its in-CSR built by the library's
sort, and the numpy restatement of remove_nodes_cases.py.  Sizes cross every boundary the
kernels have: node counts that are no multiple of 32, edge counts that are no multiple of 64,
a CSR row that straddles 64-slot chunks, an empty relation, and one relation past the flat
grid's cap so the grid-stride loops run."""
import numpy as np
import pytest
import torch

import remove_nodes_cases as rc
from remove_nodes_cases import BOUGHT, BUYS, FOLLOWS, SIMILAR

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
N_U, N_I, E = 300, 77, 3001
NUM = {"user": N_U, "item": N_I}
# unsorted, repeated; node 0, the last node, the heavy item 1, ids around the 32-id words
# (node N - 2, which has no edge, stays for a removal of its own)
RM = {"item": [5, 0, N_I - 1, 5, 1, 33, 64, 5],
      "user": [7, 0, N_U - 1, 7, 12, 0, 31, 32, 255, 256]}
UNTOUCHED = {"item": FOLLOWS, "user": SIMILAR}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _setup(cached, **kw):
    edges = rc.make_edges(N_U, N_I, E, **kw)
    nd, ed = rc.make_data(edges, NUM)
    g = rc.build_graph(edges, NUM, nd, ed, device=DEV)
    if cached:
        for ce in rc.RELS:
            g.in_csr(ce)
        g.rel_graph(BUYS)
        g.out_csr(BUYS)
        g.edge_records(BUYS)
    return g, edges, nd, ed


def _assert_equals_fresh(g, edges, num_nodes):
    """The cached CSRs against a graph built from the restated COO, bit for bit."""
    fresh = rc.build_graph(edges, num_nodes, device=DEV)
    for ce in edges:
        assert ce in g._csr
        for got, want in zip(g._csr[ce], fresh.in_csr(ce)):
            assert got.dtype == want.dtype and got.shape == want.shape, ce
            assert torch.equal(got, want), ce
        for got, want in zip(g.all_edges(etype=ce), fresh.all_edges(etype=ce)):
            assert torch.equal(got, want), ce


@pytest.mark.parametrize("ntype", ["item", "user"])
@pytest.mark.parametrize("cached", [False, True])
def test_remove_nodes_equals_the_rebuilt_graph(cached, ntype):
    g, edges, nd, ed = _setup(cached)
    deg = np.bincount(edges[BUYS][1], minlength=N_I)
    assert E % 64 and N_U % 32 and N_I % 32 and deg[1] > 128  # item 1's row straddles chunks
    before = g.clone()
    free = UNTOUCHED[ntype]
    free_coo, free_csr = g._coo[free], g._csr.get(free)
    assert g.remove_nodes(dev(np.asarray(RM[ntype], np.int64)), ntype=ntype) is None
    e2, n2, nd2, ed2, _ = rc.np_remove(edges, NUM, nd, ed, ntype, RM[ntype])
    rc.assert_graph(g, e2, n2, nd2, ed2, csr_cached=cached)
    _assert_equals_fresh(g, e2, n2)
    assert g._coo[free][0] is free_coo[0] and g._coo[free][1] is free_coo[1]
    if cached:
        assert g._csr[free] is free_csr
    assert BUYS not in g._out_csr and BUYS not in g._edge_rec
    rel = g.rel_graph(BUYS)  # rebuilt for the new numbering
    assert torch.equal(rel.edata["t"], g.edges[BUYS].data["t"][rel.eids])
    rc.assert_graph(before, edges, NUM, nd, ed, csr_cached=cached)  # the clone is unaffected
    # a second removal in the NEW numbering, then a node without edges alone (no edge goes)
    rm2 = [2, n2[ntype] - 2, 2, 40]
    g.remove_nodes(rm2, ntype=ntype)
    e3, n3, nd3, ed3, _ = rc.np_remove(e2, n2, nd2, ed2, ntype, rm2)
    rc.assert_graph(g, e3, n3, nd3, ed3)
    lonely = n3[ntype] - 1  # the old node N - 2
    for ce, (s, d) in e3.items():
        assert not (ce[0] == ntype and (s == lonely).any()), ce
        assert not (ce[2] == ntype and (d == lonely).any()), ce
    g.remove_nodes([lonely], ntype=ntype)
    e4, n4, nd4, ed4, kept_e = rc.np_remove(e3, n3, nd3, ed3, ntype, [lonely])
    assert all(len(kept_e[ce]) == len(e3[ce][0]) for ce in e3)
    rc.assert_graph(g, e4, n4, nd4, ed4)
    _assert_equals_fresh(g, e4, n4)
    # the empty list, then every node of the type
    coo = g._coo[BUYS]
    g.remove_nodes(torch.empty(0, dtype=torch.int64, device=DEV), ntype=ntype)
    assert g._coo[BUYS] is coo
    g.remove_nodes(np.arange(n4[ntype]), ntype=ntype)
    e5, n5, nd5, ed5, _ = rc.np_remove(e4, n4, nd4, ed4, ntype, np.arange(n4[ntype]))
    assert n5[ntype] == 0 and len(e5[BUYS][0]) == 0
    rc.assert_graph(g, e5, n5, nd5, ed5)
    assert g.edges[BUYS].data["t"].shape == (0, 2) and g.nodes[ntype].data["f"].shape == (0, 3)


def test_an_empty_relation_and_host_device_agreement():
    g, edges, nd, ed = _setup(True, e_similar=0)
    host = rc.build_graph(edges, NUM, nd, ed)
    for ce in rc.RELS:
        host.in_csr(ce)
    assert g.num_edges(SIMILAR) == 0
    for graph in (g, host):
        graph.remove_nodes(RM["item"], ntype="item")
    e2, n2, nd2, ed2, _ = rc.np_remove(edges, NUM, nd, ed, "item", RM["item"])
    rc.assert_graph(g, e2, n2, nd2, ed2, csr_cached=True)
    assert g._csr[SIMILAR][0].shape == (n2["item"] + 1,) and not g._csr[SIMILAR][0].any()
    for ce in rc.RELS:  # the host graph and the device graph agree
        for a, b in zip(g._csr[ce] + g._coo[ce], host._csr[ce] + host._coo[ce]):
            assert a.dtype == b.dtype and torch.equal(a.cpu(), b)
        for k in ("w", "t"):
            assert torch.equal(g.edges[ce].data[k].cpu(), host.edges[ce].data[k])
    for k in ("f", "c"):
        assert torch.equal(g.nodes["item"].data[k].cpu(), host.nodes["item"].data[k])


@pytest.mark.parametrize("bad", [[3, N_I], [-1], [2 ** 40]])
def test_a_bad_id_raises_and_changes_nothing(bad):
    # safe to run: gnnrec_node_rank_table compares every id with [0, N) before it forms the
    # bitmap word's address, and the graph launches nothing else before it has read the flag
    g, edges, nd, ed = _setup(True)
    coo, csr = dict(g._coo), dict(g._csr)
    f = g.nodes["item"].data["f"]
    with pytest.raises(ValueError, match="outside"):
        g.remove_nodes(bad, ntype="item")
    for ce in rc.RELS:
        assert g._coo[ce] is coo[ce] and g._csr[ce] is csr[ce]
    assert g.nodes["item"].data["f"] is f and BUYS in g._out_csr
    rc.assert_graph(g, edges, NUM, nd, ed, csr_cached=True)


# ---- the two ops on one relation ------------------------------------------------------------
def _reference(src, dst, n_src, n_dst, rm_src, rm_dst):
    """The filtered, relabelled COO by torch ops and its CSR by the library's sort."""
    from gnnrec import ops
    keep = torch.ones_like(src, dtype=torch.bool)
    n_new = n_dst
    if rm_src is not None:
        ks = torch.ones(n_src, dtype=torch.bool, device=DEV)
        ks[rm_src] = False
        keep &= ks[src]
    if rm_dst is not None:
        kd = torch.ones(n_dst, dtype=torch.bool, device=DEV)
        kd[rm_dst] = False
        keep &= kd[dst]
        n_new = int(kd.sum())
    kept = torch.nonzero(keep).reshape(-1)
    s2, d2 = src[kept], dst[kept]
    if rm_src is not None:
        s2 = (torch.cumsum(ks, 0) - 1)[s2]
    if rm_dst is not None:
        d2 = (torch.cumsum(kd, 0) - 1)[d2]
    return s2, d2, kept, ops.csr_build(s2.contiguous(), d2.contiguous(), n_new), n_new


def _run(src, dst, n_src, n_dst, rm_src, rm_dst, with_csr=True):
    from gnnrec import ops
    st = None if rm_src is None else ops.node_rank_table(rm_src, n_src)
    dt = None if rm_dst is None else ops.node_rank_table(rm_dst, n_dst)
    s2, d2, kept, csr2, n_new = _reference(src, dst, n_src, n_dst, rm_src, rm_dst)
    if dt is not None:
        assert dt[2].numel() == n_new
    csr = ops.csr_build(src, dst, n_dst) if with_csr else None
    got = ops.csr_remove_nodes(src, dst, csr, None if st is None else st[1],
                               None if dt is None else dt[1], n_src, n_dst, n_new)
    for name, a, b in zip(("src", "dst", "kept_eids"), got[:3], (s2, d2, kept)):
        assert a.dtype == b.dtype and torch.equal(a, b), name
    if not with_csr:
        assert got[3] is None
        return
    for name, a, b in zip(("indptr", "indices", "eids"), got[3], csr2):
        assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b), name


def _relation(n_src, n_dst, e, seed):
    g = torch.Generator().manual_seed(seed)
    src = torch.randint(0, n_src, (e,), generator=g)
    dst = torch.randint(0, n_dst, (e,), generator=g)
    dst[::3] = 1  # a heavy row
    return src.to(DEV), dst.to(DEV)


def test_node_rank_table_against_the_restatement():
    from gnnrec import ops
    for n, rm in ((1, [0]), (31, [30, 0]), (32, [31]), (33, [32, 32, 0]), (77, RM["item"]),
                  (300, RM["user"]), (64, list(range(64))), (70, []), (0, [])):
        removed, table, kept = ops.node_rank_table(dev(np.asarray(rm, np.int64)), n)
        keep = np.ones(n, bool)
        keep[rm] = False
        W = (n + 31) // 32
        bits = np.zeros(W * 32, bool)
        bits[:n] = ~keep
        words = (bits.reshape(W, 32) * (1 << np.arange(32, dtype=np.int64))).sum(1)
        np.testing.assert_array_equal(removed.cpu().numpy().view(np.uint32), words, str(n))
        rank = np.concatenate([[0], np.cumsum(np.pad(keep, (0, W * 32 - n)).reshape(W, 32).sum(1))])
        want = np.concatenate([(rank[:-1] << 32) | words, rank[-1:]]).astype(np.int64)
        np.testing.assert_array_equal(table.cpu().numpy(), want, str(n))
        np.testing.assert_array_equal(kept.cpu().numpy(), np.flatnonzero(keep), str(n))
    # safe to run: every id is compared with [0, N) before it is used as an index
    for bad in ([70], [-1], [3, 1 << 40]):
        with pytest.raises(ValueError, match="outside"):
            ops.node_rank_table(dev(np.asarray(bad, np.int64)), 70)


@pytest.mark.parametrize("side", ["src", "dst", "both"])
@pytest.mark.parametrize("e", [0, 1, 63, 64, 65, 3001])
def test_csr_remove_nodes_by_side(side, e):
    n_src, n_dst = (77, 77) if side == "both" else (300, 77)
    src, dst = _relation(n_src, n_dst, e, e)
    rm = dev(np.asarray(RM["item"] if side != "src" else RM["user"], np.int64))
    _run(src, dst, n_src, n_dst, rm if side != "dst" else None, rm if side != "src" else None)
    # nothing removed: the relation comes back as it is
    none = torch.empty(0, dtype=torch.int64, device=DEV)
    _run(src, dst, n_src, n_dst, none if side != "dst" else None, none if side != "src" else None)
    # everything removed
    every = torch.arange(n_dst if side != "src" else n_src, device=DEV)
    _run(src, dst, n_src, n_dst, every if side != "dst" else None,
         every if side != "src" else None)


def test_csr_remove_nodes_without_a_csr():
    src, dst = _relation(300, 77, 3001, 9)
    rm_u, rm_i = (dev(np.asarray(RM[k], np.int64)) for k in ("user", "item"))
    _run(src, dst, 300, 77, rm_u, None, with_csr=False)
    _run(src, dst, 300, 77, None, rm_i, with_csr=False)
    _run(src, dst, 300, 77, rm_u, rm_i, with_csr=False)  # two tables of two types


def test_csr_remove_nodes_past_the_flat_grid():
    """E = 2^21 + 321 edge ids: more than the 8192 blocks x 256 threads of the flat grid, so
    the grid-stride loops of every kernel take a second turn."""
    n_src, n_dst, e = 5003, 3001, (1 << 21) + 321
    src, dst = _relation(n_src, n_dst, e, 2)
    g = torch.Generator().manual_seed(4)
    rm_s = torch.randint(0, n_src, (500,), generator=g).to(DEV)
    rm_d = torch.randint(0, n_dst, (300,), generator=g).to(DEV)
    _run(src, dst, n_src, n_dst, rm_s, rm_d)


def test_an_endpoint_out_of_range_is_flagged_not_probed():
    # safe to run: edge_mark compares both endpoints with the node counts before it probes a
    # table, and every later kernel returns at once when the flag is set
    from gnnrec import ops
    src, dst = _relation(300, 77, 200, 1)
    src[17] = 300
    table = ops.node_rank_table(dev(np.asarray([3], np.int64)), 300)[1]
    with pytest.raises(ValueError, match="endpoint"):
        ops.csr_remove_nodes(src, dst, None, table, None, 300, 77, 77)
