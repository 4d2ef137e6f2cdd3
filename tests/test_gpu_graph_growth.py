"""Graph growth on the device (csrc/csr_merge.hip -> ops.csr_add_edges ->
HeteroGraph.add_edges / add_nodes) and what is built on it: the kernel against a rebuild of
the concatenated COO, bit for bit; a bad id writes nothing; a device graph against its host
twin and a fresh graph through one add / remove sequence; add then remove gives the starting
graph back; sampler blocks, full-graph embeddings and recommendations of a grown graph equal
those of a graph built from scratch; a clone taken before is unaffected."""
import numpy as np
import pytest
import torch

from split_cases import BOUGHT, BUYS, CLICKED, CLICKS

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

TILE = 512  # old slots per wave-tile of the shifted copy (csr_merge.hip kTile)
# wave (64), scan-tile (4096) and copy-tile boundaries, and many tiles
SIZES = [0, 1, 63, 64, 65, TILE - 1, TILE, TILE + 1, 4095, 4096, 4097, 2 * 4096 * 32 + 5]
BATCHES = [0, 1, 64, 65, 5000]
ROWS = [1, 7, 1000]  # one huge row; rows straddling tiles; mostly empty rows
N_SRC = 5000


def _base_dst(E, n_dst, rng):
    """Old destinations; with three rows or more, the rows r % 3 == 1 stay empty."""
    d = rng.integers(0, n_dst, E)
    if n_dst >= 3:
        d = np.where(d % 3 == 1, d - 1, d)
    return d


def _patterns(E, n, n_dst, src, dst, rng):
    """name -> (src_new, dst_new) as numpy int64."""
    if n == 0:
        z = np.empty(0, dtype=np.int64)
        return {"empty": (z, z)}
    s = rng.integers(0, N_SRC, n)
    p = {"row 0": (s, np.zeros(n, dtype=np.int64)),
         "last row": (s, np.full(n, n_dst - 1, dtype=np.int64)),
         "random": (s, rng.integers(0, n_dst, n))}
    if n_dst >= 3:
        empty = np.arange(1, n_dst, 3)
        p["empty rows"] = (s, empty[rng.integers(0, empty.size, n)])
    elif E == 0:  # (a single row is empty only in an empty relation)
        p["empty rows"] = (s, np.zeros(n, dtype=np.int64))
    if E:
        pick = rng.integers(0, E, n)
        p["duplicates"] = (src[pick], dst[pick])
    return p


@pytest.mark.parametrize("E", SIZES)
def test_kernel_equals_rebuild_bitwise(E):
    from gnnrec import ops
    rng = np.random.default_rng(E + 1)
    for n_dst in ROWS:
        src_h, dst_h = rng.integers(0, N_SRC, E), _base_dst(E, n_dst, rng)
        src, dst = torch.from_numpy(src_h).to(DEV), torch.from_numpy(dst_h).to(DEV)
        csr = ops.csr_build(src, dst, n_dst)
        cases = {}
        for n in BATCHES:
            for name, b in _patterns(E, n, n_dst, src_h, dst_h, rng).items():
                cases[f"n={n} {name}"] = b
        cases["every row once"] = (rng.integers(0, N_SRC, n_dst), rng.permutation(n_dst))
        for name, (u_h, v_h) in cases.items():
            u, v = torch.from_numpy(u_h).to(DEV), torch.from_numpy(v_h).to(DEV)
            want = ops.csr_build(torch.cat([src, u]), torch.cat([dst, v]), n_dst)
            got = ops.csr_add_edges(csr, u, v, N_SRC, n_dst)
            what = f"E={E} n_dst={n_dst} {name}"
            for g, w in zip(got, want):
                assert g.dtype == w.dtype and g.shape == w.shape and torch.equal(g, w), what
            assert got[0]._gnnrec_nnz == E + u.numel(), what


@pytest.mark.parametrize("E", [0, 65, 4097])
@pytest.mark.parametrize("bad", [("src", N_SRC), ("dst", -1), ("dst", 1 << 40)])
def test_bad_id_sets_the_flag_and_writes_nothing(E, bad):
    # safe to run: validate_batch_kernel is the entry's first launch, the batch's CSR build and
    # splice_points_kernel read only its clamped copy, and every kernel that writes an output
    # returns when status[1] is set (csr_merge.hip)
    from gnnrec import ops
    T = ops._T()
    n_dst, n = 7, 70
    src = torch.arange(E, dtype=torch.int64, device=DEV)
    dst = src % n_dst
    csr = ops.csr_build(src, dst, n_dst)
    u = torch.arange(n, dtype=torch.int64, device=DEV)
    v = u % n_dst
    (u if bad[0] == "src" else v)[n // 2] = bad[1]
    outs = [torch.full((n_dst + 1,), -7, dtype=torch.int64, device=DEV),
            torch.full((E + n,), -7, dtype=torch.int32, device=DEV),
            torch.full((E + n,), -7, dtype=torch.int64, device=DEV)]
    status = torch.full((2,), -7, dtype=torch.int64, device=DEV)
    ws = torch.empty(int(T.csr_add_edges_workspace_bytes(n, n_dst)), dtype=torch.uint8, device=DEV)
    T.csr_add_edges(*csr, u, v, N_SRC, n_dst, ws, *outs, status)
    total, flag = status.tolist()
    assert flag != 0 and total == E
    assert all(bool((o == -7).all()) for o in outs)
    with pytest.raises(ValueError, match="outside"):
        ops.csr_add_edges(csr, u, v, N_SRC, n_dst)


# ---- graph level: a device graph, its host twin and a fresh graph -------------------------
N_U, N_I = 120, 40


def _twin_graphs():
    from gnnrec.graph import HeteroGraph
    rng = np.random.default_rng(9)
    bu, bi = rng.integers(0, N_U, 900), rng.integers(0, N_I - 3, 900)
    cu, ci = rng.integers(0, N_U, 1500), rng.integers(0, N_I, 1500)
    edges = {BUYS: (bu, bi), BOUGHT: (bi, bu), CLICKS: (cu, ci), CLICKED: (ci, cu)}
    host = HeteroGraph({ce: (torch.from_numpy(s.astype(np.int64)), torch.from_numpy(d.astype(np.int64)))
                        for ce, (s, d) in edges.items()}, {"user": N_U, "item": N_I})
    for ce, (s, _d) in edges.items():
        host.edges[ce].data["occurrence"] = torch.from_numpy(rng.integers(1, 9, s.size))
        host.edges[ce].data["w"] = torch.from_numpy(
            rng.standard_normal((s.size, 3)).astype(np.float32))
    host.nodes["user"].data["features"] = torch.from_numpy(
        rng.standard_normal((N_U, 5)).astype(np.float32))
    host.nodes["item"].data["features"] = torch.from_numpy(
        rng.standard_normal((N_I, 6)).astype(np.float32))
    return host, host.to(DEV)


def _fresh(g):
    """A new device graph from g's whole COO, node counts and frames."""
    from gnnrec.graph import HeteroGraph
    f = HeteroGraph({ce: tuple(t.to(DEV) for t in g.all_edges(etype=ce))
                     for ce in g.canonical_etypes}, {nt: g.num_nodes(nt) for nt in g.ntypes},
                    device=DEV)
    for ce in g.canonical_etypes:
        for k, v in g._edata[ce].items():
            f.edges[ce].data[k] = v.to(DEV)
    for nt in g.ntypes:
        for k, v in g._ndata[nt].items():
            f.nodes[nt].data[k] = v.to(DEV)
    return f


def _eq(a, b, what):
    assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.cpu(), b.cpu()), what


def _same_graph(dev_g, other, what):
    """COO, both CSRs and every frame of dev_g equal other's (a host or a device graph).
    Clones answer, so that no cache of either graph is built by the comparison."""
    a_g, b_g = dev_g.clone(), other.clone()
    assert a_g.canonical_etypes == b_g.canonical_etypes
    for nt in b_g.ntypes:
        assert a_g.num_nodes(nt) == b_g.num_nodes(nt), (what, nt)
        assert set(a_g._ndata[nt].keys()) == set(b_g._ndata[nt].keys()), (what, nt)
        for k, v in b_g._ndata[nt].items():
            _eq(a_g._ndata[nt][k], v, (what, nt, k))
    for ce in b_g.canonical_etypes:
        assert a_g.num_edges(ce) == b_g.num_edges(ce), (what, ce)
        for a, b in zip(a_g.all_edges(etype=ce), b_g.all_edges(etype=ce)):
            _eq(a, b, (what, ce, "coo"))
        for a, b in zip(a_g.in_csr(ce), b_g.in_csr(ce)):
            _eq(a, b, (what, ce, "in_csr"))
        for a, b in zip(a_g.out_csr(ce), b_g.out_csr(ce)):
            _eq(a, b, (what, ce, "out_csr"))
        assert set(a_g._edata[ce].keys()) == set(b_g._edata[ce].keys()), (what, ce)
        for k, v in b_g._edata[ce].items():
            _eq(a_g._edata[ce][k], v, (what, ce, k))


def _warm(dev):
    dev.in_csr(BUYS), dev.in_csr(BOUGHT), dev.out_csr(BUYS)
    dev.rel_graph(BUYS), dev.edge_records(BUYS), dev.edge_records(BOUGHT)
    s, d = dev.all_edges(etype=BUYS)
    assert bool(dev.has_edges_between(s[:1], d[:1], etype=BUYS)[0])
    assert bool(dev.has_edges_between(d[:1], s[:1], etype=BOUGHT)[0])


def test_device_graph_follows_its_host_twin():
    host, dev = _twin_graphs()
    _warm(dev)
    host.in_csr(BUYS), host.in_csr(BOUGHT), host.out_csr(BUYS)
    rng = np.random.default_rng(4)
    old_u, old_i = (t.clone() for t in host.all_edges(etype=BUYS))
    new_user = N_U + 2
    pairs_u = torch.cat([old_u[:50], torch.tensor([new_user, new_user, N_U, 3])])
    pairs_i = torch.cat([old_i[:50], torch.tensor([N_I + 1, 0, N_I, N_I - 1])])

    def check(what):
        assert BUYS in dev._csr and BOUGHT in dev._csr and BUYS in dev._out_csr, what
        assert BOUGHT not in dev._out_csr and CLICKS not in dev._csr, what  # stay unbuilt
        assert dev.in_csr(BUYS)[0]._gnnrec_nnz == dev.num_edges(BUYS), what
        assert dev.out_csr(BUYS)[0]._gnnrec_nnz == dev.num_edges(BUYS), what
        _same_graph(dev, host, what + " / host")
        fresh = _fresh(host)
        _same_graph(dev, fresh, what + " / fresh")
        want = host.has_edges_between(pairs_u, pairs_i, etype=BUYS)
        _eq(dev.has_edges_between(pairs_u.to(DEV), pairs_i.to(DEV), etype=BUYS), want, what)
        _eq(fresh.has_edges_between(pairs_u.to(DEV), pairs_i.to(DEV), etype=BUYS), want, what)
        _eq(dev.has_edges_between(pairs_i.to(DEV), pairs_u.to(DEV), etype=BOUGHT),
            host.has_edges_between(pairs_i, pairs_u, etype=BOUGHT), what)
        if dev.num_nodes("user") > new_user:
            nodes = torch.tensor([new_user, 3, new_user])
            for a, b, c in zip(dev.out_edges(nodes.to(DEV), form="all", etype=BUYS),
                               host.out_edges(nodes, form="all", etype=BUYS),
                               fresh.out_edges(nodes.to(DEV), form="all", etype=BUYS)):
                _eq(a, b, what + " out_edges")
                _eq(a, c, what + " out_edges fresh")
            for ce in (BUYS, BOUGHT):
                _eq(dev.clone().edge_records(ce), fresh.edge_records(ce), what)
        return want

    def both(fn):
        fn(host, lambda t: t)
        fn(dev, lambda t: t.to(DEV) if torch.is_tensor(t) else t)

    feats = torch.from_numpy(rng.standard_normal((4, 5)).astype(np.float32))
    both(lambda g, mv: g.add_nodes(4, {"features": mv(feats)}, ntype="user"))
    both(lambda g, mv: g.add_nodes(3, ntype="item"))  # zero rows
    assert dev.num_nodes("user") == N_U + 4 and dev.num_nodes("item") == N_I + 3
    check("after add_nodes")

    n = 300
    u = torch.from_numpy(rng.integers(0, N_U + 4, n))
    i = torch.from_numpy(rng.integers(0, N_I + 3, n))
    i[((u == N_U) & (i == N_I)) | ((u == 3) & (i == N_I - 1))] = 0  # pairs asked for as absent
    u[0], i[0] = new_user, N_I + 1          # a new user buys a new item
    u[1], i[1] = new_user, 0                # and an old one
    u[2], i[2] = old_u[7], old_i[7]         # a duplicate of an old edge
    occ = torch.from_numpy(rng.integers(1, 9, n))
    w = torch.from_numpy(rng.standard_normal((n, 3)).astype(np.float32))
    both(lambda g, mv: g.add_edges(mv(u), mv(i), {"occurrence": mv(occ)}, etype=BUYS))
    both(lambda g, mv: g.add_edges(mv(i), mv(u), {"w": mv(w)}, etype=BOUGHT))
    assert dev.num_edges(BUYS) == 900 + n == dev.num_edges(BOUGHT)
    got = check("after add_edges")
    assert got[50:].tolist() == [True, True, False, False]
    E = 900
    _eq(dev.edges[BUYS].data["occurrence"][E:], occ, "given rows")
    assert not bool(dev.edges[BUYS].data["w"][E:].any())          # zero fill
    assert not bool(dev.edges[BOUGHT].data["occurrence"][E:].any())

    rm = torch.from_numpy(np.concatenate([rng.permutation(900)[:200], [901], 905 + np.arange(100)]))
    both(lambda g, mv: g.remove_edges(mv(rm), etype=BUYS))
    both(lambda g, mv: g.remove_edges(mv(rm), etype=BOUGHT))
    dev.out_csr(BUYS), host.out_csr(BUYS)  # (remove_edges drops the source-major CSR)
    check("after remove_edges")

    u2 = torch.from_numpy(rng.integers(0, N_U + 4, 70))
    i2 = torch.from_numpy(rng.integers(0, N_I + 3, 70))
    fresh_field = torch.arange(70, dtype=torch.float32)
    both(lambda g, mv: g.add_edges(mv(u2), mv(i2), {"recency": mv(fresh_field)}, etype="buys"))
    both(lambda g, mv: g.add_edges(i2.tolist(), u2.tolist(), etype=BOUGHT))
    check("after the second add_edges")
    assert not bool(dev.edges[BUYS].data["recency"][:-70].any())  # a new field: zeros before
    assert "recency" not in dev.edges[BOUGHT].data

    # a bad id leaves the device graph as it was, cached CSRs or not
    before = (dev.all_edges(etype=BUYS), dev.in_csr(BUYS), dev.out_csr(BUYS))
    for ce, uu, vv in ((BUYS, [0, N_U + 4], [0, 0]), (BUYS, [0], [-1]), (CLICKS, [0], [N_I + 3])):
        with pytest.raises(ValueError, match="outside"):
            dev.add_edges(uu, vv, etype=ce)
    assert dev.in_csr(BUYS) is before[1] and dev.out_csr(BUYS) is before[2]
    assert all(a is b for a, b in zip(dev.all_edges(etype=BUYS), before[0]))
    check("after the refused batches")
    # an empty batch changes nothing
    dev.add_edges(torch.empty(0, dtype=torch.int64, device=DEV), [], etype=BUYS)
    assert dev.in_csr(BUYS) is before[1]


def test_add_then_remove_gives_the_starting_graph():
    _host, start = _twin_graphs()
    _warm(start)
    g = start.clone()
    rng = np.random.default_rng(2)
    n = 257
    u = torch.from_numpy(rng.integers(0, N_U, n)).to(DEV)
    i = torch.from_numpy(rng.integers(0, N_I, n)).to(DEV)
    g.add_edges(u, i, {"occurrence": torch.full((n,), 3, device=DEV)}, etype=BUYS)
    g.add_edges(i, u, etype=BOUGHT)
    assert g.num_edges(BUYS) == 900 + n
    added = torch.arange(900, 900 + n, device=DEV)
    g.remove_edges(added, etype=BUYS)
    g.remove_edges(added, etype=BOUGHT)
    assert BUYS in g._csr and BOUGHT in g._csr  # the cached CSRs went through both kernels
    _same_graph(g, start, "round trip")


@pytest.mark.parametrize("share", [None, 0.0, float("inf")])
def test_every_batch_share_gives_the_same_graph(share, monkeypatch):
    """A batch larger than the relation (above graph.ADD_EDGES_REBUILD_SHARE the cached CSRs are
    rebuilt, below it merged), into a relation with edges and into an empty one; then with the
    rebuild and the merge forced."""
    from gnnrec import graph as graph_mod
    from gnnrec.graph import HeteroGraph
    if share is not None:
        monkeypatch.setattr(graph_mod, "ADD_EDGES_REBUILD_SHARE", share)
    host, dev = _twin_graphs()
    _warm(dev)
    rng = np.random.default_rng(8)
    n = 1000
    u = torch.from_numpy(rng.integers(0, N_U, n))
    i = torch.from_numpy(rng.integers(0, N_I, n))
    for g, mv in ((host, lambda t: t), (dev, lambda t: t.to(DEV))):
        g.add_edges(mv(u), mv(i), etype=BUYS)
        g.add_edges(mv(i), mv(u), etype=BOUGHT)
    assert BUYS in dev._csr and BUYS in dev._out_csr and BOUGHT not in dev._out_csr
    _same_graph(dev, host, f"share={share}")
    _same_graph(dev, _fresh(host), f"share={share} / fresh")
    with pytest.raises(ValueError, match="outside"):
        dev.add_edges(u.to(DEV), (i + N_I).to(DEV), etype=BUYS)
    empty = HeteroGraph({BUYS: ([], [])}, {"user": N_U, "item": N_I}, device=DEV)
    empty.in_csr(BUYS), empty.out_csr(BUYS)
    empty.add_edges(u[:1].to(DEV), i[:1].to(DEV))
    empty.add_edges(u[1:].to(DEV), i[1:].to(DEV))
    _same_graph(empty, HeteroGraph({BUYS: (u, i)}, {"user": N_U, "item": N_I}), "from empty")


def test_grown_graph_serves_like_one_built_from_scratch():
    from gnnrec import nn as gnn
    from gnnrec.graph import NID
    from gnnrec.inference import full_graph_embeddings
    from gnnrec.recs import recommend_for_graph
    from gnnrec.sampling import MultiLayerFullNeighborSampler
    _host, grown = _twin_graphs()
    for ce in grown.canonical_etypes:
        grown.in_csr(ce)
    rng = np.random.default_rng(6)
    grown.add_nodes(2, {"features": torch.ones(2, 5, device=DEV)}, ntype="user")
    n = 200
    u = torch.from_numpy(rng.integers(0, N_U + 2, n)).to(DEV)
    i = torch.from_numpy(rng.integers(0, N_I, n)).to(DEV)
    u[:3] = N_U + 1
    grown.add_edges(u, i, etype=BUYS)
    grown.add_edges(i, u, etype=BOUGHT)
    grown.add_edges(u[:50], i[50:100], etype=CLICKS)
    grown.add_edges(i[50:100], u[:50], etype=CLICKED)
    scratch = _fresh(grown)
    assert all(ce in grown._csr for ce in grown.canonical_etypes) and not scratch._csr

    seeds = {"user": torch.tensor([3, 7, N_U + 1], device=DEV), "item": torch.tensor([0, 39], device=DEV)}
    blocks = [MultiLayerFullNeighborSampler(2).sample_blocks(g, seeds) for g in (grown, scratch)]
    for b_a, b_b in zip(*blocks):
        for nt in b_b.ntypes:
            assert torch.equal(b_a.srcdata[NID][nt], b_b.srcdata[NID][nt])
        for ce in b_b.canonical_etypes:
            for a, b in zip(b_a._rels[ce], b_b._rels[ce]):
                assert torch.equal(a, b), ce
            for k in ("occurrence", "w"):
                assert torch.equal(b_a._edata[ce][k], b_b._edata[ce][k]), (ce, k)

    torch.manual_seed(0)
    model = gnn.ConvModel(scratch, 2, {"user": 5, "item": 6, "hidden": 16, "out": 8}, True, 0.0,
                          "mean", "cos", "sum", True).to(DEV).eval()
    with torch.no_grad():
        h_a, h_b = (full_graph_embeddings(g, model) for g in (grown, scratch))
    for nt in h_b:
        assert h_a[nt].shape == (grown.num_nodes(nt), 8) and torch.equal(h_a[nt], h_b[nt]), nt

    k = 5
    idx_a, val_a = recommend_for_graph(grown, h_a, k)
    idx_b, val_b = recommend_for_graph(scratch, h_b, k)
    assert torch.equal(idx_a, idx_b) and torch.equal(val_a, val_b)
    assert idx_a.shape == (N_U + 2, k)
    lists = idx_a[u]                                  # [n, k]: the list of each added edge's user
    assert not bool((lists == i[:, None]).any())      # never the item bought in the batch
    assert bool((idx_a >= 0).any())


def test_clone_taken_before_the_growth_keeps_the_old_graph():
    host, dev = _twin_graphs()
    _warm(dev)
    csr, ocsr = dev.in_csr(BUYS), dev.out_csr(BUYS)
    c = dev.clone()
    dev.add_nodes(5, ntype="item")
    dev.add_edges([0, 1, 2], [N_I + 4, 0, 1], {"occurrence": torch.tensor([1, 2, 3])}, etype=BUYS)
    assert dev.num_edges(BUYS) == 903 and dev.num_nodes("item") == N_I + 5
    assert c.num_edges(BUYS) == 900 and c.num_nodes("item") == N_I
    assert c.in_csr(BUYS) is csr and c.out_csr(BUYS) is ocsr
    assert c.nodes["item"].data["features"].shape[0] == N_I
    assert not bool(c.has_edges_between(torch.tensor([0], device=DEV),
                                        torch.tensor([N_I + 4], device=DEV), etype=BUYS)[0])
    _same_graph(c, host, "the clone")
    # and the other way round: growing a clone leaves the original
    c2 = dev.clone()
    c2.add_edges([5], [5], etype=BUYS)
    assert dev.num_edges(BUYS) == 903 and c2.num_edges(BUYS) == 904
