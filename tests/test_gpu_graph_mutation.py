"""Edge removal on the device (csrc/csr_filter.hip -> ops.csr_remove_edges ->
HeteroGraph.remove_edges) and what is built on it: the kernel against a rebuild of the masked
COO, bit for bit; a device graph against its host twin through one removal sequence;
train_valid_split(device_out=True) against the reference's fixtures; one batch of each loader
of generate_dataloaders through a one-layer ConvModel."""
import types

import numpy as np
import pytest
import torch

import split_cases as sc

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
BUYS, BOUGHT, CLICKS, CLICKED = sc.BUYS, sc.BOUGHT, sc.CLICKS, sc.CLICKED

# word (32), ballot (64) and scan-tile (4096) boundaries, and more than one scan tile of words
SIZES = [0, 1, 31, 32, 33, 63, 64, 65, 4095, 4096, 4097, 2 * 4096 * 32 + 5]
ROWS = [1, 7, 1000]  # one huge row; rows straddling 64-slot chunks; mostly empty rows


def _removal_lists(E, dst, rng):
    ids = torch.arange(E, dtype=torch.int64)
    row = ids[dst == dst[E // 2]] if E else ids
    tenth = torch.from_numpy(rng.permutation(E)[:max(1, E // 10) if E else 0])
    twice = torch.cat([tenth, tenth])[torch.from_numpy(rng.permutation(2 * tenth.numel()))]
    return {"empty": ids[:0], "all": ids, "every other": ids[::2], "one row": row,
            "last fifth": ids[int(E * 0.8):], "random tenth twice": twice}


@pytest.mark.parametrize("E", SIZES)
def test_kernel_equals_rebuild_bitwise(E):
    from gnnrec import ops
    rng = np.random.default_rng(E + 1)
    for n_dst in ROWS:
        src = torch.from_numpy(rng.integers(0, 5000, E)).to(DEV)
        dst_h = torch.from_numpy(rng.integers(0, n_dst, E))
        dst = dst_h.to(DEV)
        csr = ops.csr_build(src, dst, n_dst)
        for name, rm in _removal_lists(E, dst_h, rng).items():
            keep = torch.ones(E, dtype=torch.bool)
            keep[rm] = False
            keep = keep.to(DEV)
            want_s, want_d = src[keep], dst[keep]
            want = ops.csr_build(want_s, want_d, n_dst)
            s2, d2, kept, csr2 = ops.csr_remove_edges(src, dst, rm.to(DEV), csr)
            what = f"E={E} n_dst={n_dst} list={name}"
            assert s2.numel() == int(keep.sum()), what  # E'
            assert torch.equal(s2, want_s) and torch.equal(d2, want_d), what
            assert torch.equal(kept, torch.nonzero(keep).reshape(-1)), what
            for got, w in zip(csr2, want):
                assert got.dtype == w.dtype and torch.equal(got, w), what
            assert csr2[0]._gnnrec_nnz == s2.numel()
            # the COO alone (no CSR cached): the same COO
            s3, d3, kept3, none = ops.csr_remove_edges(src, dst, rm.to(DEV))
            assert none is None and torch.equal(s3, want_s) and torch.equal(d3, want_d), what
            assert torch.equal(kept3, kept), what


@pytest.mark.parametrize("E,rm", [(0, [0]), (65, [3, 65, 4]), (65, [-1]), (4097, [4096, 1 << 40])])
def test_bad_id_sets_the_flag_and_writes_nothing(E, rm):
    from gnnrec import ops
    T = ops._T()
    n_dst = 7
    src = torch.arange(E, dtype=torch.int64, device=DEV)
    dst = src % n_dst
    csr = ops.csr_build(src, dst, n_dst)
    rm = torch.tensor(rm, dtype=torch.int64, device=DEV)
    outs = [torch.full((E,), -7, dtype=torch.int64, device=DEV) for _ in range(3)]
    outs += [torch.full((n_dst + 1,), -7, dtype=torch.int64, device=DEV),
             torch.full((E,), -7, dtype=torch.int32, device=DEV),
             torch.full((E,), -7, dtype=torch.int64, device=DEV)]
    status = torch.full((2,), -7, dtype=torch.int64, device=DEV)
    ws = torch.empty(int(T.csr_remove_edges_workspace_bytes(E, n_dst)), dtype=torch.uint8,
                     device=DEV)
    T.csr_remove_edges(src, dst, *csr, rm, ws, *outs, status)
    n_new, bad = status.tolist()
    assert bad != 0 and n_new == E
    assert all(bool((o == -7).all()) for o in outs)
    with pytest.raises(ValueError, match="outside"):
        ops.csr_remove_edges(src, dst, rm, csr)


# ---- graph level: a device graph and its host twin ---------------------------------------
N_U, N_I = 120, 40


def _twin_graphs():
    from gnnrec.graph import HeteroGraph
    rng = np.random.default_rng(9)
    bu, bi = rng.integers(0, N_U, 900), rng.integers(0, N_I - 3, 900)
    bu[1], bi[1] = bu[0], bi[0]        # edge 1 duplicates edge 0: removing 0 leaves the pair
    bu[5], bi[5] = N_U - 1, N_I - 1    # the only edge of this pair
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


def _same_graph(dev_g, host_g):
    for ce in host_g.canonical_etypes:
        for a, b in zip(dev_g.all_edges(etype=ce), host_g.all_edges(etype=ce)):
            assert torch.equal(a.cpu(), b), ce
        for a, b in zip(dev_g.in_csr(ce), host_g.in_csr(ce)):
            assert a.dtype == b.dtype and torch.equal(a.cpu(), b), ce
        for k, v in host_g._edata[ce].items():
            got = dev_g._edata[ce][k]
            assert got.dtype == v.dtype and torch.equal(got.cpu(), v), (ce, k)
    for nt in host_g.ntypes:
        for k, v in host_g._ndata[nt].items():
            assert torch.equal(dev_g._ndata[nt][k].cpu(), v)


def test_device_graph_follows_its_host_twin():
    from gnnrec.graph import HeteroGraph, NID
    from gnnrec.sampling import MultiLayerFullNeighborSampler
    host, dev = _twin_graphs()
    dev.in_csr(BUYS), dev.in_csr(CLICKS), dev.rel_graph(BUYS), dev.edge_records(BUYS)
    host.in_csr(BUYS)
    u, i = (t.clone() for t in host.all_edges(etype=BUYS))
    assert bool(dev.has_edges_between(u[:1].to(DEV), i[:1].to(DEV), etype=BUYS)[0])  # cached
    rng = np.random.default_rng(4)
    steps = [(BUYS, [0, 5, 899, 5, 450]),                    # CSR cached on both
             (BOUGHT, [0, 5, 899, 450]),                      # no CSR cached: the COO alone
             (CLICKS, np.arange(1200, 1500)),                 # the split's own pattern
             (CLICKED, np.arange(1200, 1500)),
             (BUYS, 1 + rng.permutation(894)[:300]),          # again, in the new numbering (0: the twin)
             (CLICKS, [])]
    for ce, rm in steps:
        rm = torch.as_tensor(np.asarray(rm, dtype=np.int64))
        host.remove_edges(rm, etype=ce)
        dev.remove_edges(rm.to(DEV), etype=ce)
        assert dev.num_edges(ce) == host.num_edges(ce)
    _same_graph(dev, host)
    # membership: removed pairs, kept pairs, and the pair whose duplicate survives
    got = dev.has_edges_between(u.to(DEV), i.to(DEV), etype=BUYS).cpu()
    want = host.has_edges_between(u, i, etype=BUYS)
    assert torch.equal(got, want)
    assert bool(got[0]) and bool(got[1]) and not bool(got[5])  # 0 removed, its twin 1 kept
    assert (~want).sum() > 100  # many pairs really left
    # range queries follow the new numbering too
    nodes = torch.tensor([3, 3, N_I - 1, 0])
    for a, b in zip(dev.in_edges(nodes.to(DEV), form="all", etype=BUYS),
                    host.in_edges(nodes, form="all", etype=BUYS)):
        assert torch.equal(a.cpu(), b)
    for a, b in zip(dev.out_edges(nodes.to(DEV), form="all", etype=CLICKS),
                    host.out_edges(nodes, form="all", etype=CLICKS)):
        assert torch.equal(a.cpu(), b)
    # edge records and a full-neighbour block equal those of a graph built from the survivors
    fresh = HeteroGraph({ce: host.all_edges(etype=ce) for ce in host.canonical_etypes},
                        {"user": N_U, "item": N_I}).to(DEV)
    for ce in host.canonical_etypes:
        for k, v in host._edata[ce].items():
            fresh.edges[ce].data[k] = v.to(DEV)
        assert torch.equal(dev.edge_records(ce), fresh.edge_records(ce)), ce
    for nt in host.ntypes:
        fresh.nodes[nt].data["features"] = host.nodes[nt].data["features"].to(DEV)
    seeds = {"user": torch.tensor([3, 7, 119], device=DEV), "item": torch.tensor([0, 39], device=DEV)}
    blocks = [MultiLayerFullNeighborSampler(2).sample_blocks(g, seeds) for g in (dev, fresh)]
    for b_dev, b_new in zip(*blocks):
        for nt in b_new.ntypes:
            assert torch.equal(b_dev.srcdata[NID][nt], b_new.srcdata[NID][nt])
        for ce in b_new.canonical_etypes:
            for a, b in zip(b_dev._rels[ce], b_new._rels[ce]):
                assert torch.equal(a, b), ce
            for k in ("occurrence", "w"):
                assert torch.equal(b_dev._edata[ce][k], b_new._edata[ce][k]), (ce, k)
    # a bad id leaves the device graph as it was
    before = dev.in_csr(BUYS)
    with pytest.raises(ValueError, match="outside"):
        dev.remove_edges(torch.tensor([0, dev.num_edges(BUYS)], device=DEV), etype=BUYS)
    assert dev.in_csr(BUYS) is before
    _same_graph(dev, host)


def test_clone_on_the_device_shares_and_separates():
    host, dev = _twin_graphs()
    csr = dev.in_csr(BUYS)
    c = dev.clone()
    assert c.in_csr(BUYS) is csr and c.device == dev.device
    c.remove_edges(torch.arange(100, device=DEV), etype=BUYS)
    assert dev.num_edges(BUYS) == 900 and dev.in_csr(BUYS) is csr and c.num_edges(BUYS) == 800
    host.remove_edges(torch.arange(100), etype=BUYS)
    _same_graph(c, host)


# ---- the split and the loaders ------------------------------------------------------------
def _split_graph():
    from gnnrec import create_graph
    edges, gt_test = sc.make_inputs()
    g = create_graph(edges, device=DEV, num_nodes_dict={"user": sc.N_USER, "item": sc.N_ITEM})
    return g, gt_test


def _np(x):
    if isinstance(x, dict):
        return {k: _np(v) for k, v in x.items()}
    if isinstance(x, tuple):
        return tuple(_np(v) for v in x)
    assert torch.is_tensor(x) and x.device == DEV and x.dtype == torch.int64
    return x.cpu().numpy()


@pytest.mark.parametrize("name", sorted(sc.CASES))
def test_split_on_the_device_equals_the_reference(name):
    from gnnrec import train_valid_split
    g, gt_test = _split_graph()
    g.in_csr(BUYS), g.in_csr(BOUGHT)  # cached: removed by the CSR compaction; clicks by the COO's
    res = train_valid_split(g, gt_test, device_out=True, **sc.split_kwargs(sc.CASES[name]))
    train_graph = res[0]
    assert train_graph.device == DEV
    flat = sc.flatten((train_graph,) + _np(tuple(res[1:])),
                      lambda tg, ce: tuple(t.cpu().numpy() for t in tg.all_edges(etype=ce)))
    sc.assert_matches(flat, sc.load_golden(name))
    from gnnrec import ops
    for ce in (BUYS, BOUGHT):  # the compacted CSRs are the rebuilt ones
        s, d = train_graph.all_edges(etype=ce)
        for a, b in zip(train_graph.in_csr(ce), ops.csr_build(s, d, train_graph.num_nodes(ce[2]))):
            assert torch.equal(a, b)


@pytest.mark.parametrize("remove_train_eids", [False, True])
def test_every_loader_feeds_a_one_layer_model(remove_train_eids):
    from gnnrec import generate_dataloaders, nn as gnn, train_valid_split
    g, gt_test = _split_graph()
    rng = np.random.default_rng(1)
    for nt, n, d in (("user", sc.N_USER, 5), ("item", sc.N_ITEM, 6)):
        g.nodes[nt].data["features"] = torch.from_numpy(
            rng.standard_normal((n, d)).astype(np.float32)).to(DEV)
    res = train_valid_split(g, gt_test, device_out=True,
                            **sc.split_kwargs((True, remove_train_eids, 1, 1)))
    fixed = types.SimpleNamespace(neighbor_sampler="full", remove_train_eids=remove_train_eids,
                                  edge_batch_size=256, node_batch_size=128)
    loaders = generate_dataloaders(g, *res[:7], fixed, 0, n_layers=2, neg_sample_size=5)
    torch.manual_seed(0)
    model = gnn.ConvModel(g, 2, {"user": 5, "item": 6, "hidden": 16, "out": 8}, True, 0.0,
                          "mean", "cos", "sum", True).to(DEV).eval()
    with torch.no_grad():
        for ld in loaders[:2]:
            _inputs, pos_g, neg_g, blocks = next(iter(ld))
            assert len(blocks) == 1
            h, ps, ns = model(blocks, blocks[0].srcdata["features"], pos_g, neg_g, True)
            for ce, p in ps.items():
                assert p.numel() * 5 == ns[ce].numel() and bool(torch.isfinite(p).all())
            assert sum(p.numel() for p in ps.values()) == 256
        for ld in loaders[2:]:
            _inputs, outputs, blocks = next(iter(ld))
            h = model.get_repr(blocks, model.embed(blocks[0].srcdata["features"]))
            assert sum(v.numel() for v in outputs.values()) == 128
            for nt, ids in outputs.items():
                assert h[nt].shape == (ids.numel(), 8) and bool(torch.isfinite(h[nt]).all())
    torch.cuda.synchronize()
