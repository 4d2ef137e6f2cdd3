"""HeteroGraph.clone / remove_edges / in_edges / out_edges on a graph in host memory against a
numpy restatement written here, gnnrec.sampling.train_valid_split against fixtures made by the
reference's own function (tests/golden/make_split_golden.py), and the loader wiring of
generate_dataloaders.  Nothing here touches a device."""
import types

import numpy as np
import pytest
import torch

import split_cases as sc
from gnnrec import create_graph, generate_dataloaders, io, sampling, train_valid_split
from gnnrec.graph import HeteroGraph

BUYS, BOUGHT = sc.BUYS, sc.BOUGHT
N_U, N_I, E = 23, 11, 157


def _edges(seed=3):
    rng = np.random.default_rng(seed)
    u, i = rng.integers(0, N_U, E), rng.integers(0, N_I - 2, E)  # the last items: empty rows
    return u.astype(np.int64), i.astype(np.int64)


def _graph():
    u, i = _edges()
    g = HeteroGraph({BUYS: (torch.from_numpy(u), torch.from_numpy(i)),
                     BOUGHT: (torch.from_numpy(i), torch.from_numpy(u))},
                    {"user": N_U, "item": N_I})
    g.edges["buys"].data["w"] = torch.arange(E, dtype=torch.float32) * 0.5
    g.edges["buys"].data["t"] = torch.arange(2 * E, dtype=torch.int32).reshape(E, 2)
    g.nodes["user"].data["f"] = torch.arange(N_U, dtype=torch.float32)
    return g, u, i


def _np_csr(src, dst, n_dst):
    order = np.argsort(dst, kind="stable")
    indptr = np.zeros(n_dst + 1, dtype=np.int64)
    np.cumsum(np.bincount(dst, minlength=n_dst), out=indptr[1:])
    return indptr, src[order].astype(np.int32), order.astype(np.int64)


def _assert_csr(g, ce, src, dst, n_dst):
    want = _np_csr(src, dst, n_dst)
    for got, w in zip(g.in_csr(ce), want):
        assert got.numpy().dtype == w.dtype
        np.testing.assert_array_equal(got.numpy(), w)


@pytest.mark.parametrize("cached", [False, True])
def test_remove_edges_matches_the_masked_graph(cached):
    g, u, i = _graph()
    if cached:
        g.in_csr(BUYS)
        g.rel_graph(BUYS)  # the edge data in CSR order, cached too
    rm = np.array([5, 0, 156, 5, 77, 78, 79, 5], dtype=np.int64)  # unsorted, repeated
    keep = np.ones(E, dtype=bool)
    keep[rm] = False
    g.remove_edges(torch.from_numpy(rm), etype="buys")
    s, d = g.all_edges(etype=BUYS)
    np.testing.assert_array_equal(s.numpy(), u[keep])
    np.testing.assert_array_equal(d.numpy(), i[keep])
    assert g.num_edges(BUYS) == keep.sum() and g.num_edges(BOUGHT) == E  # the reverse is untouched
    _assert_csr(g, BUYS, u[keep], i[keep], N_I)
    np.testing.assert_array_equal(g.edges["buys"].data["w"].numpy(),
                                  (np.arange(E, dtype=np.float32) * 0.5)[keep])
    np.testing.assert_array_equal(g.edges["buys"].data["t"].numpy(),
                                  np.arange(2 * E, dtype=np.int32).reshape(E, 2)[keep])
    np.testing.assert_array_equal(g.nodes["user"].data["f"].numpy(), np.arange(N_U))
    rel = g.rel_graph(BUYS)  # rebuilt for the new numbering
    np.testing.assert_array_equal(rel.edata["w"].numpy(),
                                  g.edges["buys"].data["w"].numpy()[rel.eids.numpy()])
    # a second removal in the NEW numbering, then everything
    keep2 = np.ones(keep.sum(), dtype=bool)
    keep2[[1, 2]] = False
    g.remove_edges([2, 1], etype=BUYS)
    _assert_csr(g, BUYS, u[keep][keep2], i[keep][keep2], N_I)
    g.remove_edges(np.arange(g.num_edges(BUYS)), etype=BUYS)
    assert g.num_edges(BUYS) == 0 and g.edges["buys"].data["t"].shape == (0, 2)
    np.testing.assert_array_equal(g.in_csr(BUYS)[0].numpy(), np.zeros(N_I + 1, dtype=np.int64))
    g.remove_edges([], etype=BUYS)  # an empty relation, an empty list


def test_has_edges_between_after_removal():
    g, u, i = _graph()
    assert bool(g.has_edges_between([u[4]], [i[4]], etype=BUYS)[0])  # (builds nothing it keeps)
    dup = np.flatnonzero((u == u[4]) & (i == i[4]))
    g.remove_edges(dup, etype=BUYS)
    keep = np.ones(E, dtype=bool)
    keep[dup] = False
    got = g.has_edges_between(u, i, etype=BUYS).numpy()
    pairs = set(zip(u[keep].tolist(), i[keep].tolist()))
    np.testing.assert_array_equal(got, [(a, b) in pairs for a, b in zip(u.tolist(), i.tolist())])
    assert not got[4]


@pytest.mark.parametrize("bad", [[3, E], [-1], [2 ** 40]])
def test_remove_edges_refuses_a_bad_id_and_changes_nothing(bad):
    g, u, i = _graph()
    csr = g.in_csr(BUYS)
    w = g.edges["buys"].data["w"]
    with pytest.raises(ValueError, match="outside"):
        g.remove_edges(bad, etype=BUYS)
    assert g.all_edges(etype=BUYS)[0].numpy().tolist() == u.tolist()
    assert g.in_csr(BUYS) is csr and g.edges["buys"].data["w"] is w
    with pytest.raises(ValueError, match="etype"):
        g.remove_edges([0])  # two relations: which one?


def test_clone_is_independent_both_ways():
    g, u, i = _graph()
    csr = g.in_csr(BUYS)
    c = g.clone()
    assert c.in_csr(BUYS) is csr  # built caches are kept by reference
    assert c.all_edges(etype=BUYS)[0] is g.all_edges(etype=BUYS)[0]  # tensors are shared
    assert c.num_nodes("user") == N_U and c.ntypes == g.ntypes
    assert c.canonical_etypes == g.canonical_etypes and c.canonical_etypes is not g.canonical_etypes
    c.remove_edges([0, 1, 2], etype=BUYS)
    c.edges["buys"].data["extra"] = torch.zeros(E - 3)
    c.nodes["user"].data["f"] = torch.zeros(N_U)
    assert g.num_edges(BUYS) == E and g.in_csr(BUYS) is csr
    assert "extra" not in g.edges["buys"].data and g.edges["buys"].data["w"].shape[0] == E
    assert float(g.nodes["user"].data["f"][3]) == 3.0
    g.remove_edges([10], etype=BOUGHT)
    g.nodes["item"].data["new"] = torch.ones(N_I)
    assert c.num_edges(BOUGHT) == E and "new" not in c.nodes["item"].data
    assert c.edges["buys"].data["w"].shape[0] == E - 3
    _assert_csr(c, BUYS, u[3:], i[3:], N_I)
    _assert_csr(g, BUYS, u, i, N_I)


@pytest.mark.parametrize("direction", ["in", "out"])
def test_in_and_out_edges(direction):
    g, u, i = _graph()
    if direction == "in":
        nodes, key, n, fn = [3, 0, 3, N_I - 1, 5], i, N_I, g.in_edges  # a repeat, an empty row
    else:
        nodes, key, n, fn = [7, 7, 0, 22, 1], u, N_U, g.out_edges
    want_e = np.concatenate([np.flatnonzero(key == v) for v in nodes])  # ascending eid per node
    a, b, e = fn(nodes, form="all", etype=BUYS)
    np.testing.assert_array_equal(e.numpy(), want_e)
    np.testing.assert_array_equal(a.numpy(), u[want_e])
    np.testing.assert_array_equal(b.numpy(), i[want_e])
    assert a.dtype == b.dtype == e.dtype == torch.int64
    a2, b2 = fn(torch.tensor(nodes), etype=BUYS)  # form='uv'
    assert torch.equal(a2, a) and torch.equal(b2, b)
    assert torch.equal(fn(nodes, form="eid", etype=BUYS), e)
    assert fn([], form="eid", etype=BUYS).numel() == 0
    with pytest.raises(ValueError, match="form"):
        fn(nodes, form="vu", etype=BUYS)
    with pytest.raises(ValueError, match="outside"):
        fn([n], etype=BUYS)
    # after a removal both follow the new numbering (the source-major CSR is rebuilt)
    g.remove_edges(want_e[:2], etype=BUYS)
    keep = np.ones(E, dtype=bool)
    keep[want_e[:2]] = False
    key2 = key[keep]
    np.testing.assert_array_equal(fn(nodes, form="eid", etype=BUYS).numpy(),
                                  np.concatenate([np.flatnonzero(key2 == v) for v in nodes]))


def test_save_and_load_a_mutated_graph(tmp_path):
    g, u, i = _graph()
    g.in_csr(BUYS)
    g.remove_edges(np.arange(E - 30, E), etype=BUYS)
    g.remove_edges(np.arange(E - 30, E), etype=BOUGHT)
    path = str(tmp_path / "g.bin")
    io.save_graphs(path, [g])
    (h,), _ = io.load_graphs(path)
    for ce in (BUYS, BOUGHT):
        for a, b in zip(g.all_edges(etype=ce), h.all_edges(etype=ce)):
            assert torch.equal(a, b)
        for a, b in zip(g.in_csr(ce), h.in_csr(ce)):
            assert torch.equal(a, b) and a.dtype == b.dtype
    _assert_csr(h, BUYS, u[:E - 30], i[:E - 30], N_I)
    assert torch.equal(h.edges["buys"].data["t"], g.edges["buys"].data["t"])
    assert h.edges["buys"].data["w"].shape[0] == E - 30


# ---- train_valid_split against the reference's own outputs -------------------------------
def _split_graph():
    edges, gt_test = sc.make_inputs()
    g = create_graph(edges, num_nodes_dict={"user": sc.N_USER, "item": sc.N_ITEM})
    return g, gt_test


def _coo(g, ce):
    return tuple(t.cpu().numpy() for t in g.all_edges(etype=ce))


@pytest.mark.parametrize("name", sorted(sc.CASES))
def test_split_equals_the_reference(name):
    g, gt_test = _split_graph()
    res = train_valid_split(g, gt_test, **sc.split_kwargs(sc.CASES[name]))
    for x in (res[3], res[4], res[5], res[6], res[7][0], res[8][1], res[1][sc.BUYS],
              res[9][sc.CLICKS]):
        assert isinstance(x, np.ndarray) and x.dtype == np.int64  # the reference's types
    sc.assert_matches(sc.flatten(res, _coo), sc.load_golden(name))
    assert g.num_edges(sc.BUYS) == sc.N_BUYS  # the full graph is untouched
    # device_out on a host graph: the same values as tensors
    res_t = train_valid_split(g, gt_test, device_out=True, **sc.split_kwargs(sc.CASES[name]))
    assert torch.is_tensor(res_t[3]) and torch.is_tensor(res_t[1][sc.BUYS])
    sc.assert_matches(sc.flatten(tuple(res_t[:1]) + tuple(
        _to_numpy(x) for x in res_t[1:]), _coo), sc.load_golden(name))


def _to_numpy(x):
    if isinstance(x, dict):
        return {k: _to_numpy(v) for k, v in x.items()}
    if isinstance(x, tuple):
        return tuple(_to_numpy(v) for v in x)
    return x.cpu().numpy()


def test_split_remove_train_eids_uses_the_last_relation():
    """train_on_clicks off with remove_train_eids: the last relation of etypes (clicks) has no
    train ids — the reference's KeyError."""
    g, gt_test = _split_graph()
    with pytest.raises(KeyError):
        train_valid_split(g, gt_test, **sc.split_kwargs(sc.RAISING))


# ---- generate_dataloaders ----------------------------------------------------------------
def _loaders(remove_train_eids, sampler="full", sport=False, **kw):
    edges, gt_test = sc.make_inputs()
    nodes = {"user": sc.N_USER, "item": sc.N_ITEM}
    if sport:
        edges[("item", "utilized-for", "sport")] = (np.arange(5), np.arange(5) % 3)
        nodes["sport"] = 3
    g = create_graph(edges, num_nodes_dict=nodes)
    res = train_valid_split(g, gt_test, **sc.split_kwargs((True, remove_train_eids, 1, 1)))
    fixed = types.SimpleNamespace(neighbor_sampler=sampler, remove_train_eids=remove_train_eids,
                                  edge_batch_size=64, node_batch_size=32)
    out = generate_dataloaders(g, res[0], res[1], res[2], res[3], res[4], res[5], res[6], fixed,
                               0, n_layers=3, neg_sample_size=7, **kw)
    return g, res, out


@pytest.mark.parametrize("remove_train_eids", [False, True])
def test_generate_dataloaders_wiring(remove_train_eids):
    g, res, (e_train, e_valid, n_sub, n_valid, n_test) = _loaders(remove_train_eids)
    train_graph, train_eids, valid_eids = res[0], res[1], res[2]
    for ld in (e_train, e_valid):
        assert isinstance(ld, sampling.EdgeDataLoader) and ld.batch_size == 64 and ld.shuffle
        assert isinstance(ld.negative_sampler, sampling.negative_sampler.Uniform)
        assert ld.negative_sampler.k == 7 and not ld.drop_last
    for ld in (n_sub, n_valid, n_test):
        assert isinstance(ld, sampling.NodeDataLoader) and ld.batch_size == 32 and ld.shuffle
    sampler = e_train.sampler
    assert isinstance(sampler, sampling.MultiLayerFullNeighborSampler)
    assert sampler.num_layers == 2  # n_layers - the embedding layer
    assert all(ld.sampler is sampler for ld in (e_valid, n_sub, n_valid, n_test))
    if remove_train_eids:
        assert e_train.g is g and e_train.g_sampling is train_graph and e_train.exclude is None
        assert e_train.reverse_etypes == {}
    else:
        assert e_train.g is train_graph and e_train.g_sampling is train_graph
        assert e_train.exclude == "reverse_types"
        assert e_train.reverse_etypes == {sc.BUYS: sc.BOUGHT, sc.BOUGHT: sc.BUYS,
                                          sc.CLICKS: sc.CLICKED, sc.CLICKED: sc.CLICKS}
    assert e_valid.g is g and e_valid.g_sampling is train_graph and e_valid.exclude is None

    def ids(ld):
        b = ld.type_starts.tolist()
        return {t: ld.flat_ids[b[k]:b[k + 1]].numpy() for k, t in enumerate(ld.types)}
    for ld, want in ((e_train, train_eids), (e_valid, valid_eids)):
        got = ids(ld)
        assert list(got) == list(want)
        for k in want:
            np.testing.assert_array_equal(got[k], want[k])
    for ld, graph, users in ((n_sub, train_graph, res[3]), (n_valid, train_graph, res[4]),
                             (n_test, g, res[5])):
        assert ld.g is graph
        got = ids(ld)
        assert list(got) == ["user", "item"]
        np.testing.assert_array_equal(got["user"], users)
        np.testing.assert_array_equal(got["item"], np.arange(sc.N_ITEM))


def test_generate_dataloaders_sampler_choice_and_sport():
    _g, _res, out = _loaders(False, embedding_layer=False)
    assert out[0].sampler.num_layers == 3
    _g, _res, out = _loaders(False, sampler="partial")
    assert isinstance(out[0].sampler, sampling.MultiLayerNeighborSampler)
    assert out[0].sampler.fanouts == [1, 1, 1] and out[0].sampler.num_layers == 3
    with pytest.raises(KeyError, match="Neighbor sampler nope not recognized"):
        _loaders(False, sampler="nope")
    _g, _res, out = _loaders(False, sport=True, all_sids=np.arange(3))
    assert out[4].types == ["user", "item", "sport"] and out[3].types == ["user", "item"]
    b = out[4].type_starts.tolist()
    assert out[4].flat_ids[b[2]:b[3]].tolist() == [0, 1, 2]
