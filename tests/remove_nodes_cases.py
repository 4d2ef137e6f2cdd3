"""Shared by the remove_nodes tests: a user/item graph with a relation from a type to itself
on each side (so every removal has a relation with both ends relabelled and one it does not
touch), and the numpy restatement of DGL's remove_nodes — mask, cumsum relabel, stable-argsort
CSR — that the host and the device paths are compared with."""
import numpy as np
import torch

from gnnrec.graph import HeteroGraph

BUYS, BOUGHT = ("user", "buys", "item"), ("item", "bought-by", "user")
FOLLOWS, SIMILAR = ("user", "follows", "user"), ("item", "similar", "item")
RELS = (BUYS, BOUGHT, FOLLOWS, SIMILAR)


def make_edges(n_u, n_i, e, seed=5, e_follows=None, e_similar=None):
    """{relation: (src, dst)} int64.  Item n_i - 2 and user n_u - 2 have no edge at all; item 1
    takes every fourth buys edge (a row that straddles 64-slot chunks once e >= 512)."""
    rng = np.random.default_rng(seed)
    u = rng.integers(0, n_u - 2, e)
    u[rng.integers(0, e, max(e // 50, 1))] = n_u - 1
    i = rng.integers(0, n_i - 2, e)
    i[::4] = 1
    i[rng.integers(0, e, max(e // 50, 1))] = n_i - 1
    ef = e // 3 if e_follows is None else e_follows
    es = e // 5 if e_similar is None else e_similar
    fa, fb = rng.integers(0, n_u - 2, ef), rng.integers(0, n_u - 2, ef)
    sa, sb = rng.integers(0, n_i - 2, es), rng.integers(0, n_i - 2, es)
    out = {BUYS: (u, i), BOUGHT: (i.copy(), u.copy()), FOLLOWS: (fa, fb), SIMILAR: (sa, sb)}
    return {ce: (s.astype(np.int64), d.astype(np.int64)) for ce, (s, d) in out.items()}


def make_data(edges, num_nodes):
    """(ndata, edata) as {type / relation: {field: array}}: float rows, a 2-D int32 field."""
    nd = {nt: {"f": (np.arange(3 * n, dtype=np.float32).reshape(n, 3) + (7 if nt == "user" else 0)),
               "c": np.arange(n, dtype=np.int64) * 3}
          for nt, n in num_nodes.items()}
    ed = {}
    for ce, (s, _d) in edges.items():
        E = len(s)
        ed[ce] = {"w": np.arange(E, dtype=np.float32) * 0.5,
                  "t": np.arange(2 * E, dtype=np.int32).reshape(E, 2)}
    return nd, ed


def build_graph(edges, num_nodes, nd=None, ed=None, device=None):
    g = HeteroGraph({ce: (torch.from_numpy(s), torch.from_numpy(d))
                     for ce, (s, d) in edges.items()}, dict(num_nodes), device=device)
    for nt, f in (nd or {}).items():
        for k, v in f.items():
            g.nodes[nt].data[k] = torch.from_numpy(v).to(g.device)
    for ce, f in (ed or {}).items():
        for k, v in f.items():
            g.edges[ce].data[k] = torch.from_numpy(v).to(g.device)
    return g


def np_remove(edges, num_nodes, nd, ed, ntype, rm):
    """remove_nodes restated: -> (edges', num_nodes', ndata', edata', kept_eids per relation)."""
    N = num_nodes[ntype]
    keep_n = np.ones(N, dtype=bool)
    keep_n[np.asarray(rm, dtype=np.int64)] = False
    new_id = np.cumsum(keep_n) - 1
    edges2, ed2, kept_e = {}, {}, {}
    for ce, (s, d) in edges.items():
        keep = np.ones(len(s), dtype=bool)
        if ce[0] == ntype:
            keep &= keep_n[s]
        if ce[2] == ntype:
            keep &= keep_n[d]
        s2, d2 = s[keep], d[keep]
        if ce[0] == ntype:
            s2 = new_id[s2]
        if ce[2] == ntype:
            d2 = new_id[d2]
        edges2[ce] = (s2.astype(np.int64), d2.astype(np.int64))
        kept_e[ce] = np.flatnonzero(keep).astype(np.int64)
        ed2[ce] = {k: v[keep] for k, v in (ed or {}).get(ce, {}).items()}
    num2 = dict(num_nodes)
    num2[ntype] = int(keep_n.sum())
    nd2 = {nt: {k: (v[keep_n] if nt == ntype else v) for k, v in f.items()}
           for nt, f in (nd or {}).items()}
    return edges2, num2, nd2, ed2, kept_e


def np_csr(src, dst, n_dst):
    order = np.argsort(dst, kind="stable")
    indptr = np.zeros(n_dst + 1, dtype=np.int64)
    np.cumsum(np.bincount(dst, minlength=n_dst), out=indptr[1:])
    return indptr, src[order].astype(np.int32), order.astype(np.int64)


def assert_graph(g, edges, num_nodes, nd, ed, csr_cached=None):
    """Every array of g equals the restated graph: node counts, COO, the in-CSR with its
    dtypes (csr_cached: whether g must / must not hold it already; None: either), node and
    edge data."""
    for nt, n in num_nodes.items():
        assert g.num_nodes(nt) == n, (nt, g.num_nodes(nt), n)
    for ce, (s, d) in edges.items():
        gs, gd = g.all_edges(etype=ce)
        assert gs.dtype == gd.dtype == torch.int64
        np.testing.assert_array_equal(gs.cpu().numpy(), s, err_msg=str(ce))
        np.testing.assert_array_equal(gd.cpu().numpy(), d, err_msg=str(ce))
        if csr_cached is not None:
            assert (ce in g._csr) == csr_cached, ce
        want = np_csr(s, d, num_nodes[ce[2]])
        for name, got, w in zip(("indptr", "indices", "eids"), g.in_csr(ce), want):
            assert got.cpu().numpy().dtype == w.dtype, (ce, name)
            np.testing.assert_array_equal(got.cpu().numpy(), w, err_msg=f"{ce} {name}")
        for k, v in (ed or {}).get(ce, {}).items():
            got = g.edges[ce].data[k].cpu().numpy()
            assert got.dtype == v.dtype and got.shape == v.shape, (ce, k, got.shape, v.shape)
            np.testing.assert_array_equal(got, v, err_msg=f"{ce} {k}")
    for nt, f in (nd or {}).items():
        for k, v in f.items():
            got = g.nodes[nt].data[k].cpu().numpy()
            assert got.dtype == v.dtype and got.shape == v.shape, (nt, k, got.shape, v.shape)
            np.testing.assert_array_equal(got, v, err_msg=f"{nt} {k}")
