"""The dirty-set definition of an incremental embedding refresh restated with
numpy on a host COO, a host twin of the graph that records S and E under the same edits, and
the graphs / edit scripts the CPU and GPU tests of gnnrec.inference.IncrementalEmbeddings
share.  TEST INFRASTRUCTURE: nothing here touches the device or the product's code.

  S[T]  rows of type T whose input features changed or that were added
  E[T]  destinations of an added or removed edge of any relation into T, or rows named by mark
  D_0[T] = S[T];  D_l[T] = D_{l-1}[T] | E[T] | U_{R: A -> T} out_R(D_{l-1}[A])   (edited graph)
"""
import numpy as np

BUYS, BOUGHT = ("user", "buys", "item"), ("item", "bought-by", "user")
CLICKS, CLICKED = ("user", "clicks", "item"), ("item", "clicked-by", "user")
SPLIT = 2048  # ops.DEFAULT_SPLIT


def out_neighbours(edges, ce, rows):
    """out_R(X): the destinations of relation ce's out-edges from the set `rows`."""
    s, d = edges[ce]
    return np.unique(d[np.isin(s, rows)])


def dirty_sets(num_nodes, edges, S, E, n_layers, max_dirty_frac=1.0):
    """[D_0, ..., D_L] as {ntype: ascending int64 ids} on the EDITED graph `edges`
    {(src type, relation, dst type): (src ids, dst ids)}.  A type whose set exceeds
    max_dirty_frac of its rows (0: any non-empty set) becomes every row."""
    def cut(ids, nt):
        n = num_nodes[nt]
        if ids.size and (max_dirty_frac == 0 or ids.size > max_dirty_frac * n):
            return np.arange(n, dtype=np.int64)
        return ids

    empty = np.empty(0, np.int64)
    D = [{nt: cut(np.unique(np.asarray(S.get(nt, empty), np.int64)), nt) for nt in num_nodes}]
    for _ in range(n_layers):
        prev, cur = D[-1], {}
        for nt in num_nodes:
            parts = [prev[nt], np.asarray(E.get(nt, empty), np.int64)]
            parts += [out_neighbours(edges, ce, prev[ce[0]]) for ce in edges if ce[2] == nt]
            cur[nt] = cut(np.unique(np.concatenate(parts)), nt)
        D.append(cur)
    return D


class HostTwin:
    """The graph as host arrays under the edits of IncrementalEmbeddings, recording S and E."""

    def __init__(self, num_nodes, edges, feats, occurrence=None):
        self.num_nodes = dict(num_nodes)
        self.edges = {ce: (np.asarray(s, np.int64).copy(), np.asarray(d, np.int64).copy())
                      for ce, (s, d) in edges.items()}
        self.feats = {nt: f.copy() for nt, f in feats.items()}
        self.occurrence = {ce: o.copy() for ce, o in (occurrence or {}).items()}
        self.S = {nt: [] for nt in num_nodes}
        self.E = {nt: [] for nt in num_nodes}

    def add_edges(self, ce, u, v, occurrence=None):
        s, d = self.edges[ce]
        self.edges[ce] = (np.concatenate([s, u]), np.concatenate([d, v]))
        if ce in self.occurrence:
            add = np.zeros(len(u), self.occurrence[ce].dtype) if occurrence is None else occurrence
            self.occurrence[ce] = np.concatenate([self.occurrence[ce], add])
        self.E[ce[2]].append(np.asarray(v, np.int64))

    def remove_edges(self, ce, eids):
        s, d = self.edges[ce]
        self.E[ce[2]].append(d[eids])
        keep = np.ones(s.size, bool)
        keep[eids] = False
        self.edges[ce] = (s[keep], d[keep])
        if ce in self.occurrence:
            self.occurrence[ce] = self.occurrence[ce][keep]

    def add_nodes(self, nt, rows):
        n = self.num_nodes[nt]
        self.feats[nt] = np.concatenate([self.feats[nt], rows])
        self.num_nodes[nt] = n + len(rows)
        self.S[nt].append(np.arange(n, n + len(rows), dtype=np.int64))

    def set_features(self, nt, ids, rows):
        self.feats[nt][ids] = rows
        self.S[nt].append(np.asarray(ids, np.int64))

    def take(self):
        """(S, E) since the last call, as {ntype: ids}."""
        def flat(d):
            return {nt: np.unique(np.concatenate(v)) if v else np.empty(0, np.int64)
                    for nt, v in d.items()}
        out = flat(self.S), flat(self.E)
        self.S = {nt: [] for nt in self.num_nodes}
        self.E = {nt: [] for nt in self.num_nodes}
        return out


# ---- graphs -----------------------------------------------------------------------------
def clustered_pairs(rng, n_u, n_i, cold_u, cold_i, deg_hot, deg_cold):
    """(user, item) pairs: the first cold_u users buy deg_cold items each among the first
    cold_i items only, the others deg_hot items each among the rest — so an edit between cold
    endpoints reaches only cold rows however many layers it travels, and the restated
    |D_L[T]| stays far below N_T / 2 (the tests assert it)."""
    u_c = np.repeat(np.arange(cold_u), deg_cold)
    i_c = rng.integers(0, cold_i, u_c.size)
    u_h = np.repeat(np.arange(cold_u, n_u), deg_hot)
    i_h = rng.integers(cold_i, n_i, u_h.size)
    p = rng.permutation(u_c.size + u_h.size)
    return np.concatenate([u_c, u_h])[p].astype(np.int64), np.concatenate([i_c, i_h])[p].astype(np.int64)


COLD_U, COLD_I = 200, 24

# name -> (users, items, d, edges per hot user, aggregator, hetero aggregate, relations)
ROUTES = {
    # bought-by 26 and buys 138 edges per row: both VALU-fused
    "a_valu": (2000, 400, 128, 28, "mean", "sum", 2),
    # 9 and 17 edges per row, each source type above half the destination's: MFMA-fused
    "b_mfma": (2000, 1010, 128, 9, "mean", "sum", 2),
    # bought-by 8 edges per row from 600 <= 2400 / 2 source rows: pre-projected
    "c_preprojected": (2400, 600, 128, 8, "mean", "sum", 2),
    # one item row above DEFAULT_SPLIT in-edges: buys takes spmm + gemm
    "d_heavy": (3000, 500, 128, 8, "mean", "sum", 2),
    # d = 64: no fused kernel
    "e_d64": (2000, 400, 64, 12, "mean", "sum", 2),
    # four relations: the two-relation launch into users, sequential accumulation into items
    "f_sum": (2400, 600, 128, 6, "mean", "sum", 4),
    "f_mean": (2400, 600, 128, 6, "mean", "mean", 4),
    "f_max": (2400, 600, 128, 6, "mean", "max", 4),
    "f_attention": (2400, 600, 128, 6, "mean", "attention", 4),
    # max reducer behind fc_preagg; edge-weighted mean
    "g_pool": (2000, 400, 128, 10, "pool_nn", "sum", 2),
    "g_mean_edge": (2000, 400, 128, 10, "mean_edge", "sum", 2),
    # the LSTM reducer: the whole-layer fallback
    "h_lstm": (600, 120, 128, 4, "lstm", "sum", 2),
}
HEAVY_DEG = 2500


def route_graph(name, seed=0):
    """-> dict(num_nodes, edges, feats, occurrence, d, agg, hetero) of one route case."""
    n_u, n_i, d, deg, agg, hetero, n_rel = ROUTES[name]
    rng = np.random.default_rng(seed)
    u, i = clustered_pairs(rng, n_u, n_i, COLD_U, COLD_I, deg, 3)
    edges = {BUYS: (u, i), BOUGHT: (i, u)}
    if name == "d_heavy":
        # the heavy row lives in `buys` alone (bought-by stays the reverse of the light edges:
        # two relations are independent COOs), so the item's 2,500 buyers do not turn dirty
        # one layer after the item does
        hu = rng.permutation(np.arange(COLD_U, n_u))[:HEAVY_DEG].astype(np.int64)
        hi = np.full(HEAVY_DEG, n_i - 1, np.int64)
        edges[BUYS] = (np.concatenate([u, hu]), np.concatenate([i, hi]))
    if n_rel == 4:
        cu, ci = clustered_pairs(rng, n_u, n_i, COLD_U, COLD_I, 2 * deg, 4)
        edges = {CLICKS: (cu, ci), CLICKED: (ci, cu), BUYS: (u, i), BOUGHT: (i, u)}
    num_nodes = {"user": n_u, "item": n_i}
    feats = {nt: rng.standard_normal((n, d)).astype(np.float32) for nt, n in num_nodes.items()}
    occ = {}
    if agg.endswith("_edge"):
        occ = {ce: rng.integers(1, 5, s.size).astype(np.float32) for ce, (s, _d) in edges.items()}
    assert max(s.size for s, _d in edges.values()) <= 60000
    return dict(num_nodes=num_nodes, edges=edges, feats=feats, occurrence=occ, d=d, agg=agg,
                hetero=hetero)


def reverse_of(ce):
    return {BUYS: BOUGHT, BOUGHT: BUYS, CLICKS: CLICKED, CLICKED: CLICKS}[ce]


def cold_batch(rng, n, num_nodes):
    """n (user, item) pairs between distinct-as-possible cold users and a few cold items."""
    u = rng.permutation(min(COLD_U, num_nodes["user"]))[np.arange(n) % COLD_U].astype(np.int64)
    i = rng.integers(0, 3, n).astype(np.int64)
    return u, i
