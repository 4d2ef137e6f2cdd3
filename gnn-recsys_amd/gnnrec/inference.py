"""Full-graph inference embedding pass (rows a5/a6/e of SURVEY.md §8).

Replaces reference src/train/run.py:311-349 `get_embeddings` as driven by
main_inference.py:123-152 (NodeDataLoader over every user and item,
MultiLayerFullNeighborSampler, 128-seed batches).  With full neighbourhoods
and eval-mode dropout that loop computes, for every node, the L-layer
ConvModel output over its complete L-hop neighbourhood; here the same
function is computed LAYER-WISE over the whole graph (every edge aggregated
once per layer instead of once per batch that touches it), which is the
reference run with one batch containing every node.

Sharding (P ranks, one per GPU, RCCL over xGMI):
  * the large node type (users) is partitioned into contiguous ranges; every
    relation INTO users is aggregated by the owner of the destination row
    (sources read from the replicated item table);
  * relations into the replicated types (items, sports) are aggregated from
    the edges each rank holds (its users' edges, or an eid range) into a
    partial table of every destination row, then reduce-scattered (sum, or max
    for pool aggregators) to the row owner, which divides by the GLOBAL
    in-degree inside the projection GEMM's operand load and projects;
  * the projected replicated rows are all-gathered for the next layer.
Per layer each rank moves 2·(P−1)/P·N_item·d·4 bytes instead of the
(P−1)/P·(N_user+N_item)·d·4 of an all-gather-everything scheme, and the
collectives overlap the user-side aggregation (async RCCL work handles).
"""
from __future__ import annotations

import contextlib
import os
import time
from typing import Dict, List, Optional, Tuple

import torch

from . import _lib, ops
from .dist import Exchange, degree_ranges, even_ranges, multi_rank, padded_shard
from .graph import HeteroGraph, LazyRows, RelGraph, _FrameDict, build_csr


# --------------------------------------------------------- single process ---
@torch.no_grad()
def full_graph_embeddings(g: HeteroGraph, model, feats: Optional[Dict[str, torch.Tensor]] = None,
                          embedding_layer: Optional[bool] = None) -> Dict[str, torch.Tensor]:
    """Layer-wise full-graph pass on one device: {ntype: [N, out_dim]}."""
    if feats is None:
        feats = g.ndata['features']
    if embedding_layer is None:
        embedding_layer = model.embedding_layer
    h = model.embed(feats) if embedding_layer else dict(feats)
    for layer in model.layers:
        h = layer(g, h)
    return h


@torch.no_grad()
def get_embeddings(g, out_dim: int, trained_model, nodeloader_test, num_batches_valid: int = 0,
                   cuda: bool = True, device=None, embedding_layer: bool = True):
    """Drop-in for reference src/train/run.py:311-349 (minibatch loop over a node loader)."""
    dev = device if device is not None else torch.device('cuda')
    y = {nt: torch.zeros(g.num_nodes(nt), out_dim, device=dev) for nt in g.ntypes}
    for input_nodes, output_nodes, blocks in nodeloader_test:
        blocks = [b.to(dev) for b in blocks]
        input_features = blocks[0].srcdata['features']
        if embedding_layer:
            input_features = trained_model.embed(input_features)
        h = trained_model.get_repr(blocks, input_features)
        for ntype in h.keys():
            y[ntype][output_nodes[ntype]] = h[ntype]
    return y


# ------------------------------------------------ incremental refresh (§21) ---
class RefreshStats:
    """What one IncrementalEmbeddings.refresh() did.  rows[l][ntype]: rows of layer l's table
    recomputed (l = 0: re-embedded input rows; the table's row count where the whole layer
    ran); whole_layer[l][ntype]: the whole layer ran for that type instead of the row path;
    whole_pass: the full pass ran (first use, invalidate(), a changed weight or a relation
    whose kernel route changed).  final_dirty[ntype]: the rows of the LAST layer's table that
    can differ from before the refresh, as (mark int32 [n_rows], ids int64 ascending) device
    tensors — the last layer's dirty set D_L; None: every row (the whole pass, or a type
    above max_dirty_frac); a type that is absent: none of its rows.  A type that took the
    whole layer for a huge row or the LSTM reducer keeps its D_L."""

    def __init__(self, n_layers: int, whole_pass: bool = False):
        self.rows: List[Dict[str, int]] = [{} for _ in range(n_layers + 1)]
        self.whole_layer: List[Dict[str, bool]] = [{} for _ in range(n_layers + 1)]
        self.whole_pass = whole_pass
        self.final_dirty: Dict[str, Optional[Tuple[torch.Tensor, torch.Tensor]]] = {}

    def __repr__(self):
        return (f"RefreshStats(whole_pass={self.whole_pass}, rows={self.rows}, "
                f"whole_layer={self.whole_layer})")


class _TypeView:
    """The graph interface HeteroGraphConv.forward reads, over the relations INTO one node
    type: the whole graph's relation list and edge counts (so the same relations are active
    and the two-relation launch fires as in the whole pass) with the RelGraphs handed in —
    the whole relations, or the CSR rows of a dirty list."""

    is_block = True

    def __init__(self, g: HeteroGraph, rels: Dict[tuple, RelGraph]):
        self._g, self._rels = g, rels
        self.canonical_etypes = [ce for ce in g.canonical_etypes if ce in rels]

    def num_edges(self, ce) -> int:
        return self._g.num_edges(ce)

    def rel_graph(self, ce) -> RelGraph:
        return self._rels[ce]


class _Dirty:
    """D_l of one node type: its marks, and the ascending id list unless it is every row."""

    __slots__ = ("mark", "ids", "count", "all", "huge")

    def __init__(self, mark, ids, count: int, all_rows: bool):
        self.mark, self.ids, self.count, self.all = mark, ids, count, all_rows
        self.huge = False  # a dirty row above ROW_PATH_MAX_DEG in-edges in some relation


# Largest dirty share of a layer's rows at which the row path still beat the whole layer in
# every run of the threshold sweep: 0.5 won (13.0 against 14.9 ms), 0.75 lost
# (profiles/refresh_ab.md)
DEFAULT_MAX_DIRTY_FRAC = 0.5
# A dirty row with more in-edges than this sends its type to the whole layer: the row
# extraction (the sampler's count / fill) copies a row with one wave, and a Zipf head item's
# 34.7M-edge row alone took 620 ms that way (profiles/refresh_ab.md)
ROW_PATH_MAX_DEG = 1 << 18


class IncrementalEmbeddings:
    """full_graph_embeddings kept up to date under graph edits by recomputing only the rows an
    edit can reach.  One device, one process, model.eval().

        inc = IncrementalEmbeddings(g, model)      # runs the full pass once
        inc.add_edges(u, v, etype='buys'); inc.add_edges(v, u, etype='bought-by')
        stats = inc.refresh()                      # inc.h is what a fresh full pass gives

    layers = [h0, ..., hL] as {ntype: table}; h0 = model.embed(feats) (or the feature tables
    themselves without an embedding layer), h = layers[-1].  After refresh() every table is
    torch.equal to the same layer of a full pass over a freshly built graph with the same
    edges.  refresh() writes the tables IN PLACE, so a consumer holding inc.h['user'] sees the
    new rows; two calls replace the tables of their type: add_nodes (one concatenation each)
    and remove_nodes (one gather of the kept rows each).  `numbering` counts the calls that
    renumbered a type (remove_nodes): a consumer whose state is indexed by node id rebuilds it
    when the value changes.
    `generation` counts the refreshes that wrote anything (a consumer that keeps state derived
    from the tables compares it with the value it last saw), and each one reports the rows of
    the last layer it rewrote in RefreshStats.final_dirty.

    The mutation methods wrap the HeteroGraph calls of the same name (same arguments and
    errors; a call that raises records nothing) and record on the device what they touched.
    Both directions of a relation pair are edited with two calls, as on the graph.  A caller
    who edits the graph directly names the rows with mark().  feats given explicitly: the
    tables set_features / add_nodes maintain are those (the graph's 'features' otherwise).

    Dirty sets: S[T] rows whose input changed or that were added, E[T] destinations of an
    added / removed edge or rows named by mark(); D_0 = S, D_l[T] = D_{l-1}[T] | E[T] |
    out_R(D_{l-1}[A]) over every relation R: A -> T of the edited graph.  Layer l recomputes
    exactly D_l[T], through a CSR of those rows that takes the whole relation's kernel route
    (ops.Route).  Above max_dirty_frac of a type's rows (0: always; 1: never) the whole layer
    runs for that type and D_l[T] becomes every row; an LSTM reducer always takes the whole
    layer (its step order depends on the whole relation's degree order), and so does a type
    with a dirty row above ROW_PATH_MAX_DEG in-edges (D_l[T] stays as it is).  The whole pass
    runs when a model parameter changed (ops._wkey), after invalidate(), or when an edit
    moved a relation across a routing threshold (edges per row, the pre-projection's row
    ratio, a heavy row, empty / non-empty)."""

    def __init__(self, g: HeteroGraph, model, feats: Optional[Dict[str, torch.Tensor]] = None,
                 embedding_layer: Optional[bool] = None,
                 max_dirty_frac: Optional[float] = None):
        if not isinstance(g, HeteroGraph) or torch.device(g.device).type != 'cuda':
            raise ValueError("IncrementalEmbeddings: expected a graph on a HIP device (there is "
                             "no CPU path)")
        self._own_feats = feats is not None
        feats = dict(feats) if feats is not None else g.ndata['features']
        for nt, t in feats.items():
            if not t.is_cuda:
                raise ValueError(f"IncrementalEmbeddings: feats[{nt!r}]: expected a device "
                                 f"tensor (there is no CPU path)")
        if model.training:
            raise ValueError("IncrementalEmbeddings: model.eval() first (inference only)")
        self.g, self.model = g, model
        self._feats = feats
        self.embedding_layer = model.embedding_layer if embedding_layer is None \
            else bool(embedding_layer)
        self.max_dirty_frac = DEFAULT_MAX_DIRTY_FRAC if max_dirty_frac is None \
            else float(max_dirty_frac)
        if not 0.0 <= self.max_dirty_frac <= 1.0:
            raise ValueError("IncrementalEmbeddings: max_dirty_frac must lie in [0, 1]")
        dev = g.device
        self._S = {nt: torch.zeros(g.num_nodes(nt), dtype=torch.int32, device=dev)
                   for nt in g.ntypes}
        self._E = {nt: torch.zeros_like(m) for nt, m in self._S.items()}
        # gnnrec_mark_ids' prefix table: nothing is a prefix node here
        self._prefix = {nt: torch.full((g.num_nodes(nt),), -1, dtype=torch.int64, device=dev)
                        for nt in g.ntypes}
        self.layers: List[Dict[str, torch.Tensor]] = []
        self._stale, self._dirty = True, False
        self._keys = self._routes = None
        self._huge: Dict[tuple, torch.Tensor] = {}
        self.phase_ms: Optional[dict] = None
        self.generation = 0
        self.numbering = 0
        self.refresh()

    @property
    def h(self) -> Dict[str, torch.Tensor]:
        return self.layers[-1]

    # ---- recording ----------------------------------------------------------
    def _ids(self, ids, n: int, what: str) -> torch.Tensor:
        ids = torch.as_tensor(ids, dtype=torch.int64, device=self.g.device).reshape(-1)
        if ids.numel() and (int(ids.min()) < 0 or int(ids.max()) >= n):
            raise ValueError(f"{what}: an id lies outside [0, {n})")
        return ids.contiguous()

    def _record(self, store, ntype: str, ids: torch.Tensor) -> None:
        """ids (validated, on the device) into the type's seed marks: no host synchronisation."""
        if ids.numel():
            _lib.torch_ops().mark_ids(ids, self._prefix[ntype], store[ntype])
            self._dirty = True

    def add_edges(self, u, v, data=None, etype=None) -> None:
        """HeteroGraph.add_edges, and the destinations recorded."""
        g = self.g
        g.add_edges(u, v, data=data, etype=etype)
        ce = g.to_canonical_etype(etype if etype is not None else g.canonical_etypes[0])
        v = torch.as_tensor(v, dtype=torch.int64, device=g.device).reshape(-1)
        self._record(self._E, ce[2], v.contiguous())

    def remove_edges(self, eids, etype=None) -> None:
        """HeteroGraph.remove_edges, and the removed edges' destinations (read before the
        removal) recorded."""
        g = self.g
        if etype is None and len(g.canonical_etypes) != 1:
            raise ValueError("remove_edges: etype is needed on a graph with several relations")
        ce = g.to_canonical_etype(etype if etype is not None else g.canonical_etypes[0])
        E = g.num_edges(ce)
        rm = torch.as_tensor(eids, dtype=torch.int64, device=g.device).reshape(-1)
        if rm.numel() and (int(rm.min()) < 0 or int(rm.max()) >= E):
            raise ValueError(f"remove_edges: an edge id lies outside [0, {E})")
        v = ops.gather_rows(g.all_edges(etype=ce)[1], rm.contiguous()) if rm.numel() else rm
        g.remove_edges(rm, etype=ce)
        self._record(self._E, ce[2], v)

    def add_nodes(self, num: int, data=None, ntype=None) -> None:
        """HeteroGraph.add_nodes; the type's cached tables, marks and (own) feature table
        grow by `num` rows — one concatenation each, the only call that REPLACES tables —
        and the new rows are recorded as changed inputs."""
        g = self.g
        g.add_nodes(num, data=data, ntype=ntype)
        num = int(num)
        if num == 0:
            return
        nt = ntype if ntype is not None else g.ntypes[0]
        N, dev = g.num_nodes(nt) - num, g.device
        if self._own_feats:
            if nt in self._feats:
                cur = self._feats[nt]
                new = (data or {}).get('features')
                new = cur.new_zeros((num,) + tuple(cur.shape[1:])) if new is None else \
                    torch.as_tensor(new, dtype=cur.dtype, device=dev)
                self._feats[nt] = torch.cat([cur, new])
        else:
            self._feats = g.ndata['features']
        for tables in self.layers[1 if not self.embedding_layer else 0:]:
            if nt in tables:
                t = tables[nt]
                tables[nt] = torch.cat([t, t.new_zeros((num,) + tuple(t.shape[1:]))])
        if not self.embedding_layer and self.layers:
            self.layers[0] = dict(self._feats)
        for store in (self._S, self._E):
            store[nt] = torch.cat([store[nt], store[nt].new_zeros(num)])
        self._prefix[nt] = torch.cat([self._prefix[nt], self._prefix[nt].new_full((num,), -1)])
        self._record(self._S, nt, torch.arange(N, N + num, dtype=torch.int64, device=dev))

    def remove_nodes(self, nids, ntype=None) -> None:
        """HeteroGraph.remove_nodes.  Before the removal the destinations of the removed
        nodes' out-edges are recorded in E (frontier_mark over the source-major CSR of every
        relation that starts in the type; a relation that only ends in it marks nothing, and a
        removed row needs no mark of its own).  After it the type's cached tables, its (own)
        feature table and its marks — those just recorded included, when a relation leads from
        the type to itself — are compacted to the kept rows: one gather each, the second call
        that REPLACES tables.  `numbering` is incremented."""
        g = self.g
        if ntype is None:
            if len(g.ntypes) != 1:
                raise ValueError("remove_nodes: ntype is needed on a graph with several node "
                                 "types")
            ntype = g.ntypes[0]
        if ntype not in g.ntypes:
            raise ValueError(f"remove_nodes: no node type {ntype!r}")
        N = g.num_nodes(ntype)
        rm = torch.as_tensor(nids, dtype=torch.int64, device=g.device).reshape(-1)
        if rm.numel() == 0:
            return
        if int(rm.min()) < 0 or int(rm.max()) >= N:
            raise ValueError(f"remove_nodes: a node id lies outside [0, {N})")
        rows = torch.unique(rm)  # ascending, distinct: what frontier_mark reads
        for ce in g.canonical_etypes:
            if ce[0] == ntype and g.num_edges(ce):
                oip, oix, _ = g.out_csr(ce)
                ops.frontier_mark(rows, oip, oix, self._E[ce[2]], check=False)
        kept = g._remove_nodes(rm, ntype)
        if self._own_feats:
            if ntype in self._feats:
                self._feats[ntype] = ops.gather_rows(self._feats[ntype], kept)
        else:
            self._feats = g.ndata['features']
        for tables in self.layers[1 if not self.embedding_layer else 0:]:
            if ntype in tables:
                tables[ntype] = ops.gather_rows(tables[ntype], kept)
        if not self.embedding_layer and self.layers:
            self.layers[0] = dict(self._feats)
        for store in (self._S, self._E, self._prefix):
            store[ntype] = ops.gather_rows(store[ntype], kept)
        self.numbering += 1
        self._dirty = True

    def set_features(self, ntype: str, ids, rows) -> None:
        """feats[ntype][ids] = rows (distinct ids), recorded as changed inputs."""
        if ntype not in self._feats:
            raise ValueError(f"set_features: no features of node type {ntype!r}")
        table = self._feats[ntype]
        ids = self._ids(ids, table.shape[0], "set_features")
        rows = torch.as_tensor(rows, dtype=table.dtype, device=table.device)
        if tuple(rows.shape) != (ids.numel(),) + tuple(table.shape[1:]):
            raise ValueError(f"set_features: rows must be {(ids.numel(),) + tuple(table.shape[1:])}"
                             f", got {tuple(rows.shape)}")
        table.index_copy_(0, ids, rows)
        self._record(self._S, ntype, ids)

    def mark(self, ntype: str, ids, inputs: bool = False) -> None:
        """The caller edited the graph directly: the in-edges of these rows changed (and, with
        inputs=True, their input features: the rows are re-embedded too)."""
        if ntype not in self._S:
            raise ValueError(f"mark: no node type {ntype!r}")
        ids = self._ids(ids, self._S[ntype].numel(), "mark")
        self._record(self._E, ntype, ids)
        if inputs:
            self._record(self._S, ntype, ids)

    def invalidate(self) -> None:
        """The next refresh() runs the whole pass."""
        self._stale = True

    # ---- refresh --------------------------------------------------------------
    def _weight_keys(self):
        return tuple(ops._wkey(p) for p in self.model.parameters())

    def _relation_routes(self):
        """Per relation, the whole CSR's Route and what of it the kernel choice reads."""
        g, routes, sig = self.g, {}, {}
        for ce in g.canonical_etypes:
            if g.num_edges(ce) == 0:
                sig[ce] = None
                continue
            ip = g.in_csr(ce)[0]
            r = ops.relation_route(ip)
            routes[ce] = r
            self._huge.pop(ce, None)
            if r.has_split:  # the heavy rows are listed already: those above the cap
                heavy = ops.split_plan(ip, ops.DEFAULT_SPLIT)[0]
                huge = heavy[(ip[heavy + 1] - ip[heavy]) > ROW_PATH_MAX_DEG]
                if huge.numel():
                    self._huge[ce] = huge
            sig[ce] = (r.avg_deg >= ops.FUSED_MIN_DEG, 2 * g.num_nodes(ce[0]) <= r.n_dst,
                       r.has_split)
        return routes, sig

    def _embed_rows(self, nt: str, x: torch.Tensor) -> torch.Tensor:
        mod = getattr(self.model, nt + "_embed", None) if nt in ('user', 'item', 'sport') else None
        return x if mod is None else mod(x)

    def _full_pass(self) -> RefreshStats:
        g, model = self.g, self.model
        if not self._own_feats:
            self._feats = g.ndata['features']
        h = model.embed(self._feats) if self.embedding_layer else dict(self._feats)
        new = [h]
        for layer in model.layers:
            h = layer(g, h)
            new.append(h)
        stats = RefreshStats(len(model.layers), whole_pass=True)
        for l, tables in enumerate(new):
            old = self.layers[l] if l < len(self.layers) else {}
            for nt, t in tables.items():
                if (l > 0 or self.embedding_layer) and nt in old and old[nt].shape == t.shape:
                    tables[nt] = old[nt].copy_(t)  # in place: a held table sees the new rows
                stats.rows[l][nt] = int(t.shape[0])
                stats.whole_layer[l][nt] = True
        self.layers = new
        return stats

    def _scan_counts(self, marks, statuses=(), extra=()):
        """Ranks of every type's marks and, in ONE transfer, their counts, the status words
        of the frontier calls and the one-element tensors of `extra`."""
        ranks = {nt: ops.exclusive_scan(m) for nt, m in marks.items()}
        words = torch.cat([r[-1:] for r in ranks.values()] + [s for s, _a, _b in statuses] +
                          [t.to(torch.int64) for t in extra]).tolist()
        n = len(ranks)
        for i, (_s, n_src, n_dst) in enumerate(statuses):
            ops.frontier_status(words[n + 2 * i:n + 2 * i + 2], n_src, n_dst)
        return ranks, dict(zip(ranks.keys(), words[:n])), words[n + 2 * len(statuses):]

    def _dirty_sets(self, marks, ranks, counts):
        """{ntype: _Dirty} of one layer; a type above max_dirty_frac becomes every row."""
        T, out, frac = _lib.torch_ops(), {}, self.max_dirty_frac
        for nt, m in marks.items():
            n, c = m.numel(), counts[nt]
            if c > 0 and (frac == 0.0 or c > frac * n):
                out[nt] = _Dirty(m.fill_(1), None, n, True)
                continue
            ids = torch.empty(c, dtype=torch.int64, device=m.device)
            if c:
                T.compact_marked(m, ranks[nt], ids)
            out[nt] = _Dirty(m, ids, c, False)
        return out

    def _row_rels(self, todo, routes):
        """The CSR rows of every (type, dirty list) of one layer, per relation into the type,
        with global source ids and ONE transfer for all their sizes."""
        g, T = self.g, _lib.torch_ops()
        jobs = []
        for nt, rows, ces in todo:
            for ce in ces:
                ip, _ix, eid = g.in_csr(ce)
                jobs.append((nt, ce, rows, ops.sample_count(ip, eid, rows, -1)))
        totals = torch.cat([o[-1:] for *_k, o in jobs]).tolist() if jobs else []
        rels: Dict[str, Dict[tuple, RelGraph]] = {}
        for (nt, ce, rows, o_ip), total in zip(jobs, totals):
            ip, ix, eid = g.in_csr(ce)
            dev = rows.device
            # (a slice of a non-empty buffer: a relation whose dirty rows have no in-edge
            # still runs for its self term, and the launch wants non-null arrays)
            src = torch.empty(max(total, 1), dtype=torch.int64, device=dev)[:total]
            sub_eid = torch.empty(max(total, 1), dtype=torch.int64, device=dev)[:total]
            if total:
                T.sample_fill(ip, ix, eid, None, rows, -1, 0, o_ip, src, sub_eid, None)
            sub_ix = torch.empty(max(total, 1), dtype=torch.int32, device=dev)[:total]
            sub_ix.copy_(src)
            ops.pin_route(o_ip, routes[ce], total)
            edata = _FrameDict({k: LazyRows(v, sub_eid) for k, v in g._edata[ce].lazy_items()
                                if not isinstance(v, LazyRows)})
            rels.setdefault(nt, {})[ce] = RelGraph(ce, o_ip, sub_ix, g.num_nodes(ce[0]),
                                                   rows.numel(), edata, sub_eid)
        return rels

    def _next_dirty(self, D):
        """D_l from D_{l-1}: D_l[T] = D_{l-1}[T] | E[T] | out_R(D_{l-1}[A]) over the relations
        R: A -> T.  One transfer: every type's count and every frontier call's status."""
        g = self.g
        marks = {nt: torch.bitwise_or(d.mark, self._E[nt]) for nt, d in D.items()}
        statuses = []
        for ce in g.canonical_etypes:
            a = D[ce[0]]
            if g.num_edges(ce) == 0 or a.count == 0:
                continue
            if a.all:  # every source row: the destinations with an in-edge
                ip = g.in_csr(ce)[0]
                marks[ce[2]] |= (ip[1:] > ip[:-1]).to(torch.int32)
            else:
                oip, oix, _ = g.out_csr(ce)
                statuses.append((ops.frontier_mark(a.ids, oip, oix, marks[ce[2]], check=False),
                                 oip.numel() - 1, marks[ce[2]].numel()))
        huge = [(ce[2], marks[ce[2]][rows].sum().reshape(1)) for ce, rows in self._huge.items()]
        ranks, counts, hit = self._scan_counts(marks, statuses, [t for _nt, t in huge])
        D = self._dirty_sets(marks, ranks, counts)
        for (nt, _t), v in zip(huge, hit):
            D[nt].huge |= bool(v)
        return D

    @contextlib.contextmanager
    def _phase(self, name: str):
        """With `phase_ms` set to a dict (a measurement, tools/bench_refresh.py): the part's
        time between two device synchronisations, added to phase_ms[name]."""
        if self.phase_ms is None:
            yield
            return
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        try:
            yield
        finally:
            torch.cuda.synchronize()
            self.phase_ms[name] = self.phase_ms.get(name, 0.0) + (time.perf_counter() - t0) * 1e3

    @torch.no_grad()
    def refresh(self) -> RefreshStats:
        """Bring every table of `layers` up to date with the graph, the features and the
        recorded edits; -> RefreshStats."""
        g, model = self.g, self.model
        if model.training:
            raise ValueError("IncrementalEmbeddings.refresh: model.eval() first")
        L = len(model.layers)
        full = self._stale or self._weight_keys() != self._keys
        if not full and not self._dirty:
            return RefreshStats(L)
        self.generation += 1
        with self._phase("routes"):
            routes, sig = self._relation_routes()
        if full or sig != self._routes:
            stats = self._full_pass()
            stats.final_dirty = {nt: None for nt in self.layers[-1]}
            self._keys, self._routes = self._weight_keys(), sig
            return self._clean(stats)
        stats = RefreshStats(L)
        # D_0 = S: re-embed
        with self._phase("marks"):
            marks = {nt: m.clone() for nt, m in self._S.items()}
            ranks, counts, _ = self._scan_counts(marks)
            D = self._dirty_sets(marks, ranks, counts)
        for nt, d in D.items():
            if nt not in self.layers[0] or d.count == 0:
                continue
            stats.rows[0][nt], stats.whole_layer[0][nt] = d.count, d.all
            if not self.embedding_layer:
                continue  # h0 IS the feature table
            table = self.layers[0][nt]
            if d.all:
                with self._phase("layers"):
                    table.copy_(self._embed_rows(nt, self._feats[nt]))
                continue
            with self._phase("rows"):
                x = ops.gather_rows(self._feats[nt], d.ids)
            with self._phase("layers"):
                x = self._embed_rows(nt, x)
            with self._phase("rows"):
                ops.scatter_rows(table, d.ids, x)
        for l, layer in enumerate(model.layers, start=1):
            h_prev, tables = self.layers[l - 1], self.layers[l]
            with self._phase("marks"):
                D = self._next_dirty(D)
            todo = []
            for nt, d in D.items():
                if nt not in tables or d.count == 0:
                    continue
                ces = [ce for ce in g.canonical_etypes
                       if ce[2] == nt and g.num_edges(ce) and ce[0] in h_prev]
                whole = d.all or d.huge or any(
                    layer.mods[ce[1]]._aggre_type.startswith('lstm') for ce in ces)
                stats.whole_layer[l][nt] = whole
                stats.rows[l][nt] = tables[nt].shape[0] if whole else d.count
                if whole:
                    with self._phase("layers"):
                        view = _TypeView(g, {ce: g.rel_graph(ce) for ce in ces})
                        tables[nt].copy_(layer(view, (h_prev, {nt: h_prev[nt]}))[nt])
                else:
                    todo.append((nt, d.ids, ces))
            with self._phase("rows"):
                subs = self._row_rels(todo, routes)
                selfs = {nt: ops.gather_rows(h_prev[nt], D[nt].ids) for nt in subs}
            with self._phase("layers"):
                outs = {nt: layer(_TypeView(g, sub), (h_prev, {nt: selfs[nt]}))[nt]
                        for nt, sub in subs.items()}
            with self._phase("rows"):
                for nt, out in outs.items():
                    ops.scatter_rows(tables[nt], D[nt].ids, out)
        # D is D_L now (each layer's marks are tensors of their own: handed out as they are)
        stats.final_dirty = {nt: None if d.all else (d.mark, d.ids) for nt, d in D.items()
                             if nt in self.layers[-1] and d.count}
        return self._clean(stats)

    def _clean(self, stats: RefreshStats) -> RefreshStats:
        for store in (self._S, self._E):
            for m in store.values():
                m.zero_()
        self._stale = self._dirty = False
        return stats


# ------------------------------------------------------------- sharded ------
class RelShard:
    """One relation's edges held by this rank, as a dst-major CSR."""

    def __init__(self, ce, kind: str, indptr, indices, weights, n_rows: int, global_edges: int,
                 deg_own: Optional[torch.Tensor] = None, segs: Optional[list] = None):
        self.ce = ce
        self.kind = kind              # 'local_dst' (dst rows owned here) | 'partial'
        self.indptr = indptr
        self.indices = indices
        self.weights = weights        # float32 per edge in CSR order, or None
        self.n_rows = n_rows
        self.global_edges = global_edges
        self.deg_own = deg_own        # int32 global in-degree of the owned dst rows ('partial')
        self.segs = segs              # 'partial' + segments: [(indptr, indices, weights)] per
                                      # owned segment, in segment order

    @property
    def local_edges(self) -> int:
        return int(self.indices.numel())


def _planned(indptr: torch.Tensor, split: int = ops.DEFAULT_SPLIT) -> torch.Tensor:
    """A shard CSR with its heavy-row plan computed once, at setup (one host readback):
    the pass then launches the plain aggregation kernel when no row is heavy, instead of
    the device-planned form's plan / chunk / combine launches on every pass (C5: 32 extra
    launches per layer, ≈1.5 ms)."""
    if indptr.is_cuda:
        ops.split_plan(indptr, split)
    return indptr


# Source-range tiles are reduced by the plain aggregation kernel, never by the fused one, so
# their heavy rows can be chunked finer than the fused kernel's eligibility threshold
# (DEFAULT_SPLIT): one wave per 512 edges instead of per 2048 spreads a Zipf head over 4x
# the waves — C4 --zipf 1.0 pass 164.2 -> 142.6 ms (split 256: 146.3, 1024: 149.1); the
# uniform configs have no tile row that long.  Every rank uses the same split, so the
# deterministic tree stays bitwise P-invariant.
TILE_SPLIT = 512


class GraphShard:
    """This rank's share of a heterograph for the sharded full-graph pass."""

    def __init__(self, rank: int, world: int, ptype: str, num_nodes: Dict[str, int],
                 canonical_etypes: List[tuple], device, segments: Optional[int] = None,
                 ptype_weight: Optional[torch.Tensor] = None):
        """segments: split every 'partial' relation's edges into this many fixed key ranges
        (source id of the partitioned type, else edge id), `segments // world` per rank, so
        ShardedFullGraphPass(deterministic=True) sums the same partials in the same tree at
        any world size dividing `segments` (bitwise-equal outputs at P=1/2/4/8).

        ptype_weight: per-node weight of the partitioned type (its in-degree summed over
        relations, + 1): the contiguous id ranges are then balanced by cumulative weight
         instead of by node count.  With `segments`, the segment key ranges are
        the weight-balanced ones and every rank's range is the union of its segments, so the
        boundaries still nest at every world size."""
        if segments is not None and (segments < world or segments % world or
                                     segments & (segments - 1)):
            raise ValueError(f"segments={segments} must be a power of two and a multiple of "
                             f"the world size {world}")
        self.segments = segments
        self.rank, self.world, self.ptype = rank, world, ptype
        self.num_nodes = dict(num_nodes)
        self.canonical_etypes = list(canonical_etypes)
        self.device = torch.device(device)
        n_p = num_nodes[ptype]
        if ptype_weight is not None and ptype_weight.numel() != n_p:
            raise ValueError(f"ptype_weight has {ptype_weight.numel()} entries for {n_p} nodes")
        split = (lambda parts: degree_ranges(ptype_weight, parts)) if ptype_weight is not None \
            else (lambda parts: even_ranges(n_p, parts))
        self.balance = "degree" if ptype_weight is not None else "count"
        if segments is not None:
            self.seg_bounds = split(segments)
            k = segments // world
            self.bounds = [self.seg_bounds[r * k] for r in range(world + 1)]
        else:
            self.seg_bounds = None
            self.bounds = split(world)
        self.p_lo, self.p_hi = self.bounds[rank], self.bounds[rank + 1]
        self.shard_rows = {nt: padded_shard(n, world) for nt, n in num_nodes.items()
                           if nt != ptype}
        self.rels: Dict[tuple, RelShard] = {}
        self._in_edges = {}  # ce -> (src, dst - block start): this rank's rows' in-edges
        self._full_rows = {}

    @property
    def ptype_pad(self) -> int:
        """Rows per rank of the partitioned table gathered in rank order (the largest range)."""
        b = self.bounds
        return max(b[r + 1] - b[r] for r in range(self.world))

    def full_in_rows(self, ce):
        """(indptr [S+1], indices int32) of a relation into a replicated type over this
        rank's block of destination rows (own_slice): EVERY in-edge of those rows in edge-id
        order (the reference's mailbox order).  Sources of the partitioned type are numbered
        as rows of its table all-gathered with `ptype_pad` rows per rank; sources of a
        replicated type are its rows.  What a reducer that does not split into per-rank
        partials (the LSTM) runs over at P > 1.  Built once from the graph the shard came
        from (GraphShard.from_graph)."""
        hit = self._full_rows.get(ce)
        if hit is not None:
            return hit
        s_t, _, d_t = ce
        if d_t == self.ptype:
            raise ValueError(f"full_in_rows: {ce} ends in the partitioned type")
        if ce not in self._in_edges:
            raise NotImplementedError(
                "a relation whose reducer does not split into per-rank partials (lstm) needs "
                "the whole in-neighbourhood of the rows a rank owns: build the shard with "
                "GraphShard.from_graph")
        src, dst = self._in_edges[ce]
        S = self.shard_rows[d_t]
        if s_t == self.ptype:
            bounds = torch.tensor(self.bounds, dtype=torch.int64, device=src.device)
            owner = torch.searchsorted(bounds, src, right=True) - 1
            src = owner * self.ptype_pad + (src - bounds[owner])
        indptr, indices, _ = build_csr(src, dst, S)
        hit = (indptr.to(self.device), indices.to(self.device))
        self._full_rows[ce] = hit
        return hit

    @property
    def n_own(self) -> int:
        return self.p_hi - self.p_lo

    def padded_rows(self, nt) -> int:
        return self.shard_rows[nt] * self.world

    def own_slice(self, nt):
        S = self.shard_rows[nt]
        return slice(self.rank * S, (self.rank + 1) * S)

    def local_edge_count(self) -> int:
        return sum(r.local_edges for r in self.rels.values())

    def global_edge_count(self) -> int:
        return sum(r.global_edges for r in self.rels.values())

    def add_relation(self, ce, src: torch.Tensor, dst: torch.Tensor, eid: torch.Tensor,
                     global_edges: int, weights: Optional[torch.Tensor] = None,
                     dst_global_deg: Optional[torch.Tensor] = None):
        """Register this rank's edges of relation ce.

        src/dst are GLOBAL ids of the edges this rank holds; for relations into
        ptype they must be exactly the edges whose dst is owned here."""
        s_t, _, d_t = ce
        dev = self.device
        if d_t == self.ptype:
            if s_t == self.ptype:
                raise NotImplementedError("relations between two rows of the partitioned type "
                                          "need the full partitioned table (not in the schema)")
            rows = dst - self.p_lo
            indptr, indices, order = build_csr(src, rows, self.n_own)
            w = None if weights is None else weights[order].float().contiguous()
            self.rels[ce] = RelShard(ce, 'local_dst', _planned(indptr.to(dev)), indices.to(dev),
                                     None if w is None else w.to(dev), self.n_own, global_edges)
            return
        src_loc = src - self.p_lo if s_t == self.ptype else src
        n_rows = self.padded_rows(d_t)
        indptr, indices, order = build_csr(src_loc, dst, n_rows)
        w = None if weights is None else weights[order].float().contiguous()
        deg = torch.zeros(n_rows, dtype=torch.int32, device=dst_global_deg.device)
        deg[: dst_global_deg.numel()] = dst_global_deg.to(torch.int32)
        segs = None
        if self.segments is not None:
            # key ranges fixed by the global sizes alone: the source id when the source is
            # the partitioned type (rank ranges are unions of them), else the edge id (the
            # edge split of from_graph); each segment's rows keep the edges' input order
            k = self.segments // self.world
            if s_t == self.ptype:
                key, bounds = src, self.seg_bounds
            else:
                key, bounds = eid, even_ranges(global_edges, self.segments)
            segs = []
            for sg in range(self.rank * k, (self.rank + 1) * k):
                sel = (key >= bounds[sg]) & (key < bounds[sg + 1])
                ip, ix, od = build_csr(src_loc[sel], dst[sel], n_rows)
                ws = None if weights is None else weights[sel][od].float().contiguous().to(dev)
                segs.append((_planned(ip.to(dev), TILE_SPLIT), ix.to(dev), ws))
        self.rels[ce] = RelShard(ce, 'partial', _planned(indptr.to(dev)), indices.to(dev),
                                 None if w is None else w.to(dev), n_rows, global_edges,
                                 deg[self.own_slice(d_t)].contiguous().to(dev), segs)

    @classmethod
    def from_graph(cls, g: HeteroGraph, rank: int, world: int, ptype: str = 'user', device=None,
                   weight_field: Optional[str] = 'occurrence', segments: Optional[int] = None,
                   balance: str = 'degree'):
        """Shard a full HeteroGraph held by every rank (tests / moderate graphs).
        balance: 'degree' (ranges balanced by the partitioned type's in-degree over all
        relations + 1) or 'count' (equal node counts)."""
        dev = device if device is not None else g.device
        weight = None
        if balance == 'degree':
            weight = ptype_in_degree(g, ptype)
        elif balance != 'count':
            raise ValueError(f"balance must be 'degree' or 'count', not {balance!r}")
        sh = cls(rank, world, ptype, {nt: g.num_nodes(nt) for nt in g.ntypes},
                 g.canonical_etypes, dev, segments, weight)
        for ce in g.canonical_etypes:
            s, d = g.all_edges(etype=ce)
            if ce[2] != ptype:
                # full_in_rows' input: every in-edge (edge-id order) of this rank's block of
                # the replicated destination rows — kept instead of the whole graph
                S = sh.shard_rows[ce[2]]
                sel = (d >= rank * S) & (d < (rank + 1) * S)
                sh._in_edges[ce] = (s[sel], d[sel] - rank * S)
            E = s.numel()
            eid = torch.arange(E, device=s.device)
            w = g._edata[ce].get(weight_field) if weight_field else None
            if ce[2] == ptype:
                keep = (d >= sh.p_lo) & (d < sh.p_hi)
            elif ce[0] == ptype:
                keep = (s >= sh.p_lo) & (s < sh.p_hi)
            else:
                lo, hi = even_ranges(E, world)[rank], even_ranges(E, world)[rank + 1]
                keep = (eid >= lo) & (eid < hi)
            gdeg = torch.bincount(d, minlength=g.num_nodes(ce[2])) if ce[2] != ptype else None
            sh.add_relation(ce, s[keep], d[keep], eid[keep], E,
                            None if w is None else w[keep], gdeg)
        return sh

    def local_features(self, feats: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
        """Full per-type feature tables -> this rank's inputs (own ptype rows, padded tables)."""
        out = {}
        for nt, x in feats.items():
            if nt == self.ptype:
                out[nt] = x[self.p_lo:self.p_hi].contiguous().to(self.device)
            else:
                t = torch.zeros((self.padded_rows(nt), x.shape[1]), dtype=x.dtype,
                                device=self.device)
                t[: x.shape[0]] = x.to(self.device)
                out[nt] = t
        return out


def ptype_in_degree(g: HeteroGraph, ptype: str) -> torch.Tensor:
    """In-degree of every `ptype` node summed over the relations into it, + 1 (the
    partition weight of GraphShard: a row costs its edges plus its own read/write)."""
    w = torch.ones(g.num_nodes(ptype), dtype=torch.int64, device=g.device)
    for ce in g.canonical_etypes:
        if ce[2] == ptype:
            _, d = g.all_edges(etype=ce)
            w += torch.bincount(d, minlength=w.numel())
    return w


RESERVE_CUS = 16  # of 256: room for RCCL's channel blocks beside the aggregation


class ShardedFullGraphPass:
    """Layer-wise full-graph ConvModel pass over a GraphShard (one rank's view).

    Streams (when `overlap` and the tensors live on a HIP device):
      main  aggregation kernels and the replicated-type GEMMs;
      side  the projection GEMMs of the partitioned type (users), which are
            MFMA-bound and run concurrently with the HBM-bound aggregation of
            the other relation (events order every hand-off);
      RCCL  reduce-scatter / all-gather, issued async_op=True.
    Order per layer: partial aggregation (the item-dst tiles) first.  At world size 1
    the items' tree + projection GEMMs then go to the side stream under the user-dst
    launch (C5 157.8 -> 157.0 ms, C4 -0.1 ms: the persistent user-side launch holds every
    CU, so the GEMM blocks mostly find room only between launches; reserving CUs for them
    costs the HBM-bound launch more — 32 CUs: C5 160.7 ms); GNNREC_OWNED_SIDE=0 restores
    user-side-first on one stream.  With several ranks the reduce-scatter overlaps the
    user-dst aggregation and the all-gather the next layer's partial aggregation.

    `ops_backend` defaults to the HIP ops (gnnrec.ops); tests on CPU ranks
    inject a checker backend with the same signatures.

    The first layer's aggregates of the caller's raw feature tensors are kept across run()
    calls (cache_aggregates): a pass over the same tensors projects them with
    the current weights instead of gathering again; agg_hits / agg_saved record which
    relations did.  A feature write that does not move the tensor's version counter needs
    invalidate_aggregates().  With several ranks, run() and invalidate_aggregates() are
    collective: every rank passes the same tensors, rewritten on all ranks or on none;
    relations whose hit skips a collective are kept only with cache_exchanged=True."""

    def __init__(self, model, shard: GraphShard, exchange: Optional[Exchange] = None,
                 ops_backend=None, overlap: bool = True, fold_embedding: bool = True,
                 deterministic: bool = False, concurrency=None, cache_aggregates: bool = True,
                 cache_exchanged: bool = False):
        self.model = model
        # The first layer's aggregates of RAW feature tables (mean / sum / max over a
        # relation's in-edges of feats[src]) depend on the shard and the features alone, never
        # on a weight: a folded NodeEmbedding moves W_e into the layer's weights and leaves
        # the gather on the caller's tensor.  They are kept across passes (one buffer per
        # relation, allocated once per runner) and a later pass over the same tensors
        # projects them instead of gathering again (_agg_lookup).
        #   key: (id, _version, data_ptr, shape, stride) of the source table and of the edge
        #   weights, and the reducer; the entry holds the tensors, so an id is not recycled.
        #   SPMD: at P > 1 a hit skips the relation's partial exchange, so every rank must
        #   take the same decision — it depends on the caller's tensors alone, which every
        #   rank passes in step (the same tensors, rewritten on every rank or on none);
        #   invalidate_aggregates() is collective in the same sense.  No host read agrees it,
        #   so a rank that decides alone leaves the others waiting in the collective: with
        #   several ranks the relations whose hit skips one (those into a replicated type)
        #   are kept only on request, cache_exchanged=True or GNNREC_AGG_CACHE_EXCHANGE=1,
        #   by a caller who keeps that contract; the partitioned side, which exchanges
        #   nothing, is kept at any world size.
        #   Staleness: a write that does not move _version (a raw pointer handed to the C
        #   ABI, .data tricks) is not seen: call invalidate_aggregates() after one.
        # GNNREC_AGG_CACHE=0 or cache_aggregates=False: every pass gathers.
        self.cache_aggregates = bool(cache_aggregates)
        self.cache_exchanged = bool(cache_exchanged)
        self._agg_cache = {}  # ce -> {'key', 'refs', 'buf', 'valid'}
        self._agg_miss = {}   # ce -> buffer the current pass fills
        self._agg_on = self._agg_exchange_on = False
        self.agg_hits = set()   # relations whose kept aggregate the last run reused
        self.agg_saved = set()  # relations whose aggregate the last run kept
        self._feats_in = {}
        # deterministic: outputs bitwise independent of the world size (needs a shard built
        # with `segments`): replicated-type sums are per-segment partials folded in a fixed
        # pairwise tree (locally, then across ranks after an all-to-all) and every kernel
        # choice is made from global sizes (the embedding fold depends on neither, so it
        # stays on).  Costs the fused launch on the replicated side at one rank and the
        # partials' extra HBM passes.
        if deterministic and shard.segments is None:
            raise ValueError("deterministic=True needs a GraphShard built with segments")
        self.deterministic = deterministic
        # fold the partitioned type's NodeEmbedding into the first layer's fused launches
        # (one rank, mean/sum reducers): its 10M-row GEMM and table disappear
        self.fold_embedding = fold_embedding
        self._fold = {}  # nt -> (W_emb, b_emb) while h[nt] holds that type's raw features
        self._folded_types = set()  # types whose embedding was folded in the last run
        # folded weights per relation, kept across passes and rebuilt only when a parameter
        # changes (its version counter): no weight products inside a timed pass, and the
        # side-stream GEMMs read tensors that live as long as the runner
        self._fold_cache = {}
        self.shard = shard
        self.ex = exchange if exchange is not None else Exchange()
        self.ops = ops_backend if ops_backend is not None else ops
        self.overlap = overlap
        # keyed by the id of the tensor being produced (a layer's input and output tables
        # of one node type are alive together; keying by ntype would make a consumer of
        # the input wait for the producer of the output)
        self._pending = {}   # id(table) -> RCCL work producing it
        self._ready = {}     # id(table) -> event on the side stream producing it
        self.side = (torch.cuda.Stream(device=shard.device)
                     if overlap and shard.device.type == 'cuda' else None)
        # (reserve_cus, dynamic) of the row kernels (ops.set_concurrency) during the pass:
        # rows come from the device work queue (each XCD on its own contiguous range; C4
        # one GPU 149 -> 144 ms), and with several ranks RESERVE_CUS CUs stay free so
        # RCCL's kernels find room, while aggregation blocks that start behind one take
        # fewer rows instead of ending the launch a collective late
        # (tools/probe_comm_overlap.py).  Default on HIP devices: (0, True) at one rank,
        # (RESERVE_CUS, True) at several with overlap on.
        if concurrency is None and shard.device.type == 'cuda':
            concurrency = (RESERVE_CUS if multi_rank(self.ex) and self.side is not None else 0,
                           True)
        self.concurrency = concurrency
        self.timers = None  # optional callable(tag) -> context manager (bench)
        self.side_delay_us = 0  # tests: a delay kernel ahead of every side-stream task
        self.capture = None  # optional list: every layer's output tables are appended (tests)
        self.progress = None  # optional callable(layer index) at every layer's start (bench)
        self.fused = set()  # relations whose aggregation ran with the projection fused
        self.pair_fused = set()  # (ce_a, ce_b) run as one two-relation launch
        self.pair_raw = set()  # ... of them, the one-table form (gnnrec_spmm_pair_f32)
        self.tile_pairs = set()  # (relation a, relation b) whose tiles ran as one launch
        self._pool = {}  # scratch tables reused across passes (_scratch)
        # packed copies of the hidden tables the layers after the first gather (ops.pack_rows;
        # _pack): (node type, stream, rows) -> buffers kept for the runner's life, and the
        # tables packed so far in the current layer
        self._pack_pool, self._packs = {}, {}
        self._packed_on = False
        self.packed = set()  # relations whose gather read packed rows
        self._scratch_ev = {}  # scratch key -> event of the side-stream work reading it
        self._last, self._replicate_last = False, True
        self._side_hold = None  # (event, tensors) of the last layer's side-stream work (_layer)

    def _scratch(self, key, shape, device):
        """A per-runner scratch table reused by every pass (tile partials, unfused
        aggregates): the pass allocates the same shapes every time, and tables that the
        side-stream GEMMs read (record_stream) would otherwise park freed blocks in the
        caching allocator until that stream catches up, growing the pool by tens of GB per
        pass and stalling on fresh hipMallocs (C5: reserved 17 -> 175 GiB over 10 passes, 2 s
        host stalls).  Reuse is ordered by the pass itself: a partial is read by the tree and
        the exchange, which the owner's GEMM waits for, before the next layer's tiles write
        it; an aggregate is read by the side-stream GEMM whose output the next layer waits
        for before it reaches the same relation."""
        t = self._pool.get(key)
        if t is None or tuple(t.shape) != tuple(shape) or t.device != torch.device(device):
            t = torch.empty(shape, dtype=torch.float32, device=device)
            self._pool[key] = t
        return t

    def invalidate_aggregates(self) -> None:
        """Drop the kept first-layer aggregates: the next pass gathers them again.  For
        feature (or edge weight) writes that do not move the tensor's version counter.  With
        several ranks every rank calls it before the same pass (a hit skips a collective)."""
        self._agg_cache.clear()

    @staticmethod
    def _tkey(t):
        return (id(t), t._version, t.data_ptr(), tuple(t.shape), tuple(t.stride()))

    def _agg_lookup(self, ce, msg, preagg, weights, reduce, rows, exchanged=False):
        """The kept aggregate of first-layer relation ce: (buffer [rows, d], hit), or None
        when the relation is not cacheable — its source table must BE the caller's feature
        tensor (a folded embedding, or no embedding layer), with no fc_preagg and a reducer
        that splits (not lstm).  hit: the buffer holds the aggregate of exactly these
        tensors; else the caller fills it in this pass and reports that with _agg_filled.
        exchanged: with several ranks a hit skips a collective (cache_exchanged)."""
        if exchanged and multi_rank(self.ex) and not self._agg_exchange_on:
            return None
        if not self._agg_on or self._layer_idx != 0 or preagg or reduce == 'lstm' or \
                msg is not self._feats_in.get(ce[0]) or msg.dim() != 2:
            return None
        key = (self._tkey(msg), None if weights is None else self._tkey(weights), reduce)
        shape = (rows, msg.shape[1])
        ent = self._agg_cache.get(ce)
        buf = None
        if ent is not None and tuple(ent['buf'].shape) == shape and ent['buf'].device == msg.device:
            buf = ent['buf']
            if ent['valid'] and ent['key'] == key:
                self.agg_hits.add(ce)
                return buf, True
        if buf is None:
            buf = torch.empty(shape, dtype=torch.float32, device=msg.device)
        self._agg_cache[ce] = {'key': key, 'refs': (msg, weights), 'buf': buf, 'valid': False}
        self._agg_miss[ce] = buf
        return buf, False

    def _agg_unhit(self, ce):
        """Take back a hit (its partner in a two-relation tile launch missed): ce is
        gathered in this pass after all."""
        ent = self._agg_cache[ce]
        ent['valid'] = False
        self.agg_hits.discard(ce)
        self._agg_miss[ce] = ent['buf']

    def _agg_filled(self, ce, own=None):
        """The launches that produce relation ce's aggregate are queued; `own`: the tensor
        that holds it, copied when it is not the buffer itself (several ranks: the
        exchange's output).  -> the buffer."""
        buf = self._agg_miss.pop(ce)
        if own is not None and own.data_ptr() != buf.data_ptr():
            buf.copy_(own)
        self._agg_cache[ce]['valid'] = True
        self.agg_saved.add(ce)
        return buf

    def _pack(self, msg, nt, reduce, weighted):
        """The packed copy of hidden table `msg` = h[nt] (384-B rows: a ReLU output is about
        half zeros, ops.pack_rows) for a sum / mean, unweighted gather of a layer after the
        first, or None (GNNREC_PACKED_ROWS=0, another backend, width or reducer: the dense
        gather).  Packed once per layer and stream, on the stream that reads it, into
        buffers allocated once per runner; a table that does not compress sets packed_ok = 0
        on the device and its gathers run their dense loop."""
        if not self._packed_on or self._layer_idx == 0 or weighted or \
                reduce not in ('sum', 'mean') or not msg.is_cuda or msg.dim() != 2 or \
                msg.shape[1] != ops.PACK_D or msg.dtype != torch.float32 or \
                msg.stride(1) != 1 or msg.stride(0) % 4 or msg.data_ptr() % 16:
            return None
        cur = torch.cuda.current_stream(msg.device).cuda_stream
        pk = self._packs.get((id(msg), cur))
        if pk is None:
            key = (nt, cur, msg.shape[0])
            buf = self._pack_pool.get(key)
            if buf is None:
                buf = self._pack_pool[key] = ops.PackedRows(msg.shape[0], msg.device)
            self._packs = {k: v for k, v in self._packs.items() if v is not buf}
            with self._time('pack_rows'):
                pk = ops.pack_rows(msg, into=buf)
            self._packs[(id(msg), cur)] = pk
        return pk

    def _spmm(self, ip, ix, msg, op, pk, **kw):
        """O.spmm, from the packed copy of msg when there is one (the same bits)."""
        if pk is None:
            return self.ops.spmm(ip, ix, msg, op, **kw)
        kw.pop('edge_weight', None)
        kw.pop('empty_neginf', None)
        return ops.spmm_packed(ip, ix, pk, op, **kw)

    def _par(self) -> int:
        """Scratch set of this layer's replicated-type partials: alternating by layer when
        the previous layer's tree + GEMMs may still read theirs on the side stream."""
        return self._layer_idx % 2 if getattr(self, '_owned_side', False) else 0

    def _get(self, h, nt):
        """h[nt], ready for reading on the CURRENT stream.  A table is produced either by a
        collective (its work handle in _pending) or on the side stream (its event in
        _ready), and may be read on both streams — at one rank the replicated table is read
        by the side stream's tree + GEMMs and by main's item->user launch — so readiness is
        never consumed by the first reader: a waited work becomes an event recorded on the
        stream that waited, kept in _ready for every later reader (until the layer that
        reads the table is done, _prune_ready)."""
        t = h[nt]
        key = id(t)
        cur = torch.cuda.current_stream(self.shard.device) if t.is_cuda else None
        ev = self._ready.get(key)
        if ev is not None and cur is not None:
            cur.wait_event(ev)
        w = self._pending.pop(key, None)
        if w is not None:
            w.wait()
            if cur is not None:
                ev = torch.cuda.Event()
                ev.record(cur)
                self._ready[key] = ev
        return t

    def _prune_ready(self, h):
        """Drop readiness of tables no longer in h (a freed table's id can be reused)."""
        live = {id(t) for t in h.values()}
        self._ready = {k: v for k, v in self._ready.items() if k in live}

    def _side_delay(self):
        """Test hook (side_delay_us): hold the side stream before its work, so a reader
        that skips a wait on it reads the table before it is written."""
        if self.side_delay_us and self.side is not None:
            self.ops.hold_cus(8, self.side_delay_us, stream=self.side)

    def _time(self, tag):
        import contextlib
        return self.timers(tag) if self.timers is not None else contextlib.nullcontext()

    def _on_side(self, fn, *tensors):
        """Run fn() on the side stream after everything queued on main; returns its event."""
        if self.side is None:
            fn()
            return None
        main = torch.cuda.current_stream(self.shard.device)
        self.side.wait_stream(main)
        for t in tensors:  # keep the allocator from recycling them under the side stream
            t.record_stream(self.side)
        with torch.cuda.stream(self.side):
            self._side_delay()
            fn()
            ev = torch.cuda.Event()
            ev.record(self.side)
        return ev

    @torch.no_grad()
    def run(self, feats: Dict[str, torch.Tensor], embedding_layer: Optional[bool] = None,
            replicate_output: bool = True):
        """feats: this rank's inputs (see GraphShard.local_features) -> this rank's outputs:
        {ptype: [n_own, out]} and the replicated types as full padded tables, or — with
        replicate_output=False — as this rank's own row block of them (own_slice), so the
        last layer's all-gather is skipped and every type's output stays partitioned."""
        mode = getattr(self.ops, 'concurrency', None)
        if self.concurrency is None or mode is None:
            return self._run(feats, embedding_layer, replicate_output)
        with mode(*self.concurrency):
            return self._run(feats, embedding_layer, replicate_output)

    def _run(self, feats, embedding_layer, replicate_output):
        m, O, sh = self.model, self.ops, self.shard
        self._replicate_last = replicate_output
        self._pending.clear()
        self._ready.clear()
        self._fold.clear()
        self._folded_types.clear()
        self._packed_on = self.ops is ops and sh.device.type == 'cuda' and \
            os.environ.get("GNNREC_PACKED_ROWS", "1") != "0"
        self.packed.clear()
        self._agg_on = self.cache_aggregates and os.environ.get("GNNREC_AGG_CACHE", "1") != "0"
        self._agg_exchange_on = self.cache_exchanged or \
            os.environ.get("GNNREC_AGG_CACHE_EXCHANGE", "0") != "0"
        self._feats_in = feats
        self._agg_miss.clear()
        self._side_hold = None
        self.agg_hits.clear()
        self.agg_saved.clear()
        if embedding_layer is None:
            embedding_layer = m.embedding_layer
        h = dict(feats)
        if embedding_layer:
            embeds = [(nt, getattr(m, nt + '_embed', None)) for nt in ('item', 'sport', 'user')]
            for nt, mod in embeds:
                if mod is None or nt not in h:
                    continue
                W, b, x = mod.proj_feats.weight, mod.proj_feats.bias, h[nt]
                if self.fold_embedding and m.layers and self._foldable(m.layers[0], h, nt, W):
                    self._fold[nt] = (W, b)
                    self._folded_types.add(nt)
                    continue  # h[nt] stays the raw features
                if nt == sh.ptype and self.side is not None:
                    y = torch.empty((x.shape[0], W.shape[0]), dtype=torch.float32, device=x.device)
                    self._ready[id(y)] = self._on_side(
                        lambda: O.gemm(x, W, bias=b, out=y), x, y)
                    h[nt] = y
                else:
                    h[nt] = O.gemm(x, W, bias=b)
        # one rank with a side stream: the replicated type's tree + projection GEMMs run on
        # the side stream under the partitioned type's (HBM-bound) aggregation of the same
        # layer; the tile partials then alternate between two scratch sets by layer parity
        self._owned_side = not multi_rank(self.ex) and self.side is not None and \
            os.environ.get("GNNREC_OWNED_SIDE", "1") != "0"
        for i, layer in enumerate(m.layers):
            self._layer_idx = i
            self._last = i == len(m.layers) - 1
            if self.progress is not None:
                self.progress(i)
            h = self._layer(layer, h)
            self._prune_ready(h)
            if self.capture is not None:
                for nt in list(h):
                    self._get(h, nt)
                self.capture.append(dict(h))
        for nt in list(h):
            self._get(h, nt)
        if self._side_hold is not None:  # main is ordered after everything the side stream ran
            torch.cuda.current_stream(self.shard.device).wait_event(self._side_hold[0])
            self._side_hold = None
        return h

    def _foldable(self, hconv, h, nt, W_emb) -> bool:
        """A node type's NodeEmbedding (the partitioned users, and the replicated items,
        whose 1M-row embedding GEMM every rank would otherwise repeat) folds into every
        first-layer relation that touches nt: as the destination (W_self·W_e, bias W_self·b_e — fused kernel or GEMM
        alike) and as the source when the reducer is linear in the source rows and adds one
        b_e per non-empty row: mean, no fc_preagg (non-linear), no edge weights (they would
        scale b_e).  Needs the HIP backend (bias_nonempty) and W_e square at the fused width.
        Nothing here depends on the world size, so the deterministic mode folds too."""
        if getattr(self.ops, 'can_spmm_project', None) is None or \
                tuple(W_emb.shape) != (ops.FUSED_D, ops.FUSED_D):
            return False
        for ces in self._active(hconv, h).values():
            for ce in ces:
                if nt not in (ce[0], ce[2]):
                    continue
                preagg, weighted, reduce = hconv.mods[ce[1]]._plan_rel(ce)
                if reduce == 'lstm' or ce[0] == ce[2]:
                    return False
                if ce[0] == nt and (preagg or weighted or reduce != 'mean'):
                    return False
        return True

    def _folded(self, mod, ce):
        """(W_self, W_neigh, bias, bias_nonempty) of a fused launch, with a NodeEmbedding
        (W_e, b_e) folded in where its node type's raw features stand in for h:
        (x W_eᵀ + b_e) W_sᵀ = x (W_s W_e)ᵀ + W_s b_e; mean/sum over x[src] then W_n W_e,
        plus W_n b_e on rows that have neighbours."""
        Ws, Wn = mod.fc_self.weight, mod.fc_neigh.weight
        fd, fs = self._fold.get(ce[2]), self._fold.get(ce[0])
        if fd is None and fs is None:  # the parameters themselves: the ops detach them, and
            return Ws, Wn, None, None   # their transposes stay cached on them (ops._transposed)

        def ver(*ts):
            return tuple((id(t), t._version) for t in ts)

        key = ver(Ws, Wn, *(fd or ()), *(fs or ()))
        hit = self._fold_cache.get(ce)
        if hit is not None and hit[0] == key:
            return hit[1]
        Ws, Wn = Ws.detach(), Wn.detach()
        O, bias, bias_ne = self.ops, None, None
        # W @ W_e = linear(W, W_eᵀ); W @ b_e = linear(b_eᵀ, W) — the HIP GEMM, not vendor BLAS
        if fd is not None:
            We, be = fd[0].detach(), fd[1].detach()
            Ws, bias = (O.gemm(Ws, We.t().contiguous()),
                        O.gemm(be.view(1, -1).contiguous(), Ws).view(-1))
        if fs is not None:
            We, be = fs[0].detach(), fs[1].detach()
            Wn, bias_ne = (O.gemm(Wn, We.t().contiguous()),
                           O.gemm(be.view(1, -1).contiguous(), Wn).view(-1))
        self._fold_cache[ce] = (key, (Ws, Wn, bias, bias_ne))
        return Ws, Wn, bias, bias_ne

    @staticmethod
    def _attn(hconv, T, n_rows, device):
        """kwargs of the attention accumulate modes for dst type T (empty otherwise): the
        type's attention vector and a fresh per-row (running max, running sum) state."""
        if hconv.aggregate != 'attention':
            return {}
        return {'attn_vec': hconv.attn[T],
                'attn_state': torch.empty((n_rows, 2), dtype=torch.float32, device=device)}

    def _active(self, hconv, h):
        active: Dict[str, list] = {}
        for ce in self.shard.canonical_etypes:
            rs = self.shard.rels[ce]
            if rs.global_edges == 0 or ce[0] not in h or ce[2] not in h:
                continue
            active.setdefault(ce[2], []).append(ce)
        return active

    def _message(self, mod, ce, h, preagg):
        src = self._get(h, ce[0])
        return self.ops.gemm(src, mod.fc_preagg.weight, relu=True) if preagg else src

    def _partials(self, hconv, h, active):
        """user->item style relations: partial aggregates of the local edges -> reduce-scatter."""
        sh, O = self.shard, self.ops
        partials = {}
        for T, ces in active.items():
            if T == sh.ptype:
                continue
            tree_rels = []
            for ce in ces:
                mod = hconv.mods[ce[1]]
                preagg, weighted, reduce = mod._plan_rel(ce)
                rs = sh.rels[ce]
                msg = self._message(mod, ce, h, preagg)
                can_fuse = getattr(O, 'can_spmm_project', None)
                if self.deterministic and reduce in ('sum', 'mean'):
                    tree_rels.append((ce, rs, msg, weighted, reduce, preagg))
                    continue
                if rs.segs is not None and reduce != 'lstm':
                    # source-range tiles: each tile gathers from a slice of the source table
                    # small enough to stay in the Infinity Cache; accumulated in place
                    op = 'max' if reduce == 'max' else 'sum'
                    kept = self._agg_lookup(ce, msg, preagg, rs.weights if weighted else None,
                                            reduce, sh.shard_rows[T], exchanged=True)
                    if kept is not None and kept[1]:  # no tiles, no exchange
                        partials[ce] = (kept[0], None, reduce, 'kept')
                        continue
                    # one rank: the partial IS the owner's aggregate, accumulated in the kept
                    # buffer itself
                    part = kept[0] if kept is not None and not multi_rank(self.ex) else \
                        self._scratch(('part', ce, self._par()), (rs.n_rows, msg.shape[1]),
                                      msg.device)
                    pk = None if preagg else self._pack(msg, ce[0], reduce, weighted)
                    if pk is not None:
                        self.packed.add(ce)
                    for j, (ip, ix, w) in enumerate(rs.segs):
                        with self._time('spmm_tile'):
                            self._spmm(ip, ix, msg, op, pk, edge_weight=w if weighted else None,
                                       empty_neginf=op == 'max', out=part, accumulate=j > 0,
                                       split=TILE_SPLIT)
                    own, work = self.ex.reduce_scatter_rows(part, op, async_op=self.overlap)
                    partials[ce] = (own, work, reduce)
                    continue
                if not multi_rank(self.ex) and reduce != 'lstm' and can_fuse is not None and \
                        not self.deterministic:
                    self_rows = self._get(h, T)
                    if can_fuse(rs.indptr, msg, self_rows, mod.fc_self.weight,
                                mod.fc_neigh.weight):
                        # one rank: no partials to exchange, aggregate + project in _owned
                        partials[ce] = ('fused', msg, reduce, weighted, preagg)
                        continue
                if reduce == 'lstm':
                    # the recurrence runs over each destination's whole in-edge sequence and
                    # does not split into per-rank partials: at P > 1 the owner of a block of
                    # destination rows runs it over their every in-edge, from the partitioned
                    # table all-gathered (every row: this reducer is off the reference's
                    # hyper-parameter space and is not sized for C4)
                    if multi_rank(self.ex):
                        ip, ix = sh.full_in_rows(ce)
                        src = self._gather_ptype(msg) if ce[0] == sh.ptype else msg
                        own = self._lstm(mod, ip, ix, src)
                    else:
                        own = self._lstm(mod, rs.indptr, rs.indices, msg)
                    partials[ce] = (own, None, reduce)
                    continue
                kept = self._agg_lookup(ce, msg, preagg, rs.weights if weighted else None,
                                        reduce, sh.shard_rows[T], exchanged=True)
                if kept is not None and kept[1]:
                    partials[ce] = (kept[0], None, reduce, 'kept')
                    continue
                okw = {'out': kept[0]} if kept is not None and not multi_rank(self.ex) else {}
                with self._time('spmm'):
                    part = O.spmm(rs.indptr, rs.indices, msg, 'max' if reduce == 'max' else 'sum',
                                  edge_weight=rs.weights if weighted else None,
                                  empty_neginf=reduce == 'max', **okw)
                own, work = self.ex.reduce_scatter_rows(part, 'max' if reduce == 'max' else 'sum',
                                                        async_op=self.overlap)
                partials[ce] = (own, work, reduce)
            partials.update(self._tree_partials(tree_rels))
        return partials

    def _lstm(self, mod, indptr, indices, m):
        """ConvLayer._lstm_reducer (src/model.py:106-121) over a CSR on this pass's backend."""
        L = mod.lstm
        return self.ops.lstm_aggregate(indptr, indices, m, L.weight_ih_l0, L.weight_hh_l0,
                                       L.bias_ih_l0, L.bias_hh_l0)

    def _gather_ptype(self, rows):
        """This rank's rows of the partitioned type -> the table of every rank's rows,
        `ptype_pad` rows per rank in rank order (GraphShard.full_in_rows numbers them)."""
        sh = self.shard
        S = sh.ptype_pad
        pad = torch.zeros((S, rows.shape[1]), dtype=rows.dtype, device=rows.device)
        pad[: rows.shape[0]] = rows
        out = torch.empty((S * self.ex.ws, rows.shape[1]), dtype=rows.dtype, device=rows.device)
        out, work = self.ex.all_gather_rows(pad, out, async_op=True)
        if work is not None:  # RCCL / the emulation: the current stream waits for it
            work.wait()
        return out

    def _tree_partials(self, rels):
        """Σ over each relation's segments in one fixed pairwise tree: the rank folds its
        own contiguous block of segments (a subtree), the all-to-all hands every owner the
        P subtree roots of its rows in rank order, and the owner folds those.  The tree is
        the same at every world size dividing the segment count.

        Relations into one destination type (C5: clicks and buys into items) run their
        tiles interleaved, tile j of every relation before tile j+1, so a relation's tile
        finds the source slice the previous relation's tile j just gathered from still
        partly in the Infinity Cache; each relation's result is unchanged (same kernels,
        same inputs)."""
        # the tree's leaf pairs are formed in the kernel (tile 2i+1 accumulated onto tile 2i:
        # the same single add), the upper levels by _tree_sum
        parts = {ce: [] for ce, *_ in rels}
        n_seg = max((len(rs.segs) for _, rs, *_ in rels), default=0)
        pairs = self._tile_pairs(rels)
        # first-layer aggregates kept from an earlier pass: a relation that hits runs no
        # tile, no tree and no exchange (both relations of a two-relation launch, or
        # neither); one that misses builds its tree in the kept buffer — at one rank tile 0's
        # output, which the tree's last level is folded into
        kept = {ce: self._agg_lookup(ce, msg, preagg, rs.weights if weighted else None, reduce,
                                     self.shard.shard_rows[ce[2]], exchanged=True)
                for ce, rs, msg, weighted, reduce, preagg in rels}
        hits = {ce for ce, k in kept.items() if k is not None and k[1]}
        for item in pairs:
            both = {r[0] for r in item}
            if len(item) == 2 and len(both & hits) == 1:
                ce = (both & hits).pop()  # its partner gathers: the launch runs for both
                self._agg_unhit(ce)
                hits.discard(ce)
        one = not multi_rank(self.ex)

        def tile0(ce, j, shp, dev):
            if j == 0 and one and kept[ce] is not None:
                return kept[ce][0]
            return self._scratch(('tile', ce, j, self._par()), shp, dev)

        for j in range(n_seg):
            for item in pairs:
                if item[0][0] in hits:
                    continue
                if len(item) == 2:  # two relations, one launch per tile (gnnrec_spmm_csr2_f32)
                    (ca, ra, msg, weighted, *_), (cb, rb, *_r) = item
                    self.tile_pairs.add((ca, cb))
                    sa, sb = ra.segs[j], rb.segs[j]
                    csr_a = (sa[0], sa[1], sa[2] if weighted else None)
                    csr_b = (sb[0], sb[1], sb[2] if weighted else None)
                    with self._time('spmm_tile2'):
                        if j % 2 == 0:
                            shp = (ra.n_rows, msg.shape[1])
                            pa, pb = self.ops.spmm2(
                                csr_a, csr_b, msg, 'sum',
                                out_a=tile0(ca, j, shp, msg.device),
                                out_b=tile0(cb, j, shp, msg.device))
                            parts[ca].append(pa)
                            parts[cb].append(pb)
                        else:
                            self.ops.spmm2(csr_a, csr_b, msg, 'sum', out_a=parts[ca][-1],
                                           out_b=parts[cb][-1], accumulate=True)
                    continue
                ce, rs, msg, weighted, reduce, preagg = item[0]
                if j >= len(rs.segs):
                    continue
                ip, ix, w = rs.segs[j]
                ew = w if weighted else None
                pk = None if preagg else self._pack(msg, ce[0], reduce, weighted)
                if pk is not None:
                    self.packed.add(ce)
                with self._time('spmm_tile'):
                    if j % 2 == 0:
                        parts[ce].append(self._spmm(
                            ip, ix, msg, 'sum', pk, edge_weight=ew, split=TILE_SPLIT,
                            out=tile0(ce, j, (rs.n_rows, msg.shape[1]), msg.device)))
                    else:
                        self._spmm(ip, ix, msg, 'sum', pk, edge_weight=ew, out=parts[ce][-1],
                                   accumulate=True, split=TILE_SPLIT)
        out = {}
        for ce, rs, msg, weighted, reduce, _ in rels:
            if ce in hits:
                out[ce] = (kept[ce][0], None, reduce, 'kept')
                continue
            if not multi_rank(self.ex) and self._owned_side:
                # one rank, owner work on the side stream: the whole tree is folded there
                # (_owned), off the main stream that runs the pair launch's inputs next
                out[ce] = (parts[ce], None, reduce, 'tree_local')
                continue
            blocks, work = self.ex.all_to_all_rows(_tree_sum(parts[ce], self.ops),
                                                   async_op=self.overlap)
            out[ce] = (blocks, work, reduce, 'tree')  # the owner's fold waits for the exchange
        return out

    def _tile_pairs(self, rels):
        """Relations of one destination type grouped for the tile launches: two relations
        that gather from the same table with the same segments and no heavy tile rows run as
        one launch per tile (ops.spmm2: C5's clicks and buys); the rest alone.  Each pair's
        partials are bitwise those of separate launches."""
        pair_ok = getattr(self.ops, 'spmm2', None) is not None
        out, used = [], set()
        for i, a in enumerate(rels):
            if i in used:
                continue
            used.add(i)
            for k in range(i + 1, len(rels)):
                b = rels[k]
                if not pair_ok or k in used or b[2] is not a[2] or b[3] != a[3] or \
                        b[1].n_rows != a[1].n_rows or len(b[1].segs) != len(a[1].segs) or \
                        a[2].shape[1] > 256 or a[2].shape[1] % 4:
                    continue
                segs = a[1].segs + b[1].segs
                if any(not sg[0].is_cuda or ops.split_plan(sg[0], TILE_SPLIT) is not None
                       for sg in segs):
                    continue
                if a[3] and any(sg[2] is None for sg in segs):
                    continue
                used.add(k)
                out.append((a, b))
                break
            else:
                out.append((a,))
        return out

    def _local(self, hconv, h, active, out):
        """item->user style relations: dst rows owned here; GEMMs on the side stream."""
        sh, O = self.shard, self.ops
        T = sh.ptype
        ces = active.get(T, [])
        if not ces:
            return
        if len(ces) == 2 and self._pair(hconv, h, ces, out):
            return
        R = len(ces)
        # the self rows of the partitioned type were produced on the side stream (or by main
        # when not overlapping): the side-stream GEMM is ordered after them without making
        # the main stream wait, so this relation's aggregation can start right away
        self_rows = h[T] if self.side is not None else self._get(h, T)
        o = None
        ev = None
        can_fuse = getattr(O, 'can_spmm_project', None)
        for j, ce in enumerate(ces):
            mod = hconv.mods[ce[1]]
            preagg, weighted, reduce = mod._plan_rel(ce)
            rs = sh.rels[ce]
            msg = self._message(mod, ce, h, preagg)
            acc, div = hconv.accum_mode(j, R)
            avg = (rs.global_edges / max(sh.num_nodes[T], 1)) if self.deterministic else None
            # a pre-projected low-degree relation fuses even beside a side stream: its
            # MFMA runs the self half only (C5 bought-by: 10.6 + 0.4 ms vs 7.6 ms gather +
            # a 7 ms GEMM contending with the tiles for HBM)
            pre = reduce != 'lstm' and getattr(O, 'preproject_pays', None) is not None and \
                O.preproject_pays(msg.shape[0], rs.n_rows, reduce)
            if reduce != 'lstm' and can_fuse is not None and can_fuse(
                    rs.indptr, msg, self_rows, mod.fc_self.weight, mod.fc_neigh.weight,
                    avg_deg=avg, gemm_overlaps=self.side is not None and not pre):
                # aggregation and projection in one launch on the main stream: the self rows
                # must be ready here (they may come from the side stream)
                self_rows = self._get(h, T)
                if ev is not None:  # an earlier relation's projection ran on the side stream
                    torch.cuda.current_stream(self.shard.device).wait_event(ev)
                    ev = None
                if o is None:
                    o = torch.empty((sh.n_own, mod._out_feats), dtype=torch.float32,
                                    device=msg.device)
                    akw = self._attn(hconv, T, sh.n_own, o.device)
                Ws, Wn, bias, bias_ne = self._folded(mod, ce)
                vkw = {} if avg is None else {'avg_deg': avg}  # same kernel on every rank
                if O.fused_preprojects(rs.indptr, msg, self_rows, reduce, avg):
                    with self._time('preproject'):
                        msg = O.preproject(msg, Wn, out=self._scratch(
                            ('pre', ce), (msg.shape[0], Wn.shape[0]), msg.device))
                    Wn = None
                tag, kkw = (self._fused_tag(rs, avg), {}) if Wn is None else \
                    self._fused_kept(ce, rs, msg, preagg, weighted, reduce, avg)
                with self._time(tag):
                    O.spmm_project(rs.indptr, rs.indices, msg, self_rows, Ws, Wn, reduce,
                                   rs.weights if weighted else None, relu=True,
                                   l2norm=bool(mod.norm), accum=acc, out_div=div, out=o,
                                   bias=bias, bias_nonempty=bias_ne, **akw, **vkw, **kkw)
                if ce in self._agg_miss:
                    self._agg_filled(ce)
                self.fused.add(ce)
                continue
            # unfused: the aggregate in a scratch table, or in the kept buffer (a hit: no spmm)
            kept = self._agg_lookup(ce, msg, preagg, rs.weights if weighted else None, reduce,
                                    rs.n_rows)
            if kept is not None and kept[1]:
                a = kept[0]
            else:
                with self._time('spmm'):
                    ev_prev = self._scratch_ev.pop(('agg', ce), None)
                    if ev_prev is not None:  # the last side-stream GEMM that read this scratch
                        torch.cuda.current_stream(self.shard.device).wait_event(ev_prev)
                    a = (self._lstm(mod, rs.indptr, rs.indices, msg) if reduce == 'lstm' else
                         O.spmm(rs.indptr, rs.indices, msg, reduce,
                                edge_weight=rs.weights if weighted else None,
                                out=kept[0] if kept is not None else self._scratch(
                                    ('agg', ce), (rs.n_rows, msg.shape[1]), msg.device)))
                if kept is not None:
                    self._agg_filled(ce)
            if o is None:
                o = torch.empty((sh.n_own, mod._out_feats), dtype=torch.float32, device=a.device)
                akw = self._attn(hconv, T, sh.n_own, o.device)

            Ws, Wn, bias, bias_ne = self._folded(mod, ce)
            # a folded source-side embedding adds W_n b_e on rows that have neighbours
            fkw = {} if bias_ne is None else {'bias_nonempty': bias_ne,
                                              'a2_deg': self._local_deg(rs)}

            def proj(Ws=Ws, Wn=Wn, bias=bias, mod=mod, a=a, acc=acc, div=div, o=o, akw=akw,
                     fkw=fkw):
                O.gemm(self_rows, Ws, a, Wn, bias, relu=True, l2norm=bool(mod.norm), accum=acc,
                       out_div=div, out=o, **akw, **fkw)
            ev = self._on_side(proj, self_rows, a, o, *akw.values(), *fkw.values(),
                               *(t for t in (Ws, Wn, bias) if t is not None))
            if ev is not None:
                self._scratch_ev[('agg', ce)] = ev
        out[T] = o
        if ev is not None:
            self._ready[id(o)] = ev

    def _pair_stage(self, plan, h):
        """The pair launch's inputs: both relations' messages pre-projected (the source
        tables × W_neigh,r, into per-relation scratch), the self weights and biases."""
        O = self.ops
        msgs = [self._message(mod, ce, h, preagg) for mod, ce, _, preagg, _, _ in plan]
        rels, Wself, biases = [], [], []
        for (mod, ce, rs, _, weighted, reduce), msg in zip(plan, msgs):
            Ws, Wn, bias, bias_ne = self._folded(mod, ce)
            with self._time('preproject'):
                Y = O.preproject(msg, Wn, out=self._scratch(
                    ('pre', ce), (msg.shape[0], Wn.shape[0]), msg.device))
            rels.append((rs.indptr, rs.indices, Y, reduce, rs.weights if weighted else None,
                         bias_ne))
            Wself.append(Ws)
            biases.append(bias)
        return rels, Wself, biases

    def _pair(self, hconv, h, ces, out) -> bool:
        """Exactly two relations into the partitioned type, both linear (sum / mean) with a
        source table at most half the destination count (C5: clicked-by and bought-by
        from the 1M items into the 10M users): both source tables pre-projected, then one
        spmm_project2 launch reads each user row once and writes it once (C5 user side
        39.0 ms vs 41.0 ms for the two fused launches).
        In deterministic mode the decision uses the global user count (same on every
        rank); the HeteroGraphConv combine runs in the kernel (sum, mean as /2, max, the
        attention softmax over the two relations)."""
        sh, O = self.shard, self.ops
        T = sh.ptype
        plan = self._pair_plan(hconv, h, ces)
        if plan is None:
            return False
        mod = plan[0][0]
        from .nn import _pair_combine
        combine, div = _pair_combine(hconv.aggregate)
        if self._pair_raw(plan):
            # both relations gather the SAME raw source table: no pre-projection, the four
            # projections in the launch's MFMA epilogue (gnnrec_spmm_pair_f32) — the gathered
            # working set is one 512 MB table at C5 instead of two pre-projected ones
            X = self._get(h, plan[0][1][0])
            self_rows = self._get(h, T)
            rels, Wts = [], []
            for m, ce, rs, _, weighted, reduce in plan:
                Ws, Wn, bias, bias_ne = self._folded(m, ce)
                rels.append((rs.indptr, rs.indices, reduce, rs.weights if weighted else None,
                             bias_ne))
                Wts.append((Ws, Wn, bias))
            o = torch.empty((sh.n_own, mod._out_feats), dtype=torch.float32,
                            device=self_rows.device)
            with self._time('spmm_pair'):
                O.spmm_pair(rels[0], rels[1], X, self_rows, Wts[0][0], Wts[0][1], Wts[1][0],
                            Wts[1][1], Wts[0][2], Wts[1][2], relu=True,
                            l2norm=bool(mod.norm), combine=combine, out_div=div, out=o,
                            attn_vec=hconv.attn[T] if combine == 'attention' else None)
            self.pair_fused.add((ces[0], ces[1]))
            self.pair_raw.add((ces[0], ces[1]))
            out[T] = o
            return True
        rels, Wself, biases = self._pair_stage(plan, h)
        self_rows = self._get(h, T)
        o = torch.empty((sh.n_own, mod._out_feats), dtype=torch.float32,
                        device=self_rows.device)
        with self._time('spmm_project2'):
            O.spmm_project2(rels[0], rels[1], self_rows, Wself[0], Wself[1], biases[0],
                            biases[1], relu=True, l2norm=bool(mod.norm), combine=combine,
                            out_div=div, out=o,
                            attn_vec=hconv.attn[T] if combine == 'attention' else None)
        self.pair_fused.add((ces[0], ces[1]))
        out[T] = o
        return True

    def _pair_raw(self, plan) -> bool:
        """The pair gathers one raw table (gnnrec_spmm_pair_f32) when GNNREC_PAIR_RAW=1, both
        relations come from the same source type with no fc_preagg (their messages are that
        table itself) and the backend has the op.  Off by default: at C5 the pre-projected
        launch plus its GEMMs is 0.5 ms faster per pass (csrc/spmm_pair_mfma.hip)."""
        return getattr(self.ops, 'spmm_pair', None) is not None and \
            os.environ.get("GNNREC_PAIR_RAW", "0") != "0" and \
            plan[0][1][0] == plan[1][1][0] and not plan[0][3] and not plan[1][3]

    def _pair_plan(self, hconv, h, ces):
        """The two relations of a pair launch, or None (shapes and layouts only: nothing is
        launched or waited for)."""
        sh, O = self.shard, self.ops
        T = sh.ptype
        if getattr(O, 'spmm_project2', None) is None or \
                hconv.aggregate not in ('sum', 'mean', 'max', 'attention'):
            return None
        n_dec = sh.num_nodes[T] if self.deterministic else sh.n_own
        plan = []
        for ce in ces:
            mod = hconv.mods[ce[1]]
            preagg, weighted, reduce = mod._plan_rel(ce)
            rs = sh.rels[ce]
            src = h.get(ce[0])
            if reduce not in ('sum', 'mean') or src is None or \
                    not O.preproject_pays(src.shape[0], n_dec, reduce):
                return None
            plan.append((mod, ce, rs, preagg, weighted, reduce))
        if bool(plan[0][0].norm) != bool(plan[1][0].norm):
            return None
        # eligibility from the tables' shapes and layouts before anything is launched or
        # waited for (a message is the source table itself, or fc_preagg's fresh output of
        # the same shape): a refused pair costs no GEMM and no main-stream wait
        for mod, ce, rs, _, _, _ in plan:
            if not O.can_spmm_project(rs.indptr, h[ce[0]], h[T], mod.fc_self.weight,
                                      mod.fc_neigh.weight):
                return None
        return plan

    def _fused_kept(self, ce, rs, msg, preagg, weighted, reduce, avg):
        """(timer tag, spmm_project kwargs) of a fused launch of the VALU kernel that keeps
        the rows' aggregate (a miss: the usual tag, the launch gathers) or takes the kept one
        (a hit: 'project_cached', no aggregation launch — the tools that price the gathers do
        not count it).  The MFMA variant and other backends run as ever."""
        tag = self._fused_tag(rs, avg)
        if tag != 'spmm_project' or self.ops is not ops:
            return tag, {}
        kept = self._agg_lookup(ce, msg, preagg, rs.weights if weighted else None, reduce,
                                rs.indptr.numel() - 1)
        if kept is None:
            return tag, {}
        return ('project_cached', {'agg': kept[0], 'agg_mode': 'load'}) if kept[1] else \
            (tag, {'agg': kept[0], 'agg_mode': 'save'})

    def _fused_tag(self, rs, avg):
        """timer tag of a fused launch: 'spmm_project' (VALU kernel) or 'spmm_project_mfma'."""
        fv = getattr(self.ops, 'fused_variant', None)
        return 'spmm_project_mfma' if fv is not None and fv(rs.indptr, avg) == 'mfma' \
            else 'spmm_project'

    @staticmethod
    def _local_deg(rs):
        """int32 in-degrees of a locally owned relation's rows (cached on the relation)."""
        if getattr(rs, '_deg_i32', None) is None:
            rs._deg_i32 = (rs.indptr[1:] - rs.indptr[:-1]).to(torch.int32)
        return rs._deg_i32

    def _owned(self, hconv, h, active, partials, out):
        """owners project their replicated rows, then all-gather the table."""
        sh, O = self.shard, self.ops
        for T, ces in active.items():
            if T == sh.ptype:
                continue
            R = len(ces)
            o = None
            self_rows = self._get(h, T)[sh.own_slice(T)]
            akw = self._attn(hconv, T, self_rows.shape[0], self_rows.device)
            for j, ce in enumerate(ces):
                mod = hconv.mods[ce[1]]
                acc, div = hconv.accum_mode(j, R)
                if isinstance(partials[ce][0], str):  # ('fused', msg, reduce, weighted, preagg)
                    _, msg, reduce, weighted, preagg = partials[ce]
                    rs = sh.rels[ce]
                    if o is None:
                        o = torch.empty((self_rows.shape[0], mod._out_feats),
                                        dtype=torch.float32, device=msg.device)
                    Ws, Wn, bias, bias_ne = self._folded(mod, ce)
                    tag, kkw = self._fused_kept(ce, rs, msg, preagg, weighted, reduce, None)
                    with self._time(tag):
                        O.spmm_project(rs.indptr, rs.indices, msg, self_rows, Ws, Wn, reduce,
                                       rs.weights if weighted else None, relu=True,
                                       l2norm=bool(mod.norm), accum=acc, out_div=div, out=o,
                                       bias=bias, bias_nonempty=bias_ne, **akw, **kkw)
                    if ce in self._agg_miss:
                        self._agg_filled(ce)
                    self.fused.add(ce)
                    continue
                own, work, reduce = partials[ce][:3]
                kind = partials[ce][3] if len(partials[ce]) == 4 else None
                if work is not None:
                    work.wait()
                if kind == 'tree_local':
                    own = _tree_sum(own, self.ops)  # one rank: the segments' whole tree
                elif kind == 'tree':  # deterministic: fold the P subtree roots
                    own = _tree_sum(list(own.unbind(0)), self.ops)
                if ce in self._agg_miss:  # the owner's aggregate of raw features: kept
                    own = self._agg_filled(ce, own)
                if o is None:
                    o = torch.empty((own.shape[0], mod._out_feats), dtype=torch.float32,
                                    device=own.device)
                Ws, Wn, bias, bias_ne = self._folded(mod, ce)
                fkw = {} if bias_ne is None else {'bias_nonempty': bias_ne}
                O.gemm(self_rows, Ws, own, Wn, bias, relu=True,
                       l2norm=bool(mod.norm), accum=acc, out_div=div, out=o,
                       a2_deg=sh.rels[ce].deg_own,
                       a2_mode=(_lib.A2_NONE if reduce == 'lstm' else
                                _lib.A2_ZERO_DEG if reduce == 'max' else _lib.A2_DIV_DEG),
                       **akw, **fkw)
            if not multi_rank(self.ex) or (self._last and not self._replicate_last):
                out[T] = o  # the owned rows ARE the table (one rank), or stay partitioned
                continue
            table = torch.empty((sh.padded_rows(T), o.shape[1]), dtype=torch.float32,
                                device=o.device)
            table, work = self.ex.all_gather_rows(o, table, async_op=self.overlap)
            if work is not None:
                self._pending[id(table)] = work
            out[T] = table

    def _owned_on_side(self, hconv, h, active, partials, out):
        """_owned on the side stream (one rank): ordered after the tiles queued on main,
        its outputs handed to later main-stream readers by an event (_get)."""
        main = torch.cuda.current_stream(self.shard.device)
        self.side.wait_stream(main)
        produced = {}
        with torch.cuda.stream(self.side):
            self._side_delay()
            self._owned(hconv, h, active, partials, produced)
            ev = torch.cuda.Event()
            ev.record(self.side)
        for T, t in produced.items():
            t.record_stream(main)  # read on main later: not recycled under it
            self._ready[id(t)] = ev
            out[T] = t
        return ev

    def _layer(self, hconv, h):
        self._packs = {}
        active = self._active(hconv, h)
        out = {}
        if self._owned_side:
            # tiles (main) -> tree + GEMMs of the replicated type (side) under the
            # partitioned type's launch (main), whose inputs are the previous layer's
            # (the tiles' tree is folded on the side stream too: the partitioned type's
            # launch follows the tiles at once — C4 143.2 -> 142.9 ms, C5 152.3 -> 151.5)
            partials = self._partials(hconv, h, active)
            ev = self._owned_on_side(hconv, h, active, partials, out)
            self._local(hconv, h, active, out)
            self._fold.clear()
            # The side stream reads tensors that main allocated: this layer's input tables
            # and what _partials made (a fused launch's fc_preagg message, an untiled
            # partial).  The caller drops them when this layer returns, and the allocator
            # would hand their memory to main's next allocation (the next layer's fc_preagg
            # output is written before main waits for anything of the side stream) while a
            # late side stream still reads it.  They stay referenced for one more layer and
            # are let go once main is ordered after the side work that read them (no
            # record_stream: it would park every such block until the side stream catches
            # up, _scratch).
            held, self._side_hold = self._side_hold, (ev, partials, h)
            if held is not None:
                torch.cuda.current_stream(self.shard.device).wait_event(held[0])
            return out
        if multi_rank(self.ex):
            partials = self._partials(hconv, h, active)
            self._local(hconv, h, active, out)
        else:
            self._local(hconv, h, active, out)
            partials = self._partials(hconv, h, active)
        self._owned(hconv, h, active, partials, out)
        self._fold.clear()  # a folded embedding only stands in for the first layer's input
        return out


def _tree_sum(parts: List[torch.Tensor], O) -> torch.Tensor:
    """Pairwise tree ((p0+p1)+(p2+p3))+... over a power-of-two list, in order, in place into
    the left operand: subtrees of up to 8 leaves folded by one tree_sum_ kernel each (every
    table read once; the same additions as one add kernel per node, bitwise)."""
    parts = [p.contiguous() for p in parts]
    tree = getattr(O, "tree_sum_", None)
    aligned = all(p.data_ptr() % 16 == 0 and p.numel() % 4 == 0 for p in parts)
    while len(parts) > 1:
        g = min(8, len(parts))
        if tree is not None and aligned:
            parts = [tree(parts[i:i + g]) for i in range(0, len(parts), g)]
        else:
            parts = [O.add_(parts[i], parts[i + 1]) for i in range(0, len(parts), 2)]
    return parts[0]


def gather_partitioned(shard: GraphShard, rows: torch.Tensor, exchange: Exchange) -> torch.Tensor:
    """Assemble the full [N_ptype, d] table from every rank's owned rows (tests/tools)."""
    if exchange.ws == 1:
        return rows
    import torch.distributed as dist
    b = shard.bounds
    S = max(b[r + 1] - b[r] for r in range(exchange.ws))
    pad = torch.zeros((S, rows.shape[1]), dtype=rows.dtype, device=rows.device)
    pad[: rows.shape[0]] = rows
    parts = [torch.empty_like(pad) for _ in range(exchange.ws)]
    dist.all_gather(parts, pad, group=exchange.group)
    return torch.cat([parts[r][: b[r + 1] - b[r]] for r in range(exchange.ws)], 0)


@torch.no_grad()
def inference_ondemand(graph, trained_model, user_ids='all', k: int = 10,
                       already_bought_dict=None, remove_already_bought: bool = True,
                       pred: str = 'cos', use_popularity: bool = False,
                       weight_popularity: float = 1.0, embedding_layer=None):
    """Embedding pass + recommendations on the device, the hot part of reference
    main_inference.py:20-175 (`inference_ondemand`): full-graph embeddings of every
    user and item (:123-152), then top-k per requested user with already-bought items
    removed (:153-166).  `graph` is a HeteroGraph (or a path written by gnnrec.io).

    Returns (recs {user: np.ndarray[k]}, embeddings {ntype: tensor})."""
    import numpy as np

    from .io import read_graph
    from .recs import create_already_bought, get_recs
    g = read_graph(graph, device=torch.device('cuda')) if isinstance(graph, str) else graph
    trained_model.eval()
    h = full_graph_embeddings(g, trained_model, embedding_layer=embedding_layer)
    if isinstance(user_ids, str) and user_ids == 'all':
        user_ids = np.arange(g.num_nodes('user'))
    if already_bought_dict is None:
        users = torch.as_tensor(user_ids, device=g.device)
        s, _ = g.all_edges(etype='buys')
        bought = torch.nonzero(torch.isin(s, users)).squeeze(1)
        already_bought_dict = create_already_bought(g, bought, etype='buys')
    out_dim = h['item'].shape[1]
    recs = get_recs(g, h, trained_model, out_dim, k, list(np.asarray(user_ids).tolist()),
                    already_bought_dict, remove_already_bought, True, g.device, pred,
                    use_popularity, weight_popularity)
    return recs, h
