"""Torch-facing wrappers over the gnnrec ops (include/gnnrec.h, registered with the torch
dispatcher as torch.ops.gnnrec.* by csrc/torch_ops.cpp).

Each function validates shapes/dtypes/devices on the host, allocates the output with
torch (device memory plumbing only) and launches the HIP kernel through its
torch.ops.gnnrec op on the current HIP stream, so the launches are visible to the
dispatcher, to torch.compile (meta kernels, functionalised outputs) and to HIP-graph
capture.  There is no fallback: a missing library or a CPU tensor is an error.
"""
from __future__ import annotations

import collections
import contextlib
import os

from typing import NamedTuple, Optional

import torch

from . import _lib


def _T():
    """torch.ops.gnnrec (loads libgnnrec.so + libgnnrec_torch.so on first use)."""
    return _lib.torch_ops()

REDUCE = {"sum": _lib.REDUCE_SUM, "mean": _lib.REDUCE_MEAN, "max": _lib.REDUCE_MAX}
ACCUM = {"store": _lib.ACC_STORE, "add": _lib.ACC_ADD, "max": _lib.ACC_MAX,
         "attn_first": _lib.ACC_ATTN_FIRST, "attn": _lib.ACC_ATTN,
         "attn_last": _lib.ACC_ATTN_LAST}


def _attn_args(accum, attn_vec, attn_state, n_rows, n_cols):
    """Validated (attn_vec, attn_state) for the attention accumulate modes, else (None, None)."""
    if not accum.startswith("attn"):
        return None, None
    if attn_vec is None or attn_state is None:
        raise ValueError(f"accum={accum!r} needs attn_vec and attn_state")
    _dev(attn_vec, "attn_vec", torch.float32)
    _dev(attn_state, "attn_state", torch.float32)
    if attn_vec.numel() != n_cols or tuple(attn_state.shape) != (n_rows, 2) or \
            not attn_state.is_contiguous():
        raise ValueError(f"attention needs attn_vec [{n_cols}] and a contiguous attn_state "
                         f"[{n_rows}, 2]")
    return attn_vec.detach().contiguous(), attn_state


def _dev(t: torch.Tensor, name: str, dtype=None) -> None:
    if not (t.is_cuda or t.is_meta):  # meta: shape tracing, the ops launch nothing
        raise ValueError(f"{name} must be a HIP device tensor (got {t.device}); "
                         f"gnnrec has no CPU path")
    if dtype is not None and t.dtype != dtype:
        raise ValueError(f"{name} must be {dtype} (got {t.dtype})")


def _rowmajor(t: torch.Tensor, name: str) -> int:
    """Leading dimension of a 2-D tensor with unit column stride."""
    if t.dim() != 2:
        raise ValueError(f"{name} must be 2-D (got shape {tuple(t.shape)})")
    if t.stride(1) != 1 and t.shape[1] > 1:
        raise ValueError(f"{name} must have unit column stride")
    return max(t.stride(0), t.shape[1], 1)


def set_concurrency(reserve_cus: int = 0, dynamic: bool = False) -> None:
    """Process-wide mode of the row kernels (spmm, spmm_project) for launches that share
    the chip with kernels on other streams (gnnrec_set_concurrency): leave `reserve_cus`
    CUs free, and hand rows out through a device work queue when `dynamic`."""
    _T().set_concurrency(int(reserve_cus), bool(dynamic))


def get_concurrency():
    """(reserve_cus, dynamic) currently in force."""
    r, d = _T().get_concurrency()
    return r, bool(d)


def rowq_stats():
    """(queued launches, launches refused a busy ring slot) since the library loaded."""
    q, b = _T().rowq_stats()
    return q, b


@contextlib.contextmanager
def concurrency(reserve_cus: int, dynamic: bool = True):
    """set_concurrency for the launches enqueued inside the block, restored after."""
    old = get_concurrency()
    set_concurrency(reserve_cus, dynamic)
    try:
        yield
    finally:
        set_concurrency(*old)


def hold_cus(blocks: int, usec: int, threads: int = 256, lds_bytes: int = 16384,
             stream=None) -> None:
    """Diagnostic: `blocks` workgroups holding `lds_bytes` of LDS each stay resident for
    `usec` µs on `stream` (default: current) — a collective kernel's footprint."""
    dev = torch.device("cuda", torch.cuda.current_device())
    sink = _hold_sink.get(dev.index)
    if sink is None:
        sink = _hold_sink[dev.index] = torch.empty(1024, dtype=torch.float32, device=dev)
    with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream(dev)):
        _T().hold_cus(int(blocks), int(threads), int(lds_bytes), int(usec), sink)


_hold_sink = {}

DEFAULT_SPLIT = 2048  # edges per chunk for rows split across wavefronts


def split_plan(indptr: torch.Tensor, split: int = DEFAULT_SPLIT):
    """Heavy-row plan for a CSR, computed once and cached on the indptr tensor.

    Returns None when no row has more than `split` edges, else
    (heavy_rows, chunk_ptr, chunk_row, n_chunks)."""
    cached = getattr(indptr, "_gnnrec_split_plan", None)
    if cached is not None and cached[0] == split:
        return cached[1]
    deg = indptr[1:] - indptr[:-1]
    heavy = torch.nonzero(deg > split).squeeze(1)
    plan = None
    if heavy.numel() > 0:
        nch = (deg[heavy] + split - 1) // split
        chunk_ptr = torch.zeros(heavy.numel() + 1, dtype=torch.int64, device=indptr.device)
        torch.cumsum(nch, 0, out=chunk_ptr[1:])
        chunk_row = torch.repeat_interleave(
            torch.arange(heavy.numel(), device=indptr.device), nch)
        plan = (heavy.contiguous(), chunk_ptr, chunk_row.contiguous(), int(chunk_ptr[-1].item()))
    try:
        indptr._gnnrec_split_plan = (split, plan)
    except AttributeError:  # pragma: no cover
        pass
    return plan


def _device_plan(indptr: torch.Tensor, split: int):
    """Device-built heavy-row plan sized from the host edge count (cached on indptr);
    None when no row can have more than `split` edges."""
    cached = getattr(indptr, "_gnnrec_dev_plan", None)
    if cached is not None and cached[0] == split:
        return cached[1]
    n_dst, E = indptr.numel() - 1, indptr._gnnrec_nnz
    cap_h = min(n_dst, E // (split + 1))
    res = None
    if cap_h > 0:
        cap_c = E // split + cap_h
        pl = torch.empty(2 + cap_h + cap_h + 1 + cap_c, dtype=torch.int64, device=indptr.device)
        _T().spmm_plan_build(indptr, split, cap_h, pl)
        res = (pl, cap_h, cap_c)
    try:
        indptr._gnnrec_dev_plan = (split, res)
    except AttributeError:  # pragma: no cover
        pass
    return res


def plan_overflows() -> int:
    """Device-built heavy-row plans that overflowed their capacities since the library
    loaded (gnnrec_spmm_plan_overflows; synchronises the device).  Such a plan's gather
    reduced every row unsplit — exact, not clipped — but a nonzero count means a CSR whose
    host edge count (`_gnnrec_nnz`) understated its edges: check it after a step."""
    return int(_T().spmm_plan_overflows())


def spmm(indptr: torch.Tensor, indices: torch.Tensor, X: torch.Tensor, reduce: str = "mean",
         edge_weight: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None,
         empty_neginf: bool = False, split: Optional[int] = DEFAULT_SPLIT,
         accumulate: bool = False) -> torch.Tensor:
    """a1: out[v] = reduce_{e in row v} X[indices[e]] (* edge_weight[e]).

    indptr int64 [n_dst+1], indices int32 [E] (local rows of X), X fp32 [n_src, d].
    Rows with more than `split` edges are reduced in parallel chunks (split=None: never).
    accumulate: out[v] = out[v] (+ | max) that (source-range tiles of one relation; max
    needs empty_neginf so rows without edges in the tile leave out unchanged).
    """
    T = _T()
    _dev(indptr, "indptr", torch.int64)
    _dev(indices, "indices", torch.int32)
    _dev(X, "X", torch.float32)
    if reduce not in REDUCE:
        raise KeyError(f"Aggregator reduce {reduce} not recognized.")
    n_dst = indptr.numel() - 1
    d = X.shape[1]
    _rowmajor(X, "X")
    if edge_weight is not None:
        _dev(edge_weight, "edge_weight", torch.float32)
        if edge_weight.numel() != indices.numel():
            raise ValueError("edge_weight must have one value per edge")
        edge_weight = edge_weight.contiguous()
    if out is None:
        if accumulate:
            raise ValueError("spmm: accumulate needs out")
        out = torch.empty((n_dst, d), dtype=torch.float32, device=X.device)
    else:
        _dev(out, "out", torch.float32)
        if tuple(out.shape) != (n_dst, d):
            raise ValueError(f"out must be [{n_dst}, {d}]")
    _rowmajor(out, "out")
    flags = _lib.SPMM_EMPTY_NEGINF if empty_neginf else 0
    if accumulate:
        if reduce == "max" and not empty_neginf:
            raise ValueError("spmm: max accumulation needs empty_neginf")
        flags |= _lib.SPMM_ACCUM
    if split and getattr(indptr, "_gnnrec_split_plan", None) is None and \
            getattr(indptr, "_gnnrec_nnz", None) is not None:
        # edge count known, degrees not: heavy-row plan built on the device (no readback)
        dplan = _device_plan(indptr, split)
        if dplan is not None:
            pl, cap_h, cap_c = dplan
            ws = torch.empty((cap_c, d), dtype=torch.float32, device=X.device)
            T.spmm_csr_planned(indptr, indices, edge_weight, X, REDUCE[reduce], flags, split, pl,
                               cap_h, cap_c, out, ws)
            return out
        split = None  # no row can exceed split
    plan = split_plan(indptr, split) if split else None
    if plan is None:
        T.spmm_csr(indptr, indices, edge_weight, X, REDUCE[reduce], flags, out)
        return out
    heavy, chunk_ptr, chunk_row, n_chunks = plan
    ws = torch.empty((n_chunks, d), dtype=torch.float32, device=X.device)
    T.spmm_csr_split(indptr, indices, edge_weight, X, REDUCE[reduce], flags, split, heavy,
                     chunk_ptr, chunk_row, n_chunks, out, ws)
    return out


def spmm2(csr_a, csr_b, X: torch.Tensor, reduce: str = "sum", out_a=None, out_b=None,
          accumulate: bool = False, empty_neginf: bool = False):
    """a1 for two relations into one destination type in one launch (gnnrec_spmm_csr2_f32):
    csr_* = (indptr, indices int32, edge_weight|None) over the same n_dst rows, both gathering
    from X -> (out_a, out_b), each bitwise what spmm() gives for that relation.  No heavy-row
    split: callers use it only for CSRs without heavy rows (split_plan(...) is None)."""
    (ip_a, ix_a, w_a), (ip_b, ix_b, w_b) = csr_a, csr_b
    for t, n in ((ip_a, "indptr_a"), (ip_b, "indptr_b")):
        _dev(t, n, torch.int64)
    _dev(X, "X", torch.float32)
    if reduce not in REDUCE:
        raise KeyError(f"Aggregator reduce {reduce} not recognized.")
    if (w_a is None) != (w_b is None):
        raise ValueError("spmm2: edge weights on both relations or on neither")
    n_dst, d = ip_a.numel() - 1, X.shape[1]
    if accumulate and (out_a is None or out_b is None):
        raise ValueError("spmm2: accumulate needs out_a and out_b")
    if out_a is None:
        out_a = torch.empty((n_dst, d), dtype=torch.float32, device=X.device)
    if out_b is None:
        out_b = torch.empty((n_dst, d), dtype=torch.float32, device=X.device)
    if accumulate and reduce == "max" and not empty_neginf:
        raise ValueError("spmm2: max accumulation needs empty_neginf")
    flags = (_lib.SPMM_EMPTY_NEGINF if empty_neginf else 0) | (_lib.SPMM_ACCUM if accumulate else 0)
    _T().spmm_csr2(ip_a, ix_a, None if w_a is None else w_a.contiguous(), ip_b, ix_b,
                   None if w_b is None else w_b.contiguous(), X, REDUCE[reduce], flags, out_a,
                   out_b)
    return out_a, out_b


def csr_transpose(indptr: torch.Tensor, indices: torch.Tensor, n_src: int,
                  edge_weight: Optional[torch.Tensor] = None, mean: bool = False,
                  n_edges: Optional[int] = None):
    """Source-major CSR of a dst-major block (stable: ascending edge id per source row).
    -> (indptr_t int64 [n_src+1], indices_t int32 = dst rows, ew_t float32 or None), where
    ew_t = edge_weight (· 1/deg(dst) when mean) in the transposed order."""
    T = _T()
    _dev(indptr, "indptr", torch.int64)
    _dev(indices, "indices", torch.int32)
    dev = indptr.device
    n_dst, E = indptr.numel() - 1, _nnz(indptr) if n_edges is None else int(n_edges)
    if indices.numel() < E:
        raise ValueError("csr_transpose: indices shorter than the edge count")
    if edge_weight is not None:
        _dev(edge_weight, "edge_weight", torch.float32)
        if edge_weight.numel() < E:
            raise ValueError("csr_transpose: edge_weight shorter than the edge count")
    ip_t = torch.empty(n_src + 1, dtype=torch.int64, device=dev)
    ix_t = torch.empty(E, dtype=torch.int32, device=dev)
    w_t = torch.empty(E, dtype=torch.float32, device=dev) if (edge_weight is not None or mean) else None
    nbytes = int(T.csr_transpose_workspace_bytes(E, n_src))
    ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
    T.csr_transpose(indptr, indices, edge_weight, n_src, E, bool(mean), ws, ip_t, ix_t, w_t)
    ip_t._gnnrec_nnz = E
    return ip_t, ix_t, w_t


def csr_build(src: torch.Tensor, dst: torch.Tensor, n_dst: int):
    """dst-major CSR of the COO relation (src, dst) with in-row order = edge id
    (gnnrec_csr_build: stable radix sort of the dst ids on the device).
    -> (indptr int64 [n_dst+1], indices int32 = src ids, eids int64)."""
    T = _T()
    _dev(dst, "dst", torch.int64)
    _dev(src, "src", torch.int64)
    if src.shape != dst.shape or src.dim() != 1:
        raise ValueError("csr_build: src and dst must be 1-D tensors of one length")
    dev, E = dst.device, dst.numel()
    if E and n_dst <= 0:
        raise ValueError(f"csr_build: {E} edges into {n_dst} rows")
    src, dst = src.contiguous(), dst.contiguous()
    indptr = torch.empty(n_dst + 1, dtype=torch.int64, device=dev)
    indices = torch.empty(E, dtype=torch.int32, device=dev)
    eids = torch.empty(E, dtype=torch.int64, device=dev)
    nbytes = int(T.csr_build_workspace_bytes(E, n_dst))
    ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
    T.csr_build(src, dst, n_dst, ws, indptr, indices, eids)
    indptr._gnnrec_nnz = E
    return indptr, indices, eids


def csr_remove_edges(src: torch.Tensor, dst: torch.Tensor, rm: torch.Tensor, csr=None):
    """DGL's remove_edges on one relation, COO and dst-major CSR together
    (gnnrec_csr_remove_edges: a stream compaction, no sort).  (src, dst) the COO in edge-id
    order, csr = (indptr, indices, eids) its csr_build (None: the COO alone), rm int64 edge
    ids in any order (duplicates allowed).  -> (src', dst', kept_eids, csr'): the
    boolean-masked COO, the old id of every new edge, and (indptr', indices', eids') of the
    surviving edges in their new numbering — bit for bit csr_build(src', dst', n_dst) — or None.
    An id outside [0, E) raises ValueError (the one readback of the call: two status words)."""
    T = _T()
    dev, E = dst.device, dst.numel()
    if csr is None:
        csr = (torch.empty(0, dtype=torch.int64, device=dev),
               torch.empty(0, dtype=torch.int32, device=dev),
               torch.empty(0, dtype=torch.int64, device=dev))
        Ec = 0
    else:
        Ec = E
        if csr[0].numel() < 1:
            raise ValueError("csr_remove_edges: indptr must have n_dst + 1 entries")
    indptr, indices, eids = csr
    for t, n, dt in ((src, "src", torch.int64), (dst, "dst", torch.int64),
                     (indptr, "indptr", torch.int64), (indices, "indices", torch.int32),
                     (eids, "eids", torch.int64), (rm, "rm", torch.int64)):
        _dev(t, n, dt)
    if src.shape != dst.shape or src.dim() != 1:
        raise ValueError("csr_remove_edges: src and dst must be 1-D tensors of one length")
    if indices.numel() != Ec or eids.numel() != Ec:
        raise ValueError("csr_remove_edges: the CSR does not match the COO's edge count")
    src, dst, rm = src.contiguous(), dst.contiguous(), rm.reshape(-1).contiguous()
    indptr, indices, eids = indptr.contiguous(), indices.contiguous(), eids.contiguous()
    src_o, dst_o, kept = (torch.empty(E, dtype=torch.int64, device=dev) for _ in range(3))
    indptr_o, indices_o, eids_o = (torch.empty_like(t) for t in (indptr, indices, eids))
    status = torch.empty(2, dtype=torch.int64, device=dev)
    ws = torch.empty(max(int(T.csr_remove_edges_workspace_bytes(E, max(indptr.numel() - 1, 0))),
                         1), dtype=torch.uint8, device=dev)
    T.csr_remove_edges(src, dst, indptr, indices, eids, rm, ws, src_o, dst_o, kept, indptr_o,
                       indices_o, eids_o, status)
    n_new = E
    if dev.type != "meta":
        n_new, bad = status.tolist()
        if bad:
            raise ValueError(f"csr_remove_edges: an edge id lies outside [0, {E})")
    def fit(t):  # the valid prefix; copied out when most of the old-size buffer would idle
        return t[:n_new].clone() if 2 * n_new < E else t[:n_new]
    new_csr = None
    if indptr.numel():
        indptr_o._gnnrec_nnz = n_new
        new_csr = (indptr_o, fit(indices_o), fit(eids_o))
    return fit(src_o), fit(dst_o), fit(kept), new_csr


def node_rank_table(nids: torch.Tensor, n_nodes: int):
    """DGL's remove_nodes, part 1 (gnnrec_node_rank_table): the rank table of one node type,
    shared by every relation that touches it.  nids int64 node ids in any order (duplicates
    allowed).  -> (removed int32 [ceil(N/32)], one bit per old id; table int64 [ceil(N/32)+1],
    rank << 32 | word per 32 ids, so new_id(v) is one probe; kept int64 [N'], the ascending old
    ids of the survivors).  An id outside [0, N) raises ValueError (the one readback of the
    call: two status words)."""
    T = _T()
    _dev(nids, "nids", torch.int64)
    n_nodes = int(n_nodes)
    if n_nodes < 0:
        raise ValueError(f"node_rank_table: {n_nodes} nodes")
    dev, W = nids.device, (n_nodes + 31) // 32
    nids = nids.reshape(-1).contiguous()
    removed = torch.empty(W, dtype=torch.int32, device=dev)
    table = torch.empty(W + 1, dtype=torch.int64, device=dev)
    kept = torch.empty(n_nodes, dtype=torch.int64, device=dev)
    status = torch.empty(2, dtype=torch.int64, device=dev)
    ws = torch.empty(max(int(T.node_rank_table_workspace_bytes(n_nodes)), 1), dtype=torch.uint8,
                     device=dev)
    T.node_rank_table(nids, n_nodes, ws, removed, table, kept, status)
    n_new = n_nodes
    if dev.type != "meta":
        n_new, bad = status.tolist()
        if bad:
            raise ValueError(f"node_rank_table: a node id lies outside [0, {n_nodes})")
    return removed, table, kept[:n_new]


def csr_remove_nodes(src: torch.Tensor, dst: torch.Tensor, csr, src_table, dst_table,
                     n_src: int, n_dst: int, n_dst_new: int, sync: bool = True):
    """DGL's remove_nodes, part 2, on one relation, COO and dst-major CSR together
    (gnnrec_csr_remove_nodes: a stream compaction, no sort).  (src, dst) the COO in edge-id
    order, csr = (indptr, indices, eids) its csr_build (None: the COO alone); src_table /
    dst_table the node_rank_table of the source / destination type (None for a side that keeps
    its numbering; both for a relation from the type to itself); n_src, n_dst the old node
    counts and n_dst_new the destination type's new one.  -> (src', dst', kept_eids, csr'): the
    COO of the edges with no removed endpoint, relabelled, the old id of every new edge, and
    (indptr' [n_dst_new+1], indices', eids') — bit for bit csr_build(src', dst', n_dst_new) —
    or None.  An endpoint outside its type raises ValueError (the one readback of the call:
    two status words).  sync=False: no readback — -> (pending, status), for
    csr_remove_nodes_finish(pending, n_new, bad) once the caller has read the status words
    (of several relations in one transfer)."""
    T = _T()
    dev, E = dst.device, dst.numel()
    n_src, n_dst, n_dst_new = int(n_src), int(n_dst), int(n_dst_new)
    if csr is None:
        csr = (torch.empty(0, dtype=torch.int64, device=dev),
               torch.empty(0, dtype=torch.int32, device=dev),
               torch.empty(0, dtype=torch.int64, device=dev))
        Ec = 0
    else:
        Ec = E
        if csr[0].numel() != n_dst + 1:
            raise ValueError("csr_remove_nodes: indptr must have n_dst + 1 entries")
    indptr, indices, eids = csr
    for t, n, dt in ((src, "src", torch.int64), (dst, "dst", torch.int64),
                     (indptr, "indptr", torch.int64), (indices, "indices", torch.int32),
                     (eids, "eids", torch.int64)):
        _dev(t, n, dt)
    if src_table is None and dst_table is None:
        raise ValueError("csr_remove_nodes: a source table, a destination table or both")
    for t, n, cnt in ((src_table, "src_table", n_src), (dst_table, "dst_table", n_dst)):
        if t is not None:
            _dev(t, n, torch.int64)
            if t.dim() != 1 or t.numel() != (cnt + 31) // 32 + 1:
                raise ValueError(f"csr_remove_nodes: {n} is not the rank table of {cnt} nodes")
    if src.shape != dst.shape or src.dim() != 1:
        raise ValueError("csr_remove_nodes: src and dst must be 1-D tensors of one length")
    if indices.numel() != Ec or eids.numel() != Ec:
        raise ValueError("csr_remove_nodes: the CSR does not match the COO's edge count")
    if not (0 <= n_dst_new <= n_dst) or (dst_table is None and n_dst_new != n_dst):
        raise ValueError(f"csr_remove_nodes: {n_dst_new} new rows from {n_dst}")
    src, dst = src.contiguous(), dst.contiguous()
    indptr, indices, eids = indptr.contiguous(), indices.contiguous(), eids.contiguous()
    src_o, dst_o, kept = (torch.empty(E, dtype=torch.int64, device=dev) for _ in range(3))
    indptr_o = torch.empty(n_dst_new + 1 if indptr.numel() else 0, dtype=torch.int64, device=dev)
    indices_o, eids_o = torch.empty_like(indices), torch.empty_like(eids)
    status = torch.empty(2, dtype=torch.int64, device=dev)
    ws = torch.empty(max(int(T.csr_remove_nodes_workspace_bytes(E, n_dst)), 1), dtype=torch.uint8,
                     device=dev)
    T.csr_remove_nodes(src, dst, indptr, indices, eids,
                       None if src_table is None else src_table.contiguous(),
                       None if dst_table is None else dst_table.contiguous(), n_src, n_dst,
                       n_dst_new, ws, src_o, dst_o, kept, indptr_o, indices_o, eids_o, status)
    pending = (E, n_src, n_dst, src_o, dst_o, kept, indptr_o, indices_o, eids_o)
    if not sync:
        return pending, status
    n_new, bad = (E, 0) if dev.type == "meta" else status.tolist()
    return csr_remove_nodes_finish(pending, n_new, bad)


def csr_remove_nodes_finish(pending, n_new: int, bad: int):
    """The result of a csr_remove_nodes(..., sync=False) call from its two status words."""
    E, n_src, n_dst, src_o, dst_o, kept, indptr_o, indices_o, eids_o = pending
    if bad:
        raise ValueError(f"csr_remove_nodes: an endpoint lies outside [0, {n_src}) x "
                         f"[0, {n_dst})")
    def fit(t):  # the valid prefix; copied out when most of the old-size buffer would idle
        return t[:n_new].clone() if 2 * n_new < E else t[:n_new]
    new_csr = None
    if indptr_o.numel():
        indptr_o._gnnrec_nnz = n_new
        new_csr = (indptr_o, fit(indices_o), fit(eids_o))
    return fit(src_o), fit(dst_o), fit(kept), new_csr


def csr_add_edges(csr, src_new: torch.Tensor, dst_new: torch.Tensor, n_src: int, n_dst: int):
    """DGL's add_edges on one relation's dst-major CSR (gnnrec_csr_add_edges: the batch's own
    CSR merged into the cached one; the old edges are not sorted again).  csr = (indptr,
    indices, eids) as csr_build gives it, (src_new, dst_new) the int64 batch, which takes the
    edge ids E .. E+n-1 in the order given.  -> (indptr', indices', eids'), bit for bit
    csr_build of the concatenated COO.  An id outside [0, n_src) / [0, n_dst) raises
    ValueError (the one readback of the call: two status words)."""
    T = _T()
    indptr, indices, eids = csr
    for t, n, dt in ((indptr, "indptr", torch.int64), (indices, "indices", torch.int32),
                     (eids, "eids", torch.int64), (src_new, "src_new", torch.int64),
                     (dst_new, "dst_new", torch.int64)):
        _dev(t, n, dt)
    if src_new.shape != dst_new.shape or src_new.dim() != 1:
        raise ValueError("csr_add_edges: src_new and dst_new must be 1-D tensors of one length")
    if indptr.numel() != n_dst + 1 or indices.numel() != eids.numel():
        raise ValueError("csr_add_edges: the CSR must be indptr [n_dst+1], indices [E], eids [E]")
    dev, E, n = indptr.device, eids.numel(), dst_new.numel()
    if n and (n_src <= 0 or n_dst <= 0):
        raise ValueError(f"csr_add_edges: {n} edges between {n_src} and {n_dst} nodes")
    indptr, indices, eids = indptr.contiguous(), indices.contiguous(), eids.contiguous()
    src_new, dst_new = src_new.contiguous(), dst_new.contiguous()
    indptr_o = torch.empty(n_dst + 1, dtype=torch.int64, device=dev)
    indices_o = torch.empty(E + n, dtype=torch.int32, device=dev)
    eids_o = torch.empty(E + n, dtype=torch.int64, device=dev)
    status = torch.empty(2, dtype=torch.int64, device=dev)
    ws = torch.empty(max(int(T.csr_add_edges_workspace_bytes(n, n_dst)), 1), dtype=torch.uint8,
                     device=dev)
    T.csr_add_edges(indptr, indices, eids, src_new, dst_new, n_src, n_dst, ws, indptr_o,
                    indices_o, eids_o, status)
    if dev.type != "meta":
        _total, bad = status.tolist()
        if bad:
            raise ValueError(f"csr_add_edges: a node id lies outside [0, {n_src}) x "
                             f"[0, {n_dst})")
    indptr_o._gnnrec_nnz = E + n
    return indptr_o, indices_o, eids_o


def frontier_mark(rows: torch.Tensor, indptr: torch.Tensor, indices: torch.Tensor,
                  mark: torch.Tensor, n_rows: Optional[torch.Tensor] = None,
                  check: bool = True) -> torch.Tensor:
    """mark[indices[p]] = 1 for every slot p of the listed rows of a SOURCE-major CSR
    (gnnrec_frontier_mark): the destinations of the out-edges of `rows` (ascending, distinct
    int64 ids), without a neighbour list and balanced by edge.  mark int32 [n_dst] is written
    in place (words not marked keep their value); n_rows (one device int64, optional): only
    the first min(n_rows, len(rows)) rows count.  -> the two status words (device).  check:
    read them back and raise ValueError on a row outside [0, n_src) — nothing is marked then —
    or a neighbour id outside [0, n_dst); check=False leaves the readback to the caller."""
    T = _T()
    for t, n, dt in ((rows, "rows", torch.int64), (indptr, "indptr", torch.int64),
                     (indices, "indices", torch.int32), (mark, "mark", torch.int32)):
        _dev(t, n, dt)
    if n_rows is not None:
        _dev(n_rows, "n_rows", torch.int64)
    if rows.dim() != 1 or mark.dim() != 1 or not mark.is_contiguous():
        raise ValueError("frontier_mark: rows and mark must be 1-D, mark contiguous")
    dev = rows.device
    status = torch.empty(2, dtype=torch.int64, device=dev)
    ws = torch.empty(max(int(T.frontier_mark_workspace_bytes(rows.numel())), 1),
                     dtype=torch.uint8, device=dev)
    T.frontier_mark(rows.contiguous(), n_rows, indptr.contiguous(), indices.contiguous(), mark, ws,
                    status)
    if check and dev.type != "meta":
        frontier_status(status, indptr.numel() - 1, mark.numel())
    return status


def frontier_status(status, n_src: int, n_dst: int) -> None:
    """Raise ValueError on the status words of a frontier_mark call (a tensor or two ints)."""
    bad_row, bad_nbr = status.tolist() if isinstance(status, torch.Tensor) else status
    if bad_row:
        raise ValueError(f"frontier_mark: a listed row lies outside [0, {n_src})")
    if bad_nbr:
        raise ValueError(f"frontier_mark: a neighbour id lies outside [0, {n_dst})")


def membership_csr(src: torch.Tensor, dst: torch.Tensor, n_src: int, n_dst: int):
    """The dst-major CSR of (src, dst) with every row's source ids ascending — what
    has_edges searches.  Two stable radix sorts of the library (gnnrec_csr_build): by source
    (edge ids grouped by source), then by destination over the edges in that order, so the
    second sort's stability leaves each row sorted by source.  -> (indptr, sorted_indices)."""
    _dev(src, "src", torch.int64)
    _dev(dst, "dst", torch.int64)
    if src.numel() == 0:
        return torch.zeros(n_dst + 1, dtype=torch.int64, device=src.device), \
            torch.zeros(0, dtype=torch.int32, device=src.device)
    _, _, by_src = csr_build(dst, src, n_src)
    indptr, indices, _ = csr_build(gather_rows(src, by_src), gather_rows(dst, by_src), n_dst)
    return indptr, indices


def has_edges(indptr: torch.Tensor, sorted_indices: torch.Tensor, n_src: int,
              u: torch.Tensor, v: torch.Tensor) -> torch.Tensor:
    """K10: bool [n], (u[i] -> v[i]) is an edge of the relation whose membership_csr is
    (indptr, sorted_indices) (gnnrec_csr_has_edges: one binary search per query)."""
    _dev(indptr, "indptr", torch.int64)
    u = torch.as_tensor(u, dtype=torch.int64, device=indptr.device).reshape(-1).contiguous()
    v = torch.as_tensor(v, dtype=torch.int64, device=indptr.device).reshape(-1).contiguous()
    if u.numel() != v.numel():
        raise ValueError(f"has_edges: {u.numel()} sources for {v.numel()} destinations")
    out = torch.empty(u.numel(), dtype=torch.bool, device=indptr.device)
    if u.numel():
        _T().csr_has_edges(indptr, sorted_indices, int(n_src), u, v, out)
    return out


def csr_from_keys(keys: torch.Tensor, n_rows: int):
    """Rows of a COO list: -> (indptr int64 [n_rows+1], perm int32 [E]) with perm the edge
    ids grouped by keys[e] (ascending edge id inside a row).  keys: int32/int64 in [0, n_rows)."""
    T = _T()
    if keys.dtype != torch.int32:
        keys = keys.to(torch.int32)
    _dev(keys, "keys", torch.int32)
    keys = keys.contiguous()
    dev, E = keys.device, keys.numel()
    ip = torch.empty(n_rows + 1, dtype=torch.int64, device=dev)
    perm = torch.empty(E, dtype=torch.int32, device=dev)
    nbytes = int(T.csr_from_keys_workspace_bytes(E, n_rows))
    ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
    T.csr_from_keys(keys, n_rows, ws, ip, perm)
    ip._gnnrec_nnz = E
    return ip, perm


def add_(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """a += b (same shape, contiguous fp32) with the library's add kernel; returns a."""
    _dev(a, "a", torch.float32)
    _dev(b, "b", torch.float32)
    if a.shape != b.shape or not (a.is_contiguous() and b.is_contiguous()):
        raise ValueError("add_: operands must be contiguous and of one shape")
    _T().add_(a, b)
    return a


def tree_sum_(parts) -> torch.Tensor:
    """parts[0] = ((p0+p1)+(p2+p3))+... over 2, 4 or 8 same-shape contiguous fp32 tables in
    one kernel pass (gnnrec_tree_sum_f32): the same additions, in the same order, as
    pairwise add_ launches level by level; returns parts[0]."""
    n = len(parts)
    if n not in (2, 4, 8):
        raise ValueError("tree_sum_: 2, 4 or 8 tables")
    a = parts[0]
    for p in parts:
        _dev(p, "part", torch.float32)
        if p.shape != a.shape or not p.is_contiguous():
            raise ValueError("tree_sum_: operands must be contiguous and of one shape")
    _T().tree_sum_(a, list(parts[1:]))
    return a


def l2_normalize_rows(y: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out = y / ‖y‖ per row, rows with ‖y‖ == 0 unchanged (src/model.py:230-235), one
    wave per row (gnnrec_row_epilogue_f32)."""
    _dev(y, "y", torch.float32)
    M, N = y.shape
    _rowmajor(y, "y")
    if out is None:
        out = torch.empty((M, N), dtype=torch.float32, device=y.device)
    _T().row_epilogue(y, 1, ACCUM["store"], 0.0, None, None, out)
    return out


def spmm_backward(indptr, indices, grad_out, reduce, edge_weight=None, X=None, out=None,
                  grad_X=None, n_src=None):
    """Gradient of spmm w.r.t. its source rows (accumulated into grad_X, created if None).
    sum / mean: the float-atomic scatter (autograd uses the transposed gather instead);
    max: bitwise repeatable (_spmm_max_backward), unless GNNREC_SPMM_BWD=atomic asks for the
    scatter as it does for sum / mean in autograd.SpmmFn (faster, not repeatable)."""
    _dev(grad_out, "grad_out", torch.float32)
    n_dst, d = grad_out.shape
    if reduce == "max" and os.environ.get("GNNREC_SPMM_BWD") != "atomic":
        return _spmm_max_backward(indptr, indices, grad_out.contiguous(), edge_weight, X, out,
                                  grad_X, n_src)
    if grad_X is None:
        grad_X = torch.zeros((n_src, d), dtype=torch.float32, device=grad_out.device)
    grad_out = grad_out.contiguous()
    _T().spmm_backward(indptr, indices, edge_weight, grad_out, X, out, REDUCE[reduce], grad_X)
    return grad_X


def _spmm_max_backward(indptr, indices, grad_out, edge_weight, X, out, grad_X, n_src):
    """The max reducer's gradient, bitwise repeatable.  gnnrec_spmm_backward_f32 routes column
    c of destination v to the FIRST edge of v whose message equals the forward maximum and
    adds it into that edge's source row with a float atomic: a source row that several
    destinations route to was summed in launch order.  Here the same kernel runs over the
    edges as their own sources (source e = row e of the gathered messages), so every (edge,
    column) is written at most once and no two adds meet; the per-edge gradients are then
    summed per source row by the sum gather over the source-major CSR (stable sort of the
    source ids: ascending edge order inside a row), as the sum / mean backward does.  Costs
    two [E, d] tables for the duration of the call and about twice the scatter's time (5.7
    against 2.7 ms on 7.3M edges at d = 128, tools/bench_spmm_bwd.py).  A cheaper form would
    record the arg-max edge per (destination, column) in the forward or in one pass and gather
    over the source-major CSR, without the gathered messages and the [E, d] zero fill."""
    if X is None or out is None:
        raise ValueError("spmm_backward: max needs the forward input X and output out")
    _dev(indices, "indices", torch.int32)
    E, d = indices.numel(), grad_out.shape[1]
    rows = grad_X.shape[0] if grad_X is not None else int(n_src)
    dev = grad_out.device
    if E == 0:
        return grad_X if grad_X is not None else torch.zeros((rows, d), dtype=torch.float32,
                                                             device=dev)
    msgs = gather_rows(X, indices.to(torch.int64))  # [E, d]: row e = the message of edge e
    g_edge = torch.zeros((E, d), dtype=torch.float32, device=dev)
    _T().spmm_backward(indptr, torch.arange(E, dtype=torch.int32, device=dev), edge_weight,
                       grad_out, msgs, out, REDUCE["max"], g_edge)
    ip_t, perm = csr_from_keys(indices, rows)
    g = spmm(ip_t, perm, g_edge, "sum")
    if grad_X is None:
        return g
    if grad_X.is_contiguous():
        return add_(grad_X, g)
    grad_X += g
    return grad_X


# ---- packed rows of a ReLU-sparse table (csrc/pack_rows.hpp, pack_rows.hip) --------------
PACK_D = 128           # columns of a packable table
PACK_WORDS = 96        # int32 words per packed row (384 B)
PACK_SLOTS = 88        # values a packed row holds; above: a `dense` row
PACK_DENSE_BIT = 1 << 31
PACK_MAX_DENSE_FRAC = 1.0 / 8  # kPackMaxDenseFrac


class PackedRows:
    """A packed copy of a dense [n, 128] fp32 table: `data` int32 [n, 96], `status` int32 [4]
    ({packed_ok, dense rows, two counters of the pack kernel}) and the dense table `X` itself,
    which rows that do not fit are read from.  The buffers are allocated once and refilled
    by pack_rows(X, into=...)."""

    def __init__(self, n: int, device):
        self.data = torch.empty((n, PACK_WORDS), dtype=torch.int32, device=device)
        self.status = torch.zeros(4, dtype=torch.int32, device=device)
        self.X = None

    def rows(self, lo: int, hi: int) -> "PackedRows":
        """Rows [lo, hi) of the table (a source tile's slice), sharing the buffers."""
        v = object.__new__(PackedRows)
        v.data, v.status, v.X = self.data[lo:hi], self.status, self.X[lo:hi]
        return v


def pack_rows(X: torch.Tensor, into: Optional[PackedRows] = None,
              max_dense_frac: Optional[float] = None) -> PackedRows:
    """Pack the dense table X [n, 128] (gnnrec_pack_rows_f32) on the current stream.
    packed_ok = 1 iff at most max_dense_frac * n rows have more than 88 non-zeros."""
    _dev(X, "X", torch.float32)
    _rowmajor(X, "X")
    n, d = X.shape
    if d != PACK_D:
        raise ValueError(f"pack_rows: packed rows are {PACK_D} wide (got {d})")
    if into is None:
        into = PackedRows(n, X.device)
    elif into.data.shape[0] != n or into.data.device != X.device:
        raise ValueError("pack_rows: `into` was allocated for another table")
    _T().pack_rows_f32(X, -1.0 if max_dense_frac is None else float(max_dense_frac), into.data,
                       into.status)
    into.X = X
    return into


def pack_rows_host(x):
    """(packed uint32 [n, 96], dense rows) of a numpy fp32 [n, 128] table, on the host."""
    import numpy as np
    x = np.ascontiguousarray(x, dtype=np.float32)
    p, dense = _T().pack_rows_host(torch.from_numpy(x))
    return p.numpy().view(np.uint32), int(dense)


def unpack_rows_host(p, x_dense):
    """The fp32 [n, 128] table that `p` packs (`dense` rows copied from x_dense), on the host."""
    import numpy as np
    p = np.ascontiguousarray(p, dtype=np.uint32).view(np.int32)
    x_dense = np.ascontiguousarray(x_dense, dtype=np.float32)
    return _T().unpack_rows_host(torch.from_numpy(p), torch.from_numpy(x_dense)).numpy()


def spmm_packed(indptr: torch.Tensor, indices: torch.Tensor, packed: PackedRows,
                reduce: str = "mean", out: Optional[torch.Tensor] = None,
                split: Optional[int] = DEFAULT_SPLIT, accumulate: bool = False) -> torch.Tensor:
    """spmm(indptr, indices, packed.X, reduce) gathering from the packed copy of the table
    (gnnrec_spmm_csr_packed_f32): bitwise the same result.  sum / mean, no edge weights."""
    _dev(indptr, "indptr", torch.int64)
    _dev(indices, "indices", torch.int32)
    X = packed.X
    if reduce not in ("sum", "mean"):
        raise ValueError(f"spmm_packed: reduce {reduce!r} (sum or mean)")
    n_dst = indptr.numel() - 1
    if out is None:
        if accumulate:
            raise ValueError("spmm_packed: accumulate needs out")
        out = torch.empty((n_dst, PACK_D), dtype=torch.float32, device=X.device)
    else:
        _dev(out, "out", torch.float32)
        if tuple(out.shape) != (n_dst, PACK_D):
            raise ValueError(f"out must be [{n_dst}, {PACK_D}]")
    flags = _lib.SPMM_ACCUM if accumulate else 0
    heavy = chunk_ptr = chunk_row = counts = ws = None
    n_heavy = n_chunks = 0
    if split and getattr(indptr, "_gnnrec_split_plan", None) is None and \
            getattr(indptr, "_gnnrec_nnz", None) is not None:
        dplan = _device_plan(indptr, split)  # built on the device: {counts, rows, ptr, row}
        if dplan is not None:
            pl, n_heavy, n_chunks = dplan
            counts, heavy = pl, pl[2:]
            chunk_ptr, chunk_row = pl[2 + n_heavy:], pl[3 + 2 * n_heavy:]
        else:
            split = None
    elif split:
        plan = split_plan(indptr, split)
        if plan is not None:
            heavy, chunk_ptr, chunk_row, n_chunks = plan
            n_heavy = heavy.numel()
    if n_heavy:
        ws = torch.empty((n_chunks, PACK_D), dtype=torch.float32, device=X.device)
    _T().spmm_csr_packed_f32(indptr, indices, packed.data, packed.status, X, REDUCE[reduce], flags,
                             split or 0, heavy, n_heavy, chunk_ptr, chunk_row, n_chunks, counts,
                             out, ws)
    return out


# ---- training dropout with a counter-based mask (csrc/dropout.hpp, dropout.hip) ----------
def dropout_mask_host(seed: int, step: int, stream: int, n_rows: int, d: int, p: float):
    """The keep mask of (seed, step, stream) as a numpy bool [n_rows, d], computed on the
    host by the library (gnnrec_dropout_mask_host): what every dropout kernel regenerates."""
    import numpy as np
    lib = _lib.load()
    keep = np.empty((n_rows, d), dtype=np.uint8)
    mask64 = 0xFFFFFFFFFFFFFFFF
    _lib.check(lib.gnnrec_dropout_mask_host(seed & mask64, step & mask64, stream & mask64, n_rows,
                                            d, float(p), keep.ctypes.data),
               "gnnrec_dropout_mask_host")
    return keep.astype(bool)


def dropout_scale(p: float) -> float:
    """65536 / (65536 - round(p * 65536)): what kept elements are multiplied by."""
    return float(_lib.load().gnnrec_dropout_scale(float(p)))


def dropout_keys(seed: int, counter: torch.Tensor, n_streams: int, stream0: int = 0):
    """keys[i] = hash3(seed, counter, stream0 + i) as an int64 device tensor, and counter += 1
    on the device, in one launch (gnnrec_dropout_keys)."""
    _dev(counter, "counter", torch.int64)
    keys = torch.empty(n_streams, dtype=torch.int64, device=counter.device)
    _T().dropout_keys(_lib.i64(seed), counter, stream0, keys)
    return keys


def dropout_rows(x: torch.Tensor, keys: torch.Tensor, key_index: int, p: float, n=None,
                 out: Optional[torch.Tensor] = None, accumulate: bool = False) -> torch.Tensor:
    """out[:n] (+)= x[:n] ⊙ mask · scale with the key keys[key_index] (n: every row)."""
    _dev(x, "x", torch.float32)
    n = x.shape[0] if n is None else n
    if out is None:
        if accumulate:
            raise ValueError("dropout_rows: accumulate needs out")
        out = torch.empty((n, x.shape[1]), dtype=torch.float32, device=x.device)
    _T().dropout_rows_f32(x, n, keys, key_index, float(p), accumulate, out)
    return out


def spmm_dropout(indptr, indices, X, reduce: str, keys, key_index: int, p: float, where: str,
                 edge_weight=None, out=None, accumulate: bool = False, live=None, nnz=None,
                 split: int = DEFAULT_SPLIT):
    """The sum / mean gather with the dropout mask inside: where='src' masks every gathered
    row of X (the training forward), where='out' masks the output row at its store (the
    backward over the source-major CSR; under accumulate only this call's contribution).
    Heavy rows are planned on the device from the edge count, as the training backward's."""
    _dev(X, "X", torch.float32)
    if out is None:
        if accumulate:
            raise ValueError("spmm_dropout: accumulate needs out")
        out = torch.empty((indptr.numel() - 1, X.shape[1]), dtype=torch.float32, device=X.device)
    nnz = _nnz(indptr) if nnz is None else nnz
    T = _T()
    n, d = indptr.numel() - 1, X.shape[1]
    side = {"src": _lib.DROPOUT_SRC, "out": _lib.DROPOUT_OUT}[where]
    flags = _lib.SPMM_ACCUM if accumulate else 0
    cap_h = min(n, nnz // (split + 1))
    if cap_h <= 0:  # no row can exceed the split
        T.spmm_csr_dropout_live_f32(indptr, indices, edge_weight, X, REDUCE[reduce], flags, out,
                                    live, keys, key_index, float(p), side)
        return out
    cap_c = nnz // split + cap_h
    plan = torch.empty(3 + 2 * cap_h + cap_c, dtype=torch.int64, device=X.device)
    T.spmm_plan_build(indptr, split, cap_h, plan, live)
    ws = torch.empty((cap_c, d), dtype=torch.float32, device=X.device)
    T.spmm_csr_planned_dropout_live_f32(indptr, indices, edge_weight, X, REDUCE[reduce], flags,
                                        split, plan, cap_h, cap_c, out, ws, live, keys,
                                        key_index, float(p), side)
    return out


def gemm(A1: torch.Tensor, W1: torch.Tensor, A2: Optional[torch.Tensor] = None,
         W2: Optional[torch.Tensor] = None, bias: Optional[torch.Tensor] = None, *,
         relu: bool = False, l2norm: bool = False, sigmoid: bool = False,
         accum: str = "store", out_div: float = 0.0, out: Optional[torch.Tensor] = None,
         a2_deg: Optional[torch.Tensor] = None, a2_mode: int = _lib.A2_NONE,
         attn_vec: Optional[torch.Tensor] = None,
         attn_state: Optional[torch.Tensor] = None,
         bias_nonempty: Optional[torch.Tensor] = None,
         row_norm: Optional[torch.Tensor] = None) -> torch.Tensor:
    """a2/a3/a4: out (accum)= epi(A1 W1ᵀ + T(A2) W2ᵀ + bias [+ bias_nonempty where
    a2_deg > 0]).  W are nn.Linear weights [N, K].  row_norm [M] (with l2norm, N <=
    GEMM_ROW_N): receives each row's norm before the normalisation (training)."""
    T = _T()
    _dev(A1, "A1", torch.float32)
    _dev(W1, "W1", torch.float32)
    M, K1 = A1.shape
    N = W1.shape[0]
    if W1.shape[1] != K1:
        raise ValueError(f"W1 shape {tuple(W1.shape)} does not match A1 K={K1}")
    W1 = W1.detach().contiguous()
    _rowmajor(A1, "A1")
    if A2 is not None:
        _dev(A2, "A2", torch.float32)
        _dev(W2, "W2", torch.float32)
        if A2.shape[0] != M or W2.shape[0] != N or W2.shape[1] != A2.shape[1]:
            raise ValueError("A2/W2 shape mismatch")
        _rowmajor(A2, "A2")
        W2 = W2.detach().contiguous()
    if bias is not None:
        _dev(bias, "bias", torch.float32)
        bias = bias.detach().contiguous()
    if a2_mode != _lib.A2_NONE or bias_nonempty is not None:
        _dev(a2_deg, "a2_deg", torch.int32)
    if bias_nonempty is not None:
        _dev(bias_nonempty, "bias_nonempty", torch.float32)
        bias_nonempty = bias_nonempty.detach().contiguous()
    epi = (_lib.EPI_RELU if relu else 0) | (_lib.EPI_L2NORM if l2norm else 0) | (
        _lib.EPI_SIGMOID if sigmoid else 0)
    if out is None:
        if accum not in ("store", "attn_first"):
            raise ValueError("accumulating gemm needs an out tensor")
        out = torch.empty((M, N), dtype=torch.float32, device=A1.device)
    else:
        _dev(out, "out", torch.float32)
        if tuple(out.shape) != (M, N):
            raise ValueError(f"out must be [{M}, {N}]")
    _rowmajor(out, "out")
    av, ast = _attn_args(accum, attn_vec, attn_state, M, N)
    if row_norm is not None:
        _dev(row_norm, "row_norm", torch.float32)
        if not l2norm or N > GEMM_ROW_N or row_norm.numel() != M or not row_norm.is_contiguous():
            raise ValueError(f"row_norm needs l2norm, N <= {GEMM_ROW_N} and a contiguous [{M}]")
    if N > GEMM_ROW_N and (l2norm or av is not None):
        # the row norm / attention score needs the whole row: GEMM (bias, ReLU, sigmoid)
        # into a scratch table, then one row-epilogue pass into out
        z = gemm(A1, W1, A2, W2, bias, relu=relu, sigmoid=sigmoid, a2_deg=a2_deg,
                 a2_mode=a2_mode, bias_nonempty=bias_nonempty)
        T.row_epilogue(z, int(l2norm), ACCUM[accum], float(out_div), av, ast, out)
        return out
    T.gemm(A1, W1, A2, W2, a2_deg, a2_mode, bias, bias_nonempty, epi, ACCUM[accum],
           float(out_div), av, ast, out, row_norm)
    return out


FUSED_D = 128  # gnnrec_spmm_project_f32 handles d_neigh = d_self = out = 128
GEMM_ROW_N = 256  # widest output row gnnrec_gemm_f32 normalises / attends in one block


def can_spmm_project(indptr, X, H, W_self, W_neigh, split: Optional[int] = DEFAULT_SPLIT,
                     avg_deg: Optional[float] = None, gemm_overlaps: bool = False) -> bool:
    """True when a fused aggregation+projection kernel applies (shapes, alignment, no
    heavy rows, GPU tensors).  avg_deg: edges per row to judge
    the degree threshold by (default: this CSR's own).  gemm_overlaps: the caller can run
    an unfused projection GEMM on a second stream under other HBM-bound work (the sharded
    pass) — then low-degree CSRs, whose fused kernel is the MFMA one, stay unfused: the
    overlapped GEMM costs less than the MFMA kernel's extra time over the bare gather
    (C5 bought-by: 13.1 ms fused vs 7.6 ms gather + a 7.1 ms GEMM on the side stream)."""
    D = FUSED_D
    if not ((X.is_cuda or X.is_meta) and (H.is_cuda or H.is_meta) and X.dim() == 2
            and H.dim() == 2):
        return False
    if X.shape[1] != D or H.shape[1] != D or tuple(W_self.shape) != (D, D) or \
            tuple(W_neigh.shape) != (D, D):
        return False
    if X.dtype != torch.float32 or H.dtype != torch.float32:
        return False
    for t in (X, H):
        if t.stride(1) != 1 or t.stride(0) % 4:
            return False
        # 16-B aligned rows; torch.compile's fake tensors have no address (there the
        # library's own alignment check is what refuses a misaligned view, loudly)
        if not torch.compiler.is_compiling() and t.data_ptr() % 16:
            return False
    route = getattr(indptr, "_gnnrec_route", None)
    if route is not None and split == DEFAULT_SPLIT:
        if route.has_split:  # a row subset follows the whole relation's heavy rows
            return False
    elif split and split_plan(indptr, split) is not None:
        return False
    # below FUSED_MIN_DEG edges per row the VALU kernel's per-row weight reads bound it and
    # the MFMA variant takes the relation (C5 bought-by, 10 edges/row: VALU-fused 18.0 ms,
    # MFMA-fused 13.1 ms, spmm 7.6 + GEMM 7.1 ms back to back); GNNREC_FUSED_MFMA=0 keeps
    # aggregation + GEMM there
    if os.environ.get("GNNREC_FUSED_MFMA", "1") == "0" or gemm_overlaps:
        return fused_variant(indptr, avg_deg) == "valu"
    return True


def fused_preprojects(indptr, X, H, reduce: str, avg_deg: Optional[float] = None) -> bool:
    """A fused launch that can_spmm_project accepted runs the pre-projected form: the MFMA
    variant, a linear reduce and a source table at most half the destination count."""
    return fused_variant(indptr, avg_deg) == "mfma" and preproject_pays(
        X.shape[0], routed_n_dst(indptr, indptr.numel() - 1), reduce)


FUSED_MIN_DEG = 24


class Route(NamedTuple):
    """The whole relation's figures the kernel choice depends on, hung on the indptr of a
    CSR that holds only some of its rows (`indptr._gnnrec_route`, pin_route): a row computes
    from its own inputs alone, so a subset that takes the whole relation's route gives the
    whole pass's bits (inference.IncrementalEmbeddings).  A CSR without the
    attribute decides from itself, as ever."""
    avg_deg: float    # edges per destination row (fused_variant)
    n_dst: int        # destination rows (preproject_pays)
    has_split: bool   # some row exceeds DEFAULT_SPLIT edges (can_spmm_project)


def relation_route(indptr: torch.Tensor) -> Route:
    """The Route of a whole relation's dst-major CSR, by the rules the helpers below apply to
    it (a host readback for the heavy-row plan unless the CSR has one cached)."""
    n = indptr.numel() - 1
    avg = _nnz(indptr) / n if n else float(FUSED_MIN_DEG)
    return Route(avg, n, split_plan(indptr, DEFAULT_SPLIT) is not None)


def pin_route(indptr: torch.Tensor, route: Route, nnz: int) -> torch.Tensor:
    """Mark `indptr` (a row subset's CSR of `nnz` edges) to take `route`."""
    indptr._gnnrec_nnz = int(nnz)
    indptr._gnnrec_route = route
    return indptr


def routed_n_dst(indptr: torch.Tensor, n_dst: int) -> int:
    """The destination count to route by: the pinned whole relation's, else n_dst."""
    route = getattr(indptr, "_gnnrec_route", None)
    return n_dst if route is None else route.n_dst


def fused_variant(indptr, avg_deg: Optional[float] = None) -> str:
    """'valu' (gnnrec_spmm_project_f32: weights in LDS, read once per 2 rows — bound by
    the gather from FUSED_MIN_DEG edges per row up) or 'mfma' (gnnrec_spmm_project_mfma_f32:
    32-row tiles through fp32 MFMA, weights read once per 32 rows — low degrees).  avg_deg:
    the edges per row to decide by (the sharded pass passes the GLOBAL average so every
    rank picks the same kernel); default this CSR's own (spmm_project's `variant` forces
    one)."""
    if avg_deg is None:
        route = getattr(indptr, "_gnnrec_route", None)
        if route is not None:
            avg_deg = route.avg_deg
        else:
            n = indptr.numel() - 1
            avg_deg = _nnz(indptr) / n if n else float(FUSED_MIN_DEG)
    return "valu" if avg_deg >= FUSED_MIN_DEG else "mfma"


def _nnz(indptr: torch.Tensor) -> int:
    """indptr[-1] as a host int, read back once per CSR (cached on the tensor)."""
    v = getattr(indptr, "_gnnrec_nnz", None)
    if v is None:
        v = int(indptr[-1].item())
        try:
            indptr._gnnrec_nnz = v
        except AttributeError:  # pragma: no cover
            pass
    return v


def _wkey(W: torch.Tensor):
    return (W._version, W.data_ptr(), getattr(W, "_gnnrec_epoch", 0))


def invalidate_weight_cache(*modules_or_tensors) -> None:
    """Drop the transposed / packed weight copies the fused kernels keep on weight tensors.
    They are rebuilt when a weight's version counter moves (every in-place op through the
    autograd-visible tensor: optimizer steps, `with torch.no_grad(): W.copy_(...)`); a write
    through `W.data` (EMA or custom update code) does not move it — call this afterwards
    with the modules or tensors written."""
    for m in modules_or_tensors:
        ts = m.parameters() if isinstance(m, torch.nn.Module) else [m]
        for W in ts:
            try:
                W._gnnrec_epoch = getattr(W, "_gnnrec_epoch", 0) + 1
            except (AttributeError, RuntimeError):  # pragma: no cover
                pass


def _cached_on(W: torch.Tensor, attr: str, key, make):
    """A derived copy of weight W kept as W.<attr>, rebuilt when `key` changes.  Handed to
    another stream than the one that made it, the consumer first waits for its making and
    the copy is record_stream-ed there (so replacing it never frees memory a side-stream
    kernel is still reading)."""
    if torch.cuda.is_current_stream_capturing():
        # inside a captured step (gnnrec.capture): the copy is made by the graph on every
        # replay, after the captured optimizer step changed W — never a stale cached one
        return make()
    hit = getattr(W, attr, None)
    cur = torch.cuda.current_stream(W.device)
    if hit is None or hit[0] != key:
        ev = torch.cuda.Event()
        hit = (key, make(), ev, cur.cuda_stream)
        ev.record(cur)
        try:
            setattr(W, attr, hit)
        except (AttributeError, RuntimeError):  # pragma: no cover
            pass
    elif hit[3] != cur.cuda_stream:  # made on another stream: ordered after its copy
        cur.wait_event(hit[2])
        hit[1].record_stream(cur)
    return hit[1]


def _transposed(W: torch.Tensor) -> torch.Tensor:
    """Wᵀ (k-major, contiguous) of a fused kernel's weight, kept on the weight tensor and
    rebuilt only when the weight changes (its version counter, an optimizer step, or
    invalidate_weight_cache) — not a transpose-copy kernel per launch inside the pass (C4:
    two per layer before the fused launch, profiles/r02f_c4_timeline.txt)."""
    if torch.compiler.is_compiling() or not W.is_cuda:
        return W.detach().t().contiguous()
    return _cached_on(W, "_gnnrec_wt", _wkey(W), lambda: W.detach().t().contiguous())


def _packed4(Ws_a, Wn_a, Ws_b, Wn_b) -> torch.Tensor:
    """[W_self,aᵀ | W_neigh,aᵀ | W_self,bᵀ | W_neigh,bᵀ] as one contiguous [4, d, d] k-major
    array (gnnrec_spmm_pair_f32's WT4), cached on W_self,a like _transposed."""
    Ws = (Ws_a, Wn_a, Ws_b, Wn_b)

    def make():
        return torch.stack([W.detach().t() for W in Ws]).contiguous()

    if torch.compiler.is_compiling() or not Ws_a.is_cuda:
        return make()
    return _cached_on(Ws_a, "_gnnrec_wt4", tuple(_wkey(W) for W in Ws), make)


def spmm_project(indptr, indices, X, H, W_self, W_neigh, reduce: str = "mean",
                 edge_weight: Optional[torch.Tensor] = None, relu: bool = True,
                 l2norm: bool = False, accum: str = "store", out_div: float = 0.0,
                 out: Optional[torch.Tensor] = None, bias: Optional[torch.Tensor] = None,
                 bias_nonempty: Optional[torch.Tensor] = None,
                 attn_vec: Optional[torch.Tensor] = None,
                 attn_state: Optional[torch.Tensor] = None,
                 avg_deg: Optional[float] = None, variant: Optional[str] = None,
                 agg: Optional[torch.Tensor] = None,
                 agg_mode: Optional[str] = None) -> torch.Tensor:
    """a1+a3 fused: out (accum)= epi(H W_selfᵀ + reduce_e X[src_e] W_neighᵀ + bias
    + [deg > 0]·bias_nonempty), d = 128.  variant 'valu' | 'mfma' (default: fused_variant
    of avg_deg) picks the kernel; both give the same aggregate bits, the projection's
    fp32 summation order differs.

    W_neigh None: X holds pre-projected source rows (preproject(X, W_neigh)) and the
    neighbour term is reduce_e X[src_e] itself (sum / mean only; the mfma kernel, which
    then runs only the self half on the MFMA).  The same value up to fp32 rounding: the
    projection is applied before the (linear) reduction instead of after it.

    agg_mode 'save' | 'load' with agg [n_dst, 128] (the valu kernel only): the rows'
    aggregates reduce_e X[src_e] — which no weight enters — are also written to agg ('save':
    spmm's bits for the same CSR and reduce), or read from it instead of gathered ('load':
    indices, X and edge_weight are not read and may be None).  `out` has the same bits as the
    plain launch's on the same aggregate."""
    if agg_mode not in (None, "save", "load"):
        raise ValueError(f"spmm_project agg_mode must be 'save' or 'load', not {agg_mode!r}")
    if (agg is None) != (agg_mode is None):
        raise ValueError("spmm_project: agg and agg_mode go together")
    load = agg_mode == "load"
    _dev(indptr, "indptr", torch.int64)
    if not load or indices is not None:
        _dev(indices, "indices", torch.int32)
    if not load or X is not None:
        _dev(X, "X", torch.float32)
    _dev(H, "H", torch.float32)
    n_dst = indptr.numel() - 1
    if H.shape[0] < n_dst:
        raise ValueError(f"H has {H.shape[0]} rows, the CSR {n_dst} destinations")
    if edge_weight is not None:
        _dev(edge_weight, "edge_weight", torch.float32)
        edge_weight = edge_weight.contiguous()
    D = FUSED_D
    if out is None:
        if accum not in ("store", "attn_first"):
            raise ValueError("accumulating spmm_project needs an out tensor")
        out = torch.empty((n_dst, D), dtype=torch.float32, device=H.device)
    else:
        _dev(out, "out", torch.float32)
        if tuple(out.shape) != (n_dst, D):
            raise ValueError(f"out must be [{n_dst}, {D}], got {tuple(out.shape)}")
    if tuple(W_self.shape) != (D, D) or (W_neigh is not None
                                         and tuple(W_neigh.shape) != (D, D)):
        raise ValueError(f"spmm_project needs {D}x{D} weights")
    if W_neigh is None:
        if reduce not in ("sum", "mean"):
            raise ValueError("pre-projected source rows (W_neigh None) need reduce sum or mean")
        if variant not in (None, "mfma"):
            raise ValueError("pre-projected source rows (W_neigh None) run on the mfma kernel")
        variant = "mfma"
    WsT = _transposed(W_self)
    WnT = None if W_neigh is None else _transposed(W_neigh)
    for t, name in ((bias, "bias"), (bias_nonempty, "bias_nonempty")):
        if t is not None:
            _dev(t, name, torch.float32)
            if t.numel() != D:
                raise ValueError(f"{name} must have {D} entries")
    bias = None if bias is None else bias.detach().contiguous()
    bias_nonempty = None if bias_nonempty is None else bias_nonempty.detach().contiguous()
    av, ast = _attn_args(accum, attn_vec, attn_state, n_dst, D)
    epi = (_lib.EPI_RELU if relu else 0) | (_lib.EPI_L2NORM if l2norm else 0)
    variant = variant or ("valu" if agg_mode is not None else fused_variant(indptr, avg_deg))
    if variant not in ("valu", "mfma"):
        raise ValueError(f"spmm_project variant must be 'valu' or 'mfma', not {variant!r}")
    if X is not None:
        _rowmajor(X, "X")
    _rowmajor(H, "H")
    _rowmajor(out, "out")
    if agg_mode is not None:
        if variant != "valu" or W_neigh is None:
            raise ValueError("spmm_project: agg_mode runs on the valu kernel")
        _dev(agg, "agg", torch.float32)
        if agg.dim() != 2 or tuple(agg.shape) != (n_dst, D):
            raise ValueError(f"agg must be [{n_dst}, {D}], got {tuple(agg.shape)}")
        _rowmajor(agg, "agg")
        if n_dst == 0:  # nothing to launch
            return out
        _T().spmm_project_agg_f32(indptr, indices, edge_weight, X, H, WsT, WnT, bias,
                                  bias_nonempty, REDUCE[reduce], epi, ACCUM[accum],
                                  float(out_div), av, ast, agg,
                                  _lib.AGG_LOAD if load else _lib.AGG_SAVE, out)
        return out
    _T().spmm_project(indptr, indices, edge_weight, X, H, WsT, WnT, bias, bias_nonempty,
                      REDUCE[reduce], epi, ACCUM[accum], float(out_div), av, ast,
                      variant == "mfma", out)
    return out


def spmm_project2(rel_a, rel_b, H, W_self_a, W_self_b, bias_a=None, bias_b=None, *,
                  relu: bool = True, l2norm: bool = False, combine: str = "add",
                  out_div: float = 0.0, out: Optional[torch.Tensor] = None,
                  attn_vec: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Two pre-projected relations into one destination type in one launch
    (gnnrec_spmm_project2_f32): out = combine(epi(H W_self_aᵀ + agg_a + bias_a
    [+ bias_nonempty_a]), epi(... b ...)) / out_div.  rel_r = (indptr, indices, Y,
    reduce, edge_weight, bias_nonempty) with Y = preproject(X_r, W_neigh_r); reduce sum
    or mean; combine 'add' (HeteroGraphConv sum, mean with out_div=2), 'max', or
    'attention' with attn_vec [d] (softmax over the two relations of attn_vec·y_r)."""
    D = FUSED_D
    args = []
    n_dst = rel_a[0].numel() - 1
    # the relation with at most half the other's edges (host counts only: no readback) reads
    # its source rows non-temporally, leaving the Infinity Cache to the busier table
    # (GNNREC_SRC_STREAM; C5: bought-by's 100M edges beside clicked-by's 400M)
    ea, eb = (getattr(r[0], "_gnnrec_nnz", None) for r in (rel_a, rel_b))
    stream = None
    if ea is not None and eb is not None and rel_a[4] is None and rel_b[4] is None:
        stream = "b" if 2 * eb <= ea else "a" if 2 * ea <= eb else None
    for name, (indptr, indices, Y, reduce, ew, bne) in (("a", rel_a), ("b", rel_b)):
        _dev(indptr, f"indptr_{name}", torch.int64)
        _dev(indices, f"indices_{name}", torch.int32)
        _dev(Y, f"Y{name}", torch.float32)
        _rowmajor(Y, f"Y{name}")
        if reduce not in ("sum", "mean"):
            raise ValueError("spmm_project2: pre-projected relations reduce by sum or mean")
        if indptr.numel() - 1 != n_dst:
            raise ValueError("spmm_project2: the relations' row counts differ")
        if ew is not None:
            _dev(ew, f"ew_{name}", torch.float32)
            ew = ew.contiguous()
        if bne is not None:
            _dev(bne, f"bias_nonempty_{name}", torch.float32)
            bne = bne.detach().contiguous()
        args += [indptr, indices, ew, Y,
                 REDUCE[reduce] | (_lib.SRC_STREAM if stream == name else 0), bne]
    _dev(H, "H", torch.float32)
    _rowmajor(H, "H")
    if combine not in ("add", "max", "attention"):
        raise ValueError(f"spmm_project2: combine must be 'add', 'max' or 'attention', "
                         f"not {combine!r}")
    if (combine == "attention") != (attn_vec is not None):
        raise ValueError("spmm_project2: attn_vec goes with combine='attention'")
    if attn_vec is not None:
        _dev(attn_vec, "attn_vec", torch.float32)
        if attn_vec.numel() != D:
            raise ValueError(f"attn_vec must have {D} entries")
        attn_vec = attn_vec.detach().contiguous()
    for W in (W_self_a, W_self_b):
        if tuple(W.shape) != (D, D):
            raise ValueError(f"spmm_project2 needs {D}x{D} weights")
    if out is None:
        out = torch.empty((n_dst, D), dtype=torch.float32, device=H.device)
    else:
        _dev(out, "out", torch.float32)
        _rowmajor(out, "out")
    bias_a = None if bias_a is None else bias_a.detach().contiguous()
    bias_b = None if bias_b is None else bias_b.detach().contiguous()
    epi = (_lib.EPI_RELU if relu else 0) | (_lib.EPI_L2NORM if l2norm else 0)
    _T().spmm_project2(*args, H, _transposed(W_self_a), _transposed(W_self_b), bias_a, bias_b,
                       epi,
                       ACCUM["attn_last" if combine == "attention" else combine], attn_vec,
                       float(out_div), out)
    return out


def spmm_pair(rel_a, rel_b, X, H, W_self_a, W_neigh_a, W_self_b, W_neigh_b, bias_a=None,
              bias_b=None, *, relu: bool = True, l2norm: bool = False, combine: str = "add",
              out_div: float = 0.0, out: Optional[torch.Tensor] = None,
              attn_vec: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Two relations gathering from ONE source table X into one destination type, all four
    projections in the launch (gnnrec_spmm_pair_f32, MFMA epilogue): out = combine(
    epi(H W_self_aᵀ + agg_a W_neigh_aᵀ + bias_a [+ bias_nonempty_a]), epi(... b ...)) /
    out_div.  rel_r = (indptr, indices, reduce, edge_weight, bias_nonempty), reduce sum or
    mean; combine as spmm_project2.  Unlike spmm_project2 nothing is pre-projected: the
    gathered working set is X alone; the projections run on the fp32 MFMA."""
    D = FUSED_D
    n_dst = rel_a[0].numel() - 1
    args = []
    for name, (indptr, indices, reduce, ew, bne), b in (("a", rel_a, bias_a), ("b", rel_b, bias_b)):
        _dev(indptr, f"indptr_{name}", torch.int64)
        _dev(indices, f"indices_{name}", torch.int32)
        if reduce not in ("sum", "mean"):
            raise ValueError("spmm_pair: both relations reduce by sum or mean")
        if indptr.numel() - 1 != n_dst:
            raise ValueError("spmm_pair: the relations' row counts differ")
        if ew is not None:
            _dev(ew, f"ew_{name}", torch.float32)
            ew = ew.contiguous()
        if bne is not None:
            _dev(bne, f"bias_nonempty_{name}", torch.float32)
            bne = bne.detach().contiguous()
        if b is not None:
            b = b.detach().contiguous()
        args += [indptr, indices, ew, REDUCE[reduce], b, bne]
    _dev(X, "X", torch.float32)
    _rowmajor(X, "X")
    _dev(H, "H", torch.float32)
    _rowmajor(H, "H")
    if X.shape[1] != D or H.shape[1] != D:
        raise ValueError(f"spmm_pair needs d = {D}")
    if combine not in ("add", "max", "attention"):
        raise ValueError(f"spmm_pair: combine must be 'add', 'max' or 'attention', "
                         f"not {combine!r}")
    if (combine == "attention") != (attn_vec is not None):
        raise ValueError("spmm_pair: attn_vec goes with combine='attention'")
    if attn_vec is not None:
        _dev(attn_vec, "attn_vec", torch.float32)
        if attn_vec.numel() != D:
            raise ValueError(f"attn_vec must have {D} entries")
        attn_vec = attn_vec.detach().contiguous()
    for W in (W_self_a, W_neigh_a, W_self_b, W_neigh_b):
        if tuple(W.shape) != (D, D):
            raise ValueError(f"spmm_pair needs {D}x{D} weights")
    if out is None:
        out = torch.empty((n_dst, D), dtype=torch.float32, device=H.device)
    else:
        _dev(out, "out", torch.float32)
        _rowmajor(out, "out")
    epi = (_lib.EPI_RELU if relu else 0) | (_lib.EPI_L2NORM if l2norm else 0)
    WT4 = _packed4(W_self_a, W_neigh_a, W_self_b, W_neigh_b)
    _T().spmm_pair(*args, X, H, WT4, epi,
                   ACCUM["attn_last" if combine == "attention" else combine], attn_vec,
                   float(out_div), out)
    return out


def preproject_pays(n_src: int, n_dst: int, reduce: str) -> bool:
    """Project a low-degree relation's source rows ahead of the reduction (spmm_project
    with W_neigh=None) when the reduction is linear and the source type has at most half
    as many rows as the destination: the MFMA then runs the self half only (C5 bought-by,
    1M items -> 10M users: fused 13.0 -> 10.6 ms + 0.38 ms for the 1M-row projection)."""
    return reduce in ("sum", "mean") and 2 * n_src <= n_dst


def preproject(X: torch.Tensor, W_neigh: torch.Tensor,
               out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Y = X W_neighᵀ: a relation's source rows projected ahead of its (linear) reduction,
    for spmm_project(..., W_neigh=None).  Worth it where the source type has fewer rows
    than the destination (C5 item -> user: 1M projected rows instead of 10M aggregates)."""
    return gemm(X, W_neigh, out=out)


def gemm_tn(A: torch.Tensor, B: torch.Tensor, out: Optional[torch.Tensor] = None,
            accumulate: bool = False, colsum: Optional[torch.Tensor] = None,
            row_ptr: Optional[torch.Tensor] = None) -> torch.Tensor:
    """f2 weight gradient: out [M,N] (+)= Aᵀ B for A [K,M], B [K,N] (dW = dYᵀ X); with
    colsum [M], also colsum (+)= Σ_k A[k] (the bias gradient) from the same pass — over the
    rows k with row_ptr[k+1] > row_ptr[k] only when row_ptr (an int64 [K+1] indptr) is given.

    Deterministic split-K MFMA (gnnrec_gemm_tn_bias_rows_f32)."""
    T = _T()
    _dev(A, "A", torch.float32)
    _dev(B, "B", torch.float32)
    K, M = A.shape
    if B.shape[0] != K:
        raise ValueError(f"gemm_tn: A {tuple(A.shape)} and B {tuple(B.shape)} differ in K")
    N = B.shape[1]
    _rowmajor(A, "A")
    _rowmajor(B, "B")
    if out is None:
        if accumulate:
            raise ValueError("accumulating gemm_tn needs an out tensor")
        out = torch.empty((M, N), dtype=torch.float32, device=A.device)
    else:
        _dev(out, "out", torch.float32)
        if tuple(out.shape) != (M, N):
            raise ValueError(f"out must be [{M}, {N}]")
    if colsum is not None:
        _dev(colsum, "colsum", torch.float32)
        if colsum.numel() != M or not colsum.is_contiguous():
            raise ValueError(f"colsum must be a contiguous [{M}] tensor")
    _rowmajor(out, "out")
    nbytes = T.gemm_tn_workspace_bytes(K, M, N)
    ws = torch.empty(max(1, nbytes // 4), dtype=torch.float32, device=A.device)
    if row_ptr is not None:
        _dev(row_ptr, "row_ptr", torch.int64)
        if colsum is None or row_ptr.numel() != K + 1:
            raise ValueError(f"row_ptr must be a [{K + 1}] indptr beside colsum")
        row_ptr = row_ptr.contiguous()
    T.gemm_tn(A, B, colsum, bool(accumulate), out, ws, row_ptr)
    return out


def act_backward_normed(z: torch.Tensor, row_norm: torch.Tensor, gz: torch.Tensor,
                        relu: bool = True) -> torch.Tensor:
    """f2: gradient through relu?+L2 norm from the normalised output z and the row norms
    gemm(..., l2norm=True, row_norm=...) wrote (gnnrec_act_backward_normed_f32)."""
    _dev(z, "z", torch.float32)
    _dev(gz, "gz", torch.float32)
    _dev(row_norm, "row_norm", torch.float32)
    n, d = z.shape
    if tuple(gz.shape) != (n, d) or row_norm.numel() != n:
        raise ValueError("act_backward_normed: shape mismatch")
    gu = torch.empty((n, d), dtype=torch.float32, device=z.device)
    _T().act_backward_normed(z, row_norm.contiguous(), gz, bool(relu), gu)
    return gu


def act_backward(u: torch.Tensor, gz: torch.Tensor, relu: bool, l2norm: bool,
                 out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """f2: gradient through z = norm?(relu?(u)) (zero-guarded row norm) for pre-activation u."""
    _dev(u, "u", torch.float32)
    _dev(gz, "gz", torch.float32)
    if gz.shape != u.shape:
        raise ValueError("act_backward: u and gz shapes differ")
    n, d = u.shape
    gz = gz.contiguous()
    if out is None:
        out = torch.empty_like(u)
    flags = (_lib.EPI_RELU if relu else 0) | (_lib.EPI_L2NORM if l2norm else 0)
    _T().act_backward(u, gz, flags, out)
    return out


class LstmPlan:
    """Degree-descending visiting order of a CSR's rows and the running-row count of
    every step (one host readback of the degree histogram, cached on the indptr)."""

    def __init__(self, indptr: torch.Tensor):
        deg = indptr[1:] - indptr[:-1]
        self.order = torch.argsort(deg, descending=True, stable=True)
        hist = torch.bincount(deg, minlength=1).tolist()
        n = indptr.numel() - 1
        running, steps = n - hist[0], []
        for t in range(len(hist) - 1):
            steps.append(running)
            running -= hist[t + 1]
        self.n_active = steps  # n_active[t] = #rows with in-degree > t
        self.n_rows = steps[0] if steps else 0

    @classmethod
    def of(cls, indptr):
        p = getattr(indptr, "_gnnrec_lstm_plan", None)
        if p is None:
            p = cls(indptr)
            indptr._gnnrec_lstm_plan = p
        return p


def lstm_aggregate(indptr, indices, X, W_ih, W_hh, b_ih, b_hh,
                   out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """f4: per destination, nn.LSTM over its in-neighbour rows of X in CSR (edge) order ->
    final hidden state [n_dst, d]; 0 for zero in-degree (ConvLayer._lstm_reducer)."""
    T = _T()
    _dev(indptr, "indptr", torch.int64)
    _dev(indices, "indices", torch.int32)
    d = W_hh.shape[1]
    n_dst = indptr.numel() - 1
    plan = LstmPlan.of(indptr)
    P = gemm(X.contiguous(), W_ih.detach(), bias=(b_ih + b_hh).detach())  # [N_src, 4d]
    if out is None:
        out = torch.zeros((n_dst, d), dtype=torch.float32, device=X.device)
    else:
        out.zero_()
    if plan.n_rows == 0:
        return out
    h = [torch.zeros((plan.n_rows, d), dtype=torch.float32, device=X.device),
         torch.empty((plan.n_rows, d), dtype=torch.float32, device=X.device)]
    c = torch.zeros((plan.n_rows, d), dtype=torch.float32, device=X.device)
    WT = W_hh.detach().t().contiguous()
    for t, n_act in enumerate(plan.n_active):
        T.lstm_step(P, indptr, indices, plan.order, t, n_act, h[t % 2], h[(t + 1) % 2], c, WT,
                    out)
    return out


def lstm_aggregate_train(indptr, indices, X, W_ih, W_hh, b_ih, b_hh):
    """lstm_aggregate keeping what the backward needs: every step's hidden and cell rows and
    pre-activation gates in a step-major packing (step t: rows order[0..n_t) at slots
    [off[t], off[t] + n_t)).  -> (out [n_dst, d], state for lstm_aggregate_backward)."""
    T = _T()
    _dev(indptr, "indptr", torch.int64)
    _dev(indices, "indices", torch.int32)
    d = W_hh.shape[1]
    n_dst = indptr.numel() - 1
    plan = LstmPlan.of(indptr)
    dev = X.device
    P = gemm(X.contiguous(), W_ih.detach(), bias=(b_ih + b_hh).detach())  # [N_src, 4d]
    out = torch.zeros((n_dst, d), dtype=torch.float32, device=dev)
    steps = plan.n_active
    off = [0]
    for n in steps:
        off.append(off[-1] + n)
    n_slots = off[-1]
    H = torch.empty((n_slots, d), dtype=torch.float32, device=dev)
    C = torch.empty((n_slots, d), dtype=torch.float32, device=dev)
    Z = torch.empty((n_slots, 4 * d), dtype=torch.float32, device=dev)
    WT = W_hh.detach().t().contiguous()
    h0 = torch.zeros((plan.n_rows, d), dtype=torch.float32, device=dev)
    for t, n in enumerate(steps):
        o, q = off[t], (off[t - 1] if t else 0)
        T.lstm_step_save(P, indptr, indices, plan.order, t, n, h0[:n] if t == 0 else H[q:q + n],
                         H[o:o + n], None if t == 0 else C[q:q + n], C[o:o + n], Z[o:o + n], WT,
                         out)
    return out, (plan, off, H, C, Z, WT)


def lstm_aggregate_backward(indptr, indices, X, W_ih, state, g, need_x: bool = True):
    """Backward through time of lstm_aggregate_train on the HIP kernels: per step (t
    descending) the gate Jacobian (gnnrec_lstm_backward_step_f32) and dh_{t-1} = dz·W_hh (a
    GEMM); then dW_hh = Σ_t dz_tᵀ h_{t-1} (one split-K GEMM over the slots, h_{t-1} rows
    gathered to the slots' order), dP = dz summed per source row (the slots' CSR by source,
    one spmm), dX = dP·W_ih, dW_ih = dPᵀ X and db = Σ dP (the same split-K pass).
    -> (dX or None, dW_ih, dW_hh, db)."""
    T = _T()
    plan, off, H, C, Z, WT = state
    steps = plan.n_active
    d = WT.shape[0]
    dev = Z.device
    n_slots = off[-1]
    n_src = X.shape[0]
    if n_slots == 0:
        z = torch.zeros
        return (z(X.shape, device=dev) if need_x else None, z(W_ih.shape, device=dev),
                z((4 * d, d), device=dev), z(4 * d, device=dev))
    g = g.contiguous()
    dZ = torch.empty((n_slots, 4 * d), dtype=torch.float32, device=dev)
    dc = [torch.empty((plan.n_rows, d), dtype=torch.float32, device=dev) for _ in range(2)]
    dh_next = dc_next = None
    n_next = 0
    for t in reversed(range(len(steps))):
        n, o = steps[t], off[t]
        q = off[t - 1] if t else 0
        dcp = dc[t % 2][:n]
        T.lstm_backward_step(Z[o:o + n], C[o:o + n], C[q:q + n] if t else None, dh_next,
                             dc_next, n_next, g, plan.order, n, dZ[o:o + n], dcp)
        if t:
            dh_next = gemm(dZ[o:o + n], WT)  # dz · W_hh
            dc_next, n_next = dcp, n
    src = torch.empty(n_slots, dtype=torch.int64, device=dev)
    prev = torch.empty(n_slots, dtype=torch.int64, device=dev)
    T.lstm_slots(indptr, indices, plan.order,
                 torch.tensor(off[:-1], dtype=torch.int64, device=dev), n_slots, src, prev)
    if len(steps) > 1:
        dW_hh = gemm_tn(dZ[off[1]:], gather_rows(H, prev[off[1]:]))
    else:
        dW_hh = torch.zeros((4 * d, d), dtype=torch.float32, device=dev)
    slots = torch.arange(n_slots, dtype=torch.int64, device=dev)
    ip, ix, _ = csr_build(slots, src, n_src)
    dP = spmm(ip, ix, dZ, "sum")
    db = torch.empty(4 * d, dtype=torch.float32, device=dev)
    dW_ih = gemm_tn(dP, X.detach().contiguous(), colsum=db)
    dX = gemm(dP, W_ih.detach().t().contiguous()) if need_x else None
    return dX, dW_ih, dW_hh, db


def gather_rows(src: torch.Tensor, idx: torch.Tensor) -> torch.Tensor:
    """a10: src[idx] along dim 0 for a device tensor of any dtype whose rows are contiguous
    (node features into blocks[0].srcdata, edge data into blocks)."""
    _dev(idx, "idx", torch.int64)
    if not (src.is_cuda or src.is_meta):
        raise ValueError("src: expected a device tensor (there is no CPU path)")
    if src.dim() == 0:
        raise ValueError("src: expected at least one dimension")
    row = src[0] if src.shape[0] else src.new_empty(src.shape[1:])
    if not (row.is_contiguous() and (src.dim() == 1 or src.stride(0) >= row.numel())):
        src = src.contiguous()
    out = torch.empty((idx.numel(),) + tuple(src.shape[1:]), dtype=src.dtype, device=src.device)
    _T().gather_rows(src, idx.contiguous(), out)
    return out


def scatter_rows(dst: torch.Tensor, idx: torch.Tensor, src: torch.Tensor) -> torch.Tensor:
    """The inverse of gather_rows, in place: dst[idx[i]] = src[i] (gnnrec_scatter_rows) for a
    device tensor of any dtype whose rows are contiguous.  idx is strictly ascending int64 —
    no two rows collide; an id outside dst's rows is skipped.  -> dst."""
    _dev(idx, "idx", torch.int64)
    if not (dst.is_cuda or dst.is_meta):
        raise ValueError("dst: expected a device tensor (there is no CPU path)")
    if dst.dim() == 0 or src.dim() != dst.dim() or src.dtype != dst.dtype or \
            src.shape[1:] != dst.shape[1:] or src.shape[0] != idx.numel():
        raise ValueError("scatter_rows: src must be [len(idx), ...] of dst's dtype and row shape")
    _T().scatter_rows(src.contiguous(), idx.contiguous(), dst)
    return dst


def sddmm_cos(src: torch.Tensor, dst: torch.Tensor, Hs: torch.Tensor,
              Hd: torch.Tensor) -> torch.Tensor:
    """a7: cosine of the L2-normalised endpoint rows, one value per edge -> [E]."""
    _dev(src, "src", torch.int64)
    _dev(dst, "dst", torch.int64)
    _dev(Hs, "Hs", torch.float32)
    _dev(Hd, "Hd", torch.float32)
    E = src.numel()
    if dst.numel() != E:
        raise ValueError("src/dst length mismatch")
    if Hs.shape[1] != Hd.shape[1]:
        raise ValueError("endpoint feature sizes differ")
    out = torch.empty(E, dtype=torch.float32, device=Hs.device)
    _rowmajor(Hs, "Hs")
    _rowmajor(Hd, "Hd")
    _T().sddmm_cos(src.contiguous(), dst.contiguous(), Hs, Hd, out)
    return out


def cos_grouped_ok(Hs: torch.Tensor, Hd: torch.Tensor) -> bool:
    """Can gnnrec_sddmm_cos_grouped_f32 score these tables (d % 4 == 0, d <= 256, 16-B rows)?"""
    d = Hs.shape[1]
    return (Hs.is_cuda and d % 4 == 0 and d <= 256 and Hs.dim() == 2 and Hd.dim() == 2 and
            Hs.stride(1) == 1 and Hd.stride(1) == 1 and Hs.stride(0) % 4 == 0 and
            Hd.stride(0) % 4 == 0 and Hs.data_ptr() % 16 == 0 and Hd.data_ptr() % 16 == 0)


def sddmm_cos_grouped(src_g: torch.Tensor, first: Optional[torch.Tensor], K: int,
                      dst: torch.Tensor, Hs: torch.Tensor, Hd: torch.Tensor):
    """a7 for the pair graphs of negative_sampler.Uniform(K): group g's positive edge
    (src_g[g], first[g]) and its K negatives (src_g[g], dst[g K + j]) -> (positive scores [G]
    (None without `first`), negative scores [G K]); bitwise sddmm_cos of the expanded lists."""
    for t, n in ((src_g, "src_g"), (dst, "dst")):
        _dev(t, n, torch.int64)
    if first is not None:
        _dev(first, "first", torch.int64)
    _dev(Hs, "Hs", torch.float32)
    _dev(Hd, "Hd", torch.float32)
    G = src_g.numel()
    out_first = torch.empty(G if first is not None else 0, dtype=torch.float32, device=Hs.device)
    out = torch.empty(G * int(K), dtype=torch.float32, device=Hs.device)
    _T().sddmm_cos_grouped(src_g.contiguous(), None if first is None else first.contiguous(),
                           int(K), dst.contiguous(), Hs, Hd, out_first, out)
    return (out_first if first is not None else None), out


def sddmm_cos_backward(src: torch.Tensor, dst: torch.Tensor, Hs: torch.Tensor, Hd: torch.Tensor,
                       grad: torch.Tensor, need_src: bool = True, need_dst: bool = True,
                       groups: int = 0, K: int = 0):
    """f2: gradients of sddmm_cos w.r.t. Hs and Hd given dL/dcos [E] -> (gHs|None, gHd|None),
    one library call (key sort, planned weighted gather, normalisation Jacobian).
    groups > 0: the edges are [groups positives | groups x K negatives] with each negative's
    source its positive's (negative_sampler.Uniform): the source side sorts only the group
    keys (gnnrec_sddmm_cos_backward_grouped_f32), and src may be the positives' sources
    alone (groups entries; the only ones read)."""
    T = _T()
    _dev(src, "src", torch.int64)
    _dev(dst, "dst", torch.int64)
    _dev(Hs, "Hs", torch.float32)
    _dev(Hd, "Hd", torch.float32)
    _dev(grad, "grad", torch.float32)
    E, d = dst.numel(), Hs.shape[1]
    if not (src.numel() == E or (groups and src.numel() == groups)) or grad.numel() != E:
        raise ValueError("sddmm_cos_backward: src/dst/grad length mismatch")
    if Hd.shape[1] != d:
        raise ValueError("endpoint feature sizes differ")
    n_s, n_d = Hs.shape[0], Hd.shape[0]
    gHs = torch.empty((n_s, d), dtype=torch.float32, device=Hs.device) if need_src else None
    gHd = torch.empty((n_d, d), dtype=torch.float32, device=Hs.device) if need_dst else None
    if groups and not (groups * (K + 1) == E and d % 4 == 0 and d <= 256 and
                       Hs.stride(0) % 4 == 0 and Hd.stride(0) % 4 == 0 and
                       Hs.data_ptr() % 16 == 0 and Hd.data_ptr() % 16 == 0):
        if groups and src.numel() == groups and groups * (K + 1) == E:
            src = torch.cat([src, src.repeat_interleave(K)])  # the per-edge form's full list
        groups = K = 0  # the layout or the rows do not fit the grouped form
    nbytes = int(T.sddmm_cos_backward_workspace_bytes(E, n_s, n_d, d, groups, K))
    ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=Hs.device)
    T.sddmm_cos_backward(src.contiguous(), dst.contiguous(), Hs, Hd, grad.contiguous(), gHs, gHd,
                         ws, groups, K)
    return gHs, gHd


def margin_loss(parts, delta: float, flat: bool = False):
    """f2: max_margin_loss forward + unscaled gradients for a list of etype parts
    [(pos [E], neg [E*K], K, mask|None, recency|None)] -> (loss 0-d tensor, N_total,
    [(g_pos, g_neg)]).  Gradients are d(sum of scores)/d(score); the loss is the mean.
    They are views of one buffer, in part order (pos_0, neg_0, pos_1, ...); flat: that
    buffer is returned as well."""
    T = _T()
    dev = parts[0][0].device
    # an etype without positive edges (the pair graphs' other etypes) adds nothing: no
    # launch and no partial for it, unless every etype is empty (the NaN mean below)
    skip = any(p[0].numel() for p in parts)
    blocks = [0 if skip and p[0].numel() == 0 else int(T.margin_loss_blocks(p[0].numel()))
              for p in parts]
    partial = torch.empty(sum(blocks), dtype=torch.float32, device=dev)
    gflat = torch.empty(sum(p[0].numel() + p[1].numel() for p in parts), dtype=torch.float32,
                        device=dev)
    grads, off, total, goff = [], 0, 0, 0
    for (pos, neg, K, mask, rec), nb in zip(parts, blocks):
        _dev(pos, "pos_score", torch.float32)
        _dev(neg, "neg_score", torch.float32)
        n_pos = pos.numel()
        if neg.numel() != n_pos * K:
            raise RuntimeError(f"shape '[-1, {K}]' is invalid for input of size {neg.numel()}")
        if mask is not None:
            mask = mask.to(device=dev, dtype=torch.float32).contiguous()
            if mask.numel() != neg.numel():
                raise ValueError("negative_mask must have one value per negative score")
        if rec is not None:
            rec = rec.to(dev).reshape(-1)
            if rec.dtype not in (torch.int64, torch.float32):
                rec = rec.float()
            rec = rec.contiguous()
            if rec.numel() != n_pos:
                raise ValueError("recency must have one value per positive edge")
        g_pos = gflat.narrow(0, goff, n_pos).view(pos.shape)
        g_neg = gflat.narrow(0, goff + n_pos, neg.numel()).view(neg.shape)
        goff += n_pos + neg.numel()
        if nb == 0:
            grads.append((g_pos, g_neg))
            continue
        T.margin_loss(pos.contiguous(), neg.contiguous(), K, float(delta), mask, rec, g_pos,
                      g_neg, partial[off:off + nb])
        grads.append((g_pos, g_neg))
        off += nb
        total += neg.numel()
    loss = torch.empty((), dtype=torch.float32, device=dev)
    T.sum_scaled(partial, 1.0 / total if total else float('nan'), loss)
    return (loss, total, grads, gflat) if flat else (loss, total, grads)


def edge_mlp(src: torch.Tensor, dst: torch.Tensor, P: torch.Tensor, Q: torch.Tensor,
             W2: torch.Tensor, b2: torch.Tensor, w3: torch.Tensor, b3: torch.Tensor) -> torch.Tensor:
    """a8 tail: sigmoid(w3·relu(W2·relu(P[src]+Q[dst]) + b2) + b3) -> [E]."""
    for t, n in ((P, "P"), (Q, "Q"), (W2, "W2"), (b2, "b2"), (w3, "w3"), (b3, "b3")):
        _dev(t, n, torch.float32)
    _dev(src, "src", torch.int64)
    _dev(dst, "dst", torch.int64)
    if P.shape[1] != 128 or Q.shape[1] != 128 or tuple(W2.shape) != (32, 128):
        raise ValueError("edge_mlp expects the reference's 128/32 hidden sizes")
    P, Q, W2 = P.contiguous(), Q.contiguous(), W2.detach().contiguous()
    E = src.numel()
    out = torch.empty(E, dtype=torch.float32, device=P.device)
    _T().edge_mlp(src.contiguous(), dst.contiguous(), P, Q, W2, b2.detach().contiguous(),
                  w3.detach().contiguous(), b3.detach().contiguous(), out)
    return out


def edge_mlp_grouped(src_g: torch.Tensor, first: Optional[torch.Tensor], K: int,
                     dst: torch.Tensor, P: torch.Tensor, Q: torch.Tensor, W2: torch.Tensor,
                     b2: torch.Tensor, w3: torch.Tensor, b3: torch.Tensor):
    """a8 tail for the pair graphs of negative_sampler.Uniform(K), grouped as
    sddmm_cos_grouped: group g's positive edge (src_g[g], first[g]) and its K negatives
    (src_g[g], dst[g K + j]) -> (positive scores [G] (None without `first`), negative scores
    [G K]); edge_mlp's scores of the expanded lists."""
    for t, n in ((P, "P"), (Q, "Q"), (W2, "W2"), (b2, "b2"), (w3, "w3"), (b3, "b3")):
        _dev(t, n, torch.float32)
    for t, n in ((src_g, "src_g"), (dst, "dst")):
        _dev(t, n, torch.int64)
    if first is not None:
        _dev(first, "first", torch.int64)
    if P.shape[1] != 128 or Q.shape[1] != 128 or tuple(W2.shape) != (32, 128):
        raise ValueError("edge_mlp expects the reference's 128/32 hidden sizes")
    P, Q, W2 = P.contiguous(), Q.contiguous(), W2.detach().contiguous()
    G = src_g.numel()
    out_first = torch.empty(G if first is not None else 0, dtype=torch.float32, device=P.device)
    out = torch.empty(G * int(K), dtype=torch.float32, device=P.device)
    _T().edge_mlp_grouped(src_g.contiguous(), None if first is None else first.contiguous(),
                          int(K), dst.contiguous(), P, Q, W2, b2.detach().contiguous(),
                          w3.detach().contiguous(), b3.detach().contiguous(), out_first, out)
    return (out_first if first is not None else None), out


def synth_edges(seed: int, e0: int, n: int, n_u: int, n_i: int, device,
                zipf_cdf: Optional[torch.Tensor] = None):
    """Counter-hash bipartite edges [e0, e0+n) -> (u int32 [n], i int32 [n])."""
    u = torch.empty(n, dtype=torch.int32, device=device)
    i = torch.empty(n, dtype=torch.int32, device=device)
    if zipf_cdf is not None:
        _dev(zipf_cdf, "zipf_cdf", torch.float64)
    _T().synth_edges(_lib.i64(seed), e0, n_u, n_i, zipf_cdf, u, i)
    return u, i


def exclusive_scan(x: torch.Tensor) -> torch.Tensor:
    """[n] int32/int64 -> [n+1] int64 exclusive prefix sums (last = total)."""
    T = _T()
    _dev(x, "x")
    if x.dtype not in (torch.int64, torch.int32):
        raise ValueError("exclusive_scan supports int32/int64")
    n = x.numel()
    out = torch.empty(n + 1, dtype=torch.int64, device=x.device)
    ws = torch.empty(max(1, (T.scan_workspace_bytes(n) + 7) // 8), dtype=torch.int64,
                     device=x.device)
    T.exclusive_scan(x.contiguous(), out, ws)
    return out


def sample_count(indptr, eids, seeds, fanout: int, seed_key: int = 0,
                 excluded: Optional[torch.Tensor] = None,
                 excluded_rows: Optional[torch.Tensor] = None) -> torch.Tensor:
    """a9 phase 1: per-seed sampled in-edge counts -> out_indptr [n_seeds+1] (device).
    excluded_rows (uint8 per dst node, optional): nonzero exactly on the dst nodes of the
    excluded eids — the other seeds skip the eid checks (same counts)."""
    for t, n in ((indptr, "indptr"), (eids, "eids"), (seeds, "seeds")):
        _dev(t, n, torch.int64)
    for t, n in ((excluded, "excluded"), (excluded_rows, "excluded_rows")):
        if t is not None:
            _dev(t, n, torch.uint8)
    n = seeds.numel()
    fan = -1 if fanout is None or fanout < 0 else int(fanout)
    counts = torch.empty(n, dtype=torch.int64, device=seeds.device)
    _T().sample_count(indptr, eids, excluded, seeds, fan, _lib.i64(seed_key), counts,
                      excluded_rows)
    return exclusive_scan(counts)


def sample_fill(indptr, indices, eids, seeds, fanout: int, seed_key: int, out_indptr,
                total: int, excluded: Optional[torch.Tensor] = None,
                excluded_rows: Optional[torch.Tensor] = None):
    """a9 phase 2: copy the sampled edges at out_indptr offsets -> (src ids, eids).

    indices: the CSR's int32 source ids (graph.in_csr); outputs are int64."""
    _dev(indices, "indices", torch.int32)
    n = seeds.numel()
    fan = -1 if fanout is None or fanout < 0 else int(fanout)
    out_src = torch.empty(total, dtype=torch.int64, device=seeds.device)
    out_eid = torch.empty(total, dtype=torch.int64, device=seeds.device)
    _T().sample_fill(indptr, indices, eids, excluded, seeds, fan, _lib.i64(seed_key), out_indptr,
                     out_src, out_eid, excluded_rows)
    return out_src, out_eid


def sample_neighbors(indptr, indices, eids, seeds, fanout: int, seed_key: int = 0,
                     excluded: Optional[torch.Tensor] = None,
                     excluded_rows: Optional[torch.Tensor] = None):
    """a9: in-edges of `seeds` (all, or `fanout` without replacement), minus excluded eids.

    indices is the CSR's int32 source-id array; returns (out_indptr [n_seeds+1],
    src global ids int64 [E'], eids [E'])."""
    out_indptr = sample_count(indptr, eids, seeds, fanout, seed_key, excluded, excluded_rows)
    total = int(out_indptr[-1].item())  # size readback
    out_src, out_eid = sample_fill(indptr, indices, eids, seeds, fanout, seed_key, out_indptr,
                                   total, excluded, excluded_rows)
    return out_indptr, out_src, out_eid


def sample_layer(indptrs, indices, eids, masks, src_type, dst_type, fanouts, keys, seeds,
                 prefix_pos, marks, mask_rows=None):
    """a9, one block layer in one call (gnnrec::sample_layer): sampled in-edges of every
    relation's seeds + the to_block relabel of every node type, two host size reads.
    mask_rows: per relation the excluded_rows flags of sample_count (or None).
    -> ([out_indptr], [local src int32], [eids], [src node ids per type], [edge counts])."""
    for t in list(indptrs) + list(eids) + list(seeds) + list(prefix_pos):
        _dev(t, "sample_layer operand", torch.int64)
    fans = [-1 if f is None or f < 0 else int(f) for f in fanouts]
    rows = list(mask_rows) if mask_rows is not None else [None] * len(masks)
    return _T().sample_layer(list(indptrs), list(indices), list(eids), list(masks), rows,
                             list(src_type), list(dst_type), fans, [_lib.i64(k) for k in keys],
                             list(seeds), list(prefix_pos), list(marks))


SB_MAX_RELS, SB_MAX_TYPES, SB_MAX_STEPS, SB_MAX_FANOUT = 8, 4, 4, 64
GATHER_MAX_JOBS = 16


class SampleScratch:
    """Per-node-type state of the fused sampler (gnnrec_sample_blocks, include/gnnrec.h):
    `pos` (two arrays of stamped seed positions, used alternately, never cleared), two
    new-source bitmaps and their word ranks, new-source and seed byte marks (two each).  `stamp` advances by steps + 1 per call; before it would wrap, `pos` is zeroed
    and the count restarts (one memset per ~4e9 sampled layers)."""

    def __init__(self, n_nodes: int, device):
        w = (n_nodes + 63) // 64
        self.n_nodes = n_nodes
        self.pos = torch.zeros(2 * n_nodes, dtype=torch.int64, device=device)
        self.bits = torch.zeros(2 * w, dtype=torch.int64, device=device)
        self.word_rank = torch.empty(w + 1, dtype=torch.int64, device=device)
        # two new-source mark arrays, then two seed mark arrays (each pair used alternately)
        self.marks = torch.zeros(4 * 64 * w, dtype=torch.uint8, device=device)


SampleSizes = collections.namedtuple("SampleSizes", "nodes edges dump")


def sample_sizes(flat, L: int, T: int, R: int, dump: bool = True) -> SampleSizes:
    """The fused sampler's sizes of L steps (step 0 = the output block), T node types and R
    relations, from gnnrec::sample_blocks' flat layout — a list of ints, or a device tensor
    (one-entry views): nodes[0][t] the seeds and nodes[s + 1][t] step s's source nodes (so
    step s has nodes[s][t] destinations), edges[s][r], then dump[s][t], the dump rows after
    step s's destination rows (static shapes; zero otherwise; dump=False: flat has none)."""
    if len(flat) != (L + 1) * T + L * R + (L * T if dump else 0):
        raise ValueError(f"sample_sizes: {len(flat)} entries for {(L, T, R)} steps, types, rels")
    at = (lambda i: flat.narrow(0, i, 1)) if torch.is_tensor(flat) else flat.__getitem__
    rows = iter(range(len(flat)))  # the entries in order: no offsets to keep in step
    return SampleSizes([[at(next(rows)) for _ in range(T)] for _ in range(L + 1)],
                       [[at(next(rows)) for _ in range(R)] for _ in range(L)],
                       [[at(next(rows)) for _ in range(T)] for _ in range(L)] if dump else [])


def sample_sizes_out(L: int, T: int, R: int, device):
    """A static sample_blocks call's sizes_out, and its entries as one-entry device views."""
    flat = torch.empty((L + 1) * T + L * R, dtype=torch.int64, device=device)
    return flat, sample_sizes(flat, L, T, R, dump=False)


def sample_blocks(indptrs, indices, eids, src_type, dst_type, excl, n_nodes, seeds, scratch,
                  fanouts, keys, stamp, static_shapes=False, sizes_out=None, node_cap_hint=None,
                  overflow=None, edge_tables=(), node_tables=(), edge_recs=()):
    """a9, every block of one bounded-fanout sample_blocks call (gnnrec::sample_blocks,
    1 + 3L launches, one host size read).  fanouts / keys: [step][relation] (step 0 = the
    output block); excl: per relation None or (eids, coo_dst, mask, rows).
    -> per step: ([out_indptr], [local src int32], [eids]) per relation, [src node ids] per
    type; the sizes (SampleSizes); the gathered block data.
    static_shapes: every output at its capacity, no host read (the -1-padded layout of
    include/gnnrec.h); the sizes returned are then the capacities, and the actual ones are
    left on the device in sizes_out (int64, the flat layout of sample_sizes without the dump
    rows), which is given exactly when static_shapes is.  node_cap_hint ([step][type],
    static): tighter node capacities than the provable ones; a batch that does not fit sets
    `overflow` (int64 device flag) and must be discarded or redone.
    edge_tables [(table, relation)] / node_tables [(table, node type)]: the block data (a10),
    gathered inside an exact call (never a static one) — every step's edge data at its edge
    ids, the input block's (the last step's) node rows at its source ids — returned as a
    third value in that order (step-major for the edge tables).  edge_recs: per relation the
    packed {eid << 32 | src} records of its CSR (HeteroGraph.edge_records), or empty (the
    index / eid arrays)."""
    steps, R, NT = len(fanouts), len(indptrs), len(n_nodes)
    if (sizes_out is not None) != bool(static_shapes):
        raise ValueError("sample_blocks: sizes_out goes with static_shapes, and only with it")
    ex =[e if e is not None else (None,) * 4 for e in excl]
    o_ip, o_src, o_eid, nodes, sizes, data = _T().sample_blocks(
        list(indptrs), list(indices), list(eids), list(src_type), list(dst_type),
        [e[0] for e in ex], [e[1] for e in ex], [e[2] for e in ex], [e[3] for e in ex],
        list(n_nodes), list(seeds), [s.pos for s in scratch], [s.bits for s in scratch],
        [s.word_rank for s in scratch], [s.marks for s in scratch],
        [int(f) for fs in fanouts for f in fs],
        [_lib.i64(k) for ks in keys for k in ks], steps, int(stamp), bool(static_shapes),
        sizes_out, [int(h) for hs in (node_cap_hint or []) for h in hs], overflow,
        [t for t, _ in edge_tables], [int(r) for _, r in edge_tables],
        [t for t, _ in node_tables], [int(x) for _, x in node_tables], list(edge_recs))
    out = [(o_ip[s * R:(s + 1) * R], o_src[s * R:(s + 1) * R], o_eid[s * R:(s + 1) * R],
            nodes[s * NT:(s + 1) * NT]) for s in range(steps)]
    return out, sample_sizes(sizes, steps, NT, R), data


class CompactScratch:
    """Per-node-type scratch of compact_ids: two id bitmaps used alternately (the call marks
    one and zeroes the other) and their word ranks."""

    def __init__(self, n_nodes: int, device):
        w = (n_nodes + 63) // 64
        self.n_nodes = n_nodes
        # the two bitmaps, then the scan's ticket and tile flags (GNNREC_COMPACT_SCAN_WS)
        self.bits = torch.zeros(2 * w + 2 + w // 1024, dtype=torch.int64, device=device)
        self.word_rank = torch.empty(w + 1, dtype=torch.int64, device=device)
        self.marks = torch.zeros(2 * 64 * w, dtype=torch.uint8, device=device)
        self.parity = 0


def compact_ids(lists, scratch, caps):
    """a11, DGL's compact_graphs over id lists at static shapes (gnnrec::compact_ids, 3
    launches, no host read): lists = [(ids int64, type index)]; scratch / caps per type.
    -> ([nodes [cap] per type: ascending ids, -1 past the count], [local ids per list],
    count [types] on the device)."""
    for ids, _ in lists:
        _dev(ids, "ids", torch.int64)
    parity = scratch[0].parity
    out = _T().compact_ids([ids.contiguous() for ids, _ in lists], [int(t) for _, t in lists],
                           [s.n_nodes for s in scratch], [int(c) for c in caps],
                           [s.bits for s in scratch], [s.word_rank for s in scratch],
                           [s.marks for s in scratch], parity)
    for s in scratch:
        s.parity = 1 - parity
    return out


def copy_batch(src, dst) -> None:
    """a12: dst[j].copy_(src[j]) for contiguous same-shape device tensors, 64 per launch
    (gnnrec_copy_batch); other pairs through torch's copy."""
    a, b = [], []
    for s_, d_ in zip(src, dst):
        if s_.is_contiguous() and d_.is_contiguous() and s_.dtype == d_.dtype and \
                s_.shape == d_.shape:
            a.append(s_)
            b.append(d_)
        else:
            d_.copy_(s_)
    if a:
        _T().copy_batch(a, b)


def gather_rows_batch(jobs, n_dev=None):
    """a10, several gathers in one launch: jobs = [(src, idx)] -> [src[idx]] (any dtype,
    contiguous rows; at most GATHER_MAX_JOBS per launch).  n_dev: per job None or a one-entry
    int64 device tensor — only the first min(n_dev, len(idx)) rows are gathered (the rest of
    the output is left unwritten)."""
    outs = []
    empty = None
    for i in range(0, len(jobs), GATHER_MAX_JOBS):
        part = jobs[i:i + GATHER_MAX_JOBS]
        srcs, idxs, res, cnts = [], [], [], []
        for k, (src, idx) in enumerate(part):
            c = None if n_dev is None else n_dev[i + k]
            if c is None:
                if empty is None:
                    empty = torch.empty(0, dtype=torch.int64, device=idx.device)
                c = empty
            cnts.append(c)
            _dev(idx, "idx", torch.int64)
            if src.dim() == 0:
                raise ValueError("src: expected at least one dimension")
            row = src[0] if src.shape[0] else src.new_empty(src.shape[1:])
            if not (row.is_contiguous() and (src.dim() == 1 or src.stride(0) >= row.numel())):
                src = src.contiguous()
            srcs.append(src)
            idxs.append(idx.contiguous())
            res.append(torch.empty((idx.numel(),) + tuple(src.shape[1:]), dtype=src.dtype,
                                   device=src.device))
        _T().gather_rows_batch(srcs, idxs, res, cnts if n_dev is not None else [])
        outs.extend(res)
    return outs


def edge_batch_pairs(rel_src, rel_dst, src_type, dst_type, batch, neg_order, k, n_nodes,
                     prefix_pos, marks):
    """EdgeDataLoader's batch head in one call (gnnrec::edge_batch_pairs): positive pairs of
    the batch's edges, k uniform negatives per positive (negative_sampler.Uniform's draws),
    and compact_graphs over both, one host size read.
    -> ([node ids per type], [pos src], [pos dst], [neg src], [neg dst]) in local ids."""
    for t in list(rel_src) + list(rel_dst) + list(batch) + list(prefix_pos):
        _dev(t, "edge_batch_pairs operand", torch.int64)
    return _T().edge_batch_pairs(list(rel_src), list(rel_dst), list(src_type), list(dst_type),
                                 list(batch), list(neg_order), int(k), list(n_nodes),
                                 list(prefix_pos), list(marks))


class Relabeler:
    """Per-node-type scratch for to_block relabelling (mark array + prefix map).

    Keeps two arrays of size n_nodes resident on the device (reset after each
    use by touching only the ids that were set).  `relabel` is the one-shot form;
    begin / mark / finish split it so a caller can batch the size readback of
    several node types into one host sync."""

    def __init__(self, n_nodes: int, device):
        self.n_nodes = n_nodes
        self.prefix_pos = torch.full((n_nodes,), -1, dtype=torch.int64, device=device)
        self.mark = torch.zeros(n_nodes, dtype=torch.int32, device=device)

    def begin(self, prefix: torch.Tensor, id_lists):
        """set the prefix map, mark new ids, scan -> rank (device; rank[-1] = n_new)."""
        T = _T()
        T.set_prefix_pos(prefix, self.prefix_pos)
        for ids in id_lists:
            T.mark_ids(ids, self.prefix_pos, self.mark)
        return exclusive_scan(self.mark)

    def finish(self, prefix: torch.Tensor, id_lists, rank: torch.Tensor, n_new: int):
        """compact the new ids, relabel every list, reset the scratch."""
        T = _T()
        n_p = prefix.numel()
        src_nodes = torch.empty(n_p + n_new, dtype=torch.int64, device=prefix.device)
        src_nodes[:n_p] = prefix
        if n_new:
            T.compact_marked(self.mark, rank, src_nodes[n_p:])
        locals_ = []
        for ids in id_lists:
            loc = torch.empty(ids.numel(), dtype=torch.int64, device=prefix.device)
            T.relabel_ids(ids, self.prefix_pos, rank, n_p, loc)
            locals_.append(loc)
        T.clear_prefix_pos(prefix, self.prefix_pos)
        if n_new:
            self.mark.index_fill_(0, src_nodes[n_p:], 0)
        return src_nodes, locals_

    def relabel(self, prefix: torch.Tensor, id_lists):
        """prefix: dst ids [n_p]; id_lists: list of global src id tensors.

        Returns (src_nodes [n_p + n_new] global ids, [local ids per list])."""
        rank = self.begin(prefix, id_lists)
        return self.finish(prefix, id_lists, rank, int(rank[-1].item()))


# load the library at import (outside any torch.compile trace); if it is missing, every op
# raises GnnrecLibraryError when called — there is no fallback
try:
    _lib.torch_ops()
except _lib.GnnrecLibraryError:
    pass


# ---- f1b: exact top-k behind a bf16 MFMA prefilter (csrc/recommend.hip) ----
def normalize_rows_bf16(x: torch.Tensor, row_map: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Rows of x (row_map[r] of x when given) divided by max(norm, 1e-12) and rounded to bf16
    (nearest even) -> [n, dpad], dpad = d rounded up to a multiple of 32, the pad zero."""
    _dev(x, "x", torch.float32)
    _rowmajor(x, "x")
    if row_map is not None:
        _dev(row_map, "row_map", torch.int64)
        row_map = row_map.contiguous()
    n = x.shape[0] if row_map is None else row_map.numel()
    out = torch.empty((n, (x.shape[1] + 31) // 32 * 32), dtype=torch.bfloat16, device=x.device)
    _T().normalize_rows_bf16(x, row_map, out)
    return out


def score_bf16_store(users: torch.Tensor, items: torch.Tensor) -> torch.Tensor:
    """Approximate cosines of two normalize_rows_bf16 tables, bf16 products accumulated in
    fp32 on the MFMA -> fp32 [n_users, n_items]."""
    _dev(users, "users", torch.bfloat16)
    _dev(items, "items", torch.bfloat16)
    out = torch.empty((users.shape[0], items.shape[0]), dtype=torch.float32, device=users.device)
    _T().score_bf16_store(users, items, out)
    return out


def score_bf16_filter(users: torch.Tensor, items: torch.Tensor, tau: torch.Tensor,
                      counts: torch.Tensor, cand_items: torch.Tensor) -> None:
    """The same scores, none written: item v joins row u's list in cand_items [B, cap]
    (int32) where the score is >= tau[u] - 2 eps; counts [B] (int32, zeroed by the caller)
    counts every passing item, past cap too (counts[u] > cap: the row overflowed)."""
    _dev(users, "users", torch.bfloat16)
    _dev(items, "items", torch.bfloat16)
    _dev(tau, "tau", torch.float32)
    _dev(counts, "counts", torch.int32)
    _dev(cand_items, "cand_items", torch.int32)
    _T().score_bf16_filter(users, items, tau, counts, cand_items)


def mask_excluded(scores: torch.Tensor, user_rows: Optional[torch.Tensor],
                  exclude_indptr: torch.Tensor, exclude_indices: torch.Tensor) -> None:
    """scores[r][c] = -inf, in place, for the items c of row r's user (user_rows[r], or r) in
    the exclusion CSR (int64 indptr over user rows, int32 item ids) that are columns."""
    _dev(scores, "scores", torch.float32)
    _dev(exclude_indptr, "exclude_indptr", torch.int64)
    _dev(exclude_indices, "exclude_indices", torch.int32)
    _T().mask_excluded_f32(scores, user_rows, exclude_indptr, exclude_indices)


def topk_candidates(counts: torch.Tensor, cand_items: torch.Tensor,
                    user_rows: Optional[torch.Tensor], h_user: torch.Tensor,
                    h_item: torch.Tensor, k: int, exclude_indptr: Optional[torch.Tensor] = None,
                    exclude_indices: Optional[torch.Tensor] = None,
                    out_vals: Optional[torch.Tensor] = None,
                    out_idx: Optional[torch.Tensor] = None):
    """Per batch row: its candidates minus the user's excluded items (a CSR over h_user's
    rows, int32 ids), rescored with the fp32 cosine (bitwise sddmm_cos) and ranked by
    (score desc, item asc) -> (vals [B, k], idx [B, k]), padded with (-inf, -1).  Rows with
    counts > cap are left unwritten."""
    _dev(counts, "counts", torch.int32)
    _dev(cand_items, "cand_items", torch.int32)
    _dev(h_user, "h_user", torch.float32)
    _dev(h_item, "h_item", torch.float32)
    B = counts.numel()
    if out_vals is None:
        out_vals = torch.empty((B, k), dtype=torch.float32, device=counts.device)
    if out_idx is None:
        out_idx = torch.empty((B, k), dtype=torch.int64, device=counts.device)
    _T().topk_candidates_f32(counts, cand_items, user_rows, h_user, h_item, exclude_indptr,
                             exclude_indices, int(k), out_vals, out_idx)
    return out_vals, out_idx


UPDATE_SLOTS = 256   # gnnrec_topk_update_f32: k list entries + cap candidates per row
UPDATE_MAX_K = 64


def topk_update(rows: torch.Tensor, idx: torch.Tensor, vals: torch.Tensor,
                item_mark: torch.Tensor, counts: torch.Tensor, cand_cols: torch.Tensor,
                dirty_ids: torch.Tensor, h_user: torch.Tensor, h_item: torch.Tensor,
                redo: torch.Tensor, exclude_indptr: Optional[torch.Tensor] = None,
                exclude_indices: Optional[torch.Tensor] = None) -> None:
    """The cached lists idx / vals [n_users, k] of the clean user rows `rows`, in place, after
    a refresh that rewrote the item rows marked in item_mark [n_items] (int32; dirty_ids
    int32, ascending, lists them): per row the list's dirty entries dropped, its candidates
    (counts / cand_cols [B, cap] of score_bf16_filter over the dirty items' bf16 table with
    tau = the list's last score; columns are positions in dirty_ids) minus the user's
    excluded items rescored with the fp32 cosine of the refreshed tables, and the k best
    written where that is provably the exhaustive ranking's list.  The other
    rows, and rows with counts > cap, get redo[user] = 1 (int32 [n_users], zeroed by the
    caller) and stay as they were.  k <= UPDATE_MAX_K, cap <= UPDATE_SLOTS - k."""
    _dev(rows, "rows", torch.int64)
    _dev(idx, "idx", torch.int64)
    _dev(vals, "vals", torch.float32)
    _dev(item_mark, "item_mark", torch.int32)
    _dev(counts, "counts", torch.int32)
    _dev(cand_cols, "cand_cols", torch.int32)
    _dev(dirty_ids, "dirty_ids", torch.int32)
    _dev(h_user, "h_user", torch.float32)
    _dev(h_item, "h_item", torch.float32)
    _dev(redo, "redo", torch.int32)
    _T().topk_update(rows, idx, vals, item_mark, counts, cand_cols, dirty_ids, h_user, h_item,
                     exclude_indptr, exclude_indices, redo)


# ---- f1c: many-user top-k for the MLP head (csrc/heads.hip, csrc/recommend.hip) ----
def _dense_mlp_operands(P, Q, W2, b2, w3, b3):
    for t, n in ((P, "P"), (Q, "Q"), (W2, "W2"), (b2, "b2"), (w3, "w3"), (b3, "b3")):
        _dev(t, n, torch.float32)
    if P.dim() != 2 or Q.dim() != 2 or P.shape[1] != 128 or Q.shape[1] != 128 or \
            tuple(W2.shape) != (32, 128) or b2.numel() != 32 or w3.numel() != 32 or \
            b3.numel() != 1:
        raise ValueError("edge_mlp expects the reference's 128/32 hidden sizes")
    return (P.contiguous(), Q.contiguous(), W2.detach().contiguous(), b2.detach().contiguous(),
            w3.detach().reshape(-1).contiguous(), b3.detach().contiguous())


def edge_mlp_dense_store(P: torch.Tensor, Q: torch.Tensor, W2: torch.Tensor, b2: torch.Tensor,
                         w3: torch.Tensor, b3: torch.Tensor,
                         out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The MLP head's score of every user row of P [B, 128] against every item row of
    Q [n, 128] -> fp32 [B, n]; each value is bitwise edge_mlp's for the pair.  No id arrays:
    a 32-item tile of Q is staged once and scored for 64 users in turn."""
    ops = _dense_mlp_operands(P, Q, W2, b2, w3, b3)
    if out is None:
        out = torch.empty((P.shape[0], Q.shape[0]), dtype=torch.float32, device=P.device)
    _T().edge_mlp_dense_store_f32(*ops, out)
    return out


def edge_mlp_dense_filter(P: torch.Tensor, Q: torch.Tensor, W2: torch.Tensor, b2: torch.Tensor,
                          w3: torch.Tensor, b3: torch.Tensor, tau: torch.Tensor,
                          counts: torch.Tensor, cand_items: torch.Tensor,
                          cand_scores: torch.Tensor) -> None:
    """The same scores, none written to a matrix: where score(u, v) >= tau[u] (compared as
    is) item v and its score join row u's lists cand_items (int32) / cand_scores (fp32)
    [B, cap]; counts [B] (int32, zeroed by the caller) counts every passing item, past cap
    too (counts[u] > cap: the row overflowed)."""
    ops = _dense_mlp_operands(P, Q, W2, b2, w3, b3)
    _dev(tau, "tau", torch.float32)
    _dev(counts, "counts", torch.int32)
    _dev(cand_items, "cand_items", torch.int32)
    _dev(cand_scores, "cand_scores", torch.float32)
    _T().edge_mlp_dense_filter_f32(*ops, tau, counts, cand_items, cand_scores)


def topk_scored_candidates(counts: torch.Tensor, cand_items: torch.Tensor,
                           cand_scores: torch.Tensor, k: int,
                           user_rows: Optional[torch.Tensor] = None,
                           exclude_indptr: Optional[torch.Tensor] = None,
                           exclude_indices: Optional[torch.Tensor] = None,
                           out_vals: Optional[torch.Tensor] = None,
                           out_idx: Optional[torch.Tensor] = None):
    """Per batch row: its first min(count, cap) (item, score) pairs minus the user's excluded
    items (a CSR over the user rows, int32 ids), ranked by (score desc, item asc) ->
    (vals [B, k], idx [B, k]), padded with (-inf, -1).  Rows with counts > cap are left
    unwritten."""
    _dev(counts, "counts", torch.int32)
    _dev(cand_items, "cand_items", torch.int32)
    _dev(cand_scores, "cand_scores", torch.float32)
    B = counts.numel()
    if out_vals is None:
        out_vals = torch.empty((B, k), dtype=torch.float32, device=counts.device)
    if out_idx is None:
        out_idx = torch.empty((B, k), dtype=torch.int64, device=counts.device)
    _T().topk_scored_candidates_f32(counts, cand_items, cand_scores, user_rows, exclude_indptr,
                                    exclude_indices, int(k), out_vals, out_idx)
    return out_vals, out_idx


# ---- f1d: popularity-weighted ratings (csrc/rating.hpp, recommend_pop.hip) ----
def denominator_parts(n_items: int) -> int:
    """Partial sums the item axis is cut into for the rating's denominators: a function of
    n_items alone (1024 consecutive items each)."""
    return int(_T().cos_denominator_parts(int(n_items)))


def normalize_rows_f32(x: torch.Tensor, row_map: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Rows of x (row_map[r] of x when given) divided by max(norm, 1e-12) in fp32 — the values
    normalize_rows_bf16 rounds — -> [n, dpad], dpad = d rounded up to a multiple of 8 (the
    pad zero), each group of 8 columns stored as [0, 2, 4, 6, 1, 3, 5, 7]: the operand
    layout of cos_denominators.  d % 4 == 0, 4 <= d <= 2048."""
    _dev(x, "x", torch.float32)
    _rowmajor(x, "x")
    if row_map is not None:
        _dev(row_map, "row_map", torch.int64)
        row_map = row_map.contiguous()
    n = x.shape[0] if row_map is None else row_map.numel()
    out = torch.empty((n, (x.shape[1] + 7) // 8 * 8), dtype=torch.float32, device=x.device)
    _T().normalize_rows_f32(x, row_map, out)
    return out


def cos_denominators(users: torch.Tensor, items: torch.Tensor) -> torch.Tensor:
    """Z[u] = sum over all items v of expf(users[u] . items[v]) for two normalize_rows_f32
    tables (fp32 MFMA) -> fp32 [n_users].  A row's Z has the same bits whatever batch it is
    computed in: the item axis is cut by n_items alone and every fold has a fixed order."""
    _dev(users, "users", torch.float32)
    _dev(items, "items", torch.float32)
    B = users.shape[0]
    parts = torch.empty((denominator_parts(items.shape[0]), B), dtype=torch.float32,
                        device=users.device)
    Z = torch.empty(B, dtype=torch.float32, device=users.device)
    _T().cos_denominators_f32(users, items, parts, Z)
    return Z


# ---- f1f: exact rank among all items (csrc/rank.hip) ----
def rank_eps(d: int) -> float:
    """The bound on |a - sddmm_cos| for the fp32 MFMA dot a of two normalize_rows_f32 rows of
    width d: (4 dpad + 32) 2^-24, dpad = d rounded up to a multiple of 8 (the library's value;
    the derivation is in csrc/rank.hip)."""
    return float(_T().rank_eps(int(d)))


def cos_scores_f32(users: torch.Tensor, items: torch.Tensor) -> torch.Tensor:
    """The fp32 MFMA dots of two normalize_rows_f32 tables, stored -> fp32 [n_users, n_items]:
    the values rank_count compares and cos_denominators sums (for tests of the bound)."""
    _dev(users, "users", torch.float32)
    _dev(items, "items", torch.float32)
    out = torch.empty((users.shape[0], items.shape[0]), dtype=torch.float32, device=users.device)
    _T().cos_scores_f32(users, items, out)
    return out


def rank_count(users: torch.Tensor, items: torch.Tensor, thr: torch.Tensor,
               band_counts: torch.Tensor, band_items: torch.Tensor) -> torch.Tensor:
    """One fp32 MFMA pass over all items for the pair rows of `users` (normalize_rows_f32 of
    each pair's user; `items` the item table): -> ahead int32 [R], the items whose dot exceeds
    thr[r] + rank_eps; items within rank_eps of thr[r] join the row's list in band_items
    [R, cap] (int32), band_counts [R] (int32, zeroed by the caller) counting past cap too."""
    _dev(users, "users", torch.float32)
    _dev(items, "items", torch.float32)
    _dev(thr, "thr", torch.float32)
    _dev(band_counts, "band_counts", torch.int32)
    _dev(band_items, "band_items", torch.int32)
    R = users.shape[0]
    parts = torch.empty((denominator_parts(items.shape[0]), R), dtype=torch.int32,
                        device=users.device)
    ahead = torch.empty(R, dtype=torch.int32, device=users.device)
    _T().rank_count_f32(users, items, thr, parts, ahead, band_counts, band_items)
    return ahead


def rank_resolve(users: torch.Tensor, items: torch.Tensor, thr: torch.Tensor,
                 ahead: torch.Tensor, band_counts: torch.Tensor, band_items: torch.Tensor,
                 h_user: torch.Tensor, h_item: torch.Tensor,
                 exclude_indptr: Optional[torch.Tensor] = None,
                 exclude_indices: Optional[torch.Tensor] = None,
                 out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Per pair (users[r], items[r]): rank = 1 + ahead + (band items exactly ahead) - (the
    user's excluded items exactly ahead), 0 where the item is excluded, -1 where
    band_counts[r] > cap -> int64 [P].  Scores are bitwise sddmm_cos's; the exclusion CSR
    (over h_user's rows, int32) holds each id at most once per row, entries < 0 are skipped."""
    _dev(users, "users", torch.int64)
    _dev(items, "items", torch.int64)
    _dev(thr, "thr", torch.float32)
    _dev(ahead, "ahead", torch.int32)
    _dev(band_counts, "band_counts", torch.int32)
    _dev(band_items, "band_items", torch.int32)
    _dev(h_user, "h_user", torch.float32)
    _dev(h_item, "h_item", torch.float32)
    if out is None:
        out = torch.empty(users.numel(), dtype=torch.int64, device=users.device)
    _T().rank_resolve_f32(users, items, thr, ahead, band_counts, band_items, h_user, h_item,
                          exclude_indptr, exclude_indices, out)
    return out


# ---- f1f for the MLP head: one scored row per user (csrc/heads.hip) ----
def rank_list_slots() -> int:
    """Entries a row of the count pass holds at most (kDenseListSlots); a longer list is split
    over rows that repeat the user's P row."""
    return int(_T().rank_list_slots())


def _count_slots(Q, lptr, s, gid):
    _dev(lptr, "lptr", torch.int64)
    _dev(s, "thr", torch.float32)
    _dev(gid, "gid", torch.int32)
    E = s.numel()
    parts = torch.empty((denominator_parts(Q.shape[0]), E), dtype=torch.int32, device=Q.device)
    ahead = torch.empty(E, dtype=torch.int32, device=Q.device)
    return parts, ahead


def edge_mlp_dense_count_lists(P: torch.Tensor, Q: torch.Tensor, W2: torch.Tensor,
                               b2: torch.Tensor, w3: torch.Tensor, b3: torch.Tensor,
                               lptr: torch.Tensor, thr: torch.Tensor,
                               gid: torch.Tensor) -> torch.Tensor:
    """One pass of the dense MLP kernel over all item rows of Q with one scored row for several
    entries: row r of P [R, 128] (a user, rank_list_slots() entries of a longer list, or a
    single pair) owns the slots [lptr[r], lptr[r + 1]) (int64 [R + 1], at most
    rank_list_slots() a row) of thr (the entry's own edge_mlp score) and gid (its held-out
    item, int32) -> ahead int32 [E], per slot j the items v != gid[j] with score > thr[j], or
    == thr[j] and v < gid[j].  The compared scores are bitwise edge_mlp's, so there is no band
    and no candidate list."""
    ops = _dense_mlp_operands(P, Q, W2, b2, w3, b3)
    parts, ahead = _count_slots(Q, lptr, thr, gid)
    _T().edge_mlp_dense_count_lists_f32(*ops, lptr, thr, gid, parts, ahead)
    return ahead


def edge_mlp_dense_count_lists_rating(P: torch.Tensor, Q: torch.Tensor, W2: torch.Tensor,
                                      b2: torch.Tensor, w3: torch.Tensor, b3: torch.Tensor,
                                      Z: torch.Tensor, p_col: torch.Tensor, lptr: torch.Tensor,
                                      s: torch.Tensor, gid: torch.Tensor) -> torch.Tensor:
    """edge_mlp_dense_count_lists on R = expf(score) / Z[r] + p_col[v] (Z per ROW); slot j's
    threshold is its own R, formed in the kernel from its raw score s[j] by the same function."""
    ops = _dense_mlp_operands(P, Q, W2, b2, w3, b3)
    _dev(Z, "Z", torch.float32)
    _dev(p_col, "p_col", torch.float32)
    parts, ahead = _count_slots(Q, lptr, s, gid)
    _T().edge_mlp_dense_count_lists_rating_f32(*ops, Z, p_col, lptr, s, gid, parts, ahead)
    return ahead


def rank_resolve_mlp_lists(row_user: torch.Tensor, lptr: torch.Tensor, s: torch.Tensor,
                           gid: torch.Tensor, ahead: torch.Tensor, n_users: int,
                           P: torch.Tensor, Q: torch.Tensor, W2: torch.Tensor, b2: torch.Tensor,
                           w3: torch.Tensor, b3: torch.Tensor,
                           exclude_indptr: Optional[torch.Tensor] = None,
                           exclude_indices: Optional[torch.Tensor] = None,
                           Z: Optional[torch.Tensor] = None,
                           p_col: Optional[torch.Tensor] = None,
                           out: Optional[torch.Tensor] = None,
                           vals: Optional[torch.Tensor] = None):
    """Per row r of a count pass (P row r, user row_user[r], slots [lptr[r], lptr[r + 1]) of
    s / gid / ahead): the row walks its user's exclusion row once and resolves every slot from
    the same scores, rank = 1 + ahead[j] - (the user's excluded items exactly ahead), 0 where
    the slot's item is excluded -> (rank int64 [E], vals fp32 [E]); vals = s, or with Z [R]
    (per row) and p_col [n_items] the entries' R (the excluded items are then compared by R).
    The exclusion CSR (over n_users users, int32) holds each id at most once per row; entries
    < 0 or past the table are skipped.  Scores are bitwise edge_mlp's."""
    _dev(row_user, "row_user", torch.int64)
    _dev(lptr, "lptr", torch.int64)
    _dev(s, "s", torch.float32)
    _dev(gid, "gid", torch.int32)
    _dev(ahead, "ahead", torch.int32)
    ops = _dense_mlp_operands(P, Q, W2, b2, w3, b3)
    if Z is not None:
        _dev(Z, "Z", torch.float32)
    if p_col is not None:
        _dev(p_col, "p_col", torch.float32)
    if out is None:
        out = torch.empty(s.numel(), dtype=torch.int64, device=s.device)
    if vals is None:
        vals = torch.empty(s.numel(), dtype=torch.float32, device=s.device)
    _T().rank_resolve_mlp_lists_f32(row_user, lptr, s, gid, ahead, int(n_users), *ops, Z, p_col,
                                    exclude_indptr, exclude_indices, out, vals)
    return out, vals


def exp_rowsum(scores: torch.Tensor) -> torch.Tensor:
    """Z[r] = sum over the columns of expf(scores[r][c]), in a fixed order -> fp32 [n_rows]."""
    _dev(scores, "scores", torch.float32)
    Z = torch.empty(scores.shape[0], dtype=torch.float32, device=scores.device)
    _T().exp_rowsum_f32(scores, Z)
    return Z


def rating_rows_(scores: torch.Tensor, Z: torch.Tensor, p: torch.Tensor) -> torch.Tensor:
    """scores[r][c] = expf(scores[r][c]) / Z[r] + p[c] in place (the rating of rating.hpp)."""
    _dev(scores, "scores", torch.float32)
    _dev(Z, "Z", torch.float32)
    _dev(p, "p", torch.float32)
    _T().rating_rows_f32(scores, Z, p)
    return scores


def rating_thresholds(tau: torch.Tensor, Z: torch.Tensor, pmax: torch.Tensor) -> torch.Tensor:
    """tau[u] - 2 delta_u rounded down, delta_u = REC_RATING_BAND / Z[u] + 2^-22 |pmax|: the
    rating filter's per-row thresholds (pmax: a one-element tensor, the largest p)."""
    _dev(tau, "tau", torch.float32)
    _dev(Z, "Z", torch.float32)
    _dev(pmax, "pmax", torch.float32)
    thr = torch.empty_like(tau)
    _T().rating_thresholds_f32(tau, Z, pmax, thr)
    return thr


def mask_excluded_mapped(scores: torch.Tensor, col_ids: torch.Tensor,
                         user_rows: Optional[torch.Tensor], exclude_indptr: torch.Tensor,
                         exclude_indices: torch.Tensor) -> None:
    """mask_excluded for a table whose column c stands for item col_ids[c] (int32, strictly
    ascending): the row's excluded items that are among the columns become -inf."""
    _dev(scores, "scores", torch.float32)
    _dev(col_ids, "col_ids", torch.int32)
    _dev(exclude_indptr, "exclude_indptr", torch.int64)
    _dev(exclude_indices, "exclude_indices", torch.int32)
    _T().mask_excluded_mapped_f32(scores, col_ids, user_rows, exclude_indptr, exclude_indices)


def score_bf16_store_rating(users: torch.Tensor, items: torch.Tensor, Z: torch.Tensor,
                            p_col: torch.Tensor) -> torch.Tensor:
    """score_bf16_store with Ra = expf(a) / Z[u] + p_col[c] written instead of a."""
    _dev(users, "users", torch.bfloat16)
    _dev(items, "items", torch.bfloat16)
    _dev(Z, "Z", torch.float32)
    _dev(p_col, "p_col", torch.float32)
    out = torch.empty((users.shape[0], items.shape[0]), dtype=torch.float32, device=users.device)
    _T().score_bf16_store_rating(users, items, Z, p_col, out)
    return out


def score_bf16_filter_rating(users: torch.Tensor, items: torch.Tensor, Z: torch.Tensor,
                             p_col: torch.Tensor, thr: torch.Tensor, counts: torch.Tensor,
                             cand_items: torch.Tensor) -> None:
    """score_bf16_filter with Ra compared: item v joins row u's list where
    Ra(u, v) >= thr[u] (rating_thresholds', compared as they are)."""
    _dev(users, "users", torch.bfloat16)
    _dev(items, "items", torch.bfloat16)
    for t, n in ((Z, "Z"), (p_col, "p_col"), (thr, "thr")):
        _dev(t, n, torch.float32)
    _dev(counts, "counts", torch.int32)
    _dev(cand_items, "cand_items", torch.int32)
    _T().score_bf16_filter_rating(users, items, Z, p_col, thr, counts, cand_items)


def topk_candidates_rating(counts: torch.Tensor, cand_items: torch.Tensor,
                           user_rows: Optional[torch.Tensor], h_user: torch.Tensor,
                           h_item: torch.Tensor, Z: torch.Tensor, p: torch.Tensor, k: int,
                           exclude_indptr: Optional[torch.Tensor] = None,
                           exclude_indices: Optional[torch.Tensor] = None,
                           out_vals: Optional[torch.Tensor] = None,
                           out_idx: Optional[torch.Tensor] = None):
    """topk_candidates ranking by R = expf(cosine) / Z[r] + p[item] (Z per batch row, p per
    item); vals are the R values."""
    _dev(counts, "counts", torch.int32)
    _dev(cand_items, "cand_items", torch.int32)
    _dev(h_user, "h_user", torch.float32)
    _dev(h_item, "h_item", torch.float32)
    _dev(Z, "Z", torch.float32)
    _dev(p, "p", torch.float32)
    B = counts.numel()
    if out_vals is None:
        out_vals = torch.empty((B, k), dtype=torch.float32, device=counts.device)
    if out_idx is None:
        out_idx = torch.empty((B, k), dtype=torch.int64, device=counts.device)
    _T().topk_candidates_rating_f32(counts, cand_items, user_rows, h_user, h_item, exclude_indptr,
                                    exclude_indices, Z, p, int(k), out_vals, out_idx)
    return out_vals, out_idx


def edge_mlp_dense_denominators(P: torch.Tensor, Q: torch.Tensor, W2: torch.Tensor,
                                b2: torch.Tensor, w3: torch.Tensor,
                                b3: torch.Tensor) -> torch.Tensor:
    """Z[u] = sum over all item rows of Q of expf(score(u, v)), score the value of
    edge_mlp_dense_store, nothing else written -> fp32 [B]; the same bits for a row whatever
    batch it is computed in."""
    ops = _dense_mlp_operands(P, Q, W2, b2, w3, b3)
    B = P.shape[0]
    parts = torch.empty((denominator_parts(Q.shape[0]), B), dtype=torch.float32, device=P.device)
    Z = torch.empty(B, dtype=torch.float32, device=P.device)
    _T().edge_mlp_dense_denominators_f32(*ops, parts)
    _T().fold_partials_f32(parts, Z)
    return Z


def edge_mlp_dense_store_rating(P: torch.Tensor, Q: torch.Tensor, W2: torch.Tensor,
                                b2: torch.Tensor, w3: torch.Tensor, b3: torch.Tensor,
                                Z: torch.Tensor, p_col: torch.Tensor) -> torch.Tensor:
    """edge_mlp_dense_store with R = expf(score) / Z[u] + p_col[v] written instead."""
    ops = _dense_mlp_operands(P, Q, W2, b2, w3, b3)
    _dev(Z, "Z", torch.float32)
    _dev(p_col, "p_col", torch.float32)
    out = torch.empty((P.shape[0], Q.shape[0]), dtype=torch.float32, device=P.device)
    _T().edge_mlp_dense_store_rating_f32(*ops, Z, p_col, out)
    return out


def edge_mlp_dense_filter_rating(P: torch.Tensor, Q: torch.Tensor, W2: torch.Tensor,
                                 b2: torch.Tensor, w3: torch.Tensor, b3: torch.Tensor,
                                 Z: torch.Tensor, p_col: torch.Tensor, tau: torch.Tensor,
                                 counts: torch.Tensor, cand_items: torch.Tensor,
                                 cand_scores: torch.Tensor) -> None:
    """edge_mlp_dense_filter with R compared (no band) and kept in cand_scores."""
    ops = _dense_mlp_operands(P, Q, W2, b2, w3, b3)
    for t, n in ((Z, "Z"), (p_col, "p_col"), (tau, "tau"), (cand_scores, "cand_scores")):
        _dev(t, n, torch.float32)
    _dev(counts, "counts", torch.int32)
    _dev(cand_items, "cand_items", torch.int32)
    _T().edge_mlp_dense_filter_rating_f32(*ops, Z, p_col, tau, counts, cand_items, cand_scores)
