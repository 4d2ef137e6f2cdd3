// f3 — node removal on the device: DGLGraph.remove_nodes as the stream compaction of
// csr_filter.hip, driven by NODE rank tables instead of an edge-id list.  The nodes of one
// type leave its numbering (the survivors keep their order and become 0..N'-1); every
// relation that touches the type loses the edges incident to them, its surviving endpoints
// are relabelled and, where the type is the destination side, the rows of the removed nodes
// leave the cached dst-major CSR.
//
// gnnrec_node_rank_table, once per call and shared by every relation of the type:
//   mark        one removed bit per old node id (mark_removed_kernel of csr_filter.hpp: any
//               order, duplicates allowed, an id outside [0, N) sets status[1]);
//   word_count  kept nodes per word -> gnnrec_exclusive_scan_i32 -> rank[N/32 + 1];
//   outputs     removed[w] (the bits), table[w] = rank[w] << 32 | word — new_id(v) is ONE 8-B
//               probe, the entry format of csr_filter.hip — table[W] = N', and kept[new_id(v)]
//               = v for every kept v (ascending).  Written only when no id was bad.
//
// gnnrec_csr_remove_nodes, one relation (source table, destination table or both):
//   edge_mark   one thread per edge id: probe the endpoints' table words, the wave ballots
//               "edge e is removed" and lane 0 stores the ballot as the two 32-bit words of
//               the edge bitmap — no atomics, no memset;
//   word_count, scan, pack   as remove_edges: new_eid(e) is one probe;
//   coo         one thread per edge id: src' = new_id(src), dst' = new_id(dst) on the
//               relabelled sides, kept_eids, all at new_eid(e);
//   csr_flags   the ballots of the CSR's slots, scan of the chunk counts (csr_filter.hpp);
//   csr_fill    surviving slot j -> its rank: indices' = new_id(indices) when the source side
//               is relabelled, eids' = new_eid(eids);
//   indptr      indptr'[new_id(r)] = the slot rank of indptr[r] for every kept row r (every
//               slot of a removed row is dropped, so the ranks of the kept rows are already
//               those of the compacted CSR), indptr'[n_dst'] = E'.
// The result is bit for bit gnnrec_csr_build of the filtered, relabelled COO with n_dst'
// rows: a CSR row is in edge-id order and both renumberings are monotonic.  No sort, no host
// plan, no readback (the caller reads the two status words, for all relations at once).
//
// Bytes per edge, from the kernels below: edge_mark reads src and dst (16); coo reads them
// again (16) and writes src', dst', kept_eids (24); csr_flags reads eids (8); csr_fill reads
// eids and indices (12) and writes indices', eids' (12): 88 B with nothing removed (72 for
// remove_edges, which has no endpoint pass), 52 + 36 (1 - p) when a share p of the edges
// goes; bitmap, ranks, ballots and prefixes add < 2 B.  The node tables (N/4 bytes per type)
// are probed at random by endpoint id: 250 KB for a million nodes, resident in L2.  The
// streamed arrays go through non-temporal loads and stores.  With indptr_out == NULL (a
// relation whose CSR is not built) the COO alone is compacted: 56 B per edge.
#include "csr_filter.hpp"

namespace gnnrec {
namespace {

// x: the packed entry of v's word
__device__ __forceinline__ bool removed_bit(int64_t x, int64_t v) {
  return ((uint32_t)x >> (v & 31)) & 1u;
}

// the node table's outputs from the workspace (nothing when an id was bad); thread 0 also
// writes status[0] = N' (N when bad)
__global__ __launch_bounds__(kFT) void node_table_out_kernel(
    const uint32_t* __restrict__ mark, const int64_t* __restrict__ rank, int64_t N, int64_t W,
    int64_t* __restrict__ status, uint32_t* __restrict__ removed, int64_t* __restrict__ table,
    int64_t* __restrict__ kept) {
  const bool bad = status[1] != 0;
  const int64_t i0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i0 == 0) status[0] = bad ? N : rank[W];
  if (bad) return;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t v = i0; v < N; v += stride) {
    const int64_t w = v >> 5;
    const uint32_t m = mark[w];
    const int64_t x = (rank[w] << 32) | (int64_t)m;
    if ((v & 31) == 0) {
      removed[w] = m;
      table[w] = x;
    }
    if (!removed_bit(x, v)) __builtin_nontemporal_store(v, kept + new_eid(x, v));
  }
  if (i0 == 0) table[W] = rank[W];
}

// one thread per edge id, whole waves (e - lane is the same in every lane of a wave): the
// ballot of "an endpoint of edge e is removed" is the edge bitmap's words 2c and 2c + 1 of
// chunk c = e / 64.  An endpoint outside its type's range sets status[1] and is not probed.
__global__ __launch_bounds__(kFT) void edge_mark_kernel(
    const int64_t* __restrict__ src, const int64_t* __restrict__ dst, int64_t E, int64_t n_src,
    int64_t n_dst, const int64_t* __restrict__ st, const int64_t* __restrict__ dt, int64_t W,
    uint32_t* __restrict__ mark, int64_t* __restrict__ status) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const int64_t E64 = (E + kWave - 1) / kWave * kWave;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < E64; e += stride) {
    bool rm = false;
    if (e < E) {
      const int64_t s = __builtin_nontemporal_load(src + e);
      const int64_t d = __builtin_nontemporal_load(dst + e);
      if (s < 0 || s >= n_src || d < 0 || d >= n_dst) {
        status[1] = 1;  // benign race: every writer stores 1
        rm = true;
      } else {
        if (st) rm = removed_bit(st[s >> 5], s);
        if (dt && !rm) rm = removed_bit(dt[d >> 5], d);
      }
    }
    const uint64_t b = __ballot(rm);
    if (lane == 0) {
      const int64_t w = (e >> 6) * 2;  // < W
      mark[w] = (uint32_t)b;
      if (w + 1 < W) mark[w + 1] = (uint32_t)(b >> 32);
    }
  }
}

__global__ __launch_bounds__(kFT) void coo_relabel_kernel(
    const int64_t* __restrict__ src, const int64_t* __restrict__ dst, int64_t E,
    const int64_t* __restrict__ mr, const int64_t* __restrict__ st,
    const int64_t* __restrict__ dt, const int64_t* __restrict__ status,
    int64_t* __restrict__ src_out, int64_t* __restrict__ dst_out, int64_t* __restrict__ kept) {
  if (status[1]) return;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < E; e += stride) {
    const int64_t x = mr[e >> 5];
    if (removed_bit(x, e)) continue;
    const int64_t n = new_eid(x, e);
    int64_t s = __builtin_nontemporal_load(src + e);  // (a kept edge: both ids in range)
    int64_t d = __builtin_nontemporal_load(dst + e);
    if (st) s = new_eid(st[s >> 5], s);
    if (dt) d = new_eid(dt[d >> 5], d);
    __builtin_nontemporal_store(s, src_out + n);
    __builtin_nontemporal_store(d, dst_out + n);
    __builtin_nontemporal_store(e, kept + n);
  }
}

__global__ __launch_bounds__(kFT) void csr_fill_relabel_kernel(
    const int32_t* __restrict__ indices, const int64_t* __restrict__ eids, int64_t E, int64_t C,
    int64_t n_src, const int64_t* __restrict__ mr, const int64_t* __restrict__ st,
    const uint64_t* __restrict__ ballot, const int64_t* __restrict__ cpre,
    const int64_t* __restrict__ status, int32_t* __restrict__ indices_out,
    int64_t* __restrict__ eids_out) {
  if (status[1]) return;
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t wave0 = (int64_t)blockIdx.x * (kFT / kWave) + (threadIdx.x >> 6);
  const int64_t wstride = (int64_t)gridDim.x * (kFT / kWave);
  for (int64_t c = wave0; c < C; c += wstride) {
    const uint64_t b = ballot[c];
    if (!((b >> lane) & 1ull)) continue;  // (a kept lane has j < E and its eid in [0, E))
    const int64_t j = c * kWave + lane;
    const int64_t p = cpre[c] + __popcll(b & ((1ull << lane) - 1ull));
    const int64_t e = __builtin_nontemporal_load(eids + j);
    int64_t s = __builtin_nontemporal_load(indices + j);
    // (indices[j] = src[eids[j]], in range for a kept edge; a CSR that disagrees with its COO
    // is not probed out of range)
    if (st && s >= 0 && s < n_src) s = new_eid(st[s >> 5], s);
    __builtin_nontemporal_store((int32_t)s, indices_out + p);
    __builtin_nontemporal_store(new_eid(mr[e >> 5], e), eids_out + p);
  }
}

// indptr'[new_id(r)] = kept slots before slot indptr[r] for the kept rows r, indptr'[n_new] =
// E'; thread 0 also writes status[0] = E' (E when an endpoint was out of range: nothing else
// is written then).  indptr_out == NULL: the status word alone (cpre = the edge ranks, C = W).
__global__ __launch_bounds__(kFT) void indptr_relabel_kernel(
    const int64_t* __restrict__ indptr, int64_t n_dst, int64_t n_new, int64_t E, int64_t C,
    const int64_t* __restrict__ dt, const uint64_t* __restrict__ ballot,
    const int64_t* __restrict__ cpre, int64_t* __restrict__ status,
    int64_t* __restrict__ indptr_out) {
  const bool bad = status[1] != 0;
  const int64_t i0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i0 == 0) status[0] = bad ? E : cpre[C];
  if (bad || !indptr_out) return;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t r = i0; r <= n_dst; r += stride) {
    if (r == n_dst) {
      indptr_out[n_new] = cpre[C];
      continue;
    }
    int64_t nr = r;
    if (dt) {
      const int64_t x = dt[r >> 5];
      if (removed_bit(x, r)) continue;
      nr = new_eid(x, r);
    }
    if (nr >= n_new) continue;  // (a table that is not this call's: never out of bounds)
    const int64_t p = E > 0 ? indptr[r] : 0;
    int64_t q;
    if (p >= E) q = cpre[C];
    else if (p < 0) q = 0;
    else q = cpre[p >> 6] + __popcll(ballot[p >> 6] & ((1ull << (p & 63)) - 1ull));
    indptr_out[nr] = q;
  }
}

}  // namespace
}  // namespace gnnrec

extern "C" size_t gnnrec_node_rank_table_workspace_bytes(int64_t n_nodes) {
  if (n_nodes < 0) n_nodes = 0;
  return gnnrec::carve(n_nodes).bytes;
}

extern "C" int gnnrec_node_rank_table(const int64_t* nids, int64_t n_ids, int64_t n_nodes,
                                      void* workspace, size_t workspace_bytes,
                                      uint32_t* removed, int64_t* table, int64_t* kept,
                                      int64_t* status, void* stream) {
  using namespace gnnrec;
  const int64_t N = n_nodes, R = n_ids;
  GNNREC_REQUIRE(N >= 0 && R >= 0, "gnnrec_node_rank_table: negative size");
  GNNREC_REQUIRE(N < (int64_t(1) << 31), "gnnrec_node_rank_table: %lld nodes exceed the int32 "
                 "range", (long long)N);
  GNNREC_REQUIRE(status && workspace && table,
                 "gnnrec_node_rank_table: null status, workspace or table");
  GNNREC_REQUIRE(R == 0 || nids, "gnnrec_node_rank_table: null id list");
  GNNREC_REQUIRE(N == 0 || (removed && kept), "gnnrec_node_rank_table: null output");
  const size_t need = gnnrec_node_rank_table_workspace_bytes(N);
  GNNREC_REQUIRE(workspace_bytes >= need, "gnnrec_node_rank_table: workspace %zu < %zu bytes",
                 workspace_bytes, need);
  hipStream_t s = as_stream(stream);
  const FilterPtrs w = filter_ptrs(workspace, carve(N));
  const int64_t W = (N + 31) / 32;
  int rc = hip_ck(hipMemsetAsync(status, 0, 2 * sizeof(int64_t), s), "gnnrec_node_rank_table");
  if (rc != GNNREC_OK) return rc;
  if (W > 0) {
    rc = hip_ck(hipMemsetAsync(w.mark, 0, (size_t)W * 4, s), "gnnrec_node_rank_table");
    if (rc != GNNREC_OK) return rc;
  }
  if (R > 0)
    hipLaunchKernelGGL(mark_removed_kernel, dim3(flat_grid(R)), dim3(kFT), 0, s, nids, R, N,
                       w.mark, status);
  if (N > 0)
    hipLaunchKernelGGL(word_count_kernel, dim3(flat_grid(W)), dim3(kFT), 0, s, w.mark, N, W,
                       w.wcnt);
  rc = gnnrec_exclusive_scan_i32(w.wcnt, W, w.rank, w.scan_ws, s);  // (W == 0: rank[0] = 0)
  if (rc != GNNREC_OK) return rc;
  hipLaunchKernelGGL(node_table_out_kernel, dim3(flat_grid(N)), dim3(kFT), 0, s,
                     (const uint32_t*)w.mark, (const int64_t*)w.rank, N, W, status, removed, table,
                     kept);
  return check_launch("gnnrec_node_rank_table");
}

extern "C" size_t gnnrec_csr_remove_nodes_workspace_bytes(int64_t n_edges, int64_t n_dst) {
  (void)n_dst;
  if (n_edges < 0) n_edges = 0;
  return gnnrec::carve(n_edges).bytes;
}

extern "C" int gnnrec_csr_remove_nodes(const int64_t* src, const int64_t* dst,
                                       const int64_t* indptr, const int32_t* indices,
                                       const int64_t* eids, int64_t n_edges, int64_t n_src,
                                       int64_t n_dst, const int64_t* src_table,
                                       const int64_t* dst_table, int64_t n_dst_new,
                                       void* workspace, size_t workspace_bytes, int64_t* src_out,
                                       int64_t* dst_out, int64_t* kept_eids, int64_t* indptr_out,
                                       int32_t* indices_out, int64_t* eids_out, int64_t* status,
                                       void* stream) {
  using namespace gnnrec;
  const int64_t E = n_edges;
  GNNREC_REQUIRE(E >= 0 && n_src >= 0 && n_dst >= 0 && n_dst_new >= 0,
                 "gnnrec_csr_remove_nodes: negative size");
  GNNREC_REQUIRE(E < (int64_t(1) << 31) && n_src < (int64_t(1) << 31) &&
                     n_dst < (int64_t(1) << 31),
                 "gnnrec_csr_remove_nodes: %lld edges / %lld x %lld nodes exceed the int32 range",
                 (long long)E, (long long)n_src, (long long)n_dst);
  GNNREC_REQUIRE(dst_table ? n_dst_new <= n_dst : n_dst_new == n_dst,
                 "gnnrec_csr_remove_nodes: %lld new rows from %lld (%s destination table)",
                 (long long)n_dst_new, (long long)n_dst, dst_table ? "a" : "no");
  GNNREC_REQUIRE(status && workspace, "gnnrec_csr_remove_nodes: null status or workspace");
  GNNREC_REQUIRE(E == 0 || (src && dst && src_out && dst_out && kept_eids),
                 "gnnrec_csr_remove_nodes: null pointer");
  const bool csr = indptr_out != nullptr;  // else the COO alone (no CSR cached yet)
  GNNREC_REQUIRE(!csr || E == 0 || (indptr && indices && eids && indices_out && eids_out),
                 "gnnrec_csr_remove_nodes: null CSR pointer");
  const size_t need = gnnrec_csr_remove_nodes_workspace_bytes(E, n_dst);
  GNNREC_REQUIRE(workspace_bytes >= need, "gnnrec_csr_remove_nodes: workspace %zu < %zu bytes",
                 workspace_bytes, need);
  hipStream_t s = as_stream(stream);
  const FilterPtrs w = filter_ptrs(workspace, carve(E));
  const int64_t W = (E + 31) / 32, C = (E + 63) / 64;
  int rc = hip_ck(hipMemsetAsync(status, 0, 2 * sizeof(int64_t), s), "gnnrec_csr_remove_nodes");
  if (rc != GNNREC_OK) return rc;
  if (E > 0) {
    hipLaunchKernelGGL(edge_mark_kernel, dim3(flat_grid(E)), dim3(kFT), 0, s, src, dst, E, n_src,
                       n_dst, src_table, dst_table, W, w.mark, status);
    hipLaunchKernelGGL(word_count_kernel, dim3(flat_grid(W)), dim3(kFT), 0, s, w.mark, E, W,
                       w.wcnt);
  }
  rc = gnnrec_exclusive_scan_i32(w.wcnt, W, w.rank, w.scan_ws, s);  // (W == 0: rank[0] = 0)
  if (rc != GNNREC_OK) return rc;
  if (E > 0) {
    hipLaunchKernelGGL(pack_rank_kernel, dim3(flat_grid(W)), dim3(kFT), 0, s, w.mark, W, w.rank);
    hipLaunchKernelGGL(coo_relabel_kernel, dim3(flat_grid(E)), dim3(kFT), 0, s, src, dst, E,
                       (const int64_t*)w.rank, src_table, dst_table, (const int64_t*)status,
                       src_out, dst_out, kept_eids);
  }
  if (!csr) {  // status[0] = rank[W] = E'
    hipLaunchKernelGGL(indptr_relabel_kernel, dim3(1), dim3(kFT), 0, s, (const int64_t*)nullptr,
                       (int64_t)0, (int64_t)0, E, W, (const int64_t*)nullptr,
                       (const uint64_t*)nullptr, (const int64_t*)w.rank, status,
                       (int64_t*)nullptr);
    return check_launch("gnnrec_csr_remove_nodes");
  }
  const unsigned chunk_grid = flat_grid(C * kWave);
  if (E > 0)
    hipLaunchKernelGGL(csr_flags_kernel, dim3(chunk_grid), dim3(kFT), 0, s, eids, E, C, w.mark,
                       w.ballot, w.ccnt);
  rc = gnnrec_exclusive_scan_i32(w.ccnt, C, w.cpre, w.scan_ws, s);
  if (rc != GNNREC_OK) return rc;
  if (E > 0)
    hipLaunchKernelGGL(csr_fill_relabel_kernel, dim3(chunk_grid), dim3(kFT), 0, s, indices, eids,
                       E, C, n_src, (const int64_t*)w.rank, src_table, (const uint64_t*)w.ballot,
                       (const int64_t*)w.cpre, (const int64_t*)status, indices_out, eids_out);
  hipLaunchKernelGGL(indptr_relabel_kernel, dim3(flat_grid(n_dst + 1)), dim3(kFT), 0, s, indptr,
                     n_dst, n_dst_new, E, C, dst_table, (const uint64_t*)w.ballot,
                     (const int64_t*)w.cpre, status, indptr_out);
  return check_launch("gnnrec_csr_remove_nodes");
}
