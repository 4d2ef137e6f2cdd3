// f3 — edge removal on the device: DGLGraph.remove_edges (the reference's train_valid_split,
// src/sampling.py:5-114, removes the validation edges and their reverses from a clone of the
// graph) as a stream compaction of the relation's COO and of its cached dst-major CSR.
//
// The CSR keeps the edges of a row in edge-id order and remove_edges renumbers the surviving
// edges monotonically, so the CSR of the surviving edges is the old CSR with the removed
// slots squeezed out and every eid renumbered — what gnnrec_csr_build gives on the masked COO,
// bit for bit, without a sort:
//   mark        edge_mark: one bit per old edge id (ceil(E/32) words, zeroed), set by atomicOr
//               for every id of the removal list (any order, duplicates allowed).  A wave
//               first ORs the bits of neighbouring lanes that fall in the same word (a
//               segmented scan by shuffles) and the last lane of each run issues one atomic:
//               a sorted list — the split's "last 20 %" — costs 2-3 atomics per wave, not 64
//               on two addresses.  An id outside [0, E) sets status[1] instead;
//   word_count  kept edges per word -> gnnrec_exclusive_scan_i32 -> rank[E/32 + 1]: the scan
//               runs over E/32 entries;
//   pack        rank[w] = rank[w] << 32 | word (in place; a rank fits 31 bits), so
//               new_eid(e) = (x >> 32) + popc(~word & lowmask(e & 31)) costs ONE 8-B probe
//               x = rank[e >> 5] where it is looked up at random (csr_fill);
//   coo         one thread per edge id: src', dst', kept_eids at new_eid(e) — 8-B loads and
//               stores, both contiguous across the wave;
//   csr_flags   one lane per CSR slot: the wave ballots "slot j's edge survives" and stores
//               the 64-bit ballot and its popcount (E/8 + E/16 bytes);
//   scan        of the E/64 chunk counts -> chunk_prefix;
//   csr_fill    surviving slot j -> chunk_prefix[j >> 6] + popc(ballot below the lane):
//               indices' = indices, eids' = new_eid(eids);
//   indptr      indptr'[r] = the slot rank of indptr[r], from the stored ballot of its chunk.
// Bytes per edge: COO 16 read + 24 written, CSR eids read twice (16) + indices 4 read, 12
// written, bitmap / ranks / ballots / prefixes < 2: 72 B with nothing removed, 70 B at 10 %.
// Every array is touched once or twice; the bitmap (E/8 bytes) and the packed ranks (E/4)
// are probed at random by eid and stay in L2 / the Infinity Cache.  The streamed arrays go
// through non-temporal loads and stores.  No sort, no host plan and no readback: the caller
// reads the two status words once.  With indptr_out == NULL (a relation whose CSR is not built
// yet) only the COO is compacted.
//
// Measured on C2's buys relation (50M edges, the last 10 % removed; profiles/
// remove_edges_ab.md): this form 1.7 ms per relation, output allocation and status readback included.  A first form — one atomic per removed
// id, one thread per PAIR of edge ids with 16-B loads (its stores then have stride 2 across
// the wave), separate 4-B word and 8-B rank probes in csr_fill — took 3.1 ms: mark 0.24 ->
// 0.10 ms, coo 1.07 -> 0.44 ms, csr_fill 1.31 -> 0.69 ms.
// mark, word_count, pack, new_eid and csr_flags live in csr_filter.hpp: node removal
// (csr_remove_nodes.hip) runs the same compaction from an edge bitmap it forms itself.
#include "csr_filter.hpp"

namespace gnnrec {
namespace {

__global__ __launch_bounds__(kFT) void coo_compact_kernel(
    const int64_t* __restrict__ src, const int64_t* __restrict__ dst, int64_t E,
    const int64_t* __restrict__ mr, const int64_t* __restrict__ status,
    int64_t* __restrict__ src_out, int64_t* __restrict__ dst_out, int64_t* __restrict__ kept) {
  if (status[1]) return;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < E; e += stride) {
    const int64_t x = mr[e >> 5];
    if (((uint32_t)x >> (e & 31)) & 1u) continue;
    const int64_t n = new_eid(x, e);
    __builtin_nontemporal_store(__builtin_nontemporal_load(src + e), src_out + n);
    __builtin_nontemporal_store(__builtin_nontemporal_load(dst + e), dst_out + n);
    __builtin_nontemporal_store(e, kept + n);
  }
}

__global__ __launch_bounds__(kFT) void csr_fill_kernel(
    const int32_t* __restrict__ indices, const int64_t* __restrict__ eids, int64_t E, int64_t C,
    const int64_t* __restrict__ mr, const uint64_t* __restrict__ ballot,
    const int64_t* __restrict__ cpre, const int64_t* __restrict__ status,
    int32_t* __restrict__ indices_out, int64_t* __restrict__ eids_out) {
  if (status[1]) return;
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t wave0 = (int64_t)blockIdx.x * (kFT / kWave) + (threadIdx.x >> 6);
  const int64_t wstride = (int64_t)gridDim.x * (kFT / kWave);
  for (int64_t c = wave0; c < C; c += wstride) {
    const uint64_t b = ballot[c];
    if (!((b >> lane) & 1ull)) continue;  // (a kept lane has j < E)
    const int64_t j = c * kWave + lane;
    const int64_t p = cpre[c] + __popcll(b & ((1ull << lane) - 1ull));
    const int64_t e = __builtin_nontemporal_load(eids + j);
    __builtin_nontemporal_store(__builtin_nontemporal_load(indices + j), indices_out + p);
    __builtin_nontemporal_store(new_eid(mr[e >> 5], e), eids_out + p);
  }
}

// indptr'[r] = kept slots before slot indptr[r]; thread 0 also writes status[0] = E'
// (E when the removal list held a bad id: nothing else is written then)
__global__ __launch_bounds__(kFT) void indptr_rank_kernel(
    const int64_t* __restrict__ indptr, int64_t n_rows1, int64_t E, int64_t C,
    const uint64_t* __restrict__ ballot, const int64_t* __restrict__ cpre,
    int64_t* __restrict__ status, int64_t* __restrict__ indptr_out) {
  const bool bad = status[1] != 0;
  const int64_t i0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i0 == 0) status[0] = bad ? E : cpre[C];
  if (bad) return;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t r = i0; r < n_rows1; r += stride) {
    const int64_t p = E > 0 ? indptr[r] : 0;
    int64_t q;
    if (p >= E) q = cpre[C];
    else if (p < 0) q = 0;
    else q = cpre[p >> 6] + __popcll(ballot[p >> 6] & ((1ull << (p & 63)) - 1ull));
    indptr_out[r] = q;
  }
}

}  // namespace
}  // namespace gnnrec

extern "C" size_t gnnrec_csr_remove_edges_workspace_bytes(int64_t n_edges, int64_t n_dst) {
  (void)n_dst;
  if (n_edges < 0) n_edges = 0;
  return gnnrec::carve(n_edges).bytes;
}

extern "C" int gnnrec_csr_remove_edges(const int64_t* src, const int64_t* dst,
                                       const int64_t* indptr, const int32_t* indices,
                                       const int64_t* eids, int64_t n_edges, int64_t n_dst,
                                       const int64_t* rm, int64_t n_rm, void* workspace,
                                       size_t workspace_bytes, int64_t* src_out,
                                       int64_t* dst_out, int64_t* kept_eids, int64_t* indptr_out,
                                       int32_t* indices_out, int64_t* eids_out, int64_t* status,
                                       void* stream) {
  using namespace gnnrec;
  const int64_t E = n_edges, R = n_rm;
  GNNREC_REQUIRE(E >= 0 && n_dst >= 0 && R >= 0, "gnnrec_csr_remove_edges: negative size");
  GNNREC_REQUIRE(E < (int64_t(1) << 31) && n_dst < (int64_t(1) << 31),
                 "gnnrec_csr_remove_edges: %lld edges / %lld rows exceed the int32 range",
                 (long long)E, (long long)n_dst);
  GNNREC_REQUIRE(status && workspace, "gnnrec_csr_remove_edges: null status or workspace");
  GNNREC_REQUIRE(R == 0 || rm, "gnnrec_csr_remove_edges: null removal list");
  GNNREC_REQUIRE(E == 0 || (src && dst && src_out && dst_out && kept_eids),
                 "gnnrec_csr_remove_edges: null pointer");
  const bool csr = indptr_out != nullptr;  // else the COO alone (no CSR cached yet)
  GNNREC_REQUIRE(!csr || E == 0 || n_dst > 0, "gnnrec_csr_remove_edges: %lld edges in 0 rows",
                 (long long)E);
  GNNREC_REQUIRE(!csr || E == 0 || (indptr && indices && eids && indices_out && eids_out),
                 "gnnrec_csr_remove_edges: null CSR pointer");
  const size_t need = gnnrec_csr_remove_edges_workspace_bytes(E, n_dst);
  GNNREC_REQUIRE(workspace_bytes >= need, "gnnrec_csr_remove_edges: workspace %zu < %zu bytes",
                 workspace_bytes, need);
  hipStream_t s = as_stream(stream);
  const FilterWs o = carve(E);
  const FilterPtrs w = filter_ptrs(workspace, o);
  const int64_t W = (E + 31) / 32, C = (E + 63) / 64;
  int rc = hip_ck(hipMemsetAsync(status, 0, 2 * sizeof(int64_t), s), "gnnrec_csr_remove_edges");
  if (rc != GNNREC_OK) return rc;
  if (W > 0) {
    rc = hip_ck(hipMemsetAsync(w.mark, 0, (size_t)W * 4, s), "gnnrec_csr_remove_edges");
    if (rc != GNNREC_OK) return rc;
  }
  if (R > 0)
    hipLaunchKernelGGL(mark_removed_kernel, dim3(flat_grid(R)), dim3(kFT), 0, s, rm, R, E, w.mark,
                       status);
  if (E > 0)
    hipLaunchKernelGGL(word_count_kernel, dim3(flat_grid(W)), dim3(kFT), 0, s, w.mark, E, W,
                       w.wcnt);
  rc = gnnrec_exclusive_scan_i32(w.wcnt, W, w.rank, w.scan_ws, s);  // (W == 0: rank[0] = 0)
  if (rc != GNNREC_OK) return rc;
  if (E > 0) {
    hipLaunchKernelGGL(pack_rank_kernel, dim3(flat_grid(W)), dim3(kFT), 0, s, w.mark, W, w.rank);
    hipLaunchKernelGGL(coo_compact_kernel, dim3(flat_grid(E)), dim3(kFT), 0, s, src, dst, E,
                       (const int64_t*)w.rank, status, src_out, dst_out, kept_eids);
  }
  if (!csr) {  // status[0] = rank[W] = E'
    hipLaunchKernelGGL(indptr_rank_kernel, dim3(1), dim3(kFT), 0, s, (const int64_t*)nullptr,
                       (int64_t)0, E, W, (const uint64_t*)nullptr, (const int64_t*)w.rank, status,
                       (int64_t*)nullptr);
    return check_launch("gnnrec_csr_remove_edges");
  }
  const unsigned chunk_grid = flat_grid(C * kWave);
  if (E > 0)
    hipLaunchKernelGGL(csr_flags_kernel, dim3(chunk_grid), dim3(kFT), 0, s, eids, E, C, w.mark,
                       w.ballot, w.ccnt);
  rc = gnnrec_exclusive_scan_i32(w.ccnt, C, w.cpre, w.scan_ws, s);
  if (rc != GNNREC_OK) return rc;
  if (E > 0)
    hipLaunchKernelGGL(csr_fill_kernel, dim3(chunk_grid), dim3(kFT), 0, s, indices, eids, E, C,
                       (const int64_t*)w.rank, w.ballot, w.cpre, status, indices_out, eids_out);
  hipLaunchKernelGGL(indptr_rank_kernel, dim3(flat_grid(n_dst + 1)), dim3(kFT), 0, s, indptr,
                     n_dst + 1, E, C, (const uint64_t*)w.ballot, (const int64_t*)w.cpre, status,
                     indptr_out);
  return check_launch("gnnrec_csr_remove_edges");
}
