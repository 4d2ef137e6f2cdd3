// f3 — graph growth on the device: DGLGraph.add_edges on one relation, as a merge of the batch's
// CSR into the relation's cached dst-major CSR.
//
// The CSR keeps the edges of a row in edge-id order and the new edges take the ids E, E+1, ...,
// so every new edge of a row goes after every old edge of that row: the grown CSR is the old
// one with the batch — sorted by destination, stably — spliced in at the row ends.  That is
// what gnnrec_csr_build gives on the concatenated COO, bit for bit, without sorting the old
// edges again.  With (ipb, ixb, eb) the CSR of the batch alone:
//   validate  one thread per batch edge: an id outside [0, n_src) / [0, n_dst) sets status[1];
//             the batch is copied into the workspace with such ids clamped to 0.  EVERY later
//             kernel reads only that copy or returns when status[1] is set: no kernel indexes
//             with an unvalidated id, and on a bad id nothing but the status is written;
//   build     gnnrec_csr_build of the clamped batch -> ipb, ixb, eb (a sort of n keys);
//   splice    P[t] = indptr[dst[eb[t]] + 1], the old end of batch slot t's row (int32,
//             non-decreasing in t; clamped to [0, E] so that a malformed indptr cannot send a
//             store outside the outputs);
//   indptr    indptr'[r] = indptr[r] + ipb[r]; thread 0 writes status[0];
//   copy      old slot j moves to j + upper_bound(P, j) (the batch slots of the rows before
//             j's).  A wave takes a tile of kTile consecutive old slots and searches P once
//             for each end of the tile (a scalar search: the tile is wave-uniform); when the two
//             ranks agree — nearly every tile when n << E — the tile moves by one shift as a
//             streamed copy, else each lane searches the narrowed range.  Rows play no part;
//   scatter   batch slot t -> position P[t] + t: indices' = ixb[t], eids' = E + eb[t].
// Bytes per old edge: 12 read + 12 written; the batch costs its own CSR build (n edges) plus
// 36 B per batch edge here.  P (4n bytes) is probed at the tile ends only.  The streamed arrays
// go through non-temporal loads and stores.  No host plan and no readback: the caller reads
// the two status words once.
//
// The shifted copy keeps 8-B eids and 4-B indices accesses per lane: a shift by an odd count
// leaves neither side of a wider access aligned (measurement: profiles/add_edges_ab.md).
#include "common.hpp"

namespace gnnrec {
namespace {

constexpr int kMT = 256;                  // threads per block: 4 waves = 4 tiles
constexpr int kRun = 8;                   // old slots per lane and tile
constexpr int kTile = kWave * kRun;       // 512 old slots per wave-tile
constexpr size_t kAlign = 256;
inline size_t align_up(size_t x) { return (x + kAlign - 1) / kAlign * kAlign; }

inline unsigned flat_grid(int64_t n) {
  int64_t b = (n + kMT - 1) / kMT;
  if (b > 256 * 32) b = 256 * 32;
  return (unsigned)(b < 1 ? 1 : b);
}

// byte offsets of the workspace's parts
struct MergeWs {
  size_t src;    // int64 [n]  validated (clamped) copy of the batch
  size_t dst;    // int64 [n]
  size_t ipb;    // int64 [n_dst + 1]  the batch's CSR
  size_t ixb;    // int32 [n]
  size_t eb;     // int64 [n]
  size_t splice; // int32 [n]  P
  size_t build;  // gnnrec_csr_build's workspace
  size_t bytes;
};

inline MergeWs carve(int64_t n, int64_t n_dst) {
  size_t o = 0;
  MergeWs w;
  w.src = o; o += align_up((size_t)n * 8);
  w.dst = o; o += align_up((size_t)n * 8);
  w.ipb = o; o += align_up((size_t)(n_dst + 1) * 8);
  w.ixb = o; o += align_up((size_t)n * 4);
  w.eb = o; o += align_up((size_t)n * 8);
  w.splice = o; o += align_up((size_t)n * 4);
  w.build = o; o += align_up(gnnrec_csr_build_workspace_bytes(n, n_dst));
  w.bytes = o + kAlign;  // (never 0: the torch op allocates at least one part)
  return w;
}

__global__ __launch_bounds__(kMT) void validate_batch_kernel(
    const int64_t* __restrict__ src, const int64_t* __restrict__ dst, int64_t n, int64_t n_src,
    int64_t n_dst, int64_t* __restrict__ src_c, int64_t* __restrict__ dst_c,
    int64_t* __restrict__ status) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    int64_t u = __builtin_nontemporal_load(src + i), v = __builtin_nontemporal_load(dst + i);
    const bool bad = u < 0 || u >= n_src || v < 0 || v >= n_dst;
    if (bad) {
      status[1] = 1;  // benign race: every writer stores 1
      u = 0;
      v = 0;
    }
    src_c[i] = u;
    dst_c[i] = v;
  }
}

// P[t] = the old end of the row of batch slot t.  dst_c is the validated copy and eb comes from
// the library's own builder over n edges, so both indices are in range whatever the status.
__global__ __launch_bounds__(kMT) void splice_points_kernel(
    const int64_t* __restrict__ indptr, const int64_t* __restrict__ dst_c,
    const int64_t* __restrict__ eb, int64_t n, int64_t E, const int64_t* __restrict__ status,
    int32_t* __restrict__ P) {
  if (status[1]) return;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += stride) {
    int64_t p = E > 0 ? indptr[dst_c[eb[t]] + 1] : 0;
    p = p < 0 ? 0 : (p > E ? E : p);
    P[t] = (int32_t)p;
  }
}

// indptr'[r] = indptr[r] + ipb[r]; thread 0 also writes status[0] = E + n (E on a bad id:
// nothing else is written then).  ipb == nullptr: an empty batch.
__global__ __launch_bounds__(kMT) void indptr_add_kernel(
    const int64_t* __restrict__ indptr, const int64_t* __restrict__ ipb, int64_t n_rows1,
    int64_t E, int64_t n, int64_t* __restrict__ status, int64_t* __restrict__ indptr_out) {
  const bool bad = status[1] != 0;
  const int64_t i0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i0 == 0) status[0] = bad ? E : E + n;
  if (bad) return;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t r = i0; r < n_rows1; r += stride)
    indptr_out[r] = (E > 0 ? indptr[r] : 0) + (ipb ? ipb[r] : 0);
}

// the first t in [lo, hi) with P[t] > j (hi when there is none); P is non-decreasing
__device__ __forceinline__ int64_t upper_bound(const int32_t* __restrict__ P, int64_t lo,
                                               int64_t hi, int64_t j) {
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if ((int64_t)P[mid] <= j) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

__global__ __launch_bounds__(kMT) void shifted_copy_kernel(
    const int32_t* __restrict__ indices, const int64_t* __restrict__ eids, int64_t E,
    const int32_t* __restrict__ P, int64_t n, const int64_t* __restrict__ status,
    int32_t* __restrict__ indices_out, int64_t* __restrict__ eids_out) {
  if (status[1]) return;
  const int lane = threadIdx.x & (kWave - 1);
  const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int64_t n_tiles = (E + kTile - 1) / kTile;
  const int64_t wstride = (int64_t)gridDim.x * (kMT / kWave);
  for (int64_t tile = (int64_t)blockIdx.x * (kMT / kWave) + wv; tile < n_tiles; tile += wstride) {
    const int64_t j0 = tile * kTile;
    const int64_t j1 = j0 + kTile < E ? j0 + kTile : E;
    const int64_t lo = upper_bound(P, 0, n, j0);
    const int64_t hi = upper_bound(P, lo, n, j1 - 1);
    if (lo == hi && j1 - j0 == kTile) {  // a whole tile, one shift: the streamed copy
      int32_t x[kRun];
      int64_t e[kRun];
#pragma unroll
      for (int k = 0; k < kRun; ++k) {
        const int64_t j = j0 + k * kWave + lane;
        x[k] = __builtin_nontemporal_load(indices + j);
        e[k] = __builtin_nontemporal_load(eids + j);
      }
#pragma unroll
      for (int k = 0; k < kRun; ++k) {
        const int64_t q = j0 + k * kWave + lane + lo;
        __builtin_nontemporal_store(x[k], indices_out + q);
        __builtin_nontemporal_store(e[k], eids_out + q);
      }
    } else {
#pragma unroll
      for (int k = 0; k < kRun; ++k) {
        const int64_t j = j0 + k * kWave + lane;
        if (j < j1) {
          const int64_t q = j + (lo == hi ? lo : upper_bound(P, lo, hi, j));
          __builtin_nontemporal_store(__builtin_nontemporal_load(indices + j), indices_out + q);
          __builtin_nontemporal_store(__builtin_nontemporal_load(eids + j), eids_out + q);
        }
      }
    }
  }
}

__global__ __launch_bounds__(kMT) void scatter_batch_kernel(
    const int32_t* __restrict__ ixb, const int64_t* __restrict__ eb,
    const int32_t* __restrict__ P, int64_t n, int64_t E, const int64_t* __restrict__ status,
    int32_t* __restrict__ indices_out, int64_t* __restrict__ eids_out) {
  if (status[1]) return;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += stride) {
    const int64_t q = (int64_t)P[t] + t;  // <= E + n - 1 (P is clamped to [0, E])
    indices_out[q] = ixb[t];
    eids_out[q] = E + eb[t];
  }
}

inline int hip_ck(hipError_t e, const char* what) {
  if (e == hipSuccess) return GNNREC_OK;
  set_error("%s: %s", what, hipGetErrorString(e));
  return GNNREC_EHIP;
}

}  // namespace
}  // namespace gnnrec

extern "C" size_t gnnrec_csr_add_edges_workspace_bytes(int64_t n_new, int64_t n_dst) {
  if (n_new < 0) n_new = 0;
  if (n_dst < 0) n_dst = 0;
  return gnnrec::carve(n_new, n_dst).bytes;
}

extern "C" int gnnrec_csr_add_edges(const int64_t* indptr, const int32_t* indices,
                                    const int64_t* eids, int64_t n_edges, int64_t n_src,
                                    int64_t n_dst, const int64_t* src_new,
                                    const int64_t* dst_new, int64_t n_new, void* workspace,
                                    size_t workspace_bytes, int64_t* indptr_out,
                                    int32_t* indices_out, int64_t* eids_out, int64_t* status,
                                    void* stream) {
  using namespace gnnrec;
  const int64_t E = n_edges, n = n_new;
  const int64_t lim = int64_t(1) << 31;
  GNNREC_REQUIRE(E >= 0 && n >= 0 && n_src >= 0 && n_dst >= 0,
                 "gnnrec_csr_add_edges: negative size");
  GNNREC_REQUIRE(E < lim && n < lim && E + n < lim && n_src < lim && n_dst < lim,
                 "gnnrec_csr_add_edges: %lld + %lld edges / %lld x %lld nodes exceed the int32 "
                 "range", (long long)E, (long long)n, (long long)n_src, (long long)n_dst);
  GNNREC_REQUIRE(status && workspace && indptr_out,
                 "gnnrec_csr_add_edges: null status, workspace or indptr_out");
  GNNREC_REQUIRE(E + n == 0 || (n_dst > 0 && n_src > 0),
                 "gnnrec_csr_add_edges: %lld edges between %lld and %lld nodes",
                 (long long)(E + n), (long long)n_src, (long long)n_dst);
  GNNREC_REQUIRE(E == 0 || (indptr && indices && eids), "gnnrec_csr_add_edges: null CSR pointer");
  GNNREC_REQUIRE(n == 0 || (src_new && dst_new), "gnnrec_csr_add_edges: null batch pointer");
  GNNREC_REQUIRE(E + n == 0 || (indices_out && eids_out),
                 "gnnrec_csr_add_edges: null output pointer");
  const size_t need = gnnrec_csr_add_edges_workspace_bytes(n, n_dst);
  GNNREC_REQUIRE(workspace_bytes >= need, "gnnrec_csr_add_edges: workspace %zu < %zu bytes",
                 workspace_bytes, need);
  hipStream_t s = as_stream(stream);
  const MergeWs o = carve(n, n_dst);
  char* base = static_cast<char*>(workspace);
  int64_t* src_c = reinterpret_cast<int64_t*>(base + o.src);
  int64_t* dst_c = reinterpret_cast<int64_t*>(base + o.dst);
  int64_t* ipb = reinterpret_cast<int64_t*>(base + o.ipb);
  int32_t* ixb = reinterpret_cast<int32_t*>(base + o.ixb);
  int64_t* eb = reinterpret_cast<int64_t*>(base + o.eb);
  int32_t* P = reinterpret_cast<int32_t*>(base + o.splice);
  int rc = hip_ck(hipMemsetAsync(status, 0, 2 * sizeof(int64_t), s), "gnnrec_csr_add_edges");
  if (rc != GNNREC_OK) return rc;
  if (n > 0) {
    hipLaunchKernelGGL(validate_batch_kernel, dim3(flat_grid(n)), dim3(kMT), 0, s, src_new,
                       dst_new, n, n_src, n_dst, src_c, dst_c, status);
    rc = gnnrec_csr_build(src_c, dst_c, n, n_dst, base + o.build, o.bytes - o.build, ipb, ixb, eb,
                          s);
    if (rc != GNNREC_OK) return rc;
    hipLaunchKernelGGL(splice_points_kernel, dim3(flat_grid(n)), dim3(kMT), 0, s, indptr,
                       (const int64_t*)dst_c, (const int64_t*)eb, n, E, (const int64_t*)status, P);
  }
  hipLaunchKernelGGL(indptr_add_kernel, dim3(flat_grid(n_dst + 1)), dim3(kMT), 0, s, indptr,
                     n > 0 ? (const int64_t*)ipb : (const int64_t*)nullptr, n_dst + 1, E, n,
                     status, indptr_out);
  if (E > 0)
    hipLaunchKernelGGL(shifted_copy_kernel, dim3(flat_grid((E + kTile - 1) / kTile * kWave)),
                       dim3(kMT), 0, s, indices, eids, E, (const int32_t*)P, n,
                       (const int64_t*)status, indices_out, eids_out);
  if (n > 0)
    hipLaunchKernelGGL(scatter_batch_kernel, dim3(flat_grid(n)), dim3(kMT), 0, s,
                       (const int32_t*)ixb, (const int64_t*)eb, (const int32_t*)P, n, E,
                       (const int64_t*)status, indices_out, eids_out);
  return check_launch("gnnrec_csr_add_edges");
}
