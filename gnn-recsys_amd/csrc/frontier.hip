// f4 — the dirty-set frontier of an incremental embedding refresh: the
// destinations of one relation's out-edges from a list of dirty source rows, as marks.
//
//   mark[indices[p]] = 1  for every slot p of rows[i]'s range in the source-major CSR
//
// The neighbour list is never materialised, and the work is balanced by EDGE, not by row: a
// Zipf head item has tens of millions of out-edges, and a wave per row would serialise it.
//   degrees   one thread per listed row: its out-degree (0 past the device count, and 0 for
//             an id outside [0, n_src), which sets status[0]); the range is clamped to
//             [0, n_edges] so a malformed indptr cannot send a load outside `indices`;
//   scan      gnnrec_exclusive_scan_i64 in place: off[i] = the first slot of listed row i in
//             the concatenation of the listed ranges, off[n] the total (stays on the device);
//   mark      a fixed grid of waves loops over kTile-slot tiles of the concatenated range; a
//             wave finds its tile's first and last listed row with one wave-uniform search
//             each (csr_merge.hip's shifted copy does the same); a tile inside one row —
//             every tile of a heavy row — is a streamed run of `indices`, else each lane
//             searches the narrowed range.  The loop bound is off[n], read on the device.
// No kernel indexes with an unvalidated id: a bad listed row makes the mark kernel return at
// once (nothing but the status is written), and a neighbour id outside [0, n_dst) is skipped
// and sets status[1].  The stores are plain vector stores of the constant 1: every writer of
// a word stores the same value, so the result does not depend on the order.  The CSR arrays
// are read once and go through the non-temporal loads of gather.hpp.
#include "common.hpp"
#include "gather.hpp"

namespace gnnrec {
namespace {

constexpr int kFT = 256;                 // threads per block: 4 waves = 4 tiles
constexpr int kFRun = 8;                 // slots per lane and tile
constexpr int kFTile = kWave * kFRun;    // 512 slots per wave-tile
constexpr size_t kFAlign = 256;
inline size_t falign(size_t x) { return (x + kFAlign - 1) / kFAlign * kFAlign; }

// the listed rows in play: the host capacity, cut by the device count when there is one
__device__ __forceinline__ int64_t listed(int64_t n, const int64_t* __restrict__ n_dev) {
  if (n_dev == nullptr) return n;
  const int64_t m = *n_dev;
  return m < 0 ? 0 : (m < n ? m : n);
}

// [beg, end) of a validated row, clamped to the edge array
__device__ __forceinline__ void row_range(const int64_t* __restrict__ indptr, int64_t r,
                                          int64_t E, int64_t& beg, int64_t& end) {
  beg = indptr[r];
  end = indptr[r + 1];
  beg = beg < 0 ? 0 : (beg > E ? E : beg);
  end = end < beg ? beg : (end > E ? E : end);
}

__global__ __launch_bounds__(kFT) void frontier_degrees_kernel(
    const int64_t* __restrict__ rows, int64_t n, const int64_t* __restrict__ n_dev,
    const int64_t* __restrict__ indptr, int64_t n_src, int64_t E, int64_t* __restrict__ off,
    int64_t* __restrict__ status) {
  const int64_t m = listed(n, n_dev);
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    int64_t deg = 0;
    if (i < m) {
      const int64_t r = ld_stream(rows + i);
      if (r < 0 || r >= n_src) {
        status[0] = 1;  // benign race: every writer stores 1
      } else {
        int64_t beg, end;
        row_range(indptr, r, E, beg, end);
        deg = end - beg;
      }
    }
    off[i] = deg;
  }
}

// the last i in [lo, hi) with off[i] <= t (off is non-decreasing, off[lo] <= t): the listed
// row that holds slot t — empty rows, whose off equals the next row's, are stepped over
__device__ __forceinline__ int64_t row_of(const int64_t* __restrict__ off, int64_t lo, int64_t hi,
                                          int64_t t) {
  while (hi - lo > 1) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (off[mid] <= t) lo = mid;
    else hi = mid;
  }
  return lo;
}

__global__ __launch_bounds__(kFT) void frontier_mark_kernel(
    const int64_t* __restrict__ rows, int64_t n, const int64_t* __restrict__ off,
    const int64_t* __restrict__ indptr, const int32_t* __restrict__ indices, int64_t E,
    int64_t n_dst, int32_t* __restrict__ mark, int64_t* __restrict__ status) {
  if (status[0]) return;  // a listed row out of range: nothing but the status is written
  const int lane = threadIdx.x & (kWave - 1);
  const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int64_t total = off[n];
  const int64_t n_tiles = (total + kFTile - 1) / kFTile;
  const int64_t wstride = (int64_t)gridDim.x * (kFT / kWave);
  bool bad = false;
  for (int64_t tile = (int64_t)blockIdx.x * (kFT / kWave) + wv; tile < n_tiles; tile += wstride) {
    const int64_t t0 = tile * kFTile;
    const int64_t t1 = t0 + kFTile < total ? t0 + kFTile : total;
    const int64_t lo = row_of(off, 0, n, t0);       // wave-uniform: the tile's first row
    const int64_t hi = row_of(off, lo, n, t1 - 1);  // and its last
    // every listed row with a slot is in range (a bad one has degree 0 and returned above)
    int64_t beg = 0, end = 0, first = 0;
    if (lo == hi) {
      row_range(indptr, rows[lo], E, beg, end);
      first = off[lo];
    }
#pragma unroll
    for (int k = 0; k < kFRun; ++k) {
      const int64_t t = t0 + k * kWave + lane;
      if (t >= t1) continue;
      if (lo != hi) {
        const int64_t i = row_of(off, lo, hi + 1, t);
        row_range(indptr, rows[i], E, beg, end);
        first = off[i];
      }
      const int64_t p = beg + (t - first);
      if (p >= end) continue;  // (cannot happen: off was scanned from these ranges)
      const int64_t v = ld_stream(indices + p);
      if (v < 0 || v >= n_dst) bad = true;
      else mark[v] = 1;
    }
  }
  if (bad) status[1] = 1;
}

inline int hip_ck(hipError_t e, const char* what) {
  if (e == hipSuccess) return GNNREC_OK;
  set_error("%s: %s", what, hipGetErrorString(e));
  return GNNREC_EHIP;
}

}  // namespace
}  // namespace gnnrec

extern "C" size_t gnnrec_frontier_mark_workspace_bytes(int64_t n_rows) {
  if (n_rows < 0) n_rows = 0;
  return gnnrec::falign((size_t)(n_rows + 1) * 8) +
         gnnrec::falign((size_t)gnnrec_scan_workspace_bytes(n_rows)) + gnnrec::kFAlign;
}

extern "C" int gnnrec_frontier_mark(const int64_t* rows, int64_t n_rows, const int64_t* n_rows_dev,
                                    const int64_t* indptr, const int32_t* indices,
                                    int64_t n_edges, int64_t n_src, int64_t n_dst, int32_t* mark,
                                    void* workspace, size_t workspace_bytes, int64_t* status,
                                    void* stream) {
  using namespace gnnrec;
  const int64_t n = n_rows, E = n_edges;
  const int64_t lim = int64_t(1) << 31;
  GNNREC_REQUIRE(n >= 0 && E >= 0 && n_src >= 0 && n_dst >= 0,
                 "gnnrec_frontier_mark: negative size");
  GNNREC_REQUIRE(E < lim && n_src < lim && n_dst < lim,
                 "gnnrec_frontier_mark: %lld edges / %lld x %lld nodes exceed the int32 range",
                 (long long)E, (long long)n_src, (long long)n_dst);
  GNNREC_REQUIRE(status, "gnnrec_frontier_mark: null status");
  // every refusal comes before the first memset or launch
  GNNREC_REQUIRE(n == 0 || (rows && indptr && workspace), "gnnrec_frontier_mark: null pointer");
  GNNREC_REQUIRE(n == 0 || E == 0 || (indices && mark),
                 "gnnrec_frontier_mark: null indices or mark");
  const size_t need = gnnrec_frontier_mark_workspace_bytes(n);
  GNNREC_REQUIRE(n == 0 || workspace_bytes >= need,
                 "gnnrec_frontier_mark: workspace %zu < %zu bytes", workspace_bytes, need);
  hipStream_t s = as_stream(stream);
  int rc = hip_ck(hipMemsetAsync(status, 0, 2 * sizeof(int64_t), s), "gnnrec_frontier_mark");
  if (rc != GNNREC_OK || n == 0) return rc;
  char* base = static_cast<char*>(workspace);
  int64_t* off = reinterpret_cast<int64_t*>(base);
  void* scan_ws = base + falign((size_t)(n + 1) * 8);
  int64_t blocks = (n + kFT - 1) / kFT;
  if (blocks > 256 * 32) blocks = 256 * 32;
  hipLaunchKernelGGL(frontier_degrees_kernel, dim3((unsigned)blocks), dim3(kFT), 0, s, rows, n,
                     n_rows_dev, indptr, n_src, E, off, status);
  rc = gnnrec_exclusive_scan_i64(off, n, off, scan_ws, stream);
  if (rc != GNNREC_OK) return rc;
  if (E > 0) {
    // the listed rows are distinct, so their ranges hold at most E slots: a grid for that
    // many tiles, capped — the kernel's loop bound is the scan's total, read on the device
    int64_t grid = ((E + kFTile - 1) / kFTile + kFT / kWave - 1) / (kFT / kWave);
    if (grid > 256 * 8) grid = 256 * 8;
    hipLaunchKernelGGL(frontier_mark_kernel, dim3((unsigned)grid), dim3(kFT), 0, s, rows, n,
                       (const int64_t*)off, indptr, indices, E, n_dst, mark, status);
  }
  return check_launch("gnnrec_frontier_mark");
}
