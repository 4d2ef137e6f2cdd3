// pack_rows: a dense [n, 128] fp32 table -> packed rows (pack_rows.hpp), the count of rows
// that do not fit (`dense` rows) and the table's packed_ok flag.
//
// Mapping: one 32-lane group per row (two rows per wave), lane l holds columns 4l..4l+3
// from one 16-B non-temporal load (the dense table is a stream here, read once).  A value's
// packed position is a popcount over the four per-bit ballots of the group; the row is
// assembled in the wave's LDS image and leaves as 24 coalesced 16-B stores.
#include "common.hpp"
#include "gather.hpp"
#include "pack_rows.hpp"
#include "rowq.hpp"

namespace gnnrec {
namespace {

__global__ __launch_bounds__(256) void pack_rows_kernel(const float* __restrict__ X, int64_t ldx,
                                                        int64_t n, uint32_t* __restrict__ P,
                                                        int64_t max_dense,
                                                        int* __restrict__ status) {
  __shared__ __attribute__((aligned(16))) uint32_t img[4][2 * kPackWords];
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int grp = lane >> 5, l = lane & 31;
  uint32_t* row_img = img[wave] + grp * kPackWords;
  const uint32_t below = (1u << l) - 1u;
  int n_dense = 0;  // lane 0 of each group counts its group's dense rows
  const int64_t wstride = (int64_t)gridDim.x * 4;
  for (int64_t pair = (int64_t)blockIdx.x * 4 + wave; pair * 2 < n; pair += wstride) {
    const int64_t row = pair * 2 + grp;
    const bool live = row < n;
    uint32_t b[4] = {0u, 0u, 0u, 0u};
    if (live) {
      const float4 t = ld_stream4(X + row * ldx + 4 * l);
      b[0] = __builtin_bit_cast(uint32_t, t.x);
      b[1] = __builtin_bit_cast(uint32_t, t.y);
      b[2] = __builtin_bit_cast(uint32_t, t.z);
      b[3] = __builtin_bit_cast(uint32_t, t.w);
    }
    // ballots of "column 4l + j is non-zero" over the group's 32 lanes
    uint32_t bal[4];
    uint32_t nib = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      nib |= (b[j] != 0u ? 1u : 0u) << j;
      bal[j] = (uint32_t)(__ballot(b[j] != 0u) >> (32 * grp));
    }
    uint32_t p = 0, nnz = 0, pre = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      p += __popc(bal[j] & below);
      nnz += __popc(bal[j]);
#pragma unroll
      for (int w = 1; w < 4; ++w) pre += (uint32_t)__popc(bal[j] & ((1u << (8 * w)) - 1u)) << (8 * w);
    }
    const bool dense = nnz > (uint32_t)kPackSlots;
    // the row's mask word of this lane's octet: the 8 nibbles of lanes 8w..8w+7
    uint32_t m = nib << (4 * (l & 7));
    m |= __shfl_xor(m, 1);
    m |= __shfl_xor(m, 2);
    m |= __shfl_xor(m, 4);
    uint32_t mw[4];
#pragma unroll
    for (int w = 0; w < 4; ++w) mw[w] = __shfl(m, 32 * grp + 8 * w);
    // image: header from lanes 0 and 1, zeros elsewhere, then the values at their positions
    uint4 h = make_uint4(0u, 0u, 0u, 0u);
    if (l == 0) h = make_uint4(mw[0], mw[1], mw[2], mw[3]);
    if (l == 1) h = make_uint4(pre, nnz | (dense ? kPackDenseBit : 0u), 0u, 0u);
    if (l < kPackWords / 4) *reinterpret_cast<uint4*>(row_img + 4 * l) = h;
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    if (!dense) {
      uint32_t q = kPackHdrWords + p;
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (b[j] != 0u) row_img[q++] = b[j];
    }
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    if (live && l < kPackWords / 4)
      *reinterpret_cast<uint4*>(P + row * kPackWords + 4 * l) =
          *reinterpret_cast<const uint4*>(row_img + 4 * l);
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");  // the image is rewritten next
    if (l == 0 && live && dense) ++n_dense;
  }
  // dense rows of the grid, then the last block to finish settles the table's flag and
  // leaves both counters zero for the next launch (the row queue's idiom, rowq.hpp)
  if (n_dense > 0) atomicAdd(status + 2, n_dense);
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned* done = reinterpret_cast<unsigned*>(status + 3);
    if (__hip_atomic_fetch_add(done, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) ==
        gridDim.x - 1) {
      const int total = __hip_atomic_load(status + 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      status[1] = total;
      status[0] = (int64_t)total <= max_dense ? 1 : 0;
      __hip_atomic_store(status + 2, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(done, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

}  // namespace
}  // namespace gnnrec

extern "C" int gnnrec_pack_rows_f32(const float* X, int64_t ldx, int64_t n, int64_t d,
                                    double max_dense_frac, void* packed, int32_t* status,
                                    void* stream) {
  using namespace gnnrec;
  GNNREC_REQUIRE(n >= 0 && n < (int64_t)1 << 31, "gnnrec_pack_rows_f32: bad row count %lld",
                 (long long)n);
  GNNREC_REQUIRE(d == kPackD, "gnnrec_pack_rows_f32: d=%lld (packed rows are %d wide)",
                 (long long)d, kPackD);
  GNNREC_REQUIRE(status, "gnnrec_pack_rows_f32: null status");
  GNNREC_REQUIRE(n == 0 || (X && packed), "gnnrec_pack_rows_f32: null table");
  GNNREC_REQUIRE(ldx >= d && ldx % 4 == 0 && aligned16(X) && aligned16(packed),
                 "gnnrec_pack_rows_f32: needs 16-B aligned rows");
  GNNREC_REQUIRE(!(max_dense_frac > 1.0), "gnnrec_pack_rows_f32: max_dense_frac=%g above 1",
                 max_dense_frac);
  if (max_dense_frac < 0.0) max_dense_frac = kPackMaxDenseFrac;
  const int64_t max_dense = (int64_t)(max_dense_frac * (double)n);
  int64_t blocks = (n + 7) / 8;  // 4 waves x 2 rows
  const int64_t cap = (int64_t)device_cus() * 8;
  if (blocks > cap) blocks = cap;
  if (blocks < 1) blocks = 1;
  hipLaunchKernelGGL(pack_rows_kernel, dim3((unsigned)blocks), dim3(256), 0, as_stream(stream), X,
                     ldx, n, static_cast<uint32_t*>(packed), max_dense, status);
  return check_launch("gnnrec_pack_rows_f32");
}

extern "C" int gnnrec_pack_rows_host(const float* X, int64_t n, void* packed,
                                     int64_t* dense_rows) {
  using namespace gnnrec;
  GNNREC_REQUIRE(n >= 0, "gnnrec_pack_rows_host: negative row count");
  GNNREC_REQUIRE(n == 0 || (X && packed), "gnnrec_pack_rows_host: null table");
  uint32_t* p = static_cast<uint32_t*>(packed);
  int64_t dense = 0;
  for (int64_t r = 0; r < n; ++r) {
    pack_row_host(X + r * kPackD, p + r * kPackWords);
    dense += (p[r * kPackWords + 5] & kPackDenseBit) != 0;
  }
  if (dense_rows) *dense_rows = dense;
  return GNNREC_OK;
}

extern "C" int gnnrec_unpack_rows_host(const void* packed, const float* X_dense, int64_t n,
                                       float* out) {
  using namespace gnnrec;
  GNNREC_REQUIRE(n >= 0, "gnnrec_unpack_rows_host: negative row count");
  GNNREC_REQUIRE(n == 0 || (packed && X_dense && out), "gnnrec_unpack_rows_host: null table");
  const uint32_t* p = static_cast<const uint32_t*>(packed);
  for (int64_t r = 0; r < n; ++r)
    unpack_row_host(p + r * kPackWords, X_dense + r * kPackD, out + r * kPackD);
  return GNNREC_OK;
}
