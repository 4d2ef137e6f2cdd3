// f1d — popularity-weighted exact top-k for many users without a score matrix: the row
// denominators of the rating (rating.hpp) and the small kernels around them.
//
//   R(u, v) = expf(score(u, v)) / Z_u + p_v,     Z_u = sum over ALL items v of expf(g(u, v))
//
// WHAT g IS.  For the cosine head on the fast path g(u, v) is the fp32 MFMA dot product
// (v_mfma_f32_32x32x2_f32, k ascending) of the two fp32-normalised tables, each row
// x / max(|x|, 1e-12) as normalize_rows_bf16 forms it before rounding.  It is NOT
// cos_score.hpp's wave-per-pair value (the score that is ranked): scoring every pair that way
// costs far more than the MFMA.  g and score differ by the order of d 2^-23, which moves Z_u
// by the same relative amount at most.  Where the widths rule the MFMA kernel out (d % 4 != 0
// or d > 2048) Z_u is summed from the exhaustive score rows instead (exp_rowsum), and g is
// then the score itself.
//
// THE FIXED ORDER.  Z_u is a function of (h_user row, h_item) only — the same bits for any
// batch size, any order or repetition of the served rows, any grid, any run:
//   * the item axis is cut into partials of kZItems = 1024 consecutive items, by n_items
//     alone; a block owns (one partial, one 128-user tile) and nothing else writes its sums;
//   * inside a partial, wave w of the block takes the 32-item subtiles 4 t + w (t ascending);
//     a lane adds expf(g) of its column of each subtile into one register per user row (items
//     past the end are skipped, never scored as zeros), the 32 lanes of a row are folded by
//     an xor tree (offsets 1, 2, 4, 8, 16), the four waves in the order ((w0 + w1) + w2) + w3;
//   * a combine kernel folds a row's partials in index order.
// No float atomics anywhere.  A row's arithmetic does not depend on its place in the tile:
// an MFMA row is computed from that row of A alone, and the folds run along the item axis.
// The partials of a batch are n_items / 1024 x n_users floats: 32 MB for 8192 users x 1M
// items.
//
// THE KERNEL.  The tile loop (staging, swizzle, operand order, the clamped loads past the end)
// is cos_tile.hpp's, shared with the full-ranking count pass (rank.hip); this kernel's epilogue
// adds expf of the lane's column into the row registers and writes nothing but the partials.
#include "common.hpp"
#include "cos_tile.hpp"
#include "rating.hpp"
#include <algorithm>
#include <cmath>

namespace gnnrec {
namespace {

constexpr double kRecEpsD = 0.0078125 + 0.00048828125;  // recommend.hip's eps = 2^-7 + 2^-11
constexpr double kRatingRound = 0x1p-20;  // fp32 rounding of expf and the divide, both sides
constexpr double kRatingSlack = 0x1p-22;  // fp32 rounding of the add, both sides, per unit of p

// ------------------------------------------------------------ normalise ----
// One wave per row, the sum of squares and the divide of normalize_rows_bf16's 16-B path (the
// same bits before its rounding), written as fp32 in the permuted layout above, the pad zero.
__global__ __launch_bounds__(256) void normalize_rows_f32_kernel(
    const float* __restrict__ X, int64_t ld, int64_t n, int d, const int64_t* __restrict__ map,
    float* __restrict__ out, int dpad) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= n) return;  // wave-uniform
  const float* src = X + (map ? map[row] : row) * ld;
  float* dst = out + row * dpad;
  float ss = 0.f;
  for (int c = lane * 4; c < d; c += kWave * 4) {
    const float4 v = *reinterpret_cast<const float4*>(src + c);
    ss += v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w;
  }
#pragma unroll
  for (int off = 1; off < kWave; off <<= 1) ss += __shfl_xor(ss, off);
  const float nrm = fmaxf(sqrtf(ss), 1e-12f);
  for (int c = lane * 4; c < dpad; c += kWave * 4) {
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (c < d) {
      v = *reinterpret_cast<const float4*>(src + c);
      v.x /= nrm; v.y /= nrm; v.z /= nrm; v.w /= nrm;
    }
    // columns q .. q + 3 of a group of 8 (q = 0 or 4) go to (q + j) / 2 + 4 ((q + j) & 1)
    float* g8 = dst + (c & ~7) + ((c & 4) >> 1);
    g8[0] = v.x;
    g8[4] = v.y;
    g8[1] = v.z;
    g8[5] = v.w;
  }
}

// ---------------------------------------------------------- denominators ----
__global__ __launch_bounds__(256, 2) void cos_denominator_kernel(
    const float* __restrict__ U, int64_t B, const float* __restrict__ V, int64_t n, int dpad,
    int64_t n_ut, float* __restrict__ part) {
  __shared__ f32x4 sA[128 * 32];  // [row][chunk ^ (row & 31)]; the wave sums at the end
  const int64_t ut = (int64_t)blockIdx.x % n_ut, pi = (int64_t)blockIdx.x / n_ut;
  float rs[4][16];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) rs[i][r] = 0.f;
  cos_tile_loop(U, B, V, n, dpad, ut, pi, sA, [&](const f32x16(&acc)[4], int64_t) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) rs[i][r] += expf(acc[i][r]);
  });
  fold_tile_rows(rs, reinterpret_cast<float*>(sA), B, ut, pi, part);
}

// Z[u] = the row's partials folded in index order.
__global__ __launch_bounds__(256) void fold_partials_kernel(const float* __restrict__ part,
                                                            int64_t n_part, int64_t B,
                                                            float* __restrict__ Z) {
  const int64_t u = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (u >= B) return;
  float z = 0.f;
  for (int64_t p = 0; p < n_part; ++p) z += part[p * B + u];
  Z[u] = z;
}

// Z[r] = sum of expf over a stored score row, for the widths the MFMA kernel does not take:
// one block per row, thread t adds columns t, t + 256, ... ascending, a wave's lanes are
// folded by the xor tree and the four waves in order.
__global__ __launch_bounds__(256) void exp_rowsum_kernel(const float* __restrict__ S, int64_t ld,
                                                         int64_t n_cols, float* __restrict__ Z) {
  __shared__ float red[4];
  const float* row = S + (int64_t)blockIdx.x * ld;
  float x = 0.f;
  for (int64_t c = threadIdx.x; c < n_cols; c += 256) x += expf(row[c]);
#pragma unroll
  for (int off = 1; off < kWave; off <<= 1) x += __shfl_xor(x, off);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = x;
  __syncthreads();
  if (threadIdx.x == 0) Z[blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}

// S[r][c] = rating(S[r][c], Z[r], p[c]) in place: the exhaustive rows' scores become ratings.
__global__ __launch_bounds__(256) void rating_rows_kernel(float* __restrict__ S, int64_t ld,
                                                          int64_t n_rows, int64_t n_cols,
                                                          const float* __restrict__ Z,
                                                          const float* __restrict__ p) {
  const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (c >= n_cols) return;
  const float pc = p[c];
  for (int64_t r = blockIdx.y; r < n_rows; r += gridDim.y)
    S[r * ld + c] = rating(S[r * ld + c], Z[r], pc);
}

// thr[u] = tau[u] - 2 delta_u rounded down (recommend.hip, THE RATING BAND), formed in
// double once per batch; tau = -inf (fewer than k eligible sample items) stays -inf.
__global__ __launch_bounds__(256) void rating_thresholds_kernel(
    const float* __restrict__ tau, const float* __restrict__ Z, const float* __restrict__ pmax,
    int64_t n, double band, double slack, float* __restrict__ thr) {
  const int64_t u = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (u >= n) return;
  const double t = tau[u];
  const double delta = band / (double)Z[u] + slack * fabs((double)pmax[0]);
  thr[u] = t == -INFINITY ? -INFINITY : __double2float_rd(t - 2.0 * delta);
}

// mask_excluded for a score table whose column c stands for item col_ids[c] (strictly
// ascending): one wave per row, each excluded id looked up by bisection.
__global__ __launch_bounds__(256) void mask_excluded_mapped_kernel(
    float* __restrict__ S, int64_t ld, int64_t n_rows, int64_t n_cols,
    const int32_t* __restrict__ col_ids, const int64_t* __restrict__ user_rows,
    const int64_t* __restrict__ ex_ptr, const int32_t* __restrict__ ex_idx) {
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= n_rows) return;
  const int64_t u = user_rows ? user_rows[row] : row;
  const int64_t e1 = ex_ptr[u + 1];
  for (int64_t e = ex_ptr[u] + (threadIdx.x & 63); e < e1; e += kWave) {
    const int32_t v = ex_idx[e];
    int64_t lo = 0, hi = n_cols;  // first column with id >= v
    while (lo < hi) {
      const int64_t mid = (lo + hi) >> 1;
      if (col_ids[mid] < v) lo = mid + 1;
      else hi = mid;
    }
    if (lo < n_cols && col_ids[lo] == v) S[row * ld + lo] = -INFINITY;
  }
}

}  // namespace
}  // namespace gnnrec

extern "C" int gnnrec_normalize_rows_f32(const float* x, int64_t ld, int64_t n_rows, int64_t d,
                                         const int64_t* row_map, float* out, int64_t dpad,
                                         void* stream) {
  using namespace gnnrec;
  GNNREC_REQUIRE(n_rows >= 0 && d >= 4 && d % 4 == 0 && d <= kZMaxD,
                 "gnnrec_normalize_rows_f32: d must be a multiple of 4 in [4, %d] (got %lld)",
                 kZMaxD, (long long)d);
  GNNREC_REQUIRE(dpad == (d + 7) / 8 * 8,
                 "gnnrec_normalize_rows_f32: dpad must be d rounded up to a multiple of 8 "
                 "(d %lld, dpad %lld)", (long long)d, (long long)dpad);
  if (n_rows == 0) return GNNREC_OK;
  GNNREC_REQUIRE(x && out && ld >= d && ld % 4 == 0,
                 "gnnrec_normalize_rows_f32: bad pointers / ld");
  GNNREC_REQUIRE(aligned16(x) && aligned16(out),
                 "gnnrec_normalize_rows_f32: x and out must be 16-byte aligned");
  GNNREC_REQUIRE((n_rows + 3) / 4 < (int64_t(1) << 31), "gnnrec_normalize_rows_f32: too many rows");
  hipLaunchKernelGGL(normalize_rows_f32_kernel, dim3((unsigned)((n_rows + 3) / 4)), dim3(256), 0,
                     as_stream(stream), x, ld, n_rows, (int)d, row_map, out, (int)dpad);
  return check_launch("gnnrec_normalize_rows_f32");
}

extern "C" int64_t gnnrec_cos_denominator_parts(int64_t n_items) {
  return n_items <= 0 ? 0 : (n_items + gnnrec::kZItems - 1) / gnnrec::kZItems;
}

extern "C" int gnnrec_cos_denominators_f32(const float* users, int64_t n_users, const float* items,
                                           int64_t n_items, int64_t dpad, float* parts, float* Z,
                                           void* stream) {
  using namespace gnnrec;
  const char* fn = "gnnrec_cos_denominators_f32";
  GNNREC_REQUIRE(n_users >= 0 && n_items >= 0, "%s: negative size", fn);
  GNNREC_REQUIRE(dpad >= 8 && dpad % 8 == 0 && dpad <= kZMaxD,
                 "%s: dpad must be a multiple of 8 in [8, %d] (got %lld)", fn, kZMaxD,
                 (long long)dpad);
  if (n_users == 0) return GNNREC_OK;
  GNNREC_REQUIRE(Z, "%s: null Z", fn);
  const int64_t n_part = gnnrec_cos_denominator_parts(n_items), n_ut = (n_users + 127) / 128;
  if (n_items > 0) {
    GNNREC_REQUIRE(users && items && parts && aligned16(users) && aligned16(items),
                   "%s: null or unaligned table", fn);
    GNNREC_REQUIRE(n_part * n_ut < (int64_t(1) << 31), "%s: too many tiles for one launch", fn);
    hipLaunchKernelGGL(cos_denominator_kernel, dim3((unsigned)(n_part * n_ut)), dim3(256), 0,
                       as_stream(stream), users, n_users, items, n_items, (int)dpad, n_ut, parts);
    const int rc = check_launch(fn);
    if (rc != GNNREC_OK) return rc;
  }
  GNNREC_REQUIRE((n_users + 255) / 256 < (int64_t(1) << 31), "%s: too many rows", fn);
  hipLaunchKernelGGL(fold_partials_kernel, dim3((unsigned)((n_users + 255) / 256)), dim3(256), 0,
                     as_stream(stream), parts, n_part, n_users, Z);
  return check_launch(fn);
}

extern "C" int gnnrec_fold_partials_f32(const float* parts, int64_t n_parts, int64_t n_rows,
                                        float* Z, void* stream) {
  using namespace gnnrec;
  GNNREC_REQUIRE(n_parts >= 0 && n_rows >= 0 && (n_rows + 255) / 256 < (int64_t(1) << 31),
                 "gnnrec_fold_partials_f32: bad size");
  if (n_rows == 0) return GNNREC_OK;
  GNNREC_REQUIRE(Z && (n_parts == 0 || parts), "gnnrec_fold_partials_f32: null pointer");
  hipLaunchKernelGGL(fold_partials_kernel, dim3((unsigned)((n_rows + 255) / 256)), dim3(256), 0,
                     as_stream(stream), parts, n_parts, n_rows, Z);
  return check_launch("gnnrec_fold_partials_f32");
}

extern "C" int gnnrec_exp_rowsum_f32(const float* scores, int64_t ld, int64_t n_rows,
                                     int64_t n_cols, float* Z, void* stream) {
  using namespace gnnrec;
  GNNREC_REQUIRE(n_rows >= 0 && n_cols >= 0 && n_rows < (int64_t(1) << 31),
                 "gnnrec_exp_rowsum_f32: bad size");
  if (n_rows == 0) return GNNREC_OK;
  GNNREC_REQUIRE(Z && (n_cols == 0 || (scores && ld >= n_cols)),
                 "gnnrec_exp_rowsum_f32: bad pointers / ld");
  hipLaunchKernelGGL(exp_rowsum_kernel, dim3((unsigned)n_rows), dim3(256), 0, as_stream(stream),
                     scores, ld, n_cols, Z);
  return check_launch("gnnrec_exp_rowsum_f32");
}

extern "C" int gnnrec_rating_rows_f32(float* scores, int64_t ld, int64_t n_rows, int64_t n_cols,
                                      const float* Z, const float* p, void* stream) {
  using namespace gnnrec;
  GNNREC_REQUIRE(n_rows >= 0 && n_cols >= 0 && (n_cols + 255) / 256 < (int64_t(1) << 31),
                 "gnnrec_rating_rows_f32: bad size");
  if (n_rows == 0 || n_cols == 0) return GNNREC_OK;
  GNNREC_REQUIRE(scores && ld >= n_cols && Z && p, "gnnrec_rating_rows_f32: bad pointers / ld");
  const dim3 grid((unsigned)((n_cols + 255) / 256), (unsigned)std::min<int64_t>(n_rows, 1024));
  hipLaunchKernelGGL(rating_rows_kernel, grid, dim3(256), 0, as_stream(stream), scores, ld, n_rows,
                     n_cols, Z, p);
  return check_launch("gnnrec_rating_rows_f32");
}

extern "C" int gnnrec_rating_thresholds_f32(const float* tau, const float* Z, const float* pmax,
                                            int64_t n_rows, float* thr, void* stream) {
  using namespace gnnrec;
  GNNREC_REQUIRE(n_rows >= 0 && (n_rows + 255) / 256 < (int64_t(1) << 31),
                 "gnnrec_rating_thresholds_f32: bad size");
  if (n_rows == 0) return GNNREC_OK;
  GNNREC_REQUIRE(tau && Z && pmax && thr, "gnnrec_rating_thresholds_f32: null pointer");
  // delta_u = e^(1 + eps) ((e^eps - 1) + 2^-20) / Z_u + 2^-22 max p (recommend.hip)
  const double band = std::exp(1.0 + kRecEpsD) * (std::expm1(kRecEpsD) + kRatingRound);
  hipLaunchKernelGGL(rating_thresholds_kernel, dim3((unsigned)((n_rows + 255) / 256)), dim3(256),
                     0, as_stream(stream), tau, Z, pmax, n_rows, band, kRatingSlack, thr);
  return check_launch("gnnrec_rating_thresholds_f32");
}

extern "C" int gnnrec_mask_excluded_mapped_f32(float* scores, int64_t ld, int64_t n_rows,
                                               int64_t n_cols, const int32_t* col_ids,
                                               const int64_t* user_rows,
                                               const int64_t* exclude_indptr,
                                               const int32_t* exclude_indices, void* stream) {
  using namespace gnnrec;
  GNNREC_REQUIRE(n_rows >= 0 && n_cols >= 0 && (n_rows + 3) / 4 < (int64_t(1) << 31),
                 "gnnrec_mask_excluded_mapped_f32: bad size");
  if (n_rows == 0 || n_cols == 0) return GNNREC_OK;
  GNNREC_REQUIRE(scores && ld >= n_cols && col_ids,
                 "gnnrec_mask_excluded_mapped_f32: bad scores / ld / col_ids");
  GNNREC_REQUIRE(exclude_indptr && exclude_indices,
                 "gnnrec_mask_excluded_mapped_f32: null exclusion list");
  hipLaunchKernelGGL(mask_excluded_mapped_kernel, dim3((unsigned)((n_rows + 3) / 4)), dim3(256), 0,
                     as_stream(stream), scores, ld, n_rows, n_cols, col_ids, user_rows,
                     exclude_indptr, exclude_indices);
  return check_launch("gnnrec_mask_excluded_mapped_f32");
}
