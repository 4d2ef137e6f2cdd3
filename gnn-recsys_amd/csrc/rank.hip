// f1f — the exact rank of held-out items among all items, without a score matrix
// (recs.rank_items).
//
//   s(u, v)    = the value gnnrec_sddmm_cos_f32 returns for the pair (what recommend ranks by)
//   rank(u, g) = 1 + #{ v not in exclude(u), v != g : s(u,v) > s(u,g) or (s(u,v) == s(u,g), v < g) }
//   rank(u, g) = 0 where g is in exclude(u)
//
// Rows are PAIRS (u_r, g_r).  Two kernels:
//
//   rank_count    one fp32 MFMA pass over all items (cos_tile.hpp's loop, the one the rating
//                 denominators run): a(r, v) = the MFMA dot of the fp32-normalised rows of u_r
//                 and v.  With the row's threshold t_r = s(u_r, g_r) (computed beforehand by
//                 the per-pair cosine kernel: sddmm_cos's bits) and eps >= |a - s|:
//                   a > t_r + eps   v is provably ahead of g_r: counted (an integer per row,
//                                   summed in registers, folded as the denominators fold expf,
//                                   then over the partials; integers: no order to fix)
//                   a < t_r - eps   v is provably behind: dropped
//                   otherwise       v joins the row's band list [R, cap] through an int32
//                                   atomicAdd on the row's band count, which keeps counting
//                                   past cap (ids are stored only below it)
//                 The two bounds are formed once per block, in double, hi = t + eps rounded UP
//                 and lo = t - eps rounded DOWN to fp32 (eps itself carries a 2^-30 relative
//                 guard for the double add), and kept in LDS (1 KB beside the 64 KB row image):
//                 a lane reads the bounds of four consecutive rows with one ds_read_b128 that
//                 every lane of a half-wave addresses alike (a broadcast) — 64 accumulators and
//                 64 counters per lane leave no room for 128 bound registers.  Rows past the
//                 end get hi = -inf, lo = +inf: they count (into registers nobody reads) and
//                 never append.
//   rank_resolve  one wave per pair: the band items rescored with cos_pair_vec4 (sddmm_cos's
//                 bits) and those exactly ahead under the tie rule counted; the user's excluded
//                 items (the caller hands a CSR whose duplicate ids are replaced by -1)
//                 rescored the same way and those exactly ahead counted; a flag where g itself
//                 is excluded.  rank = 1 + ahead + band_ahead - excluded_ahead, or 0.  The
//                 excluded count is exact arithmetic on its own: an excluded item was counted by
//                 the pass (ahead, or band and then band_ahead) exactly when it is exactly
//                 ahead, so the subtraction never needs the pass's classification.
//                 Rows whose band count exceeds cap are left to the caller (rank -1), who
//                 redoes them exhaustively.
//
// THE BOUND eps(d).  u = 2^-24.  x, y the raw rows, c their exact cosine.  Norms in fp32's
// normal range and away from the 1e-12 guard (or exactly zero), as for REC_EPS.
//   the fp32 norm   ss = a sum of d rounded squares, any order: ss = |x|^2 (1 + th), |th| <= d u;
//                   nrm = sqrt rounded: |x| (1 + e), |e| <= d u / 2 + u.
//   a   each normalised entry x_i / nrm is rounded once (u), so the exact dot of the two
//       normalised rows differs from c by at most (2 u + 2 (d u / 2 + u)) sum |x_i y_i| /
//       (|x| |y|) <= (d + 4) u; on gfx950 the MFMA dot is an fmaf chain, k ascending, one
//       rounding per step: at most d u sum |x^_i y^_i| <= d u more (pad columns add exact
//       zeros).                                                   |a - c| <= (2 d + 4) u
//   s   cos_pair_vec4: every product passes through at most 4 (dot4) + d / (4 LPR)
//       (the lane's running sum) + 6 (the DPP tree) <= d + 8 roundings: |dot - x.y| <=
//       (d + 8) u |x| |y|; the two norms as above, their product and the divide one rounding
//       each: relative (d u + 2 u) + 2 u.                         |s - c| <= (2 d + 12) u
//   Second-order terms are below (4 d u)^2 / 2 <= 2^-23 at d = 2048, under 16 u.  Hence
//       eps(d) = (4 d + 32) 2^-24,   d the padded width (d rounded up to a multiple of 8):
//   3.2e-5 at d = 128, 4.9e-4 at d = 2048.  It is derived, not tuned; the device test only
//   confirms it (profiles/rank_device_bound.md).
#include "common.hpp"
#include "cos_score.hpp"
#include "cos_tile.hpp"
#include "fold_i32.hpp"
#include <cmath>

namespace gnnrec {
namespace {

constexpr int kRankCandMax = 4096;

inline double rank_eps(int64_t dpad) { return (4.0 * (double)dpad + 32.0) * 0x1p-24; }

// ------------------------------------------------------------------ count ----
__global__ __launch_bounds__(256, 2) void rank_count_kernel(
    const float* __restrict__ U, int64_t B, const float* __restrict__ V, int64_t n, int dpad,
    int64_t n_ut, const float* __restrict__ thr, double eps, int* __restrict__ part,
    int* __restrict__ band_cnt, int* __restrict__ band, int cap) {
  __shared__ f32x4 sA[128 * 32];
  __shared__ f32x4 sHi[32], sLo[32];  // the bounds of row 4 q + j in [q][j]
  const int tid = threadIdx.x;
  const int h = (tid & 63) >> 5;
  const int64_t ut = (int64_t)blockIdx.x % n_ut, pi = (int64_t)blockIdx.x / n_ut;
  if (tid < 128) {
    const int64_t row = ut * 128 + tid;
    float hi = -INFINITY, lo = INFINITY;
    if (row < B) {
      const double t = thr[row];
      hi = __double2float_ru(t + eps);
      lo = __double2float_rd(t - eps);
    }
    reinterpret_cast<float*>(sHi)[tid] = hi;
    reinterpret_cast<float*>(sLo)[tid] = lo;
  }
  __syncthreads();
  int cnt[4][16];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) cnt[i][r] = 0;
  cos_tile_loop(U, B, V, n, dpad, ut, pi, sA, [&](const f32x16(&acc)[4], int64_t c) {
    // the bounds are read here, per subtile: hoisted out of the item loop they would be 256
    // registers.  The compare only marks the band's members (bit 16 i + reg); their addresses
    // are formed in the loops below, from the bit, so that none of the 64 rows' list pointers
    // is kept in registers across the item loop
    asm volatile("" ::: "memory");
    unsigned inband[2] = {0u, 0u};  // 32-bit words: the bit constants stay literals
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int base = i * 32 + 8 * q + 4 * h;  // rows base .. base + 3: regs 4 q .. 4 q + 3
        const f32x4 hi = sHi[base >> 2], lo = sLo[base >> 2];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float a = acc[i][4 * q + j];
          const bool up = a > hi[j];
          cnt[i][4 * q + j] += up ? 1 : 0;
          // never for a row past the end (lo = +inf)
          if (!up && a >= lo[j]) inband[i >> 1] |= 1u << (16 * (i & 1) + 4 * q + j);
        }
      }
#pragma unroll
    for (int w = 0; w < 2; ++w)
      while (inband[w]) {  // rare: the items within eps of a row's threshold
        const int bit = __ffs((int)inband[w]) - 1 + 32 * w;
        inband[w] &= inband[w] - 1;
        const int64_t row = ut * 128 + (bit >> 4) * 32 + (bit & 3) + 8 * ((bit >> 2) & 3) + 4 * h;
        const int pos = atomicAdd(band_cnt + row, 1);
        if (pos < cap) band[row * cap + pos] = (int)c;
      }
  });
  fold_tile_rows(cnt, reinterpret_cast<int*>(sA), B, ut, pi, part);
}

// The loop's scores themselves, stored: what the count pass compares (for the bound's test;
// one block per CU: the 64 output addresses want registers, and nothing times this kernel).
__global__ __launch_bounds__(256, 1) void cos_scores_kernel(
    const float* __restrict__ U, int64_t B, const float* __restrict__ V, int64_t n, int dpad,
    int64_t n_ut, float* __restrict__ out, int64_t ldo) {
  __shared__ f32x4 sA[128 * 32];
  const int h = (threadIdx.x & 63) >> 5;
  const int64_t ut = (int64_t)blockIdx.x % n_ut, pi = (int64_t)blockIdx.x / n_ut;
  cos_tile_loop(U, B, V, n, dpad, ut, pi, sA, [&](const f32x16(&acc)[4], int64_t c) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int64_t row = ut * 128 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
        if (row < B) out[row * ldo + c] = acc[i][r];
      }
  });
}

// ---------------------------------------------------------------- resolve ----
template <int LPR>
__global__ __launch_bounds__(256) void rank_resolve_kernel(
    const int64_t* __restrict__ users, const int64_t* __restrict__ items,
    const float* __restrict__ thr, const int* __restrict__ ahead,
    const int* __restrict__ band_cnt, const int* __restrict__ band, int cap, int64_t P,
    const float* __restrict__ Hu, int64_t ldu, int64_t n_users, const float* __restrict__ Hi,
    int64_t ldi, int64_t n_items, int d, const int64_t* __restrict__ ex_ptr,
    const int32_t* __restrict__ ex_idx, int64_t* __restrict__ rank) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t b = (int64_t)blockIdx.x * 4 + wave;
  if (b >= P) return;  // wave-uniform, as every exit below
  const int64_t u = users[b], g = items[b];
  if (u < 0 || u >= n_users || g < 0 || g >= n_items) return;
  const int bc = band_cnt[b];
  if (bc < 0 || bc > cap) {  // the caller redoes the row exhaustively
    if (lane == 0) rank[b] = -1;
    return;
  }
  const float t = thr[b];
  constexpr int NPW = kWave / LPR;
  const int grp = lane / LPR, gl = lane % LPR;
  const float* pu = Hu + u * ldu;
  // every lane of the wave calls cos_pair_vec4 (its DPP sums read their neighbours); the
  // value and the counts live in each group's last lane
  int delta = 0;
  for (int i0 = 0; i0 < bc; i0 += NPW) {  // wave-uniform bound
    const int i = i0 + grp;
    const int64_t c = i < bc ? band[b * cap + i] : -1;
    const bool ok = c >= 0 && c < n_items && c != g;
    const float r = cos_pair_vec4<LPR>(pu, Hi + (ok ? c : 0) * ldi, d, gl, ok);
    if (gl == LPR - 1 && ok && (r > t || (r == t && c < g))) ++delta;
  }
  bool excluded = false;
  if (ex_ptr) {
    const int64_t e0 = ex_ptr[u], e1 = ex_ptr[u + 1];
    for (int64_t base = e0; base < e1; base += NPW) {  // wave-uniform bound
      const int64_t e = base + grp;
      const int64_t c = e < e1 ? ex_idx[e] : -1;  // -1: a duplicate the caller struck
      excluded |= c == g;
      const bool ok = c >= 0 && c < n_items && c != g;
      const float r = cos_pair_vec4<LPR>(pu, Hi + (ok ? c : 0) * ldi, d, gl, ok);
      if (gl == LPR - 1 && ok && (r > t || (r == t && c < g))) --delta;
    }
  }
#pragma unroll
  for (int off = 1; off < kWave; off <<= 1) delta += __shfl_xor(delta, off);
  const bool any_excluded = __ballot(excluded) != 0;
  if (lane == 0) rank[b] = any_excluded ? 0 : 1 + (int64_t)ahead[b] + delta;
}

int check_tables(const char* fn, const float* U, int64_t B, const float* V, int64_t n,
                 int64_t dpad) {
  GNNREC_REQUIRE(B >= 0 && n >= 0, "%s: negative size", fn);
  GNNREC_REQUIRE(dpad >= 8 && dpad % 8 == 0 && dpad <= kZMaxD,
                 "%s: dpad must be a multiple of 8 in [8, %d] (got %lld)", fn, kZMaxD,
                 (long long)dpad);
  GNNREC_REQUIRE(n < (int64_t(1) << 31), "%s: item ids must fit int32", fn);
  if (B == 0 || n == 0) return GNNREC_OK;
  GNNREC_REQUIRE(U && V && aligned16(U) && aligned16(V), "%s: null or unaligned table", fn);
  GNNREC_REQUIRE(((n + kZItems - 1) / kZItems) * ((B + 127) / 128) < (int64_t(1) << 31),
                 "%s: too many tiles for one launch", fn);
  return GNNREC_OK;
}

}  // namespace
}  // namespace gnnrec

extern "C" double gnnrec_rank_eps(int64_t d) {
  return d < 1 ? 0.0 : gnnrec::rank_eps((d + 7) / 8 * 8);
}

extern "C" int gnnrec_cos_scores_f32(const float* users, int64_t n_users, const float* items,
                                     int64_t n_items, int64_t dpad, float* out, int64_t ldo,
                                     void* stream) {
  using namespace gnnrec;
  const char* fn = "gnnrec_cos_scores_f32";
  const int rc = check_tables(fn, users, n_users, items, n_items, dpad);
  if (rc != GNNREC_OK || n_users == 0 || n_items == 0) return rc;
  GNNREC_REQUIRE(out && ldo >= n_items, "%s: bad out / ldo", fn);
  const int64_t n_part = (n_items + kZItems - 1) / kZItems, n_ut = (n_users + 127) / 128;
  hipLaunchKernelGGL(cos_scores_kernel, dim3((unsigned)(n_part * n_ut)), dim3(256), 0,
                     as_stream(stream), users, n_users, items, n_items, (int)dpad, n_ut, out, ldo);
  return check_launch(fn);
}

extern "C" int gnnrec_rank_count_f32(const float* users, int64_t n_rows, const float* items,
                                     int64_t n_items, int64_t dpad, const float* thr,
                                     int32_t* parts, int32_t* ahead, int32_t* band_counts,
                                     int32_t* band_items, int64_t cap, void* stream) {
  using namespace gnnrec;
  const char* fn = "gnnrec_rank_count_f32";
  const int rc = check_tables(fn, users, n_rows, items, n_items, dpad);
  if (rc != GNNREC_OK) return rc;
  GNNREC_REQUIRE(cap >= 1 && cap <= kRankCandMax, "%s: cap must be in [1, %d] (got %lld)", fn,
                 kRankCandMax, (long long)cap);
  if (n_rows == 0) return GNNREC_OK;
  GNNREC_REQUIRE(ahead, "%s: null ahead", fn);
  GNNREC_REQUIRE((n_rows + 255) / 256 < (int64_t(1) << 31), "%s: too many rows", fn);
  const int64_t n_part = (n_items + kZItems - 1) / kZItems, n_ut = (n_rows + 127) / 128;
  if (n_items > 0) {
    GNNREC_REQUIRE(thr && parts && band_counts && band_items, "%s: null pointer", fn);
    const double eps = rank_eps(dpad) * (1.0 + 0x1p-30);
    hipLaunchKernelGGL(rank_count_kernel, dim3((unsigned)(n_part * n_ut)), dim3(256), 0,
                       as_stream(stream), users, n_rows, items, n_items, (int)dpad, n_ut, thr, eps,
                       parts, band_counts, band_items, (int)cap);
    const int rc2 = check_launch(fn);
    if (rc2 != GNNREC_OK) return rc2;
  }
  return launch_fold_partials_i32(fn, parts, n_part, n_rows, ahead, as_stream(stream));
}

extern "C" int gnnrec_rank_resolve_f32(const int64_t* users, const int64_t* items,
                                       const float* thr, const int32_t* ahead,
                                       const int32_t* band_counts, const int32_t* band_items,
                                       int64_t cap, int64_t n_pairs, const float* h_user,
                                       int64_t ldu, int64_t n_users, const float* h_item,
                                       int64_t ldi, int64_t n_items, int64_t d,
                                       const int64_t* exclude_indptr,
                                       const int32_t* exclude_indices, int64_t* rank,
                                       void* stream) {
  using namespace gnnrec;
  const char* fn = "gnnrec_rank_resolve_f32";
  GNNREC_REQUIRE(n_pairs >= 0 && (n_pairs + 3) / 4 < (int64_t(1) << 31) && n_users >= 0 &&
                     n_items >= 0 && n_items < (int64_t(1) << 31),
                 "%s: bad size", fn);
  GNNREC_REQUIRE(cap >= 1 && cap <= kRankCandMax, "%s: cap must be in [1, %d] (got %lld)", fn,
                 kRankCandMax, (long long)cap);
  GNNREC_REQUIRE(d >= 4 && d % 4 == 0 && ldu % 4 == 0 && ldi % 4 == 0 && ldu >= d && ldi >= d,
                 "%s: needs d %% 4 == 0 and row strides that are multiples of 4 and >= d", fn);
  GNNREC_REQUIRE(!exclude_indptr == !exclude_indices,
                 "%s: exclusion indptr and indices come together", fn);
  if (n_pairs == 0) return GNNREC_OK;
  GNNREC_REQUIRE(users && items && thr && ahead && band_counts && band_items && rank,
                 "%s: null pointer", fn);
  GNNREC_REQUIRE(h_user && h_item && aligned16(h_user) && aligned16(h_item),
                 "%s: tables must be non-null and 16-byte aligned", fn);
  hipStream_t s = as_stream(stream);
  const dim3 grid((unsigned)((n_pairs + 3) / 4)), block(256);
#define GNNREC_LAUNCH_RESOLVE(LPR)                                                               \
  hipLaunchKernelGGL((rank_resolve_kernel<LPR>), grid, block, 0, s, users, items, thr, ahead,    \
                     band_counts, band_items, (int)cap, n_pairs, h_user, ldu, n_users, h_item,   \
                     ldi, n_items, (int)d, exclude_indptr, exclude_indices, rank)
  if (d <= 64) GNNREC_LAUNCH_RESOLVE(16);  // the lane groups of gnnrec_sddmm_cos_f32
  else if (d <= 128) GNNREC_LAUNCH_RESOLVE(32);
  else GNNREC_LAUNCH_RESOLVE(64);
#undef GNNREC_LAUNCH_RESOLVE
  return check_launch(fn);
}
