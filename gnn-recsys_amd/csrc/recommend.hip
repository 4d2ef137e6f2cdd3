// f1b — exact top-k recommendations without a score matrix: a bf16 MFMA prefilter, then the
// library's own fp32 cosine on the few pairs it cannot rule out.
//
// score(u, v) is, by definition, the value gnnrec_sddmm_cos_f32 returns for the pair from the
// raw fp32 tables (CosinePrediction's arithmetic, rows divided by max(|.|, 1e-12)), and the
// ranking is (score desc, item id asc) with the user's excluded items removed — what
// gnnrec_topk_rows_f32 gives over a full score row.  The kernels:
//
//   normalize_rows_bf16   û = x / max(|x|, 1e-12) in fp32, rounded to bf16 (nearest even),
//                         rows padded with zeros to a multiple of 32 columns
//   score_bf16            a(u, v) = sum_c bf16(û_c) bf16(v̂_c), fp32 accumulation on
//                         v_mfma_f32_32x32x16_bf16; one main loop, two epilogues:
//                           store   a as fp32 [B, m] (the sample that sets the thresholds)
//                           filter  append item v to row u's candidate list where
//                                   a >= tau_u - 2 eps
//   mask_excluded         the sample's excluded columns to -inf, so that a plain top-k of
//                         the sample gives tau (the k-th best non-excluded score there)
//   topk_candidates       drop a row's excluded candidates, rescore the rest with the fp32
//                         cosine (cos_score.hpp: the bits of gnnrec_sddmm_cos_f32), rank
//   topk_scored_candidates  the same strike and ranking of (item, score) pairs that need no
//                         rescoring: the MLP head's, whose filter (heads.hip) compares and
//                         keeps the final fp32 score
//   topk_update           f1e: a cached list merged, in place, with the dirty items the filter
//                         kept after a refresh, where the result is provably the exact list
//                         (one wave per row)
//
// THE BOUND.  bf16 has unit roundoff 2^-8: |bf16(û) - û| <= 2^-8 |û| as vectors, and the same
// for v̂.  With |û| = |v̂| = 1 (up to fp32 rounding) Cauchy-Schwarz gives
//   |bf16(û).bf16(v̂) - û.v̂| <= |bf16(û) - û| |bf16(v̂)| + |û| |bf16(v̂) - v̂|
//                             <= 2^-8 (1 + 2^-8) + 2^-8.
// fp32 accumulation of d products of magnitude <= 1 and the fp32 rounding of the
// normalisation add at most about d 2^-23, and score itself carries the same order of fp32
// error against the real cosine: for d <= 2048 all of it is below 2^-11 - 2^-16, so
//   |a(u, v) - score(u, v)| <= eps = 2^-7 + 2^-11.
// The derivation assumes row norms (and the squares they are summed from) in fp32's normal
// range and away from the 1e-12 guard, or exactly zero: where the squares underflow, or the
// guard applies to one computed norm and not to the other, a and score divide by different
// norms and the derivation says nothing.
//
// THE FILTER.  Let tau_r be ANY value such that at least k non-excluded items of row r have
// a >= tau_r.  Those k items have score >= tau_r - eps, so the true k-th best score is
// >= tau_r - eps, and every item of the true top k has a >= tau_r - 2 eps.  Items below
// that are discarded; a looser tau_r only admits more candidates, never loses one.  (Ties in
// score at the k-th place are covered too: a tied item's score is >= tau_r - eps as well.)
//
// THE RATING BAND (f1d, popularity: rating.hpp, recommend_pop.hip).  With
// popularity the ranking is by R(u, v) = expf(score) / Z_u + p_v, and the scorer's rating
// epilogues form Ra = rating(a, Z_u, p_v) from the approximate score.  In real numbers, with
// |a - score| <= eps and score <= 1 (up to fp32 rounding, covered by the e^eps),
//   |e^a - e^score| <= e^(1 + eps) (e^eps - 1),
// the two sides share Z_u and p_v, and each side's three fp32 operations add at most
// 2^-22 (expf, within 2 ulp) + 2^-24 (divide) relative to its quotient <= e^(1 + eps) / Z_u
// and 2^-24 (add) relative to the sum <= e^(1 + eps) / Z_u + max p: together, both sides,
// below 2^-20 e^(1 + eps) / Z_u + 2^-22 max p.  So
//   |Ra - R| <= delta_u = e^(1 + eps) ((e^eps - 1) + 2^-20) / Z_u + 2^-22 max p,
// and THE FILTER's argument carries over with R, Ra, delta_u for score, a, eps: for any tau_u
// with k eligible items at Ra >= tau_u, every member of the true top k (ties at the k-th
// place too) has Ra >= tau_u - 2 delta_u.  gnnrec_rating_thresholds_f32 forms
// tau_u - 2 delta_u in double, once per batch, rounded down; the epilogue compares with it
// as it is.
#include "common.hpp"
#include "cos_score.hpp"
#include "rating.hpp"
#include <algorithm>
#include <cmath>

namespace gnnrec {
namespace {

constexpr float kRecEps = 0.0078125f + 0.00048828125f;  // 2^-7 + 2^-11, derived above
constexpr int kRecMaxD = 2048;                           // the bound's range of d
constexpr int kCandMax = 4096;                           // candidate slots per row, at most
constexpr int kExChunk = 2048;                           // exclusion ids staged per round

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));  // 16 B in flight

// fp32 -> bf16 bits, round to nearest even (finite inputs; non-finite is outside the contract)
__device__ __forceinline__ uint32_t bf16_rne(float x) {
  const uint32_t u = __builtin_bit_cast(uint32_t, x);
  return (u + 0x7FFFu + ((u >> 16) & 1u)) >> 16;
}

// ------------------------------------------------------------ normalise ----
// One wave per row: sum of squares (16-B loads when the rows allow), xor-tree reduce, then
// x / max(|x|, 1e-12) rounded to bf16; the second read of the row comes from L1.
__global__ __launch_bounds__(256) void normalize_rows_bf16_kernel(
    const float* __restrict__ X, int64_t ld, int64_t n, int d, const int64_t* __restrict__ map,
    uint16_t* __restrict__ out, int dpad, bool vec) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= n) return;  // wave-uniform
  const float* src = X + (map ? map[row] : row) * ld;
  uint16_t* dst = out + row * dpad;
  float ss = 0.f;
  if (vec) {
    for (int c = lane * 4; c < d; c += kWave * 4) {
      const float4 v = *reinterpret_cast<const float4*>(src + c);
      ss += v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w;
    }
  } else {
    for (int c = lane; c < d; c += kWave) ss += src[c] * src[c];
  }
#pragma unroll
  for (int off = 1; off < kWave; off <<= 1) ss += __shfl_xor(ss, off);
  const float nrm = fmaxf(sqrtf(ss), 1e-12f);
  if (vec) {  // d % 4 == 0: a group of four columns is all data or all pad
    for (int c = lane * 4; c < dpad; c += kWave * 4) {
      uint2 o = make_uint2(0u, 0u);
      if (c < d) {
        const float4 v = *reinterpret_cast<const float4*>(src + c);
        o.x = bf16_rne(v.x / nrm) | (bf16_rne(v.y / nrm) << 16);
        o.y = bf16_rne(v.z / nrm) | (bf16_rne(v.w / nrm) << 16);
      }
      *reinterpret_cast<uint2*>(dst + c) = o;
    }
  } else {
    for (int c = lane; c < dpad; c += kWave)
      dst[c] = c < d ? (uint16_t)bf16_rne(src[c] / nrm) : (uint16_t)0;
  }
}

// ---------------------------------------------------------------- score ----
// A 256-thread block scores a 128 x 128 (users x items) tile, each of its four waves a
// 64 x 64 quarter as 2 x 2 MFMA tiles of 32 x 32 (64 accumulator registers per lane).  Both
// tables are row-major with K contiguous, which is the operand layout of
// v_mfma_f32_32x32x16_bf16 for A and for B alike: lane l holds row (l & 31), k = 8 (l >> 5)
// .. + 7 of a k-step, one 16-B load straight from the table.  No LDS, no transpose; the user
// batch is served by L2 (consecutive blocks walk the user tiles of one item slab).
// Rows and items past the end read a clamped (valid) row and are masked in the epilogue:
// they are never scored as zeros, which a negative threshold would pass.
// C layout: col = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5).

// A wave's 64 x 64 accumulators (rows r0.., columns c0..) to their destination, rows >= B
// and columns >= n masked here, at the compare or the store.  The filter's 32 row thresholds
// (tau - 2 eps, +inf for rows past the end) are fetched as one batch before the compares — a
// load per row in front of its compare serialises 32 memory latencies per tile — from
// thr_lds (the wave's 64 thresholds, staged with the user tile: four rows per 16-B read)
// when given, else from tau.
//
// RATING (f1d): the value stored or compared is Ra = rating(a, Z_row, p_col)
// (rating.hpp) instead of a.  Z (per batch row, from z_lds — staged like the thresholds — or
// the array) and pcol (per column of the table) come with it, and tau then holds the
// finished per-row thresholds tau_u - 2 delta_u (gnnrec_rating_thresholds_f32), formed once
// per batch, compared as they are.
template <bool FILTER, bool RATING>
__device__ __forceinline__ void score_epilogue(const f32x16 (&acc)[2][2], int64_t r0, int64_t c0,
                                               int l31, int h, int64_t B, int64_t n,
                                               float* __restrict__ out, int64_t ldo,
                                               const float* __restrict__ tau,
                                               const float* thr_lds, int* __restrict__ counts,
                                               int* __restrict__ cand, int cap,
                                               const float* __restrict__ Z, const float* z_lds,
                                               const float* __restrict__ pcol) {
  float pj[2] = {0.f, 0.f};
  if constexpr (RATING) {
#pragma unroll
    for (int j = 0; j < 2; ++j)
      if (c0 + j * 32 + l31 < n) pj[j] = pcol[c0 + j * 32 + l31];
  }
  // RATING: the Z of rows i 32 + 8 g + 4 h + (0..3), fetched per 32-row half (all 32 at once
  // leave the dpad = 128 tile no registers)
  auto fetch_z = [&](int i, f32x4 (&zr)[4]) {
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      if (z_lds) {
        zr[g] = *reinterpret_cast<const f32x4*>(z_lds + i * 32 + 8 * g + 4 * h);
      } else {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int64_t row = r0 + i * 32 + 8 * g + 4 * h + q;
          zr[g][q] = row < B ? Z[row] : 1.f;
        }
      }
    }
  };
  auto value = [&](const f32x4 (&zr)[4], int i, int j, int reg) -> float {
    if constexpr (RATING) return rating(acc[i][j][reg], zr[reg >> 2][reg & 3], pj[j]);
    else return acc[i][j][reg];
  };
  if constexpr (FILTER) {
    f32x4 thr[2][4];  // [i][g]: rows i 32 + 8 g + 4 h + (0..3), the registers 4 g .. 4 g + 3
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        if (thr_lds) {
          thr[i][g] = *reinterpret_cast<const f32x4*>(thr_lds + i * 32 + 8 * g + 4 * h);
        } else {
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const int64_t row = r0 + i * 32 + 8 * g + 4 * h + q;
            if constexpr (RATING) thr[i][g][q] = row < B ? tau[row] : INFINITY;
            else thr[i][g][q] = row < B ? tau[row] - 2.f * kRecEps : INFINITY;
          }
        }
      }
    const bool colok[2] = {c0 + l31 < n, c0 + 32 + l31 < n};
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      f32x4 zr[4];
      if constexpr (RATING) fetch_z(i, zr);
#pragma unroll
      for (int reg = 0; reg < 16; ++reg)
#pragma unroll
        for (int j = 0; j < 2; ++j)
          if (colok[j] && value(zr, i, j, reg) >= thr[i][reg >> 2][reg & 3]) {
            // the counter keeps counting past cap (the overflow signal); a store happens
            // only inside the row's cap slots
            const int64_t row = r0 + i * 32 + (reg & 3) + 8 * (reg >> 2) + 4 * h;
            const int slot = atomicAdd(counts + row, 1);
            if (slot >= 0 && slot < cap) cand[row * cap + slot] = (int)(c0 + j * 32 + l31);
          }
    }
  } else {
    // addresses split into a wave-uniform part (scalar registers) and one lane offset, so
    // that the 32 rows' address arithmetic does not sit in vector registers
    const int64_t lane_out = (int64_t)(4 * h) * ldo + l31;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      f32x4 zr[4];
      if constexpr (RATING) fetch_z(i, zr);
#pragma unroll
      for (int reg = 0; reg < 16; ++reg) {
        const int64_t urow = r0 + i * 32 + (reg & 3) + 8 * (reg >> 2);  // uniform
        if (urow + 4 * h >= B) continue;
#pragma unroll
        for (int j = 0; j < 2; ++j)
          if (c0 + j * 32 + l31 < n)
            (out + urow * ldo + c0 + j * 32)[lane_out] = value(zr, i, j, reg);
      }
    }
  }
}

template <bool FILTER, bool RATING>
__global__ __launch_bounds__(256) void score_bf16_kernel(
    const uint16_t* __restrict__ U, int64_t B, const uint16_t* __restrict__ V, int64_t n,
    int dpad, int64_t n_utiles, float* __restrict__ out, int64_t ldo,
    const float* __restrict__ tau, int* __restrict__ counts, int* __restrict__ cand, int cap,
    const float* __restrict__ Z, const float* __restrict__ pcol) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int l31 = lane & 31, h = lane >> 5;
  const int64_t tile = blockIdx.x;
  const int64_t r0 = (tile % n_utiles) * 128 + (wave >> 1) * 64;
  const int64_t c0 = (tile / n_utiles) * 128 + (wave & 1) * 64;
  if (r0 >= B || c0 >= n) return;  // wave-uniform; the kernel has no barrier
  const uint16_t* pa[2];
  const uint16_t* pb[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int64_t r = min(r0 + i * 32 + l31, B - 1);
    const int64_t c = min(c0 + i * 32 + l31, n - 1);
    pa[i] = U + r * dpad + 8 * h;
    pb[i] = V + c * dpad + 8 * h;
  }
  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
  for (int k0 = 0; k0 < dpad; k0 += 32) {  // dpad % 32 == 0: two k-steps, 8 loads in flight
    bf16x8 a[2][2], b[2][2];
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        a[s][i] = *reinterpret_cast<const bf16x8*>(pa[i] + k0 + 16 * s);
        b[s][i] = *reinterpret_cast<const bf16x8*>(pb[i] + k0 + 16 * s);
      }
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[s][i], b[s][j], acc[i][j], 0, 0, 0);
  }
  score_epilogue<FILTER, RATING>(acc, r0, c0, l31, h, B, n, out, ldo, tau, nullptr, counts, cand,
                                 cap, Z, nullptr, pcol);
}

// The same tile for dpad = 32, 64 and 128 (d <= 64 and 97..128; at 96 the registers of two
// resident blocks do not hold the slab and a tile in flight without scratch), arranged so that every byte comes through a coalesced load:
// a block owns a slab of 128 items for its whole life — each wave's 64 item rows, all of K,
// stay in registers as B fragments (dpad / 16 x 2 fragments of 4 VGPRs, 64 at dpad = 128) —
// and walks the batch's user tiles (every gridDim.y-th one).  A user tile (128 rows x dpad)
// is staged into LDS with 16-B loads that cover whole rows (issued one tile ahead, into
// registers, so that their latency runs under the MFMAs), and read back in the MFMA
// layout (lane l: row l & 31, 16 B at k = 8 (l >> 5)); rows are padded by 16 B so that the
// 16 lanes of a ds_read_b128 phase fall in distinct bank groups (row stride 272 B = 68
// banks at dpad = 128).  Direct operand loads touch 32 rows per instruction for 32 B each;
// this form moves the same bytes as full lines.
template <int DPAD>
__device__ __forceinline__ void fetch_user_tile(u32x4 (&pf)[DPAD / 16], const uint16_t* U,
                                                int64_t B, int64_t ut, int tid) {
  constexpr int CH = DPAD / 8;
#pragma unroll
  for (int p = 0; p < DPAD / 16; ++p) {
    const int idx = tid + p * 256;
    const int64_t r = min(ut * 128 + idx / CH, B - 1);  // past the end: a valid row, masked later
    pf[p] = *reinterpret_cast<const u32x4*>(U + r * DPAD + (idx % CH) * 8);
  }
}

template <int DPAD, bool FILTER, bool RATING>
__global__ __launch_bounds__(256, 2) void score_bf16_slab_kernel(
    const uint16_t* __restrict__ U, int64_t B, const uint16_t* __restrict__ V, int64_t n,
    float* __restrict__ out, int64_t ldo, const float* __restrict__ tau,
    int* __restrict__ counts, int* __restrict__ cand, int cap, const float* __restrict__ Z,
    const float* __restrict__ pcol) {
  constexpr int KS = DPAD / 16;        // k-steps
  constexpr int CH = DPAD / 8;         // 16-B chunks per row
  constexpr int ROWB = DPAD * 2 + 16;  // LDS bytes per staged row
  __shared__ __attribute__((aligned(16))) unsigned char sA[128 * ROWB];
  __shared__ __attribute__((aligned(16))) float sThr[128];  // the tile's tau - 2 eps (filter)
  __shared__ __attribute__((aligned(16))) float sZ[RATING ? 128 : 4];  // the tile's Z (rating)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l31 = lane & 31, h = lane >> 5;
  const int wr = wave >> 1, wc = wave & 1;
  const int64_t c0 = (int64_t)blockIdx.x * 128 + wc * 64;
  const bool has_items = c0 < n;  // wave-uniform; a wave without items still joins the barriers
  bf16x8 bfr[2][KS];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int64_t c = min(c0 + j * 32 + l31, n - 1);
#pragma unroll
    for (int ks = 0; ks < KS; ++ks)
      bfr[j][ks] = *reinterpret_cast<const bf16x8*>(V + c * DPAD + ks * 16 + 8 * h);
  }
  const int64_t n_ut = (B + 127) / 128;
  // the next user tile travels from L2 into registers while this one is multiplied
  constexpr int PF = 128 * CH / 256;  // 16-B chunks per thread per tile
  static_assert(128 * CH % 256 == 0, "a tile is a whole number of block-wide loads");
  u32x4 pf[PF];
  // (the filter pass only: the store pass scores the short sample, and its epilogue's
  // addresses leave no room for the tile in flight at two blocks per CU)
  // (nor the rating filter, whose epilogue holds Z and p beside the thresholds)
  constexpr bool kAhead = FILTER && !RATING;
  float tpf = INFINITY;  // thread t < 128: row t's threshold, +inf past the end (never passed)
  float zpf = 1.f;       // and, for the ratings, row t's Z
  auto fetch_thr = [&](int64_t ut) {
    const int64_t r = ut * 128 + tid;
    if constexpr (FILTER && !RATING) {
      if (tid < 128) tpf = r < B ? tau[r] - 2.f * kRecEps : INFINITY;
    } else if (tid < 128) {
      if constexpr (FILTER) tpf = r < B ? tau[r] : INFINITY;
      zpf = r < B ? Z[r] : 1.f;
    }
  };
  if (kAhead && (int64_t)blockIdx.y < n_ut) {
    fetch_user_tile<DPAD>(pf, U, B, blockIdx.y, tid);
    fetch_thr(blockIdx.y);
  }
  for (int64_t ut = blockIdx.y; ut < n_ut; ut += gridDim.y) {  // block-uniform trip count
    __syncthreads();  // the previous tile's reads are done
    if constexpr (!kAhead) {
      fetch_user_tile<DPAD>(pf, U, B, ut, tid);
      if constexpr (RATING) fetch_thr(ut);
    }
#pragma unroll
    for (int p = 0; p < PF; ++p) {
      const int idx = tid + p * 256;
      *reinterpret_cast<u32x4*>(sA + (idx / CH) * ROWB + (idx % CH) * 16) = pf[p];
    }
    if (FILTER && tid < 128) sThr[tid] = tpf;
    if (RATING && tid < 128) sZ[tid] = zpf;
    __syncthreads();
    if (kAhead && ut + gridDim.y < n_ut) {
      fetch_user_tile<DPAD>(pf, U, B, ut + gridDim.y, tid);
      fetch_thr(ut + gridDim.y);
    }
    const int64_t r0 = ut * 128 + wr * 64;
    if (!has_items || r0 >= B) continue;
    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      bf16x8 a[2];
#pragma unroll
      for (int i = 0; i < 2; ++i)
        a[i] = *reinterpret_cast<const bf16x8*>(sA + (wr * 64 + i * 32 + l31) * ROWB + ks * 32 +
                                                h * 16);
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[i], bfr[j][ks], acc[i][j], 0, 0, 0);
    }
    score_epilogue<FILTER, RATING>(acc, r0, c0, l31, h, B, n, out, ldo, tau,
                                   FILTER ? sThr + wr * 64 : nullptr, counts, cand, cap, Z,
                                   RATING ? sZ + wr * 64 : nullptr, pcol);
  }
}

template <bool FILTER, bool RATING = false>
void launch_score(const uint16_t* U, int64_t B, const uint16_t* V, int64_t n, int dpad, float* out,
                  int64_t ldo, const float* tau, int* counts, int* cand, int cap, hipStream_t s,
                  const float* Z = nullptr, const float* pcol = nullptr) {
  const int64_t nu = (B + 127) / 128, ni = (n + 127) / 128;
  if (dpad != 32 && dpad != 64 && dpad != 128) {
    hipLaunchKernelGGL((score_bf16_kernel<FILTER, RATING>), dim3((unsigned)(nu * ni)), dim3(256),
                       0, s, U, B, V, n, dpad, nu, out, ldo, tau, counts, cand, cap, Z, pcol);
    return;
  }
  // enough blocks to fill the chip when the item range is short (the sample pass, small tables)
  const int64_t gy = std::min<int64_t>(nu, std::max<int64_t>(1, (2048 + ni - 1) / ni));
  const dim3 grid((unsigned)ni, (unsigned)gy), block(256);
#define GNNREC_LAUNCH_SLAB(D)                                                                    \
  hipLaunchKernelGGL((score_bf16_slab_kernel<D, FILTER, RATING>), grid, block, 0, s, U, B, V, n, \
                     out, ldo, tau, counts, cand, cap, Z, pcol)
  if (dpad == 32) GNNREC_LAUNCH_SLAB(32);
  else if (dpad == 64) GNNREC_LAUNCH_SLAB(64);
  else GNNREC_LAUNCH_SLAB(128);
#undef GNNREC_LAUNCH_SLAB
}

// ------------------------------------------------------------ mask ----
// One wave per score row: the columns of the row's user's exclusion list become -inf, so a
// plain top-k over the sample's scores yields tau (the k-th best NON-excluded score, -inf
// when fewer than k columns are eligible).  Ids outside [0, n_cols) are skipped.
__global__ __launch_bounds__(256) void mask_excluded_kernel(
    float* __restrict__ S, int64_t ld, int64_t n_rows, int64_t n_cols,
    const int64_t* __restrict__ user_rows, const int64_t* __restrict__ ex_ptr,
    const int32_t* __restrict__ ex_idx) {
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= n_rows) return;
  const int64_t u = user_rows ? user_rows[row] : row;
  const int64_t e1 = ex_ptr[u + 1];
  for (int64_t e = ex_ptr[u] + (threadIdx.x & 63); e < e1; e += kWave) {
    const int64_t c = ex_idx[e];
    if (c >= 0 && c < n_cols) S[row * ld + c] = -INFINITY;
  }
}

// ------------------------------------------------------------ candidates ----
__device__ __forceinline__ bool better(float a, int ia, float b, int ib) {
  return a > b || (a == b && ia < ib);
}

// The two steps every candidate ranking shares, on a block's LDS lists (ids[n], sc[n]):
//
// strike_excluded: the ids found in user row urow's exclusion list become -1 (the list
// staged kExChunk ids at a time into ex; rows are unsorted and candidates few, so a scan).
// The caller's writes of ids are synchronised before the call; the strikes are after it.
__device__ __forceinline__ void strike_excluded(int* ids, int n, int* ex,
                                                const int64_t* __restrict__ ex_ptr,
                                                const int32_t* __restrict__ ex_idx, int64_t urow,
                                                int tid) {
  if (!ex_ptr) return;
  const int64_t e0 = ex_ptr[urow], ne = ex_ptr[urow + 1] - e0;
  for (int64_t base = 0; base < ne; base += kExChunk) {
    const int m = (int)min<int64_t>(kExChunk, ne - base);
    for (int j = tid; j < m; j += 256) ex[j] = ex_idx[e0 + base + j];
    __syncthreads();
    for (int i = tid; i < n; i += 256) {
      const int c = ids[i];
      if (c < 0) continue;
      for (int j = 0; j < m; ++j)
        if (ex[j] == c) { ids[i] = -1; break; }
    }
    __syncthreads();
  }
}

// rank_and_emit: each surviving candidate's rank is the number of better candidates (ids
// are distinct, so the order (score desc, id asc) is total and the ranks 0 .. n-1 are each
// taken once); ranks below k go to row b of out_v / out_i, the rest of the row is padded
// with (-inf, -1).  *n_valid is zero and ids / sc synchronised on entry.
__device__ __forceinline__ void rank_and_emit(const int* ids, const float* sc, int n, int k,
                                              int64_t b, float* __restrict__ out_v,
                                              int64_t* __restrict__ out_i, int* n_valid,
                                              int tid) {
  int mine = 0;
  for (int i = tid; i < n; i += 256) {
    const int c = ids[i];
    if (c < 0) continue;
    ++mine;
    const float v = sc[i];
    int rank = 0;
    for (int j = 0; j < n; ++j) {
      const int cj = ids[j];
      rank += (cj >= 0 && better(sc[j], cj, v, c)) ? 1 : 0;
    }
    if (rank < k) {
      out_v[b * k + rank] = v;
      out_i[b * k + rank] = c;
    }
  }
  if (mine) atomicAdd(n_valid, mine);
  __syncthreads();
  for (int r = *n_valid + tid; r < k; r += 256) {
    out_v[b * k + r] = -INFINITY;
    out_i[b * k + r] = -1;
  }
}

// One block per batch row: its min(count, cap) candidates into LDS, the excluded ones
// struck, the rest scored by lane groups exactly as sddmm_cos_kernel<LPR, 4> scores an edge,
// then ranked.
// RATING: the rescored cosine becomes R = rating(score, Z[b], p[item]) (rating.hpp) before the
// ranking, Z per batch row and p per item.
template <int LPR, bool RATING>
__global__ __launch_bounds__(256) void topk_candidates_kernel(
    const int* __restrict__ counts, const int* __restrict__ cand, int cap,
    const int64_t* __restrict__ user_rows, const float* __restrict__ Hu, int64_t ldu,
    const float* __restrict__ Hi, int64_t ldi, int d, const int64_t* __restrict__ ex_ptr,
    const int32_t* __restrict__ ex_idx, int k, float* __restrict__ out_v,
    int64_t* __restrict__ out_i, const float* __restrict__ Z, const float* __restrict__ p) {
  __shared__ int ids[kCandMax];
  __shared__ float sc[kCandMax];
  __shared__ int ex[kExChunk];
  __shared__ int n_valid;
  const int tid = threadIdx.x;
  const int64_t b = blockIdx.x;
  const int cnt = counts[b];
  if (cnt > cap || cnt < 0) return;  // overflowed: nothing is emitted, the caller recomputes
  const int n = cnt;
  const int64_t urow = user_rows ? user_rows[b] : b;
  for (int i = tid; i < n; i += 256) ids[i] = cand[b * cap + i];
  if (tid == 0) n_valid = 0;
  __syncthreads();
  strike_excluded(ids, n, ex, ex_ptr, ex_idx, urow, tid);
  constexpr int NPW = kWave / LPR;
  const int lane = tid & 63, wave = tid >> 6;
  const int grp = lane / LPR, gl = lane % LPR;
  const float* pu = Hu + urow * ldu;
  for (int i0 = wave * NPW; i0 < n; i0 += 4 * NPW) {  // wave-uniform bound
    const int i = i0 + grp;
    const int c = i < n ? ids[i] : -1;
    const bool ok = c >= 0;
    float r = cos_pair_vec4<LPR>(pu, Hi + (int64_t)(ok ? c : 0) * ldi, d, gl, ok);
    if constexpr (RATING) r = rating(r, Z[b], p[ok ? c : 0]);
    if (gl == LPR - 1 && i < n) sc[i] = ok ? r : -INFINITY;
  }
  __syncthreads();
  rank_and_emit(ids, sc, n, k, b, out_v, out_i, &n_valid, tid);
}

// The same ranking of candidates that come with their scores (the dense MLP filter's
// (item, score) pairs, heads.hip): nothing is rescored.
__global__ __launch_bounds__(256) void topk_scored_candidates_kernel(
    const int* __restrict__ counts, const int* __restrict__ cand,
    const float* __restrict__ cand_sc, int cap, const int64_t* __restrict__ user_rows,
    const int64_t* __restrict__ ex_ptr, const int32_t* __restrict__ ex_idx, int k,
    float* __restrict__ out_v, int64_t* __restrict__ out_i) {
  __shared__ int ids[kCandMax];
  __shared__ float sc[kCandMax];
  __shared__ int ex[kExChunk];
  __shared__ int n_valid;
  const int tid = threadIdx.x;
  const int64_t b = blockIdx.x;
  const int cnt = counts[b];
  if (cnt > cap || cnt < 0) return;  // overflowed: nothing is emitted, the caller recomputes
  const int n = cnt;
  const int64_t urow = user_rows ? user_rows[b] : b;
  for (int i = tid; i < n; i += 256) {
    ids[i] = cand[b * cap + i];
    sc[i] = cand_sc[b * cap + i];
  }
  if (tid == 0) n_valid = 0;
  __syncthreads();
  strike_excluded(ids, n, ex, ex_ptr, ex_idx, urow, tid);
  rank_and_emit(ids, sc, n, k, b, out_v, out_i, &n_valid, tid);
}

// ---------------------------------------------------------------- update ----
// f1e: a clean user's cached top-k list brought up to date after a refresh
// that rewrote the item rows marked in item_mark, in place.  One WAVE per row, four rows per
// block: a row holds its k entries and the handful of dirty items the filter kept
// (tau = the list's last score), and the kernel runs for every clean user, most of whom
// leave after reading k marks and one count.  The block-wide strike_excluded /
// rank_and_emit above spend 256 threads and their barriers on a row; their wave forms are
// kept apart here because sharing them would make those kernels branch on the caller
// (barrier or none, strided by 256 or by 64, emit or decide first); better() and
// cos_pair_vec4 are shared.  Rows are wave-private: no __syncthreads anywhere.
//
// Per row u = rows[b], with kappa = (score, id) of the list's last real entry:
//   the list's clean entries keep their cached scores, its dirty entries are dropped;
//   the candidates (columns of the dirty-item list) become item ids, the ones in u's
//   exclusion row are struck, the rest rescored with the fp32 cosine;
//   SETTLED when the old list was padded (no clean eligible item lies outside it, and
//   tau = -inf kept every dirty item), or when k entries remain and the k-th is not worse
//   than kappa (everything outside the merged set ranks after kappa): the k best are
//   written; otherwise redo[u] = 1 and the row stays as it was.
// NaN scores, cached or rescored, are outside the contract, as for recommend(): better() is
// not a total order with them, and two entries could then claim one rank (never an address
// outside the row).
constexpr int kUpdSlots = 256;  // LDS list slots per wave: k kept entries + cap candidates
constexpr int kUpdMaxK = 64;    // one lane per cached entry

// the wave's LDS writes before, its reads after: the hardware keeps one wave's LDS
// operations in order, this keeps the compiler from moving them across
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

template <int LPR>
__global__ __launch_bounds__(256) void topk_update_kernel(
    const int64_t* __restrict__ rows, int64_t B, int64_t* __restrict__ idx,
    float* __restrict__ vals, int64_t n_users, int k, const int* __restrict__ item_mark,
    int64_t n_items, const int* __restrict__ counts, const int* __restrict__ cand, int cap,
    const int* __restrict__ dirty_ids, int64_t nd, const float* __restrict__ Hu, int64_t ldu,
    const float* __restrict__ Hi, int64_t ldi, int d, const int64_t* __restrict__ ex_ptr,
    const int32_t* __restrict__ ex_idx, int* __restrict__ redo) {
  __shared__ int s_ids[4][kUpdSlots];
  __shared__ float s_sc[4][kUpdSlots];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t b = (int64_t)blockIdx.x * 4 + wave;
  if (b >= B) return;  // wave-uniform, as every exit below
  const int64_t u = rows[b];
  if (u < 0 || u >= n_users) return;
  int* ids = s_ids[wave];
  float* sc = s_sc[wave];
  // 1. the cached entries (lane e holds entry e), their marks, the count
  int my_id = -1;
  float my_v = -INFINITY;
  bool dirty = false;
  if (lane < k) {
    const int64_t c = idx[u * k + lane];
    my_v = vals[u * k + lane];
    if (c >= 0) {
      my_id = (int)c;
      dirty = c >= n_items || item_mark[c] != 0;  // an id past the table: dropped, never read
    }
  }
  const int cnt = counts[b];
  const unsigned long long real_m = __ballot(my_id >= 0);
  const unsigned long long dirty_m = __ballot(dirty);
  if (dirty_m == 0 && cnt == 0) return;  // nothing of this row changed: left unwritten
  if (cnt < 0 || cnt > cap) {            // more candidates than slots: the caller re-ranks
    if (lane == 0) redo[u] = 1;
    return;
  }
  const int n_real = __popcll(real_m);  // real entries come first: the list is padded behind
  const bool padded = n_real < k;
  // kappa, read before anything is overwritten (unused when the list is empty)
  const int last = n_real > 0 ? n_real - 1 : 0;
  const float kap_s = __shfl(my_v, last);
  const int kap_id = __shfl(my_id, last);
  // 2. the kept entries, compacted, then the candidates as item ids
  const bool keep = my_id >= 0 && !dirty;
  const unsigned long long keep_m = __ballot(keep);
  const int n_keep = __popcll(keep_m);
  if (keep) {
    const int pos = __popcll(keep_m & ((1ull << lane) - 1ull));
    ids[pos] = my_id;
    sc[pos] = my_v;
  }
  for (int i = lane; i < cnt; i += kWave) {
    const int col = cand[b * cap + i];
    int item = -1;
    if (col >= 0 && col < nd) {
      item = dirty_ids[col];
      if (item < 0 || item >= n_items) item = -1;
    }
    ids[n_keep + i] = item;
    sc[n_keep + i] = -INFINITY;
  }
  const int n = n_keep + cnt;  // <= k + cap <= kUpdSlots
  wave_lds_sync();
  // the candidates found in the user's exclusion row are struck (the kept entries were
  // eligible before and still are): 64 exclusion ids per round in the lanes, each
  // candidate compared with all of them at once.  The row may be unsorted and of any
  // length; nothing is staged.
  if (ex_ptr && cnt > 0) {
    const int64_t e0 = ex_ptr[u], e1 = ex_ptr[u + 1];
    for (int64_t base = e0; base < e1; base += kWave) {  // wave-uniform trip count
      const int ex = base + lane < e1 ? ex_idx[base + lane] : -1;
      for (int i = 0; i < cnt; ++i) {
        const int c = ids[n_keep + i];  // one address: a broadcast read
        if (c < 0) continue;            // wave-uniform
        if (__ballot(ex == c) != 0 && lane == 0) ids[n_keep + i] = -1;
      }
      wave_lds_sync();
    }
  }
  // 3. the surviving candidates rescored by lane groups, as topk_candidates_kernel does;
  // every lane of the wave calls cos_pair_vec4 (its DPP sums read their neighbours)
  constexpr int NPW = kWave / LPR;
  const int grp = lane / LPR, gl = lane % LPR;
  const float* pu = Hu + u * ldu;
  for (int i0 = 0; i0 < cnt; i0 += NPW) {  // wave-uniform bound
    const int i = i0 + grp;
    const int c = i < cnt ? ids[n_keep + i] : -1;
    const bool ok = c >= 0;
    const float r = cos_pair_vec4<LPR>(pu, Hi + (int64_t)(ok ? c : 0) * ldi, d, gl, ok);
    if (gl == LPR - 1 && ok) sc[n_keep + i] = r;
  }
  wave_lds_sync();
  // 4. ranks: ids are distinct (candidates are dirty, kept entries clean), so the order is
  // total; a lane owns slots lane, lane + 64, ...
  constexpr int PASSES = kUpdSlots / kWave;
  int rank[PASSES];
  int n_valid = 0;
  bool kth_ok = false;  // the entry of rank k - 1 is not worse than kappa
#pragma unroll
  for (int p = 0; p < PASSES; ++p) {
    const int i = p * kWave + lane;
    rank[p] = -1;
    const int c = i < n ? ids[i] : -1;
    if (c >= 0) {
      const float v = sc[i];
      int r = 0;
      for (int j = 0; j < n; ++j) {
        const int cj = ids[j];
        r += (cj >= 0 && better(sc[j], cj, v, c)) ? 1 : 0;
      }
      rank[p] = r;
      if (r == k - 1) kth_ok = !better(kap_s, kap_id, v, c);
    }
    n_valid += __popcll(__ballot(c >= 0));
  }
  // 5. the settle test against the OLD key, before any write
  const bool settled = padded || __ballot(kth_ok) != 0;
  if (!settled) {
    if (lane == 0) redo[u] = 1;
    return;
  }
#pragma unroll
  for (int p = 0; p < PASSES; ++p) {
    const int i = p * kWave + lane;
    if (rank[p] >= 0 && rank[p] < k) {
      vals[u * k + rank[p]] = sc[i];
      idx[u * k + rank[p]] = ids[i];
    }
  }
  for (int r = n_valid + lane; r < k; r += kWave) {  // only a padded list can come up short
    vals[u * k + r] = -INFINITY;
    idx[u * k + r] = -1;
  }
}

int check_score_args(const char* fn, const void* U, int64_t B, const void* V, int64_t n,
                     int64_t dpad) {
  GNNREC_REQUIRE(B >= 0 && n >= 0, "%s: negative size", fn);
  GNNREC_REQUIRE(dpad >= 32 && dpad % 32 == 0 && dpad <= kRecMaxD,
                 "%s: dpad must be a multiple of 32 in [32, %d] (got %lld)", fn, kRecMaxD,
                 (long long)dpad);
  GNNREC_REQUIRE(n < (int64_t(1) << 31), "%s: item ids must fit int32", fn);
  if (B == 0 || n == 0) return GNNREC_OK;
  GNNREC_REQUIRE(U && V && aligned16(U) && aligned16(V), "%s: null or unaligned table", fn);
  GNNREC_REQUIRE(((B + 127) / 128) * ((n + 127) / 128) < (int64_t(1) << 31),
                 "%s: too many tiles for one launch", fn);
  return GNNREC_OK;
}

}  // namespace
}  // namespace gnnrec

extern "C" int gnnrec_normalize_rows_bf16(const float* x, int64_t ld, int64_t n_rows, int64_t d,
                                          const int64_t* row_map, void* out, int64_t dpad,
                                          void* stream) {
  using namespace gnnrec;
  GNNREC_REQUIRE(n_rows >= 0 && d >= 1, "gnnrec_normalize_rows_bf16: bad size");
  GNNREC_REQUIRE(dpad == (d + 31) / 32 * 32 && dpad <= (int64_t(1) << 20),
                 "gnnrec_normalize_rows_bf16: dpad must be d rounded up to a multiple of 32 "
                 "(d %lld, dpad %lld)", (long long)d, (long long)dpad);
  if (n_rows == 0) return GNNREC_OK;
  GNNREC_REQUIRE(x && out && ld >= d, "gnnrec_normalize_rows_bf16: bad pointers / ld");
  GNNREC_REQUIRE(aligned16(out), "gnnrec_normalize_rows_bf16: out must be 16-byte aligned");
  GNNREC_REQUIRE((n_rows + 3) / 4 < (int64_t(1) << 31), "gnnrec_normalize_rows_bf16: too many rows");
  const bool vec = d % 4 == 0 && ld % 4 == 0 && aligned16(x);
  hipLaunchKernelGGL(normalize_rows_bf16_kernel, dim3((unsigned)((n_rows + 3) / 4)), dim3(256), 0,
                     as_stream(stream), x, ld, n_rows, (int)d, row_map,
                     static_cast<uint16_t*>(out), (int)dpad, vec);
  return check_launch("gnnrec_normalize_rows_bf16");
}

extern "C" int gnnrec_score_bf16_store(const void* users, int64_t n_users, const void* items,
                                       int64_t n_items, int64_t dpad, float* out, int64_t ldo,
                                       void* stream) {
  using namespace gnnrec;
  const int rc = check_score_args("gnnrec_score_bf16_store", users, n_users, items, n_items, dpad);
  if (rc != GNNREC_OK || n_users == 0 || n_items == 0) return rc;
  GNNREC_REQUIRE(out && ldo >= n_items, "gnnrec_score_bf16_store: bad out / ldo");
  launch_score<false>(static_cast<const uint16_t*>(users), n_users,
                      static_cast<const uint16_t*>(items), n_items, (int)dpad, out, ldo, nullptr,
                      nullptr, nullptr, 0, as_stream(stream));
  return check_launch("gnnrec_score_bf16_store");
}

extern "C" int gnnrec_score_bf16_filter(const void* users, int64_t n_users, const void* items,
                                        int64_t n_items, int64_t dpad, const float* tau,
                                        int32_t* counts, int32_t* cand_items, int64_t cap,
                                        void* stream) {
  using namespace gnnrec;
  const int rc = check_score_args("gnnrec_score_bf16_filter", users, n_users, items, n_items, dpad);
  if (rc != GNNREC_OK) return rc;
  GNNREC_REQUIRE(cap >= 1 && cap <= kCandMax, "gnnrec_score_bf16_filter: cap must be in [1, %d] "
                 "(got %lld)", kCandMax, (long long)cap);
  if (n_users == 0 || n_items == 0) return GNNREC_OK;
  GNNREC_REQUIRE(tau && counts && cand_items, "gnnrec_score_bf16_filter: null pointer");
  launch_score<true>(static_cast<const uint16_t*>(users), n_users,
                     static_cast<const uint16_t*>(items), n_items, (int)dpad, nullptr, 0, tau,
                     counts, cand_items, (int)cap, as_stream(stream));
  return check_launch("gnnrec_score_bf16_filter");
}

extern "C" int gnnrec_mask_excluded_f32(float* scores, int64_t ld, int64_t n_rows, int64_t n_cols,
                                       const int64_t* user_rows, const int64_t* exclude_indptr,
                                       const int32_t* exclude_indices, void* stream) {
  using namespace gnnrec;
  GNNREC_REQUIRE(n_rows >= 0 && n_cols >= 0 && (n_rows + 3) / 4 < (int64_t(1) << 31),
                 "gnnrec_mask_excluded_f32: bad size");
  if (n_rows == 0 || n_cols == 0) return GNNREC_OK;
  GNNREC_REQUIRE(scores && ld >= n_cols, "gnnrec_mask_excluded_f32: bad scores / ld");
  GNNREC_REQUIRE(exclude_indptr && exclude_indices,
                 "gnnrec_mask_excluded_f32: null exclusion list");
  hipLaunchKernelGGL(mask_excluded_kernel, dim3((unsigned)((n_rows + 3) / 4)), dim3(256), 0,
                     as_stream(stream), scores, ld, n_rows, n_cols, user_rows, exclude_indptr,
                     exclude_indices);
  return check_launch("gnnrec_mask_excluded_f32");
}

namespace gnnrec {
namespace {
// gnnrec_topk_candidates_f32, and with Z / p its rating form
int topk_candidates_impl(const int32_t* counts, const int32_t* cand_items, int64_t cap,
                         int64_t n_rows, const int64_t* user_rows, const float* h_user,
                         int64_t ldu, const float* h_item, int64_t ldi, int64_t d,
                         const int64_t* exclude_indptr, const int32_t* exclude_indices, int64_t k,
                         float* out_vals, int64_t* out_idx, const float* Z, const float* p,
                         void* stream) {
  GNNREC_REQUIRE(n_rows >= 0 && n_rows < (int64_t(1) << 31),
                 "gnnrec_topk_candidates_f32: bad row count");
  GNNREC_REQUIRE(cap >= 1 && cap <= kCandMax, "gnnrec_topk_candidates_f32: cap must be in "
                 "[1, %d] (got %lld)", kCandMax, (long long)cap);
  GNNREC_REQUIRE(k >= 1 && k <= cap, "gnnrec_topk_candidates_f32: k must be in [1, cap] "
                 "(got %lld)", (long long)k);
  GNNREC_REQUIRE(d >= 4 && d % 4 == 0 && ldu % 4 == 0 && ldi % 4 == 0 && ldu >= d && ldi >= d,
                 "gnnrec_topk_candidates_f32: needs d %% 4 == 0 and row strides that are "
                 "multiples of 4 and >= d");
  if (n_rows == 0) return GNNREC_OK;
  GNNREC_REQUIRE(counts && cand_items && h_user && h_item && out_vals && out_idx,
                 "gnnrec_topk_candidates_f32: null pointer");
  GNNREC_REQUIRE(aligned16(h_user) && aligned16(h_item),
                 "gnnrec_topk_candidates_f32: tables must be 16-byte aligned");
  GNNREC_REQUIRE(!exclude_indptr || exclude_indices,
                 "gnnrec_topk_candidates_f32: exclusion indptr without indices");
  hipStream_t s = as_stream(stream);
  const dim3 grid((unsigned)n_rows), block(256);
#define GNNREC_LAUNCH_CAND(LPR, RATING)                                                         \
  hipLaunchKernelGGL((topk_candidates_kernel<LPR, RATING>), grid, block, 0, s, counts,          \
                     cand_items, (int)cap, user_rows, h_user, ldu, h_item, ldi, (int)d,         \
                     exclude_indptr, exclude_indices, (int)k, out_vals, out_idx, Z, p)
  if (Z) {
    if (d <= 64) GNNREC_LAUNCH_CAND(16, true);
    else if (d <= 128) GNNREC_LAUNCH_CAND(32, true);
    else GNNREC_LAUNCH_CAND(64, true);
  } else {
    if (d <= 64) GNNREC_LAUNCH_CAND(16, false);  // the lane groups of gnnrec_sddmm_cos_f32
    else if (d <= 128) GNNREC_LAUNCH_CAND(32, false);
    else GNNREC_LAUNCH_CAND(64, false);
  }
#undef GNNREC_LAUNCH_CAND
  return check_launch("gnnrec_topk_candidates_f32");
}
}  // namespace
}  // namespace gnnrec

extern "C" int gnnrec_topk_candidates_f32(const int32_t* counts, const int32_t* cand_items,
                                          int64_t cap, int64_t n_rows, const int64_t* user_rows,
                                          const float* h_user, int64_t ldu, const float* h_item,
                                          int64_t ldi, int64_t d, const int64_t* exclude_indptr,
                                          const int32_t* exclude_indices, int64_t k,
                                          float* out_vals, int64_t* out_idx, void* stream) {
  return gnnrec::topk_candidates_impl(counts, cand_items, cap, n_rows, user_rows, h_user, ldu,
                                      h_item, ldi, d, exclude_indptr, exclude_indices, k, out_vals,
                                      out_idx, nullptr, nullptr, stream);
}

extern "C" int gnnrec_topk_candidates_rating_f32(
    const int32_t* counts, const int32_t* cand_items, int64_t cap, int64_t n_rows,
    const int64_t* user_rows, const float* h_user, int64_t ldu, const float* h_item, int64_t ldi,
    int64_t d, const int64_t* exclude_indptr, const int32_t* exclude_indices, const float* Z,
    const float* p, int64_t k, float* out_vals, int64_t* out_idx, void* stream) {
  using namespace gnnrec;
  GNNREC_REQUIRE(n_rows <= 0 || (Z && p), "gnnrec_topk_candidates_rating_f32: null Z / p");
  return topk_candidates_impl(counts, cand_items, cap, n_rows, user_rows, h_user, ldu, h_item, ldi,
                              d, exclude_indptr, exclude_indices, k, out_vals, out_idx, Z, p,
                              stream);
}

extern "C" int gnnrec_score_bf16_store_rating(const void* users, int64_t n_users,
                                              const void* items, int64_t n_items, int64_t dpad,
                                              const float* Z, const float* p_col, float* out,
                                              int64_t ldo, void* stream) {
  using namespace gnnrec;
  const char* fn = "gnnrec_score_bf16_store_rating";
  const int rc = check_score_args(fn, users, n_users, items, n_items, dpad);
  if (rc != GNNREC_OK || n_users == 0 || n_items == 0) return rc;
  GNNREC_REQUIRE(out && ldo >= n_items, "%s: bad out / ldo", fn);
  GNNREC_REQUIRE(Z && p_col, "%s: null Z / p_col", fn);
  launch_score<false, true>(static_cast<const uint16_t*>(users), n_users,
                            static_cast<const uint16_t*>(items), n_items, (int)dpad, out, ldo,
                            nullptr, nullptr, nullptr, 0, as_stream(stream), Z, p_col);
  return check_launch(fn);
}

extern "C" int gnnrec_score_bf16_filter_rating(const void* users, int64_t n_users,
                                               const void* items, int64_t n_items, int64_t dpad,
                                               const float* Z, const float* p_col,
                                               const float* thr, int32_t* counts,
                                               int32_t* cand_items, int64_t cap, void* stream) {
  using namespace gnnrec;
  const char* fn = "gnnrec_score_bf16_filter_rating";
  const int rc = check_score_args(fn, users, n_users, items, n_items, dpad);
  if (rc != GNNREC_OK) return rc;
  GNNREC_REQUIRE(cap >= 1 && cap <= kCandMax, "%s: cap must be in [1, %d] (got %lld)", fn,
                 kCandMax, (long long)cap);
  if (n_users == 0 || n_items == 0) return GNNREC_OK;
  GNNREC_REQUIRE(Z && p_col && thr && counts && cand_items, "%s: null pointer", fn);
  launch_score<true, true>(static_cast<const uint16_t*>(users), n_users,
                           static_cast<const uint16_t*>(items), n_items, (int)dpad, nullptr, 0,
                           thr, counts, cand_items, (int)cap, as_stream(stream), Z, p_col);
  return check_launch(fn);
}

extern "C" int gnnrec_topk_scored_candidates_f32(const int32_t* counts, const int32_t* cand_items,
                                                 const float* cand_scores, int64_t cap,
                                                 int64_t n_rows, const int64_t* user_rows,
                                                 const int64_t* exclude_indptr,
                                                 const int32_t* exclude_indices, int64_t k,
                                                 float* out_vals, int64_t* out_idx, void* stream) {
  using namespace gnnrec;
  GNNREC_REQUIRE(n_rows >= 0 && n_rows < (int64_t(1) << 31),
                 "gnnrec_topk_scored_candidates_f32: bad row count");
  GNNREC_REQUIRE(cap >= 1 && cap <= kCandMax, "gnnrec_topk_scored_candidates_f32: cap must be in "
                 "[1, %d] (got %lld)", kCandMax, (long long)cap);
  GNNREC_REQUIRE(k >= 1 && k <= cap, "gnnrec_topk_scored_candidates_f32: k must be in [1, cap] "
                 "(got %lld)", (long long)k);
  if (n_rows == 0) return GNNREC_OK;
  GNNREC_REQUIRE(counts && cand_items && cand_scores && out_vals && out_idx,
                 "gnnrec_topk_scored_candidates_f32: null pointer");
  GNNREC_REQUIRE(!exclude_indptr || exclude_indices,
                 "gnnrec_topk_scored_candidates_f32: exclusion indptr without indices");
  hipLaunchKernelGGL(topk_scored_candidates_kernel, dim3((unsigned)n_rows), dim3(256), 0,
                     as_stream(stream), counts, cand_items, cand_scores, (int)cap, user_rows,
                     exclude_indptr, exclude_indices, (int)k, out_vals, out_idx);
  return check_launch("gnnrec_topk_scored_candidates_f32");
}

extern "C" int gnnrec_topk_update_f32(const int64_t* rows, int64_t n_rows, int64_t* idx,
                                      float* vals, int64_t n_users, int64_t k,
                                      const int32_t* item_mark, int64_t n_items,
                                      const int32_t* counts, const int32_t* cand_cols,
                                      int64_t cap, const int32_t* dirty_ids, int64_t n_dirty,
                                      const float* h_user, int64_t ldu, const float* h_item,
                                      int64_t ldi, int64_t d, const int64_t* exclude_indptr,
                                      const int32_t* exclude_indices, int32_t* redo,
                                      void* stream) {
  using namespace gnnrec;
  const char* fn = "gnnrec_topk_update_f32";
  GNNREC_REQUIRE(n_rows >= 0 && n_users >= 0 && n_items >= 0 && n_dirty >= 0 &&
                     (n_rows + 3) / 4 < (int64_t(1) << 31),
                 "%s: bad size", fn);
  GNNREC_REQUIRE(n_items < (int64_t(1) << 31), "%s: item ids must fit int32", fn);
  GNNREC_REQUIRE(k >= 1 && k <= kUpdMaxK, "%s: k must be in [1, %d] (got %lld)", fn, kUpdMaxK,
                 (long long)k);
  GNNREC_REQUIRE(cap >= 1 && cap <= kUpdSlots - k, "%s: cap must be in [1, %d - k] (got %lld)",
                 fn, kUpdSlots, (long long)cap);
  GNNREC_REQUIRE(d >= 4 && d % 4 == 0 && ldu % 4 == 0 && ldi % 4 == 0 && ldu >= d && ldi >= d,
                 "%s: needs d %% 4 == 0 and row strides that are multiples of 4 and >= d", fn);
  if (n_rows == 0 || n_dirty == 0) return GNNREC_OK;  // no dirty item: no list can change
  GNNREC_REQUIRE(rows && idx && vals && item_mark && counts && cand_cols && dirty_ids && h_user &&
                     h_item && redo,
                 "%s: null pointer", fn);
  GNNREC_REQUIRE(aligned16(h_user) && aligned16(h_item), "%s: tables must be 16-byte aligned", fn);
  GNNREC_REQUIRE(!exclude_indptr || exclude_indices, "%s: exclusion indptr without indices", fn);
  hipStream_t s = as_stream(stream);
  const dim3 grid((unsigned)((n_rows + 3) / 4)), block(256);
#define GNNREC_LAUNCH_UPD(LPR)                                                                  \
  hipLaunchKernelGGL((topk_update_kernel<LPR>), grid, block, 0, s, rows, n_rows, idx, vals,     \
                     n_users, (int)k, item_mark, n_items, counts, cand_cols, (int)cap,          \
                     dirty_ids, n_dirty, h_user, ldu, h_item, ldi, (int)d, exclude_indptr,      \
                     exclude_indices, redo)
  if (d <= 64) GNNREC_LAUNCH_UPD(16);  // the lane groups of gnnrec_sddmm_cos_f32
  else if (d <= 128) GNNREC_LAUNCH_UPD(32);
  else GNNREC_LAUNCH_UPD(64);
#undef GNNREC_LAUNCH_UPD
  return check_launch(fn);
}
