// Shared device helpers of the neighbour gather (a1): used by the aggregation
// kernels (spmm.hip: dense, packed and dropout-masked source rows) and the fused
// aggregate+project kernels (spmm_project.hip, spmm_pair_mfma.hip), so all reduce
// every row in the same fixed order.  Below the gather: what the fused kernels share past
// it, their row epilogue and the streamed-weight MFMA projection.
#pragma once
#include "common.hpp"
#include "pack_rows.hpp"
#include <cmath>

namespace gnnrec {
namespace {

template <int VEC>
struct Frag {
  float v[VEC];
};

// Streams read or written once per launch (CSR indices / indptr, self rows, outputs and
// partials) vs the gathered source table, which should keep the caches: the streams use
// non-temporal loads / stores (C4 pass 143.0 -> 142.3 ms against plain ones in an alternating
// A/B, tools/micro/bench_ab.sh; tiles 4.45 -> 4.42 ms, fused 34.58 -> 34.45).
typedef float f32x4s __attribute__((ext_vector_type(4)));
template <typename T>
__device__ __forceinline__ T ld_stream(const T* p) {
  return __builtin_nontemporal_load(p);
}
__device__ __forceinline__ float4 ld_stream4(const float* p) {
  const f32x4s t = __builtin_nontemporal_load(reinterpret_cast<const f32x4s*>(p));
  return make_float4(t[0], t[1], t[2], t[3]);
}
__device__ __forceinline__ void st_stream4(float* p, float a, float b, float c, float d) {
  const f32x4s t = {a, b, c, d};
  __builtin_nontemporal_store(t, reinterpret_cast<f32x4s*>(p));
}

template <int VEC>
__device__ __forceinline__ void load_frag(Frag<VEC>& f, const float* p) {
  if constexpr (VEC == 4) {
    const float4 t = *reinterpret_cast<const float4*>(p);
    f.v[0] = t.x; f.v[1] = t.y; f.v[2] = t.z; f.v[3] = t.w;
  } else {
    f.v[0] = *p;
  }
}

template <int VEC>
__device__ __forceinline__ void store_frag(float* p, const Frag<VEC>& f) {
  if constexpr (VEC == 4) {
    st_stream4(p, f.v[0], f.v[1], f.v[2], f.v[3]);
  } else {
    *p = f.v[0];
  }
}

// A gather step's per-edge source index (and weight) to each lane group: lane group grp
// takes the range's edge base + grp, held by that lane of the index load.
// (readlane + select: at C4 the same pass time as __shfl's ds_bpermute, 142.56 ms both,
// with the LDS pipe left free; profiles/r06ad_c4_gather_readlane_ab.txt)
template <int NPI, typename T>
__device__ __forceinline__ T edge_bcast(T x, int base, int grp) {
  return bcast_groups<NPI>(x, base, grp);
}

template <int REDUCE>
__device__ __forceinline__ float combine(float a, float b) {
  return REDUCE == GNNREC_REDUCE_MAX ? fmaxf(a, b) : a + b;
}

// A gather's per-source-row hook: none.  One that is kOn (dropout.hpp's DropSrcMask) gives
// word(src, col), a value of the source row alone, and apply(frag, word, col).
struct NoSrcHook {
  static constexpr bool kOn = false;
};

// Per-lane partial reduction of edges [beg, end) (lane group grp takes k % NPI == grp).
// PRE: the first 64 indices of the range were loaded by the caller (lane k holds
// indices[beg + k]) — a row kernel prefetches them for row i+1 while row i gathers.
// hook: applied to every gathered fragment; its words depend on the broadcast indices only,
// so they are computed after a step's UNROLL loads are issued, while those are in flight.
template <int LPR, int VEC, int REDUCE, bool WEIGHTED, int UNROLL, bool PRE = false,
          class Hook = NoSrcHook>
__device__ __forceinline__ void gather_range(int64_t beg, int64_t end,
                                             const int32_t* __restrict__ indices,
                                             const float* __restrict__ ew,
                                             const float* __restrict__ X, int64_t ldx, int col,
                                             bool colok, int lane, int grp, Frag<VEC>& acc,
                                             int pre_idx = 0, const Hook& hook = {}) {
  constexpr int NPI = kWave / LPR;
  for (int64_t base = beg; base < end; base += 64) {
    const int cnt = (int)((end - base) < 64 ? (end - base) : 64);
    int myidx;
    if (PRE && base == beg) myidx = pre_idx;
    else myidx = lane < cnt ? ld_stream(indices + base + lane) : 0;
    float myw = 0.f;
    if constexpr (WEIGHTED) myw = lane < cnt ? ld_stream(ew + base + lane) : 0.f;
    for (int j = 0; j < cnt; j += NPI * UNROLL) {
      Frag<VEC> val[UNROLL];
      bool ok[UNROLL];
      int src[UNROLL];
#pragma unroll
      for (int u = 0; u < UNROLL; ++u) {
        const int k = j + u * NPI + grp;
        ok[u] = (k < cnt) && colok;
        src[u] = edge_bcast<NPI>(myidx, j + u * NPI, grp);
        if (ok[u]) {
          load_frag<VEC>(val[u], X + (int64_t)src[u] * ldx + col);
        } else {
#pragma unroll
          for (int v = 0; v < VEC; ++v) val[u].v[v] = 0.f;
        }
      }
      [[maybe_unused]] uint64_t word[UNROLL];
      if constexpr (Hook::kOn) {
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) word[u] = hook.word(src[u], col);
      }
#pragma unroll
      for (int u = 0; u < UNROLL; ++u) {
        float w = 1.f;
        if constexpr (WEIGHTED) w = edge_bcast<NPI>(myw, j + u * NPI, grp);
        if constexpr (Hook::kOn) hook.apply(val[u], word[u], col);
#pragma unroll
        for (int v = 0; v < VEC; ++v) {
          const float m = WEIGHTED ? val[u].v[v] * w : val[u].v[v];
          if constexpr (REDUCE == GNNREC_REDUCE_MAX) {
            if (ok[u]) acc.v[v] = fmaxf(acc.v[v], m);
          } else {
            acc.v[v] += m;
          }
        }
      }
    }
  }
}

// gather_range (LPR = 32, VEC = 4, sum / mean, unweighted) over a packed table
// (pack_rows.hpp): the same chunks, lane groups, UNROLL and adds in the same order, so an
// aggregate is bitwise the dense gather's — an unset mask bit decodes to +0.0, the value it
// stands for.  Per step, lanes 0-23 of a group load the 16-B pieces of the packed row (no
// dependent load); the wave stages the step's UNROLL row pairs in its own LDS (`stage`:
// UNROLL x 192 words, written and read by this wave only) and every lane reads back its
// mask nibble, the popcount prefix and its up to four values at their packed positions.
// A step in which any group drew a `dense` row takes a wave-uniform branch and reads those
// rows' fragments from the dense table X.
template <int UNROLL, bool PRE = false>
__device__ __forceinline__ void gather_range_packed(int64_t beg, int64_t end,
                                                    const int32_t* __restrict__ indices,
                                                    const uint32_t* __restrict__ P,
                                                    const float* __restrict__ X, int64_t ldx,
                                                    int lane, int grp, Frag<4>& acc,
                                                    uint32_t* stage, int pre_idx = 0) {
  constexpr int NPI = 2;
  const int l = lane & 31;
  const int w = l >> 3, sh = (l & 7) * 4;
  uint32_t* mine = stage + grp * kPackWords;
  for (int64_t base = beg; base < end; base += 64) {
    const int cnt = (int)((end - base) < 64 ? (end - base) : 64);
    int myidx;
    if (PRE && base == beg) myidx = pre_idx;
    else myidx = lane < cnt ? ld_stream(indices + base + lane) : 0;
    for (int j = 0; j < cnt; j += NPI * UNROLL) {
      uint4 q[UNROLL];
      int src[UNROLL];
#pragma unroll
      for (int u = 0; u < UNROLL; ++u) {
        const int k = j + u * NPI + grp;
        src[u] = edge_bcast<NPI>(myidx, j + u * NPI, grp);
        q[u] = make_uint4(0u, 0u, 0u, 0u);
        if (k < cnt && l < kPackWords / 4)
          q[u] = *reinterpret_cast<const uint4*>(P + (int64_t)src[u] * kPackWords + 4 * l);
      }
      Frag<4> val[UNROLL];
      uint64_t dense[UNROLL], any_dense = 0;  // lane 1 of a group holds its row's flag word
#pragma unroll
      for (int u = 0; u < UNROLL; ++u) {
        if (l < kPackWords / 4)
          *reinterpret_cast<uint4*>(mine + u * 2 * kPackWords + 4 * l) = q[u];
        dense[u] = __ballot(l == 1 && (q[u].y & kPackDenseBit) != 0u);
        any_dense |= dense[u];
      }
      __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
#pragma unroll
      for (int u = 0; u < UNROLL; ++u) {
        const uint32_t* r = mine + u * 2 * kPackWords;
        const uint32_t m = r[w];
        const uint32_t nib = (m >> sh) & 15u;
        uint32_t p = ((r[4] >> (8 * w)) & 255u) + __popc(m & ((1u << sh) - 1u));
#pragma unroll
        for (int v = 0; v < 4; ++v) {
          // slot of column 4l + v (read whether or not the bit is set: clamped to the row)
          const uint32_t x =
              r[kPackHdrWords + (p < (uint32_t)kPackSlots - 1 ? p : kPackSlots - 1)];
          val[u].v[v] = (nib >> v) & 1u ? __builtin_bit_cast(float, x) : 0.f;
          p += (nib >> v) & 1u;
        }
      }
      __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");  // the stage is rewritten next
      if (any_dense != 0) {
#pragma unroll
        for (int u = 0; u < UNROLL; ++u)
          if ((dense[u] >> (32 * grp + 1)) & 1ull)
            load_frag<4>(val[u], X + (int64_t)src[u] * ldx + 4 * l);
      }
#pragma unroll
      for (int u = 0; u < UNROLL; ++u)
#pragma unroll
        for (int v = 0; v < 4; ++v) acc.v[v] += val[u].v[v];
    }
  }
}

template <int LPR, int VEC, int REDUCE>
__device__ __forceinline__ void combine_groups(Frag<VEC>& acc) {
#pragma unroll
  for (int off = LPR; off < kWave; off <<= 1) {
#pragma unroll
    for (int v = 0; v < VEC; ++v) acc.v[v] = combine<REDUCE>(acc.v[v], __shfl_xor(acc.v[v], off));
  }
}

// acc = out[row] (+ | max) acc: a source-range tile added to the partial of earlier tiles
template <int VEC, int REDUCE>
__device__ __forceinline__ void accumulate_into(Frag<VEC>& acc, const float* p) {
  Frag<VEC> o;
  if constexpr (VEC == 4) {
    const float4 t = ld_stream4(p);
    o.v[0] = t.x; o.v[1] = t.y; o.v[2] = t.z; o.v[3] = t.w;
  } else {
    load_frag<VEC>(o, p);
  }
#pragma unroll
  for (int v = 0; v < VEC; ++v) acc.v[v] = combine<REDUCE>(o.v[v], acc.v[v]);
}

template <int VEC, int REDUCE>
__device__ __forceinline__ void finalize(Frag<VEC>& acc, int64_t deg, int empty_neginf) {
  if constexpr (REDUCE == GNNREC_REDUCE_MEAN) {
    const float dd = (float)(deg > 0 ? deg : 1);
#pragma unroll
    for (int v = 0; v < VEC; ++v) acc.v[v] = acc.v[v] / dd;
  } else if constexpr (REDUCE == GNNREC_REDUCE_MAX) {
    if (deg == 0 && !empty_neginf) {
#pragma unroll
      for (int v = 0; v < VEC; ++v) acc.v[v] = 0.f;
    }
  }
}

// Up to 4 rows [rbase, rbase + nv) of one relation gathered in lockstep (LPR = 32, VEC = 4):
// their bounds and first 64 indices (and weights) are requested together, then every step
// issues the loads of all 4 rows (4·LU·2 source rows in flight per wave), so a 10-edge row
// does not pay its own index -> row round trips.  Each row's neighbours are still summed by
// lane group in gather_range's order (k = j + u·NPI + grp, ascending: the same sequence for
// any LU), so the aggregate has gather_range's bits; when any of the rows has more than 64
// edges, all take gather_range<..., UNROLL, PRE> row by row.  acc[i]: row i's aggregate after
// combine_groups and finalize, in every lane group; dg[i]: its degree (0 from row nv on).
template <int REDUCE, bool WEIGHTED, int LU, int UNROLL>
__device__ __forceinline__ void gather_lockstep4(const int64_t* __restrict__ indptr,
                                                 const int32_t* __restrict__ indices,
                                                 const float* __restrict__ ew,
                                                 const float* __restrict__ X, int64_t ldx,
                                                 int64_t rbase, int nv, int lane,
                                                 Frag<4> (&acc)[4], int (&dg)[4]) {
  constexpr int LPR = 32, VEC = 4, NPI = kWave / LPR, kLR = 4;
  const int grp = lane / LPR, col = (lane % LPR) * VEC;
  const float init = (REDUCE == GNNREC_REDUCE_MAX) ? -INFINITY : 0.f;
  const int64_t ipl = nv > 0 && lane <= nv ? ld_stream(indptr + rbase + lane) : 0;
  int64_t b[kLR + 1];
#pragma unroll
  for (int i = 0; i <= kLR; ++i) b[i] = __shfl(ipl, i <= nv ? i : nv);
  int ridx[kLR];
  float rwt[kLR];
  int dmax = 0;
#pragma unroll
  for (int i = 0; i < kLR; ++i) {
    dg[i] = i < nv ? (int)(b[i + 1] - b[i]) : 0;
    ridx[i] = lane < dg[i] ? ld_stream(indices + b[i] + lane) : 0;
    rwt[i] = 0.f;
    if constexpr (WEIGHTED) rwt[i] = lane < dg[i] ? ld_stream(ew + b[i] + lane) : 0.f;
    dmax = dg[i] > dmax ? dg[i] : dmax;
#pragma unroll
    for (int v = 0; v < VEC; ++v) acc[i].v[v] = init;
  }
  if (dmax <= 64) {
    for (int j = 0; j < dmax; j += NPI * LU) {
      Frag<VEC> val[kLR][LU];
      bool ok[kLR][LU];
#pragma unroll
      for (int i = 0; i < kLR; ++i)
#pragma unroll
        for (int u = 0; u < LU; ++u) {
          ok[i][u] = j + u * NPI + grp < dg[i];
          const int src = edge_bcast<NPI>(ridx[i], j + u * NPI, grp);
          if (ok[i][u]) {
            load_frag<VEC>(val[i][u], X + (int64_t)src * ldx + col);
          } else {
#pragma unroll
            for (int v = 0; v < VEC; ++v) val[i][u].v[v] = 0.f;
          }
        }
#pragma unroll
      for (int i = 0; i < kLR; ++i)
#pragma unroll
        for (int u = 0; u < LU; ++u) {
          float w = 1.f;
          if constexpr (WEIGHTED) w = edge_bcast<NPI>(rwt[i], j + u * NPI, grp);
#pragma unroll
          for (int v = 0; v < VEC; ++v) {
            const float m = WEIGHTED ? val[i][u].v[v] * w : val[i][u].v[v];
            if constexpr (REDUCE == GNNREC_REDUCE_MAX) {
              if (ok[i][u]) acc[i].v[v] = fmaxf(acc[i].v[v], m);
            } else {
              acc[i].v[v] += m;
            }
          }
        }
    }
  } else {
#pragma unroll
    for (int i = 0; i < kLR; ++i)
      if (i < nv)
        gather_range<LPR, VEC, REDUCE, WEIGHTED, UNROLL, true>(
            b[i], b[i + 1], indices, ew, X, ldx, col, true, lane, grp, acc[i], ridx[i]);
  }
#pragma unroll
  for (int i = 0; i < kLR; ++i) {
    combine_groups<LPR, VEC, REDUCE>(acc[i]);
    finalize<VEC, REDUCE>(acc[i], dg[i], 0);
  }
}

// ---- row epilogue of the fused aggregate+project kernels: a wave holds one output row, lane
// = its columns j0 = 2·lane and j0 + 1 ---------------------------------------------------------
typedef float f32x2s __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void st_stream2(float* p, float a, float b) {
  __builtin_nontemporal_store(f32x2s{a, b}, reinterpret_cast<f32x2s*>(p));
}

// ReLU and the zero-guarded row L2 norm over the wave's 64 lanes
__device__ __forceinline__ void activate(bool relu, bool l2, float& y0, float& y1) {
  if (relu) {
    y0 = fmaxf(y0, 0.f);
    y1 = fmaxf(y1, 0.f);
  }
  if (l2) {
    float ss = y0 * y0 + y1 * y1;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) ss += __shfl_xor(ss, off);
    float nrm = sqrtf(ss);
    if (nrm == 0.f) nrm = 1.f;
    y0 = y0 / nrm;
    y1 = y1 / nrm;
  }
}

// Two relations' activated rows ya, yb into one: max, sum, or (GNNREC_ACC_ATTN_LAST) the
// softmax over the two relations of s_r = a·y_r, (at0, at1) this lane's pair of a — as the
// single-relation launches' online form: a first (max s_a, sum 1), then b rescales and
// normalises.  Then out_div and one non-temporal store to p (the row's columns j0, j0 + 1)
// when `valid` (wave-uniform; padding rows take part in the shuffles, store nothing).
__device__ __forceinline__ void combine2_store(float ya0, float ya1, float yb0, float yb1,
                                               int combine, float at0, float at1, float out_div,
                                               bool valid, float* p) {
  float y0, y1;
  if (combine == GNNREC_ACC_MAX) {
    y0 = fmaxf(ya0, yb0);
    y1 = fmaxf(ya1, yb1);
  } else if (combine == GNNREC_ACC_ATTN_LAST) {
    float sa = ya0 * at0 + ya1 * at1, sb = yb0 * at0 + yb1 * at1;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      sa += __shfl_xor(sa, off);
      sb += __shfl_xor(sb, off);
    }
    const float mnew = fmaxf(sa, sb);
    const float keep = expf(sa - mnew), cnew = expf(sb - mnew);
    const float nrm = 1.f / (1.f * keep + cnew);
    y0 = (ya0 * keep + yb0 * cnew) * nrm;
    y1 = (ya1 * keep + yb1 * cnew) * nrm;
  } else {
    y0 = ya0 + yb0;
    y1 = ya1 + yb1;
  }
  if (out_div > 0.f) {
    y0 = y0 / out_div;
    y1 = y1 / out_div;
  }
  if (valid) st_stream2(p, y0, y1);
}

// ---- 32-row projection on the fp32 MFMA, the B operands (weights) streamed from L2 --------------
typedef float f32x16 __attribute__((ext_vector_type(16)));
constexpr int kMfmaWChunk = 16;  // B operands per chunk (64 — all loaded up front — measured slower)

// Buffer resource over `bytes` of weights at the wave-uniform pointer p: loads then take one
// 32-bit per-lane offset plus an immediate row offset, instead of hoisted 64-bit addresses
// (which the compiler spills)
__device__ __forceinline__ auto weight_rsrc(const void* p, int bytes) {
  const uint64_t base =
      ((uint64_t)__builtin_amdgcn_readfirstlane((unsigned)((uintptr_t)p >> 32)) << 32) |
      (unsigned)__builtin_amdgcn_readfirstlane((unsigned)(uintptr_t)p);
  return __builtin_amdgcn_make_buffer_rsrc(reinterpret_cast<void*>(base), 0, bytes, 0x00020000);
}

// C (32 × 32) = A · B over KL values of K per lane half, as KL v_mfma_f32_32x32x2_f32: lane
// (row li = lane & 31, half bh = lane >> 5) reads its A operands from ap[0, KL) (an LDS tile
// row, ds_read_b128) and B operand i from byte offset wvoff + i·WLD·4 of the weight buffer, in
// chunks of kMfmaWChunk, double-buffered: the next chunk's loads are in flight under this
// chunk's MFMAs instead of KL live registers.
template <int KL, int WLD, class Rsrc>
__device__ __forceinline__ f32x16 mfma_project32(const Rsrc& wrsrc, int wvoff, const float* ap) {
  constexpr int kWC = kMfmaWChunk;
  float bw[2][kWC];
  auto load_w = [&](float* dst, int i0) __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < kWC; ++i)
      dst[i] = __uint_as_float(
          __builtin_amdgcn_raw_buffer_load_b32(wrsrc, wvoff, (i0 + i) * WLD * 4, 0));
  };
  f32x16 c;
#pragma unroll
  for (int v = 0; v < 16; ++v) c[v] = 0.f;
  load_w(bw[0], 0);
#pragma unroll
  for (int ch = 0; ch < KL / kWC; ++ch) {
    if (ch + 1 < KL / kWC) load_w(bw[(ch + 1) & 1], (ch + 1) * kWC);
    __builtin_amdgcn_sched_barrier(0);
    const float* w = bw[ch & 1];
#pragma unroll
    for (int i = 0; i < kWC; i += 4) {
      const f32x4s a = *reinterpret_cast<const f32x4s*>(ap + ch * kWC + i);
      c = __builtin_amdgcn_mfma_f32_32x32x2f32(a[0], w[i], c, 0, 0, 0);
      c = __builtin_amdgcn_mfma_f32_32x32x2f32(a[1], w[i + 1], c, 0, 0, 0);
      c = __builtin_amdgcn_mfma_f32_32x32x2f32(a[2], w[i + 2], c, 0, 0, 0);
      c = __builtin_amdgcn_mfma_f32_32x32x2f32(a[3], w[i + 3], c, 0, 0, 0);
    }
    __builtin_amdgcn_sched_barrier(0);
  }
  return c;
}

// The accumulator to a C tile of row stride ld, cp = the tile's column of this lane (block
// column + lane & 31).  D map of the 32x32 MFMA: col = lane & 31, row = (v & 3) + 8 (v >> 2) + 4 bh
__device__ __forceinline__ void store_c32(float* cp, int ld, int bh, const f32x16& c) {
#pragma unroll
  for (int v = 0; v < 16; ++v) cp[((v & 3) + 8 * (v >> 2) + 4 * bh) * ld] = c[v];
}

}  // namespace
}  // namespace gnnrec
