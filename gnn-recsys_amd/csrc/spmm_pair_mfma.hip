// a1+a3+a4 fused for TWO relations that gather from ONE source table (C5's clicked-by and
// bought-by, both item -> user), the projections on the fp32 MFMA:
//   out[v] = combine( epi(h[v]·W_self,aᵀ + agg_a(v)·W_neigh,aᵀ + b_a [+ bne_a]),
//                     epi(h[v]·W_self,bᵀ + agg_b(v)·W_neigh,bᵀ + b_b [+ bne_b]) ) / out_div
// agg_r = sum / mean over relation r's in-edges of X[src] (· w_e), X the SHARED source table.
// Reference: ConvLayer.forward (src/model.py:143-148 aggregation, :226-235 projection, ReLU,
// norm) for each relation, HeteroGraphConv's cross-relation combine (:384-406).
//
// Why a second pair kernel: gnnrec_spmm_project2_f32 gathers two PRE-projected tables
// (X·W_neigh,aᵀ and X·W_neigh,bᵀ, 512 MB each at C5): a 1 GB working set against the
// 256 MB Infinity Cache, so the lower-degree relation's gathers go to HBM proper (the
// launch ran at 0.906 of 8 TB/s against 0.955 for C4's one-table launch), and the two
// pre-projection GEMMs sit on the layer's critical path.  Here both relations gather the
// one raw 512 MB table, and all four 128×128 projections run in the epilogue.  Four fp32
// weight matrices (256 KiB) do not fit in LDS, so the VALU matvec of the one-relation kernel
// is out; instead a block owns 32-row tiles:
//   gather   each of the 8 waves gathers 4 rows of relation a, then of relation b, with
//            gather.hpp's gather_lockstep4 (the one spmm_project_mfma_kernel calls; per row
//            gather_range's summation order, so each aggregate has spmm_csr_kernel's bits),
//            into the LDS tile A = [h_self | agg_a | agg_b] (32 × 384 fp32, row stride 388
//            floats: conflict-free ds_read_b128);
//   project  wave w owns output columns 32·(w & 3) of relation (w >> 2): C = [h | agg_r] ·
//            [W_self,r | W_neigh,r]ᵀ, K = 256, as 128 v_mfma_f32_32x32x2_f32 — lane half 0
//            consumes the self half of K, lane half 1 the neighbour half (a fixed
//            permutation of the reference's summation order); the B operands stream from L2
//            by buffer loads out of ONE packed [4][128][128] k-major weight array (a
//            wave-uniform base) in gather.hpp's mfma_project32, chunks of 16 double-buffered
//            under the MFMAs — 256 KiB per 32 rows instead of per row pair;
//   epilogue C of both relations lands in LDS over the A tile; each wave finishes 4 rows:
//            bias (+ the non-empty bias), then gather.hpp's activate and combine2_store
//            (spmm_project2_pipe_kernel's row epilogue: sum, max, or the attention softmax
//            over the two relations, in registers), one non-temporal 512-B store per row.
// Two blocks per CU (≈50 KiB of LDS each), so one block's MFMA phase runs under the other's
// gather.  Rows come in whole tiles through rowq.hpp's TileCursor (the row queue, or an
// XCD-contiguous static walk).
//
// Measured (C5 user side, 10M rows × (40 + 10) edges, 268 GB, tools/gpu/r04c_pairvar.sh and
// r04e_pairh.sh): the gather phase alone (a round-4 timing build) 34.6 ms = 0.969 of
// 8 TB/s — one 512 MB table is the cache-friendly working set the pre-projected launch lacks —
// the MFMA phase alone 14.8 ms, the launch 38.4–38.6 ms (0.87): while one block sits in its
// MFMA phase only the other block's 8 waves gather.  The pre-projected launch takes 36.6–37.8
// ms plus its two 1M-row GEMMs, so the C5 passes come out within 0.5 ms of each other
// (153.3–154.0 vs 154.0–154.4 ms); the sharded pass keeps the pre-projected form by default
// (GNNREC_PAIR_RAW=1 selects this one).  Not kept: a software-pipelined form (the previous
// tile's MFMAs interleaved into this tile's gather steps, operands loaded one chunk ahead,
// aggregates double-buffered, self rows straight from H by buffer loads) — 43.9 ms, its MFMA
// state and gather share 128 VGPRs and spill 124–152 B/lane; LU = 1 / 3 lockstep unrolls 39.9
// / 39.1 ms; the self rows requested ahead of the gathers: unchanged.
//
// Not kept either (tools/EXPERIMENTS.md): the projections as six bf16 MFMA products of
// three-way split operands (fp32-accurate, 2.7x fewer MFMA issue cycles but 1.5x the weight
// bytes per tile: launch 47.3 vs 38.7 ms, profiles/r04j_pair_bf16x3_ab.md).  What bounds the
// projection phase (14.2 ms against 8.3 ms of MFMA issue at 2.4 GHz) is not the weight
// stream's latency — streaming the weights 8, 16 or 32 k-steps ahead changed nothing
// (profiles/r04r_pair_weight_stream.md) — but the clock under MFMA load (≈2.0-2.2 GHz) and
// each tile's epilogue and barriers beside the MFMAs; both phases need all 16 resident waves
// (profiles/r04s_pair_waves_per_cu.md).  48-row tiles / a third block per CU were not
// attempted: the pre-projected launch stays the default.
#include "common.hpp"
#include "gather.hpp"
#include "rowq.hpp"

namespace gnnrec {
namespace {

constexpr int kQD = 128;                 // d (source, self and output width)
constexpr int kQT = 32;                  // rows per tile
constexpr int kQWaves = 8;               // waves per block
constexpr int kQRows = kQT / kQWaves;    // rows gathered per wave per tile
constexpr int kQALd = 3 * kQD + 4;       // A tile row stride (floats)
constexpr int kQCLd = kQD + 8;           // C tile row stride
constexpr int kQLU = 2;   // lockstep gather: steps of 2·LU neighbours of 4 rows at once
constexpr int kQU = 4;    // gather_range unroll for rows above 64 edges
static_assert(2 * kQT * kQCLd <= kQT * kQALd, "C tiles must fit over the A tile");
static_assert(kQRows == 4, "a wave gathers its rows with one gather_lockstep4");

// Four consecutive A-tile elements of row `row`, columns [c, c + 4)
__device__ __forceinline__ void put4(float* tile, int row, int c, float4 v) {
  *reinterpret_cast<float4*>(tile + row * kQALd + c) = v;
}

struct RawRel {
  const int64_t* indptr;
  const int32_t* indices;
  const float* ew;
  const float* bias;     // b_r (NULL: none)
  const float* bias_ne;  // added to rows with >= 1 in-edge (NULL: none)
  int mean;
};

// The 4 rows [rbase, rbase + nv) of one relation, gathered in lockstep into A tile columns
// [cofs, cofs + 128) of tile rows [r0, r0 + 4); their non-empty flags into ne[].
template <bool W>
__device__ __forceinline__ void gather_rel(const RawRel& r, const float* __restrict__ X,
                                           int64_t ldx, int64_t rbase, int nv, float* As,
                                           int r0, int cofs, int* ne, int lane) {
  Frag<4> acc[kQRows];
  int dg[kQRows];
  gather_lockstep4<GNNREC_REDUCE_SUM, W, kQLU, kQU>(r.indptr, r.indices, r.ew, X, ldx, rbase, nv,
                                                    lane, acc, dg);
#pragma unroll
  for (int i = 0; i < kQRows; ++i) {
    if (r.mean) finalize<4, GNNREC_REDUCE_MEAN>(acc[i], dg[i], 0);
    if (lane < 32)
      put4(As, r0 + i, cofs + lane * 4,
           make_float4(acc[i].v[0], acc[i].v[1], acc[i].v[2], acc[i].v[3]));
    if (lane == 0) ne[r0 + i] = dg[i] > 0;
  }
}

template <bool WA, bool WB>
__global__ __launch_bounds__(kQWaves * 64, 4) void spmm_pair_mfma_kernel(
    RawRel ra, RawRel rb, const float* __restrict__ X, int64_t ldx, const float* __restrict__ H,
    int64_t ldh, const float* __restrict__ WT4, int64_t n_dst, int epilogue, int combine,
    const float* __restrict__ attn_vec, float out_div, float* __restrict__ out, int64_t ldo,
    unsigned* rq, int rq_ch) {
  __shared__ __attribute__((aligned(16))) float As[kQT * kQALd];
  __shared__ int nes[2][kQT];
  __shared__ int64_t blk_r[2];
  float* const Ca = reinterpret_cast<float*>(As);  // over the A tile once the MFMAs read it
  float* const Cb = Ca + kQT * kQCLd;

  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int li = lane & 31, bh = lane >> 5;
  const int col = li * 4;
  const int j0 = 2 * lane;
  const int cb = wave & 3, rr = wave >> 2;
  const bool relu = epilogue & GNNREC_EPI_RELU, l2 = epilogue & GNNREC_EPI_L2NORM;

  // B operands: lane half bh of a relation-rr wave reads matrix 2·rr + bh of the packed
  // [W_self,aᵀ, W_neigh,aᵀ, W_self,bᵀ, W_neigh,bᵀ] (each k-major 128×128): element
  // [i][32·cb + li]
  const auto wrsrc = weight_rsrc(WT4, 4 * kQD * kQD * 4);
  const int wvoff = ((2 * rr + bh) * kQD * kQD + 32 * cb + li) * 4;
  // A operands: row li of the tile, K columns [0, 128) (self) for lane half 0 and the
  // relation's aggregate [128 + 128·rr, +128) for lane half 1
  const int acol = bh ? kQD + kQD * rr : 0;
  const float* const ap = As + li * kQALd + acol;

  auto tile = [&](int64_t t0, int64_t lim) __attribute__((always_inline)) {
    const int64_t rbase = t0 + wave * kQRows;
    const int64_t left = lim - rbase;
    const int nv = (int)(left <= 0 ? 0 : left < kQRows ? left : kQRows);
    const int r0 = wave * kQRows;
    // self rows, two per instruction, requested before the gathers (their latency hides
    // under the gathers instead of ahead of the MFMA phase's barrier)
    float4 hs[kQRows / 2];
#pragma unroll
    for (int q = 0; q < kQRows / 2; ++q) {
      const int rl = 2 * q + bh;
      hs[q] = rl < nv ? ld_stream4(H + (rbase + rl) * ldh + col) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    gather_rel<WA>(ra, X, ldx, rbase, nv, As, r0, kQD, nes[0], lane);
    gather_rel<WB>(rb, X, ldx, rbase, nv, As, r0, 2 * kQD, nes[1], lane);
#pragma unroll
    for (int q = 0; q < kQRows / 2; ++q) put4(As, r0 + 2 * q + bh, col, hs[q]);
    __syncthreads();

    const f32x16 c = mfma_project32<kQD, kQD>(wrsrc, wvoff, ap);
    __syncthreads();  // every wave's MFMAs have read the A tile: C goes over it
    store_c32((rr ? Cb : Ca) + 32 * cb + li, kQCLd, bh, c);
    __syncthreads();

    const float ba0 = ra.bias ? ra.bias[j0] : 0.f, ba1 = ra.bias ? ra.bias[j0 + 1] : 0.f;
    const float bb0 = rb.bias ? rb.bias[j0] : 0.f, bb1 = rb.bias ? rb.bias[j0 + 1] : 0.f;
    const bool attn = combine == GNNREC_ACC_ATTN_LAST;
    const float at0 = attn ? attn_vec[j0] : 0.f, at1 = attn ? attn_vec[j0 + 1] : 0.f;
#pragma unroll
    for (int r = 0; r < kQRows; ++r) {
      const int rl = r0 + r;
      const float2 za = *reinterpret_cast<const float2*>(&Ca[rl * kQCLd + j0]);
      const float2 zb = *reinterpret_cast<const float2*>(&Cb[rl * kQCLd + j0]);
      float ya0 = za.x + ba0, ya1 = za.y + ba1;
      float yb0 = zb.x + bb0, yb1 = zb.y + bb1;
      if (ra.bias_ne && nes[0][rl]) {
        ya0 += ra.bias_ne[j0];
        ya1 += ra.bias_ne[j0 + 1];
      }
      if (rb.bias_ne && nes[1][rl]) {
        yb0 += rb.bias_ne[j0];
        yb1 += rb.bias_ne[j0 + 1];
      }
      activate(relu, l2, ya0, ya1);
      activate(relu, l2, yb0, yb1);
      combine2_store(ya0, ya1, yb0, yb1, combine, at0, at1, out_div, r < nv,
                     out + (rbase + r) * ldo + j0);
    }
    __syncthreads();  // the tile's LDS is free for the next one
  };

  TileCursor<kQT> cur;
  cur.begin(rq, n_dst, rq_ch, blk_r);
  int64_t r0, r1;
  while (cur.next(r0, r1))
    for (int64_t t0 = r0; t0 < r1; t0 += kQT) tile(t0, r1);
  if (rq != nullptr) rq_finish(rq);
}

}  // namespace
}  // namespace gnnrec

using namespace gnnrec;

extern "C" int gnnrec_spmm_pair_f32(
    const int64_t* indptr_a, const int32_t* indices_a, const float* ew_a, int reduce_a,
    const float* bias_a, const float* bias_nonempty_a, const int64_t* indptr_b,
    const int32_t* indices_b, const float* ew_b, int reduce_b, const float* bias_b,
    const float* bias_nonempty_b, const float* X, int64_t n_src, int64_t ldx, const float* H,
    int64_t ldh, const float* WT4, int64_t n_dst, int64_t d, int epilogue,
    int combine, const float* attn_vec, float out_div, float* out, int64_t ldo, void* stream) {
  const char* const name = "gnnrec_spmm_pair_f32";
  GNNREC_REQUIRE((reduce_a == GNNREC_REDUCE_SUM || reduce_a == GNNREC_REDUCE_MEAN) &&
                     (reduce_b == GNNREC_REDUCE_SUM || reduce_b == GNNREC_REDUCE_MEAN),
                 "gnnrec_spmm_pair_f32: both relations reduce by sum or mean");
  const int st = fused_check(name, d, epilogue, true, combine, attn_vec, nullptr, n_dst, 'X',
                             {indptr_a, indptr_b, X, H}, {X, H, WT4}, {ldx, ldh}, out, ldo);
  if (st != GNNREC_OK || n_dst == 0) return st;
  GNNREC_REQUIRE(WT4 != nullptr, "gnnrec_spmm_pair_f32: null WT4");
  GNNREC_REQUIRE(n_src >= 0, "gnnrec_spmm_pair_f32: negative n_src");
  // two persistent 8-wave blocks per CU, a queue ticket of two whole tiles per block draw
  const int64_t blocks = persistent_blocks((n_dst + kQT - 1) / kQT, 2);
  constexpr int rq_ch = 2 * kQT;
  hipStream_t s = as_stream(stream);
  int ticket = -1;
  unsigned* rq = rowq_slot_for(n_dst, blocks, rq_ch, s, &ticket);
  const RawRel a{indptr_a, indices_a, ew_a, bias_a, bias_nonempty_a,
                 reduce_a == GNNREC_REDUCE_MEAN};
  const RawRel b{indptr_b, indices_b, ew_b, bias_b, bias_nonempty_b,
                 reduce_b == GNNREC_REDUCE_MEAN};
  const dim3 grid((unsigned)blocks), block(kQWaves * 64);
  dispatch_bool(ew_a != nullptr, [&](auto wa) {
    dispatch_bool(ew_b != nullptr, [&](auto wb) {
      hipLaunchKernelGGL((spmm_pair_mfma_kernel<decltype(wa)::value, decltype(wb)::value>), grid,
                         block, 0, s, a, b, X, ldx, H, ldh, WT4, n_dst, epilogue, combine,
                         attn_vec, out_div, out, ldo, rq, rq_ch);
    });
  });
  rowq_launched(ticket, s);
  return check_launch(name);
}
