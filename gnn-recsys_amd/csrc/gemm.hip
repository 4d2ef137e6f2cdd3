// a2/a3/a4 — fp32 MFMA GEMM with the SAGE epilogue fused in.
//
// Replaces (reference src/model.py):
//   fc_self(h_self) + fc_neigh(h_neigh), relu, zero-guarded row L2 norm   :98-99,226-235
//   relu(fc_preagg(h_neigh))                                              :102,151,158,185,198
//   NodeEmbedding (Linear + bias)                                         :19-24
//   PredictingLayer hidden_1 (bias)                                       :258
//   HeteroGraphConv(aggregate='sum'|'mean'|'max') across relations [DGL]  :384-406
//
// One launch computes, for a block of BM=128 rows and the full (padded) output
// width BN, acc = A1·W1ᵀ + T(A2)·W2ᵀ with v_mfma_f32_32x32x2_f32 (exact fp32,
// one rounding per product — no reduced-precision path exists for f32 on
// gfx950), then bias, activation, the row L2 norm (the whole row is in the
// block, reduced across the 32 lanes that hold it) and the cross-relation
// accumulate into `out`.
//
// Tiling, both kernels: 4 waves, each owning 32 rows × BN columns (BN/32
// accumulators of 16 regs), BN = 32, 64, 128 or 256 by the output width (256
// only where the row norm or the attention score needs the whole row in one
// block).  K is staged through LDS in tiles; lane half h of the MFMA consumes
// the h-th half of a tile's k, ascending, 4 at a time — a permutation of the
// summation order inside the tile that keeps both operand reads vectorised
// (fp32 sums stay within the 1e-4 parity tolerance).
//
//   gemm_f32_kernel      the general form: any alignment, any K.  Bounds-checked
//                        loads staged through registers into 32-deep tiles stored
//                        [row][k] with a 36-float row stride, so the per-lane
//                        ds_read_b128 of 4 consecutive k is bank-conflict free
//                        (r·36 mod 64 covers 16 distinct 4-bank slots).
//   gemm_f32_dma_kernel  16-B aligned operands, K1 and K2 multiples of the tile
//                        depth: global -> LDS DMA into unpadded, XOR-swizzled
//                        tiles, S stages, (A1,W1) and (A2,W2) as one stream of
//                        tiles.  Template over BN, the depth, S and a
//                        compile-time epilogue FE (-1: the run-time one).
//
// Dispatch (launch_gemm), first match:
//   BN 64 | 128, K % 16 == 0, aligned   -> dma<BN, 16, 3, FE>: FE = bias | relu << 1
//                                          | l2norm << 2 in {0, 1, 2, 3, 6, 7} for a
//                                          store-only, full-width (N == BN), aligned
//                                          output without sigmoid / bias_nonempty;
//                                          FE = -1 otherwise
//   BN 32 | 256, K % 32 == 0, aligned   -> dma<BN, 32, 2, -1>
//   anything else                       -> gemm_f32_kernel<BN>
#include "common.hpp"
#include <cmath>

namespace gnnrec {
namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int BM = 128;
constexpr int BK = 32;
constexpr int LDSK = 36;  // padded k stride (floats)
constexpr int GEMM_WAVES_PER_SIMD = 2;

struct GemmArgs {
  const float* A1; int64_t lda1; int64_t K1; const float* W1;
  const float* A2; int64_t lda2; int64_t K2; const float* W2;
  const int32_t* a2_deg; int a2_mode;
  const int64_t* a2_ip;  // GNNREC_A2_DEG_INDPTR: the degrees as indptr differences instead
  const float* bias;
  const float* bias_ne;  // added on rows with a2_deg > 0 (a folded NodeEmbedding's W_n b_e)
  int64_t M; int64_t N;
  int epilogue; int accum; float out_div;
  const float* attn_vec; float* attn_state;
  float* out; int64_t ldo;
  float* row_norm;  // nullable: |row| before the L2 norm (training keeps it for the backward)
  int vecA1, vecA2, vecW1, vecW2, vecO;
};

__device__ __forceinline__ int32_t a2_degree(const GemmArgs& g, int64_t row) {
  return g.a2_ip ? (int32_t)(g.a2_ip[row + 1] - g.a2_ip[row]) : g.a2_deg[row];
}

__device__ __forceinline__ f32x4 load4(const float* base, int64_t row, int64_t ld, int64_t k,
                                        int64_t K, bool rowok, bool vec) {
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
  if (!rowok || k >= K) return v;
  const float* p = base + row * ld + k;
  if (vec) {
    v = *reinterpret_cast<const f32x4*>(p);
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (k + j < K) v[j] = p[j];
  }
  return v;
}

// the epilogue stages the output tile in LDS in column halves, so the block's LDS
// is just the K-loop tiles (36.9 KB at BN=128) and LDS never limits occupancy
template <int BN>
constexpr int stage_cols() { return BN >= 64 ? BN / 2 : BN; }

template <int BN>
constexpr int smem_floats() {
  // K-loop tiles, or the epilogue's output staging + 2 attention factors per row
  return (BM + BN) * LDSK > BM * (stage_cols<BN>() + 4) + 2 * BM
             ? (BM + BN) * LDSK
             : BM * (stage_cols<BN>() + 4) + 2 * BM;
}

// Shared epilogue: bias, activation, zero-guarded row L2 norm, then the cross-relation
// accumulate into `out`, staged through LDS (column halves) into whole-row 16-B stores.
template <int BN>
__device__ __forceinline__ void gemm_epilogue(const GemmArgs& g, f32x16 (&acc)[BN / 32],
                                              float* smem, int64_t m0, int64_t n0, int wave,
                                              int lane) {
  constexpr int NT = BN / 32;
  const int r = lane & 31;
  const int h = lane >> 5;
  // ---- epilogue: C/D map of 32x32 MFMA: col = lane&31, row = (v&3) + 8(v>>2) + 4h
  const bool relu = g.epilogue & GNNREC_EPI_RELU;
  const bool sigm = g.epilogue & GNNREC_EPI_SIGMOID;
  const bool l2 = g.epilogue & GNNREC_EPI_L2NORM;
  float bias_t[NT], bne_t[NT];
  bool colok[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const int64_t col = n0 + t * 32 + r;
    colok[t] = col < g.N;
    bias_t[t] = (g.bias && colok[t]) ? g.bias[col] : 0.f;
    bne_t[t] = (g.bias_ne && colok[t]) ? g.bias_ne[col] : 0.f;
  }
  // staged store: the wave's 32 x BN tile goes through LDS (in column halves) and leaves
  // as whole rows of 16-B stores (4x fewer, fully coalesced store instructions)
  constexpr int SC = stage_cols<BN>();
  constexpr int OSTR = SC + 4;
  constexpr int TPR = SC / 32;  // accumulator tiles per staging round
  const bool attn = g.accum >= GNNREC_ACC_ATTN_FIRST;
  const bool staged = g.vecO;
  float* Ot = smem + wave * 32 * OSTR;
  float* Fa = smem + BM * OSTR + wave * 64;  // attention: (keep, norm) per staged row
  float z[16][NT];
  float a_t[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) a_t[t] = (attn && colok[t]) ? g.attn_vec[n0 + t * 32 + r] : 0.f;
  float keep[16], norm[16];  // attention: weight of the running out, 1 / running sum
#pragma unroll
  for (int v = 0; v < 16; ++v) {
    float ss = 0.f;
    bool ne = false;
    if (g.bias_ne) {
      const int64_t row = m0 + wave * 32 + (v & 3) + 8 * (v >> 2) + 4 * h;
      ne = row < g.M && a2_degree(g, row) > 0;
    }
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      float x = acc[t][v] + bias_t[t];
      if (ne) x += bne_t[t];
      if (relu) x = fmaxf(x, 0.f);
      if (sigm) x = 1.f / (1.f + expf(-x));
      if (!colok[t]) x = 0.f;
      z[v][t] = x;
      ss += x * x;
    }
    if (l2) {
#pragma unroll
      for (int off = 1; off < 32; off <<= 1) ss += __shfl_xor(ss, off);
      float nrm = sqrtf(ss);
      if (g.row_norm && r == 0) {
        const int64_t row = m0 + wave * 32 + (v & 3) + 8 * (v >> 2) + 4 * h;
        if (row < g.M) g.row_norm[row] = nrm;
      }
      if (nrm == 0.f) nrm = 1.f;
#pragma unroll
      for (int t = 0; t < NT; ++t) z[v][t] = z[v][t] / nrm;
    }
    keep[v] = 0.f;
    norm[v] = 1.f;
    if (attn) {  // online softmax over relations: score e = a . z(row)
      float e = 0.f;
#pragma unroll
      for (int t = 0; t < NT; ++t) e += z[v][t] * a_t[t];
#pragma unroll
      for (int off = 1; off < 32; off <<= 1) e += __shfl_xor(e, off);
      const int64_t row = m0 + wave * 32 + (v & 3) + 8 * (v >> 2) + 4 * h;
      float mnew = e, snew = 1.f, cnew = 1.f;
      if (row < g.M && g.accum != GNNREC_ACC_ATTN_FIRST) {
        const float2 st = reinterpret_cast<const float2*>(g.attn_state)[row];
        mnew = fmaxf(st.x, e);
        keep[v] = expf(st.x - mnew);
        cnew = expf(e - mnew);
        snew = st.y * keep[v] + cnew;
      }
      if (g.accum == GNNREC_ACC_ATTN_LAST) norm[v] = 1.f / snew;
      if (row < g.M && r == 0)
        reinterpret_cast<float2*>(g.attn_state)[row] = make_float2(mnew, snew);

#pragma unroll
      for (int t = 0; t < NT; ++t) z[v][t] *= cnew;
    }
  }
  if (!staged) {
#pragma unroll
    for (int v = 0; v < 16; ++v) {
      const int64_t row = m0 + wave * 32 + (v & 3) + 8 * (v >> 2) + 4 * h;
      if (row >= g.M) continue;
      float* orow = g.out + row * g.ldo + n0;
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        if (!colok[t]) continue;
        float* p = orow + t * 32 + r;
        float y = z[v][t];
        if (g.accum == GNNREC_ACC_ADD) y = *p + y;
        else if (g.accum == GNNREC_ACC_MAX) y = fmaxf(*p, y);
        else if (attn) {
          if (g.accum != GNNREC_ACC_ATTN_FIRST) y = *p * keep[v] + y;
          y = y * norm[v];
        }
        if (g.out_div > 0.f) y = y / g.out_div;
        *p = y;
      }
    }
    return;
  }
#pragma unroll
  for (int round = 0; round < NT / TPR; ++round) {
    __syncthreads();  // K-loop tiles (or the previous round) fully read
    if (attn && round == 0 && r == 0) {  // per-row factors for the store loop (Fa may
#pragma unroll                              // overlap the K-loop tiles: written after the barrier)
      for (int v = 0; v < 16; ++v) {
        const int rl = (v & 3) + 8 * (v >> 2) + 4 * h;
        Fa[2 * rl] = keep[v];
        Fa[2 * rl + 1] = norm[v];
      }
    }
#pragma unroll
    for (int v = 0; v < 16; ++v) {
      const int rl = (v & 3) + 8 * (v >> 2) + 4 * h;
#pragma unroll
      for (int tt = 0; tt < TPR; ++tt) Ot[rl * OSTR + tt * 32 + r] = z[v][round * TPR + tt];
    }
    __syncthreads();
    constexpr int C4 = SC / 4;               // float4 per staged row
    constexpr int ITER = 32 * C4 / kWave;    // float4 per lane
#pragma unroll 4
    for (int q = 0; q < ITER; ++q) {
      const int flat = q * kWave + lane;
      const int rl = flat / C4;
      const int c = (flat % C4) * 4;
      const int64_t row = m0 + wave * 32 + rl;
      const int64_t col = n0 + round * SC + c;
      if (row >= g.M || col >= g.N) continue;
      f32x4 y = *reinterpret_cast<const f32x4*>(Ot + rl * OSTR + c);
      f32x4* p = reinterpret_cast<f32x4*>(g.out + row * g.ldo + col);
      if (g.accum == GNNREC_ACC_ADD) {
        y = *p + y;
      } else if (g.accum == GNNREC_ACC_MAX) {
        const f32x4 o = *p;
#pragma unroll
        for (int j = 0; j < 4; ++j) y[j] = fmaxf(o[j], y[j]);
      } else if (attn) {
        if (g.accum != GNNREC_ACC_ATTN_FIRST) y = *p * Fa[2 * rl] + y;
        y = y * Fa[2 * rl + 1];
      }
      if (g.out_div > 0.f) y = y / g.out_div;
      *p = y;
    }
  }
}

// The common epilogues with their flags known at compile time — FE = bias | relu << 1 |
// l2norm << 2 (the SAGE projection: ReLU + row norm; fc_preagg: ReLU; NodeEmbedding: bias),
// store-only, full 128-column tiles, 16-B aligned output — instead of runtime flags in the
// unrolled value loops (selects per value: the 1M x 256 x 128 GEMM issued 4.8 non-MFMA VALU
// instructions per MFMA, profiles/r03_gemm_pmc.md).  The row norm divides once per row and
// scales by the reciprocal.
template <int BN, int FE>
__device__ __forceinline__ void gemm_epilogue_fast(const GemmArgs& g, f32x16 (&acc)[BN / 32],
                                                   float* smem, int64_t m0, int wave, int lane) {
  constexpr int NT = BN / 32;
  constexpr bool BIAS = FE & 1, RELU = FE & 2, L2 = FE & 4;
  const int r = lane & 31;
  const int h = lane >> 5;
  float bias_t[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) bias_t[t] = BIAS ? g.bias[t * 32 + r] : 0.f;
#pragma unroll
  for (int v = 0; v < 16; ++v) {
    float ss = 0.f;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      float x = acc[t][v];
      if constexpr (BIAS) x += bias_t[t];
      if constexpr (RELU) x = fmaxf(x, 0.f);
      acc[t][v] = x;
      if constexpr (L2) ss = fmaf(x, x, ss);
    }
    if constexpr (L2) {
#pragma unroll
      for (int off = 1; off < 32; off <<= 1) ss += __shfl_xor(ss, off);
      const float nrm = sqrtf(ss);
      if (g.row_norm && r == 0) {
        const int64_t row = m0 + wave * 32 + (v & 3) + 8 * (v >> 2) + 4 * h;
        if (row < g.M) g.row_norm[row] = nrm;
      }
      const float inv = 1.f / (nrm == 0.f ? 1.f : nrm);
#pragma unroll
      for (int t = 0; t < NT; ++t) acc[t][v] *= inv;
    }
  }
  constexpr int SC = stage_cols<BN>();
  constexpr int OSTR = SC + 4;
  constexpr int TPR = SC / 32;
  float* Ot = smem + wave * 32 * OSTR;
#pragma unroll
  for (int round = 0; round < NT / TPR; ++round) {
    __syncthreads();
#pragma unroll
    for (int v = 0; v < 16; ++v) {
      const int rl = (v & 3) + 8 * (v >> 2) + 4 * h;
#pragma unroll
      for (int tt = 0; tt < TPR; ++tt) Ot[rl * OSTR + tt * 32 + r] = acc[round * TPR + tt][v];
    }
    __syncthreads();
    constexpr int C4 = SC / 4;
    constexpr int ITER = 32 * C4 / kWave;
#pragma unroll
    for (int q = 0; q < ITER; ++q) {
      const int flat = q * kWave + lane;
      const int rl = flat / C4;
      const int c = (flat % C4) * 4;
      const int64_t row = m0 + wave * 32 + rl;
      if (row < g.M) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(Ot + rl * OSTR + c);
        f32x4* o = reinterpret_cast<f32x4*>(g.out + row * g.ldo + round * SC + c);
        *o = v;  // (non-temporal stores: +1 %, no store at all: the K loop still holds it —
                 // profiles/r04i_gemm_store_ab.md)
      }
    }
  }
}

// the general form (any alignment, any K): bounds-checked loads staged through registers;
// aligned operands with K a multiple of the tile depth take gemm_f32_dma_kernel
template <int BN>
__global__ __launch_bounds__(256, GEMM_WAVES_PER_SIMD) void gemm_f32_kernel(GemmArgs g) {
  __shared__ __attribute__((aligned(16))) float smem[smem_floats<BN>()];
  float* As = smem;
  float* Ws = smem + BM * LDSK;
  constexpr int NT = BN / 32;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int r = lane & 31;
  const int h = lane >> 5;
  const int64_t m0 = (int64_t)blockIdx.x * BM;
  const int64_t n0 = (int64_t)blockIdx.y * BN;

  f32x16 acc[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int v = 0; v < 16; ++v) acc[t][v] = 0.f;

  // rows / columns this thread stages (fixed for the whole kernel)
  bool arow_ok[4];
  int64_t arow[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int64_t gm = m0 + ((tid + i * 256) >> 3);
    arow_ok[i] = gm < g.M;
    arow[i] = arow_ok[i] ? gm : g.M - 1;
  }
  bool wrow_ok[NT];
  int64_t wrow[NT];
#pragma unroll
  for (int i = 0; i < NT; ++i) {
    const int64_t gn = n0 + ((tid + i * 256) >> 3);
    wrow_ok[i] = gn < g.N;
    wrow[i] = wrow_ok[i] ? gn : g.N - 1;
  }
  const int kc = (tid & 7) * 4;  // k offset of this thread's float4 inside a tile

#pragma unroll 1
  for (int seg = 0; seg < 2; ++seg) {
    const float* A = seg ? g.A2 : g.A1;
    const float* W = seg ? g.W2 : g.W1;
    const int64_t K = seg ? g.K2 : g.K1;
    const int64_t lda = seg ? g.lda2 : g.lda1;
    const bool vecA = seg ? g.vecA2 : g.vecA1;
    const bool vecW = seg ? g.vecW2 : g.vecW1;
    if (K == 0) continue;
    const int mode = seg ? g.a2_mode : GNNREC_A2_NONE;
    // per-row transform of the A rows this thread stages (uniform branch on `mode`)
    float rowdiv[4];
    bool rowzero[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      rowdiv[i] = 1.f;
      rowzero[i] = !arow_ok[i];
    }
    if (mode != GNNREC_A2_NONE) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int32_t dg = a2_degree(g, arow[i]);
        if (mode == GNNREC_A2_DIV_DEG) rowdiv[i] = (float)(dg > 0 ? dg : 1);
        else rowzero[i] = rowzero[i] || dg == 0;
      }
    }
    f32x4 ra[4], rw[NT];
    auto load_tile = [&](int64_t k0) {
#pragma unroll
      for (int i = 0; i < 4; ++i) ra[i] = load4(A, arow[i], lda, k0 + kc, K, true, vecA);
#pragma unroll
      for (int i = 0; i < NT; ++i) rw[i] = load4(W, wrow[i], K, k0 + kc, K, true, vecW);
    };
    load_tile(0);
#pragma unroll 1
    for (int64_t k0 = 0; k0 < K; k0 += BK) {
      __syncthreads();  // previous tile fully consumed
      const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
      if (mode == GNNREC_A2_DIV_DEG) {
#pragma unroll
        for (int i = 0; i < 4; ++i) ra[i] = ra[i] / rowdiv[i];
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int idx = tid + i * 256;
        *reinterpret_cast<f32x4*>(As + (idx >> 3) * LDSK + kc) = rowzero[i] ? zero : ra[i];
      }
#pragma unroll
      for (int i = 0; i < NT; ++i) {
        const int idx = tid + i * 256;
        *reinterpret_cast<f32x4*>(Ws + (idx >> 3) * LDSK + kc) = wrow_ok[i] ? rw[i] : zero;
      }
      __syncthreads();
      if (k0 + BK < K) load_tile(k0 + BK);
      const float* Ar = As + (wave * 32 + r) * LDSK + h * 16;
#pragma unroll
      for (int s4 = 0; s4 < 4; ++s4) {
        const f32x4 a = *reinterpret_cast<const f32x4*>(Ar + s4 * 4);
        f32x4 b[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t)
          b[t] = *reinterpret_cast<const f32x4*>(Ws + (t * 32 + r) * LDSK + h * 16 + s4 * 4);
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
          for (int t = 0; t < NT; ++t)
            acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[s], b[t][s], acc[t], 0, 0, 0);
      }
    }
  }

  gemm_epilogue<BN>(g, acc, smem, m0, n0, wave, lane);
}

// ---- the LDS-DMA kernel (aligned operands, K1/K2 multiples of the tile depth) -----------
// Tiles move global -> LDS with global_load_lds_dwordx4 (no staging registers) through S
// buffers: S-1 tiles are in flight while the MFMAs consume one; a counted `s_waitcnt vmcnt`
// + raw s_barrier publishes the oldest (a __syncthreads() would drain the DMA).  Two depths:
//   32 deep, S = 2: 32- and 256-column outputs.
//   16 deep, S = 3: 64- and 128-column outputs.  Half the LDS per stage, so three blocks
//     share a CU and one block's DMA prologue and store epilogue overlap the others' MFMAs,
//     which is where a K = 128..256 GEMM loses its time; and a 16-deep tile is only 2048
//     MFMA cycles per wave, shorter than an HBM round trip, so two tiles fly, not one (two
//     stages: MFMA busy ~56 % at M = 1M, K = 256, N = 128).
// The LDS image is lane-linear per wave-instruction (1 KiB = dma_rows rows of `depth` floats,
// unpadded), so bank conflicts are removed on the SOURCE side: 16-B chunk j of tile row R is
// stored at chunk j ^ ((R >> swz_shift) & swz_mask) of that row, which makes every 16-lane
// ds_read_b128 group of the fragment reads hit 16 distinct 4-bank slots.
constexpr int BK16 = 16;

constexpr int dma_rows(int depth) { return 256 / depth; }           // rows per 1-KiB DMA: 8 | 16
constexpr int swz_shift(int depth) { return depth == 32 ? 1 : 2; }
constexpr int swz_mask(int depth) { return depth / 4 - 1; }         // chunks per row - 1: 7 | 3
constexpr int k_steps(int depth) { return depth / 8; }              // 4-wide k-steps per lane half
constexpr int dma_instrs(int rows, int depth) { return rows * depth / 1024; }  // per wave, per tile
constexpr int tile_floats(int bn, int depth) { return (BM + bn) * depth; }
// k-steps whose fragments are requested from LDS before their MFMAs start.  16 deep: both, so
// the second step's LDS latency hides under the first step's MFMAs; 32 deep: one (four steps
// of a 256-column tile do not fit the register file).  Scheduling only: the k order is the same.
constexpr int frag_ahead(int depth) { return depth == 16 ? 2 : 1; }
// waves per SIMD the kernel is built for (blocks per CU): what the stages' LDS allows, and
// the 256-column accumulators' registers
constexpr int dma_waves(int bn, int depth) { return depth == 16 ? 3 : (bn > 128 ? 1 : 2); }
// The only arithmetic difference between the depths, kept so neither changes a result: the
// mean's 1/deg (GNNREC_A2_DIV_DEG) is one division per row and a multiply per operand at 16
// deep (64 IEEE divisions per lane per launch otherwise: half the VALU of the owned-row
// GEMM), and a division per operand at 32 deep.
constexpr bool deg_by_reciprocal(int depth) { return depth == 16; }

template <int BN, int DEPTH, int S>
constexpr int dma_smem_floats() {
  return S * tile_floats(BN, DEPTH) > smem_floats<BN>() ? S * tile_floats(BN, DEPTH)
                                                        : smem_floats<BN>();
}

// one 16-B-per-lane LDS-DMA (global_load_lds_dwordx4): lane L's bytes land at lds + 16 L.
// (Kept out of lambdas and host-invisible: a device builtin inside a kernel-template
// lambda makes hipcc drop the kernel's host launch stub.)
__device__ __forceinline__ void dma16(const float* src, float* lds) {
#if defined(__HIP_DEVICE_COMPILE__)
  __builtin_amdgcn_global_load_lds(src, (__attribute__((address_space(3))) void*)lds, 16, 0, 0);
#endif
}

template <int N>
__device__ __forceinline__ void wait_vmcnt_barrier() {
  static_assert(N >= 0 && N <= 63, "vmcnt immediate");
  asm volatile("s_waitcnt vmcnt(%0)\n\ts_barrier" ::"n"(N) : "memory");
}

// this wave's oldest tile landed while `ahead` (0..J) younger tiles of PER DMA instructions
// each may still fly; then all waves are past it
template <int PER, int J>
__device__ __forceinline__ void wait_oldest_tile(int ahead) {
  if constexpr (J == 0) {
    wait_vmcnt_barrier<0>();
  } else {
    if (ahead >= J) wait_vmcnt_barrier<J * PER>();
    else wait_oldest_tile<PER, J - 1>(ahead);
  }
}

template <int BN, int DEPTH, int S, int FE = -1>
__global__ __launch_bounds__(256, dma_waves(BN, DEPTH)) void gemm_f32_dma_kernel(GemmArgs g) {
  constexpr int NT = BN / 32;
  constexpr int AI = dma_instrs(BM, DEPTH);   // A-tile DMA instructions per wave
  constexpr int WI = dma_instrs(BN, DEPTH);   // W-tile DMA instructions per wave
  constexpr int TILE = tile_floats(BN, DEPTH);
  constexpr int ROWS = dma_rows(DEPTH), CPR = DEPTH / 4;  // rows per DMA, 16-B chunks per row
  constexpr int KS = k_steps(DEPTH), FA = frag_ahead(DEPTH);
  static_assert(DEPTH == 32 || DEPTH == 16, "tile depth");
  static_assert(WI >= 1 && S >= 2 && KS % FA == 0, "tile shape");
  static_assert(dma_waves(BN, DEPTH) * dma_smem_floats<BN, DEPTH, S>() * 4 <= 160 * 1024,
                "the blocks the launch bounds ask for do not fit the CU's LDS");
  __shared__ __attribute__((aligned(16))) float smem[dma_smem_floats<BN, DEPTH, S>()];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int r = lane & 31;
  const int h = lane >> 5;
  const int64_t m0 = (int64_t)blockIdx.x * BM;
  const int64_t n0 = (int64_t)blockIdx.y * BN;
  const int sw = (r >> swz_shift(DEPTH)) & swz_mask(DEPTH);  // read-side swizzle of this lane's rows

  f32x16 acc[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int v = 0; v < 16; ++v) acc[t][v] = 0.f;

  // this lane's DMA source pointers of both operand pairs, formed once (a tile adds k0): tile
  // row R = instr * ROWS + lane / CPR (clamped to the last row / column), physical chunk
  // lane % CPR
  const float* pa[2][AI];
  const float* pw[2][WI];
#pragma unroll
  for (int q = 0; q < AI; ++q) {
    const int R = (wave * AI + q) * ROWS + lane / CPR;
    const int64_t row = m0 + R < g.M ? m0 + R : g.M - 1;
    const int chk = ((lane % CPR) ^ ((R >> swz_shift(DEPTH)) & swz_mask(DEPTH))) * 4;
    pa[0][q] = g.A1 + row * g.lda1 + chk;
    pa[1][q] = g.K2 > 0 ? g.A2 + row * g.lda2 + chk : pa[0][q];
  }
#pragma unroll
  for (int q = 0; q < WI; ++q) {
    const int R = (wave * WI + q) * ROWS + lane / CPR;
    const int64_t row = n0 + R < g.N ? n0 + R : g.N - 1;
    const int chk = ((lane % CPR) ^ ((R >> swz_shift(DEPTH)) & swz_mask(DEPTH))) * 4;
    pw[0][q] = g.W1 + row * g.K1 + chk;
    pw[1][q] = g.K2 > 0 ? g.W2 + row * g.K2 + chk : pw[0][q];
  }

  // both operand pairs (A1,W1) then (A2,W2) as ONE stream of K tiles, so the DMA of the
  // first A2 tile overlaps the last A1 tile's MFMAs (no pipeline restart between segments)
  const int nk1 = (int)(g.K1 / DEPTH), nk = nk1 + (int)(g.K2 / DEPTH);
  const int64_t my_row = m0 + wave * 32 + r;  // the A row this lane's fragments come from
  float rowdeg2 = 1.f;  // the degree, or its reciprocal (deg_by_reciprocal)
  bool rowzero2 = false;
  if (g.K2 > 0 && g.a2_mode != GNNREC_A2_NONE) {
    const int32_t dg = a2_degree(g, my_row < g.M ? my_row : g.M - 1);
    if (g.a2_mode == GNNREC_A2_DIV_DEG) {
      rowdeg2 = (float)(dg > 0 ? dg : 1);
      if constexpr (deg_by_reciprocal(DEPTH)) rowdeg2 = 1.f / rowdeg2;
    } else {
      rowzero2 = dg == 0;
    }
  }
  auto issue = [&](int kt, int buf) {
    const int s2 = kt >= nk1;
    const int k0 = (s2 ? kt - nk1 : kt) * DEPTH;
    float* base = smem + buf * TILE;
#pragma unroll
    for (int q = 0; q < AI; ++q) dma16(pa[s2][q] + k0, base + (wave * AI + q) * 256);
#pragma unroll
    for (int q = 0; q < WI; ++q) dma16(pw[s2][q] + k0, base + BM * DEPTH + (wave * WI + q) * 256);
  };
#pragma unroll
  for (int j = 0; j < S - 1; ++j)
    if (j < nk) issue(j, j);
#pragma unroll 1
  for (int kt = 0; kt < nk; ++kt) {
    const int buf = kt % S;
    if (kt + S - 1 < nk) issue(kt + S - 1, (kt + S - 1) % S);
    wait_oldest_tile<AI + WI, S - 1>(nk - 1 - kt);
    const bool s2 = kt >= nk1;
    const bool divide = s2 && g.a2_mode == GNNREC_A2_DIV_DEG;
    const bool zero = s2 && rowzero2;
    const float* As = smem + buf * TILE + (wave * 32 + r) * DEPTH;
    const float* Ws = smem + buf * TILE + BM * DEPTH + r * DEPTH;
    // lane half h consumes k in [h DEPTH/2, (h+1) DEPTH/2) of the tile, ascending, 4 at a time
#pragma unroll
    for (int s0 = 0; s0 < KS; s0 += FA) {
      f32x4 a[FA], b[FA][NT];
#pragma unroll
      for (int j = 0; j < FA; ++j) {
        const int pc = ((h * KS + s0 + j) ^ sw) * 4;
        a[j] = *reinterpret_cast<const f32x4*>(As + pc);
#pragma unroll
        for (int t = 0; t < NT; ++t)
          b[j][t] = *reinterpret_cast<const f32x4*>(Ws + t * 32 * DEPTH + pc);
      }
#pragma unroll
      for (int j = 0; j < FA; ++j) {
        if (divide) {
          if constexpr (deg_by_reciprocal(DEPTH)) a[j] = a[j] * rowdeg2;
          else a[j] = a[j] / rowdeg2;
        } else if (zero) {
          a[j] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
          for (int t = 0; t < NT; ++t)
            acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[j][s], b[j][t][s], acc[t], 0, 0, 0);
      }
    }
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");  // buffer free for reuse
  }
  if constexpr (FE >= 0) gemm_epilogue_fast<BN, FE>(g, acc, smem, m0, wave, lane);
  else gemm_epilogue<BN>(g, acc, smem, m0, n0, wave, lane);
}

template <int BN>
int launch_gemm(const GemmArgs& g, hipStream_t s) {
  dim3 grid((unsigned)((g.M + BM - 1) / BM), (unsigned)((g.N + BN - 1) / BN));
  const bool fast = g.vecA1 && g.vecW1 && g.K1 % BK == 0 &&
                    (g.K2 == 0 || (g.vecA2 && g.vecW2 && g.K2 % BK == 0));
  // 16-deep K tiles, three stages (three blocks per CU) for 128- and 64-column outputs:
  // +5-10 % at K = 128..256 (tools/bench_gemm_k.py; the d = 64 minibatch layers overlap one
  // block's DMA prologue and epilogue with the other blocks' MFMAs), and the compile-time
  // epilogue (gemm_epilogue_fast) for the common flag sets (profiles/r03_gemm_experiments.md)
  if constexpr (BN == 128 || BN == 64) {
    const bool fast16 = g.vecA1 && g.vecW1 && g.K1 % BK16 == 0 &&
                        (g.K2 == 0 || (g.vecA2 && g.vecW2 && g.K2 % BK16 == 0));
    if (fast16) {
      const bool sig = g.epilogue & GNNREC_EPI_SIGMOID;
      const int fe = (g.bias ? 1 : 0) | ((g.epilogue & GNNREC_EPI_RELU) ? 2 : 0) |
                     ((g.epilogue & GNNREC_EPI_L2NORM) ? 4 : 0);
      if (!sig && g.accum == GNNREC_ACC_STORE && !g.bias_ne && g.N == BN && g.vecO &&
          (g.row_norm == nullptr || (fe & 4))) {
        switch (fe) {
          case 0: hipLaunchKernelGGL((gemm_f32_dma_kernel<BN, BK16, 3, 0>), grid, dim3(256), 0, s, g); break;
          case 1: hipLaunchKernelGGL((gemm_f32_dma_kernel<BN, BK16, 3, 1>), grid, dim3(256), 0, s, g); break;
          case 2: hipLaunchKernelGGL((gemm_f32_dma_kernel<BN, BK16, 3, 2>), grid, dim3(256), 0, s, g); break;
          case 3: hipLaunchKernelGGL((gemm_f32_dma_kernel<BN, BK16, 3, 3>), grid, dim3(256), 0, s, g); break;
          case 6: hipLaunchKernelGGL((gemm_f32_dma_kernel<BN, BK16, 3, 6>), grid, dim3(256), 0, s, g); break;
          case 7: hipLaunchKernelGGL((gemm_f32_dma_kernel<BN, BK16, 3, 7>), grid, dim3(256), 0, s, g); break;
          default: hipLaunchKernelGGL((gemm_f32_dma_kernel<BN, BK16, 3>), grid, dim3(256), 0, s, g);
        }
        return check_launch("gnnrec_gemm_f32");
      }
      hipLaunchKernelGGL((gemm_f32_dma_kernel<BN, BK16, 3>), grid, dim3(256), 0, s, g);
      return check_launch("gnnrec_gemm_f32");
    }
  } else {
    // (at 64 and 128 columns `fast` implies `fast16`, which has returned: no 32-deep
    // instantiation exists for them)
    if (fast) {
      hipLaunchKernelGGL((gemm_f32_dma_kernel<BN, BK, 2>), grid, dim3(256), 0, s, g);
      return check_launch("gnnrec_gemm_f32");
    }
  }
  hipLaunchKernelGGL((gemm_f32_kernel<BN>), grid, dim3(256), 0, s, g);
  return check_launch("gnnrec_gemm_f32");
}

}  // namespace
}  // namespace gnnrec

extern "C" int gnnrec_gemm_f32(const float* A1, int64_t lda1, int64_t K1, const float* W1,
                               const float* A2, int64_t lda2, int64_t K2, const float* W2,
                               const int32_t* a2_deg, int a2_mode, const float* bias,
                               const float* bias_nonempty, int64_t M,
                               int64_t N, int epilogue, int accum, float out_div,
                               const float* attn_vec, float* attn_state, float* out,
                               int64_t ldo, void* stream) {
  return gnnrec_gemm_rownorm_f32(A1, lda1, K1, W1, A2, lda2, K2, W2, a2_deg, a2_mode, bias,
                                 bias_nonempty, M, N, epilogue, accum, out_div, attn_vec,
                                 attn_state, out, ldo, nullptr, stream);
}

extern "C" int gnnrec_gemm_rownorm_f32(const float* A1, int64_t lda1, int64_t K1,
                                       const float* W1, const float* A2, int64_t lda2,
                                       int64_t K2, const float* W2, const int32_t* a2_deg,
                                       int a2_mode, const float* bias,
                                       const float* bias_nonempty, int64_t M, int64_t N,
                                       int epilogue, int accum, float out_div,
                                       const float* attn_vec, float* attn_state, float* out,
                                       int64_t ldo, float* row_norm, void* stream) {
  using namespace gnnrec;
  GNNREC_REQUIRE(row_norm == nullptr || (epilogue & GNNREC_EPI_L2NORM),
                 "gnnrec_gemm_rownorm_f32: row_norm needs the L2NORM epilogue");
  GNNREC_REQUIRE(M >= 0 && N >= 0 && K1 >= 0 && K2 >= 0, "gnnrec_gemm_f32: negative size");
  if (M == 0 || N == 0) return GNNREC_OK;
  GNNREC_REQUIRE(out != nullptr && ldo >= N, "gnnrec_gemm_f32: bad output");
  GNNREC_REQUIRE(K1 == 0 || (A1 && W1 && lda1 >= K1), "gnnrec_gemm_f32: bad A1/W1");
  GNNREC_REQUIRE(K2 == 0 || (A2 && W2 && lda2 >= K2), "gnnrec_gemm_f32: bad A2/W2");
  // GNNREC_A2_DEG_INDPTR: a2_deg is an int64 indptr [M + 1] (a block CSR's: no degree array
  // to build first)
  const bool deg_ip = (a2_mode & GNNREC_A2_DEG_INDPTR) != 0;
  a2_mode &= ~GNNREC_A2_DEG_INDPTR;
  GNNREC_REQUIRE(a2_mode == GNNREC_A2_NONE || a2_deg != nullptr,
                 "gnnrec_gemm_f32: a2_mode needs a2_deg");
  GNNREC_REQUIRE(bias_nonempty == nullptr || a2_deg != nullptr,
                 "gnnrec_gemm_f32: bias_nonempty needs a2_deg");
  GNNREC_REQUIRE(accum >= GNNREC_ACC_STORE && accum <= GNNREC_ACC_ATTN_LAST,
                 "gnnrec_gemm_f32: unknown accumulate mode %d", accum);
  const bool attn = accum >= GNNREC_ACC_ATTN_FIRST;
  GNNREC_REQUIRE(!attn || (attn_vec && attn_state && N <= 256),
                 "gnnrec_gemm_f32: attention accumulation needs attn_vec, attn_state, N <= 256");
  GNNREC_REQUIRE(!(epilogue & GNNREC_EPI_L2NORM) || N <= 256,
                 "gnnrec_gemm_f32: L2NORM needs N <= 256 (got %lld)", (long long)N);
  GemmArgs g;
  g.A1 = A1; g.lda1 = lda1; g.K1 = K1; g.W1 = W1;
  g.A2 = A2; g.lda2 = lda2; g.K2 = K2; g.W2 = W2;
  g.a2_deg = deg_ip ? nullptr : a2_deg;
  g.a2_ip = deg_ip ? reinterpret_cast<const int64_t*>(a2_deg) : nullptr;
  g.a2_mode = a2_mode; g.bias = bias; g.bias_ne = bias_nonempty;
  g.M = M; g.N = N; g.epilogue = epilogue; g.accum = accum; g.out_div = out_div;
  g.attn_vec = attn_vec; g.attn_state = attn_state;
  g.out = out; g.ldo = ldo;
  g.row_norm = row_norm;
  g.vecA1 = (K1 % 4 == 0) && (lda1 % 4 == 0) && aligned16(A1);
  g.vecA2 = (K2 % 4 == 0) && (lda2 % 4 == 0) && aligned16(A2);
  g.vecW1 = (K1 % 4 == 0) && aligned16(W1);
  g.vecW2 = (K2 % 4 == 0) && aligned16(W2);
  g.vecO = (N % 4 == 0) && (ldo % 4 == 0) && aligned16(out);
  hipStream_t s = as_stream(stream);
  if (N <= 32) return launch_gemm<32>(g, s);
  if (N <= 64) return launch_gemm<64>(g, s);
  if (N <= 128) return launch_gemm<128>(g, s);
  // wider outputs: 128-column blocks (two waves per SIMD) unless the row norm needs the
  // whole row in one block (the 256-column tile runs at one wave per SIMD)
  if (!(epilogue & GNNREC_EPI_L2NORM) && !attn) return launch_gemm<128>(g, s);
  return launch_gemm<256>(g, s);
}
