// a7/a8 — edge-score heads.
//
// a7 CosinePrediction (reference src/model.py:317-327): per canonical etype
//    F.normalize(h, p=2, dim=-1, eps=1e-12) on both endpoint tables, then
//    DGL apply_edges(fn.u_dot_v).  Fused here into one pass over the edges:
//    each edge reads its two rows once, and the dot product and both squared
//    norms are reduced together (no normalised copy of either table is
//    materialised).  out = dot / (max(|u|,eps) · max(|v|,eps)).
//
// a8 PredictingModule/PredictingLayer (reference src/model.py:290-305,
//    256-271): σ(w3·relu(W2·relu(W1[h_u‖h_v]+b1)+b2)+b3).  W1[h_u‖h_v] is
//    re-associated into P[u] + Q[v] with P = H_src·W1aᵀ + b1, Q = H_dst·W1bᵀ
//    computed once per node by gnnrec_gemm_f32, so the per-edge work is a
//    128-wide gather-add + ReLU feeding a [E×128]·[128×32] MFMA product, then
//    a 32-wide dot and the sigmoid — the [E, 2d] concatenation of the
//    reference is never built.
#include "common.hpp"
#include "cos_score.hpp"
#include "fold_i32.hpp"
#include "rating.hpp"
#include <cmath>

namespace gnnrec {
namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

// ---------------------------------------------------------------- cosine ----
// dot4 and group_sum_last, the lane arithmetic every cosine kernel shares: cos_score.hpp
template <int LPR, int VEC>
__global__ __launch_bounds__(256) void sddmm_cos_kernel(const int64_t* __restrict__ src,
                                                        const int64_t* __restrict__ dst,
                                                        int64_t n_edges,
                                                        const float* __restrict__ Hs, int64_t lds,
                                                        const float* __restrict__ Hd, int64_t ldd,
                                                        int d, float* __restrict__ out) {
  constexpr int NPW = kWave / LPR;  // edges per wave per step
  const int lane = threadIdx.x & 63;
  const int grp = lane / LPR;
  const int gl = lane % LPR;
  const int64_t wstride = (int64_t)gridDim.x * 4 * NPW;
  for (int64_t e0 = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * NPW; e0 < n_edges;
       e0 += wstride) {
    const int64_t e = e0 + grp;
    const bool eok = e < n_edges;
    float dot = 0.f, su = 0.f, sv = 0.f;
    if (eok) {
      const float* pu = Hs + src[e] * lds;
      const float* pv = Hd + dst[e] * ldd;
      for (int c = gl * VEC; c < d; c += LPR * VEC) {
        if constexpr (VEC == 4) {
          const float4 a = *reinterpret_cast<const float4*>(pu + c);
          const float4 b = *reinterpret_cast<const float4*>(pv + c);
          dot += dot4(a, b);
          su += dot4(a, a);
          sv += dot4(b, b);
        } else {
          const float a = pu[c], b = pv[c];
          dot += a * b;
          su += a * a;
          sv += b * b;
        }
      }
    }
    dot = group_sum_last<LPR>(dot);
    su = group_sum_last<LPR>(su);
    sv = group_sum_last<LPR>(sv);
    if (eok && gl == LPR - 1) {
      const float nu = fmaxf(sqrtf(su), 1e-12f);
      const float nv = fmaxf(sqrtf(sv), 1e-12f);
      out[e] = dot / (nu * nv);
    }
  }
}

template <int LPR, int VEC>
int launch_cos(const int64_t* src, const int64_t* dst, int64_t n, const float* Hs, int64_t lds,
               const float* Hd, int64_t ldd, int d, float* out, hipStream_t s) {
  constexpr int NPW = kWave / LPR;
  int64_t blocks = (n + 4 * NPW - 1) / (4 * NPW);
  if (blocks > 256 * 32) blocks = 256 * 32;
  if (blocks < 1) blocks = 1;
  hipLaunchKernelGGL((sddmm_cos_kernel<LPR, VEC>), dim3((unsigned)blocks), dim3(256), 0, s, src,
                     dst, n, Hs, lds, Hd, ldd, d, out);
  return check_launch("gnnrec_sddmm_cos_f32");
}

// ------------------------------------------------------- grouped cosine ----
// The training pair graphs of EdgeDataLoader + negative_sampler.Uniform(K) (reference
// src/sampling.py:163-165: neg src = pos src repeated K times, dst uniform): group g is one
// positive edge (u_g, first[g]) and its K negatives (u_g, dst[g K + j]).  A wave takes a
// chunk of one group's negatives and keeps h_u — its fragment in registers, its norm
// reduced once — so every edge reads one gathered row (4d B) and its dst id, not two rows and
// two ids, and the u norm is not recomputed K times.  Each value is formed exactly as
// sddmm_cos_kernel forms it (same lane fragments, same reduction tree, same final expression):
// the scores are bitwise those of the per-edge kernel.
constexpr int kCosU = 16;      // edges in flight per lane group
constexpr int kCosChunk = 64;  // negatives per wave (40 waves per group at K = 2500: the
                               // grid ends in a short tail; 256 per wave left a 25 % round)

template <int LPR>
__global__ __launch_bounds__(256) void sddmm_cos_grouped_kernel(
    const int64_t* __restrict__ src_g, int64_t n_groups, const int64_t* __restrict__ first,
    float* __restrict__ out_first, int64_t K, int64_t chunks, const int64_t* __restrict__ dst,
    float* __restrict__ out, const float* __restrict__ Hs, int64_t lds,
    const float* __restrict__ Hd, int64_t ldd, int d) {
  constexpr int NPW = kWave / LPR;   // edges per wave-instruction
  constexpr int STEP = NPW * kCosU;  // edges per step (<= 64: one id per lane)
  static_assert(kCosChunk <= 64 && kCosChunk % STEP == 0, "a chunk's ids fit one wave load");
  const int lane = threadIdx.x & 63;
  const int grp = lane / LPR;
  const int gl = lane % LPR;
  const int64_t task = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (task >= n_groups * chunks) return;  // wave-uniform
  const int64_t g = task / chunks, c = task - g * chunks;
  const int col = gl * 4;
  const bool cok = col < d;
  float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
  float su = 0.f;
  if (cok) {
    a = *reinterpret_cast<const float4*>(Hs + src_g[g] * lds + col);
    su += dot4(a, a);
  }
#pragma unroll
  for (int off = 1; off < LPR; off <<= 1) su += __shfl_xor(su, off);
  const float nu = fmaxf(sqrtf(su), 1e-12f);
  auto score = [&](const float4& b, bool ok) {  // -> the cosine on lane gl == 0 of the group
    float dot = 0.f, sv = 0.f;
    if (ok) {
      dot += dot4(a, b);
      sv += dot4(b, b);
    }
    dot = group_sum_last<LPR>(dot);
    sv = group_sum_last<LPR>(sv);
    const float nv = fmaxf(sqrtf(sv), 1e-12f);
    return dot / (nu * nv);  // (valid in the group's last lane)
  };
  if (c == 0 && first != nullptr) {  // the group's positive edge
    const int64_t v = first[g];
    float4 b = make_float4(0.f, 0.f, 0.f, 0.f);
    if (cok) b = *reinterpret_cast<const float4*>(Hd + v * ldd + col);
    const float r = score(b, cok);
    if (lane == LPR - 1) out_first[g] = r;
  }
  const int64_t e_beg = g * K + c * kCosChunk;
  const int64_t e_end = g * K + min<int64_t>(K, (c + 1) * kCosChunk);
  // the chunk's ids in one coalesced load (lane l: the chunk's l-th edge; row ids < 2^31)
  const int all_ids = e_beg + lane < e_end ? (int)dst[e_beg + lane] : 0;
  for (int64_t e0 = e_beg; e0 < e_end; e0 += STEP) {
    const int id = STEP == kCosChunk ? all_ids : __shfl(all_ids, (int)(e0 - e_beg) + lane);
    float4 b[kCosU];
#pragma unroll
    for (int k = 0; k < kCosU; ++k) {
      const int slot = k * NPW + grp;
      const int64_t v = bcast_groups<NPW>(id, k * NPW, grp);
      b[k] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (cok && e0 + slot < e_end) b[k] = *reinterpret_cast<const float4*>(Hd + v * ldd + col);
    }
#pragma unroll
    for (int k = 0; k < kCosU; ++k) {
      const int64_t e = e0 + k * NPW + grp;
      const float r = score(b[k], cok && e < e_end);
      if (gl == LPR - 1 && e < e_end) out[e] = r;
    }
  }
}

template <int LPR>
int launch_cos_grouped(const int64_t* src_g, int64_t G, const int64_t* first, float* out_first,
                       int64_t K, const int64_t* dst, float* out, const float* Hs, int64_t lds,
                       const float* Hd, int64_t ldd, int d, hipStream_t s) {
  const int64_t chunks = K > 0 ? (K + kCosChunk - 1) / kCosChunk : 1;
  const int64_t waves = G * chunks;
  hipLaunchKernelGGL(sddmm_cos_grouped_kernel<LPR>, dim3((unsigned)((waves + 3) / 4)), dim3(256),
                     0, s, src_g, G, first, out_first, K, chunks, dst, out, Hs, lds, Hd, ldd, d);
  return check_launch("gnnrec_sddmm_cos_grouped_f32");
}

// ------------------------------------------------------------- edge MLP ----
// A[i][k] = relu(P[src_i][k] + Q[dst_i][k]) (k < 128) feeds the 128x32 layer on the MFMA,
// then relu(+b2) . w3 and the sigmoid; hidden sizes 128 and 32 (src/model.py:258-260).

// One wave scores tiles of 32 edges: the tile's hidden-1 activations
// A[i][k] = relu(P[u_i][k] + Q[v_i][k]) are built from coalesced row loads (two 512-B rows
// of P and of Q per wave-instruction, each row's 32 16-B chunks in one lane half) and
// stored to the wave's LDS image with row i's chunk j at position j ^ (i & 15), so that the
// MFMA-layout reads (lane r reads row r) meet 16 distinct 4-bank groups per lane group.
// (Per-lane row loads in the MFMA layout — lane r reading its own edge's rows — touch 32
// rows per wave-instruction and each row's 128-B lines again from eight instructions:
// 0.37 ms against 0.27 ms at 2.56M edges, tools/micro/edge_mlp_ab.py.)  The 128x32 layer runs transposed, C^T = W2 A^T: W2 as the A operand
// (lane r holds hidden-2 unit r's row, in registers for the wave's life) and the staged A
// as the B operand (lane r = edge r), so lane (r, h) ends with 16 of edge r's 32 hidden-2
// units: the output dot is an in-register sum and one add across the lane halves.
// GROUPED: the edges are n_groups runs of one source (negative_sampler.Uniform's negatives:
// group g = optionally its positive (g, first[g]) then its K negatives (g, dst[g K + j])).
constexpr int kMlpTile = 32;        // edges per MFMA tile
constexpr int kMlpChunkTiles = 8;   // tiles per work item, at most
constexpr int kMlpWaves = 4;        // waves per 256-thread block, each with its own image
constexpr int kMlpResidentWaves = 2 * 256 * kMlpWaves;  // two blocks per CU (registers)

struct EdgeMlpArgs {
  const int64_t* src;    // per edge; GROUPED: per group
  const int64_t* dst;    // per edge; GROUPED: [n_groups x K] negatives
  const int64_t* first;  // GROUPED: per-group positive destination, or null
  float* out_first;
  float* out;
  const float* P;
  const float* Q;
  const float* W2;
  const float* b2;
  const float* w3;
  const float* b3;
  int64_t n_edges;       // ungrouped edge count
  int64_t K;             // GROUPED: negatives per group
  int64_t per_group;     // GROUPED: K + (first != null)
  int64_t chunks;        // GROUPED: work items per group
  int64_t n_items;
  int64_t chunk_tiles;   // tiles per work item
};

// A tile's 32 edges: lane r's destination row (and source row, per-edge form); -1 past the
// end.  Both lane halves hold the same ids.
template <bool GROUPED>
__device__ __forceinline__ void mlp_tile_ids(const EdgeMlpArgs& a, int64_t g, int64_t e,
                                             int64_t e_end, int64_t lead, int& v, int& u) {
  v = -1;
  if (e >= e_end) return;
  if constexpr (GROUPED) {
    v = (int)(e < lead ? a.first[g] : a.dst[g * a.K + e - lead]);
  } else {
    v = (int)a.dst[e];
    u = (int)a.src[e];
  }
}

// Row loads of a tile, wave-instruction i = rows 2 i + h (lane half h), chunk r ^ (row & 15):
// GROUPED the Q chunks of rows i in [i0, i0 + N); per edge the (Q, P) chunk pairs.
template <bool GROUPED, int N>
__device__ __forceinline__ void mlp_load(const float4* __restrict__ Q4,
                                         const float4* __restrict__ P4, int v, int u, int r,
                                         int h, int i0, float4 (&q)[N], float4 (&p)[N]) {
#pragma unroll
  for (int i = 0; i < N; ++i) {
    const int row = 2 * (i0 + i) + h;
    const int vr = bcast_groups<2>(v, 2 * (i0 + i), h);
    const int ur = GROUPED ? 0 : bcast_groups<2>(u, 2 * (i0 + i), h);
    const int j = r ^ (row & 15);
    q[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    if constexpr (!GROUPED) p[i] = q[i];
    if (vr >= 0) {
      q[i] = Q4[(int64_t)vr * 32 + j];
      if constexpr (!GROUPED) p[i] = P4[(int64_t)ur * 32 + j];
    }
  }
}

__device__ __forceinline__ float4 relu_add4(const float4& p, const float4& q) {
  return make_float4(fmaxf(p.x + q.x, 0.f), fmaxf(p.y + q.y, 0.f), fmaxf(p.z + q.z, 0.f),
                     fmaxf(p.w + q.w, 0.f));
}

// The 128x32 layer of one staged tile (C^T = W2 A^T) and the output: sigmoid(w3 . relu(. + b2)
// + b3) of edge r, stored by lane r of the first half.  RELU_P: the image holds Q rows only,
// A = relu(P + Q) formed here with the source's P chunks pc (16 h + c).
template <bool RELU_P>
__device__ __forceinline__ float mlp_tile_score(const EdgeMlpArgs& a, const float4* S,
                                                const float4 (&w)[16], const float4* pc, int r,
                                                int h, float b3v) {
  f32x16 acc;
#pragma unroll
  for (int q = 0; q < 16; ++q) acc[q] = 0.f;
#pragma unroll
  for (int c = 0; c < 16; ++c) {
    float4 x = S[r * 32 + ((16 * h + c) ^ (r & 15))];
    if constexpr (RELU_P) x = relu_add4(pc[c], x);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(w[c].x, x.x, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(w[c].y, x.y, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(w[c].z, x.z, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(w[c].w, x.w, acc, 0, 0, 0);
  }
  // acc[q]: hidden-2 unit 8 (q >> 2) + 4 h + (q & 3) of edge r
  float y = 0.f;
#pragma unroll
  for (int q = 0; q < 16; ++q) {
    const int jj = 8 * (q >> 2) + 4 * h + (q & 3);
    y = fmaf(fmaxf(acc[q] + a.b2[jj], 0.f), a.w3[jj], y);
  }
  y += __shfl_xor(y, 32);
  return 1.f / (1.f + expf(-(y + b3v)));
}

__device__ __forceinline__ void mlp_store(const EdgeMlpArgs& a, bool grouped, int64_t g,
                                          int64_t e, int64_t lead, float sc) {
  if (!grouped) a.out[e] = sc;
  else if (e < lead) a.out_first[g] = sc;
  else a.out[g * a.K + e - lead] = sc;
}

__device__ __forceinline__ void mlp_load_w2(const EdgeMlpArgs& a, int r, int h, float4 (&w)[16]) {
  const float4* W4 = reinterpret_cast<const float4*>(a.W2) + r * 32 + 16 * h;
#pragma unroll
  for (int c = 0; c < 16; ++c) w[c] = W4[c];  // W2 row r, chunks 16 h + c: k = 64 h + 4 c + s
}

// work item -> (group, tiles [t0, t1), edge end)
template <bool GROUPED>
__device__ __forceinline__ void mlp_item(const EdgeMlpArgs& a, int64_t item, int64_t tiles_pg,
                                         int64_t& g, int64_t& t0, int64_t& t1, int64_t& e_end) {
  if constexpr (GROUPED) {
    g = item / a.chunks;
    t0 = (item - g * a.chunks) * a.chunk_tiles;
    t1 = t0 + a.chunk_tiles < tiles_pg ? t0 + a.chunk_tiles : tiles_pg;
    e_end = a.per_group;
  } else {
    g = 0;
    t0 = item * a.chunk_tiles;
    t1 = t0 + a.chunk_tiles;
    e_end = a.n_edges;
  }
}

template <bool GROUPED>
__global__ __launch_bounds__(256, 2) void edge_mlp_lds_kernel(EdgeMlpArgs a) {
  __shared__ float4 image[kMlpWaves][kMlpTile * 32];  // 16 KB per wave
  const int lane = threadIdx.x & 63;
  const int wv = threadIdx.x >> 6;
  const int r = lane & 31;
  const int h = lane >> 5;
  float4* S = image[wv];
  const float4* P4 = reinterpret_cast<const float4*>(a.P);
  const float4* Q4 = reinterpret_cast<const float4*>(a.Q);
  float4 w[16];
  mlp_load_w2(a, r, h, w);
  const float b3v = a.b3[0];
  const int64_t tiles_pg = GROUPED ? (a.per_group + kMlpTile - 1) / kMlpTile : 0;
  const int64_t lead = (GROUPED && a.first) ? 1 : 0;
  for (int64_t item = (int64_t)blockIdx.x * kMlpWaves + wv; item < a.n_items;
       item += (int64_t)gridDim.x * kMlpWaves) {
    int64_t g, t0, t1, e_end;
    mlp_item<GROUPED>(a, item, tiles_pg, g, t0, t1, e_end);
    const int u_g = GROUPED ? (int)a.src[g] : 0;
    // GROUPED: the source's P chunks this lane adds, r ^ (row & 15) for the 16 row
    // residues of one lane half (rows 2 i + h, i < 8, then the same residues again)
    float4 pg[8];
    if constexpr (GROUPED) {
#pragma unroll
      for (int i = 0; i < 8; ++i) pg[i] = P4[(int64_t)u_g * 32 + (r ^ ((2 * i + h) & 15))];
    }
    for (int64_t t = t0; t < t1; ++t) {
      const int64_t e = t * kMlpTile + r;  // this lane's edge (both halves)
      int v, u = u_g;
      mlp_tile_ids<GROUPED>(a, g, e, e_end, lead, v, u);
      // stage, eight row pairs at a time
#pragma unroll
      for (int half = 0; half < 2; ++half) {
        float4 q[8], p[8];
        mlp_load<GROUPED, 8>(Q4, P4, v, u, r, h, 8 * half, q, p);
#pragma unroll
        for (int i = 0; i < 8; ++i)
          S[(2 * (8 * half + i) + h) * 32 + r] = relu_add4(GROUPED ? pg[i] : p[i], q[i]);
      }
      // (the wave's own LDS writes precede its reads in issue order)
      const float sc = mlp_tile_score<false>(a, S, w, nullptr, r, h, b3v);
      if (h == 0 && e < e_end) mlp_store(a, GROUPED, g, e, lead, sc);
    }
  }
}

// tiles per work item: up to kMlpChunkTiles (the wave's W2 / P registers reused), fewer when
// the launch would otherwise leave resident waves idle
int64_t mlp_chunk_tiles(int64_t tiles) {
  int64_t c = (tiles + kMlpResidentWaves - 1) / kMlpResidentWaves;
  return c < 1 ? 1 : (c > kMlpChunkTiles ? kMlpChunkTiles : c);
}

int launch_edge_mlp_lds(bool grouped, EdgeMlpArgs& a, hipStream_t s) {
  if (a.n_items <= 0) return GNNREC_OK;
  int64_t blocks = (a.n_items + kMlpWaves - 1) / kMlpWaves;
  if (blocks > kMlpResidentWaves / kMlpWaves) blocks = kMlpResidentWaves / kMlpWaves;
  if (grouped)
    hipLaunchKernelGGL(edge_mlp_lds_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, s, a);
  else
    hipLaunchKernelGGL(edge_mlp_lds_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, s, a);
  return check_launch(grouped ? "gnnrec_edge_mlp_grouped_f32" : "gnnrec_edge_mlp_f32");
}

// ------------------------------------------------------- dense edge MLP ----
// Every (user, item) pair of a user batch and an item range, without id arrays: the item of
// a tile lane is the tile's base plus the lane.  A work item is (item tile, user group): the
// wave stages the tile's 32 Q rows in its LDS image once (raw, no P added) and scores it for
// the group's users (at most kDenseUsers) in turn with mlp_tile_score<true>, which forms
// relu(P[u] + Q[v]) from the image and the user's 16 P chunks of this lane half.  The P rows
// come from a table that lives in L2; they pass through a small LDS stage, kDenseStage users
// at a time with the next stage's loads in flight, and a lane half reads a chunk as one
// broadcast address (16 loads per user straight from the table found no registers left
// beside W2 and the tile, and ran one at a time, each waiting out its L2 latency).  The
// arithmetic per pair
// is that of edge_mlp_lds_kernel — the same relu(p + q) per element, the same k order on the
// MFMA, the same half-combine and sigmoid — so the scores are bitwise gnnrec_edge_mlp_f32's.
// Q traffic: each Q row is read once per user group, n_users / kDenseUsers x |Q| in all
// (16 x 512 MB for 1024 users x 1M items, against 1024 x for a per-user walk).
// Two epilogues: STORE writes out[u, v]; FILTER appends (v, score) to row u's candidate
// list where score >= tau[u] (no band: the score is the final fp32 value), counting past
// cap.  Items past n_cols are staged as zero rows and masked at the store or the compare;
// rows past n_users are never visited.
//
// The popularity-weighted rating (f1d, rating.hpp) adds three epilogues:
// STORE_R and FILTER_R are STORE and FILTER with R = rating(score, Z[u], pcol[v]) in the
// score's place (no band either: the compared value is the final fp32 R, and it is what the
// filter keeps), and DENOM writes nothing but the partial sums of Z[u] = sum over all items
// of expf(score).  Their order is fixed by n_items alone: a DENOM work item is (a chunk of
// kDenseZTiles consecutive item tiles, user group) — the partial is addressed by the chunk's
// index, whichever wave takes it — the wave walks the chunk's tiles in ascending order, a
// tile's 32 values expf(score) (items past the end count zero) are folded over the lanes by
// an xor tree (offsets 1, 2, 4, 8, 16) and added to the user's sum in the wave's LDS; the
// partials [chunks, n_users] are folded in index order by gnnrec_fold_partials_f32.  No float
// atomics; a user's sums do not depend on the group it is scored in.
//
// Full-ranking evaluation (f1f for this head) adds two epilogues on
// DENOM's work decomposition, COUNT_L and COUNT_LR, which share one scored row among a user's
// held-out items.  A row r is a USER (or kDenseListSlots entries of a longer list: the caller
// splits it over rows that repeat the user's P row; a single pair (u, g) is a row with one
// slot); its entries are the slots [lptr[r], lptr[r + 1]) of thr (the entry's own edge_mlp
// score) and gid (its held-out item).  An item v counts for slot j of row r where
//   v != gid[j]  and  (x > t_j  or  (x == t_j and v < gid[j]))
// with x the final fp32 score and t_j = thr[j], or for COUNT_LR x = rating(score, Z[r], pcol[v])
// and t_j = rating(thr[j], Z[r], pcol[gid[j]]) formed here by the same inline function.  No
// band: x is the very value the ranking is defined on.
// After a (row, tile) is scored, lane j loads slot j's threshold and item — for COUNT_LR the
// threshold is rated then (loading them before the row's 64 MFMAs spilled 360 B a lane around
// the MFMA chain) — and a wave-uniform loop over the row's slots reads them back by v_readlane
// and counts, per slot, the compare above by ballot and popcount; lane j keeps slot j's count
// and adds it to the slot's 16-bit counter in the wave's LDS (a chunk holds 1024 items: no
// overflow), 64 rows x 16 slots x 2 B = the 2 KB a wave has left beside the image and the P
// stage with two blocks on a CU.  After the chunk the counters go to part[chunk, slot] (int32)
// and fold_partials_i32_kernel sums them.  Integers: no order to fix, no atomics.
constexpr int kDenseZTiles = 32;  // item tiles (1024 items) per partial of the denominators
enum DenseMode { kDenseStore = 0, kDenseFilter = 1, kDenseDenom = 2, kDenseStoreR = 3,
                 kDenseFilterR = 4, kDenseCountL = 5, kDenseCountLR = 6 };
constexpr int kDenseListSlots = 16;  // COUNT_L / COUNT_LR: list entries per row, at most
static_assert(kDenseZTiles * kMlpTile <= 65535, "a chunk's count fits a 16-bit counter");
constexpr int kDenseUsers = 64;  // users scored per staged item tile, at most
constexpr int kDenseStage = 4;   // users whose P rows are staged in LDS at a time
constexpr int kDenseCandMax = 4096;  // candidate slots per row, at most (recommend.hip's)

struct DenseMlpArgs {
  EdgeMlpArgs m;        // P, Q, W2, b2, w3, b3; the edge-list fields unused
  int64_t n_users;
  int64_t n_cols;       // items
  int64_t groups;       // user groups per item tile
  int64_t per_group;    // users per group: the batch split evenly, at most kDenseUsers
  int64_t work;         // work items: item tiles x user groups
  float* out;           // STORE
  int64_t ldo;
  const float* tau;     // FILTER; COUNT_L / COUNT_LR: the slot's own raw score
  int* counts;
  int* cand_items;
  float* cand_scores;
  int cap;
  const float* Z;       // STORE_R / FILTER_R: per user row
  const float* pcol;    //                     per column of Q
  float* part;          // DENOM: [chunks, n_users]
  int64_t n_tiles;      // DENOM / COUNT_L / COUNT_LR: item tiles
  const int* gid;       // COUNT_L / COUNT_LR: the slot's held-out item
  int* ipart;           // COUNT_L / COUNT_LR: [chunks, n_slots]
  const int64_t* lptr;  // COUNT_L / COUNT_LR: [n_users + 1], row r's slots of tau / gid
  int64_t n_slots;
};

// The slots of list row u: its first slot in b0 and their number (wave-uniform where u is),
// zero where the row's bounds do not lie inside [0, n_slots] or span more than
// kDenseListSlots slots (out of contract: a row is never counted in part) — nothing is read or
// written then.
__device__ __forceinline__ int dense_list_slots(const int64_t* __restrict__ lptr, int64_t n_slots,
                                                int64_t u, int64_t& b0) {
  b0 = lptr[u];
  const int64_t b1 = lptr[u + 1];
  if (b0 < 0 || b1 > n_slots || b1 <= b0 || b1 - b0 > kDenseListSlots) return 0;
  return (int)(b1 - b0);
}

// The P rows of users [u0, u0 + kDenseStage) as the stage holds them (row-major, 32 chunks a
// row: contiguous in the table), lane l the chunks l and 64 + l; zero past u1.
__device__ __forceinline__ void dense_fetch_p(const float4* __restrict__ P4, int64_t u0,
                                              int64_t u1, int lane, float4 (&pf)[2]) {
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    pf[k] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (u0 + 2 * k + (lane >> 5) < u1) pf[k] = P4[u0 * 32 + k * 64 + lane];
  }
}

template <int MODE>
__global__ __launch_bounds__(256, 2) void edge_mlp_dense_kernel(DenseMlpArgs a) {
  constexpr bool FILTER = MODE == kDenseFilter || MODE == kDenseFilterR;
  constexpr bool RATING = MODE == kDenseStoreR || MODE == kDenseFilterR ||
                          MODE == kDenseCountLR;
  constexpr bool DENOM = MODE == kDenseDenom;
  constexpr bool LISTS = MODE == kDenseCountL || MODE == kDenseCountLR;
  constexpr bool CHUNKED = DENOM || LISTS;  // a work item walks a chunk of tiles
  __shared__ float4 image[kMlpWaves][kMlpTile * 32];     // 16 KB per wave
  __shared__ float4 pstage[kMlpWaves][kDenseStage * 32];  // 2 KB per wave
  __shared__ float zsum[kMlpWaves][DENOM ? kDenseUsers : 1];  // DENOM: the group's sums
  // LISTS: the group's slot counters, [row][slot], two to a word
  __shared__ unsigned short lsum[kMlpWaves][LISTS ? kDenseUsers * kDenseListSlots : 2];
  static_assert(kDenseStage * 32 == 2 * kWave, "a stage is two chunks per lane");
  const int lane = threadIdx.x & 63;
  const int wv = threadIdx.x >> 6;
  const int r = lane & 31;
  const int h = lane >> 5;
  float4* S = image[wv];
  float4* Ps = pstage[wv];
  const float4* P4 = reinterpret_cast<const float4*>(a.m.P);
  const float4* Q4 = reinterpret_cast<const float4*>(a.m.Q);
  float4 w[16];
  mlp_load_w2(a.m, r, h, w);
  const float b3v = a.m.b3[0];
  // user group fastest: the waves of a block (and neighbouring blocks) share a Q tile in L2
  for (int64_t item = (int64_t)blockIdx.x * kMlpWaves + wv; item < a.work;
       item += (int64_t)gridDim.x * kMlpWaves) {
    const int64_t t0 = item / a.groups, g = item - t0 * a.groups;
    // CHUNKED: t0 is a chunk of tiles, walked in order; else the tile itself
    const int64_t t_beg = CHUNKED ? t0 * kDenseZTiles : t0;
    const int64_t n_walk = CHUNKED ? min<int64_t>(kDenseZTiles, a.n_tiles - t_beg) : 1;
    if constexpr (DENOM) zsum[wv][lane] = 0.f;  // only lane 0 touches it until the write-out
    if constexpr (LISTS) {
      unsigned* z = reinterpret_cast<unsigned*>(lsum[wv]);
#pragma unroll
      for (int k = 0; k < kDenseUsers * kDenseListSlots / 2 / kWave; ++k) z[k * kWave + lane] = 0u;
    }
    // one item tile for the group's users (the body stays at the loop's indentation); a
    // lambda, called once outside DENOM: as a loop with one trip the store and filter forms
    // compiled to 12 and 8 more bytes of scratch per lane
    auto score_tile = [&](const int64_t t) {
    const int64_t col = t * kMlpTile + r;  // this lane's item (both halves)
    const int v = col < a.n_cols ? (int)col : -1;
    float pv = 0.f;
    if constexpr (RATING) pv = v >= 0 ? a.pcol[col] : 0.f;
    // the previous work item's reads of the image are done before it is overwritten
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
#pragma unroll
    for (int half = 0; half < 2; ++half) {
      float4 q[8], p[8];
      mlp_load<true, 8>(Q4, P4, v, 0, r, h, 8 * half, q, p);
#pragma unroll
      for (int i = 0; i < 8; ++i) S[(2 * (8 * half + i) + h) * 32 + r] = q[i];
    }
    // the staging stores are visible to the MFMA-layout reads (lane r reads row r)
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    const int64_t u_beg = g * a.per_group;
    const int64_t u1 = min<int64_t>(a.n_users, u_beg + a.per_group);
    // kDenseStage users' P rows at a time (4 rows x 32 chunks = two per lane, row-major),
    // the next stage's chunks in flight while this one is scored
    float4 pf[2];
    dense_fetch_p(P4, u_beg, u1, lane, pf);
    for (int64_t u0 = u_beg; u0 < u1; u0 += kDenseStage) {  // wave-uniform
      // the previous stage's reads are done before it is overwritten
      __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
      Ps[lane] = pf[0];
      Ps[64 + lane] = pf[1];
      __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
      if (u0 + kDenseStage < u1) dense_fetch_p(P4, u0 + kDenseStage, u1, lane, pf);
      const int nu = (int)min<int64_t>(kDenseStage, u1 - u0);
      for (int j = 0; j < nu; ++j) {
        const int64_t u = u0 + j;
        float4 pc[16];  // both lane halves read one address each: LDS broadcasts
#pragma unroll
        for (int c = 0; c < 16; ++c) pc[c] = Ps[j * 32 + 16 * h + c];
        float thr = 0.f, zu = 1.f;
        int gu = -1;
        if constexpr (FILTER) thr = a.tau[u];
        if constexpr (RATING) zu = a.Z[u];
        float sc = mlp_tile_score<true>(a.m, S, w, pc, r, h, b3v);
        if constexpr (RATING) sc = rating(sc, zu, pv);
        int ns = 0;  // LISTS: the row's slots, lane j holding slot j's threshold and item
        if constexpr (LISTS) {
          int64_t b0;
          ns = __builtin_amdgcn_readfirstlane(dense_list_slots(a.lptr, a.n_slots, u, b0));
          if (lane < ns) {
            thr = a.tau[b0 + lane];
            gu = a.gid[b0 + lane];
            if constexpr (RATING)
              thr = rating(thr, zu, gu >= 0 && gu < a.n_cols ? a.pcol[gu] : 0.f);
          }
        }
        if constexpr (LISTS) {
          int mine = 0;
          const bool live = h == 0 && v >= 0;
          for (int sl = 0; sl < ns; ++sl) {  // wave-uniform
            const float tj = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(thr), sl));
            const int gj = __builtin_amdgcn_readlane(gu, sl);
            // the compare, its terms combined without branches (| and & on bools: every
            // term is a lane mask, and a short-circuit form compiled to two branches a slot)
            const bool ahead = live & (v != gj) & ((sc > tj) | ((sc == tj) & (v < gj)));
            const int n_ahead = __popcll(__ballot(ahead));
            mine = lane == sl ? n_ahead : mine;
          }
          // lane j alone touches (row, slot j)'s counter, in every tile of the chunk
          if (lane < ns) lsum[wv][(u - u_beg) * kDenseListSlots + lane] += (unsigned short)mine;
        } else if constexpr (DENOM) {
          float x = (h == 0 && v >= 0) ? expf(sc) : 0.f;
#pragma unroll
          for (int off = 1; off < 32; off <<= 1) x += __shfl_xor(x, off);
          if (lane == 0) zsum[wv][u - u_beg] += x;
        } else if (h == 0 && v >= 0) {
          if constexpr (FILTER) {
            if (sc >= thr) {
              // the counter keeps counting past cap (the overflow signal); a store happens
              // only inside the row's cap slots
              const int slot = atomicAdd(a.counts + u, 1);
              if (slot >= 0 && slot < a.cap) {
                a.cand_items[u * a.cap + slot] = v;
                a.cand_scores[u * a.cap + slot] = sc;
              }
            }
          } else {
            a.out[u * a.ldo + col] = sc;
          }
        }
      }
    }
    };
    if constexpr (CHUNKED) {
      for (int64_t tt = 0; tt < n_walk; ++tt) score_tile(t_beg + tt);
    } else {
      score_tile(t0);
    }
    if constexpr (LISTS) {
      __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");  // the slot lanes' counts are visible
      static_assert(kWave % kDenseListSlots == 0, "a wave writes whole rows of counters");
      constexpr int kRows = kWave / kDenseListSlots;  // rows written at a time
      const int64_t u_beg = g * a.per_group;
      const int64_t u1 = min<int64_t>(a.n_users, u_beg + a.per_group);
      const int j = lane % kDenseListSlots;
      for (int64_t ub = u_beg; ub < u1; ub += kRows) {  // wave-uniform
        const int64_t u = ub + lane / kDenseListSlots;
        if (u < u1) {
          int64_t b0;
          const int ns = dense_list_slots(a.lptr, a.n_slots, u, b0);
          if (j < ns)
            a.ipart[t0 * a.n_slots + b0 + j] = lsum[wv][(u - u_beg) * kDenseListSlots + j];
        }
      }
      __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    } else if constexpr (DENOM) {
      __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");  // lane 0's sums are visible
      const int64_t u = g * a.per_group + lane;
      if (lane < a.per_group && u < a.n_users) a.part[t0 * a.n_users + u] = zsum[wv][lane];
      __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    }
  }
}

int check_dense(const char* fn, const float* P, int64_t n_users, const float* Q, int64_t n_items,
                const float* W2, const float* b2, const float* w3, const float* b3) {
  GNNREC_REQUIRE(n_users >= 0 && n_items >= 0, "%s: negative size", fn);
  GNNREC_REQUIRE(n_items < (int64_t(1) << 31), "%s: item ids must fit int32", fn);
  if (n_users == 0 || n_items == 0) return GNNREC_OK;
  GNNREC_REQUIRE(P && Q && W2 && b2 && w3 && b3, "%s: null pointer", fn);
  GNNREC_REQUIRE(aligned16(P) && aligned16(Q) && aligned16(W2),
                 "%s: P/Q/W2 must be 16-byte aligned", fn);
  return GNNREC_OK;
}

int launch_edge_mlp_dense(int mode, const char* fn, DenseMlpArgs& a, hipStream_t s) {
  // the users split evenly over the groups: 67 users (get_recs' batch against 1M items) are
  // 34 + 33, not 64 + 3 with every tile staged a second time for three users
  a.groups = (a.n_users + kDenseUsers - 1) / kDenseUsers;
  a.per_group = (a.n_users + a.groups - 1) / a.groups;
  a.n_tiles = (a.n_cols + kMlpTile - 1) / kMlpTile;
  const bool chunked = mode == kDenseDenom || mode == kDenseCountL || mode == kDenseCountLR;
  a.work = (chunked ? (a.n_tiles + kDenseZTiles - 1) / kDenseZTiles : a.n_tiles) * a.groups;
  int64_t blocks = (a.work + kMlpWaves - 1) / kMlpWaves;
  if (blocks > kMlpResidentWaves / kMlpWaves) blocks = kMlpResidentWaves / kMlpWaves;
#define GNNREC_LAUNCH_DENSE(M) \
  hipLaunchKernelGGL(edge_mlp_dense_kernel<M>, dim3((unsigned)blocks), dim3(256), 0, s, a)
  if (mode == kDenseFilter) GNNREC_LAUNCH_DENSE(kDenseFilter);
  else if (mode == kDenseStore) GNNREC_LAUNCH_DENSE(kDenseStore);
  else if (mode == kDenseDenom) GNNREC_LAUNCH_DENSE(kDenseDenom);
  else if (mode == kDenseStoreR) GNNREC_LAUNCH_DENSE(kDenseStoreR);
  else if (mode == kDenseCountL) GNNREC_LAUNCH_DENSE(kDenseCountL);
  else if (mode == kDenseCountLR) GNNREC_LAUNCH_DENSE(kDenseCountLR);
  else GNNREC_LAUNCH_DENSE(kDenseFilterR);
#undef GNNREC_LAUNCH_DENSE
  return check_launch(fn);
}

// The count pass's launch for either form, then the fold of the slots' partials into ahead.
int launch_dense_count_lists(int mode, const char* fn, DenseMlpArgs& a, int32_t* ahead,
                             hipStream_t s) {
  const int rc = launch_edge_mlp_dense(mode, fn, a, s);
  if (rc != GNNREC_OK) return rc;
  return launch_fold_partials_i32(fn, a.ipart, (a.n_tiles + kDenseZTiles - 1) / kDenseZTiles,
                                  a.n_slots, ahead, s);
}

// ------------------------------------------------- rank resolve, MLP head ----
// One wave per list row — a user, kDenseListSlots entries of a longer list, or a single pair —
// of the count pass's row plan: P row b, slots [lptr[b], lptr[b + 1]) of
// sraw / gid / ahead, row_user[b] the user whose exclusion row is walked.  The count pass
// counted EVERY item exactly ahead of a slot's item g, the user's excluded ones too.  The
// user's exclusion row (a CSR over the users whose repeats and out-of-table ids the caller
// struck to -1) is walked ONCE, in tiles of 32 entries: the tile's Q rows staged as the dense
// kernel stages an item tile and scored against the row's P row by mlp_tile_score<true>
// (edge_mlp's bits), turned into R = rating(score, Z, p[v]) for the rating form; a
// wave-uniform loop over the row's slots (lane j holds slot j's threshold and item, read back
// by v_readlane) counts the entries exactly ahead of each slot under the count pass's rule and
// notes a slot whose item is among them.  An excluded item was counted by the pass exactly
// when it is exactly ahead, so
//   rank = (g is in the row) ? 0 : 1 + ahead - excluded_ahead
// is exact arithmetic (rank.hip's header).  Lane j keeps slot j's two results and writes rank
// and vals of its slot, vals = the value the entry is ranked by: its raw score, or its R.  A
// slot whose item is out of range, and a row whose user is, are left unwritten.
template <bool RATING>
__global__ __launch_bounds__(256) void rank_resolve_mlp_lists_kernel(
    EdgeMlpArgs m, const int64_t* __restrict__ row_user, const int64_t* __restrict__ lptr,
    int64_t n_rows, const float* __restrict__ sraw, const int* __restrict__ gid,
    const int* __restrict__ ahead, int64_t n_slots, int64_t n_users, int64_t n_cols,
    const float* __restrict__ Z, const float* __restrict__ pcol,
    const int64_t* __restrict__ ex_ptr, const int32_t* __restrict__ ex_idx,
    int64_t* __restrict__ rank, float* __restrict__ vals) {
  __shared__ float4 image[kMlpWaves][kMlpTile * 32];  // 16 KB per wave
  const int lane = threadIdx.x & 63;
  const int wv = threadIdx.x >> 6;
  const int r = lane & 31;
  const int h = lane >> 5;
  const int64_t b = (int64_t)blockIdx.x * kMlpWaves + wv;
  if (b >= n_rows) return;  // wave-uniform, as every exit below; no block-wide barrier follows
  const int64_t u = row_user[b];
  int64_t b0;
  const int ns = __builtin_amdgcn_readfirstlane(dense_list_slots(lptr, n_slots, b, b0));
  if (u < 0 || u >= n_users || ns == 0) return;
  float4* S = image[wv];
  const float4* P4 = reinterpret_cast<const float4*>(m.P);
  const float4* Q4 = reinterpret_cast<const float4*>(m.Q);
  float zb = 1.f;
  if constexpr (RATING) zb = Z[b];
  float t = 0.f;  // lane j: slot j's threshold and item
  int g = -1;
  if (lane < ns) {
    t = sraw[b0 + lane];
    g = gid[b0 + lane];
    if (g < 0 || g >= n_cols) g = -1;
    if constexpr (RATING) t = rating(t, zb, g >= 0 ? pcol[g] : 0.f);
  }
  int behind = 0;  // lane j: the excluded items exactly ahead of slot j
  bool excluded = false;
  if (ex_ptr) {
    const int64_t e0 = ex_ptr[u], e1 = ex_ptr[u + 1];
    if (e0 < e1) {
      float4 w[16], pc[16];
      mlp_load_w2(m, r, h, w);
      const float b3v = m.b3[0];
#pragma unroll
      for (int c = 0; c < 16; ++c) pc[c] = P4[b * 32 + 16 * h + c];  // the row's P row
      for (int64_t base = e0; base < e1; base += kMlpTile) {  // wave-uniform bound
        const int64_t e = base + r;
        const int64_t c = e < e1 ? ex_idx[e] : -1;  // -1: a repeat or an id past the table
        const int v = c >= 0 && c < n_cols ? (int)c : -1;
        float pv = 0.f;
        if constexpr (RATING) pv = v >= 0 ? pcol[v] : 0.f;
        // the previous tile's reads of the image are done before it is overwritten
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
#pragma unroll
        for (int half = 0; half < 2; ++half) {
          float4 q[8], p[8];
          mlp_load<true, 8>(Q4, P4, v, 0, r, h, 8 * half, q, p);
#pragma unroll
          for (int i = 0; i < 8; ++i) S[(2 * (8 * half + i) + h) * 32 + r] = q[i];
        }
        // the staging stores are visible to the MFMA-layout reads (lane r reads row r)
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        float sc = mlp_tile_score<true>(m, S, w, pc, r, h, b3v);
        if constexpr (RATING) sc = rating(sc, zb, pv);
        for (int j = 0; j < ns; ++j) {  // wave-uniform
          const float tj = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(t), j));
          const int gj = __builtin_amdgcn_readlane(g, j);
          const bool hit = __ballot((v >= 0) & (v == gj)) != 0;
          const bool is_ahead =
              (h == 0) & (v >= 0) & (v != gj) & ((sc > tj) | ((sc == tj) & (v < gj)));
          const int n_ahead = __popcll(__ballot(is_ahead));
          if (lane == j) {
            behind += n_ahead;
            excluded |= hit;
          }
        }
      }
    }
  }
  if (lane < ns && g >= 0) {
    vals[b0 + lane] = t;
    rank[b0 + lane] = excluded ? 0 : 1 + (int64_t)ahead[b0 + lane] - behind;
  }
}

}  // namespace
}  // namespace gnnrec

extern "C" int gnnrec_sddmm_cos_f32(const int64_t* src, const int64_t* dst, int64_t n_edges,
                                    const float* Hs, int64_t lds, const float* Hd, int64_t ldd,
                                    int64_t d, float* out, void* stream) {
  using namespace gnnrec;
  GNNREC_REQUIRE(n_edges >= 0 && d >= 0, "gnnrec_sddmm_cos_f32: negative size");
  if (n_edges == 0) return GNNREC_OK;
  GNNREC_REQUIRE(src && dst && out && Hs && Hd, "gnnrec_sddmm_cos_f32: null pointer");
  GNNREC_REQUIRE(lds >= d && ldd >= d, "gnnrec_sddmm_cos_f32: leading dimension < d");
  hipStream_t s = as_stream(stream);
  const bool vec4 = d % 4 == 0 && lds % 4 == 0 && ldd % 4 == 0 && aligned16(Hs) && aligned16(Hd);
  if (!vec4) return launch_cos<64, 1>(src, dst, n_edges, Hs, lds, Hd, ldd, (int)d, out, s);
  if (d <= 64) return launch_cos<16, 4>(src, dst, n_edges, Hs, lds, Hd, ldd, (int)d, out, s);
  if (d <= 128) return launch_cos<32, 4>(src, dst, n_edges, Hs, lds, Hd, ldd, (int)d, out, s);
  return launch_cos<64, 4>(src, dst, n_edges, Hs, lds, Hd, ldd, (int)d, out, s);
}

extern "C" int gnnrec_sddmm_cos_grouped_f32(const int64_t* src_g, int64_t n_groups,
                                            const int64_t* first, float* out_first, int64_t K,
                                            const int64_t* dst, float* out, const float* Hs,
                                            int64_t lds, const float* Hd, int64_t ldd, int64_t d,
                                            void* stream) {
  using namespace gnnrec;
  GNNREC_REQUIRE(n_groups >= 0 && K >= 0 && d >= 0, "gnnrec_sddmm_cos_grouped_f32: negative size");
  if (n_groups == 0 || (K == 0 && first == nullptr)) return GNNREC_OK;
  GNNREC_REQUIRE(src_g && Hs && Hd && (K == 0 || (dst && out)) && (!first || out_first),
                 "gnnrec_sddmm_cos_grouped_f32: null pointer");
  GNNREC_REQUIRE(lds >= d && ldd >= d, "gnnrec_sddmm_cos_grouped_f32: leading dimension < d");
  GNNREC_REQUIRE(d % 4 == 0 && d <= 256 && lds % 4 == 0 && ldd % 4 == 0 && aligned16(Hs) &&
                     aligned16(Hd),
                 "gnnrec_sddmm_cos_grouped_f32: needs d %% 4 == 0, d <= 256 and 16-B aligned "
                 "rows (gnnrec_sddmm_cos_f32 takes the rest)");
  // one wave per (group, kCosChunk negatives): the launch's work-items (4 waves per
  // 256-thread block) must stay below 2^32
  GNNREC_REQUIRE((n_groups * (K > 0 ? (K + kCosChunk - 1) / kCosChunk : 1) + 3) / 4 * 256 <
                     (int64_t(1) << 32),
                 "gnnrec_sddmm_cos_grouped_f32: too many groups x negatives for one launch");
  hipStream_t s = as_stream(stream);
  if (d <= 64)
    return launch_cos_grouped<16>(src_g, n_groups, first, out_first, K, dst, out, Hs, lds, Hd, ldd,
                                  (int)d, s);
  if (d <= 128)
    return launch_cos_grouped<32>(src_g, n_groups, first, out_first, K, dst, out, Hs, lds, Hd, ldd,
                                  (int)d, s);
  return launch_cos_grouped<64>(src_g, n_groups, first, out_first, K, dst, out, Hs, lds, Hd, ldd,
                                (int)d, s);
}

extern "C" int gnnrec_edge_mlp_f32(const int64_t* src, const int64_t* dst, int64_t n_edges,
                                   const float* P, const float* Q, const float* W2,
                                   const float* b2, const float* w3, const float* b3, float* out,
                                   void* stream) {
  using namespace gnnrec;
  GNNREC_REQUIRE(n_edges >= 0, "gnnrec_edge_mlp_f32: negative size");
  if (n_edges == 0) return GNNREC_OK;
  GNNREC_REQUIRE(src && dst && P && Q && W2 && b2 && w3 && b3 && out,
                 "gnnrec_edge_mlp_f32: null pointer");
  GNNREC_REQUIRE(aligned16(P) && aligned16(Q) && aligned16(W2),
                 "gnnrec_edge_mlp_f32: P/Q/W2 must be 16-byte aligned");
  const int64_t tiles = (n_edges + kMlpTile - 1) / kMlpTile;
  const int64_t ct = mlp_chunk_tiles(tiles);
  EdgeMlpArgs a{src, dst, nullptr, nullptr, out, P, Q, W2, b2, w3, b3, n_edges, 0, 0, 0,
                (tiles + ct - 1) / ct, ct};
  return launch_edge_mlp_lds(false, a, as_stream(stream));
}

extern "C" int gnnrec_edge_mlp_grouped_f32(const int64_t* src_g, int64_t n_groups,
                                           const int64_t* first, float* out_first, int64_t K,
                                           const int64_t* dst, float* out, const float* P,
                                           const float* Q, const float* W2, const float* b2,
                                           const float* w3, const float* b3, void* stream) {
  using namespace gnnrec;
  GNNREC_REQUIRE(n_groups >= 0 && K >= 0, "gnnrec_edge_mlp_grouped_f32: negative size");
  if (n_groups == 0 || (K == 0 && first == nullptr)) return GNNREC_OK;
  GNNREC_REQUIRE(src_g && P && Q && W2 && b2 && w3 && b3 && (K == 0 || (dst && out)) &&
                     (!first || out_first),
                 "gnnrec_edge_mlp_grouped_f32: null pointer");
  GNNREC_REQUIRE(aligned16(P) && aligned16(Q) && aligned16(W2),
                 "gnnrec_edge_mlp_grouped_f32: P/Q/W2 must be 16-byte aligned");
  const int64_t per_group = K + (first ? 1 : 0);
  const int64_t tiles = (per_group + kMlpTile - 1) / kMlpTile;
  const int64_t ct = mlp_chunk_tiles(n_groups * tiles);
  const int64_t chunks = (tiles + ct - 1) / ct;
  EdgeMlpArgs a{src_g, dst, first, out_first, out, P, Q, W2, b2, w3, b3, 0, K, per_group, chunks,
                n_groups * chunks, ct};
  return launch_edge_mlp_lds(true, a, as_stream(stream));
}

extern "C" int gnnrec_edge_mlp_dense_store_f32(const float* P, int64_t n_users, const float* Q,
                                               int64_t n_items, const float* W2, const float* b2,
                                               const float* w3, const float* b3, float* out,
                                               int64_t ldo, void* stream) {
  using namespace gnnrec;
  const char* fn = "gnnrec_edge_mlp_dense_store_f32";
  const int rc = check_dense(fn, P, n_users, Q, n_items, W2, b2, w3, b3);
  if (rc != GNNREC_OK || n_users == 0 || n_items == 0) return rc;
  GNNREC_REQUIRE(out && ldo >= n_items, "%s: bad out / ldo", fn);
  DenseMlpArgs a{};
  a.m.P = P; a.m.Q = Q; a.m.W2 = W2; a.m.b2 = b2; a.m.w3 = w3; a.m.b3 = b3;
  a.n_users = n_users; a.n_cols = n_items;
  a.out = out; a.ldo = ldo;
  return launch_edge_mlp_dense(kDenseStore, fn, a, as_stream(stream));
}

extern "C" int gnnrec_edge_mlp_dense_filter_f32(const float* P, int64_t n_users, const float* Q,
                                                int64_t n_items, const float* W2, const float* b2,
                                                const float* w3, const float* b3, const float* tau,
                                                int32_t* counts, int32_t* cand_items,
                                                float* cand_scores, int64_t cap, void* stream) {
  using namespace gnnrec;
  const char* fn = "gnnrec_edge_mlp_dense_filter_f32";
  const int rc = check_dense(fn, P, n_users, Q, n_items, W2, b2, w3, b3);
  if (rc != GNNREC_OK) return rc;
  GNNREC_REQUIRE(cap >= 1 && cap <= kDenseCandMax, "%s: cap must be in [1, %d] (got %lld)", fn,
                 kDenseCandMax, (long long)cap);
  if (n_users == 0 || n_items == 0) return GNNREC_OK;
  GNNREC_REQUIRE(tau && counts && cand_items && cand_scores, "%s: null pointer", fn);
  DenseMlpArgs a{};
  a.m.P = P; a.m.Q = Q; a.m.W2 = W2; a.m.b2 = b2; a.m.w3 = w3; a.m.b3 = b3;
  a.n_users = n_users; a.n_cols = n_items;
  a.tau = tau; a.counts = counts; a.cand_items = cand_items; a.cand_scores = cand_scores;
  a.cap = (int)cap;
  return launch_edge_mlp_dense(kDenseFilter, fn, a, as_stream(stream));
}

extern "C" int gnnrec_edge_mlp_dense_denominators_f32(const float* P, int64_t n_users,
                                                      const float* Q, int64_t n_items,
                                                      const float* W2, const float* b2,
                                                      const float* w3, const float* b3,
                                                      float* parts, void* stream) {
  using namespace gnnrec;
  const char* fn = "gnnrec_edge_mlp_dense_denominators_f32";
  const int rc = check_dense(fn, P, n_users, Q, n_items, W2, b2, w3, b3);
  if (rc != GNNREC_OK || n_users == 0 || n_items == 0) return rc;
  GNNREC_REQUIRE(parts, "%s: null parts", fn);
  DenseMlpArgs a{};
  a.m.P = P; a.m.Q = Q; a.m.W2 = W2; a.m.b2 = b2; a.m.w3 = w3; a.m.b3 = b3;
  a.n_users = n_users; a.n_cols = n_items;
  a.part = parts;
  return launch_edge_mlp_dense(kDenseDenom, fn, a, as_stream(stream));
}

extern "C" int gnnrec_edge_mlp_dense_store_rating_f32(const float* P, int64_t n_users,
                                                      const float* Q, int64_t n_items,
                                                      const float* W2, const float* b2,
                                                      const float* w3, const float* b3,
                                                      const float* Z, const float* p_col,
                                                      float* out, int64_t ldo, void* stream) {
  using namespace gnnrec;
  const char* fn = "gnnrec_edge_mlp_dense_store_rating_f32";
  const int rc = check_dense(fn, P, n_users, Q, n_items, W2, b2, w3, b3);
  if (rc != GNNREC_OK || n_users == 0 || n_items == 0) return rc;
  GNNREC_REQUIRE(out && ldo >= n_items, "%s: bad out / ldo", fn);
  GNNREC_REQUIRE(Z && p_col, "%s: null Z / p_col", fn);
  DenseMlpArgs a{};
  a.m.P = P; a.m.Q = Q; a.m.W2 = W2; a.m.b2 = b2; a.m.w3 = w3; a.m.b3 = b3;
  a.n_users = n_users; a.n_cols = n_items;
  a.out = out; a.ldo = ldo; a.Z = Z; a.pcol = p_col;
  return launch_edge_mlp_dense(kDenseStoreR, fn, a, as_stream(stream));
}

extern "C" int gnnrec_edge_mlp_dense_filter_rating_f32(
    const float* P, int64_t n_users, const float* Q, int64_t n_items, const float* W2,
    const float* b2, const float* w3, const float* b3, const float* Z, const float* p_col,
    const float* tau, int32_t* counts, int32_t* cand_items, float* cand_scores, int64_t cap,
    void* stream) {
  using namespace gnnrec;
  const char* fn = "gnnrec_edge_mlp_dense_filter_rating_f32";
  const int rc = check_dense(fn, P, n_users, Q, n_items, W2, b2, w3, b3);
  if (rc != GNNREC_OK) return rc;
  GNNREC_REQUIRE(cap >= 1 && cap <= kDenseCandMax, "%s: cap must be in [1, %d] (got %lld)", fn,
                 kDenseCandMax, (long long)cap);
  if (n_users == 0 || n_items == 0) return GNNREC_OK;
  GNNREC_REQUIRE(Z && p_col && tau && counts && cand_items && cand_scores, "%s: null pointer", fn);
  DenseMlpArgs a{};
  a.m.P = P; a.m.Q = Q; a.m.W2 = W2; a.m.b2 = b2; a.m.w3 = w3; a.m.b3 = b3;
  a.n_users = n_users; a.n_cols = n_items;
  a.tau = tau; a.counts = counts; a.cand_items = cand_items; a.cand_scores = cand_scores;
  a.cap = (int)cap; a.Z = Z; a.pcol = p_col;
  return launch_edge_mlp_dense(kDenseFilterR, fn, a, as_stream(stream));
}

// ---- the full-ranking evaluation ----
extern "C" int64_t gnnrec_rank_list_slots(void) { return gnnrec::kDenseListSlots; }

// the slot operands of a count pass, after check_dense: ahead is zeroed where there is nothing
// to count, and no kernel is launched then
static int dense_count_lists_operands(const char* fn, int64_t n_rows, int64_t n_items,
                                      const void* lptr, int64_t n_slots, const void* thr,
                                      const void* gid, const void* parts, int32_t* ahead,
                                      void* stream, bool* empty) {
  using namespace gnnrec;
  GNNREC_REQUIRE(n_slots >= 0 && (n_slots + 255) / 256 < (int64_t(1) << 31) &&
                     n_slots <= n_rows * kDenseListSlots,
                 "%s: n_slots must be in [0, %d n_rows] (got %lld for %lld rows)", fn,
                 kDenseListSlots, (long long)n_slots, (long long)n_rows);
  *empty = n_slots == 0 || n_items == 0;
  if (n_slots == 0) return GNNREC_OK;
  GNNREC_REQUIRE(ahead, "%s: null ahead", fn);
  if (n_items == 0) {
    const hipError_t e = hipMemsetAsync(ahead, 0, (size_t)n_slots * sizeof(int32_t),
                                        as_stream(stream));
    GNNREC_REQUIRE(e == hipSuccess, "%s: %s", fn, hipGetErrorString(e));
    return GNNREC_OK;
  }
  GNNREC_REQUIRE(lptr && thr && gid && parts, "%s: null lptr / thr / gid / parts", fn);
  return GNNREC_OK;
}

extern "C" int gnnrec_edge_mlp_dense_count_lists_f32(
    const float* P, int64_t n_rows, const float* Q, int64_t n_items, const float* W2,
    const float* b2, const float* w3, const float* b3, const int64_t* lptr, int64_t n_slots,
    const float* thr, const int32_t* gid, int32_t* parts, int32_t* ahead, void* stream) {
  using namespace gnnrec;
  const char* fn = "gnnrec_edge_mlp_dense_count_lists_f32";
  int rc = check_dense(fn, P, n_rows, Q, n_items, W2, b2, w3, b3);
  if (rc != GNNREC_OK) return rc;
  bool empty;
  rc = dense_count_lists_operands(fn, n_rows, n_items, lptr, n_slots, thr, gid, parts, ahead,
                                  stream, &empty);
  if (rc != GNNREC_OK || empty) return rc;
  DenseMlpArgs a{};
  a.m.P = P; a.m.Q = Q; a.m.W2 = W2; a.m.b2 = b2; a.m.w3 = w3; a.m.b3 = b3;
  a.n_users = n_rows; a.n_cols = n_items;
  a.tau = thr; a.gid = gid; a.ipart = parts; a.lptr = lptr; a.n_slots = n_slots;
  return launch_dense_count_lists(kDenseCountL, fn, a, ahead, as_stream(stream));
}

extern "C" int gnnrec_edge_mlp_dense_count_lists_rating_f32(
    const float* P, int64_t n_rows, const float* Q, int64_t n_items, const float* W2,
    const float* b2, const float* w3, const float* b3, const float* Z, const float* p_col,
    const int64_t* lptr, int64_t n_slots, const float* s, const int32_t* gid, int32_t* parts,
    int32_t* ahead, void* stream) {
  using namespace gnnrec;
  const char* fn = "gnnrec_edge_mlp_dense_count_lists_rating_f32";
  int rc = check_dense(fn, P, n_rows, Q, n_items, W2, b2, w3, b3);
  if (rc != GNNREC_OK) return rc;
  bool empty;
  rc = dense_count_lists_operands(fn, n_rows, n_items, lptr, n_slots, s, gid, parts, ahead,
                                  stream, &empty);
  if (rc != GNNREC_OK || empty) return rc;
  GNNREC_REQUIRE(Z && p_col, "%s: null Z / p_col", fn);
  DenseMlpArgs a{};
  a.m.P = P; a.m.Q = Q; a.m.W2 = W2; a.m.b2 = b2; a.m.w3 = w3; a.m.b3 = b3;
  a.n_users = n_rows; a.n_cols = n_items;
  a.tau = s; a.gid = gid; a.ipart = parts; a.Z = Z; a.pcol = p_col;
  a.lptr = lptr; a.n_slots = n_slots;
  return launch_dense_count_lists(kDenseCountLR, fn, a, ahead, as_stream(stream));
}

extern "C" int gnnrec_rank_resolve_mlp_lists_f32(
    const int64_t* row_user, const int64_t* lptr, int64_t n_rows, const float* s,
    const int32_t* gid, const int32_t* ahead, int64_t n_slots, int64_t n_users, const float* P,
    const float* Q, int64_t n_items, const float* W2, const float* b2, const float* w3,
    const float* b3, const float* Z, const float* p_col, const int64_t* exclude_indptr,
    const int32_t* exclude_indices, int64_t* rank, float* vals, void* stream) {
  using namespace gnnrec;
  const char* fn = "gnnrec_rank_resolve_mlp_lists_f32";
  GNNREC_REQUIRE(n_rows >= 0 && (n_rows + kMlpWaves - 1) / kMlpWaves < (int64_t(1) << 31) &&
                     n_users >= 0 && n_slots >= 0 && n_slots <= n_rows * kDenseListSlots,
                 "%s: bad size", fn);
  const int rc = check_dense(fn, P, n_rows, Q, n_items, W2, b2, w3, b3);
  if (rc != GNNREC_OK) return rc;
  GNNREC_REQUIRE(!exclude_indptr == !exclude_indices,
                 "%s: exclusion indptr and indices come together", fn);
  GNNREC_REQUIRE(!Z == !p_col, "%s: Z and p_col come together", fn);
  if (n_slots == 0) return GNNREC_OK;
  GNNREC_REQUIRE(n_items > 0 && n_users > 0, "%s: entries without users or items", fn);
  GNNREC_REQUIRE(row_user && lptr && s && gid && ahead && rank && vals, "%s: null pointer", fn);
  EdgeMlpArgs m{};
  m.P = P; m.Q = Q; m.W2 = W2; m.b2 = b2; m.w3 = w3; m.b3 = b3;
  const dim3 grid((unsigned)((n_rows + kMlpWaves - 1) / kMlpWaves)), block(256);
  hipStream_t st = as_stream(stream);
  if (Z)
    hipLaunchKernelGGL(rank_resolve_mlp_lists_kernel<true>, grid, block, 0, st, m, row_user, lptr,
                       n_rows, s, gid, ahead, n_slots, n_users, n_items, Z, p_col,
                       exclude_indptr, exclude_indices, rank, vals);
  else
    hipLaunchKernelGGL(rank_resolve_mlp_lists_kernel<false>, grid, block, 0, st, m, row_user, lptr,
                       n_rows, s, gid, ahead, n_slots, n_users, n_items, Z, p_col,
                       exclude_indptr, exclude_indices, rank, vals);
  return check_launch(fn);
}
