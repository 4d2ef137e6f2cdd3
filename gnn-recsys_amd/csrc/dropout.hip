// Dropout of the training layers (reference src/model.py:140-141: ConvLayer.forward applies
// dropout_fn to h_neigh and h_self) without a stored mask or a dropped copy of a source
// table: the mask is the counter-based function of dropout.hpp, regenerated where it is
// needed.
//
//   * forward, neighbour side: the sum / mean gather of spmm.hip with the mask of the
//     GATHERED row applied to every fragment as it arrives (GNNREC_DROPOUT_SRC);
//   * backward, neighbour side: the same gather over the source-major CSR, with the mask of
//     the OUTPUT row applied once, at the store of the row (GNNREC_DROPOUT_OUT) — before an
//     accumulate, so it multiplies this relation's contribution only;
//   * self side: x ⊙ mask · scale over the first n rows of a table (stored or accumulated);
//   * the keys of one forward call from a device-resident step counter, which the same
//     launch advances: a replayed graph draws a new mask on every replay.
//
// The gathers keep spmm.hip's mapping (one wave per row, LPR lanes per source row, a lane
// group per row for low-degree CSRs, heavy rows through chunk partials and a combine) and
// its fixed reduction order, so they are reproducible run to run.  The inference kernels of
// spmm.hip are not touched.
#include "common.hpp"
#include "dropout.hpp"
#include "gather.hpp"
#include "rowq.hpp"

namespace gnnrec {
namespace {

struct DropArgs {
  const uint64_t* keys;  // device: one key per stream of the forward call
  int index;             // this launch's stream
  uint32_t T;
  float scale;
  int Q;  // words per row: ceil(d / 4)
};

// zero the dropped columns of the fragment at column col of a row whose word is `word`
// (VEC == 4: col % 4 == 0, the word's four draws are the fragment's columns)
template <int VEC>
__device__ __forceinline__ void drop_frag(Frag<VEC>& f, uint64_t word, int col, uint32_t T) {
  if constexpr (VEC == 4) {
#pragma unroll
    for (int v = 0; v < 4; ++v)
      if (!drop_keep(word, v, T)) f.v[v] = 0.f;
  } else {
    if (!drop_keep(word, col, T)) f.v[0] = 0.f;
  }
}

// gather_range (gather.hpp) with the mask of each gathered source row: the words depend on
// the broadcast index only, so they are computed while the row loads are in flight
template <int LPR, int VEC, bool WEIGHTED, int UNROLL>
__device__ __forceinline__ void gather_range_drop(int64_t beg, int64_t end,
                                                  const int32_t* __restrict__ indices,
                                                  const float* __restrict__ ew,
                                                  const float* __restrict__ X, int64_t ldx,
                                                  int col, bool colok, int lane, int grp,
                                                  Frag<VEC>& acc, uint64_t key, uint32_t T,
                                                  int Q) {
  constexpr int NPI = kWave / LPR;
  const int q = col >> 2;
  for (int64_t base = beg; base < end; base += 64) {
    const int cnt = (int)((end - base) < 64 ? (end - base) : 64);
    const int myidx = lane < cnt ? ld_stream(indices + base + lane) : 0;
    float myw = 0.f;
    if constexpr (WEIGHTED) myw = lane < cnt ? ld_stream(ew + base + lane) : 0.f;
    for (int j = 0; j < cnt; j += NPI * UNROLL) {
      Frag<VEC> val[UNROLL];
      int src[UNROLL];
#pragma unroll
      for (int u = 0; u < UNROLL; ++u) {
        const int k = j + u * NPI + grp;
        const bool ok = (k < cnt) && colok;
        src[u] = edge_bcast<NPI>(myidx, j + u * NPI, grp);
        if (ok) {
          load_frag<VEC>(val[u], X + (int64_t)src[u] * ldx + col);
        } else {
#pragma unroll
          for (int v = 0; v < VEC; ++v) val[u].v[v] = 0.f;
        }
      }
      uint64_t word[UNROLL];
#pragma unroll
      for (int u = 0; u < UNROLL; ++u) word[u] = drop_word(key, src[u], Q, q);
#pragma unroll
      for (int u = 0; u < UNROLL; ++u) {
        float w = 1.f;
        if constexpr (WEIGHTED) w = edge_bcast<NPI>(myw, j + u * NPI, grp);
        drop_frag<VEC>(val[u], word[u], col, T);
#pragma unroll
        for (int v = 0; v < VEC; ++v) acc.v[v] += WEIGHTED ? val[u].v[v] * w : val[u].v[v];
      }
    }
  }
}

// the end of a row: the mean's division, the output row's mask (WHERE == OUT), the scale,
// then the store — or the add into what the table holds (GNNREC_SPMM_ACCUM)
template <int VEC, int REDUCE, int WHERE>
__device__ __forceinline__ void finish_row(Frag<VEC>& acc, int64_t row, int64_t deg, int col,
                                           float* __restrict__ out, int64_t ldo, int flags,
                                           uint64_t key, const DropArgs& da) {
  finalize<VEC, REDUCE>(acc, deg, 0);
  if constexpr (WHERE == GNNREC_DROPOUT_OUT)
    drop_frag<VEC>(acc, drop_word(key, row, da.Q, col >> 2), col, da.T);
#pragma unroll
  for (int v = 0; v < VEC; ++v) acc.v[v] *= da.scale;
  if (flags & GNNREC_SPMM_ACCUM) accumulate_into<VEC, REDUCE>(acc, out + row * ldo + col);
  store_frag<VEC>(out + row * ldo + col, acc);
}

// spmm.hip's group_rows (one lane group per low-degree row, the wave kernel's reduction
// order) with the mask
template <int LPR, int VEC, int REDUCE, bool WEIGHTED, int WHERE>
__device__ __forceinline__ void group_rows_drop(
    const int64_t* __restrict__ indptr, const int32_t* __restrict__ indices,
    const float* __restrict__ ew, const float* __restrict__ X, int64_t ldx, int64_t n_dst, int d,
    float* __restrict__ out, int64_t ldo, int flags, int64_t max_deg, uint64_t key,
    const DropArgs& da) {
  constexpr int NPI = kWave / LPR;
  constexpr int U = NPI >= 8 ? NPI : 8;
  const int lane = threadIdx.x & 63;
  const int col = (lane % LPR) * VEC;
  const bool colok = col < d;
  const int64_t stride = (int64_t)gridDim.x * 4 * NPI;
  int64_t row = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * NPI + lane / LPR;
  int64_t beg = 0, end = 0;
  if (row < n_dst) {
    beg = ld_stream(indptr + row);
    end = ld_stream(indptr + row + 1);
  }
  for (; row < n_dst; row += stride) {
    const int64_t nrow = row + stride;
    int64_t nbeg = 0, nend = 0;
    if (nrow < n_dst) {
      nbeg = ld_stream(indptr + nrow);
      nend = ld_stream(indptr + nrow + 1);
    }
    if (end - beg <= max_deg) {  // heavy rows: reduced by the chunk kernels
      Frag<VEC> p[NPI];
#pragma unroll
      for (int i = 0; i < NPI; ++i)
#pragma unroll
        for (int v = 0; v < VEC; ++v) p[i].v[v] = 0.f;
      for (int64_t k = beg; k < end; k += U) {
        const int cnt = (int)(end - k < U ? end - k : U);
        int src[U];
        float w[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          src[u] = u < cnt ? ld_stream(indices + k + u) : 0;
          if constexpr (WEIGHTED) w[u] = u < cnt ? ld_stream(ew + k + u) : 0.f;
        }
        Frag<VEC> val[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          if (u < cnt && colok) {
            load_frag<VEC>(val[u], X + (int64_t)src[u] * ldx + col);
          } else {
#pragma unroll
            for (int v = 0; v < VEC; ++v) val[u].v[v] = 0.f;
          }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
          if (u < cnt) {
            if constexpr (WHERE == GNNREC_DROPOUT_SRC)
              drop_frag<VEC>(val[u], drop_word(key, src[u], da.Q, col >> 2), col, da.T);
#pragma unroll
            for (int v = 0; v < VEC; ++v)
              p[u % NPI].v[v] += WEIGHTED ? val[u].v[v] * w[u] : val[u].v[v];
          }
        }
      }
#pragma unroll
      for (int s = 1; s < NPI; s <<= 1)
#pragma unroll
        for (int i = 0; i < NPI; i += 2 * s)
#pragma unroll
          for (int v = 0; v < VEC; ++v) p[i].v[v] += p[i + s].v[v];
      if (colok)
        finish_row<VEC, REDUCE, WHERE>(p[0], row, end - beg, col, out, ldo, flags, key, da);
    }
    beg = nbeg;
    end = nend;
  }
}

constexpr int64_t kGroupMaxAvgDeg = 16;  // spmm.hip's: mean degree the group form takes

template <int LPR, int VEC, int REDUCE, bool WEIGHTED, int UNROLL, int WHERE>
__global__ __launch_bounds__(256) void drop_csr_kernel(
    const int64_t* __restrict__ indptr, const int32_t* __restrict__ indices,
    const float* __restrict__ ew, const float* __restrict__ X, int64_t ldx, int64_t n_dst, int d,
    float* __restrict__ out, int64_t ldo, int flags, int64_t max_deg,
    const int64_t* __restrict__ live, const int64_t* __restrict__ plan_counts, DropArgs da) {
  // an overflowed device plan covers no row: every row is reduced here (spmm.hip)
  if (plan_counts != nullptr && plan_counts[0] < 0) max_deg = INT64_MAX;
  if (live != nullptr) {
    // rows from the device count on: 0 (left as they are under ACCUM), no gathers
    const int64_t l = *live;
    const int64_t n_rows = l < 0 ? 0 : (l < n_dst ? l : n_dst);
    if (!(flags & GNNREC_SPMM_ACCUM) && blockIdx.y == 0) {
      const int64_t nw = (int64_t)gridDim.x * 4;
      for (int64_t r = n_rows + (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); r < n_dst; r += nw)
        for (int c = threadIdx.x & 63; c < d; c += 64) out[r * ldo + c] = 0.f;
    }
    n_dst = n_rows;
    if (n_dst == 0) return;
  }
  const uint64_t key = da.keys[da.index];
  if constexpr (VEC == 4 && (LPR == 8 || LPR == 16)) {
    if (indptr[n_dst] - indptr[0] <= kGroupMaxAvgDeg * n_dst) {
      group_rows_drop<LPR, VEC, REDUCE, WEIGHTED, WHERE>(indptr, indices, ew, X, ldx, n_dst, d,
                                                         out, ldo, flags, max_deg, key, da);
      return;
    }
  }
  const int lane = threadIdx.x & 63;
  const int grp = lane / LPR;
  const int col = blockIdx.y * (LPR * VEC) + (lane % LPR) * VEC;
  const bool colok = col < d;
  const int64_t wstride = (int64_t)gridDim.x * 4;
  for (int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); row < n_dst; row += wstride) {
    const int64_t beg = indptr[row];
    const int64_t end = indptr[row + 1];
    if (end - beg > max_deg) continue;  // heavy row: reduced by the chunk kernels
    Frag<VEC> acc;
#pragma unroll
    for (int v = 0; v < VEC; ++v) acc.v[v] = 0.f;
    if constexpr (WHERE == GNNREC_DROPOUT_SRC)
      gather_range_drop<LPR, VEC, WEIGHTED, UNROLL>(beg, end, indices, ew, X, ldx, col, colok,
                                                    lane, grp, acc, key, da.T, da.Q);
    else
      gather_range<LPR, VEC, GNNREC_REDUCE_SUM, WEIGHTED, UNROLL>(beg, end, indices, ew, X, ldx,
                                                                  col, colok, lane, grp, acc);
    combine_groups<LPR, VEC, GNNREC_REDUCE_SUM>(acc);
    if (grp == 0 && colok)
      finish_row<VEC, REDUCE, WHERE>(acc, row, end - beg, col, out, ldo, flags, key, da);
  }
}

// heavy rows, phase 1: one wave per chunk of `split` edges -> raw partial in ws[chunk]
template <int LPR, int VEC, bool WEIGHTED, int UNROLL, int WHERE>
__global__ __launch_bounds__(256) void drop_chunk_kernel(
    const int64_t* __restrict__ indptr, const int32_t* __restrict__ indices,
    const float* __restrict__ ew, const float* __restrict__ X, int64_t ldx, int d, int64_t split,
    const int64_t* __restrict__ heavy_rows, const int64_t* __restrict__ chunk_ptr,
    const int64_t* __restrict__ chunk_row, int64_t n_chunks, const int64_t* __restrict__ counts,
    float* __restrict__ ws, DropArgs da) {
  const int lane = threadIdx.x & 63;
  const int grp = lane / LPR;
  const int col = blockIdx.y * (LPR * VEC) + (lane % LPR) * VEC;
  const bool colok = col < d;
  const int64_t wstride = (int64_t)gridDim.x * 4;
  if (counts) n_chunks = counts[1];  // device-built plan (0 when it overflowed)
  const uint64_t key = da.keys[da.index];
  for (int64_t c = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); c < n_chunks; c += wstride) {
    const int64_t h = chunk_row[c];
    const int64_t row = heavy_rows[h];
    const int64_t rbeg = indptr[row], rend = indptr[row + 1];
    const int64_t beg = rbeg + (c - chunk_ptr[h]) * split;
    const int64_t end = (beg + split < rend) ? beg + split : rend;
    Frag<VEC> acc;
#pragma unroll
    for (int v = 0; v < VEC; ++v) acc.v[v] = 0.f;
    if constexpr (WHERE == GNNREC_DROPOUT_SRC)
      gather_range_drop<LPR, VEC, WEIGHTED, UNROLL>(beg, end, indices, ew, X, ldx, col, colok,
                                                    lane, grp, acc, key, da.T, da.Q);
    else
      gather_range<LPR, VEC, GNNREC_REDUCE_SUM, WEIGHTED, UNROLL>(beg, end, indices, ew, X, ldx,
                                                                  col, colok, lane, grp, acc);
    combine_groups<LPR, VEC, GNNREC_REDUCE_SUM>(acc);
    if (grp == 0 && colok) store_frag<VEC>(ws + c * (int64_t)d + col, acc);
  }
}

// heavy rows, phase 2: one wave per heavy row, partials combined in chunk order; the output
// row's mask at the store
template <int VEC, int REDUCE, int WHERE>
__global__ __launch_bounds__(256) void drop_combine_kernel(
    const int64_t* __restrict__ indptr, int d, const int64_t* __restrict__ heavy_rows,
    int64_t n_heavy, const int64_t* __restrict__ chunk_ptr, const float* __restrict__ ws,
    float* __restrict__ out, int64_t ldo, int flags, const int64_t* __restrict__ counts,
    DropArgs da) {
  const int lane = threadIdx.x & 63;
  const int64_t wstride = (int64_t)gridDim.x * 4;
  if (counts) n_heavy = counts[0];  // < 0: an overflowed plan (the row kernel took them)
  const uint64_t key = da.keys[da.index];
  for (int64_t h = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); h < n_heavy; h += wstride) {
    const int64_t row = heavy_rows[h];
    const int64_t deg = indptr[row + 1] - indptr[row];
    for (int col = blockIdx.y * 64 * VEC + lane * VEC; col < d; col += gridDim.y * 64 * VEC) {
      Frag<VEC> acc;
#pragma unroll
      for (int v = 0; v < VEC; ++v) acc.v[v] = 0.f;
      const int64_t c_end = chunk_ptr[h + 1];
      int64_t c = chunk_ptr[h];
      for (; c + 16 <= c_end; c += 16) {
        Frag<VEC> p[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) load_frag<VEC>(p[u], ws + (c + u) * (int64_t)d + col);
#pragma unroll
        for (int u = 0; u < 16; ++u)
#pragma unroll
          for (int v = 0; v < VEC; ++v) acc.v[v] += p[u].v[v];
      }
      for (; c < c_end; ++c) {
        Frag<VEC> p;
        load_frag<VEC>(p, ws + c * (int64_t)d + col);
#pragma unroll
        for (int v = 0; v < VEC; ++v) acc.v[v] += p.v[v];
      }
      finish_row<VEC, REDUCE, WHERE>(acc, row, deg, col, out, ldo, flags, key, da);
    }
  }
}

struct DropSpmm {
  const int64_t* indptr; const int32_t* indices; const float* ew; const float* X; int64_t ldx;
  int64_t n_dst; int d; float* out; int64_t ldo; int flags;
  int64_t split; const int64_t* plan; int64_t cap_h; int64_t cap_c; float* ws;
  const int64_t* live;
  DropArgs da;
};

inline unsigned grid_waves(int64_t units) {  // spmm.hip's: every wave slot of the free CUs
  int64_t blocks = (units + 3) / 4;
  const int cus = device_cus() - cu_reserve();
  const int64_t max_blocks = (int64_t)(cus > 8 ? cus : 8) * 8;
  if (blocks > max_blocks) blocks = max_blocks;
  return (unsigned)(blocks < 1 ? 1 : blocks);
}

template <int LPR, int VEC, int REDUCE, bool WEIGHTED, int WHERE>
int launch_drop(const DropSpmm& a, hipStream_t s) {
  constexpr int UNROLL = (VEC == 4) ? 4 : 2;
  const int cols_per_slice = LPR * VEC;
  const unsigned slices = (unsigned)((a.d + cols_per_slice - 1) / cols_per_slice);
  const bool planned = a.plan != nullptr;
  const int64_t max_deg = planned ? a.split : INT64_MAX;
  hipLaunchKernelGGL((drop_csr_kernel<LPR, VEC, REDUCE, WEIGHTED, UNROLL, WHERE>),
                     dim3(grid_waves(a.n_dst), slices), dim3(256), 0, s, a.indptr, a.indices, a.ew,
                     a.X, a.ldx, a.n_dst, a.d, a.out, a.ldo, a.flags, max_deg, a.live,
                     planned ? a.plan : nullptr, a.da);
  if (planned) {
    const int64_t* heavy = a.plan + 2;
    const int64_t* chunk_ptr = a.plan + 2 + a.cap_h;
    const int64_t* chunk_row = a.plan + 3 + 2 * a.cap_h;
    hipLaunchKernelGGL((drop_chunk_kernel<LPR, VEC, WEIGHTED, UNROLL, WHERE>),
                       dim3(grid_waves(a.cap_c), slices), dim3(256), 0, s, a.indptr, a.indices,
                       a.ew, a.X, a.ldx, a.d, a.split, heavy, chunk_ptr, chunk_row, a.cap_c,
                       a.plan, a.ws, a.da);
    const unsigned cslices = (unsigned)((a.d + 64 * VEC - 1) / (64 * VEC));
    hipLaunchKernelGGL((drop_combine_kernel<VEC, REDUCE, WHERE>),
                       dim3(grid_waves(a.cap_h), cslices), dim3(256), 0, s, a.indptr, a.d, heavy,
                       a.cap_h, chunk_ptr, a.ws, a.out, a.ldo, a.flags, a.plan, a.da);
  }
  return check_launch("gnnrec_spmm_csr_dropout_f32");
}

template <int LPR, int VEC, int WHERE>
int dispatch_drop(int reduce, const DropSpmm& a, hipStream_t s) {
  const bool w = a.ew != nullptr;
  if (reduce == GNNREC_REDUCE_SUM)
    return w ? launch_drop<LPR, VEC, GNNREC_REDUCE_SUM, true, WHERE>(a, s)
             : launch_drop<LPR, VEC, GNNREC_REDUCE_SUM, false, WHERE>(a, s);
  return w ? launch_drop<LPR, VEC, GNNREC_REDUCE_MEAN, true, WHERE>(a, s)
           : launch_drop<LPR, VEC, GNNREC_REDUCE_MEAN, false, WHERE>(a, s);
}

template <int WHERE>
int dispatch_drop_lpr(bool vec4, int lpr, int reduce, const DropSpmm& a, hipStream_t s) {
  if (!vec4) return dispatch_drop<64, 1, WHERE>(reduce, a, s);
  switch (lpr) {
    case 4: return dispatch_drop<4, 4, WHERE>(reduce, a, s);
    case 8: return dispatch_drop<8, 4, WHERE>(reduce, a, s);
    case 16: return dispatch_drop<16, 4, WHERE>(reduce, a, s);
    case 32: return dispatch_drop<32, 4, WHERE>(reduce, a, s);
    default: return dispatch_drop<64, 4, WHERE>(reduce, a, s);
  }
}

int drop_spmm_entry(DropSpmm a, int64_t d, int reduce, const uint64_t* keys, int64_t key_index,
                    double p, int where, void* stream) {
  GNNREC_REQUIRE(a.n_dst >= 0 && d >= 0, "gnnrec_spmm_csr_dropout_f32: negative size");
  GNNREC_REQUIRE(reduce == GNNREC_REDUCE_SUM || reduce == GNNREC_REDUCE_MEAN,
                 "gnnrec_spmm_csr_dropout_f32: sum or mean, got reduce %d", reduce);
  GNNREC_REQUIRE(where == GNNREC_DROPOUT_SRC || where == GNNREC_DROPOUT_OUT,
                 "gnnrec_spmm_csr_dropout_f32: unknown mask side %d", where);
  GNNREC_REQUIRE(p >= 0.0 && p <= 1.0, "gnnrec_spmm_csr_dropout_f32: p=%g outside [0, 1]", p);
  GNNREC_REQUIRE(d <= (1 << 20), "gnnrec_spmm_csr_dropout_f32: d=%lld too large", (long long)d);
  GNNREC_REQUIRE(key_index >= 0 && key_index < (1 << 30),
                 "gnnrec_spmm_csr_dropout_f32: bad key index");
  if (a.n_dst == 0 || d == 0) return GNNREC_OK;
  GNNREC_REQUIRE(a.indptr && a.out && keys, "gnnrec_spmm_csr_dropout_f32: null indptr/out/keys");
  GNNREC_REQUIRE(a.ldx >= d && a.ldo >= d, "gnnrec_spmm_csr_dropout_f32: leading dimension < d");
  GNNREC_REQUIRE(a.plan == nullptr || (a.split > 0 && a.cap_h > 0 && a.cap_c > 0 && a.ws),
                 "gnnrec_spmm_csr_planned_dropout_f32: incomplete heavy-row plan");
  a.d = (int)d;
  a.flags &= GNNREC_SPMM_ACCUM;
  const DropParams dp = drop_params(p);
  a.da = DropArgs{keys, (int)key_index, dp.T, dp.scale, (int)((d + 3) / 4)};
  const bool vec4 = (d % 4 == 0) && (a.ldx % 4 == 0) && (a.ldo % 4 == 0) && aligned16(a.X) &&
                    aligned16(a.out) && (a.plan == nullptr || aligned16(a.ws));
  int lpr = 64;
  if (vec4) {
    const int64_t lanes = d / 4;
    lpr = 4;
    while (lpr < lanes && lpr < 64) lpr <<= 1;
  }
  hipStream_t s = as_stream(stream);
  return where == GNNREC_DROPOUT_SRC
             ? dispatch_drop_lpr<GNNREC_DROPOUT_SRC>(vec4, lpr, reduce, a, s)
             : dispatch_drop_lpr<GNNREC_DROPOUT_OUT>(vec4, lpr, reduce, a, s);
}

// out[r, :] (+)= x[r, :] ⊙ mask(r, :) · scale for r < n: one thread per word (four columns)
// (out may be x itself: every element is read and written by the one thread that owns it)
__global__ __launch_bounds__(256) void drop_rows_kernel(const float* x, int64_t ldx, int64_t n,
                                                        int d, int accumulate, float* out,
                                                        int64_t ldo, DropArgs da) {
  const uint64_t key = da.keys[da.index];
  const int64_t total = n * da.Q;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
    const int64_t r = i / da.Q;
    const int q = (int)(i - r * da.Q);
    const uint64_t word = drop_word(key, r, da.Q, q);
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const int c = q * 4 + v;
      if (c < d) {
        const float y = drop_keep(word, v, da.T) ? x[r * ldx + c] * da.scale : 0.f;
        float* o = out + r * ldo + c;
        *o = accumulate ? *o + y : y;
      }
    }
  }
}

// keys[i] = hash3(seed, *counter, stream0 + i), then *counter += 1 — one block, every
// thread reads the counter before thread 0 advances it
__global__ __launch_bounds__(256) void drop_keys_kernel(uint64_t seed, int64_t* counter,
                                                        int64_t stream0, int n,
                                                        uint64_t* __restrict__ keys) {
  const uint64_t step = (uint64_t)*counter;
  __syncthreads();
  for (int i = threadIdx.x; i < n; i += blockDim.x)
    keys[i] = drop_key(seed, step, (uint64_t)(stream0 + i));
  if (threadIdx.x == 0) *counter = (int64_t)(step + 1);
}

}  // namespace
}  // namespace gnnrec

extern "C" int gnnrec_dropout_mask_host(uint64_t seed, uint64_t step, uint64_t stream,
                                        int64_t n_rows, int64_t d, double p, uint8_t* keep) {
  using namespace gnnrec;
  GNNREC_REQUIRE(n_rows >= 0 && d >= 0 && d <= (1 << 20), "gnnrec_dropout_mask_host: bad size");
  GNNREC_REQUIRE(p >= 0.0 && p <= 1.0, "gnnrec_dropout_mask_host: p=%g outside [0, 1]", p);
  if (n_rows == 0 || d == 0) return GNNREC_OK;
  GNNREC_REQUIRE(keep, "gnnrec_dropout_mask_host: null output");
  const DropParams dp = drop_params(p);
  const uint64_t key = drop_key(seed, step, stream);
  const int Q = (int)((d + 3) / 4);
  for (int64_t r = 0; r < n_rows; ++r)
    for (int q = 0; q < Q; ++q) {
      const uint64_t word = drop_word(key, r, Q, q);
      for (int v = 0; v < 4 && q * 4 + v < d; ++v)
        keep[r * d + q * 4 + v] = drop_keep(word, v, dp.T) ? 1 : 0;
    }
  return GNNREC_OK;
}

extern "C" float gnnrec_dropout_scale(double p) { return gnnrec::drop_params(p).scale; }

extern "C" int gnnrec_dropout_keys(uint64_t seed, int64_t* counter, int64_t stream0,
                                   int64_t n_streams, uint64_t* keys, void* stream) {
  using namespace gnnrec;
  GNNREC_REQUIRE(n_streams >= 0 && n_streams <= (1 << 20) && stream0 >= 0,
                 "gnnrec_dropout_keys: bad stream range");
  GNNREC_REQUIRE(counter && (keys || n_streams == 0), "gnnrec_dropout_keys: null pointer");
  hipLaunchKernelGGL(drop_keys_kernel, dim3(1), dim3(256), 0, as_stream(stream), seed, counter,
                     stream0, (int)n_streams, keys);
  return check_launch("gnnrec_dropout_keys");
}

extern "C" int gnnrec_dropout_rows_f32(const float* x, int64_t ldx, int64_t n, int64_t d,
                                       const uint64_t* keys, int64_t key_index, double p,
                                       int accumulate, float* out, int64_t ldo, void* stream) {
  using namespace gnnrec;
  GNNREC_REQUIRE(n >= 0 && d >= 0 && d <= (1 << 20), "gnnrec_dropout_rows_f32: bad size");
  GNNREC_REQUIRE(p >= 0.0 && p <= 1.0, "gnnrec_dropout_rows_f32: p=%g outside [0, 1]", p);
  GNNREC_REQUIRE(key_index >= 0 && key_index < (1 << 30), "gnnrec_dropout_rows_f32: bad key index");
  if (n == 0 || d == 0) return GNNREC_OK;
  GNNREC_REQUIRE(x && out && keys, "gnnrec_dropout_rows_f32: null pointer");
  GNNREC_REQUIRE(ldx >= d && ldo >= d, "gnnrec_dropout_rows_f32: leading dimension < d");
  const DropParams dp = drop_params(p);
  const int Q = (int)((d + 3) / 4);
  const DropArgs da{keys, (int)key_index, dp.T, dp.scale, Q};
  int64_t blocks = (n * Q + 255) / 256;
  if (blocks > 8192) blocks = 8192;
  hipLaunchKernelGGL(drop_rows_kernel, dim3((unsigned)blocks), dim3(256), 0, as_stream(stream), x,
                     ldx, n, (int)d, accumulate, out, ldo, da);
  return check_launch("gnnrec_dropout_rows_f32");
}

extern "C" int gnnrec_spmm_csr_dropout_live_f32(const int64_t* indptr, const int32_t* indices,
                                                const float* ew, const float* X, int64_t ldx,
                                                int64_t n_dst, int64_t d, int reduce, int flags,
                                                float* out, int64_t ldo, const int64_t* live,
                                                const uint64_t* keys, int64_t key_index,
                                                double p, int where, void* stream) {
  gnnrec::DropSpmm a{indptr, indices, ew, X, ldx, n_dst, 0, out, ldo, flags,
                     0, nullptr, 0, 0, nullptr, live, {}};
  return gnnrec::drop_spmm_entry(a, d, reduce, keys, key_index, p, where, stream);
}

extern "C" int gnnrec_spmm_csr_planned_dropout_live_f32(
    const int64_t* indptr, const int32_t* indices, const float* ew, const float* X, int64_t ldx,
    int64_t n_dst, int64_t d, int reduce, int flags, float* out, int64_t ldo, int64_t split,
    const int64_t* plan, int64_t cap_h, int64_t cap_c, float* workspace, const int64_t* live,
    const uint64_t* keys, int64_t key_index, double p, int where, void* stream) {
  GNNREC_REQUIRE(plan && cap_h > 0 && cap_c > 0,
                 "gnnrec_spmm_csr_planned_dropout_f32: empty plan");
  gnnrec::DropSpmm a{indptr, indices, ew, X, ldx, n_dst, 0, out, ldo, flags,
                     split, plan, cap_h, cap_c, workspace, live, {}};
  return gnnrec::drop_spmm_entry(a, d, reduce, keys, key_index, p, where, stream);
}
