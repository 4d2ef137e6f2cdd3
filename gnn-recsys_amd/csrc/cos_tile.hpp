// The fp32 MFMA tile loop over all items shared by the rating denominators
// (recommend_pop.hip) and the full-ranking count pass (rank.hip): one block owns (one partial
// of kZItems consecutive items, one 128-row tile of A), every kernel supplies what is done
// with a finished 128 x 32 score subtile (the epilogue) and what becomes of the per-row
// registers it kept.
//
// THE LOOP.  256 threads, four waves.  The block's 128 A rows are staged once into LDS
// (64 KB: 128 rows x 128 columns, 16-B chunks xor-swizzled by the row so that the 16 lanes of
// a ds_read_b128 phase fall into distinct bank groups without padding; wider tables are
// staged 128 columns at a time) and every wave multiplies all of them (4 x 32 rows, 64
// accumulator registers) with a 32-item subtile whose rows it loads straight from the table,
// 16 B per lane and k-step: wave w takes the subtiles 4 t + w, t ascending.  Both tables are
// stored with each group of 8 columns permuted to [0, 2, 4, 6, 1, 3, 5, 7]
// (normalize_rows_f32): lane half h's 16-B load at 8 s + 4 h then holds k = 8 s + h + 2 j,
// j = 0..3 — the operand of the j-th of four consecutive MFMAs (v_mfma_f32_32x32x2_f32),
// k ascending.  Rows and items past the end read a clamped (valid) row: the epilogue is not
// called for an item past the end, and rows past the end are the kernel's to mask.
//
// C layout of a subtile: col = lane & 31, row = 32 i + (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
// for acc[i][reg].
#pragma once
#include "common.hpp"

namespace gnnrec {

constexpr int kZItems = 1024;  // items per partial
constexpr int kZK = 128;       // columns staged at a time
constexpr int kZMaxD = 2048;

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

// sA: 128 * 32 f32x4 of LDS.  epi(acc, c): the lane's column c < n of a finished subtile.
template <class Epi>
__device__ __forceinline__ void cos_tile_loop(const float* __restrict__ U, int64_t B,
                                              const float* __restrict__ V, int64_t n, int dpad,
                                              int64_t ut, int64_t pi, f32x4* sA, Epi&& epi) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l31 = lane & 31, h = lane >> 5;
  const int nkc = (dpad + kZK - 1) / kZK;
  for (int it = 0; it < kZItems / 128; ++it) {
    if (pi * kZItems + (int64_t)it * 128 >= n) break;  // block-uniform: nothing left to add
    const int64_t c = pi * kZItems + (int64_t)(it * 4 + wave) * 32 + l31;
    const float* pb = V + min(c, n - 1) * dpad + 4 * h;
    f32x16 acc[4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;
    for (int kc = 0; kc < nkc; ++kc) {
      const int k0 = kc * kZK;
      const int ks = min(kZK, dpad - k0) / 8;  // dpad % 8 == 0
      if (nkc > 1 || it == 0) {  // block-uniform
        __syncthreads();         // the previous chunk's reads are done
#pragma unroll 4
        for (int p = 0; p < 16; ++p) {
          const int idx = tid + p * 256, row = idx >> 5, ch = idx & 31;
          const int64_t r = min(ut * 128 + row, B - 1);  // past the end: a valid row, masked later
          f32x4 v = {0.f, 0.f, 0.f, 0.f};
          if (k0 + ch * 4 < dpad) v = *reinterpret_cast<const f32x4*>(U + r * dpad + k0 + ch * 4);
          sA[row * 32 + (ch ^ (row & 31))] = v;
        }
        __syncthreads();
      }
      // the item rows, 8 k-steps (256 B a row) at a time: every load of a half in flight
      // before its first MFMA needs one
#pragma unroll
      for (int half = 0; half < 2; ++half) {
        f32x4 b[8];
#pragma unroll
        for (int s = 0; s < 8; ++s)
          if (half * 8 + s < ks) b[s] = *reinterpret_cast<const f32x4*>(pb + k0 + 64 * half + 8 * s);
#pragma unroll
        for (int s = 0; s < 8; ++s) {
          if (half * 8 + s < ks) {  // wave-uniform
            f32x4 a[4];
#pragma unroll
            for (int i = 0; i < 4; ++i)
              a[i] = sA[(i * 32 + l31) * 32 + ((2 * (half * 8 + s) + h) ^ l31)];
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
              for (int i = 0; i < 4; ++i)
                acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i][j], b[s][j], acc[i], 0, 0, 0);
          }
        }
      }
    }
    if (c < n) epi(acc, c);
  }
}

// The per-row registers rs[i][reg] (one per row of the C layout, summed by the lane over its
// columns) folded to one value per row and written to part[pi * B + row]: the 32 lanes of a
// row by an xor tree (offsets 1, 2, 4, 8, 16), the four waves in the order
// ((w0 + w1) + w2) + w3.  red: 512 T of LDS — the staged rows' own storage, which every wave
// has finished reading after the barrier.
template <class T>
__device__ __forceinline__ void fold_tile_rows(const T (&rs)[4][16], T* red, int64_t B, int64_t ut,
                                               int64_t pi, T* __restrict__ part) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l31 = lane & 31, h = lane >> 5;
  __syncthreads();  // every wave's reads of the staged rows are done: sA becomes the sums
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      T x = rs[i][r];
#pragma unroll
      for (int off = 1; off < 32; off <<= 1) x += __shfl_xor(x, off);
      if (l31 == 0) red[wave * 128 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * h] = x;
    }
  __syncthreads();
  const int64_t row = ut * 128 + tid;
  if (tid < 128 && row < B)
    part[pi * B + row] = ((red[tid] + red[128 + tid]) + red[256 + tid]) + red[384 + tid];
}

}  // namespace gnnrec
