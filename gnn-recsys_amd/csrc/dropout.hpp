// The counter-based dropout mask of the training layers: a pure function of
// (seed, step, stream, row, column), the same on the host and on the device, so a mask is
// regenerated wherever it is needed (the forward gather, the backward's store) and never
// stored.  Built on mix64 / hash3 (common.hpp), which the fanout sampler keys on as well.
//
//   key        = hash3(seed, step, stream)
//   word(r, q) = mix64(key ^ (r * Q + q)),  Q = ceil(d / 4)
//   bits(r, c) = (word(r, c / 4) >> 16 * (c % 4)) & 0xFFFF
//   T          = round(p * 65536) (ties to even), clamped to [0, 65536]
//   keep(r, c) = bits(r, c) >= T;  kept elements are multiplied by 65536 / (65536 - T)
//
// so the keep probability is exactly 1 - T / 65536 and the expectation of a dropped row is
// the row.  One word serves the four columns of a 16-byte load.
#pragma once
#include <cmath>
#include <cstdint>

#include "common.hpp"
#include "gather.hpp"

namespace gnnrec {

struct DropParams {
  uint32_t T;   // drop threshold on the 16-bit draw
  float scale;  // 65536 / (65536 - T); 0 when everything is dropped
};

inline DropParams drop_params(double p) {
  double t = std::nearbyint(p * 65536.0);
  if (!(t > 0.0)) t = 0.0;
  if (t > 65536.0) t = 65536.0;
  DropParams r;
  r.T = (uint32_t)t;
  r.scale = r.T >= 65536u ? 0.f : 65536.0f / (float)(65536u - r.T);
  return r;
}

__host__ __device__ inline uint64_t drop_key(uint64_t seed, uint64_t step, uint64_t stream) {
  return hash3(seed, step, stream);
}

__host__ __device__ inline uint64_t drop_word(uint64_t key, int64_t row, int Q, int q) {
  return mix64(key ^ ((uint64_t)row * (uint64_t)Q + (uint64_t)q));
}

__host__ __device__ inline bool drop_keep(uint64_t word, int c, uint32_t T) {
  return (uint32_t)((word >> (16 * (c & 3))) & 0xFFFFu) >= T;
}

// what a kernel that masks needs (dropout.hip's row kernel, spmm.hip's gathers)
struct DropArgs {
  const uint64_t* keys;  // device: one key per stream of the forward call
  int index;             // this launch's stream
  uint32_t T;
  float scale;
  int Q;  // words per row: ceil(d / 4)
};

namespace {

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

// gather_range's hook (gather.hpp): the mask of each gathered source row
struct DropSrcMask {
  static constexpr bool kOn = true;
  uint64_t key;
  uint32_t T;
  int Q;
  __device__ __forceinline__ uint64_t word(int src, int col) const {
    return drop_word(key, src, Q, col >> 2);
  }
  template <int VEC>
  __device__ __forceinline__ void apply(Frag<VEC>& f, uint64_t w, int col) const {
    drop_frag<VEC>(f, w, col, T);
  }
};

}  // namespace
}  // namespace gnnrec
