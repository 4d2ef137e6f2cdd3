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

}  // namespace gnnrec
