// The fold of the full-ranking count passes' int32 partials (rank.hip's cosine pass and
// heads.hip's MLP pass): out[r] = sum over p of part[p, r].  Integers: the
// order does not matter, and nothing is added atomically.
#pragma once
#include "common.hpp"

namespace gnnrec {
namespace {

__global__ __launch_bounds__(256) void fold_partials_i32_kernel(const int* __restrict__ part,
                                                                int64_t n_part, int64_t B,
                                                                int* __restrict__ out) {
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (r >= B) return;
  int z = 0;
  for (int64_t p = 0; p < n_part; ++p) z += part[p * B + r];
  out[r] = z;
}

// B >= 1 and (B + 255) / 256 < 2^31, checked by the caller
inline int launch_fold_partials_i32(const char* fn, const int* part, int64_t n_part, int64_t B,
                                    int* out, hipStream_t s) {
  hipLaunchKernelGGL(fold_partials_i32_kernel, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, s,
                     part, n_part, B, out);
  return check_launch(fn);
}

}  // namespace
}  // namespace gnnrec
