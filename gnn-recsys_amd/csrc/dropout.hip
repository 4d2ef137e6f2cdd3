// Dropout of the training layers (reference src/model.py:140-141: ConvLayer.forward applies
// dropout_fn to h_neigh and h_self) without a stored mask or a dropped copy of a source
// table: the mask is the counter-based function of dropout.hpp, regenerated where it is
// needed.  This file owns the mask's own entry points:
//
//   * the host mask and the scale (what every masking kernel regenerates);
//   * self side: x ⊙ mask · scale over the first n rows of a table (stored or accumulated);
//   * the keys of one forward call from a device-resident step counter, which the same
//     launch advances: a replayed graph draws a new mask on every replay.
//
// The neighbour side — the sum / mean gather with the mask of the GATHERED row on every
// fragment (GNNREC_DROPOUT_SRC, the forward) or of the OUTPUT row at its store
// (GNNREC_DROPOUT_OUT, the backward) — is the aggregation family of spmm.hip under its
// dropout policy (gnnrec_spmm_csr_dropout_live_f32 and the planned form live there).
#include "common.hpp"
#include "dropout.hpp"

namespace gnnrec {
namespace {

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
