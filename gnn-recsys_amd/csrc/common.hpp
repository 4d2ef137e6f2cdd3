// Shared helpers for the gnnrec HIP library (gfx950 / CDNA4 only).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>
#include <cstdarg>
#include <initializer_list>
#include <type_traits>

#include "gnnrec.h"

namespace gnnrec {

void set_error(const char* fmt, ...);

inline hipStream_t as_stream(void* s) { return reinterpret_cast<hipStream_t>(s); }

inline int check_launch(const char* what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    set_error("%s: kernel launch failed: %s", what, hipGetErrorString(e));
    return GNNREC_EHIP;
  }
  return GNNREC_OK;
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// A launch's run-time mode as a compile-time constant: f(std::bool_constant<b>{}) and
// f(std::integral_constant<int, reduce>{}), reduce one of GNNREC_REDUCE_SUM / _MEAN / _MAX
// (validated by the caller).  Nested, they pick one instantiation of a kernel template.
template <class F>
inline void dispatch_bool(bool b, F&& f) {
  if (b) f(std::true_type{});
  else f(std::false_type{});
}
template <class F>
inline void dispatch_reduce(int reduce, F&& f) {
  if (reduce == GNNREC_REDUCE_SUM) f(std::integral_constant<int, GNNREC_REDUCE_SUM>{});
  else if (reduce == GNNREC_REDUCE_MEAN) f(std::integral_constant<int, GNNREC_REDUCE_MEAN>{});
  else f(std::integral_constant<int, GNNREC_REDUCE_MAX>{});
}

// CDNA4 wavefront is 64 lanes.
constexpr int kWave = 64;

// Lane group g (of NPW groups of kWave / NPW consecutive lanes) receives lane (base + g)'s x,
// base wave-uniform: NPW v_readlane (VALU -> SGPR) and selects, where __shfl is one
// ds_bpermute through the LDS pipe per call.  Lane indices wrap at 64 (a group whose lane
// is past the data ignores the value).
template <int NPW>
__device__ __forceinline__ int bcast_groups(int x, int base, int grp) {
  int r = __builtin_amdgcn_readlane(x, base & 63);
#pragma unroll
  for (int g = 1; g < NPW; ++g) {
    const int y = __builtin_amdgcn_readlane(x, (base + g) & 63);
    r = grp == g ? y : r;
  }
  return r;
}
template <int NPW>
__device__ __forceinline__ float bcast_groups(float x, int base, int grp) {
  return __builtin_bit_cast(float, bcast_groups<NPW>(__builtin_bit_cast(int, x), base, grp));
}

// 64-bit counter hash (splitmix64 finaliser): the synthetic generator and the
// Philox-free fanout sampler both key on it; oracle/oracle.c restates it.
__host__ __device__ inline uint64_t mix64(uint64_t z) {
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
__host__ __device__ inline uint64_t hash3(uint64_t seed, uint64_t a, uint64_t b) {
  return mix64(mix64(seed ^ mix64(a)) ^ (b * 0xD1B54A32D192ED03ull));
}

}  // namespace gnnrec

#define GNNREC_REQUIRE(cond, ...)        \
  do {                                   \
    if (!(cond)) {                       \
      ::gnnrec::set_error(__VA_ARGS__);  \
      return GNNREC_EINVAL;              \
    }                                    \
  } while (0)

namespace gnnrec {

// What the four fused aggregate+project entries (spmm_project.hip, spmm_pair_mfma.hip) check
// alike; `name` is the entry's, so every message keeps its prefix.  d, the epilogue bits,
// the accumulate mode (one relation: attention takes attn_vec and attn_state) or the combine
// (two relations: attn_vec goes with GNNREC_ACC_ATTN_LAST), n_dst; then, unless the problem
// is empty (the entry returns GNNREC_OK): `need` non-null, the tables `rows16` 16-B aligned
// (a null one is optional) with row strides `ld4` multiples of 4, out 8-B aligned.  `table`:
// the source table's letter in the message.
inline int fused_check(const char* name, int64_t d, int epilogue, bool two_relations, int mode,
                       const void* attn_vec, const void* attn_state, int64_t n_dst, char table,
                       std::initializer_list<const void*> need,
                       std::initializer_list<const void*> rows16,
                       std::initializer_list<int64_t> ld4, const float* out, int64_t ldo) {
  GNNREC_REQUIRE(d == 128, "%s: only d = %d (got %lld)", name, 128, (long long)d);
  GNNREC_REQUIRE((epilogue & ~(GNNREC_EPI_RELU | GNNREC_EPI_L2NORM)) == 0,
                 "%s: epilogue must be RELU|L2NORM", name);
  if (two_relations) {
    GNNREC_REQUIRE(mode == GNNREC_ACC_ADD || mode == GNNREC_ACC_MAX ||
                       mode == GNNREC_ACC_ATTN_LAST,
                   "%s: combine must be GNNREC_ACC_ADD, _MAX or _ATTN_LAST", name);
    GNNREC_REQUIRE((mode == GNNREC_ACC_ATTN_LAST) == (attn_vec != nullptr),
                   "%s: attn_vec goes with combine GNNREC_ACC_ATTN_LAST", name);
  } else {
    GNNREC_REQUIRE(mode >= GNNREC_ACC_STORE && mode <= GNNREC_ACC_ATTN_LAST,
                   "%s: unknown accumulate mode %d", name, mode);
    GNNREC_REQUIRE(mode < GNNREC_ACC_ATTN_FIRST || (attn_vec && attn_state),
                   "%s: attention accumulation needs attn_vec, attn_state", name);
  }
  GNNREC_REQUIRE(n_dst >= 0, "%s: negative n_dst", name);
  if (n_dst == 0) return GNNREC_OK;
  bool have = out != nullptr, ok = ldo % 2 == 0 && (reinterpret_cast<uintptr_t>(out) & 7u) == 0;
  for (const void* p : need) have = have && p != nullptr;
  for (const void* p : rows16) ok = ok && aligned16(p);
  for (const int64_t ld : ld4) ok = ok && ld % 4 == 0;
  GNNREC_REQUIRE(have, "%s: null pointer", name);
  GNNREC_REQUIRE(ok, "%s: %c/H/W need 16-B aligned rows, out 8-B", name, table);
  return GNNREC_OK;
}

}  // namespace gnnrec
