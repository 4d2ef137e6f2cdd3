// The lane arithmetic of the cosine score (a7, gnnrec_sddmm_cos_f32), shared by every kernel
// that must return that kernel's bits: the per-edge and grouped kernels of heads.hip and the
// candidate rescoring of recommend.hip.
#pragma once
#include "common.hpp"

namespace gnnrec {

// one lane's 4-column partial of <a, b>, the fma chain written out: the per-edge and the
// grouped kernel must round every score the same way (left to the compiler's contraction,
// the same source expression fused differently in the two kernels: 1-ulp differences)
__device__ __forceinline__ float dot4(const float4& a, const float4& b) {
  return fmaf(a.w, b.w, fmaf(a.z, b.z, fmaf(a.y, b.y, a.x * b.x)));
}

// Sum over a lane group of LPR (16, 32 or 64) lanes by DPP adds — VALU only, where a
// __shfl_xor tree is one ds_bpermute per level — valid in the group's LAST lane.  Each level
// adds the same two partial sums the xor tree adds (quad_perm [1,0,3,2] / [2,3,0,1] pair the
// xor-1 / xor-2 partners; after them a quad's lanes agree, so row_half_mirror and row_mirror
// add the xor-4 / xor-8 partner's value; row_bcast15 / 31 add the lower row's / half's sum
// to the upper one): the bits of the xor tree, which the u-norm reductions still use.
template <int CTRL, int ROWS>
__device__ __forceinline__ float dpp_add(float x) {
  const int y = __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), CTRL, ROWS, 0xF, false);
  return x + __builtin_bit_cast(float, y);
}

template <int LPR>
__device__ __forceinline__ float group_sum_last(float x) {
  static_assert(LPR == 16 || LPR == 32 || LPR == 64, "lane groups of 16, 32 or 64");
  x = dpp_add<0xB1, 0xF>(x);   // quad_perm [1,0,3,2]
  x = dpp_add<0x4E, 0xF>(x);   // quad_perm [2,3,0,1]
  x = dpp_add<0x141, 0xF>(x);  // row_half_mirror
  x = dpp_add<0x140, 0xF>(x);  // row_mirror
  if constexpr (LPR >= 32) x = dpp_add<0x142, 0xA>(x);  // row_bcast15 into rows 1 and 3
  if constexpr (LPR >= 64) x = dpp_add<0x143, 0xC>(x);  // row_bcast31 into rows 2 and 3
  return x;
}

// The cosine of rows pu and pv (d % 4 == 0, 16-B aligned) over a group of LPR lanes, lane gl
// of the group taking columns 4 gl, 4 gl + 4 LPR, ...: sddmm_cos_kernel<LPR, 4>'s value,
// valid in the group's last lane.  ok = false lanes add zeros (every lane of the wave must
// call it: the DPP sums read their neighbours).
template <int LPR>
__device__ __forceinline__ float cos_pair_vec4(const float* pu, const float* pv, int d, int gl,
                                               bool ok) {
  float dot = 0.f, su = 0.f, sv = 0.f;
  if (ok) {
    for (int c = gl * 4; c < d; c += LPR * 4) {
      const float4 a = *reinterpret_cast<const float4*>(pu + c);
      const float4 b = *reinterpret_cast<const float4*>(pv + c);
      dot += dot4(a, b);
      su += dot4(a, a);
      sv += dot4(b, b);
    }
  }
  dot = group_sum_last<LPR>(dot);
  su = group_sum_last<LPR>(su);
  sv = group_sum_last<LPR>(sv);
  const float nu = fmaxf(sqrtf(su), 1e-12f);
  const float nv = fmaxf(sqrtf(sv), 1e-12f);
  return dot / (nu * nv);
}

}  // namespace gnnrec
