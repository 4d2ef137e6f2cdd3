// The popularity-weighted rating (f1d), the one place it is computed:
//
//   p_v     = popularity[v] * weight_popularity      one fp32 multiply, once per call
//   E(u,v)  = expf(score(u,v))                        score: the bits recommend() ranks by
//   Z_u     = sum over ALL items v of expf(g(u,v))    fixed order (recommend_pop.hip)
//   R(u,v)  = E(u,v) / Z_u + p_v                      expf, one IEEE divide, one add, each
//                                                     rounded separately
//
// the reference's softmax(ratings) + popularity * weight (src/metrics.py:69-72) without the
// max-subtraction: both heads' scores are bounded (cosine <= 1, sigmoid < 1), so it protects
// nothing, and the quotient is the same real number.  Every kernel that produces an R — the
// bf16 scorer's rating epilogues (of the approximate score), the candidate rescoring and the
// exhaustive rows' transform — calls rating(): "bitwise equal" between them holds by
// construction.  The library is built without fast-math; __fdiv_rn / __fadd_rn and the
// contraction pragma keep the divide a divide (no reciprocal multiply) and the add unfused
// under any flags.
#pragma once
#include "common.hpp"

namespace gnnrec {

__device__ __forceinline__ float rating(float score, float Z, float p) {
#pragma clang fp contract(off)
  const float e = expf(score);
  const float q = __fdiv_rn(e, Z);
  return __fadd_rn(q, p);
}

}  // namespace gnnrec
