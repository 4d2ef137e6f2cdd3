// torch_ops.cpp — TORCH_LIBRARY(gnnrec) over the C ABI of libgnnrec.so (include/gnnrec.h).
//
// Every op is a thin, validated wrapper of one C-ABI entry point: device pointers and the
// current HIP stream of the operand's device in, the library's status out (GNNREC_EINVAL
// -> ValueError, anything else -> RuntimeError with gnnrec_last_error()).  Outputs are
// preallocated by the caller and declared mutable in the schema (Tensor(a!)), the same
// contract as the C ABI, so torch.compile functionalises them (auto_functionalize).  The
// Meta kernel of each op is the same function: on meta /
// fake tensors it runs the shape checks and returns before the launch, which is all that
// shape inference of an op with mutated outputs needs.
//
// Reference call sites these ops serve (the nn.Module drop-ins in gnnrec/nn.py):
//   spmm_csr*, spmm_project, gemm   <- ConvLayer.forward src/model.py:143-208,226-235
//   sddmm_cos                       <- CosinePrediction.forward src/model.py:317-327
//   edge_mlp                        <- PredictingModule.forward src/model.py:290-305
//   edge_mlp_grouped                <- the same over negative_sampler.Uniform's pair graphs
//   edge_mlp_dense_store / _filter  <- the same for every (user, item) pair: get_recs(pred='nn')
//                                      src/metrics.py:31-78 and recs.recommend(head=...)
// The sampler and loader ops (sample_*, scan, relabel, gathers) are in torch_sampler.cpp.
#include <algorithm>
#include <utility>
#include <vector>

#include "torch_common.hpp"

namespace {

using namespace gnnrec_torch;

// ---------------------------------------------------------------- a1 aggregation
// live (nullable, one device int64): rows from it on are empty rows (gnnrec_spmm_csr_live_f32)
const int64_t* live_ptr(const optional<Tensor>& live) {
  if (!has(live)) return nullptr;
  dev(live, "live", at::kLong);
  TORCH_CHECK_VALUE(live->numel() == 1, "live must hold one row count");
  return p<int64_t>(live);
}

void spmm_csr(const Tensor& indptr, const Tensor& indices, const optional<Tensor>& ew,
              const Tensor& X, int64_t reduce, int64_t flags, Tensor& out,
              const optional<Tensor>& live) {
  const OneDevice one_device_;
  dev(indptr, "indptr", at::kLong);
  dev(indices, "indices", at::kInt);
  dev(X, "X", at::kFloat);
  dev(ew, "edge_weight", at::kFloat);
  dev(out, "out", at::kFloat);
  const int64_t n_dst = indptr.numel() - 1, d = X.size(1);
  TORCH_CHECK_VALUE(out.size(0) == n_dst && out.size(1) == d, "out must be [", n_dst, ", ", d,
                    "], got ", out.sizes());
  const int64_t ldx = ld(X, "X"), ldo = ld(out, "out");
  if (meta(X)) return;
  const c10::DeviceGuard g(X.device());
  ck(gnnrec_spmm_csr_live_f32(p<int64_t>(indptr), p<int32_t>(indices), p<float>(ew), p<float>(X),
                              ldx, n_dst, d, (int)reduce, (int)flags, p<float>(out), ldo,
                              live_ptr(live), stream_of(X)),
     "gnnrec_spmm_csr_f32");
}

void spmm_csr_split(const Tensor& indptr, const Tensor& indices, const optional<Tensor>& ew,
                    const Tensor& X, int64_t reduce, int64_t flags, int64_t split,
                    const Tensor& heavy, const Tensor& chunk_ptr, const Tensor& chunk_row,
                    int64_t n_chunks, Tensor& out, Tensor& ws) {
  const OneDevice one_device_;
  dev(indptr, "indptr", at::kLong);
  dev(indices, "indices", at::kInt);
  dev(X, "X", at::kFloat);
  dev(ew, "edge_weight", at::kFloat);
  dev(heavy, "heavy_rows", at::kLong);
  dev(chunk_ptr, "chunk_ptr", at::kLong);
  dev(chunk_row, "chunk_row", at::kLong);
  dev(out, "out", at::kFloat);
  dev(ws, "workspace", at::kFloat);
  const int64_t n_dst = indptr.numel() - 1, d = X.size(1);
  TORCH_CHECK_VALUE(out.size(0) == n_dst && out.size(1) == d, "out must be [", n_dst, ", ", d, "]");
  TORCH_CHECK_VALUE(ws.numel() >= n_chunks * d, "workspace must hold n_chunks x d floats");
  const int64_t ldx = ld(X, "X"), ldo = ld(out, "out");
  if (meta(X)) return;
  const c10::DeviceGuard g(X.device());
  ck(gnnrec_spmm_csr_split_f32(p<int64_t>(indptr), p<int32_t>(indices), p<float>(ew), p<float>(X),
                               ldx, n_dst, d, (int)reduce, (int)flags, p<float>(out), ldo, split,
                               p<int64_t>(heavy), heavy.numel(), p<int64_t>(chunk_ptr),
                               p<int64_t>(chunk_row), n_chunks, p<float>(ws), stream_of(X)),
     "gnnrec_spmm_csr_split_f32");
}

void spmm_csr2(const Tensor& indptr_a, const Tensor& indices_a, const optional<Tensor>& ew_a,
               const Tensor& indptr_b, const Tensor& indices_b, const optional<Tensor>& ew_b,
               const Tensor& X, int64_t reduce, int64_t flags, Tensor& out_a, Tensor& out_b) {
  const OneDevice one_device_;
  dev(indptr_a, "indptr_a", at::kLong);
  dev(indices_a, "indices_a", at::kInt);
  dev(ew_a, "ew_a", at::kFloat);
  dev(indptr_b, "indptr_b", at::kLong);
  dev(indices_b, "indices_b", at::kInt);
  dev(ew_b, "ew_b", at::kFloat);
  dev(X, "X", at::kFloat);
  dev(out_a, "out_a", at::kFloat);
  dev(out_b, "out_b", at::kFloat);
  const int64_t n_dst = indptr_a.numel() - 1, d = X.size(1);
  TORCH_CHECK_VALUE(indptr_b.numel() == n_dst + 1, "spmm_csr2: the relations' row counts differ");
  TORCH_CHECK_VALUE(out_a.size(0) == n_dst && out_a.size(1) == d && out_b.sizes() == out_a.sizes(),
                    "out_a / out_b must be [", n_dst, ", ", d, "]");
  const int64_t ldx = ld(X, "X"), ldo = ld(out_a, "out_a");
  TORCH_CHECK_VALUE(ld(out_b, "out_b") == ldo, "out_a and out_b must share a row stride");
  if (meta(X)) return;
  const c10::DeviceGuard g(X.device());
  ck(gnnrec_spmm_csr2_f32(p<int64_t>(indptr_a), p<int32_t>(indices_a), p<float>(ew_a),
                          p<int64_t>(indptr_b), p<int32_t>(indices_b), p<float>(ew_b), p<float>(X),
                          ldx, n_dst, d, (int)reduce, (int)flags, p<float>(out_a), p<float>(out_b),
                          ldo, stream_of(X)),
     "gnnrec_spmm_csr2_f32");
}

void spmm_plan_build(const Tensor& indptr, int64_t split, int64_t cap_h, Tensor& plan,
                     const optional<Tensor>& live) {
  const OneDevice one_device_;
  dev(indptr, "indptr", at::kLong);
  dev(plan, "plan", at::kLong);
  const int64_t cap_c = plan.numel() - (3 + 2 * cap_h);  // plan = {2 | cap_h | cap_h+1 | cap_c}
  TORCH_CHECK_VALUE(cap_h >= 0 && cap_c >= 0, "spmm_plan_build: plan shorter than 3 + 2 cap_h");
  if (meta(indptr)) return;
  const c10::DeviceGuard g(indptr.device());
  ck(gnnrec_spmm_plan_build_live(p<int64_t>(indptr), indptr.numel() - 1, split, cap_h, cap_c,
                                 p<int64_t>(plan), live_ptr(live), stream_of(indptr)),
     "gnnrec_spmm_plan_build");
}

void spmm_csr_planned(const Tensor& indptr, const Tensor& indices, const optional<Tensor>& ew,
                      const Tensor& X, int64_t reduce, int64_t flags, int64_t split,
                      const Tensor& plan, int64_t cap_h, int64_t cap_c, Tensor& out, Tensor& ws,
                      const optional<Tensor>& live) {
  const OneDevice one_device_;
  dev(indptr, "indptr", at::kLong);
  dev(indices, "indices", at::kInt);
  dev(X, "X", at::kFloat);
  dev(ew, "edge_weight", at::kFloat);
  dev(plan, "plan", at::kLong);
  dev(out, "out", at::kFloat);
  dev(ws, "workspace", at::kFloat);
  const int64_t n_dst = indptr.numel() - 1, d = X.size(1);
  TORCH_CHECK_VALUE(out.size(0) == n_dst && out.size(1) == d, "out must be [", n_dst, ", ", d, "]");
  TORCH_CHECK_VALUE(ws.numel() >= cap_c * d, "workspace must hold cap_c x d floats");
  const int64_t ldx = ld(X, "X"), ldo = ld(out, "out");
  if (meta(X)) return;
  const c10::DeviceGuard g(X.device());
  ck(gnnrec_spmm_csr_planned_live_f32(p<int64_t>(indptr), p<int32_t>(indices), p<float>(ew),
                                      p<float>(X), ldx, n_dst, d, (int)reduce, (int)flags,
                                      p<float>(out), ldo, split, p<int64_t>(plan), cap_h, cap_c,
                                      p<float>(ws), live_ptr(live), stream_of(X)),
     "gnnrec_spmm_csr_planned_f32");
}

void spmm_backward(const Tensor& indptr, const Tensor& indices, const optional<Tensor>& ew,
                   const Tensor& grad_out, const optional<Tensor>& X,
                   const optional<Tensor>& out, int64_t reduce, Tensor& grad_X) {
  const OneDevice one_device_;
  dev(indptr, "indptr", at::kLong);
  dev(indices, "indices", at::kInt);
  dev(ew, "edge_weight", at::kFloat);
  dev(grad_out, "grad_out", at::kFloat);
  dev(X, "X", at::kFloat);
  dev(out, "out", at::kFloat);
  dev(grad_X, "grad_X", at::kFloat);
  const int64_t n_dst = grad_out.size(0), d = grad_out.size(1);
  const int64_t ldg = ld(grad_out, "grad_out"), ldgx = ld(grad_X, "grad_X");
  const int64_t ldx = has(X) ? ld(*X, "X") : 0, ldo = has(out) ? ld(*out, "out") : 0;
  if (meta(grad_out)) return;
  const c10::DeviceGuard g(grad_out.device());
  ck(gnnrec_spmm_backward_f32(p<int64_t>(indptr), p<int32_t>(indices), p<float>(ew),
                              p<float>(grad_out), ldg, p<float>(X), ldx, p<float>(out), ldo,
                              n_dst, d, (int)reduce, p<float>(grad_X), ldgx, stream_of(grad_out)),
     "gnnrec_spmm_backward_f32");
}

// ---------------------------------------------------------------- a2-a4 projections
void gemm(const Tensor& A1, const Tensor& W1, const optional<Tensor>& A2,
          const optional<Tensor>& W2, const optional<Tensor>& a2_deg, int64_t a2_mode,
          const optional<Tensor>& bias, const optional<Tensor>& bias_nonempty, int64_t epilogue,
          int64_t accum, double out_div, const optional<Tensor>& attn_vec,
          const optional<Tensor>& attn_state, Tensor& out, const optional<Tensor>& row_norm) {
  const OneDevice one_device_;
  dev(A1, "A1", at::kFloat);
  dev(W1, "W1", at::kFloat);
  dev(A2, "A2", at::kFloat);
  dev(W2, "W2", at::kFloat);
  dev(a2_deg, "a2_deg", at::kInt);
  dev(bias, "bias", at::kFloat);
  dev(bias_nonempty, "bias_nonempty", at::kFloat);
  dev(attn_vec, "attn_vec", at::kFloat);
  dev(attn_state, "attn_state", at::kFloat);
  dev(out, "out", at::kFloat);
  dev(row_norm, "row_norm", at::kFloat);
  const int64_t M = A1.size(0), K1 = A1.size(1), N = W1.size(0);
  TORCH_CHECK_VALUE(W1.size(1) == K1 && W1.is_contiguous(), "W1 must be a contiguous [N, ", K1, "]");
  const int64_t lda1 = ld(A1, "A1");
  int64_t K2 = 0, lda2 = 1;
  if (has(A2)) {
    TORCH_CHECK_VALUE(has(W2) && A2->size(0) == M && W2->size(0) == N &&
                          W2->size(1) == A2->size(1) && W2->is_contiguous(),
                      "A2/W2 shape mismatch");
    K2 = A2->size(1);
    lda2 = ld(*A2, "A2");
  }
  TORCH_CHECK_VALUE(out.size(0) == M && out.size(1) == N, "out must be [", M, ", ", N, "]");
  const int64_t ldo = ld(out, "out");
  if (meta(A1)) return;
  const c10::DeviceGuard g(A1.device());
  ck(gnnrec_gemm_rownorm_f32(p<float>(A1), lda1, K1, p<float>(W1), p<float>(A2), lda2, K2,
                             p<float>(W2), p<int32_t>(a2_deg), (int)a2_mode, p<float>(bias),
                             p<float>(bias_nonempty), M, N, (int)epilogue, (int)accum,
                             (float)out_div, p<float>(attn_vec), p<float>(attn_state),
                             p<float>(out), ldo, p<float>(row_norm), stream_of(A1)),
     "gnnrec_gemm_f32");
}

void row_epilogue(const Tensor& z, int64_t l2norm, int64_t accum, double out_div,
                  const optional<Tensor>& attn_vec, const optional<Tensor>& attn_state,
                  Tensor& out) {
  const OneDevice one_device_;
  dev(z, "z", at::kFloat);
  dev(attn_vec, "attn_vec", at::kFloat);
  dev(attn_state, "attn_state", at::kFloat);
  dev(out, "out", at::kFloat);
  const int64_t M = z.size(0), N = z.size(1);
  TORCH_CHECK_VALUE(out.size(0) == M && out.size(1) == N, "out must be [", M, ", ", N, "]");
  const int64_t ldz = ld(z, "z"), ldo = ld(out, "out");
  if (meta(z)) return;
  const c10::DeviceGuard g(z.device());
  ck(gnnrec_row_epilogue_f32(p<float>(z), ldz, M, N, (int)l2norm, (int)accum, (float)out_div,
                             p<float>(attn_vec), p<float>(attn_state), p<float>(out), ldo,
                             stream_of(z)),
     "gnnrec_row_epilogue_f32");
}

void spmm_project(const Tensor& indptr, const Tensor& indices, const optional<Tensor>& ew,
                  const Tensor& X, const Tensor& H, const Tensor& W_selfT,
                  const optional<Tensor>& W_neighT, const optional<Tensor>& bias,
                  const optional<Tensor>& bias_nonempty, int64_t reduce, int64_t epilogue,
                  int64_t accum, double out_div, const optional<Tensor>& attn_vec,
                  const optional<Tensor>& attn_state, bool mfma, Tensor& out) {
  const OneDevice one_device_;
  dev(indptr, "indptr", at::kLong);
  dev(indices, "indices", at::kInt);
  dev(ew, "edge_weight", at::kFloat);
  dev(X, "X", at::kFloat);
  dev(H, "H", at::kFloat);
  dev(W_selfT, "W_selfT", at::kFloat);
  dev(W_neighT, "W_neighT", at::kFloat);
  dev(bias, "bias", at::kFloat);
  dev(bias_nonempty, "bias_nonempty", at::kFloat);
  dev(attn_vec, "attn_vec", at::kFloat);
  dev(attn_state, "attn_state", at::kFloat);
  dev(out, "out", at::kFloat);
  const int64_t n_dst = indptr.numel() - 1, d = X.size(1);
  TORCH_CHECK_VALUE(H.size(0) >= n_dst, "H has ", H.size(0), " rows, the CSR ", n_dst,
                    " destinations");
  TORCH_CHECK_VALUE(out.size(0) == n_dst && out.size(1) == d, "out must be [", n_dst, ", ", d, "]");
  TORCH_CHECK_VALUE(W_selfT.is_contiguous() && (!has(W_neighT) || W_neighT->is_contiguous()),
                    "transposed weights must be contiguous");
  TORCH_CHECK_VALUE(has(W_neighT) || mfma, "pre-projected source rows (W_neighT None) need the "
                    "mfma variant");
  const int64_t ldx = ld(X, "X"), ldh = ld(H, "H"), ldo = ld(out, "out");
  if (meta(X)) return;
  const c10::DeviceGuard g(X.device());
  auto fn = mfma ? gnnrec_spmm_project_mfma_f32 : gnnrec_spmm_project_f32;
  ck(fn(p<int64_t>(indptr), p<int32_t>(indices), p<float>(ew), p<float>(X), ldx, p<float>(H), ldh,
        p<float>(W_selfT), p<float>(W_neighT), p<float>(bias), p<float>(bias_nonempty), n_dst, d,
        (int)reduce, (int)epilogue, (int)accum, (float)out_div, p<float>(attn_vec),
        p<float>(attn_state), p<float>(out), ldo, stream_of(X)),
     mfma ? "gnnrec_spmm_project_mfma_f32" : "gnnrec_spmm_project_f32");
}

// the VALU launch that saves (agg_mode 1) or takes (2) the rows' aggregates: agg [n_dst, d];
// a load launch reads neither indices, edge weights nor X (all three optional there)
void spmm_project_agg_f32(const Tensor& indptr, const optional<Tensor>& indices,
                          const optional<Tensor>& ew, const optional<Tensor>& X, const Tensor& H,
                          const Tensor& W_selfT, const Tensor& W_neighT,
                          const optional<Tensor>& bias, const optional<Tensor>& bias_nonempty,
                          int64_t reduce, int64_t epilogue, int64_t accum, double out_div,
                          const optional<Tensor>& attn_vec, const optional<Tensor>& attn_state,
                          Tensor& agg, int64_t agg_mode, Tensor& out) {
  const OneDevice one_device_;
  dev(indptr, "indptr", at::kLong);
  dev(indices, "indices", at::kInt);
  dev(ew, "edge_weight", at::kFloat);
  dev(X, "X", at::kFloat);
  dev(H, "H", at::kFloat);
  dev(W_selfT, "W_selfT", at::kFloat);
  dev(W_neighT, "W_neighT", at::kFloat);
  dev(bias, "bias", at::kFloat);
  dev(bias_nonempty, "bias_nonempty", at::kFloat);
  dev(attn_vec, "attn_vec", at::kFloat);
  dev(attn_state, "attn_state", at::kFloat);
  dev(agg, "agg", at::kFloat);
  dev(out, "out", at::kFloat);
  const int64_t n_dst = indptr.numel() - 1, d = H.size(1);
  TORCH_CHECK_VALUE(agg_mode == GNNREC_AGG_SAVE || agg_mode == GNNREC_AGG_LOAD,
                    "agg_mode must be GNNREC_AGG_SAVE or GNNREC_AGG_LOAD");
  TORCH_CHECK_VALUE(agg_mode == GNNREC_AGG_LOAD || (has(indices) && has(X)),
                    "a saving launch gathers: it needs indices and X");
  TORCH_CHECK_VALUE(!has(X) || X->size(1) == d, "X and H widths differ");
  TORCH_CHECK_VALUE(H.size(0) >= n_dst, "H has ", H.size(0), " rows, the CSR ", n_dst,
                    " destinations");
  TORCH_CHECK_VALUE(out.size(0) == n_dst && out.size(1) == d, "out must be [", n_dst, ", ", d, "]");
  TORCH_CHECK_VALUE(agg.dim() == 2 && agg.size(0) == n_dst && agg.size(1) == d, "agg must be [",
                    n_dst, ", ", d, "]");
  TORCH_CHECK_VALUE(W_selfT.is_contiguous() && W_neighT.is_contiguous(),
                    "transposed weights must be contiguous");
  const int64_t ldx = has(X) ? ld(*X, "X") : 0, ldh = ld(H, "H"), ldo = ld(out, "out");
  const int64_t lda = ld(agg, "agg");
  if (meta(H)) return;
  const c10::DeviceGuard g(H.device());
  ck(gnnrec_spmm_project_agg_f32(p<int64_t>(indptr), p<int32_t>(indices), p<float>(ew),
                                 p<float>(X), ldx, p<float>(H), ldh, p<float>(W_selfT),
                                 p<float>(W_neighT), p<float>(bias), p<float>(bias_nonempty),
                                 n_dst, d, (int)reduce, (int)epilogue, (int)accum, (float)out_div,
                                 p<float>(attn_vec), p<float>(attn_state), p<float>(out), ldo,
                                 p<float>(agg), lda, (int)agg_mode, stream_of(H)),
     "gnnrec_spmm_project_agg_f32");
}

// ---------------------------------------------------------------- packed rows
// packed: int32 [n, 96] (csrc/pack_rows.hpp), status: int32 [4]
void packed_pair(const Tensor& packed, const Tensor& status, const Tensor& X) {
  dev(packed, "packed", at::kInt);
  dev(status, "status", at::kInt);
  TORCH_CHECK_VALUE(X.dim() == 2 && X.size(1) == 128, "packed rows need X [n, 128]");
  TORCH_CHECK_VALUE(packed.dim() == 2 && packed.size(0) == X.size(0) && packed.size(1) == 96 &&
                        packed.is_contiguous(),
                    "packed must be a contiguous int32 [", X.size(0), ", 96]");
  TORCH_CHECK_VALUE(status.numel() == 4 && status.is_contiguous(), "status must be int32 [4]");
}

void pack_rows_f32(const Tensor& X, double max_dense_frac, Tensor& packed, Tensor& status) {
  const OneDevice one_device_;
  dev(X, "X", at::kFloat);
  packed_pair(packed, status, X);
  const int64_t ldx = ld(X, "X");
  if (meta(X)) return;
  const c10::DeviceGuard g(X.device());
  ck(gnnrec_pack_rows_f32(p<float>(X), ldx, X.size(0), X.size(1), max_dense_frac,
                          p<int32_t>(packed), p<int32_t>(status), stream_of(X)),
     "gnnrec_pack_rows_f32");
}

// host only: a CPU fp32 [n, 128] table -> (packed int32 [n, 96], dense rows), and back
std::tuple<Tensor, int64_t> pack_rows_host(const Tensor& X) {
  TORCH_CHECK_VALUE(X.device().is_cpu() && X.scalar_type() == at::kFloat && X.dim() == 2 &&
                        X.size(1) == 128,
                    "pack_rows_host: needs a CPU float32 [n, 128] table");
  const Tensor x = X.contiguous();
  Tensor packed = at::empty({x.size(0), 96}, at::TensorOptions().dtype(at::kInt));
  int64_t dense = 0;
  ck(gnnrec_pack_rows_host(x.data_ptr<float>(), x.size(0), packed.data_ptr<int32_t>(), &dense),
     "gnnrec_pack_rows_host");
  return {packed, dense};
}

Tensor unpack_rows_host(const Tensor& packed, const Tensor& X_dense) {
  TORCH_CHECK_VALUE(packed.device().is_cpu() && packed.scalar_type() == at::kInt &&
                        packed.dim() == 2 && packed.size(1) == 96 && X_dense.device().is_cpu() &&
                        X_dense.scalar_type() == at::kFloat && X_dense.dim() == 2 &&
                        X_dense.size(0) == packed.size(0) && X_dense.size(1) == 128,
                    "unpack_rows_host: needs CPU int32 [n, 96] and float32 [n, 128]");
  const Tensor pk = packed.contiguous(), x = X_dense.contiguous();
  Tensor out = at::empty({pk.size(0), 128}, at::TensorOptions().dtype(at::kFloat));
  ck(gnnrec_unpack_rows_host(pk.data_ptr<int32_t>(), x.data_ptr<float>(), pk.size(0),
                             out.data_ptr<float>()),
     "gnnrec_unpack_rows_host");
  return out;
}

// n_heavy > 0: a heavy-row plan (host-built: the three lists; device-built: views of the
// plan tensor and `counts` = the plan itself, n_heavy / n_chunks its capacities)
void spmm_csr_packed_f32(const Tensor& indptr, const Tensor& indices, const Tensor& packed,
                         const Tensor& status, const Tensor& X, int64_t reduce, int64_t flags,
                         int64_t split, const optional<Tensor>& heavy, int64_t n_heavy,
                         const optional<Tensor>& chunk_ptr, const optional<Tensor>& chunk_row,
                         int64_t n_chunks, const optional<Tensor>& counts, Tensor& out,
                         const optional<Tensor>& ws) {
  const OneDevice one_device_;
  dev(indptr, "indptr", at::kLong);
  dev(indices, "indices", at::kInt);
  dev(X, "X", at::kFloat);
  packed_pair(packed, status, X);
  dev(heavy, "heavy_rows", at::kLong);
  dev(chunk_ptr, "chunk_ptr", at::kLong);
  dev(chunk_row, "chunk_row", at::kLong);
  dev(counts, "counts", at::kLong);
  dev(out, "out", at::kFloat);
  dev(ws, "workspace", at::kFloat);
  const int64_t n_dst = indptr.numel() - 1, d = X.size(1);
  TORCH_CHECK_VALUE(out.size(0) == n_dst && out.size(1) == d, "out must be [", n_dst, ", ", d, "]");
  TORCH_CHECK_VALUE(n_heavy >= 0 && n_chunks >= 0, "negative plan size");
  if (n_heavy > 0)
    TORCH_CHECK_VALUE(has(heavy) && has(chunk_ptr) && has(chunk_row) && has(ws) &&
                          heavy->numel() >= n_heavy && chunk_ptr->numel() >= n_heavy + 1 &&
                          chunk_row->numel() >= n_chunks && ws->numel() >= n_chunks * d,
                      "spmm_csr_packed_f32: incomplete heavy-row plan");
  const int64_t ldx = ld(X, "X"), ldo = ld(out, "out");
  if (meta(X)) return;
  const c10::DeviceGuard g(X.device());
  ck(gnnrec_spmm_csr_packed_f32(p<int64_t>(indptr), p<int32_t>(indices), p<int32_t>(packed),
                                p<int32_t>(status), p<float>(X), ldx, n_dst, d, (int)reduce,
                                (int)flags, p<float>(out), ldo, split, p<int64_t>(heavy), n_heavy,
                                p<int64_t>(chunk_ptr), p<int64_t>(chunk_row), n_chunks,
                                p<float>(ws), p<int64_t>(counts), stream_of(X)),
     "gnnrec_spmm_csr_packed_f32");
}

void spmm_project2(const Tensor& indptr_a, const Tensor& indices_a, const optional<Tensor>& ew_a,
                   const Tensor& Ya, int64_t reduce_a, const optional<Tensor>& bias_nonempty_a,
                   const Tensor& indptr_b, const Tensor& indices_b, const optional<Tensor>& ew_b,
                   const Tensor& Yb, int64_t reduce_b, const optional<Tensor>& bias_nonempty_b,
                   const Tensor& H, const Tensor& W_self_aT, const Tensor& W_self_bT,
                   const optional<Tensor>& bias_a, const optional<Tensor>& bias_b,
                   int64_t epilogue, int64_t combine, const optional<Tensor>& attn_vec,
                   double out_div, Tensor& out) {
  const OneDevice one_device_;
  dev(indptr_a, "indptr_a", at::kLong);
  dev(indices_a, "indices_a", at::kInt);
  dev(ew_a, "ew_a", at::kFloat);
  dev(Ya, "Ya", at::kFloat);
  dev(bias_nonempty_a, "bias_nonempty_a", at::kFloat);
  dev(indptr_b, "indptr_b", at::kLong);
  dev(indices_b, "indices_b", at::kInt);
  dev(ew_b, "ew_b", at::kFloat);
  dev(Yb, "Yb", at::kFloat);
  dev(bias_nonempty_b, "bias_nonempty_b", at::kFloat);
  dev(H, "H", at::kFloat);
  dev(W_self_aT, "W_self_aT", at::kFloat);
  dev(W_self_bT, "W_self_bT", at::kFloat);
  dev(bias_a, "bias_a", at::kFloat);
  dev(bias_b, "bias_b", at::kFloat);
  dev(attn_vec, "attn_vec", at::kFloat);
  dev(out, "out", at::kFloat);
  const int64_t n_dst = indptr_a.numel() - 1, d = Ya.size(1);
  TORCH_CHECK_VALUE(indptr_b.numel() == n_dst + 1,
                    "spmm_project2: the relations' row counts differ");
  TORCH_CHECK_VALUE(Yb.size(1) == d && H.size(0) >= n_dst, "spmm_project2: Yb / H shapes");
  TORCH_CHECK_VALUE(out.size(0) == n_dst && out.size(1) == d, "out must be [", n_dst, ", ", d,
                    "]");
  TORCH_CHECK_VALUE(W_self_aT.is_contiguous() && W_self_bT.is_contiguous(),
                    "transposed weights must be contiguous");
  const int64_t ldya = ld(Ya, "Ya"), ldyb = ld(Yb, "Yb"), ldh = ld(H, "H"), ldo = ld(out, "out");
  if (meta(Ya)) return;
  const c10::DeviceGuard g(Ya.device());
  ck(gnnrec_spmm_project2_f32(p<int64_t>(indptr_a), p<int32_t>(indices_a), p<float>(ew_a),
                              p<float>(Ya), ldya, (int)reduce_a, p<float>(bias_nonempty_a),
                              p<int64_t>(indptr_b), p<int32_t>(indices_b), p<float>(ew_b),
                              p<float>(Yb), ldyb, (int)reduce_b, p<float>(bias_nonempty_b),
                              p<float>(H), ldh, p<float>(W_self_aT), p<float>(W_self_bT),
                              p<float>(bias_a), p<float>(bias_b), n_dst, d, (int)epilogue,
                              (int)combine, p<float>(attn_vec), (float)out_div, p<float>(out),
                              ldo, stream_of(Ya)),
     "gnnrec_spmm_project2_f32");
}

void spmm_pair(const Tensor& indptr_a, const Tensor& indices_a, const optional<Tensor>& ew_a,
               int64_t reduce_a, const optional<Tensor>& bias_a,
               const optional<Tensor>& bias_nonempty_a, const Tensor& indptr_b,
               const Tensor& indices_b, const optional<Tensor>& ew_b, int64_t reduce_b,
               const optional<Tensor>& bias_b, const optional<Tensor>& bias_nonempty_b,
               const Tensor& X, const Tensor& H, const Tensor& WT4, int64_t epilogue,
               int64_t combine,
               const optional<Tensor>& attn_vec, double out_div, Tensor& out) {
  const OneDevice one_device_;
  dev(indptr_a, "indptr_a", at::kLong);
  dev(indices_a, "indices_a", at::kInt);
  dev(ew_a, "ew_a", at::kFloat);
  dev(bias_a, "bias_a", at::kFloat);
  dev(bias_nonempty_a, "bias_nonempty_a", at::kFloat);
  dev(indptr_b, "indptr_b", at::kLong);
  dev(indices_b, "indices_b", at::kInt);
  dev(ew_b, "ew_b", at::kFloat);
  dev(bias_b, "bias_b", at::kFloat);
  dev(bias_nonempty_b, "bias_nonempty_b", at::kFloat);
  dev(X, "X", at::kFloat);
  dev(H, "H", at::kFloat);
  dev(WT4, "WT4", at::kFloat);
  dev(attn_vec, "attn_vec", at::kFloat);
  dev(out, "out", at::kFloat);
  const int64_t n_dst = indptr_a.numel() - 1, d = X.size(1);
  TORCH_CHECK_VALUE(indptr_b.numel() == n_dst + 1, "spmm_pair: the relations' row counts differ");
  TORCH_CHECK_VALUE(H.size(1) == d && H.size(0) >= n_dst, "spmm_pair: H shape");
  TORCH_CHECK_VALUE(WT4.is_contiguous() && WT4.numel() == 4 * d * d,
                    "spmm_pair: WT4 must be a contiguous [4, d, d] weight array");
  TORCH_CHECK_VALUE(out.size(0) == n_dst && out.size(1) == d, "out must be [", n_dst, ", ", d,
                    "]");
  // the kernel reads d entries of every bias and of the attention vector
  for (const auto& v : {std::make_pair(&bias_a, "bias_a"), std::make_pair(&bias_b, "bias_b"),
                        std::make_pair(&bias_nonempty_a, "bias_nonempty_a"),
                        std::make_pair(&bias_nonempty_b, "bias_nonempty_b"),
                        std::make_pair(&attn_vec, "attn_vec")})
    TORCH_CHECK_VALUE(!has(*v.first) || ((*v.first)->numel() == d && (*v.first)->is_contiguous()),
                      "spmm_pair: ", v.second, " must be a contiguous vector of ", d, " floats");
  const int64_t ldx = ld(X, "X"), ldh = ld(H, "H"), ldo = ld(out, "out");
  if (meta(X)) return;
  const c10::DeviceGuard g(X.device());
  ck(gnnrec_spmm_pair_f32(p<int64_t>(indptr_a), p<int32_t>(indices_a), p<float>(ew_a),
                          (int)reduce_a, p<float>(bias_a), p<float>(bias_nonempty_a),
                          p<int64_t>(indptr_b), p<int32_t>(indices_b), p<float>(ew_b),
                          (int)reduce_b, p<float>(bias_b), p<float>(bias_nonempty_b),
                          p<float>(X), X.size(0), ldx, p<float>(H), ldh, p<float>(WT4), n_dst, d,
                          (int)epilogue, (int)combine, p<float>(attn_vec), (float)out_div,
                          p<float>(out), ldo, stream_of(X)),
     "gnnrec_spmm_pair_f32");
}

// ---------------------------------------------------------------- a7 / a8 heads
void sddmm_cos(const Tensor& src, const Tensor& dst, const Tensor& Hs, const Tensor& Hd,
               Tensor& out) {
  const OneDevice one_device_;
  dev(src, "src", at::kLong);
  dev(dst, "dst", at::kLong);
  dev(Hs, "Hs", at::kFloat);
  dev(Hd, "Hd", at::kFloat);
  dev(out, "out", at::kFloat);
  const int64_t E = src.numel();
  TORCH_CHECK_VALUE(dst.numel() == E && out.numel() == E, "src/dst/out length mismatch");
  TORCH_CHECK_VALUE(Hs.size(1) == Hd.size(1), "endpoint feature sizes differ");
  TORCH_CHECK_VALUE(src.is_contiguous() && dst.is_contiguous(), "src/dst must be contiguous");
  const int64_t lds = ld(Hs, "Hs"), ldd = ld(Hd, "Hd");
  if (meta(Hs)) return;
  const c10::DeviceGuard g(Hs.device());
  ck(gnnrec_sddmm_cos_f32(p<int64_t>(src), p<int64_t>(dst), E, p<float>(Hs), lds, p<float>(Hd),
                          ldd, Hs.size(1), p<float>(out), stream_of(Hs)),
     "gnnrec_sddmm_cos_f32");
}

void sddmm_cos_grouped(const Tensor& src_g, const optional<Tensor>& first, int64_t K,
                       const Tensor& dst, const Tensor& Hs, const Tensor& Hd,
                       Tensor& out_first, Tensor& out) {
  const OneDevice one_device_;
  dev(src_g, "src_g", at::kLong);
  dev(first, "first", at::kLong);
  dev(dst, "dst", at::kLong);
  dev(Hs, "Hs", at::kFloat);
  dev(Hd, "Hd", at::kFloat);
  dev(out_first, "out_first", at::kFloat);
  dev(out, "out", at::kFloat);
  const int64_t G = src_g.numel();
  TORCH_CHECK_VALUE(K >= 0 && dst.numel() == G * K && out.numel() == G * K,
                    "sddmm_cos_grouped: dst and out must hold n_groups x K entries");
  TORCH_CHECK_VALUE(!has(first) || (first->numel() == G && out_first.numel() == G),
                    "sddmm_cos_grouped: first and out_first must hold n_groups entries");
  TORCH_CHECK_VALUE(Hs.size(1) == Hd.size(1), "endpoint feature sizes differ");
  TORCH_CHECK_VALUE(src_g.is_contiguous() && dst.is_contiguous() &&
                        (!has(first) || first->is_contiguous()) && out.is_contiguous() &&
                        out_first.is_contiguous(),
                    "sddmm_cos_grouped: contiguous ids and outputs");
  const int64_t lds = ld(Hs, "Hs"), ldd = ld(Hd, "Hd");
  if (meta(Hs)) return;
  const c10::DeviceGuard g(Hs.device());
  ck(gnnrec_sddmm_cos_grouped_f32(p<int64_t>(src_g), G, p<int64_t>(first), p<float>(out_first),
                                  K, p<int64_t>(dst), p<float>(out), p<float>(Hs), lds,
                                  p<float>(Hd), ldd, Hs.size(1), stream_of(Hs)),
     "gnnrec_sddmm_cos_grouped_f32");
}

// groups > 0: the grouped layout of gnnrec_sddmm_cos_backward_grouped_f32 (K negatives per
// positive, E = groups (K + 1))
void sddmm_cos_backward(const Tensor& src, const Tensor& dst, const Tensor& Hs, const Tensor& Hd,
                        const Tensor& grad, const optional<Tensor>& gHs,
                        const optional<Tensor>& gHd, Tensor& ws, int64_t groups, int64_t K) {
  const OneDevice one_device_;
  dev(src, "src", at::kLong);
  dev(dst, "dst", at::kLong);
  dev(Hs, "Hs", at::kFloat);
  dev(Hd, "Hd", at::kFloat);
  dev(grad, "grad", at::kFloat);
  dev(gHs, "gHs", at::kFloat);
  dev(gHd, "gHd", at::kFloat);
  // grouped (groups > 0): src may hold only the positives' sources (the only entries read)
  const int64_t E = dst.numel(), d = Hs.size(1);
  TORCH_CHECK_VALUE((src.numel() == E || (groups > 0 && src.numel() == groups)) &&
                        grad.numel() == E,
                    "src/dst/grad length mismatch");
  TORCH_CHECK_VALUE(Hd.size(1) == d, "endpoint feature sizes differ");
  TORCH_CHECK_VALUE(groups <= 0 || (K >= 0 && groups * (K + 1) == E),
                    "sddmm_cos_backward: groups x (K + 1) must equal the edge count");
  const int64_t lds = ld(Hs, "Hs"), ldd = ld(Hd, "Hd");
  if (meta(Hs)) return;
  const c10::DeviceGuard g(Hs.device());
  if (groups > 0) {
    ck(gnnrec_sddmm_cos_backward_grouped_f32(
           p<int64_t>(src), p<int64_t>(dst), groups, K, p<float>(Hs), lds, Hs.size(0),
           p<float>(Hd), ldd, Hd.size(0), d, p<float>(grad), p<float>(gHs), p<float>(gHd),
           ws.data_ptr(), ws.nbytes(), stream_of(Hs)),
       "gnnrec_sddmm_cos_backward_grouped_f32");
    return;
  }
  ck(gnnrec_sddmm_cos_backward_f32(p<int64_t>(src), p<int64_t>(dst), E, p<float>(Hs), lds,
                                   Hs.size(0), p<float>(Hd), ldd, Hd.size(0), d, p<float>(grad),
                                   p<float>(gHs), p<float>(gHd), ws.data_ptr(), ws.nbytes(),
                                   stream_of(Hs)),
     "gnnrec_sddmm_cos_backward_f32");
}

void edge_mlp(const Tensor& src, const Tensor& dst, const Tensor& P, const Tensor& Q,
              const Tensor& W2, const Tensor& b2, const Tensor& w3, const Tensor& b3,
              Tensor& out) {
  const OneDevice one_device_;
  dev(src, "src", at::kLong);
  dev(dst, "dst", at::kLong);
  for (auto* t : {&P, &Q, &W2, &b2, &w3, &b3}) dev(*t, "edge_mlp operand", at::kFloat);
  dev(out, "out", at::kFloat);
  TORCH_CHECK_VALUE(P.size(1) == 128 && Q.size(1) == 128 && W2.size(0) == 32 && W2.size(1) == 128,
                    "edge_mlp expects the reference's 128/32 hidden sizes");
  TORCH_CHECK_VALUE(P.is_contiguous() && Q.is_contiguous() && W2.is_contiguous(),
                    "edge_mlp operands must be contiguous");
  const int64_t E = src.numel();
  TORCH_CHECK_VALUE(dst.numel() == E && out.numel() == E, "src/dst/out length mismatch");
  if (meta(P)) return;
  const c10::DeviceGuard g(P.device());
  ck(gnnrec_edge_mlp_f32(p<int64_t>(src), p<int64_t>(dst), E, p<float>(P), p<float>(Q),
                         p<float>(W2), p<float>(b2), p<float>(w3), p<float>(b3), p<float>(out),
                         stream_of(P)),
     "gnnrec_edge_mlp_f32");
}

void edge_mlp_grouped(const Tensor& src_g, const optional<Tensor>& first, int64_t K,
                      const Tensor& dst, const Tensor& P, const Tensor& Q, const Tensor& W2,
                      const Tensor& b2, const Tensor& w3, const Tensor& b3, Tensor& out_first,
                      Tensor& out) {
  const OneDevice one_device_;
  dev(src_g, "src_g", at::kLong);
  dev(first, "first", at::kLong);
  dev(dst, "dst", at::kLong);
  for (auto* t : {&P, &Q, &W2, &b2, &w3, &b3}) dev(*t, "edge_mlp operand", at::kFloat);
  dev(out_first, "out_first", at::kFloat);
  dev(out, "out", at::kFloat);
  TORCH_CHECK_VALUE(P.size(1) == 128 && Q.size(1) == 128 && W2.size(0) == 32 && W2.size(1) == 128,
                    "edge_mlp expects the reference's 128/32 hidden sizes");
  TORCH_CHECK_VALUE(P.is_contiguous() && Q.is_contiguous() && W2.is_contiguous(),
                    "edge_mlp operands must be contiguous");
  const int64_t G = src_g.numel();
  TORCH_CHECK_VALUE(K >= 0 && dst.numel() == G * K && out.numel() == G * K,
                    "edge_mlp_grouped: dst and out must hold n_groups x K entries");
  TORCH_CHECK_VALUE(!has(first) || (first->numel() == G && out_first.numel() == G),
                    "edge_mlp_grouped: first and out_first must hold n_groups entries");
  TORCH_CHECK_VALUE(src_g.is_contiguous() && dst.is_contiguous() &&
                        (!has(first) || first->is_contiguous()) && out.is_contiguous() &&
                        out_first.is_contiguous(),
                    "edge_mlp_grouped: contiguous ids and outputs");
  if (meta(P)) return;
  const c10::DeviceGuard g(P.device());
  ck(gnnrec_edge_mlp_grouped_f32(p<int64_t>(src_g), G, p<int64_t>(first), p<float>(out_first), K,
                                 p<int64_t>(dst), p<float>(out), p<float>(P), p<float>(Q),
                                 p<float>(W2), p<float>(b2), p<float>(w3), p<float>(b3),
                                 stream_of(P)),
     "gnnrec_edge_mlp_grouped_f32");
}

// the operands of a dense MLP scoring launch: P [B, 128], Q [n, 128], W2 [32, 128] contiguous
void dense_mlp_tables(const Tensor& P, const Tensor& Q, const Tensor& W2, const Tensor& b2,
                      const Tensor& w3, const Tensor& b3) {
  for (auto* t : {&P, &Q, &W2, &b2, &w3, &b3}) dev(*t, "edge_mlp operand", at::kFloat);
  TORCH_CHECK_VALUE(P.dim() == 2 && Q.dim() == 2 && W2.dim() == 2 && P.size(1) == 128 &&
                        Q.size(1) == 128 && W2.size(0) == 32 && W2.size(1) == 128 &&
                        b2.numel() == 32 && w3.numel() == 32 && b3.numel() == 1,
                    "edge_mlp expects the reference's 128/32 hidden sizes");
  TORCH_CHECK_VALUE(P.is_contiguous() && Q.is_contiguous() && W2.is_contiguous() &&
                        b2.is_contiguous() && w3.is_contiguous(),
                    "edge_mlp operands must be contiguous");
}

void edge_mlp_dense_store(const Tensor& P, const Tensor& Q, const Tensor& W2, const Tensor& b2,
                          const Tensor& w3, const Tensor& b3, Tensor& out) {
  const OneDevice one_device_;
  dense_mlp_tables(P, Q, W2, b2, w3, b3);
  dev(out, "out", at::kFloat);
  const int64_t B = P.size(0), n = Q.size(0);
  const int64_t ldo = ld(out, "out");
  TORCH_CHECK_VALUE(out.size(0) == B && out.size(1) == n, "out must be [", B, ", ", n, "], got ",
                    out.sizes());
  if (meta(P)) return;
  const c10::DeviceGuard g(P.device());
  ck(gnnrec_edge_mlp_dense_store_f32(p<float>(P), B, p<float>(Q), n, p<float>(W2), p<float>(b2),
                                     p<float>(w3), p<float>(b3), p<float>(out), ldo,
                                     stream_of(P)),
     "gnnrec_edge_mlp_dense_store_f32");
}

void edge_mlp_dense_filter(const Tensor& P, const Tensor& Q, const Tensor& W2, const Tensor& b2,
                           const Tensor& w3, const Tensor& b3, const Tensor& tau, Tensor& counts,
                           Tensor& cand_items, Tensor& cand_scores) {
  const OneDevice one_device_;
  dense_mlp_tables(P, Q, W2, b2, w3, b3);
  dev(tau, "tau", at::kFloat);
  dev(counts, "counts", at::kInt);
  dev(cand_items, "cand_items", at::kInt);
  dev(cand_scores, "cand_scores", at::kFloat);
  const int64_t B = P.size(0), n = Q.size(0);
  TORCH_CHECK_VALUE(tau.numel() == B && counts.numel() == B && tau.is_contiguous() &&
                        counts.is_contiguous(),
                    "tau / counts must be contiguous [", B, "]");
  TORCH_CHECK_VALUE(cand_items.dim() == 2 && cand_items.size(0) == B && cand_items.is_contiguous(),
                    "cand_items must be a contiguous [", B, ", cap], got ", cand_items.sizes());
  const int64_t cap = cand_items.size(1);
  TORCH_CHECK_VALUE(cap >= 1 && cap <= 4096, "cand_items: cap must be in [1, 4096], got ", cap);
  TORCH_CHECK_VALUE(cand_scores.sizes() == cand_items.sizes() && cand_scores.is_contiguous(),
                    "cand_scores must be a contiguous [", B, ", ", cap, "], got ",
                    cand_scores.sizes());
  if (meta(P)) return;
  const c10::DeviceGuard g(P.device());
  ck(gnnrec_edge_mlp_dense_filter_f32(p<float>(P), B, p<float>(Q), n, p<float>(W2), p<float>(b2),
                                      p<float>(w3), p<float>(b3), p<float>(tau),
                                      p<int32_t>(counts), p<int32_t>(cand_items),
                                      p<float>(cand_scores), cap, stream_of(P)),
     "gnnrec_edge_mlp_dense_filter_f32");
}

// ---------------------------------------------------------------- f1 top-k
void topk_rows(const Tensor& scores, int64_t k, const optional<Tensor>& exclude_indptr,
               const optional<Tensor>& exclude_indices, Tensor& out_vals, Tensor& out_idx) {
  const OneDevice one_device_;
  dev(scores, "scores", at::kFloat);
  dev(exclude_indptr, "exclude_indptr", at::kLong);
  dev(exclude_indices, "exclude_indices", at::kLong);
  dev(out_vals, "out_vals", at::kFloat);
  dev(out_idx, "out_idx", at::kLong);
  const int64_t lds = ld(scores, "scores");
  const int64_t n_rows = scores.size(0), n_cols = scores.size(1);
  TORCH_CHECK_VALUE(k >= 1, "k must be at least 1, got ", k);
  // the kernel writes row r at out + r * k: a view with any other layout (a column slice of a
  // wider result table) would be written in the wrong elements
  TORCH_CHECK_VALUE(out_vals.dim() == 2 && out_vals.size(0) == n_rows && out_vals.size(1) == k &&
                        out_vals.is_contiguous(),
                    "out_vals must be a contiguous [", n_rows, ", ", k, "], got ",
                    out_vals.sizes(), " with strides ", out_vals.strides());
  TORCH_CHECK_VALUE(out_idx.dim() == 2 && out_idx.size(0) == n_rows && out_idx.size(1) == k &&
                        out_idx.is_contiguous(),
                    "out_idx must be a contiguous [", n_rows, ", ", k, "], got ", out_idx.sizes(),
                    " with strides ", out_idx.strides());
  bool lists = has(exclude_indptr);
  if (lists) {  // the kernel reads exclude_indptr[row] and [row + 1] for every row
    TORCH_CHECK_VALUE(exclude_indptr->is_contiguous() && exclude_indptr->numel() == n_rows + 1,
                      "exclude_indptr must be contiguous with n_rows + 1 = ", n_rows + 1,
                      " elements, got ", exclude_indptr->sizes());
    TORCH_CHECK_VALUE(has(exclude_indices) && exclude_indices->is_contiguous(),
                      "exclude_indices must be given, contiguous, with exclude_indptr");
    lists = exclude_indices->numel() > 0;  // no entries (a null data pointer): nothing listed
  }
  if (meta(scores)) return;
  const c10::DeviceGuard g(scores.device());
  ck(gnnrec_topk_rows_f32(p<float>(scores), lds, n_rows, n_cols, k,
                          lists ? p<int64_t>(exclude_indptr) : nullptr,
                          lists ? p<int64_t>(exclude_indices) : nullptr, p<float>(out_vals),
                          p<int64_t>(out_idx), stream_of(scores)),
     "gnnrec_topk_rows_f32");
}

// ---------------------------------------------------------------- f1b bf16 prefilter
void normalize_rows_bf16(const Tensor& x, const optional<Tensor>& row_map, Tensor& out) {
  const OneDevice one_device_;
  dev(x, "x", at::kFloat);
  dev(row_map, "row_map", at::kLong);
  dev(out, "out", at::kBFloat16);
  const int64_t ldx = ld(x, "x"), d = x.size(1);
  const int64_t n = has(row_map) ? row_map->numel() : x.size(0);
  const int64_t dpad = (d + 31) / 32 * 32;
  TORCH_CHECK_VALUE(d >= 1, "x must have at least one column");
  TORCH_CHECK_VALUE(out.dim() == 2 && out.size(0) == n && out.size(1) == dpad &&
                        out.is_contiguous(),
                    "out must be a contiguous [", n, ", ", dpad, "] (dpad = d rounded up to 32), "
                    "got ", out.sizes());
  TORCH_CHECK_VALUE(!has(row_map) || row_map->is_contiguous(), "row_map must be contiguous");
  if (meta(x)) return;
  const c10::DeviceGuard g(x.device());
  ck(gnnrec_normalize_rows_bf16(p<float>(x), ldx, n, d, p<int64_t>(row_map), out.data_ptr(), dpad,
                                stream_of(x)),
     "gnnrec_normalize_rows_bf16");
}

// the two bf16 tables of a scoring launch: [n, dpad] contiguous, one dpad, a multiple of 32
int64_t score_tables(const Tensor& users, const Tensor& items) {
  dev(users, "users", at::kBFloat16);
  dev(items, "items", at::kBFloat16);
  TORCH_CHECK_VALUE(users.dim() == 2 && items.dim() == 2 && users.is_contiguous() &&
                        items.is_contiguous(),
                    "users / items must be contiguous 2-D bf16 tables");
  const int64_t dpad = users.size(1);
  TORCH_CHECK_VALUE(items.size(1) == dpad && dpad >= 32 && dpad % 32 == 0 && dpad <= 2048,
                    "users / items must share a dpad that is a multiple of 32 in [32, 2048], got ",
                    users.size(1), " and ", items.size(1));
  return dpad;
}

void score_bf16_store(const Tensor& users, const Tensor& items, Tensor& out) {
  const OneDevice one_device_;
  const int64_t dpad = score_tables(users, items);
  dev(out, "out", at::kFloat);
  const int64_t B = users.size(0), n = items.size(0);
  const int64_t ldo = ld(out, "out");
  TORCH_CHECK_VALUE(out.size(0) == B && out.size(1) == n, "out must be [", B, ", ", n, "], got ",
                    out.sizes());
  if (meta(users)) return;
  const c10::DeviceGuard g(users.device());
  ck(gnnrec_score_bf16_store(users.data_ptr(), B, items.data_ptr(), n, dpad, p<float>(out), ldo,
                             stream_of(users)),
     "gnnrec_score_bf16_store");
}

void score_bf16_filter(const Tensor& users, const Tensor& items, const Tensor& tau, Tensor& counts,
                       Tensor& cand_items) {
  const OneDevice one_device_;
  const int64_t dpad = score_tables(users, items);
  dev(tau, "tau", at::kFloat);
  dev(counts, "counts", at::kInt);
  dev(cand_items, "cand_items", at::kInt);
  const int64_t B = users.size(0), n = items.size(0);
  TORCH_CHECK_VALUE(tau.numel() == B && counts.numel() == B && tau.is_contiguous() &&
                        counts.is_contiguous(),
                    "tau / counts must be contiguous [", B, "]");
  TORCH_CHECK_VALUE(cand_items.dim() == 2 && cand_items.size(0) == B && cand_items.is_contiguous(),
                    "cand_items must be a contiguous [", B, ", cap], got ", cand_items.sizes());
  const int64_t cap = cand_items.size(1);
  TORCH_CHECK_VALUE(cap >= 1 && cap <= 4096, "cand_items: cap must be in [1, 4096], got ", cap);
  if (meta(users)) return;
  const c10::DeviceGuard g(users.device());
  ck(gnnrec_score_bf16_filter(users.data_ptr(), B, items.data_ptr(), n, dpad, p<float>(tau),
                              p<int32_t>(counts), p<int32_t>(cand_items), cap, stream_of(users)),
     "gnnrec_score_bf16_filter");
}

void mask_excluded_f32(Tensor& scores, const optional<Tensor>& user_rows,
                       const Tensor& exclude_indptr, const Tensor& exclude_indices) {
  const OneDevice one_device_;
  dev(scores, "scores", at::kFloat);
  dev(user_rows, "user_rows", at::kLong);
  dev(exclude_indptr, "exclude_indptr", at::kLong);
  dev(exclude_indices, "exclude_indices", at::kInt);
  const int64_t lds = ld(scores, "scores"), n_rows = scores.size(0);
  TORCH_CHECK_VALUE(!has(user_rows) || (user_rows->numel() == n_rows && user_rows->is_contiguous()),
                    "user_rows must be contiguous [", n_rows, "]");
  TORCH_CHECK_VALUE(exclude_indptr.is_contiguous() && exclude_indices.is_contiguous() &&
                        exclude_indptr.numel() >= 1 &&
                        (has(user_rows) || exclude_indptr.numel() > n_rows),
                    "exclude_indptr must be a contiguous indptr over the user rows");
  if (meta(scores)) return;
  const c10::DeviceGuard g(scores.device());
  ck(gnnrec_mask_excluded_f32(p<float>(scores), lds, n_rows, scores.size(1), p<int64_t>(user_rows),
                              p<int64_t>(exclude_indptr), p<int32_t>(exclude_indices),
                              stream_of(scores)),
     "gnnrec_mask_excluded_f32");
}

void topk_candidates_f32(const Tensor& counts, const Tensor& cand_items,
                         const optional<Tensor>& user_rows, const Tensor& h_user,
                         const Tensor& h_item, const optional<Tensor>& exclude_indptr,
                         const optional<Tensor>& exclude_indices, int64_t k, Tensor& out_vals,
                         Tensor& out_idx) {
  const OneDevice one_device_;
  dev(counts, "counts", at::kInt);
  dev(cand_items, "cand_items", at::kInt);
  dev(user_rows, "user_rows", at::kLong);
  dev(h_user, "h_user", at::kFloat);
  dev(h_item, "h_item", at::kFloat);
  dev(exclude_indptr, "exclude_indptr", at::kLong);
  dev(exclude_indices, "exclude_indices", at::kInt);
  dev(out_vals, "out_vals", at::kFloat);
  dev(out_idx, "out_idx", at::kLong);
  const int64_t B = counts.numel();
  TORCH_CHECK_VALUE(cand_items.dim() == 2 && cand_items.size(0) == B && cand_items.is_contiguous() &&
                        counts.is_contiguous(),
                    "cand_items must be a contiguous [", B, ", cap], got ", cand_items.sizes());
  const int64_t cap = cand_items.size(1);
  TORCH_CHECK_VALUE(cap >= 1 && cap <= 4096, "cand_items: cap must be in [1, 4096], got ", cap);
  TORCH_CHECK_VALUE(k >= 1 && k <= cap, "k must be in [1, cap = ", cap, "], got ", k);
  const int64_t ldu = ld(h_user, "h_user"), ldi = ld(h_item, "h_item"), d = h_user.size(1);
  TORCH_CHECK_VALUE(h_item.size(1) == d && d >= 4 && d % 4 == 0 && ldu % 4 == 0 && ldi % 4 == 0,
                    "h_user / h_item must share a feature size that is a multiple of 4 (and row "
                    "strides too), got ", h_user.sizes(), " and ", h_item.sizes());
  TORCH_CHECK_VALUE(!has(user_rows) || (user_rows->numel() == B && user_rows->is_contiguous()),
                    "user_rows must be contiguous [", B, "]");
  TORCH_CHECK_VALUE(has(user_rows) || h_user.size(0) >= B, "h_user has fewer rows than the batch");
  TORCH_CHECK_VALUE(has(exclude_indptr) == has(exclude_indices),
                    "exclude_indptr and exclude_indices come together");
  TORCH_CHECK_VALUE(!has(exclude_indptr) ||
                        (exclude_indptr->numel() == h_user.size(0) + 1 &&
                         exclude_indptr->is_contiguous() && exclude_indices->is_contiguous()),
                    "exclude_indptr must be a contiguous [n_user_rows + 1] over h_user's rows");
  TORCH_CHECK_VALUE(out_vals.numel() == B * k && out_idx.numel() == B * k &&
                        out_vals.is_contiguous() && out_idx.is_contiguous(),
                    "out_vals / out_idx must be contiguous [", B, ", ", k, "]");
  if (meta(counts)) return;
  const c10::DeviceGuard g(counts.device());
  ck(gnnrec_topk_candidates_f32(p<int32_t>(counts), p<int32_t>(cand_items), cap, B,
                                p<int64_t>(user_rows), p<float>(h_user), ldu, p<float>(h_item), ldi,
                                d, p<int64_t>(exclude_indptr), p<int32_t>(exclude_indices), k,
                                p<float>(out_vals), p<int64_t>(out_idx), stream_of(counts)),
     "gnnrec_topk_candidates_f32");
}

// f1e: cached lists merged with the dirty items the filter kept (gnnrec_topk_update_f32)
void topk_update(const Tensor& rows, Tensor& idx, Tensor& vals, const Tensor& item_mark,
                 const Tensor& counts, const Tensor& cand_cols, const Tensor& dirty_ids,
                 const Tensor& h_user, const Tensor& h_item,
                 const optional<Tensor>& exclude_indptr, const optional<Tensor>& exclude_indices,
                 Tensor& redo) {
  const OneDevice one_device_;
  dev(rows, "rows", at::kLong);
  dev(idx, "idx", at::kLong);
  dev(vals, "vals", at::kFloat);
  dev(item_mark, "item_mark", at::kInt);
  dev(counts, "counts", at::kInt);
  dev(cand_cols, "cand_cols", at::kInt);
  dev(dirty_ids, "dirty_ids", at::kInt);
  dev(h_user, "h_user", at::kFloat);
  dev(h_item, "h_item", at::kFloat);
  dev(exclude_indptr, "exclude_indptr", at::kLong);
  dev(exclude_indices, "exclude_indices", at::kInt);
  dev(redo, "redo", at::kInt);
  const int64_t ldu = ld(h_user, "h_user"), ldi = ld(h_item, "h_item"), d = h_user.size(1);
  const int64_t n_users = h_user.size(0), n_items = h_item.size(0), B = rows.numel();
  TORCH_CHECK_VALUE(idx.dim() == 2 && idx.size(0) == n_users && idx.is_contiguous() &&
                        vals.sizes() == idx.sizes() && vals.is_contiguous(),
                    "idx / vals must be contiguous [n_users = ", n_users, ", k], got ",
                    idx.sizes(), " and ", vals.sizes());
  const int64_t k = idx.size(1);
  TORCH_CHECK_VALUE(k >= 1 && k <= 64, "k must be in [1, 64], got ", k);
  TORCH_CHECK_VALUE(cand_cols.dim() == 2 && cand_cols.size(0) == B && cand_cols.is_contiguous() &&
                        counts.numel() == B && counts.is_contiguous() && rows.is_contiguous(),
                    "rows / counts must be contiguous [", B, "] and cand_cols a contiguous [", B,
                    ", cap], got ", cand_cols.sizes());
  const int64_t cap = cand_cols.size(1);
  TORCH_CHECK_VALUE(cap >= 1 && cap <= 256 - k, "cand_cols: cap must be in [1, 256 - k = ",
                    256 - k, "], got ", cap);
  TORCH_CHECK_VALUE(h_item.size(1) == d && d >= 4 && d % 4 == 0 && ldu % 4 == 0 && ldi % 4 == 0,
                    "h_user / h_item must share a feature size that is a multiple of 4 (and row "
                    "strides too), got ", h_user.sizes(), " and ", h_item.sizes());
  TORCH_CHECK_VALUE(item_mark.numel() == n_items && item_mark.is_contiguous(),
                    "item_mark must be contiguous [n_items = ", n_items, "]");
  TORCH_CHECK_VALUE(dirty_ids.dim() == 1 && dirty_ids.is_contiguous(),
                    "dirty_ids must be a contiguous list");
  TORCH_CHECK_VALUE(redo.numel() == n_users && redo.is_contiguous(),
                    "redo must be contiguous [n_users = ", n_users, "]");
  TORCH_CHECK_VALUE(has(exclude_indptr) == has(exclude_indices),
                    "exclude_indptr and exclude_indices come together");
  TORCH_CHECK_VALUE(!has(exclude_indptr) ||
                        (exclude_indptr->numel() == n_users + 1 &&
                         exclude_indptr->is_contiguous() && exclude_indices->is_contiguous()),
                    "exclude_indptr must be a contiguous [n_user_rows + 1] over h_user's rows");
  if (meta(rows)) return;
  const c10::DeviceGuard g(rows.device());
  ck(gnnrec_topk_update_f32(p<int64_t>(rows), B, p<int64_t>(idx), p<float>(vals), n_users, k,
                            p<int32_t>(item_mark), n_items, p<int32_t>(counts),
                            p<int32_t>(cand_cols), cap, p<int32_t>(dirty_ids), dirty_ids.numel(),
                            p<float>(h_user), ldu, p<float>(h_item), ldi, d,
                            p<int64_t>(exclude_indptr), p<int32_t>(exclude_indices),
                            p<int32_t>(redo), stream_of(rows)),
     "gnnrec_topk_update_f32");
}

// ---------------------------------------------------------------- f1d popularity ratings
// a per-row / per-column fp32 vector of a rating launch: contiguous, n entries
void rating_vec(const Tensor& t, const char* name, int64_t n) {
  dev(t, name, at::kFloat);
  TORCH_CHECK_VALUE(t.numel() == n && t.is_contiguous(), name, " must be contiguous [", n,
                    "], got ", t.sizes());
}

void normalize_rows_f32(const Tensor& x, const optional<Tensor>& row_map, Tensor& out) {
  const OneDevice one_device_;
  dev(x, "x", at::kFloat);
  dev(row_map, "row_map", at::kLong);
  dev(out, "out", at::kFloat);
  const int64_t ldx = ld(x, "x"), d = x.size(1);
  const int64_t n = has(row_map) ? row_map->numel() : x.size(0);
  const int64_t dpad = (d + 7) / 8 * 8;
  TORCH_CHECK_VALUE(d >= 4 && d % 4 == 0 && d <= 2048 && ldx % 4 == 0,
                    "x must have a multiple of 4 columns in [4, 2048] (and such a row stride), "
                    "got ", x.sizes());
  TORCH_CHECK_VALUE(out.dim() == 2 && out.size(0) == n && out.size(1) == dpad &&
                        out.is_contiguous(),
                    "out must be a contiguous [", n, ", ", dpad, "] (dpad = d rounded up to 8), "
                    "got ", out.sizes());
  TORCH_CHECK_VALUE(!has(row_map) || row_map->is_contiguous(), "row_map must be contiguous");
  if (meta(x)) return;
  const c10::DeviceGuard g(x.device());
  ck(gnnrec_normalize_rows_f32(p<float>(x), ldx, n, d, p<int64_t>(row_map), p<float>(out), dpad,
                               stream_of(x)),
     "gnnrec_normalize_rows_f32");
}

void cos_denominators(const Tensor& users, const Tensor& items, Tensor& parts, Tensor& Z) {
  const OneDevice one_device_;
  dev(users, "users", at::kFloat);
  dev(items, "items", at::kFloat);
  dev(parts, "parts", at::kFloat);
  dev(Z, "Z", at::kFloat);
  TORCH_CHECK_VALUE(users.dim() == 2 && items.dim() == 2 && users.is_contiguous() &&
                        items.is_contiguous(),
                    "users / items must be contiguous 2-D fp32 tables");
  const int64_t dpad = users.size(1), B = users.size(0), n = items.size(0);
  TORCH_CHECK_VALUE(items.size(1) == dpad && dpad >= 8 && dpad % 8 == 0 && dpad <= 2048,
                    "users / items must share a dpad that is a multiple of 8 in [8, 2048], got ",
                    users.size(1), " and ", items.size(1));
  const int64_t n_part = gnnrec_cos_denominator_parts(n);
  TORCH_CHECK_VALUE(parts.numel() >= n_part * B && parts.is_contiguous(),
                    "parts must hold ", n_part, " x ", B, " floats, got ", parts.sizes());
  rating_vec(Z, "Z", B);
  if (meta(users)) return;
  const c10::DeviceGuard g(users.device());
  ck(gnnrec_cos_denominators_f32(p<float>(users), B, p<float>(items), n, dpad, p<float>(parts),
                                 p<float>(Z), stream_of(users)),
     "gnnrec_cos_denominators_f32");
}

// ---------------------------------------------------------------- f1f full-ranking evaluation
// the two normalize_rows_f32 tables of an MFMA pass -> dpad
int64_t f32_tables(const Tensor& users, const Tensor& items) {
  dev(users, "users", at::kFloat);
  dev(items, "items", at::kFloat);
  TORCH_CHECK_VALUE(users.dim() == 2 && items.dim() == 2 && users.is_contiguous() &&
                        items.is_contiguous(),
                    "users / items must be contiguous 2-D fp32 tables");
  const int64_t dpad = users.size(1);
  TORCH_CHECK_VALUE(items.size(1) == dpad && dpad >= 8 && dpad % 8 == 0 && dpad <= 2048,
                    "users / items must share a dpad that is a multiple of 8 in [8, 2048], got ",
                    users.size(1), " and ", items.size(1));
  return dpad;
}

void cos_scores(const Tensor& users, const Tensor& items, Tensor& out) {
  const OneDevice one_device_;
  const int64_t dpad = f32_tables(users, items);
  dev(out, "out", at::kFloat);
  const int64_t B = users.size(0), n = items.size(0);
  const int64_t ldo = ld(out, "out");
  TORCH_CHECK_VALUE(out.size(0) == B && out.size(1) == n, "out must be [", B, ", ", n, "], got ",
                    out.sizes());
  if (meta(users)) return;
  const c10::DeviceGuard g(users.device());
  ck(gnnrec_cos_scores_f32(p<float>(users), B, p<float>(items), n, dpad, p<float>(out), ldo,
                           stream_of(users)),
     "gnnrec_cos_scores_f32");
}

void rank_count(const Tensor& users, const Tensor& items, const Tensor& thr, Tensor& parts,
                Tensor& ahead, Tensor& band_counts, Tensor& band_items) {
  const OneDevice one_device_;
  const int64_t dpad = f32_tables(users, items);
  dev(thr, "thr", at::kFloat);
  dev(parts, "parts", at::kInt);
  dev(ahead, "ahead", at::kInt);
  dev(band_counts, "band_counts", at::kInt);
  dev(band_items, "band_items", at::kInt);
  const int64_t B = users.size(0), n = items.size(0);
  TORCH_CHECK_VALUE(thr.numel() == B && ahead.numel() == B && band_counts.numel() == B &&
                        thr.is_contiguous() && ahead.is_contiguous() &&
                        band_counts.is_contiguous(),
                    "thr / ahead / band_counts must be contiguous [", B, "]");
  TORCH_CHECK_VALUE(band_items.dim() == 2 && band_items.size(0) == B && band_items.is_contiguous(),
                    "band_items must be a contiguous [", B, ", cap], got ", band_items.sizes());
  const int64_t cap = band_items.size(1);
  TORCH_CHECK_VALUE(cap >= 1 && cap <= 4096, "band_items: cap must be in [1, 4096], got ", cap);
  const int64_t n_part = gnnrec_cos_denominator_parts(n);
  TORCH_CHECK_VALUE(parts.numel() >= n_part * B && parts.is_contiguous(),
                    "parts must hold ", n_part, " x ", B, " int32, got ", parts.sizes());
  if (meta(users)) return;
  const c10::DeviceGuard g(users.device());
  ck(gnnrec_rank_count_f32(p<float>(users), B, p<float>(items), n, dpad, p<float>(thr),
                           p<int32_t>(parts), p<int32_t>(ahead), p<int32_t>(band_counts),
                           p<int32_t>(band_items), cap, stream_of(users)),
     "gnnrec_rank_count_f32");
}

void rank_resolve(const Tensor& users, const Tensor& items, const Tensor& thr, const Tensor& ahead,
                  const Tensor& band_counts, const Tensor& band_items, const Tensor& h_user,
                  const Tensor& h_item, const optional<Tensor>& exclude_indptr,
                  const optional<Tensor>& exclude_indices, Tensor& rank) {
  const OneDevice one_device_;
  dev(users, "users", at::kLong);
  dev(items, "items", at::kLong);
  dev(thr, "thr", at::kFloat);
  dev(ahead, "ahead", at::kInt);
  dev(band_counts, "band_counts", at::kInt);
  dev(band_items, "band_items", at::kInt);
  dev(h_user, "h_user", at::kFloat);
  dev(h_item, "h_item", at::kFloat);
  dev(exclude_indptr, "exclude_indptr", at::kLong);
  dev(exclude_indices, "exclude_indices", at::kInt);
  dev(rank, "rank", at::kLong);
  const int64_t P = users.numel();
  TORCH_CHECK_VALUE(items.numel() == P && thr.numel() == P && ahead.numel() == P &&
                        band_counts.numel() == P && rank.numel() == P && users.is_contiguous() &&
                        items.is_contiguous() && thr.is_contiguous() && ahead.is_contiguous() &&
                        band_counts.is_contiguous() && rank.is_contiguous(),
                    "users / items / thr / ahead / band_counts / rank must be contiguous [", P,
                    "]");
  TORCH_CHECK_VALUE(band_items.dim() == 2 && band_items.size(0) == P && band_items.is_contiguous(),
                    "band_items must be a contiguous [", P, ", cap], got ", band_items.sizes());
  const int64_t cap = band_items.size(1);
  TORCH_CHECK_VALUE(cap >= 1 && cap <= 4096, "band_items: cap must be in [1, 4096], got ", cap);
  const int64_t ldu = ld(h_user, "h_user"), ldi = ld(h_item, "h_item"), d = h_user.size(1);
  TORCH_CHECK_VALUE(h_item.size(1) == d && d >= 4 && d % 4 == 0 && ldu % 4 == 0 && ldi % 4 == 0,
                    "h_user / h_item must share a feature size that is a multiple of 4 (and row "
                    "strides too), got ", h_user.sizes(), " and ", h_item.sizes());
  TORCH_CHECK_VALUE(has(exclude_indptr) == has(exclude_indices),
                    "exclude_indptr and exclude_indices come together");
  TORCH_CHECK_VALUE(!has(exclude_indptr) ||
                        (exclude_indptr->numel() == h_user.size(0) + 1 &&
                         exclude_indptr->is_contiguous() && exclude_indices->is_contiguous()),
                    "exclude_indptr must be a contiguous [n_user_rows + 1] over h_user's rows");
  if (meta(users)) return;
  const c10::DeviceGuard g(users.device());
  ck(gnnrec_rank_resolve_f32(p<int64_t>(users), p<int64_t>(items), p<float>(thr),
                             p<int32_t>(ahead), p<int32_t>(band_counts), p<int32_t>(band_items),
                             cap, P, p<float>(h_user), ldu, h_user.size(0), p<float>(h_item), ldi,
                             h_item.size(0), d, p<int64_t>(exclude_indptr),
                             p<int32_t>(exclude_indices), p<int64_t>(rank), stream_of(users)),
     "gnnrec_rank_resolve_f32");
}

void exp_rowsum(const Tensor& scores, Tensor& Z) {
  const OneDevice one_device_;
  dev(scores, "scores", at::kFloat);
  const int64_t lds = ld(scores, "scores"), n_rows = scores.size(0);
  rating_vec(Z, "Z", n_rows);
  if (meta(scores)) return;
  const c10::DeviceGuard g(scores.device());
  ck(gnnrec_exp_rowsum_f32(p<float>(scores), lds, n_rows, scores.size(1), p<float>(Z),
                           stream_of(scores)),
     "gnnrec_exp_rowsum_f32");
}

void rating_rows_(Tensor& scores, const Tensor& Z, const Tensor& pv) {
  const OneDevice one_device_;
  dev(scores, "scores", at::kFloat);
  const int64_t lds = ld(scores, "scores"), n_rows = scores.size(0);
  rating_vec(Z, "Z", n_rows);
  rating_vec(pv, "p", scores.size(1));
  if (meta(scores)) return;
  const c10::DeviceGuard g(scores.device());
  ck(gnnrec_rating_rows_f32(p<float>(scores), lds, n_rows, scores.size(1), p<float>(Z),
                            p<float>(pv), stream_of(scores)),
     "gnnrec_rating_rows_f32");
}

void rating_thresholds(const Tensor& tau, const Tensor& Z, const Tensor& pmax, Tensor& thr) {
  const OneDevice one_device_;
  const int64_t B = tau.numel();
  rating_vec(tau, "tau", B);
  rating_vec(Z, "Z", B);
  rating_vec(pmax, "pmax", 1);
  rating_vec(thr, "thr", B);
  if (meta(tau)) return;
  const c10::DeviceGuard g(tau.device());
  ck(gnnrec_rating_thresholds_f32(p<float>(tau), p<float>(Z), p<float>(pmax), B, p<float>(thr),
                                  stream_of(tau)),
     "gnnrec_rating_thresholds_f32");
}

void mask_excluded_mapped_f32(Tensor& scores, const Tensor& col_ids,
                              const optional<Tensor>& user_rows, const Tensor& exclude_indptr,
                              const Tensor& exclude_indices) {
  const OneDevice one_device_;
  dev(scores, "scores", at::kFloat);
  dev(col_ids, "col_ids", at::kInt);
  dev(user_rows, "user_rows", at::kLong);
  dev(exclude_indptr, "exclude_indptr", at::kLong);
  dev(exclude_indices, "exclude_indices", at::kInt);
  const int64_t lds = ld(scores, "scores"), n_rows = scores.size(0);
  TORCH_CHECK_VALUE(col_ids.numel() == scores.size(1) && col_ids.is_contiguous(),
                    "col_ids must be contiguous [", scores.size(1), "], got ", col_ids.sizes());
  TORCH_CHECK_VALUE(!has(user_rows) || (user_rows->numel() == n_rows && user_rows->is_contiguous()),
                    "user_rows must be contiguous [", n_rows, "]");
  TORCH_CHECK_VALUE(exclude_indptr.is_contiguous() && exclude_indices.is_contiguous() &&
                        exclude_indptr.numel() >= 1 &&
                        (has(user_rows) || exclude_indptr.numel() > n_rows),
                    "exclude_indptr must be a contiguous indptr over the user rows");
  if (meta(scores)) return;
  const c10::DeviceGuard g(scores.device());
  ck(gnnrec_mask_excluded_mapped_f32(p<float>(scores), lds, n_rows, scores.size(1),
                                     p<int32_t>(col_ids), p<int64_t>(user_rows),
                                     p<int64_t>(exclude_indptr), p<int32_t>(exclude_indices),
                                     stream_of(scores)),
     "gnnrec_mask_excluded_mapped_f32");
}

void score_bf16_store_rating(const Tensor& users, const Tensor& items, const Tensor& Z,
                             const Tensor& p_col, Tensor& out) {
  const OneDevice one_device_;
  const int64_t dpad = score_tables(users, items);
  dev(out, "out", at::kFloat);
  const int64_t B = users.size(0), n = items.size(0);
  const int64_t ldo = ld(out, "out");
  TORCH_CHECK_VALUE(out.size(0) == B && out.size(1) == n, "out must be [", B, ", ", n, "], got ",
                    out.sizes());
  rating_vec(Z, "Z", B);
  rating_vec(p_col, "p_col", n);
  if (meta(users)) return;
  const c10::DeviceGuard g(users.device());
  ck(gnnrec_score_bf16_store_rating(users.data_ptr(), B, items.data_ptr(), n, dpad, p<float>(Z),
                                    p<float>(p_col), p<float>(out), ldo, stream_of(users)),
     "gnnrec_score_bf16_store_rating");
}

void score_bf16_filter_rating(const Tensor& users, const Tensor& items, const Tensor& Z,
                              const Tensor& p_col, const Tensor& thr, Tensor& counts,
                              Tensor& cand_items) {
  const OneDevice one_device_;
  const int64_t dpad = score_tables(users, items);
  dev(counts, "counts", at::kInt);
  dev(cand_items, "cand_items", at::kInt);
  const int64_t B = users.size(0), n = items.size(0);
  rating_vec(Z, "Z", B);
  rating_vec(p_col, "p_col", n);
  rating_vec(thr, "thr", B);
  TORCH_CHECK_VALUE(counts.numel() == B && counts.is_contiguous(),
                    "counts must be contiguous [", B, "]");
  TORCH_CHECK_VALUE(cand_items.dim() == 2 && cand_items.size(0) == B && cand_items.is_contiguous(),
                    "cand_items must be a contiguous [", B, ", cap], got ", cand_items.sizes());
  const int64_t cap = cand_items.size(1);
  TORCH_CHECK_VALUE(cap >= 1 && cap <= 4096, "cand_items: cap must be in [1, 4096], got ", cap);
  if (meta(users)) return;
  const c10::DeviceGuard g(users.device());
  ck(gnnrec_score_bf16_filter_rating(users.data_ptr(), B, items.data_ptr(), n, dpad, p<float>(Z),
                                     p<float>(p_col), p<float>(thr), p<int32_t>(counts),
                                     p<int32_t>(cand_items), cap, stream_of(users)),
     "gnnrec_score_bf16_filter_rating");
}

void topk_candidates_rating_f32(const Tensor& counts, const Tensor& cand_items,
                                const optional<Tensor>& user_rows, const Tensor& h_user,
                                const Tensor& h_item, const optional<Tensor>& exclude_indptr,
                                const optional<Tensor>& exclude_indices, const Tensor& Z,
                                const Tensor& pv, int64_t k, Tensor& out_vals, Tensor& out_idx) {
  const OneDevice one_device_;
  dev(counts, "counts", at::kInt);
  dev(cand_items, "cand_items", at::kInt);
  dev(user_rows, "user_rows", at::kLong);
  dev(h_user, "h_user", at::kFloat);
  dev(h_item, "h_item", at::kFloat);
  dev(exclude_indptr, "exclude_indptr", at::kLong);
  dev(exclude_indices, "exclude_indices", at::kInt);
  dev(out_vals, "out_vals", at::kFloat);
  dev(out_idx, "out_idx", at::kLong);
  const int64_t B = counts.numel();
  TORCH_CHECK_VALUE(cand_items.dim() == 2 && cand_items.size(0) == B && cand_items.is_contiguous() &&
                        counts.is_contiguous(),
                    "cand_items must be a contiguous [", B, ", cap], got ", cand_items.sizes());
  const int64_t cap = cand_items.size(1);
  TORCH_CHECK_VALUE(cap >= 1 && cap <= 4096, "cand_items: cap must be in [1, 4096], got ", cap);
  TORCH_CHECK_VALUE(k >= 1 && k <= cap, "k must be in [1, cap = ", cap, "], got ", k);
  const int64_t ldu = ld(h_user, "h_user"), ldi = ld(h_item, "h_item"), d = h_user.size(1);
  TORCH_CHECK_VALUE(h_item.size(1) == d && d >= 4 && d % 4 == 0 && ldu % 4 == 0 && ldi % 4 == 0,
                    "h_user / h_item must share a feature size that is a multiple of 4 (and row "
                    "strides too), got ", h_user.sizes(), " and ", h_item.sizes());
  TORCH_CHECK_VALUE(!has(user_rows) || (user_rows->numel() == B && user_rows->is_contiguous()),
                    "user_rows must be contiguous [", B, "]");
  TORCH_CHECK_VALUE(has(user_rows) || h_user.size(0) >= B, "h_user has fewer rows than the batch");
  TORCH_CHECK_VALUE(has(exclude_indptr) == has(exclude_indices),
                    "exclude_indptr and exclude_indices come together");
  TORCH_CHECK_VALUE(!has(exclude_indptr) ||
                        (exclude_indptr->numel() == h_user.size(0) + 1 &&
                         exclude_indptr->is_contiguous() && exclude_indices->is_contiguous()),
                    "exclude_indptr must be a contiguous [n_user_rows + 1] over h_user's rows");
  rating_vec(Z, "Z", B);
  rating_vec(pv, "p", h_item.size(0));
  TORCH_CHECK_VALUE(out_vals.numel() == B * k && out_idx.numel() == B * k &&
                        out_vals.is_contiguous() && out_idx.is_contiguous(),
                    "out_vals / out_idx must be contiguous [", B, ", ", k, "]");
  if (meta(counts)) return;
  const c10::DeviceGuard g(counts.device());
  ck(gnnrec_topk_candidates_rating_f32(p<int32_t>(counts), p<int32_t>(cand_items), cap, B,
                                       p<int64_t>(user_rows), p<float>(h_user), ldu,
                                       p<float>(h_item), ldi, d, p<int64_t>(exclude_indptr),
                                       p<int32_t>(exclude_indices), p<float>(Z), p<float>(pv), k,
                                       p<float>(out_vals), p<int64_t>(out_idx), stream_of(counts)),
     "gnnrec_topk_candidates_rating_f32");
}

void edge_mlp_dense_denominators(const Tensor& P, const Tensor& Q, const Tensor& W2,
                                 const Tensor& b2, const Tensor& w3, const Tensor& b3,
                                 Tensor& parts) {
  const OneDevice one_device_;
  dense_mlp_tables(P, Q, W2, b2, w3, b3);
  dev(parts, "parts", at::kFloat);
  const int64_t B = P.size(0), n = Q.size(0);
  const int64_t n_part = gnnrec_cos_denominator_parts(n);
  TORCH_CHECK_VALUE(parts.dim() == 2 && parts.size(0) == n_part && parts.size(1) == B &&
                        parts.is_contiguous(),
                    "parts must be a contiguous [", n_part, ", ", B, "], got ", parts.sizes());
  if (meta(P)) return;
  const c10::DeviceGuard g(P.device());
  ck(gnnrec_edge_mlp_dense_denominators_f32(p<float>(P), B, p<float>(Q), n, p<float>(W2),
                                            p<float>(b2), p<float>(w3), p<float>(b3),
                                            p<float>(parts), stream_of(P)),
     "gnnrec_edge_mlp_dense_denominators_f32");
}

void fold_partials_f32(const Tensor& parts, Tensor& Z) {
  const OneDevice one_device_;
  dev(parts, "parts", at::kFloat);
  TORCH_CHECK_VALUE(parts.dim() == 2 && parts.is_contiguous(),
                    "parts must be a contiguous [n_parts, n_rows], got ", parts.sizes());
  rating_vec(Z, "Z", parts.size(1));
  if (meta(parts)) return;
  const c10::DeviceGuard g(parts.device());
  ck(gnnrec_fold_partials_f32(p<float>(parts), parts.size(0), parts.size(1), p<float>(Z),
                              stream_of(parts)),
     "gnnrec_fold_partials_f32");
}

void edge_mlp_dense_store_rating(const Tensor& P, const Tensor& Q, const Tensor& W2,
                                 const Tensor& b2, const Tensor& w3, const Tensor& b3,
                                 const Tensor& Z, const Tensor& p_col, Tensor& out) {
  const OneDevice one_device_;
  dense_mlp_tables(P, Q, W2, b2, w3, b3);
  dev(out, "out", at::kFloat);
  const int64_t B = P.size(0), n = Q.size(0);
  const int64_t ldo = ld(out, "out");
  TORCH_CHECK_VALUE(out.size(0) == B && out.size(1) == n, "out must be [", B, ", ", n, "], got ",
                    out.sizes());
  rating_vec(Z, "Z", B);
  rating_vec(p_col, "p_col", n);
  if (meta(P)) return;
  const c10::DeviceGuard g(P.device());
  ck(gnnrec_edge_mlp_dense_store_rating_f32(p<float>(P), B, p<float>(Q), n, p<float>(W2),
                                            p<float>(b2), p<float>(w3), p<float>(b3), p<float>(Z),
                                            p<float>(p_col), p<float>(out), ldo, stream_of(P)),
     "gnnrec_edge_mlp_dense_store_rating_f32");
}

void edge_mlp_dense_filter_rating(const Tensor& P, const Tensor& Q, const Tensor& W2,
                                  const Tensor& b2, const Tensor& w3, const Tensor& b3,
                                  const Tensor& Z, const Tensor& p_col, const Tensor& tau,
                                  Tensor& counts, Tensor& cand_items, Tensor& cand_scores) {
  const OneDevice one_device_;
  dense_mlp_tables(P, Q, W2, b2, w3, b3);
  dev(counts, "counts", at::kInt);
  dev(cand_items, "cand_items", at::kInt);
  dev(cand_scores, "cand_scores", at::kFloat);
  const int64_t B = P.size(0), n = Q.size(0);
  rating_vec(Z, "Z", B);
  rating_vec(p_col, "p_col", n);
  rating_vec(tau, "tau", B);
  TORCH_CHECK_VALUE(counts.numel() == B && counts.is_contiguous(),
                    "counts must be contiguous [", B, "]");
  TORCH_CHECK_VALUE(cand_items.dim() == 2 && cand_items.size(0) == B && cand_items.is_contiguous(),
                    "cand_items must be a contiguous [", B, ", cap], got ", cand_items.sizes());
  const int64_t cap = cand_items.size(1);
  TORCH_CHECK_VALUE(cap >= 1 && cap <= 4096, "cand_items: cap must be in [1, 4096], got ", cap);
  TORCH_CHECK_VALUE(cand_scores.sizes() == cand_items.sizes() && cand_scores.is_contiguous(),
                    "cand_scores must be a contiguous [", B, ", ", cap, "], got ",
                    cand_scores.sizes());
  if (meta(P)) return;
  const c10::DeviceGuard g(P.device());
  ck(gnnrec_edge_mlp_dense_filter_rating_f32(p<float>(P), B, p<float>(Q), n, p<float>(W2),
                                             p<float>(b2), p<float>(w3), p<float>(b3),
                                             p<float>(Z), p<float>(p_col), p<float>(tau),
                                             p<int32_t>(counts), p<int32_t>(cand_items),
                                             p<float>(cand_scores), cap, stream_of(P)),
     "gnnrec_edge_mlp_dense_filter_rating_f32");
}

// ---------------------------------------------------------------- f1f for the MLP head
// the slot operands of a count pass over B rows and n items -> nothing; all checked
void dense_count_slots(const Tensor& lptr, const Tensor& thr, const Tensor& gid,
                       const Tensor& parts, const Tensor& ahead, int64_t B, int64_t n) {
  dev(lptr, "lptr", at::kLong);
  TORCH_CHECK_VALUE(lptr.numel() == B + 1 && lptr.is_contiguous(), "lptr must be contiguous [",
                    B + 1, "], got ", lptr.sizes());
  const int64_t E = thr.numel();
  TORCH_CHECK_VALUE(E <= B * gnnrec_rank_list_slots(), "at most ", gnnrec_rank_list_slots(),
                    " slots a row: ", E, " slots for ", B, " rows");
  rating_vec(thr, "thr", E);
  dev(gid, "gid", at::kInt);
  dev(parts, "parts", at::kInt);
  dev(ahead, "ahead", at::kInt);
  TORCH_CHECK_VALUE(gid.numel() == E && ahead.numel() == E && gid.is_contiguous() &&
                        ahead.is_contiguous(),
                    "gid / ahead must be contiguous [", E, "]");
  const int64_t n_part = gnnrec_cos_denominator_parts(n);
  TORCH_CHECK_VALUE(parts.dim() == 2 && parts.size(0) == n_part && parts.size(1) == E &&
                        parts.is_contiguous(),
                    "parts must be a contiguous [", n_part, ", ", E, "], got ", parts.sizes());
}

void edge_mlp_dense_count_lists(const Tensor& P, const Tensor& Q, const Tensor& W2,
                                const Tensor& b2, const Tensor& w3, const Tensor& b3,
                                const Tensor& lptr, const Tensor& thr, const Tensor& gid,
                                Tensor& parts, Tensor& ahead) {
  const OneDevice one_device_;
  dense_mlp_tables(P, Q, W2, b2, w3, b3);
  const int64_t B = P.size(0), n = Q.size(0);
  dense_count_slots(lptr, thr, gid, parts, ahead, B, n);
  if (meta(P)) return;
  const c10::DeviceGuard g(P.device());
  ck(gnnrec_edge_mlp_dense_count_lists_f32(p<float>(P), B, p<float>(Q), n, p<float>(W2),
                                           p<float>(b2), p<float>(w3), p<float>(b3),
                                           p<int64_t>(lptr), thr.numel(), p<float>(thr),
                                           p<int32_t>(gid), p<int32_t>(parts), p<int32_t>(ahead),
                                           stream_of(P)),
     "gnnrec_edge_mlp_dense_count_lists_f32");
}

void edge_mlp_dense_count_lists_rating(const Tensor& P, const Tensor& Q, const Tensor& W2,
                                       const Tensor& b2, const Tensor& w3, const Tensor& b3,
                                       const Tensor& Z, const Tensor& p_col, const Tensor& lptr,
                                       const Tensor& s, const Tensor& gid, Tensor& parts,
                                       Tensor& ahead) {
  const OneDevice one_device_;
  dense_mlp_tables(P, Q, W2, b2, w3, b3);
  const int64_t B = P.size(0), n = Q.size(0);
  rating_vec(Z, "Z", B);
  rating_vec(p_col, "p_col", n);
  dense_count_slots(lptr, s, gid, parts, ahead, B, n);
  if (meta(P)) return;
  const c10::DeviceGuard g(P.device());
  ck(gnnrec_edge_mlp_dense_count_lists_rating_f32(
         p<float>(P), B, p<float>(Q), n, p<float>(W2), p<float>(b2), p<float>(w3), p<float>(b3),
         p<float>(Z), p<float>(p_col), p<int64_t>(lptr), s.numel(), p<float>(s), p<int32_t>(gid),
         p<int32_t>(parts), p<int32_t>(ahead), stream_of(P)),
     "gnnrec_edge_mlp_dense_count_lists_rating_f32");
}

void rank_resolve_mlp_lists(const Tensor& row_user, const Tensor& lptr, const Tensor& s,
                            const Tensor& gid, const Tensor& ahead, int64_t n_users,
                            const Tensor& P, const Tensor& Q, const Tensor& W2, const Tensor& b2,
                            const Tensor& w3, const Tensor& b3, const optional<Tensor>& Z,
                            const optional<Tensor>& p_col, const optional<Tensor>& exclude_indptr,
                            const optional<Tensor>& exclude_indices, Tensor& rank, Tensor& vals) {
  const OneDevice one_device_;
  dev(row_user, "row_user", at::kLong);
  dev(lptr, "lptr", at::kLong);
  dense_mlp_tables(P, Q, W2, b2, w3, b3);
  dev(gid, "gid", at::kInt);
  dev(ahead, "ahead", at::kInt);
  dev(exclude_indptr, "exclude_indptr", at::kLong);
  dev(exclude_indices, "exclude_indices", at::kInt);
  dev(rank, "rank", at::kLong);
  const int64_t B = row_user.numel(), E = s.numel(), n = Q.size(0);
  rating_vec(s, "s", E);
  rating_vec(vals, "vals", E);
  TORCH_CHECK_VALUE(P.size(0) == B, "P must hold one row per list row: [", B, ", 128], got ",
                    P.sizes());
  TORCH_CHECK_VALUE(lptr.numel() == B + 1 && lptr.is_contiguous() && row_user.is_contiguous(),
                    "row_user / lptr must be contiguous [", B, "] / [", B + 1, "]");
  TORCH_CHECK_VALUE(E <= B * gnnrec_rank_list_slots(), "at most ", gnnrec_rank_list_slots(),
                    " slots a row: ", E, " slots for ", B, " rows");
  TORCH_CHECK_VALUE(gid.numel() == E && ahead.numel() == E && rank.numel() == E &&
                        gid.is_contiguous() && ahead.is_contiguous() && rank.is_contiguous(),
                    "gid / ahead / rank must be contiguous [", E, "]");
  TORCH_CHECK_VALUE(n_users >= 0 && (E == 0 || (n_users > 0 && n > 0)),
                    "entries need users and items (n_users = ", n_users, ", n_items = ", n, ")");
  TORCH_CHECK_VALUE(has(Z) == has(p_col), "Z and p_col come together");
  if (has(Z)) {
    rating_vec(*Z, "Z", B);
    rating_vec(*p_col, "p_col", n);
  }
  TORCH_CHECK_VALUE(has(exclude_indptr) == has(exclude_indices),
                    "exclude_indptr and exclude_indices come together");
  TORCH_CHECK_VALUE(!has(exclude_indptr) ||
                        (exclude_indptr->numel() == n_users + 1 &&
                         exclude_indptr->is_contiguous() && exclude_indices->is_contiguous()),
                    "exclude_indptr must be a contiguous [n_users + 1]");
  if (meta(row_user)) return;
  const c10::DeviceGuard g(row_user.device());
  ck(gnnrec_rank_resolve_mlp_lists_f32(
         p<int64_t>(row_user), p<int64_t>(lptr), B, p<float>(s), p<int32_t>(gid),
         p<int32_t>(ahead), E, n_users, p<float>(P), p<float>(Q), n, p<float>(W2), p<float>(b2),
         p<float>(w3), p<float>(b3), p<float>(Z), p<float>(p_col), p<int64_t>(exclude_indptr),
         p<int32_t>(exclude_indices), p<int64_t>(rank), p<float>(vals), stream_of(row_user)),
     "gnnrec_rank_resolve_mlp_lists_f32");
}

void topk_scored_candidates_f32(const Tensor& counts, const Tensor& cand_items,
                                const Tensor& cand_scores, const optional<Tensor>& user_rows,
                                const optional<Tensor>& exclude_indptr,
                                const optional<Tensor>& exclude_indices, int64_t k,
                                Tensor& out_vals, Tensor& out_idx) {
  const OneDevice one_device_;
  dev(counts, "counts", at::kInt);
  dev(cand_items, "cand_items", at::kInt);
  dev(cand_scores, "cand_scores", at::kFloat);
  dev(user_rows, "user_rows", at::kLong);
  dev(exclude_indptr, "exclude_indptr", at::kLong);
  dev(exclude_indices, "exclude_indices", at::kInt);
  dev(out_vals, "out_vals", at::kFloat);
  dev(out_idx, "out_idx", at::kLong);
  const int64_t B = counts.numel();
  TORCH_CHECK_VALUE(cand_items.dim() == 2 && cand_items.size(0) == B && cand_items.is_contiguous() &&
                        counts.is_contiguous(),
                    "cand_items must be a contiguous [", B, ", cap], got ", cand_items.sizes());
  const int64_t cap = cand_items.size(1);
  TORCH_CHECK_VALUE(cap >= 1 && cap <= 4096, "cand_items: cap must be in [1, 4096], got ", cap);
  TORCH_CHECK_VALUE(cand_scores.sizes() == cand_items.sizes() && cand_scores.is_contiguous(),
                    "cand_scores must be a contiguous [", B, ", ", cap, "], got ",
                    cand_scores.sizes());
  TORCH_CHECK_VALUE(k >= 1 && k <= cap, "k must be in [1, cap = ", cap, "], got ", k);
  TORCH_CHECK_VALUE(!has(user_rows) || (user_rows->numel() == B && user_rows->is_contiguous()),
                    "user_rows must be contiguous [", B, "]");
  TORCH_CHECK_VALUE(has(exclude_indptr) == has(exclude_indices),
                    "exclude_indptr and exclude_indices come together");
  TORCH_CHECK_VALUE(!has(exclude_indptr) ||
                        (exclude_indptr->is_contiguous() && exclude_indices->is_contiguous() &&
                         exclude_indptr->numel() >= 1 &&
                         (has(user_rows) || exclude_indptr->numel() > B)),
                    "exclude_indptr must be a contiguous indptr over the user rows");
  TORCH_CHECK_VALUE(out_vals.numel() == B * k && out_idx.numel() == B * k &&
                        out_vals.is_contiguous() && out_idx.is_contiguous(),
                    "out_vals / out_idx must be contiguous [", B, ", ", k, "]");
  if (meta(counts)) return;
  const c10::DeviceGuard g(counts.device());
  ck(gnnrec_topk_scored_candidates_f32(p<int32_t>(counts), p<int32_t>(cand_items),
                                       p<float>(cand_scores), cap, B, p<int64_t>(user_rows),
                                       p<int64_t>(exclude_indptr), p<int32_t>(exclude_indices), k,
                                       p<float>(out_vals), p<int64_t>(out_idx), stream_of(counts)),
     "gnnrec_topk_scored_candidates_f32");
}

// ---------------------------------------------------------------- f2 training
void gemm_tn(const Tensor& A, const Tensor& B, const optional<Tensor>& colsum, bool accumulate,
             Tensor& out, Tensor& ws, const optional<Tensor>& row_ptr) {
  const OneDevice one_device_;
  dev(A, "A", at::kFloat);
  dev(B, "B", at::kFloat);
  dev(colsum, "colsum", at::kFloat);
  dev(out, "out", at::kFloat);
  dev(row_ptr, "row_ptr", at::kLong);
  const int64_t K = A.size(0), M = A.size(1), N = B.size(1);
  TORCH_CHECK_VALUE(B.size(0) == K, "gemm_tn: A and B differ in K");
  TORCH_CHECK_VALUE(out.size(0) == M && out.size(1) == N, "out must be [", M, ", ", N, "]");
  TORCH_CHECK_VALUE(!has(row_ptr) || (has(colsum) && row_ptr->numel() == K + 1 &&
                                      row_ptr->is_contiguous()),
                    "gemm_tn: row_ptr must be a contiguous [", K + 1, "] indptr beside colsum");
  const int64_t lda = ld(A, "A"), ldb = ld(B, "B"), ldc = ld(out, "out");
  if (meta(A)) return;
  const c10::DeviceGuard g(A.device());
  ck(gnnrec_gemm_tn_bias_rows_f32(p<float>(A), lda, p<float>(B), ldb, K, M, N, p<float>(out),
                                  ldc, p<float>(colsum), p<int64_t>(row_ptr), (int)accumulate,
                                  p<float>(ws), stream_of(A)),
     "gnnrec_gemm_tn_bias_rows_f32");
}

void act_backward(const Tensor& u, const Tensor& gz, int64_t flags, Tensor& out) {
  const OneDevice one_device_;
  dev(u, "u", at::kFloat);
  dev(gz, "gz", at::kFloat);
  dev(out, "out", at::kFloat);
  TORCH_CHECK_VALUE(u.sizes() == gz.sizes() && u.sizes() == out.sizes(),
                    "act_backward: u / gz / out shapes differ");
  const int64_t ldu = ld(u, "u"), ldg = ld(gz, "gz"), ldo = ld(out, "out");
  if (meta(u)) return;
  const c10::DeviceGuard g(u.device());
  ck(gnnrec_act_backward_f32(p<float>(u), ldu, p<float>(gz), ldg, u.size(0), u.size(1),
                             (int)flags, p<float>(out), ldo, stream_of(u)),
     "gnnrec_act_backward_f32");
}

void act_backward_normed(const Tensor& z, const Tensor& row_norm, const Tensor& gz, bool relu,
                         Tensor& out) {
  const OneDevice one_device_;
  dev(z, "z", at::kFloat);
  dev(row_norm, "row_norm", at::kFloat);
  dev(gz, "gz", at::kFloat);
  dev(out, "out", at::kFloat);
  TORCH_CHECK_VALUE(z.sizes() == gz.sizes() && z.sizes() == out.sizes() &&
                        row_norm.numel() == z.size(0) && row_norm.is_contiguous(),
                    "act_backward_normed: shape mismatch");
  const int64_t ldz = ld(z, "z"), ldg = ld(gz, "gz"), ldo = ld(out, "out");
  if (meta(z)) return;
  const c10::DeviceGuard g(z.device());
  ck(gnnrec_act_backward_normed_f32(p<float>(z), ldz, p<float>(row_norm), p<float>(gz), ldg,
                                    z.size(0), z.size(1), (int)relu, p<float>(out), ldo,
                                    stream_of(z)),
     "gnnrec_act_backward_normed_f32");
}

void csr_transpose(const Tensor& indptr, const Tensor& indices, const optional<Tensor>& ew,
                   int64_t n_src, int64_t n_edges, bool mean, Tensor& ws, Tensor& indptr_t,
                   Tensor& indices_t, const optional<Tensor>& ew_t) {
  const OneDevice one_device_;
  dev(indptr, "indptr", at::kLong);
  dev(indices, "indices", at::kInt);
  dev(ew, "edge_weight", at::kFloat);
  dev(indptr_t, "indptr_t", at::kLong);
  dev(indices_t, "indices_t", at::kInt);
  dev(ew_t, "ew_t", at::kFloat);
  TORCH_CHECK_VALUE(indices.numel() >= n_edges, "csr_transpose: indices shorter than the edge count");
  TORCH_CHECK_VALUE(indptr_t.numel() == n_src + 1 && indices_t.numel() >= n_edges,
                    "csr_transpose: output sizes");
  if (meta(indptr)) return;
  const c10::DeviceGuard g(indptr.device());
  ck(gnnrec_csr_transpose(p<int64_t>(indptr), p<int32_t>(indices), p<float>(ew),
                          indptr.numel() - 1, n_src, n_edges, (int)mean, ws.data_ptr(), ws.nbytes(),
                          p<int64_t>(indptr_t), p<int32_t>(indices_t), p<float>(ew_t),
                          stream_of(indptr)),
     "gnnrec_csr_transpose");
}

void csr_from_keys(const Tensor& keys, int64_t n_rows, Tensor& ws, Tensor& indptr, Tensor& perm) {
  const OneDevice one_device_;
  dev(keys, "keys", at::kInt);
  dev(indptr, "indptr", at::kLong);
  dev(perm, "perm", at::kInt);
  TORCH_CHECK_VALUE(keys.is_contiguous() && indptr.numel() == n_rows + 1 &&
                        perm.numel() == keys.numel(),
                    "csr_from_keys: output sizes");
  if (meta(keys)) return;
  const c10::DeviceGuard g(keys.device());
  ck(gnnrec_csr_from_keys(p<int32_t>(keys), keys.numel(), n_rows, ws.data_ptr(), ws.nbytes(),
                          p<int64_t>(indptr), p<int32_t>(perm), stream_of(keys)),
     "gnnrec_csr_from_keys");
}

// ---------------------------------------------------------------- f3 graph construction
void csr_build(const Tensor& src, const Tensor& dst, int64_t n_dst, Tensor& ws, Tensor& indptr,
               Tensor& indices, Tensor& eids) {
  const OneDevice one_device_;
  dev(src, "src", at::kLong);
  dev(dst, "dst", at::kLong);
  dev(indptr, "indptr", at::kLong);
  dev(indices, "indices", at::kInt);
  dev(eids, "eids", at::kLong);
  const int64_t E = dst.numel();
  TORCH_CHECK_VALUE(src.numel() == E && src.is_contiguous() && dst.is_contiguous(),
                    "csr_build: src and dst must be contiguous 1-D tensors of one length");
  TORCH_CHECK_VALUE(indptr.numel() == n_dst + 1 && indices.numel() == E && eids.numel() == E,
                    "csr_build: output sizes");
  if (meta(dst)) return;
  const c10::DeviceGuard g(dst.device());
  ck(gnnrec_csr_build(p<int64_t>(src), p<int64_t>(dst), E, n_dst, ws.data_ptr(), ws.nbytes(),
                      p<int64_t>(indptr), p<int32_t>(indices), p<int64_t>(eids), stream_of(dst)),
     "gnnrec_csr_build");
}

// remove_edges of one relation: the masked COO and the compacted CSR (csr_filter.hip)
void csr_remove_edges(const Tensor& src, const Tensor& dst, const Tensor& indptr,
                      const Tensor& indices, const Tensor& eids, const Tensor& rm, Tensor& ws,
                      Tensor& src_out, Tensor& dst_out, Tensor& kept_eids, Tensor& indptr_out,
                      Tensor& indices_out, Tensor& eids_out, Tensor& status) {
  const OneDevice one_device_;
  dev(src, "src", at::kLong);
  dev(dst, "dst", at::kLong);
  dev(indptr, "indptr", at::kLong);
  dev(indices, "indices", at::kInt);
  dev(eids, "eids", at::kLong);
  dev(rm, "rm", at::kLong);
  dev(ws, "workspace", at::kByte);
  dev(src_out, "src_out", at::kLong);
  dev(dst_out, "dst_out", at::kLong);
  dev(kept_eids, "kept_eids", at::kLong);
  dev(indptr_out, "indptr_out", at::kLong);
  dev(indices_out, "indices_out", at::kInt);
  dev(eids_out, "eids_out", at::kLong);
  dev(status, "status", at::kLong);
  // an EMPTY indptr (a CSR has at least one entry): the relation's CSR is not built, the COO
  // alone is compacted and every CSR operand must be empty
  const bool csr = indptr.numel() > 0;
  const int64_t E = dst.numel(), n_dst = csr ? indptr.numel() - 1 : 0, Ec = csr ? E : 0;
  TORCH_CHECK_VALUE(src.dim() == 1 && dst.dim() == 1 && src.numel() == E &&
                        src.is_contiguous() && dst.is_contiguous(),
                    "csr_remove_edges: src and dst must be contiguous 1-D tensors of one length");
  TORCH_CHECK_VALUE(indices.numel() == Ec && eids.numel() == Ec && indptr.is_contiguous() &&
                        indices.is_contiguous() && eids.is_contiguous(),
                    "csr_remove_edges: the CSR must be indptr [n_dst+1], indices [E], eids [E], "
                    "contiguous (or all empty)");
  TORCH_CHECK_VALUE(rm.dim() == 1 && rm.is_contiguous(),
                    "csr_remove_edges: rm must be a contiguous 1-D tensor");
  TORCH_CHECK_VALUE(src_out.numel() == E && dst_out.numel() == E && kept_eids.numel() == E &&
                        indptr_out.numel() == indptr.numel() && indices_out.numel() == Ec &&
                        eids_out.numel() == Ec && status.numel() == 2 &&
                        src_out.is_contiguous() && dst_out.is_contiguous() &&
                        kept_eids.is_contiguous() && indptr_out.is_contiguous() &&
                        indices_out.is_contiguous() && eids_out.is_contiguous() &&
                        status.is_contiguous(),
                    "csr_remove_edges: output sizes");
  if (meta(dst)) return;
  const c10::DeviceGuard g(dst.device());
  ck(gnnrec_csr_remove_edges(p<int64_t>(src), p<int64_t>(dst), csr ? p<int64_t>(indptr) : nullptr,
                             p<int32_t>(indices), p<int64_t>(eids), E, n_dst, p<int64_t>(rm),
                             rm.numel(), ws.data_ptr(), ws.nbytes(), p<int64_t>(src_out),
                             p<int64_t>(dst_out), p<int64_t>(kept_eids),
                             csr ? p<int64_t>(indptr_out) : nullptr, p<int32_t>(indices_out),
                             p<int64_t>(eids_out), p<int64_t>(status), stream_of(dst)),
     "gnnrec_csr_remove_edges");
}

// remove_nodes, part 1: one node type's rank table (csr_remove_nodes.hip)
void node_rank_table(const Tensor& nids, int64_t n_nodes, Tensor& ws, Tensor& removed,
                     Tensor& table, Tensor& kept, Tensor& status) {
  const OneDevice one_device_;
  dev(nids, "nids", at::kLong);
  dev(ws, "workspace", at::kByte);
  dev(removed, "removed", at::kInt);
  dev(table, "table", at::kLong);
  dev(kept, "kept", at::kLong);
  dev(status, "status", at::kLong);
  TORCH_CHECK_VALUE(n_nodes >= 0, "node_rank_table: negative node count");
  TORCH_CHECK_VALUE(nids.dim() == 1 && nids.is_contiguous(),
                    "node_rank_table: nids must be a contiguous 1-D tensor");
  const int64_t W = (n_nodes + 31) / 32;
  TORCH_CHECK_VALUE(removed.numel() == W && table.numel() == W + 1 && kept.numel() == n_nodes &&
                        status.numel() == 2 && removed.is_contiguous() &&
                        table.is_contiguous() && kept.is_contiguous() && status.is_contiguous(),
                    "node_rank_table: output sizes (removed [ceil(N/32)], table [ceil(N/32)+1], "
                    "kept [N], status [2])");
  if (meta(nids)) return;
  const c10::DeviceGuard g(nids.device());
  ck(gnnrec_node_rank_table(p<int64_t>(nids), nids.numel(), n_nodes, ws.data_ptr(), ws.nbytes(),
                            reinterpret_cast<uint32_t*>(p<int32_t>(removed)), p<int64_t>(table),
                            p<int64_t>(kept), p<int64_t>(status), stream_of(nids)),
     "gnnrec_node_rank_table");
}

// remove_nodes, part 2: one relation under its types' rank tables (csr_remove_nodes.hip)
void csr_remove_nodes(const Tensor& src, const Tensor& dst, const Tensor& indptr,
                      const Tensor& indices, const Tensor& eids,
                      const optional<Tensor>& src_table, const optional<Tensor>& dst_table,
                      int64_t n_src, int64_t n_dst, int64_t n_dst_new, Tensor& ws,
                      Tensor& src_out, Tensor& dst_out, Tensor& kept_eids, Tensor& indptr_out,
                      Tensor& indices_out, Tensor& eids_out, Tensor& status) {
  const OneDevice one_device_;
  dev(src, "src", at::kLong);
  dev(dst, "dst", at::kLong);
  dev(indptr, "indptr", at::kLong);
  dev(indices, "indices", at::kInt);
  dev(eids, "eids", at::kLong);
  dev(src_table, "src_table", at::kLong);
  dev(dst_table, "dst_table", at::kLong);
  dev(ws, "workspace", at::kByte);
  dev(src_out, "src_out", at::kLong);
  dev(dst_out, "dst_out", at::kLong);
  dev(kept_eids, "kept_eids", at::kLong);
  dev(indptr_out, "indptr_out", at::kLong);
  dev(indices_out, "indices_out", at::kInt);
  dev(eids_out, "eids_out", at::kLong);
  dev(status, "status", at::kLong);
  // an EMPTY indptr (a CSR has at least one entry): the relation's CSR is not built, the COO
  // alone is compacted and every CSR operand must be empty
  const bool csr = indptr.numel() > 0;
  const int64_t E = dst.numel(), Ec = csr ? E : 0;
  TORCH_CHECK_VALUE(n_src >= 0 && n_dst >= 0 && n_dst_new >= 0,
                    "csr_remove_nodes: negative node count");
  TORCH_CHECK_VALUE(src.dim() == 1 && dst.dim() == 1 && src.numel() == E &&
                        src.is_contiguous() && dst.is_contiguous(),
                    "csr_remove_nodes: src and dst must be contiguous 1-D tensors of one length");
  TORCH_CHECK_VALUE((!csr || indptr.numel() == n_dst + 1) && indices.numel() == Ec &&
                        eids.numel() == Ec && indptr.is_contiguous() &&
                        indices.is_contiguous() && eids.is_contiguous(),
                    "csr_remove_nodes: the CSR must be indptr [n_dst+1], indices [E], eids [E], "
                    "contiguous (or all empty)");
  TORCH_CHECK_VALUE(has(src_table) || has(dst_table),
                    "csr_remove_nodes: a source table, a destination table or both");
  TORCH_CHECK_VALUE((!has(src_table) || (src_table->dim() == 1 && src_table->is_contiguous() &&
                                         src_table->numel() == (n_src + 31) / 32 + 1)) &&
                        (!has(dst_table) ||
                         (dst_table->dim() == 1 && dst_table->is_contiguous() &&
                          dst_table->numel() == (n_dst + 31) / 32 + 1)),
                    "csr_remove_nodes: a rank table must be a contiguous [ceil(N/32)+1] tensor");
  TORCH_CHECK_VALUE(has(dst_table) ? n_dst_new <= n_dst : n_dst_new == n_dst,
                    "csr_remove_nodes: n_dst_new must be the destination type's new node count");
  TORCH_CHECK_VALUE(src_out.numel() == E && dst_out.numel() == E && kept_eids.numel() == E &&
                        indptr_out.numel() == (csr ? n_dst_new + 1 : 0) &&
                        indices_out.numel() == Ec && eids_out.numel() == Ec &&
                        status.numel() == 2 && src_out.is_contiguous() &&
                        dst_out.is_contiguous() && kept_eids.is_contiguous() &&
                        indptr_out.is_contiguous() && indices_out.is_contiguous() &&
                        eids_out.is_contiguous() && status.is_contiguous(),
                    "csr_remove_nodes: output sizes");
  if (meta(dst)) return;
  const c10::DeviceGuard g(dst.device());
  ck(gnnrec_csr_remove_nodes(p<int64_t>(src), p<int64_t>(dst), csr ? p<int64_t>(indptr) : nullptr,
                             p<int32_t>(indices), p<int64_t>(eids), E, n_src, n_dst,
                             p<int64_t>(src_table), p<int64_t>(dst_table), n_dst_new,
                             ws.data_ptr(), ws.nbytes(), p<int64_t>(src_out), p<int64_t>(dst_out),
                             p<int64_t>(kept_eids), csr ? p<int64_t>(indptr_out) : nullptr,
                             p<int32_t>(indices_out), p<int64_t>(eids_out), p<int64_t>(status),
                             stream_of(dst)),
     "gnnrec_csr_remove_nodes");
}

// add_edges of one relation: the batch merged into the cached CSR (csr_merge.hip)
void csr_add_edges(const Tensor& indptr, const Tensor& indices, const Tensor& eids,
                   const Tensor& src_new, const Tensor& dst_new, int64_t n_src, int64_t n_dst,
                   Tensor& ws, Tensor& indptr_out, Tensor& indices_out, Tensor& eids_out,
                   Tensor& status) {
  const OneDevice one_device_;
  dev(indptr, "indptr", at::kLong);
  dev(indices, "indices", at::kInt);
  dev(eids, "eids", at::kLong);
  dev(src_new, "src_new", at::kLong);
  dev(dst_new, "dst_new", at::kLong);
  dev(ws, "workspace", at::kByte);
  dev(indptr_out, "indptr_out", at::kLong);
  dev(indices_out, "indices_out", at::kInt);
  dev(eids_out, "eids_out", at::kLong);
  dev(status, "status", at::kLong);
  const int64_t E = eids.numel(), n = dst_new.numel();
  TORCH_CHECK_VALUE(n_src >= 0 && n_dst >= 0, "csr_add_edges: negative node count");
  TORCH_CHECK_VALUE(indptr.dim() == 1 && indptr.numel() == n_dst + 1 && indices.dim() == 1 &&
                        eids.dim() == 1 && indices.numel() == E && indptr.is_contiguous() &&
                        indices.is_contiguous() && eids.is_contiguous(),
                    "csr_add_edges: the CSR must be indptr [n_dst+1], indices [E], eids [E], "
                    "contiguous");
  TORCH_CHECK_VALUE(src_new.dim() == 1 && dst_new.dim() == 1 && src_new.numel() == n &&
                        src_new.is_contiguous() && dst_new.is_contiguous(),
                    "csr_add_edges: src_new and dst_new must be contiguous 1-D tensors of one "
                    "length");
  TORCH_CHECK_VALUE(indptr_out.numel() == n_dst + 1 && indices_out.numel() == E + n &&
                        eids_out.numel() == E + n && status.numel() == 2 &&
                        indptr_out.is_contiguous() && indices_out.is_contiguous() &&
                        eids_out.is_contiguous() && status.is_contiguous(),
                    "csr_add_edges: output sizes");
  if (meta(indptr)) return;
  const c10::DeviceGuard g(indptr.device());
  ck(gnnrec_csr_add_edges(p<int64_t>(indptr), p<int32_t>(indices), p<int64_t>(eids), E, n_src,
                          n_dst, p<int64_t>(src_new), p<int64_t>(dst_new), n, ws.data_ptr(),
                          ws.nbytes(), p<int64_t>(indptr_out), p<int32_t>(indices_out),
                          p<int64_t>(eids_out), p<int64_t>(status), stream_of(indptr)),
     "gnnrec_csr_add_edges");
}

// the destinations of the out-edges of the listed source rows, as marks (frontier.hip)
void frontier_mark(const Tensor& rows, const optional<Tensor>& n_rows, const Tensor& indptr,
                   const Tensor& indices, Tensor& mark, Tensor& ws, Tensor& status) {
  const OneDevice one_device_;
  dev(rows, "rows", at::kLong);
  dev(n_rows, "n_rows", at::kLong);
  dev(indptr, "indptr", at::kLong);
  dev(indices, "indices", at::kInt);
  dev(mark, "mark", at::kInt);
  dev(ws, "workspace", at::kByte);
  dev(status, "status", at::kLong);
  TORCH_CHECK_VALUE(rows.dim() == 1 && rows.is_contiguous(),
                    "frontier_mark: rows must be a contiguous 1-D tensor");
  TORCH_CHECK_VALUE(!has(n_rows) || n_rows->numel() == 1,
                    "frontier_mark: n_rows is one device count");
  TORCH_CHECK_VALUE(indptr.dim() == 1 && indptr.numel() >= 1 && indices.dim() == 1 &&
                        indptr.is_contiguous() && indices.is_contiguous(),
                    "frontier_mark: the CSR must be indptr [n_src+1], indices [E], contiguous");
  TORCH_CHECK_VALUE(mark.dim() == 1 && mark.is_contiguous() && status.numel() == 2 &&
                        status.is_contiguous(),
                    "frontier_mark: mark [n_dst] and status [2], contiguous");
  if (meta(rows)) return;
  const c10::DeviceGuard g(rows.device());
  ck(gnnrec_frontier_mark(p<int64_t>(rows), rows.numel(), p<int64_t>(n_rows), p<int64_t>(indptr),
                          p<int32_t>(indices), indices.numel(), indptr.numel() - 1, mark.numel(),
                          p<int32_t>(mark), ws.data_ptr(), ws.nbytes(), p<int64_t>(status),
                          stream_of(rows)),
     "gnnrec_frontier_mark");
}

// ---------------------------------------------------------------- f2 fused relation
// One ConvLayer relation of a TRAINING step (sum / mean aggregation), forward and backward
// each as ONE dispatcher call that issues every launch from C++ (gnnrec/autograd.py
// SageRelFn): the per-launch Python wrappers and the second autograd node per relation were
// most of the C2 step's host time (profiles/r03_c2_step_probe.txt).  Same kernels, same
// order, same values as SpmmFn + SageProjectFn.
//   forward:  agg = spmm(indptr, indices, m, reduce, ew); z = norm?(relu(h_self[:M] Wsᵀ +
//             agg Wnᵀ)) with the row norms kept (norm, N <= 256) -> (z, agg, row_norm)
//   backward: gu = the ReLU / norm Jacobian applied to gz; g_self = gu Ws (whole table,
//             zero past M); g_m = transposed gather of gu Wn over the source-major CSR (the
//             mean's 1/deg folded into the edge weights); g_Ws = guᵀ h_self; g_Wn = guᵀ agg
namespace {
constexpr int64_t kSplit = 2048;  // ops.DEFAULT_SPLIT: heavy rows of the transposed gather

float* pw(const Tensor& t) { return t.defined() ? p<float>(t) : nullptr; }

Tensor gemm_nt(const Tensor& A, const Tensor& W, const Tensor* A2, const Tensor* W2, int epi,
               Tensor out, Tensor* row_norm, int accum = GNNREC_ACC_STORE,
               const float* bias = nullptr, const float* bias_ne = nullptr,
               const int32_t* a2_deg = nullptr, int a2_mode = GNNREC_A2_NONE) {
  const int64_t M = A.size(0), K1 = A.size(1), N = W.size(0);
  const int64_t K2 = A2 ? A2->size(1) : 0;
  ck(gnnrec_gemm_rownorm_f32(p<float>(A), ld(A, "A"), K1, p<float>(W), A2 ? p<float>(*A2) : nullptr,
                             A2 ? ld(*A2, "A2") : 1, K2, W2 ? p<float>(*W2) : nullptr, a2_deg,
                             a2_mode, bias, bias_ne, M, N, epi, accum, 0.f,
                             nullptr, nullptr, p<float>(out), ld(out, "out"),
                             row_norm ? p<float>(*row_norm) : nullptr, stream_of(A)),
     "gnnrec_gemm_f32");
  return out;
}

// guᵀ X, split-K MFMA; colsum (nullable, [M]) receives Σ_k gu[k] from the same pass — over
// the rows with row_ptr[k+1] > row_ptr[k] only, when row_ptr is given
Tensor weight_grad(const Tensor& gu, const Tensor& X, Tensor* colsum = nullptr,
                   const Tensor* row_ptr = nullptr) {
  const int64_t K = gu.size(0), M = gu.size(1), N = X.size(1);
  Tensor out = at::empty({M, N}, gu.options());
  const int64_t wsb = gnnrec_gemm_tn_workspace_bytes(K, M, N);
  Tensor ws = at::empty({std::max<int64_t>(wsb / 4, 1)}, gu.options());
  ck(gnnrec_gemm_tn_bias_rows_f32(p<float>(gu), ld(gu, "gu"), p<float>(X), ld(X, "X"), K, M, N,
                                  p<float>(out), ld(out, "out"),
                                  colsum ? p<float>(*colsum) : nullptr,
                                  row_ptr ? p<int64_t>(*row_ptr) : nullptr, 0, p<float>(ws),
                                  stream_of(gu)),
     "gnnrec_gemm_tn_bias_rows_f32");
  return out;
}

// int32 in-degrees of a CSR's rows (the GEMM epilogue's non-empty test for bias_nonempty)
Tensor row_degrees(const Tensor& indptr) {
  const int64_t M = indptr.numel() - 1;
  return (indptr.narrow(0, 1, M) - indptr.narrow(0, 0, M)).to(at::kInt).contiguous();
}

// gather of X over a CSR whose edge count is known on the host but whose degrees are
// not (the transposed block, a static-shape block's dump row): heavy rows planned on the
// device, as ops.spmm does
//
// drop (nullable): the gather with the dropout mask inside (csrc/dropout.hip), by gathered
// row (GNNREC_DROPOUT_SRC) or at the store of the output row (GNNREC_DROPOUT_OUT)
struct Drop {
  const uint64_t* keys;
  int64_t index;
  double p;
  int where;
};

// the keys tensor of a forward call (int64 storage of the uint64 keys) and one stream of it
const uint64_t* drop_keys_ptr(const optional<Tensor>& keys, std::initializer_list<int64_t> idx) {
  TORCH_CHECK_VALUE(has(keys), "dropout: p > 0 needs the keys tensor of the forward call");
  dev(keys, "drop_keys", at::kLong);
  TORCH_CHECK_VALUE(keys->is_contiguous(), "dropout: keys must be contiguous");
  for (const int64_t i : idx)
    TORCH_CHECK_VALUE(i >= 0 && i < keys->numel(), "dropout: stream ", i, " outside the ",
                      keys->numel(), " keys");
  return keys->is_meta() ? nullptr : reinterpret_cast<const uint64_t*>(keys->data_ptr());
}

void gather_planned(const Tensor& ip, const Tensor& ix, const Tensor& w, const Tensor& X,
                    int64_t nnz, Tensor& out, bool accumulate = false,
                    int reduce = GNNREC_REDUCE_SUM, const int64_t* live = nullptr,
                    const Drop* drop = nullptr) {
  const int64_t n = ip.numel() - 1, d = X.size(1);
  const int64_t cap_h = std::min<int64_t>(n, nnz / (kSplit + 1));
  void* s = stream_of(X);
  const int flags = accumulate ? GNNREC_SPMM_ACCUM : 0;
  if (cap_h <= 0) {
    if (drop) {
      ck(gnnrec_spmm_csr_dropout_live_f32(p<int64_t>(ip), p<int32_t>(ix), pw(w), p<float>(X),
                                          ld(X, "X"), n, d, reduce, flags, p<float>(out),
                                          ld(out, "out"), live, drop->keys, drop->index, drop->p,
                                          drop->where, s),
         "gnnrec_spmm_csr_dropout_f32");
      return;
    }
    ck(gnnrec_spmm_csr_live_f32(p<int64_t>(ip), p<int32_t>(ix), pw(w), p<float>(X), ld(X, "X"), n,
                                d, reduce, flags, p<float>(out), ld(out, "out"), live, s),
       "gnnrec_spmm_csr_f32");
    return;
  }
  const int64_t cap_c = nnz / kSplit + cap_h;
  Tensor plan = at::empty({2 + cap_h + cap_h + 1 + cap_c}, ip.options());
  ck(gnnrec_spmm_plan_build_live(p<int64_t>(ip), n, kSplit, cap_h, cap_c, p<int64_t>(plan), live,
                                 s),
     "gnnrec_spmm_plan_build");
  Tensor wsp = at::empty({cap_c, d}, X.options());
  if (drop) {
    ck(gnnrec_spmm_csr_planned_dropout_live_f32(
           p<int64_t>(ip), p<int32_t>(ix), pw(w), p<float>(X), ld(X, "X"), n, d, reduce, flags,
           p<float>(out), ld(out, "out"), kSplit, p<int64_t>(plan), cap_h, cap_c, p<float>(wsp),
           live, drop->keys, drop->index, drop->p, drop->where, s),
       "gnnrec_spmm_csr_planned_dropout_f32");
    return;
  }
  ck(gnnrec_spmm_csr_planned_live_f32(p<int64_t>(ip), p<int32_t>(ix), pw(w), p<float>(X),
                                      ld(X, "X"), n, d, reduce, flags, p<float>(out),
                                      ld(out, "out"), kSplit, p<int64_t>(plan), cap_h, cap_c,
                                      p<float>(wsp), live, s),
     "gnnrec_spmm_csr_planned_f32");
}

// x[:n] ⊙ mask · scale into out[:n] (stored, or added under accumulate); out may be x
void drop_rows(const Tensor& x, int64_t n, const uint64_t* keys, int64_t index, double p_drop,
               bool accumulate, Tensor& out) {
  ck(gnnrec_dropout_rows_f32(p<float>(x), ld(x, "x"), n, x.size(1), keys, index, p_drop,
                             (int)accumulate, p<float>(out), ld(out, "out"), stream_of(x)),
     "gnnrec_dropout_rows_f32");
}
}  // namespace

// ---------------------------------------------------------------- training dropout
// keys[i] = hash3(seed, *counter, stream0 + i), then *counter += 1, in one launch
void dropout_keys(int64_t seed, Tensor& counter, int64_t stream0, Tensor& keys) {
  const OneDevice one_device_;
  dev(counter, "counter", at::kLong);
  dev(keys, "keys", at::kLong);
  TORCH_CHECK_VALUE(counter.numel() == 1 && keys.is_contiguous() && stream0 >= 0,
                    "dropout_keys: one counter, contiguous keys, stream0 >= 0");
  if (meta(keys)) return;
  const c10::DeviceGuard g(keys.device());
  ck(gnnrec_dropout_keys((uint64_t)seed, p<int64_t>(counter), stream0, keys.numel(),
                         reinterpret_cast<uint64_t*>(p<int64_t>(keys)), stream_of(keys)),
     "gnnrec_dropout_keys");
}

void dropout_rows_f32(const Tensor& x, int64_t n, const Tensor& keys, int64_t key_index,
                      double p_drop, bool accumulate, Tensor& out) {
  const OneDevice one_device_;
  dev(x, "x", at::kFloat);
  dev(out, "out", at::kFloat);
  TORCH_CHECK_VALUE(x.dim() == 2 && out.dim() == 2 && n >= 0 && x.size(0) >= n &&
                        out.size(0) >= n && out.size(1) == x.size(1),
                    "dropout_rows: x and out must hold n rows of one width");
  const uint64_t* k = drop_keys_ptr(keys, {key_index});
  ld(x, "x");
  ld(out, "out");
  if (meta(x)) return;
  const c10::DeviceGuard g(x.device());
  drop_rows(x, n, k, key_index, p_drop, accumulate, out);
}

// the sum / mean gathers with the dropout mask inside (gnnrec_spmm_csr_dropout_live_f32 and
// its planned form): spmm_csr / spmm_csr_planned with the keys, the stream, p and the side
void spmm_csr_dropout_live_f32(const Tensor& indptr, const Tensor& indices,
                               const optional<Tensor>& ew, const Tensor& X, int64_t reduce,
                               int64_t flags, Tensor& out, const optional<Tensor>& live,
                               const Tensor& keys, int64_t key_index, double p_drop,
                               int64_t where) {
  const OneDevice one_device_;
  dev(indptr, "indptr", at::kLong);
  dev(indices, "indices", at::kInt);
  dev(X, "X", at::kFloat);
  dev(ew, "edge_weight", at::kFloat);
  dev(out, "out", at::kFloat);
  const int64_t n_dst = indptr.numel() - 1, d = X.size(1);
  TORCH_CHECK_VALUE(out.size(0) == n_dst && out.size(1) == d, "out must be [", n_dst, ", ", d,
                    "], got ", out.sizes());
  const uint64_t* k = drop_keys_ptr(keys, {key_index});
  const int64_t ldx = ld(X, "X"), ldo = ld(out, "out");
  if (meta(X)) return;
  const c10::DeviceGuard g(X.device());
  ck(gnnrec_spmm_csr_dropout_live_f32(p<int64_t>(indptr), p<int32_t>(indices), p<float>(ew),
                                      p<float>(X), ldx, n_dst, d, (int)reduce, (int)flags,
                                      p<float>(out), ldo, live_ptr(live), k, key_index, p_drop,
                                      (int)where, stream_of(X)),
     "gnnrec_spmm_csr_dropout_f32");
}

void spmm_csr_planned_dropout_live_f32(const Tensor& indptr, const Tensor& indices,
                                       const optional<Tensor>& ew, const Tensor& X,
                                       int64_t reduce, int64_t flags, int64_t split,
                                       const Tensor& plan, int64_t cap_h, int64_t cap_c,
                                       Tensor& out, Tensor& ws, const optional<Tensor>& live,
                                       const Tensor& keys, int64_t key_index, double p_drop,
                                       int64_t where) {
  const OneDevice one_device_;
  dev(indptr, "indptr", at::kLong);
  dev(indices, "indices", at::kInt);
  dev(X, "X", at::kFloat);
  dev(ew, "edge_weight", at::kFloat);
  dev(plan, "plan", at::kLong);
  dev(out, "out", at::kFloat);
  dev(ws, "workspace", at::kFloat);
  const int64_t n_dst = indptr.numel() - 1, d = X.size(1);
  TORCH_CHECK_VALUE(out.size(0) == n_dst && out.size(1) == d, "out must be [", n_dst, ", ", d, "]");
  TORCH_CHECK_VALUE(cap_h >= 0 && cap_c >= 0 && plan.numel() >= 3 + 2 * cap_h + cap_c,
                    "plan shorter than 3 + 2 cap_h + cap_c");
  TORCH_CHECK_VALUE(ws.numel() >= cap_c * d, "workspace must hold cap_c x d floats");
  const uint64_t* k = drop_keys_ptr(keys, {key_index});
  const int64_t ldx = ld(X, "X"), ldo = ld(out, "out");
  if (meta(X)) return;
  const c10::DeviceGuard g(X.device());
  ck(gnnrec_spmm_csr_planned_dropout_live_f32(
         p<int64_t>(indptr), p<int32_t>(indices), p<float>(ew), p<float>(X), ldx, n_dst, d,
         (int)reduce, (int)flags, p<float>(out), ldo, split, p<int64_t>(plan), cap_h, cap_c,
         p<float>(ws), live_ptr(live), k, key_index, p_drop, (int)where, stream_of(X)),
     "gnnrec_spmm_csr_planned_dropout_f32");
}

// host only: the keep mask as a CPU uint8 tensor [n_rows, d], and the scale of p
Tensor dropout_mask_host(int64_t seed, int64_t step, int64_t stream, int64_t n_rows, int64_t d,
                         double p_drop) {
  TORCH_CHECK_VALUE(n_rows >= 0 && d >= 0, "dropout_mask_host: negative size");
  Tensor keep = at::empty({n_rows, d}, at::TensorOptions().dtype(at::kByte));
  ck(gnnrec_dropout_mask_host((uint64_t)seed, (uint64_t)step, (uint64_t)stream, n_rows, d, p_drop,
                              keep.data_ptr<uint8_t>()),
     "gnnrec_dropout_mask_host");
  return keep;
}

double dropout_scale(double p_drop) { return gnnrec_dropout_scale(p_drop); }

std::tuple<Tensor, Tensor, Tensor> sage_rel_forward(const Tensor& m, const Tensor& h_self,
                                                    int64_t n_self, const Tensor& Ws,
                                                    const Tensor& Wn, const Tensor& indptr,
                                                    const Tensor& indices,
                                                    const optional<Tensor>& ew, int64_t reduce,
                                                    bool norm, const optional<Tensor>& bias,
                                                    const optional<Tensor>& bias_ne,
                                                    const optional<Tensor>& live, double drop_p,
                                                    const optional<Tensor>& drop_keys,
                                                    int64_t drop_neigh, int64_t drop_self) {
  const OneDevice one_device_;
  dev(m, "m", at::kFloat);
  dev(h_self, "h_self", at::kFloat);
  dev(Ws, "W_self", at::kFloat);
  dev(Wn, "W_neigh", at::kFloat);
  dev(indptr, "indptr", at::kLong);
  dev(indices, "indices", at::kInt);
  dev(ew, "edge_weight", at::kFloat);
  TORCH_CHECK_VALUE(reduce == GNNREC_REDUCE_SUM || reduce == GNNREC_REDUCE_MEAN,
                    "sage_rel_forward: sum or mean");
  const int64_t M = indptr.numel() - 1, N = Ws.size(0);
  TORCH_CHECK_VALUE(N <= 256 || !norm, "sage_rel_forward: the row norm needs N <= 256");
  TORCH_CHECK_VALUE(h_self.size(0) >= M && (n_self == 0 || n_self == M),
                    "sage_rel_forward: h_self must hold the ", M, " destination rows first");
  TORCH_CHECK_VALUE(Wn.size(0) == N && Ws.size(1) == h_self.size(1) && Wn.size(1) == m.size(1),
                    "sage_rel_forward: weight shapes");
  // bias (every row) and bias_ne (rows with an in-edge): a NodeEmbedding folded into the
  // layer (autograd.HeteroSageFn's first-layer fold): W_self b_e and W_neigh b_e
  dev(bias, "bias", at::kFloat);
  dev(bias_ne, "bias_nonempty", at::kFloat);
  TORCH_CHECK_VALUE((!has(bias) || bias->numel() == N) && (!has(bias_ne) || bias_ne->numel() == N),
                    "sage_rel_forward: biases must have ", N, " entries");
  // drop_p > 0: dropout inside the node (csrc/dropout.hip).  The neighbour mask is applied to
  // every gathered row of m (stream drop_neigh, rows = m's rows), the self mask to a dropped
  // copy of the M destination rows (stream drop_self); no dropped copy of m is written
  const bool drop = drop_p > 0.0;
  const uint64_t* dkeys = drop ? drop_keys_ptr(drop_keys, {drop_neigh, drop_self}) : nullptr;
  TORCH_CHECK_VALUE(!drop || (!has(bias) && !has(bias_ne)),
                    "sage_rel_forward: a folded embedding and dropout exclude each other");
  const Tensor X = m.contiguous();
  Tensor H = h_self.narrow(0, 0, M).contiguous();
  const Tensor bc = has(bias) ? bias->contiguous() : Tensor();
  const Tensor bnc = has(bias_ne) ? bias_ne->contiguous() : Tensor();
  const optional<Tensor> ewc = has(ew) ? optional<Tensor>(ew->contiguous()) : ew;
  const Tensor Wsc = Ws.contiguous(), Wnc = Wn.contiguous();
  Tensor agg = at::empty({M, m.size(1)}, m.options());
  Tensor z = at::empty({M, N}, m.options());
  Tensor nrm = norm ? at::empty({M}, m.options()) : at::empty({0}, m.options());
  if (meta(m)) return {z, agg, nrm};
  const c10::DeviceGuard g(m.device());
  // live: the static block's real destination count on the device (its padding and dump
  // rows aggregate nothing: their outputs feed no real row and get no gradient)
  // The forward blocks' rows are bounded (fanout rows; a static block's dump rows hold at
  // most kDumpEdges = the heavy-row split), so the gather needs no heavy-row plan; a
  // full-neighbour block's long rows run unsplit (one wave each, the same values)
  const int64_t* lv = live_ptr(live);
  if (drop) {
    ck(gnnrec_spmm_csr_dropout_live_f32(p<int64_t>(indptr), p<int32_t>(indices), p<float>(ewc),
                                        p<float>(X), ld(X, "m"), M, X.size(1), (int)reduce, 0,
                                        p<float>(agg), ld(agg, "agg"), lv, dkeys, drop_neigh,
                                        drop_p, GNNREC_DROPOUT_SRC, stream_of(m)),
       "gnnrec_spmm_csr_dropout_f32");
    Tensor Hd = at::empty({M, h_self.size(1)}, m.options());
    drop_rows(H, M, dkeys, drop_self, drop_p, false, Hd);
    H = Hd;
  } else {
    ck(gnnrec_spmm_csr_live_f32(p<int64_t>(indptr), p<int32_t>(indices), p<float>(ewc),
                                p<float>(X), ld(X, "m"), M, X.size(1), (int)reduce, 0,
                                p<float>(agg), ld(agg, "agg"), lv, stream_of(m)),
       "gnnrec_spmm_csr_f32");
  }
  // bias_ne's non-empty test reads the block CSR's indptr directly (GNNREC_A2_DEG_INDPTR)
  const Tensor ipc = bnc.defined() ? indptr.contiguous() : Tensor();
  gemm_nt(H, Wsc, &agg, &Wnc, GNNREC_EPI_RELU | (norm ? GNNREC_EPI_L2NORM : 0), z,
          norm ? &nrm : nullptr, GNNREC_ACC_STORE, bc.defined() ? p<float>(bc) : nullptr,
          bnc.defined() ? p<float>(bnc) : nullptr,
          ipc.defined() ? reinterpret_cast<const int32_t*>(p<int64_t>(ipc)) : nullptr,
          ipc.defined() ? GNNREC_A2_DEG_INDPTR : GNNREC_A2_NONE);
  return {z, agg, nrm};
}

std::tuple<Tensor, Tensor, Tensor, Tensor, Tensor, Tensor> sage_rel_backward(
    const Tensor& gz_in, const Tensor& z, const Tensor& row_norm, const Tensor& h_self,
    const Tensor& agg, const Tensor& Ws, const Tensor& Wn, const Tensor& indptr,
    const Tensor& indices, const optional<Tensor>& ew, int64_t reduce, int64_t n_src,
    int64_t nnz, bool norm, int64_t need, const optional<Tensor>& indptr_t_in,
    const optional<Tensor>& indices_t_in, const optional<Tensor>& w_mean_in,
    const optional<Tensor>& g_self_out, bool g_self_acc, const optional<Tensor>& g_m_out,
    bool g_m_acc, const optional<Tensor>& live_src, double drop_p,
    const optional<Tensor>& drop_keys, int64_t drop_neigh, int64_t drop_self) {
  // drop_*: the forward's dropout arguments and the keys tensor it read (the same masks)
  // need bits: 1 g_self, 2 g_m, 4 g_Ws, 8 g_Wn, 16 g_bias (Σ rows of the pre-activation
  // gradient), 32 g_bias_nonempty (the same over rows with an in-edge)
  const OneDevice one_device_;
  dev(gz_in, "gz", at::kFloat);
  dev(z, "z", at::kFloat);
  dev(h_self, "h_self", at::kFloat);
  dev(agg, "agg", at::kFloat);
  dev(Ws, "W_self", at::kFloat);
  dev(Wn, "W_neigh", at::kFloat);
  dev(indptr, "indptr", at::kLong);
  dev(indices, "indices", at::kInt);
  dev(ew, "edge_weight", at::kFloat);
  const int64_t M = z.size(0), N = z.size(1);
  TORCH_CHECK_VALUE(gz_in.sizes() == z.sizes() && agg.size(0) == M && h_self.size(0) >= M &&
                        indptr.numel() == M + 1 && (!norm || row_norm.numel() == M),
                    "sage_rel_backward: shapes");
  const Tensor gz = gz_in.contiguous();
  // g_self_out / g_m_out: a layer's gradient tables (autograd.HeteroSageFn) written in place
  // — stored, or accumulated when *_acc — instead of fresh tensors that autograd then adds
  dev(g_self_out, "g_self_out", at::kFloat);
  dev(g_m_out, "g_m_out", at::kFloat);
  TORCH_CHECK_VALUE(!has(g_self_out) || (g_self_out->is_contiguous() &&
                                         g_self_out->size(0) == h_self.size(0) &&
                                         g_self_out->size(1) == Ws.size(1)),
                    "sage_rel_backward: g_self_out must be a contiguous [h_self rows, d_self]");
  TORCH_CHECK_VALUE(!has(g_m_out) || (g_m_out->is_contiguous() && g_m_out->size(0) == n_src &&
                                      g_m_out->size(1) == Wn.size(1)),
                    "sage_rel_backward: g_m_out must be a contiguous [n_src, d_neigh]");
  Tensor none = at::empty({0}, z.options());  // outputs not asked for (`need` bits)
  Tensor g_self = none, g_m = none, g_Ws = none, g_Wn = none, g_b = none, g_bne = none;
  if (meta(z)) {
    if ((need & 1) && !has(g_self_out)) g_self = at::empty({h_self.size(0), Ws.size(1)}, z.options());
    if ((need & 2) && !has(g_m_out)) g_m = at::empty({n_src, Wn.size(1)}, z.options());
    if (need & 4) g_Ws = at::empty_like(Ws);
    if (need & 8) g_Wn = at::empty_like(Wn);
    if (need & 16) g_b = at::empty({N}, z.options());
    if (need & 32) g_bne = at::empty({N}, z.options());
    return {g_self, g_m, g_Ws, g_Wn, g_b, g_bne};
  }
  const bool drop = drop_p > 0.0;
  const uint64_t* dkeys = drop ? drop_keys_ptr(drop_keys, {drop_neigh, drop_self}) : nullptr;
  const c10::DeviceGuard g(z.device());
  void* s = stream_of(z);
  Tensor gu = at::empty({M, N}, z.options());
  if (norm) {
    dev(row_norm, "row_norm", at::kFloat);
    ck(gnnrec_act_backward_normed_f32(p<float>(z), ld(z, "z"), p<float>(row_norm), p<float>(gz),
                                      ld(gz, "gz"), M, N, 1, p<float>(gu), N, s),
       "gnnrec_act_backward_normed_f32");
  } else {  // z = relu(u): the same mask
    ck(gnnrec_act_backward_f32(p<float>(z), ld(z, "z"), p<float>(gz), ld(gz, "gz"), M, N,
                               GNNREC_EPI_RELU, p<float>(gu), N, s),
       "gnnrec_act_backward_f32");
  }
  if (need & 1) {  // gu Ws over the whole source table of the dst type (zero past M)
    const bool acc = has(g_self_out) && g_self_acc;
    g_self = has(g_self_out) ? *g_self_out : at::empty({h_self.size(0), Ws.size(1)}, z.options());
    Tensor head = g_self.narrow(0, 0, M);
    if (drop) {
      // (gu Ws) ⊙ the self mask: in place when stored; through a copy of the M rows when the
      // table already holds other relations' gradient, which the mask must not touch
      Tensor t = acc ? at::empty({M, Ws.size(1)}, z.options()) : head;
      gemm_nt(gu, Ws.t().contiguous(), nullptr, nullptr, 0, t, nullptr);
      drop_rows(t, M, dkeys, drop_self, drop_p, acc, head);
    } else {
      gemm_nt(gu, Ws.t().contiguous(), nullptr, nullptr, 0, head, nullptr,
              acc ? GNNREC_ACC_ADD : GNNREC_ACC_STORE);
    }
    if (!acc && h_self.size(0) > M) g_self.narrow(0, M, h_self.size(0) - M).zero_();
  }
  if (need & 2) {  // transposed gather of g_agg = gu Wn (DGL: the backward of a gSpMM)
    Tensor g_agg = at::empty({M, Wn.size(1)}, z.options());
    gemm_nt(gu, Wn.t().contiguous(), nullptr, nullptr, 0, g_agg, nullptr);
    const bool mean = reduce == GNNREC_REDUCE_MEAN;
    Tensor ip_t, ix_t, w_t;
    if (has(indptr_t_in) && !has(ew)) {
      // the block's source-major CSR, built by the sampler (block_transposes) beside the
      // block itself: no sort on the training thread
      TORCH_CHECK_VALUE(indptr_t_in->numel() == n_src + 1 && has(indices_t_in) &&
                            (!mean || has(w_mean_in)),
                        "sage_rel_backward: precomputed transpose does not fit the block");
      ip_t = *indptr_t_in;
      ix_t = *indices_t_in;
      if (mean) w_t = *w_mean_in;
    } else {
      ip_t = at::empty({n_src + 1}, indptr.options());
      ix_t = at::empty({std::max<int64_t>(nnz, 1)}, indices.options());
      if (has(ew) || mean) w_t = at::empty({std::max<int64_t>(nnz, 1)}, z.options());
      const size_t wsb = gnnrec_csr_transpose_workspace_bytes(nnz, n_src);
      Tensor ws = at::empty({(int64_t)std::max<size_t>(wsb, 1)},
                            indptr.options().dtype(at::kByte));
      const optional<Tensor> ewc = has(ew) ? optional<Tensor>(ew->contiguous()) : ew;
      ck(gnnrec_csr_transpose(p<int64_t>(indptr), p<int32_t>(indices), p<float>(ewc), M, n_src,
                              nnz, (int)mean, ws.data_ptr(), ws.nbytes(), p<int64_t>(ip_t),
                              p<int32_t>(ix_t), pw(w_t), s),
         "gnnrec_csr_transpose");
    }
    g_m = has(g_m_out) ? *g_m_out : at::empty({n_src, Wn.size(1)}, z.options());
    // live_src: the static block's real source count (its padding sources' gradient rows
    // are zero: only padding rows, whose gradient is zero, point at them)
    // dropout: the mask of the source row at the store of its gradient row
    const Drop dm{dkeys, drop_neigh, drop_p, GNNREC_DROPOUT_OUT};
    gather_planned(ip_t, ix_t, w_t, g_agg, nnz, g_m, has(g_m_out) && g_m_acc, GNNREC_REDUCE_SUM,
                   live_ptr(live_src), drop ? &dm : nullptr);
  }
  if (need & 16) g_b = at::empty({N}, z.options());
  if (need & 4) {
    Tensor Hs = h_self.narrow(0, 0, M).contiguous();
    if (drop) {  // the dropped self rows the forward projected, regenerated
      Tensor Hd = at::empty({M, h_self.size(1)}, z.options());
      drop_rows(Hs, M, dkeys, drop_self, drop_p, false, Hd);
      Hs = Hd;
    }
    g_Ws = weight_grad(gu, Hs, (need & 16) ? &g_b : nullptr);
  } else if (need & 16) {
    g_b = gu.sum(0);
  }
  // g_bne: Σ over the rows with an in-edge (the mean of an empty set carries no bias), from
  // the W_neigh gradient's own pass over gu
  if (need & 32) g_bne = at::empty({N}, z.options());
  if (need & 8) {
    const Tensor ip = indptr.contiguous();
    g_Wn = weight_grad(gu, agg.contiguous(), (need & 32) ? &g_bne : nullptr,
                       (need & 32) ? &ip : nullptr);
  } else if (need & 32) {
    const Tensor ne = (row_degrees(indptr) > 0).to(gu.scalar_type()).unsqueeze(1);
    g_bne = (gu * ne).sum(0);
  }
  // gradients written in place come back as empty tensors (the caller holds the tables)
  return {has(g_self_out) ? none : g_self, has(g_m_out) ? none : g_m, g_Ws, g_Wn, g_b, g_bne};
}

// Every relation's source-major CSR of one sampled block, in one call (the sampler's
// training side, gnnrec/sampling.py): (indptr_t, dst rows, 1/deg(dst) per edge) per relation,
// the transposes the aggregation backward gathers over (sage_rel_backward).
std::tuple<std::vector<Tensor>, std::vector<Tensor>, std::vector<Tensor>> block_transposes(
    at::TensorList indptrs, at::TensorList indices, at::IntArrayRef n_src,
    at::IntArrayRef nnz) {
  const OneDevice one_device_;
  const size_t R = indptrs.size();
  TORCH_CHECK_VALUE(indices.size() == R && n_src.size() == R && nnz.size() == R,
                    "block_transposes: one entry per relation");
  std::vector<Tensor> ips(R), ixs(R), ws_(R);
  for (size_t r = 0; r < R; ++r) {
    dev(indptrs[r], "indptr", at::kLong);
    dev(indices[r], "indices", at::kInt);
    const int64_t E = nnz[r], ns = n_src[r];
    TORCH_CHECK_VALUE(indices[r].numel() >= E && ns >= 0, "block_transposes: sizes");
    ips[r] = at::empty({ns + 1}, indptrs[r].options());
    ixs[r] = at::empty({std::max<int64_t>(E, 1)}, indices[r].options());
    ws_[r] = at::empty({std::max<int64_t>(E, 1)}, indptrs[r].options().dtype(at::kFloat));
    if (meta(indptrs[r])) continue;
    const c10::DeviceGuard g(indptrs[r].device());
    const size_t wsb = gnnrec_csr_transpose_workspace_bytes(E, ns);
    Tensor ws = at::empty({(int64_t)std::max<size_t>(wsb, 1)},
                          indptrs[r].options().dtype(at::kByte));
    ck(gnnrec_csr_transpose(p<int64_t>(indptrs[r]), p<int32_t>(indices[r]), nullptr,
                            indptrs[r].numel() - 1, ns, E, 1, ws.data_ptr(), ws.nbytes(),
                            p<int64_t>(ips[r]), p<int32_t>(ixs[r]), p<float>(ws_[r]),
                            stream_of(indptrs[r])),
       "gnnrec_csr_transpose");
  }
  return {ips, ixs, ws_};
}

// K10 membership: has_edges_between over a source-sorted in-CSR
void csr_has_edges(const Tensor& indptr, const Tensor& sorted_indices, int64_t n_src, const Tensor& u,
               const Tensor& v, Tensor& out) {
  const OneDevice one_device_;
  dev(indptr, "indptr", at::kLong);
  dev(sorted_indices, "sorted_indices", at::kInt);
  dev(u, "u", at::kLong);
  dev(v, "v", at::kLong);
  dev(out, "out", at::kBool);
  const int64_t n = u.numel();
  TORCH_CHECK_VALUE(v.numel() == n && out.numel() == n && u.is_contiguous() && v.is_contiguous() &&
                        out.is_contiguous() && indptr.numel() >= 1,
                    "has_edges: contiguous u, v, out of one length and a non-empty indptr");
  if (meta(u)) return;
  const c10::DeviceGuard g(u.device());
  ck(gnnrec_csr_has_edges(p<int64_t>(indptr), p<int32_t>(sorted_indices), indptr.numel() - 1,
                          n_src, p<int64_t>(u), p<int64_t>(v), n,
                          reinterpret_cast<uint8_t*>(out.data_ptr()), stream_of(u)),
     "gnnrec_csr_has_edges");
}

// ---------------------------------------------------------------- sharded-pass helpers
void add_(Tensor& a, const Tensor& b) {
  const OneDevice one_device_;
  dev(a, "a", at::kFloat);
  dev(b, "b", at::kFloat);
  TORCH_CHECK_VALUE(a.sizes() == b.sizes() && a.is_contiguous() && b.is_contiguous(),
                    "add_: operands must be contiguous and of one shape");
  if (meta(a)) return;
  const c10::DeviceGuard g(a.device());
  ck(gnnrec_add_f32(p<float>(a), p<float>(b), p<float>(a), a.numel(), stream_of(a)),
     "gnnrec_add_f32");
}

void tree_sum_(Tensor& a, at::TensorList rest) {
  const OneDevice one_device_;
  dev(a, "part", at::kFloat);
  const int n = (int)rest.size() + 1;
  TORCH_CHECK_VALUE(n == 2 || n == 4 || n == 8, "tree_sum_: 2, 4 or 8 tables");
  TORCH_CHECK_VALUE(a.is_contiguous(), "tree_sum_: operands must be contiguous");
  for (const Tensor& t : rest) {
    dev(t, "part", at::kFloat);
    TORCH_CHECK_VALUE(t.sizes() == a.sizes() && t.is_contiguous(),
                      "tree_sum_: operands must be contiguous and of one shape");
  }
  if (meta(a)) return;
  std::vector<const float*> parts{p<float>(a)};
  for (const Tensor& t : rest) parts.push_back(p<float>(t));
  const c10::DeviceGuard g(a.device());
  ck(gnnrec_tree_sum_f32(parts.data(), n, a.numel(), p<float>(a), stream_of(a)),
     "gnnrec_tree_sum_f32");
}

// ---------------------------------------------------------------- f4 LSTM reducer
void lstm_step(const Tensor& P, const Tensor& indptr, const Tensor& indices, const Tensor& order,
               int64_t t, int64_t n_act, const Tensor& h_in, Tensor& h_out, Tensor& c,
               const Tensor& W_hhT, Tensor& out) {
  const OneDevice one_device_;
  dev(P, "P", at::kFloat);
  dev(indptr, "indptr", at::kLong);
  dev(indices, "indices", at::kInt);
  dev(order, "order", at::kLong);
  dev(h_in, "h_in", at::kFloat);
  dev(h_out, "h_out", at::kFloat);
  dev(c, "c", at::kFloat);
  dev(W_hhT, "W_hhT", at::kFloat);
  dev(out, "out", at::kFloat);
  const int64_t d = h_in.size(1);
  TORCH_CHECK_VALUE(W_hhT.size(0) == d && W_hhT.size(1) == 4 * d && W_hhT.is_contiguous(),
                    "W_hhT must be a contiguous [d, 4d]");
  const int64_t ldp = ld(P, "P"), ldo = ld(out, "out");
  if (meta(P)) return;
  const c10::DeviceGuard g(P.device());
  ck(gnnrec_lstm_step_f32(p<float>(P), ldp, p<int64_t>(indptr), p<int32_t>(indices),
                          p<int64_t>(order), t, n_act, p<float>(h_in), p<float>(h_out),
                          p<float>(c), d, p<float>(W_hhT), p<float>(out), ldo, stream_of(P)),
     "gnnrec_lstm_step_f32");
}

// training: the step with its state kept (step-major packing), one step of BPTT, and the
// slots' source rows / previous-step slots (gnnrec_lstm_step_save_f32 & co., lstm.hip)
void lstm_step_save(const Tensor& P, const Tensor& indptr, const Tensor& indices,
                    const Tensor& order, int64_t t, int64_t n_act, const Tensor& h_in,
                    Tensor& h_out, const optional<Tensor>& c_in, Tensor& c_out, Tensor& z_out,
                    const Tensor& W_hhT, Tensor& out) {
  const OneDevice one_device_;
  dev(P, "P", at::kFloat);
  dev(indptr, "indptr", at::kLong);
  dev(indices, "indices", at::kInt);
  dev(order, "order", at::kLong);
  dev(h_in, "h_in", at::kFloat);
  dev(h_out, "h_out", at::kFloat);
  dev(c_in, "c_in", at::kFloat);
  dev(c_out, "c_out", at::kFloat);
  dev(z_out, "z_out", at::kFloat);
  dev(W_hhT, "W_hhT", at::kFloat);
  dev(out, "out", at::kFloat);
  const int64_t d = h_out.size(1);
  TORCH_CHECK_VALUE(W_hhT.size(0) == d && W_hhT.size(1) == 4 * d && W_hhT.is_contiguous(),
                    "W_hhT must be a contiguous [d, 4d]");
  for (const Tensor* x : std::initializer_list<const Tensor*>{&h_in, &h_out, &c_out})
    TORCH_CHECK_VALUE(x->is_contiguous() && x->dim() == 2 && x->size(0) >= n_act &&
                          x->size(1) == d,
                      "h_in / h_out / c_out must be contiguous [>= n_act, d]");
  TORCH_CHECK_VALUE(!has(c_in) || (c_in->is_contiguous() && c_in->size(0) >= n_act &&
                                   c_in->size(1) == d),
                    "c_in must be a contiguous [>= n_act, d]");
  TORCH_CHECK_VALUE(z_out.is_contiguous() && z_out.size(0) >= n_act && z_out.size(1) == 4 * d,
                    "z_out must be a contiguous [>= n_act, 4d]");
  TORCH_CHECK_VALUE(order.numel() >= n_act, "order shorter than n_act");
  const int64_t ldp = ld(P, "P"), ldo = ld(out, "out");
  if (meta(P)) return;
  const c10::DeviceGuard g(P.device());
  ck(gnnrec_lstm_step_save_f32(p<float>(P), ldp, p<int64_t>(indptr), p<int32_t>(indices),
                               p<int64_t>(order), t, n_act, p<float>(h_in), p<float>(h_out),
                               p<float>(c_in), p<float>(c_out), p<float>(z_out), d,
                               p<float>(W_hhT), p<float>(out), ldo, stream_of(P)),
     "gnnrec_lstm_step_save_f32");
}

void lstm_backward_step(const Tensor& z, const Tensor& c_t, const optional<Tensor>& c_prev,
                        const optional<Tensor>& dh_next, const optional<Tensor>& dc_next,
                        int64_t n_next, const Tensor& g_out, const Tensor& order, int64_t n_act,
                        Tensor& dz, Tensor& dc_prev) {
  const OneDevice one_device_;
  dev(z, "z", at::kFloat);
  dev(c_t, "c_t", at::kFloat);
  dev(c_prev, "c_prev", at::kFloat);
  dev(dh_next, "dh_next", at::kFloat);
  dev(dc_next, "dc_next", at::kFloat);
  dev(g_out, "g_out", at::kFloat);
  dev(order, "order", at::kLong);
  dev(dz, "dz", at::kFloat);
  dev(dc_prev, "dc_prev", at::kFloat);
  const int64_t d = c_t.size(1);
  TORCH_CHECK_VALUE(n_next >= 0 && n_next <= n_act && order.numel() >= n_act,
                    "lstm_backward_step: need 0 <= n_next <= n_act <= order.numel()");
  auto rows = [&](const Tensor& x, int64_t n, int64_t w, const char* name) {
    TORCH_CHECK_VALUE(x.is_contiguous() && x.dim() == 2 && x.size(0) >= n && x.size(1) == w,
                      name, ": expected a contiguous [>= ", n, ", ", w, "] tensor");
  };
  rows(z, n_act, 4 * d, "z");
  rows(c_t, n_act, d, "c_t");
  if (has(c_prev)) rows(*c_prev, n_act, d, "c_prev");
  TORCH_CHECK_VALUE(n_next == 0 || (has(dh_next) && has(dc_next)),
                    "lstm_backward_step: rows carried from step t+1 need dh_next and dc_next");
  if (n_next > 0) {
    rows(*dh_next, n_next, d, "dh_next");
    rows(*dc_next, n_next, d, "dc_next");
  }
  rows(dz, n_act, 4 * d, "dz");
  rows(dc_prev, n_act, d, "dc_prev");
  TORCH_CHECK_VALUE(g_out.dim() == 2 && g_out.size(1) == d && g_out.stride(1) == 1,
                    "g_out must be [n_dst, d] with unit column stride");
  if (meta(z)) return;
  const c10::DeviceGuard g(z.device());
  ck(gnnrec_lstm_backward_step_f32(p<float>(z), p<float>(c_t), p<float>(c_prev),
                                   p<float>(dh_next), p<float>(dc_next), n_next, p<float>(g_out),
                                   g_out.stride(0), p<int64_t>(order), n_act, d, p<float>(dz),
                                   p<float>(dc_prev), stream_of(z)),
     "gnnrec_lstm_backward_step_f32");
}

void lstm_slots(const Tensor& indptr, const Tensor& indices, const Tensor& order,
                const Tensor& step_off, int64_t n_slots, Tensor& src, Tensor& prev) {
  const OneDevice one_device_;
  dev(indptr, "indptr", at::kLong);
  dev(indices, "indices", at::kInt);
  dev(order, "order", at::kLong);
  dev(step_off, "step_off", at::kLong);
  dev(src, "src", at::kLong);
  dev(prev, "prev", at::kLong);
  TORCH_CHECK_VALUE(src.numel() >= n_slots && prev.numel() >= n_slots && step_off.dim() == 1,
                    "lstm_slots: src / prev shorter than n_slots");
  if (meta(indptr)) return;
  const c10::DeviceGuard g(indptr.device());
  ck(gnnrec_lstm_slots(p<int64_t>(indptr), p<int32_t>(indices), p<int64_t>(order),
                       p<int64_t>(step_off), step_off.numel(), n_slots, p<int64_t>(src),
                       p<int64_t>(prev), stream_of(indptr)),
     "gnnrec_lstm_slots");
}

// ---------------------------------------------------------------- f2 loss
void margin_loss(const Tensor& pos, const Tensor& neg, int64_t K, double delta,
                 const optional<Tensor>& mask, const optional<Tensor>& recency, Tensor& g_pos,
                 Tensor& g_neg, Tensor& partial) {
  const OneDevice one_device_;
  dev(pos, "pos_score", at::kFloat);
  dev(neg, "neg_score", at::kFloat);
  dev(mask, "negative_mask", at::kFloat);
  dev(g_pos, "g_pos", at::kFloat);
  dev(g_neg, "g_neg", at::kFloat);
  dev(partial, "partial", at::kFloat);
  const int64_t n_pos = pos.numel();
  TORCH_CHECK_VALUE(neg.numel() == n_pos * K, "neg must hold n_pos x K scores");
  TORCH_CHECK_VALUE(pos.is_contiguous() && neg.is_contiguous(), "scores must be contiguous");
  int rec_i64 = 0;
  if (has(recency)) {
    TORCH_CHECK_VALUE(recency->scalar_type() == at::kLong || recency->scalar_type() == at::kFloat,
                      "recency must be float32 or int64");
    rec_i64 = recency->scalar_type() == at::kLong;
  }
  if (meta(pos)) return;
  const c10::DeviceGuard g(pos.device());
  ck(gnnrec_margin_loss_f32(p<float>(pos), p<float>(neg), n_pos, K, (float)delta, p<float>(mask),
                            has(recency) ? recency->data_ptr() : nullptr, rec_i64, p<float>(g_pos),
                            p<float>(g_neg), p<float>(partial), partial.numel(), stream_of(pos)),
     "gnnrec_margin_loss_f32");
}

void sum_scaled(const Tensor& x, double scale, Tensor& out) {
  const OneDevice one_device_;
  dev(x, "x", at::kFloat);
  dev(out, "out", at::kFloat);
  if (meta(x)) return;
  const c10::DeviceGuard g(x.device());
  ck(gnnrec_sum_scaled_f32(p<float>(x), x.numel(), (float)scale, p<float>(out), stream_of(x)),
     "gnnrec_sum_scaled_f32");
}

// ---------------------------------------------------------------- synthetic generator
void synth_edges(int64_t seed, int64_t e0, int64_t n_u, int64_t n_i,
                 const optional<Tensor>& zipf_cdf, Tensor& u, Tensor& i) {
  const OneDevice one_device_;
  dev(zipf_cdf, "zipf_cdf", at::kDouble);
  dev(u, "u", at::kInt);
  dev(i, "i", at::kInt);
  TORCH_CHECK_VALUE(u.numel() == i.numel(), "u and i must have one length");
  if (meta(u)) return;
  const c10::DeviceGuard g(u.device());
  ck(gnnrec_synth_edges((uint64_t)seed, e0, u.numel(), n_u, n_i, p<double>(zipf_cdf),
                        p<int32_t>(u), p<int32_t>(i), stream_of(u)),
     "gnnrec_synth_edges");
}

void hold_cus(int64_t blocks, int64_t threads, int64_t lds_bytes, int64_t usec, Tensor& sink) {
  const OneDevice one_device_;
  dev(sink, "sink", at::kFloat);
  TORCH_CHECK_VALUE(sink.numel() >= threads, "sink must hold >= threads floats");
  if (meta(sink)) return;
  const c10::DeviceGuard g(sink.device());
  ck(gnnrec_hold_cus((int)blocks, (int)threads, (int)lds_bytes, usec, p<float>(sink),
                     stream_of(sink)),
     "gnnrec_hold_cus");
}

// ---------------------------------------------------------------- host-only queries
int64_t version() { return gnnrec_version(); }
void set_concurrency(int64_t reserve_cus, bool dynamic) {
  const OneDevice one_device_;
  ck(gnnrec_set_concurrency((int)reserve_cus, (int)dynamic), "gnnrec_set_concurrency");
}
std::tuple<int64_t, int64_t> get_concurrency() {
  const OneDevice one_device_;
  int r = 0, d = 0;
  ck(gnnrec_get_concurrency(&r, &d), "gnnrec_get_concurrency");
  return {r, d};
}
int64_t spmm_plan_overflows() {
  int64_t n = 0;
  ck(gnnrec_spmm_plan_overflows(&n), "gnnrec_spmm_plan_overflows");
  return n;
}

std::tuple<int64_t, int64_t> rowq_stats() {
  const OneDevice one_device_;
  int64_t q = 0, b = 0;
  ck(gnnrec_rowq_stats(&q, &b), "gnnrec_rowq_stats");
  return {q, b};
}
int64_t scan_workspace_bytes(int64_t n) { return gnnrec_scan_workspace_bytes(n); }
int64_t gemm_tn_workspace_bytes(int64_t K, int64_t M, int64_t N) {
  const OneDevice one_device_;
  return gnnrec_gemm_tn_workspace_bytes(K, M, N);
}
int64_t csr_transpose_workspace_bytes(int64_t E, int64_t n_src) {
  const OneDevice one_device_;
  return (int64_t)gnnrec_csr_transpose_workspace_bytes(E, n_src);
}
int64_t csr_from_keys_workspace_bytes(int64_t E, int64_t n_rows) {
  const OneDevice one_device_;
  return (int64_t)gnnrec_csr_from_keys_workspace_bytes(E, n_rows);
}
int64_t csr_build_workspace_bytes(int64_t E, int64_t n_dst) {
  const OneDevice one_device_;
  return (int64_t)gnnrec_csr_build_workspace_bytes(E, n_dst);
}
int64_t cos_denominator_parts(int64_t n_items) { return gnnrec_cos_denominator_parts(n_items); }
double rank_eps(int64_t d) { return gnnrec_rank_eps(d); }
int64_t rank_list_slots() { return gnnrec_rank_list_slots(); }
int64_t csr_remove_edges_workspace_bytes(int64_t E, int64_t n_dst) {
  return (int64_t)gnnrec_csr_remove_edges_workspace_bytes(E, n_dst);
}
int64_t node_rank_table_workspace_bytes(int64_t n_nodes) {
  return (int64_t)gnnrec_node_rank_table_workspace_bytes(n_nodes);
}
int64_t csr_remove_nodes_workspace_bytes(int64_t E, int64_t n_dst) {
  return (int64_t)gnnrec_csr_remove_nodes_workspace_bytes(E, n_dst);
}
int64_t csr_add_edges_workspace_bytes(int64_t n_new, int64_t n_dst) {
  return (int64_t)gnnrec_csr_add_edges_workspace_bytes(n_new, n_dst);
}
int64_t frontier_mark_workspace_bytes(int64_t n_rows) {
  return (int64_t)gnnrec_frontier_mark_workspace_bytes(n_rows);
}
int64_t sddmm_cos_backward_workspace_bytes(int64_t E, int64_t n_src, int64_t n_dst, int64_t d,
                                           int64_t groups, int64_t K) {
  if (groups > 0)
    return (int64_t)gnnrec_sddmm_cos_backward_grouped_workspace_bytes(groups, K, n_src, n_dst, d);
  const OneDevice one_device_;
  return (int64_t)gnnrec_sddmm_cos_backward_workspace_bytes(E, n_src, n_dst, d);
}
int64_t margin_loss_blocks(int64_t n_pos) { return gnnrec_margin_loss_blocks(n_pos); }

}  // namespace

// Schemas: mutated outputs are annotated (a!) so functionalisation knows what each op
// writes; every launch op returns ().
TORCH_LIBRARY(gnnrec, m) {
  m.def("spmm_csr(Tensor indptr, Tensor indices, Tensor? edge_weight, Tensor X, int reduce, "
        "int flags, Tensor(a!) out, Tensor? live=None) -> ()");
  m.def("spmm_csr_split(Tensor indptr, Tensor indices, Tensor? edge_weight, Tensor X, "
        "int reduce, int flags, int split, Tensor heavy_rows, Tensor chunk_ptr, "
        "Tensor chunk_row, int n_chunks, Tensor(a!) out, Tensor(b!) workspace) -> ()");
  m.def("spmm_plan_build(Tensor indptr, int split, int cap_h, Tensor(a!) plan, "
        "Tensor? live=None) -> ()");
  m.def("spmm_csr2(Tensor indptr_a, Tensor indices_a, Tensor? ew_a, Tensor indptr_b, "
        "Tensor indices_b, Tensor? ew_b, Tensor X, int reduce, int flags, Tensor(a!) out_a, "
        "Tensor(b!) out_b) -> ()");
  m.def("spmm_csr_planned(Tensor indptr, Tensor indices, Tensor? edge_weight, Tensor X, "
        "int reduce, int flags, int split, Tensor plan, int cap_h, int cap_c, Tensor(a!) out, "
        "Tensor(b!) workspace, Tensor? live=None) -> ()");
  m.def("spmm_backward(Tensor indptr, Tensor indices, Tensor? edge_weight, Tensor grad_out, "
        "Tensor? X, Tensor? out, int reduce, Tensor(a!) grad_X) -> ()");
  m.def("gemm(Tensor A1, Tensor W1, Tensor? A2, Tensor? W2, Tensor? a2_deg, int a2_mode, "
        "Tensor? bias, Tensor? bias_nonempty, int epilogue, int accum, float out_div, "
        "Tensor? attn_vec, Tensor(b!)? attn_state, Tensor(a!) out, Tensor(c!)? row_norm) -> ()");
  m.def("row_epilogue(Tensor z, int l2norm, int accum, float out_div, Tensor? attn_vec, "
        "Tensor(b!)? attn_state, Tensor(a!) out) -> ()");
  m.def("spmm_project(Tensor indptr, Tensor indices, Tensor? edge_weight, Tensor X, Tensor H, "
        "Tensor W_selfT, Tensor? W_neighT, Tensor? bias, Tensor? bias_nonempty, int reduce, "
        "int epilogue, int accum, float out_div, Tensor? attn_vec, Tensor(b!)? attn_state, "
        "bool mfma, Tensor(a!) out) -> ()");
  m.def("spmm_project_agg_f32(Tensor indptr, Tensor? indices, Tensor? edge_weight, Tensor? X, "
        "Tensor H, Tensor W_selfT, Tensor W_neighT, Tensor? bias, Tensor? bias_nonempty, "
        "int reduce, int epilogue, int accum, float out_div, Tensor? attn_vec, "
        "Tensor(b!)? attn_state, Tensor(c!) agg, int agg_mode, Tensor(a!) out) -> ()");
  m.def("pack_rows_f32(Tensor X, float max_dense_frac, Tensor(a!) packed, Tensor(b!) status) "
        "-> ()");
  m.def("spmm_csr_packed_f32(Tensor indptr, Tensor indices, Tensor packed, Tensor status, "
        "Tensor X, int reduce, int flags, int split, Tensor? heavy_rows, int n_heavy, "
        "Tensor? chunk_ptr, Tensor? chunk_row, int n_chunks, Tensor? counts, Tensor(a!) out, "
        "Tensor(b!)? workspace) -> ()");
  m.def("spmm_project2(Tensor indptr_a, Tensor indices_a, Tensor? ew_a, Tensor Ya, int reduce_a, "
        "Tensor? bias_nonempty_a, Tensor indptr_b, Tensor indices_b, Tensor? ew_b, Tensor Yb, "
        "int reduce_b, Tensor? bias_nonempty_b, Tensor H, Tensor W_self_aT, Tensor W_self_bT, "
        "Tensor? bias_a, Tensor? bias_b, int epilogue, int combine, Tensor? attn_vec, "
        "float out_div, Tensor(a!) out) -> ()");
  m.def("spmm_pair(Tensor indptr_a, Tensor indices_a, Tensor? ew_a, int reduce_a, "
        "Tensor? bias_a, Tensor? bias_nonempty_a, Tensor indptr_b, Tensor indices_b, "
        "Tensor? ew_b, int reduce_b, Tensor? bias_b, Tensor? bias_nonempty_b, Tensor X, "
        "Tensor H, Tensor WT4, int epilogue, int combine, Tensor? attn_vec, "
        "float out_div, "
        "Tensor(a!) out) -> ()");
  m.def("sddmm_cos(Tensor src, Tensor dst, Tensor Hs, Tensor Hd, Tensor(a!) out) -> ()");
  m.def("sddmm_cos_grouped(Tensor src_g, Tensor? first, int K, Tensor dst, Tensor Hs, Tensor Hd, "
        "Tensor(a!) out_first, Tensor(b!) out) -> ()");
  m.def("sddmm_cos_backward(Tensor src, Tensor dst, Tensor Hs, Tensor Hd, Tensor grad, "
        "Tensor(a!)? gHs, Tensor(b!)? gHd, Tensor(c!) workspace, int groups=0, int K=0) -> ()");
  m.def("edge_mlp(Tensor src, Tensor dst, Tensor P, Tensor Q, Tensor W2, Tensor b2, Tensor w3, "
        "Tensor b3, Tensor(a!) out) -> ()");
  m.def("edge_mlp_grouped(Tensor src_g, Tensor? first, int K, Tensor dst, Tensor P, Tensor Q, "
        "Tensor W2, Tensor b2, Tensor w3, Tensor b3, Tensor(a!) out_first, Tensor(b!) out) -> ()");
  m.def("edge_mlp_dense_store_f32(Tensor P, Tensor Q, Tensor W2, Tensor b2, Tensor w3, Tensor b3, "
        "Tensor(a!) out) -> ()");
  m.def("edge_mlp_dense_filter_f32(Tensor P, Tensor Q, Tensor W2, Tensor b2, Tensor w3, Tensor b3, "
        "Tensor tau, Tensor(a!) counts, Tensor(b!) cand_items, Tensor(c!) cand_scores) -> ()");
  m.def("topk_scored_candidates_f32(Tensor counts, Tensor cand_items, Tensor cand_scores, "
        "Tensor? user_rows, Tensor? exclude_indptr, Tensor? exclude_indices, int k, "
        "Tensor(a!) out_vals, Tensor(b!) out_idx) -> ()");
  m.def("topk_rows(Tensor scores, int k, Tensor? exclude_indptr, Tensor? exclude_indices, "
        "Tensor(a!) out_vals, Tensor(b!) out_idx) -> ()");
  m.def("normalize_rows_bf16(Tensor x, Tensor? row_map, Tensor(a!) out) -> ()");
  m.def("score_bf16_store(Tensor users, Tensor items, Tensor(a!) out) -> ()");
  m.def("score_bf16_filter(Tensor users, Tensor items, Tensor tau, Tensor(a!) counts, "
        "Tensor(b!) cand_items) -> ()");
  m.def("mask_excluded_f32(Tensor(a!) scores, Tensor? user_rows, Tensor exclude_indptr, "
        "Tensor exclude_indices) -> ()");
  m.def("topk_candidates_f32(Tensor counts, Tensor cand_items, Tensor? user_rows, Tensor h_user, "
        "Tensor h_item, Tensor? exclude_indptr, Tensor? exclude_indices, int k, "
        "Tensor(a!) out_vals, Tensor(b!) out_idx) -> ()");
  // one function under two names: topk_update, and the C entry's name like its neighbours
  m.def("topk_update(Tensor rows, Tensor(a!) idx, Tensor(b!) vals, Tensor item_mark, "
        "Tensor counts, Tensor cand_cols, Tensor dirty_ids, Tensor h_user, Tensor h_item, "
        "Tensor? exclude_indptr, Tensor? exclude_indices, Tensor(c!) redo) -> ()");
  m.def("topk_update_f32(Tensor rows, Tensor(a!) idx, Tensor(b!) vals, Tensor item_mark, "
        "Tensor counts, Tensor cand_cols, Tensor dirty_ids, Tensor h_user, Tensor h_item, "
        "Tensor? exclude_indptr, Tensor? exclude_indices, Tensor(c!) redo) -> ()");
  m.def("edge_mlp_dense_denominators_f32(Tensor P, Tensor Q, Tensor W2, Tensor b2, Tensor w3, "
        "Tensor b3, Tensor(a!) parts) -> ()");
  m.def("fold_partials_f32(Tensor parts, Tensor(a!) Z) -> ()");
  m.def("edge_mlp_dense_store_rating_f32(Tensor P, Tensor Q, Tensor W2, Tensor b2, Tensor w3, "
        "Tensor b3, Tensor Z, Tensor p_col, Tensor(a!) out) -> ()");
  m.def("edge_mlp_dense_filter_rating_f32(Tensor P, Tensor Q, Tensor W2, Tensor b2, Tensor w3, "
        "Tensor b3, Tensor Z, Tensor p_col, Tensor tau, Tensor(a!) counts, "
        "Tensor(b!) cand_items, Tensor(c!) cand_scores) -> ()");
  m.def("edge_mlp_dense_count_lists_f32(Tensor P, Tensor Q, Tensor W2, Tensor b2, Tensor w3, "
        "Tensor b3, Tensor lptr, Tensor thr, Tensor gid, Tensor(a!) parts, Tensor(b!) ahead) "
        "-> ()");
  m.def("edge_mlp_dense_count_lists_rating_f32(Tensor P, Tensor Q, Tensor W2, Tensor b2, "
        "Tensor w3, Tensor b3, Tensor Z, Tensor p_col, Tensor lptr, Tensor s, Tensor gid, "
        "Tensor(a!) parts, Tensor(b!) ahead) -> ()");
  m.def("rank_resolve_mlp_lists_f32(Tensor row_user, Tensor lptr, Tensor s, Tensor gid, "
        "Tensor ahead, int n_users, Tensor P, Tensor Q, Tensor W2, Tensor b2, Tensor w3, "
        "Tensor b3, Tensor? Z, Tensor? p_col, Tensor? exclude_indptr, Tensor? exclude_indices, "
        "Tensor(a!) rank, Tensor(b!) vals) -> ()");
  m.def("normalize_rows_f32(Tensor x, Tensor? row_map, Tensor(a!) out) -> ()");
  m.def("cos_denominators_f32(Tensor users, Tensor items, Tensor(a!) parts, Tensor(b!) Z) -> ()");
  m.def("cos_scores_f32(Tensor users, Tensor items, Tensor(a!) out) -> ()");
  m.def("rank_count_f32(Tensor users, Tensor items, Tensor thr, Tensor(a!) parts, "
        "Tensor(b!) ahead, Tensor(c!) band_counts, Tensor(d!) band_items) -> ()");
  m.def("rank_resolve_f32(Tensor users, Tensor items, Tensor thr, Tensor ahead, "
        "Tensor band_counts, Tensor band_items, Tensor h_user, Tensor h_item, "
        "Tensor? exclude_indptr, Tensor? exclude_indices, Tensor(a!) rank) -> ()");
  m.def("exp_rowsum_f32(Tensor scores, Tensor(a!) Z) -> ()");
  m.def("rating_rows_f32(Tensor(a!) scores, Tensor Z, Tensor p) -> ()");
  m.def("rating_thresholds_f32(Tensor tau, Tensor Z, Tensor pmax, Tensor(a!) thr) -> ()");
  m.def("mask_excluded_mapped_f32(Tensor(a!) scores, Tensor col_ids, Tensor? user_rows, "
        "Tensor exclude_indptr, Tensor exclude_indices) -> ()");
  m.def("score_bf16_store_rating(Tensor users, Tensor items, Tensor Z, Tensor p_col, "
        "Tensor(a!) out) -> ()");
  m.def("score_bf16_filter_rating(Tensor users, Tensor items, Tensor Z, Tensor p_col, "
        "Tensor thr, Tensor(a!) counts, Tensor(b!) cand_items) -> ()");
  m.def("topk_candidates_rating_f32(Tensor counts, Tensor cand_items, Tensor? user_rows, "
        "Tensor h_user, Tensor h_item, Tensor? exclude_indptr, Tensor? exclude_indices, "
        "Tensor Z, Tensor p, int k, Tensor(a!) out_vals, Tensor(b!) out_idx) -> ()");
  m.def("gemm_tn(Tensor A, Tensor B, Tensor(b!)? colsum, bool accumulate, Tensor(a!) out, "
        "Tensor(c!) workspace, Tensor? row_ptr=None) -> ()");
  m.def("act_backward(Tensor u, Tensor gz, int flags, Tensor(a!) out) -> ()");
  m.def("act_backward_normed(Tensor z, Tensor row_norm, Tensor gz, bool relu, "
        "Tensor(a!) out) -> ()");
  m.def("csr_transpose(Tensor indptr, Tensor indices, Tensor? edge_weight, int n_src, "
        "int n_edges, bool mean, Tensor(a!) workspace, Tensor(b!) indptr_t, "
        "Tensor(c!) indices_t, Tensor(d!)? ew_t) -> ()");
  m.def("csr_from_keys(Tensor keys, int n_rows, Tensor(a!) workspace, Tensor(b!) indptr, "
        "Tensor(c!) perm) -> ()");
  m.def("csr_build(Tensor src, Tensor dst, int n_dst, Tensor(a!) workspace, Tensor(b!) indptr, "
        "Tensor(c!) indices, Tensor(d!) eids) -> ()");
  m.def("csr_remove_edges(Tensor src, Tensor dst, Tensor indptr, Tensor indices, Tensor eids, "
        "Tensor rm, Tensor(a!) workspace, Tensor(b!) src_out, Tensor(c!) dst_out, "
        "Tensor(d!) kept_eids, Tensor(e!) indptr_out, Tensor(f!) indices_out, "
        "Tensor(g!) eids_out, Tensor(h!) status) -> ()");
  m.def("node_rank_table(Tensor nids, int n_nodes, Tensor(a!) workspace, Tensor(b!) removed, "
        "Tensor(c!) table, Tensor(d!) kept, Tensor(e!) status) -> ()");
  m.def("csr_remove_nodes(Tensor src, Tensor dst, Tensor indptr, Tensor indices, Tensor eids, "
        "Tensor? src_table, Tensor? dst_table, int n_src, int n_dst, int n_dst_new, "
        "Tensor(a!) workspace, Tensor(b!) src_out, Tensor(c!) dst_out, Tensor(d!) kept_eids, "
        "Tensor(e!) indptr_out, Tensor(f!) indices_out, Tensor(g!) eids_out, "
        "Tensor(h!) status) -> ()");
  m.def("csr_add_edges(Tensor indptr, Tensor indices, Tensor eids, Tensor src_new, "
        "Tensor dst_new, int n_src, int n_dst, Tensor(a!) workspace, Tensor(b!) indptr_out, "
        "Tensor(c!) indices_out, Tensor(d!) eids_out, Tensor(e!) status) -> ()");
  m.def("frontier_mark(Tensor rows, Tensor? n_rows, Tensor indptr, Tensor indices, "
        "Tensor(a!) mark, Tensor(b!) workspace, Tensor(c!) status) -> ()");
  m.def("add_(Tensor(a!) a, Tensor b) -> ()");
  m.def("tree_sum_(Tensor(a!) a, Tensor[] rest) -> ()");
  m.def("lstm_step(Tensor P, Tensor indptr, Tensor indices, Tensor order, int t, int n_act, "
        "Tensor h_in, Tensor(a!) h_out, Tensor(b!) c, Tensor W_hhT, Tensor(c!) out) -> ()");
  m.def("lstm_step_save(Tensor P, Tensor indptr, Tensor indices, Tensor order, int t, "
        "int n_act, Tensor h_in, Tensor(a!) h_out, Tensor? c_in, Tensor(b!) c_out, "
        "Tensor(c!) z_out, Tensor W_hhT, Tensor(d!) out) -> ()");
  m.def("lstm_backward_step(Tensor z, Tensor c_t, Tensor? c_prev, Tensor? dh_next, "
        "Tensor? dc_next, int n_next, Tensor g_out, Tensor order, int n_act, Tensor(a!) dz, "
        "Tensor(b!) dc_prev) -> ()");
  m.def("lstm_slots(Tensor indptr, Tensor indices, Tensor order, Tensor step_off, int n_slots, "
        "Tensor(a!) src, Tensor(b!) prev) -> ()");
  m.def("csr_has_edges(Tensor indptr, Tensor sorted_indices, int n_src, Tensor u, Tensor v, "
        "Tensor(a!) out) -> ()");
  m.def("sage_rel_forward(Tensor m, Tensor h_self, int n_self, Tensor W_self, Tensor W_neigh, "
        "Tensor indptr, Tensor indices, Tensor? edge_weight, int reduce, bool norm, "
        "Tensor? bias=None, Tensor? bias_nonempty=None, Tensor? live=None, float drop_p=0.0, "
        "Tensor? drop_keys=None, int drop_neigh=0, int drop_self=0) "
        "-> (Tensor, Tensor, Tensor)");
  m.def("sage_rel_backward(Tensor gz, Tensor z, Tensor row_norm, Tensor h_self, Tensor agg, "
        "Tensor W_self, Tensor W_neigh, Tensor indptr, Tensor indices, Tensor? edge_weight, "
        "int reduce, int n_src, int nnz, bool norm, int need, Tensor? indptr_t=None, "
        "Tensor? indices_t=None, Tensor? w_mean=None, Tensor(a!)? g_self_out=None, "
        "bool g_self_acc=False, Tensor(b!)? g_m_out=None, bool g_m_acc=False, "
        "Tensor? live_src=None, float drop_p=0.0, Tensor? drop_keys=None, int drop_neigh=0, "
        "int drop_self=0) -> (Tensor, Tensor, Tensor, Tensor, Tensor, Tensor)");
  m.def("dropout_keys(int seed, Tensor(a!) counter, int stream0, Tensor(b!) keys) -> ()");
  m.def("dropout_rows_f32(Tensor x, int n, Tensor keys, int key_index, float p, bool accumulate, "
        "Tensor(a!) out) -> ()");
  m.def("spmm_csr_dropout_live_f32(Tensor indptr, Tensor indices, Tensor? edge_weight, Tensor X, "
        "int reduce, int flags, Tensor(a!) out, Tensor? live, Tensor keys, int key_index, "
        "float p, int where) -> ()");
  m.def("spmm_csr_planned_dropout_live_f32(Tensor indptr, Tensor indices, Tensor? edge_weight, "
        "Tensor X, int reduce, int flags, int split, Tensor plan, int cap_h, int cap_c, "
        "Tensor(a!) out, Tensor(b!) workspace, Tensor? live, Tensor keys, int key_index, "
        "float p, int where) -> ()");
  m.def("block_transposes(Tensor[] indptrs, Tensor[] indices, int[] n_src, int[] nnz) "
        "-> (Tensor[], Tensor[], Tensor[])");
  m.def("margin_loss(Tensor pos, Tensor neg, int K, float delta, Tensor? mask, Tensor? recency, "
        "Tensor(a!) g_pos, Tensor(b!) g_neg, Tensor(c!) partial) -> ()");
  m.def("sum_scaled(Tensor x, float scale, Tensor(a!) out) -> ()");
  m.def("synth_edges(int seed, int e0, int n_u, int n_i, Tensor? zipf_cdf, Tensor(a!) u, "
        "Tensor(b!) i) -> ()");
  m.def("hold_cus(int blocks, int threads, int lds_bytes, int usec, Tensor(a!) sink) -> ()");
  // host-only entry points (no tensors: one catch-all kernel each)
  m.def("version() -> int", &version);
  m.def("dropout_mask_host(int seed, int step, int stream, int n_rows, int d, float p) -> Tensor",
        &dropout_mask_host);
  m.def("dropout_scale(float p) -> float", &dropout_scale);
  m.def("pack_rows_host(Tensor X) -> (Tensor, int)", &pack_rows_host);
  m.def("unpack_rows_host(Tensor packed, Tensor X_dense) -> Tensor", &unpack_rows_host);
  m.def("set_concurrency(int reserve_cus, bool dynamic) -> ()", &set_concurrency);
  m.def("get_concurrency() -> (int, int)", &get_concurrency);
  m.def("rowq_stats() -> (int, int)", &rowq_stats);
  m.def("spmm_plan_overflows() -> int", &spmm_plan_overflows);
  m.def("scan_workspace_bytes(int n) -> int", &scan_workspace_bytes);
  m.def("gemm_tn_workspace_bytes(int K, int M, int N) -> int", &gemm_tn_workspace_bytes);
  m.def("csr_transpose_workspace_bytes(int n_edges, int n_src) -> int",
        &csr_transpose_workspace_bytes);
  m.def("csr_from_keys_workspace_bytes(int n_edges, int n_rows) -> int",
        &csr_from_keys_workspace_bytes);
  m.def("csr_build_workspace_bytes(int n_edges, int n_dst) -> int", &csr_build_workspace_bytes);
  m.def("cos_denominator_parts(int n_items) -> int", &cos_denominator_parts);
  m.def("rank_eps(int d) -> float", &rank_eps);
  m.def("rank_list_slots() -> int", &rank_list_slots);
  m.def("csr_remove_edges_workspace_bytes(int n_edges, int n_dst) -> int",
        &csr_remove_edges_workspace_bytes);
  m.def("node_rank_table_workspace_bytes(int n_nodes) -> int", &node_rank_table_workspace_bytes);
  m.def("csr_remove_nodes_workspace_bytes(int n_edges, int n_dst) -> int",
        &csr_remove_nodes_workspace_bytes);
  m.def("csr_add_edges_workspace_bytes(int n_new, int n_dst) -> int",
        &csr_add_edges_workspace_bytes);
  m.def("frontier_mark_workspace_bytes(int n_rows) -> int", &frontier_mark_workspace_bytes);
  m.def("sddmm_cos_backward_workspace_bytes(int n_edges, int n_src, int n_dst, int d, "
        "int groups=0, int K=0) -> int", &sddmm_cos_backward_workspace_bytes);
  m.def("margin_loss_blocks(int n_pos) -> int", &margin_loss_blocks);
}

#define GNNREC_IMPLS(m)                                  \
  m.impl("spmm_csr", &spmm_csr);                         \
  m.impl("spmm_csr_split", &spmm_csr_split);             \
  m.impl("spmm_plan_build", &spmm_plan_build);           \
  m.impl("spmm_csr2", &spmm_csr2);                       \
  m.impl("spmm_csr_planned", &spmm_csr_planned);         \
  m.impl("spmm_backward", &spmm_backward);               \
  m.impl("gemm", &gemm);                                 \
  m.impl("row_epilogue", &row_epilogue);                 \
  m.impl("spmm_project", &spmm_project);                 \
  m.impl("spmm_project_agg_f32", &spmm_project_agg_f32); \
  m.impl("spmm_project2", &spmm_project2);               \
  m.impl("pack_rows_f32", &pack_rows_f32);               \
  m.impl("spmm_csr_packed_f32", &spmm_csr_packed_f32);   \
  m.impl("spmm_pair", &spmm_pair);                       \
  m.impl("sddmm_cos", &sddmm_cos);                       \
  m.impl("sddmm_cos_grouped", &sddmm_cos_grouped);       \
  m.impl("sddmm_cos_backward", &sddmm_cos_backward);     \
  m.impl("edge_mlp", &edge_mlp);                         \
  m.impl("edge_mlp_grouped", &edge_mlp_grouped);         \
  m.impl("edge_mlp_dense_store_f32", &edge_mlp_dense_store); \
  m.impl("edge_mlp_dense_filter_f32", &edge_mlp_dense_filter); \
  m.impl("topk_scored_candidates_f32", &topk_scored_candidates_f32); \
  m.impl("topk_rows", &topk_rows);                       \
  m.impl("normalize_rows_bf16", &normalize_rows_bf16);   \
  m.impl("score_bf16_store", &score_bf16_store);         \
  m.impl("score_bf16_filter", &score_bf16_filter);       \
  m.impl("mask_excluded_f32", &mask_excluded_f32);       \
  m.impl("topk_candidates_f32", &topk_candidates_f32);   \
  m.impl("topk_update", &topk_update);                   \
  m.impl("topk_update_f32", &topk_update);               \
  m.impl("edge_mlp_dense_denominators_f32", &edge_mlp_dense_denominators); \
  m.impl("fold_partials_f32", &fold_partials_f32);       \
  m.impl("edge_mlp_dense_store_rating_f32", &edge_mlp_dense_store_rating); \
  m.impl("edge_mlp_dense_filter_rating_f32", &edge_mlp_dense_filter_rating); \
  m.impl("edge_mlp_dense_count_lists_f32", &edge_mlp_dense_count_lists); \
  m.impl("edge_mlp_dense_count_lists_rating_f32", &edge_mlp_dense_count_lists_rating); \
  m.impl("rank_resolve_mlp_lists_f32", &rank_resolve_mlp_lists); \
  m.impl("normalize_rows_f32", &normalize_rows_f32);     \
  m.impl("cos_denominators_f32", &cos_denominators);         \
  m.impl("cos_scores_f32", &cos_scores);                     \
  m.impl("rank_count_f32", &rank_count);                     \
  m.impl("rank_resolve_f32", &rank_resolve);                 \
  m.impl("exp_rowsum_f32", &exp_rowsum);                     \
  m.impl("rating_rows_f32", &rating_rows_);                 \
  m.impl("rating_thresholds_f32", &rating_thresholds);       \
  m.impl("mask_excluded_mapped_f32", &mask_excluded_mapped_f32); \
  m.impl("score_bf16_store_rating", &score_bf16_store_rating); \
  m.impl("score_bf16_filter_rating", &score_bf16_filter_rating); \
  m.impl("topk_candidates_rating_f32", &topk_candidates_rating_f32); \
  m.impl("gemm_tn", &gemm_tn);                           \
  m.impl("act_backward", &act_backward);                 \
  m.impl("act_backward_normed", &act_backward_normed);   \
  m.impl("csr_transpose", &csr_transpose);               \
  m.impl("csr_from_keys", &csr_from_keys);               \
  m.impl("csr_build", &csr_build);                       \
  m.impl("csr_remove_edges", &csr_remove_edges);         \
  m.impl("node_rank_table", &node_rank_table);           \
  m.impl("csr_remove_nodes", &csr_remove_nodes);         \
  m.impl("csr_add_edges", &csr_add_edges);               \
  m.impl("frontier_mark", &frontier_mark);               \
  m.impl("add_", &add_);                                 \
  m.impl("tree_sum_", &tree_sum_);                       \
  m.impl("lstm_step", &lstm_step);                       \
  m.impl("lstm_step_save", &lstm_step_save);             \
  m.impl("lstm_backward_step", &lstm_backward_step);     \
  m.impl("lstm_slots", &lstm_slots);                     \
  m.impl("csr_has_edges", &csr_has_edges);               \
  m.impl("sage_rel_forward", &sage_rel_forward);         \
  m.impl("sage_rel_backward", &sage_rel_backward);       \
  m.impl("dropout_keys", &dropout_keys);                 \
  m.impl("dropout_rows_f32", &dropout_rows_f32);         \
  m.impl("spmm_csr_dropout_live_f32", &spmm_csr_dropout_live_f32); \
  m.impl("spmm_csr_planned_dropout_live_f32", &spmm_csr_planned_dropout_live_f32); \
  m.impl("block_transposes", &block_transposes);         \
  m.impl("margin_loss", &margin_loss);                   \
  m.impl("sum_scaled", &sum_scaled);                     \
  m.impl("synth_edges", &synth_edges);                   \
  m.impl("hold_cus", &hold_cus)

// HIP tensors dispatch under the CUDA key in ROCm PyTorch.
TORCH_LIBRARY_IMPL(gnnrec, CUDA, m) { GNNREC_IMPLS(m); }
// Meta / fake tensors (torch.compile tracing): the same functions stop after their checks.
TORCH_LIBRARY_IMPL(gnnrec, Meta, m) { GNNREC_IMPLS(m); }
// CPU tensors: the same functions refuse them in their first operand check (ValueError:
// "must be a HIP device tensor") — there is no CPU path, and the error says so.
TORCH_LIBRARY_IMPL(gnnrec, CPU, m) { GNNREC_IMPLS(m); }
