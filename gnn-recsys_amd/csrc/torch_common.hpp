// torch_common.hpp — what every TORCH_LIBRARY(gnnrec) translation unit shares: the status
// check, the stream lookup, the one-device rule and the operand checks.
#pragma once
#include <ATen/ATen.h>
#include <c10/core/DeviceGuard.h>
#include <c10/hip/HIPStream.h>
#include <torch/library.h>

#include <algorithm>

#include "gnnrec.h"

namespace gnnrec_torch {

using at::Tensor;
using c10::optional;

inline void ck(int rc, const char* what) {
  if (rc == GNNREC_OK) return;
  const char* msg = gnnrec_last_error();
  TORCH_CHECK_VALUE(rc != GNNREC_EINVAL, what, ": ", msg);
  TORCH_CHECK(false, what, ": ", msg, " (status ", rc, ")");
}

inline void* stream_of(const Tensor& t) {
  return c10::hip::getCurrentHIPStream(t.device().index()).stream();
}

// Every device operand of one op must sit on ONE device: the guard and the stream come from
// one of them, and a pointer into another GPU's memory would fault in the kernel instead of
// raising.  Each op opens a OneDevice scope; dev()/same_dev() compare every operand with
// the first one seen in it.
inline thread_local bool g_op_dev_set = false;
inline thread_local c10::Device g_op_device{c10::DeviceType::CPU};
struct OneDevice {
  OneDevice() { g_op_dev_set = false; }
  ~OneDevice() { g_op_dev_set = false; }
};
inline void same_dev(const Tensor& t, const char* name) {
  if (!t.defined() || !t.is_cuda()) return;
  if (!g_op_dev_set) {
    g_op_device = t.device();
    g_op_dev_set = true;
    return;
  }
  TORCH_CHECK_VALUE(t.device() == g_op_device, name, " is on ", t.device(),
                    " but the op's other operands are on ", g_op_device);
}

// device operand (or meta/fake during tracing) of the given dtype
inline void dev(const Tensor& t, const char* name, c10::ScalarType dt) {
  TORCH_CHECK_VALUE(t.is_cuda() || t.is_meta(), name,
                    " must be a HIP device tensor (gnnrec has no CPU path), got ", t.device());
  TORCH_CHECK_VALUE(t.scalar_type() == dt, name, " must be ", dt, ", got ", t.scalar_type());
  same_dev(t, name);
}
inline void dev(const optional<Tensor>& t, const char* name, c10::ScalarType dt) {
  if (t.has_value() && t->defined()) dev(*t, name, dt);
}

inline bool has(const optional<Tensor>& t) { return t.has_value() && t->defined(); }

template <typename T>
T* p(const Tensor& t) { return reinterpret_cast<T*>(t.data_ptr()); }
template <typename T>
T* p(const optional<Tensor>& t) { return has(t) ? reinterpret_cast<T*>(t->data_ptr()) : nullptr; }

// leading dimension of a 2-D row-major operand (unit column stride)
inline int64_t ld(const Tensor& t, const char* name) {
  TORCH_CHECK_VALUE(t.dim() == 2, name, " must be 2-D, got ", t.sizes());
  TORCH_CHECK_VALUE(t.stride(1) == 1 || t.size(1) <= 1, name, " must have unit column stride");
  return std::max<int64_t>({t.stride(0), t.size(1), 1});
}

inline bool meta(const Tensor& t) { return t.is_meta(); }

}  // namespace gnnrec_torch
