// Host-side choice of a launcher's template instantiation from the run-time dtype code / head dim, used with generic lambdas.  A code outside the table is an
// error that names the launcher, never a silent fp32 (or fp16) run.  Secondary selectors (np, op, CPT, NX, ...) stay plain chains inside the lambda.
#pragma once
#include "common.h"
#include <type_traits>

namespace lmx {

template <typename T> struct TypeTag { using type = T; };
#define LMX_T(tag) typename decltype(tag)::type      // the element type behind a lambda's `auto t`

template <typename F> inline void dispatch_dtype(int dtype, const char* who, F&& f) {
    if (dtype == kBF16) f(TypeTag<bf16_t>{});
    else if (dtype == kF16) f(TypeTag<f16_t>{});
    else if (dtype == kF32) f(TypeTag<float>{});
    else throw Error{std::string(who) + ": bad dtype " + std::to_string(dtype)};
}
// the launchers whose kernels exist for the two 16-bit types only (MFMA / packed-pair paths)
template <typename F> inline void dispatch_dtype16(int dtype, const char* who, F&& f) {
    if (dtype == kBF16) f(TypeTag<bf16_t>{});
    else if (dtype == kF16) f(TypeTag<f16_t>{});
    else throw Error{std::string(who) + ": 16-bit dtypes only (got " + std::to_string(dtype) + ")"};
}
template <typename F> inline void dispatch_head_dim(int D, const char* who, F&& f) {
    if (D == 128) f(std::integral_constant<int, 128>{});
    else if (D == 64) f(std::integral_constant<int, 64>{});
    else throw Error{std::string(who) + ": head_dim must be 64 or 128 (got " + std::to_string(D) + ")"};
}

}  // namespace lmx
