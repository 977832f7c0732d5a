// ptv_grad.hpp — np.gradient's elementwise division rule, shared by the stencil passes that restate
// it (ptv_flow.hip, ptv_drag.hip).
//
// np.gradient with scalar spacings takes the difference in the field dtype T and divides it by the
// spacing.  For float32 fields numpy has two rules: a Python-float spacing is weak, the divisor
// becomes (float)(2. * h) and the division is float32; a np.float64 spacing is strong, the
// difference is widened, divided in float64 and the quotient rounded to float32 when np.gradient
// stores it.
#pragma once

#include <hip/hip_runtime.h>

#include <type_traits>

namespace ptv {

// the divisor's type: float64 for float64 fields and for the strong rule, else float32
template <typename T, bool STRONG>
using Div = std::conditional_t<std::is_same<T, double>::value || STRONG, double, float>;

// (difference in T) / divisor under numpy's rule, rounded to T
template <typename T, bool STRONG>
__device__ __forceinline__ T quot(T d, Div<T, STRONG> h) {
    return (T)((Div<T, STRONG>)d / h);
}

}  // namespace ptv
