// The float64 product and sum of both device resamples (kernels_resample.h in the sliding-window unit, kernels_resample_in.h in the
// input-side unit): its own header so that neither unit has to include the other's kernels.
#pragma once
#include <hip/hip_runtime.h>

namespace ts2d {

// a float64 product / sum that is rounded on its own: never half of a fused multiply-add
__device__ __forceinline__ double rs_mul(double a, double b) {
#pragma clang fp contract(off)
    return a * b;
}
__device__ __forceinline__ double rs_add(double a, double b) {
#pragma clang fp contract(off)
    return a + b;
}

}  // namespace ts2d
