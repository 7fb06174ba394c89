// Device side of nnU-Net's fold ensemble (reference: `folds` of model.json go straight into the predictor, ts2d/core/inference/nnu.py:31-33,
// 146-165; upstream predict_logits_from_preprocessed_data: `prediction += predict_sliding_window_return_logits(...)` per fold, then
// `prediction /= n` when n > 1, all in the float16 of the aggregated logits).  sw_fold_mean is that statement over the F half buffers
// sw_aggregate left in the scratch, so the logits of a fold never travel to the host and numpy never adds halves there.
//
// Arithmetic per element, bit for bit numpy's float16 `+` and `/` (a half operation = the fp32 operation + round-to-nearest-even to
// half; predictor.fold_mean_f16 is the statement in numpy):
//     acc = x[0];  for f = 1 .. F-1: acc = half(float(acc) + float(x[f]));  acc = half(float(acc) / float(half(F)))
// in fold order, no atomics, through h_add / h_div of kernels_sw.h: one fp32 add or one correctly rounded fp32 division, then ONE
// conversion - nothing for the compiler to contract.  inf, the subnormals and the signed zeros follow IEEE (inf + -inf = NaN; a NaN
// stays a NaN, its payload is not pinned).
//
// Pure memory traffic, (F + 1) x 2 bytes per element: a lane owns 8 consecutive halves, reads 16 bytes per fold and stores 16 (and, with
// `seg`, the 8 bytes of the export predicate float(mean) > thr, which for F = 1 sw_aggregate writes itself); the n % 8 last elements
// take one lane each.  The buffers are slots of one allocation: fold f at x + f * stride, the mean goes to slot 0, which every lane
// reads before it writes and no other lane touches.
#pragma once
#include "kernels_sw.h"

namespace ts2d {

__device__ __forceinline__ __half fold_mean_one(__half acc, const __half* x, long long stride, int F, __half hF) {
    for (int f = 1; f < F; ++f) acc = h_add(acc, x[(size_t)f * stride]);
    return h_div(acc, hF);
}

// x: F slots of `stride` halves (stride a multiple of 8, x 16-byte aligned); n <= stride elements of every slot are averaged into slot 0
__global__ __launch_bounds__(256) void sw_fold_mean(__half* __restrict__ x, long long stride, int F, long long n, uint8_t* __restrict__ seg,
                                                    float thr) {
    const long long q = (long long)blockIdx.x * 256 + threadIdx.x, nv = n >> 3;
    const __half hF = __float2half_rn((float)F);
    if (q < nv) {
        const size_t o = (size_t)q * 8;
        union { uint4 v; __half h[8]; } acc, b;
        acc.v = *reinterpret_cast<const uint4*>(x + o);
        for (int f = 1; f < F; ++f) {
            b.v = *reinterpret_cast<const uint4*>(x + (size_t)f * stride + o);
            for (int j = 0; j < 8; ++j) acc.h[j] = h_add(acc.h[j], b.h[j]);
        }
        for (int j = 0; j < 8; ++j) acc.h[j] = h_div(acc.h[j], hF);
        *reinterpret_cast<uint4*>(x + o) = acc.v;
        if (seg) {
            uint2 w = make_uint2(0u, 0u);
            for (int j = 0; j < 4; ++j) {
                w.x |= (__half2float(acc.h[j]) > thr ? 1u : 0u) << (8 * j);
                w.y |= (__half2float(acc.h[j + 4]) > thr ? 1u : 0u) << (8 * j);
            }
            *reinterpret_cast<uint2*>(seg + o) = w;
        }
    } else if (q < nv + (n & 7)) {
        const size_t o = (size_t)(nv * 8 + (q - nv));
        const __half m = fold_mean_one(x[o], x + o, stride, F, hF);
        x[o] = m;
        if (seg) seg[o] = __half2float(m) > thr ? 1 : 0;
    }
}

}  // namespace ts2d
