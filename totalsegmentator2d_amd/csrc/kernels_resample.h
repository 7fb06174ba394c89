// Device side of the export's resample-back: nnU-Net resamples the aggregated logits to the extent the case had
// before preprocessing (`resampling_fn_probabilities`, order 1, per plane for the 2-D configurations) and thresholds them afterwards.
// sw_resample_threshold does both where sw_aggregate left the half logits, so that K uint8 planes of the ORIGINAL extent travel to
// the host and the host neither widens nor interpolates.
//
// Arithmetic = preprocess.resize_linear_f64, bit for bit, which is bit for bit scipy's zoom(order=1, mode='nearest', grid_mode=True) -
// what skimage's resize(order=1, mode='edge') calls and the host route of the export computes (tests/test_resample_cpu.py): per output pixel
//     value = ((((a00*wy0)*wx0 + (a01*wy0)*wx1) + (a10*wy1)*wx0) + (a11*wy1)*wx1      every product and sum rounded to float64, no FMA
// then ONE rounding to float32 and the export predicate float32(value) > 1.5 * 2^-24.  The per-axis taps (two source indices, two
// weights per output row / column) are computed in float64 on the host (tiled_plan.cpp: rs_axis_taps) and uploaded, so the kernel holds
// no division and no floor whose device rounding would have to be argued about: it widens four halves, multiplies and adds.
// Every product and sum is written under `#pragma clang fp contract(off)` (rs_mul / rs_add): hipcc contracts by default, and HIP's
// __dmul_rn / __dadd_rn are plain operators that it fuses into v_fmac_f64 just the same; tests/test_resample_cpu.py asserts that the
// emitted stream holds v_mul_f64 / v_add_f64 and no fused form.  A zero weight on an infinite logit gives NaN, as it does in scipy;
// NaN is not above the threshold.
//
// Like sw_gather / sw_aggregate it is pure memory traffic under the segment-table scheme: ONE launch serves every image of a call, a
// block belongs to exactly one image, a lane owns 4 consecutive output X of one (k, Y) row and stores 4 bytes.  The source planes
// (a few MB at most) are read through L2.
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <stdint.h>
#include "device_tables.h"      // RsSeg, RsTap
#include "rs_arith.h"           // rs_mul, rs_add

namespace ts2d {

__device__ __forceinline__ int rs_find_seg(const RsSeg* __restrict__ segs, int n, unsigned blk) {
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (segs[mid].block0 <= blk) lo = mid; else hi = mid - 1;
    }
    return lo;
}

__device__ __forceinline__ double rs_widen(const __half* p) { return (double)__half2float(*p); }

// one lane per 4 consecutive X of one (k, Y) row of one image's output extent; seg / out32: either may be null
__global__ __launch_bounds__(256) void sw_resample_threshold(const __half* __restrict__ src16, const RsSeg* __restrict__ segs, int n_segs,
                                                             int K, const RsTap* __restrict__ taps, uint8_t* __restrict__ seg,
                                                             float* __restrict__ out32, float thr) {
    const RsSeg sg = segs[rs_find_seg(segs, n_segs, blockIdx.x)];
    const int Wq = (sg.out_w + 3) >> 2;
    const long long q = (long long)(blockIdx.x - sg.block0) * 256 + threadIdx.x;
    if (q >= (long long)K * sg.out_h * Wq) return;
    const int X0 = (int)(q % Wq) * 4; const long long r = q / Wq;
    const int Y = (int)(r % sg.out_h), k = (int)(r / sg.out_h);
    const RsTap ty = taps[sg.tap0 + Y];
    const __half* row0 = src16 + sg.src_off + ((size_t)k * sg.Hp + ty.i0) * sg.Wp;
    const __half* row1 = src16 + sg.src_off + ((size_t)k * sg.Hp + ty.i1) * sg.Wp;
    const int nx = sg.out_w - X0 < 4 ? sg.out_w - X0 : 4;      // (the last quad of a row whose extent is no multiple of 4)
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    for (int j = 0; j < 4; ++j) {                               // (constant trip count: v[] stays in registers)
        if (j >= nx) continue;
        const RsTap tx = taps[sg.tap0 + sg.out_h + X0 + j];
        double s = rs_mul(rs_mul(rs_widen(row0 + tx.i0), ty.w0), tx.w0);
        s = rs_add(s, rs_mul(rs_mul(rs_widen(row0 + tx.i1), ty.w0), tx.w1));
        s = rs_add(s, rs_mul(rs_mul(rs_widen(row1 + tx.i0), ty.w1), tx.w0));
        s = rs_add(s, rs_mul(rs_mul(rs_widen(row1 + tx.i1), ty.w1), tx.w1));
        v[j] = __double2float_rn(s);
    }
    const size_t o = (size_t)sg.dst_off + ((size_t)k * sg.out_h + Y) * sg.out_w + X0;
    if ((sg.out_w & 3) == 0) {
        if (seg) {
            unsigned w = 0;
            for (int j = 0; j < 4; ++j) w |= (v[j] > thr ? 1u : 0u) << (8 * j);
            *reinterpret_cast<unsigned*>(seg + o) = w;
        }
        if (out32) *reinterpret_cast<float4*>(out32 + o) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
        for (int j = 0; j < 4; ++j) {
            if (j >= nx) continue;
            if (seg) seg[o + j] = v[j] > thr ? 1 : 0;
            if (out32) out32[o + j] = v[j];
        }
    }
}

}  // namespace ts2d
