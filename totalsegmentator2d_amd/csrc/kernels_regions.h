// Device side of the export of a REGION-BASED model (nnU-Net's third label convention: the label values of
// dataset.json are lists, one head per foreground region, `regions_class_order` names the class each region paints): nnU-Net resamples
// the aggregated logits back to the extent the case had before preprocessing (`resampling_fn_probabilities`, order 1, per plane for the
// 2-D configurations), applies the sigmoid in float32 and paints [UPSTREAM-RECALL: LabelManager.convert_probabilities_to_segmentation]
//     seg = 0;  for i, c in enumerate(regions_class_order): seg[prob[i] > 0.5] = c
// so the HIGHEST head index above one half decides a pixel, whatever its class value (values may repeat, and may be 0).  sw_regions does
// all three where sw_aggregate / sw_fold_mean left the half logits [K, Hp, Wp], so that ONE uint8 plane of the ORIGINAL extent travels
// to the host instead of K float16 planes of the network's extent that the host widens, interpolates, thresholds and paints.
//
// The value per head is the one the host route thresholds (export.regions_statement is the numpy statement):
//   resampled      sw_resample_threshold's value, bit for bit (kernels_resample.h): (((a00*wy0)*wx0 + (a01*wy0)*wx1) + (a10*wy1)*wx0) +
//                  (a11*wy1)*wx1, every product and sum rounded to float64 on its own (rs_mul / rs_add: no FMA), ONE rounding to float32;
//                  the taps come from the host (tiled_plan.cpp: rs_axis_taps).  A zero weight on an infinite logit gives NaN, as in scipy.
//   identity       output extent == source rectangle (RsSeg::tap0 < 0): the host route does not resample, so the widened half itself - no
//                  taps, no weights: an infinite logit stays infinite.
// The predicate is the export's: sigmoid(float32 v) > 0.5  <=>  v > 1.5 * 2^-24 (`thr`; tests/test_oracle.py) - NaN is not above it
// and is not painted, +inf is.
//
// The lane keeps the running HEAD (index + 1; 0: none yet) of its four pixels, not the running class: "the last head above the threshold"
// is what the painting loop computes, and the class-order table (K bytes behind the taps in the call's one table blob) is then read once
// per pixel behind the walk instead of once per head inside it.
//
// What bounds it: memory traffic, like its sibling sw_labelmap, whose bytes it moves exactly - K half planes of the network's extent
// in through L2 (a few MB: they were written by the aggregation a moment ago and fit the 4 MB L2 / 256 MB MALL), ONE byte per output
// pixel out.  No LDS, no barrier; the float64 products of the resampling branch (16 v_mul_f64 + 12 v_add_f64 per head and lane) ride
// under the loads at these sizes.  ONE launch serves every image of a call, a block belongs to exactly one image, a lane owns 4
// consecutive output X of one output row, reads its row tap and its four column taps ONCE and stores 4 bytes.
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <stdint.h>
#include "device_tables.h"      // RsSeg, RsTap
#include "rs_arith.h"           // rs_mul, rs_add
#include "kernels_resample.h"   // rs_find_seg, rs_widen

namespace ts2d {

// one lane per 4 consecutive X of one output row Y of one image; order: K class values; out8: [out_h, out_w] per image at RsSeg::dst_off
__global__ __launch_bounds__(256) void sw_regions(const __half* __restrict__ src16, const RsSeg* __restrict__ segs, int n_segs, int K,
                                                  const RsTap* __restrict__ taps, const uint8_t* __restrict__ order,
                                                  uint8_t* __restrict__ out8, float thr) {
    const RsSeg sg = segs[rs_find_seg(segs, n_segs, blockIdx.x)];
    const int Wq = (sg.out_w + 3) >> 2;
    const long long q = (long long)(blockIdx.x - sg.block0) * 256 + threadIdx.x;
    if (q >= (long long)sg.out_h * Wq) return;
    const int X0 = (int)(q % Wq) * 4, Y = (int)(q / Wq);
    const int nx = sg.out_w - X0 < 4 ? sg.out_w - X0 : 4;      // (the last quad of a row whose extent is no multiple of 4)
    const size_t plane = (size_t)sg.Hp * sg.Wp;
    int head[4] = {0, 0, 0, 0};                                 // index + 1 of the last head above the threshold
    if (sg.tap0 < 0) {                                          // (block-uniform) identity: src_off is the rectangle's first sample
        const __half* p = src16 + sg.src_off + (size_t)Y * sg.Wp + X0;
        const bool vec = ((sg.src_off | sg.Wp) & 3) == 0;       // 8-byte aligned quads that stay inside the row of the padded plane
        for (int k = 0; k < K; ++k, p += plane) {
            float v[4] = {0.f, 0.f, 0.f, 0.f};
            if (vec) {
                const uint2 w = *reinterpret_cast<const uint2*>(p);
                v[0] = __half2float(__ushort_as_half((unsigned short)(w.x & 0xFFFFu))); v[1] = __half2float(__ushort_as_half((unsigned short)(w.x >> 16)));
                v[2] = __half2float(__ushort_as_half((unsigned short)(w.y & 0xFFFFu))); v[3] = __half2float(__ushort_as_half((unsigned short)(w.y >> 16)));
            } else {
                for (int j = 0; j < 4; ++j)
                    if (j < nx) v[j] = __half2float(p[j]);
            }
            for (int j = 0; j < 4; ++j)
                if (v[j] > thr) head[j] = k + 1;
        }
    } else {
        const RsTap ty = taps[sg.tap0 + Y];
        RsTap tx[4];
        int o00[4], o01[4], o10[4], o11[4];
        for (int j = 0; j < 4; ++j) {                           // (a lane past the row's end repeats the last column: every read stays in bounds)
            tx[j] = taps[sg.tap0 + sg.out_h + (j < nx ? X0 + j : sg.out_w - 1)];
            o00[j] = ty.i0 * sg.Wp + tx[j].i0; o01[j] = ty.i0 * sg.Wp + tx[j].i1;
            o10[j] = ty.i1 * sg.Wp + tx[j].i0; o11[j] = ty.i1 * sg.Wp + tx[j].i1;
        }
        const __half* p = src16 + sg.src_off;
        for (int k = 0; k < K; ++k, p += plane) {
            for (int j = 0; j < 4; ++j) {                       // (constant trip count: head[] stays in registers)
                double s = rs_mul(rs_mul(rs_widen(p + o00[j]), ty.w0), tx[j].w0);
                s = rs_add(s, rs_mul(rs_mul(rs_widen(p + o01[j]), ty.w0), tx[j].w1));
                s = rs_add(s, rs_mul(rs_mul(rs_widen(p + o10[j]), ty.w1), tx[j].w0));
                s = rs_add(s, rs_mul(rs_mul(rs_widen(p + o11[j]), ty.w1), tx[j].w1));
                if (__double2float_rn(s) > thr) head[j] = k + 1;
            }
        }
    }
    unsigned lab[4];
    for (int j = 0; j < 4; ++j) lab[j] = head[j] ? (unsigned)order[head[j] - 1] : 0u;      // (head <= K: inside the table)
    uint8_t* o = out8 + sg.dst_off + (size_t)Y * sg.out_w + X0;
    if ((sg.out_w & 3) == 0) {
        *reinterpret_cast<unsigned*>(o) = lab[0] | (lab[1] << 8) | (lab[2] << 16) | (lab[3] << 24);
    } else {
        for (int j = 0; j < 4; ++j)
            if (j < nx) o[j] = (uint8_t)lab[j];
    }
}

}  // namespace ts2d
