// Device side of the export's PROBABILITIES (`save_probabilities=True` of the reference's predictor,
// ts2d/core/inference/predictor.py:99-111 -> export_prediction_from_logits, prediction_worker.py:215-221): nnU-Net resamples the aggregated
// logits back to the extent the case had before preprocessing (`resampling_fn_probabilities`, order 1, per plane for the 2-D
// configurations), applies the inference non-linearity in float32 - the sigmoid per head for a multilabel or region-based model, the
// softmax over the heads for a label-map model - and reverts the crop on the probabilities: outside the crop box they are 0, except head
// 0 of a label-map model, which is 1 [UPSTREAM-RECALL: LabelManager.apply_inference_nonlin, revert_cropping_on_probabilities].
// sw_probabilities does all of it where sw_aggregate / sw_fold_mean left the half logits [K, Hp, Wp] and writes the float32 planes
// [K, full_h, full_w] of the PRE-CROP extent, fill included, so that the host neither widens, interpolates, exponentiates nor inserts
// K float32 planes into a larger array.  The decision of the model's convention is taken in the same pass, on the LOGIT value with the
// predicate and comparator of the sibling kernels, so a case that asks for probabilities gets the segmentation bytes of one that does not.
//
// The value per head is the one the siblings decide on (export.probabilities_statement is the numpy statement):
//   resampled      sw_resample_threshold's value, bit for bit (kernels_resample.h): (((a00*wy0)*wx0 + (a01*wy0)*wx1) + (a10*wy1)*wx0) +
//                  (a11*wy1)*wx1, every product and sum rounded to float64 on its own (rs_mul / rs_add: no FMA), ONE rounding to float32.
//   identity       output extent == source rectangle (RsSeg::tap0 < 0): the widened half itself, no taps, no weights.
// The non-linearity, in float32:
//   sigmoid        1 / (1 + exp(-v)): a correctly rounded add and a correctly rounded division (hipcc's default for `/`; this unit is
//                  not built with fast-math).
//   softmax        exp(v - m) / sum_k exp(v_k - m), m the maximum over the heads, the sum taken in head order.  A +inf or NaN head
//                  makes every head of the pixel NaN (inf - inf), a -inf head gives 0: what torch.softmax does on the CPU.
//   exp            the float64 exp rounded once to float32 (pr_exp): within half a float32 unit (+ 2^-29 of one) of the true value, where
//                  the float32 routine is allowed a whole one.  What it costs has NOT been measured (the kernel is expected to be bound
//                  by its stores); it is what keeps `p > 0.5` equal to the logit predicate on ALL half inputs: exp(-2^-23) must round to 1 - 2^-23 for the add to
//                  land below 2.
// The K values of a pixel are RECOMPUTED per pass through L2 (softmax: maximum and argmax, then the sum, then the quotients): the half
// planes were written a moment ago and fit L2 / MALL, the float64 products are expected to ride under the stores (NOT measured: the softmax
// evaluates the 28-operation interpolation three times and the float64 exp twice per value), and nothing depends on K - no register
// array sized by it, no online rescaling whose extra roundings would enter the sum.
//
// Launch shape: the segment-table scheme of the siblings - ONE launch serves every image of a call, a block belongs to exactly one
// image - but a lane owns 4 consecutive X of one row of the FULL extent (so that its float4 store is 16-byte aligned whatever the box
// offset) and walks the K heads.  Per head a wave stores 1 KiB of consecutive floats where full_w is a multiple of 4; otherwise every lane
// issues four scalar stores per head, 16 bytes apart across lanes (the common case for real images; its cost is NOT measured either).
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <stdint.h>
#include "device_tables.h"      // RsSeg, RsTap, ProbSeg, ProbMode
#include "rs_arith.h"           // rs_mul, rs_add
#include "kernels_resample.h"   // rs_find_seg, rs_widen
#include "labelmap_cmp.h"       // lm_replaces

namespace ts2d {

__device__ __forceinline__ float pr_exp(float x) { return __double2float_rn(exp((double)x)); }

__device__ __forceinline__ float pr_sigmoid(float v) {
#pragma clang fp contract(off)
    return 1.0f / (1.0f + pr_exp(-v));
}

// what a lane knows of its four pixels for the walk over the heads
struct PrQuad {
    RsTap ty, tx[4];
    int o00[4], o01[4], o10[4], o11[4];     // resampling: the four samples; identity: o00 alone
    bool ident;
};

__device__ __forceinline__ float pr_value(const __half* __restrict__ p, const PrQuad& q, int j) {
    if (q.ident) return __half2float(p[q.o00[j]]);
    double s = rs_mul(rs_mul(rs_widen(p + q.o00[j]), q.ty.w0), q.tx[j].w0);
    s = rs_add(s, rs_mul(rs_mul(rs_widen(p + q.o01[j]), q.ty.w0), q.tx[j].w1));
    s = rs_add(s, rs_mul(rs_mul(rs_widen(p + q.o10[j]), q.ty.w1), q.tx[j].w0));
    s = rs_add(s, rs_mul(rs_mul(rs_widen(p + q.o11[j]), q.ty.w1), q.tx[j].w1));
    return __double2float_rn(s);
}

__device__ __forceinline__ void pr_store4(float* __restrict__ o, const float v[4], int nx, bool vec) {
    if (vec) {
        *reinterpret_cast<float4*>(o) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
        for (int j = 0; j < 4; ++j)
            if (j < nx) o[j] = v[j];
    }
}

__device__ __forceinline__ void pr_store4(uint8_t* __restrict__ o, const unsigned v[4], int nx, bool vec) {
    if (vec) {
        *reinterpret_cast<unsigned*>(o) = v[0] | (v[1] << 8) | (v[2] << 16) | (v[3] << 24);
    } else {
        for (int j = 0; j < 4; ++j)
            if (j < nx) o[j] = (uint8_t)v[j];
    }
}

// elements between the heads of an image's outputs: the dense block of ProbSeg, the run's stride of ProbStackSeg
__device__ __forceinline__ size_t pr_prob_stride(const ProbSeg& ps) { return (size_t)ps.full_h * ps.full_w; }
__device__ __forceinline__ size_t pr_dec_stride(const ProbSeg& ps) { return (size_t)ps.full_h * ps.full_w; }
__device__ __forceinline__ size_t pr_prob_stride(const ProbStackSeg& ps) { return (size_t)ps.prob_stride; }
__device__ __forceinline__ size_t pr_dec_stride(const ProbStackSeg& ps) { return (size_t)ps.dec_stride; }

// one lane per 4 consecutive X of one row Y of one image's FULL extent; mode: ProbMode; order: K class values (kProbRegions only);
// Seg = ProbSeg: prob [K, full_h, full_w] per image at ProbSeg::prob_off; dec (or null): the decided map at ProbSeg::dec_off
// Seg = ProbStackSeg (ts2d_ensemble_predict_tiled_probabilities_stack): the image is a slice of a run whose outputs are [K][n_slices][full_h][full_w] -
// head k at prob_off + k * prob_stride (dec likewise): the ONE difference between the two instantiations; all offsets are 64-bit
template <class Seg>
__global__ __launch_bounds__(256) void sw_probabilities(const __half* __restrict__ src16, const RsSeg* __restrict__ segs,
                                                        const Seg* __restrict__ psegs, int n_segs, int K, const RsTap* __restrict__ taps,
                                                        int mode, const uint8_t* __restrict__ order, float* __restrict__ prob,
                                                        uint8_t* __restrict__ dec, float thr) {
    const int si = rs_find_seg(segs, n_segs, blockIdx.x);
    const RsSeg sg = segs[si];
    const Seg ps = psegs[si];
    const int Wq = (ps.full_w + 3) >> 2;
    const long long l = (long long)(blockIdx.x - sg.block0) * 256 + threadIdx.x;
    if (l >= (long long)ps.full_h * Wq) return;
    const int X0 = (int)(l % Wq) * 4, Y = (int)(l / Wq);
    const int nx = ps.full_w - X0 < 4 ? ps.full_w - X0 : 4;     // (the last quad of a row whose extent is no multiple of 4)
    const bool softmax = mode == kProbLabelmap;
    const bool vec = (ps.full_w & 3) == 0;                      // (block-uniform) every quad is whole and 16 / 4 bytes aligned: the offsets are multiples of 4
    const size_t pstride = pr_prob_stride(ps), dstride = pr_dec_stride(ps);
    const size_t at = (size_t)Y * ps.full_w + X0;
    float* po = prob + ps.prob_off + at;
    uint8_t* dk = dec ? dec + ps.dec_off + at : nullptr;
    const int y = Y - ps.box_y;
    bool in[4];
    bool any = false;
    for (int j = 0; j < 4; ++j) {
        const int x = X0 + j - ps.box_x;
        in[j] = j < nx && y >= 0 && y < sg.out_h && x >= 0 && x < sg.out_w;
        any |= in[j];
    }
    if (!any) {                                                 // the fill alone: a row above or below the box, a quad beside it
        const float zero[4] = {0.f, 0.f, 0.f, 0.f}, one[4] = {1.f, 1.f, 1.f, 1.f};
        const unsigned none[4] = {0u, 0u, 0u, 0u};
        for (int k = 0; k < K; ++k) {
            pr_store4(po + k * pstride, softmax && k == 0 ? one : zero, nx, vec);
            if (dk && (mode == kProbMultilabel || k == 0)) pr_store4(dk + k * dstride, none, nx, vec);
        }
        return;
    }
    // a pixel outside the box computes the nearest one inside it (every read stays in bounds) and stores the fill
    PrQuad q;
    q.ident = sg.tap0 < 0;                                      // (block-uniform)
    if (!q.ident) q.ty = taps[sg.tap0 + y];
    for (int j = 0; j < 4; ++j) {
        int x = X0 + j - ps.box_x;
        x = x < 0 ? 0 : x >= sg.out_w ? sg.out_w - 1 : x;
        if (q.ident) {                                          // src_off is the rectangle's first sample
            q.o00[j] = y * sg.Wp + x; q.o01[j] = q.o10[j] = q.o11[j] = 0;
        } else {
            q.tx[j] = taps[sg.tap0 + sg.out_h + x];
            q.o00[j] = q.ty.i0 * sg.Wp + q.tx[j].i0; q.o01[j] = q.ty.i0 * sg.Wp + q.tx[j].i1;
            q.o10[j] = q.ty.i1 * sg.Wp + q.tx[j].i0; q.o11[j] = q.ty.i1 * sg.Wp + q.tx[j].i1;
        }
    }
    const size_t plane = (size_t)sg.Hp * sg.Wp;
    const __half* p0 = src16 + sg.src_off;
    if (!softmax) {                                             // (block-uniform) sigmoid per head; the decision on the logit
        int head[4] = {0, 0, 0, 0};                             // regions: index + 1 of the last head above the threshold
        const __half* p = p0;
        for (int k = 0; k < K; ++k, p += plane) {
            float pr[4];
            unsigned ab[4];
            for (int j = 0; j < 4; ++j) {
                const float v = pr_value(p, q, j);
                const bool above = in[j] && v > thr;
                pr[j] = in[j] ? pr_sigmoid(v) : 0.f;
                ab[j] = above ? 1u : 0u;
                if (above) head[j] = k + 1;
            }
            pr_store4(po + k * pstride, pr, nx, vec);
            if (dk && mode == kProbMultilabel) pr_store4(dk + k * dstride, ab, nx, vec);
        }
        if (dk && mode == kProbRegions) {
            unsigned lab[4];
            for (int j = 0; j < 4; ++j) lab[j] = head[j] ? (unsigned)order[head[j] - 1] : 0u;      // (head <= K: inside the table)
            pr_store4(dk, lab, nx, vec);
        }
        return;
    }
    float best[4] = {0.f, 0.f, 0.f, 0.f}, sum[4] = {0.f, 0.f, 0.f, 0.f};
    unsigned idx[4] = {0u, 0u, 0u, 0u};
    const __half* p = p0;
    for (int k = 0; k < K; ++k, p += plane)                     // numpy's argmax (labelmap_cmp.h): its value is the maximum, or the first NaN
        for (int j = 0; j < 4; ++j) {
            const float v = pr_value(p, q, j);
            if (k == 0 || lm_replaces(v, best[j])) { best[j] = v; idx[j] = (unsigned)k; }
        }
    p = p0;
    for (int k = 0; k < K; ++k, p += plane)
        for (int j = 0; j < 4; ++j) {
#pragma clang fp contract(off)
            sum[j] = sum[j] + pr_exp(pr_value(p, q, j) - best[j]);
        }
    p = p0;
    for (int k = 0; k < K; ++k, p += plane) {
        float pr[4];
        for (int j = 0; j < 4; ++j) {
#pragma clang fp contract(off)
            const float e = pr_exp(pr_value(p, q, j) - best[j]) / sum[j];
            pr[j] = in[j] ? e : k == 0 ? 1.f : 0.f;
        }
        pr_store4(po + k * pstride, pr, nx, vec);
    }
    if (dk) {
        for (int j = 0; j < 4; ++j)
            if (!in[j]) idx[j] = 0u;
        pr_store4(dk, idx, nx, vec);
    }
}

}  // namespace ts2d
