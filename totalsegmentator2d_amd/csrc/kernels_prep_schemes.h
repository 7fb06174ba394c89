// The other normalisation schemes of nnU-Net on the device-resident planes of kernels_prep.h (reference flow DefaultPreprocessor.run_case,
// ts2d/core/inference/prediction_worker.py:194-199; the schemes are nnunetv2's default_normalization_schemes): CTNormalization,
// RescaleTo01Normalization, RGBTo01Normalization, NoNormalization and ZScoreNormalization inside the non-zero mask, beside the plain z-score.
// Four kernels behind ts2d_planes_crop_normalize (prep.hip):
//     prep_mask_counts      the mask "non-zero in ANY plane" of the cropped planes as bytes, and how many pixels of it each block of 2048 holds
//     prep_mask_scan        the exclusive scan of those block counts (one workgroup), and their total n_m
//     prep_mask_scatter     plane[mask] of every plane, in index order, into a dense [planes][n_m] buffer: numpy's `img[m]`
//     prep_apply_schemes<A> A = true: every plane normalised in place by its row of the scheme table, its float32 minimum and maximum left
//                           as integer keys (what prep_normalise leaves); A = false: the keys of the planes as they are, nothing written
//
// Arithmetic = the statements of preprocess.py (ct_f32_statement, rescale01_f32_statement, rgb01_f32_statement,
// masked_zscore_f32_statement), bit for bit, which are bit for bit preprocess.normalize_channel (tests/test_prep_schemes_cpu.py).  The sums
// behind the masked z-score are prep_chunk_sums<0 / 1> of kernels_prep.h over the dense buffer, unchanged: numpy reduces `img[m]`, a compact
// 1-D copy in row-major order, so the chunks and leaves are those of a run of n_m elements.  The compaction keeps that order with integers
// only: a pixel's place is (masked pixels in the blocks before its block, from the scan) + (masked pixels before it in its block, from wave
// ballots and a scan of the block's 32 wave counts).  A block's 2048 pixels are 8 rows of 256 lanes, so every load and store of the mask
// kernels is coalesced.  No float atomics; the result does not depend on the launch shape; two runs give the same bytes.
//
// Every subtraction and division of prep_apply_schemes is a plain operator under `#pragma clang fp contract(off)`, the division the correctly
// rounded float32 `/`.  numpy's clip is spelled out with comparisons (x < lo ? lo : x, then x > hi ? hi : x): a sample equal to a bound keeps
// its own sign of zero and a NaN sample stays NaN, neither of which v_max_f32 / v_min_f32 would do.
//
// Pure HBM streaming, no MFMA; LDS holds 33 integers per workgroup of the mask kernels, 1024 in the scan.
#pragma once
#include "kernels_prep.h"

namespace ts2d {

constexpr int kPrepMaskRows = kPrepMaskBlock / 256;     // rows of 256 lanes in a block of the mask kernels
static_assert(kPrepMaskRows == 8 && kPrepMaskRows * 4 == 32, "prep_mask_scatter scans the block's wave counts in one half wave");

// mask [n] <- 1 where some plane is non-zero (`!= 0` as numpy has it: a NaN is not zero), counts [blocks] <- masked pixels of each block.
// x [planes][n]; grid = ceil(n / 2048), 256 lanes.
__global__ __launch_bounds__(256) void prep_mask_counts(const float* __restrict__ x, int n_planes, long long n, uint8_t* __restrict__ mask,
                                                        int* __restrict__ counts) {
    __shared__ int total;
    if (threadIdx.x == 0) total = 0;
    __syncthreads();
    const long long i0 = (long long)blockIdx.x * kPrepMaskBlock + threadIdx.x;
    int mine = 0;
#pragma unroll
    for (int k = 0; k < kPrepMaskRows; ++k) {
        const long long i = i0 + k * 256;
        bool nz = false;
        if (i < n) {
            for (int c = 0; c < n_planes; ++c) nz |= x[(size_t)c * n + i] != 0.f;
            mask[i] = nz ? 1 : 0;
        }
        mine += __popcll(__ballot(nz));                          // (every lane of the wave holds the wave's count)
    }
    if ((threadIdx.x & 63) == 0) atomicAdd(&total, mine);        // integers: the order of the four waves does not show
    __syncthreads();
    if (threadIdx.x == 0) counts[blockIdx.x] = total;
}

// offs [nb] <- exclusive scan of counts [nb]; *total <- their sum.  One workgroup of 1024 lanes, each over a run of consecutive blocks.
__global__ __launch_bounds__(1024) void prep_mask_scan(const int* __restrict__ counts, int nb, int* __restrict__ offs, int* __restrict__ total) {
    __shared__ int part[1024];
    const int t = threadIdx.x, per = (nb + 1023) / 1024;
    const int b0 = t * per < nb ? t * per : nb, b1 = b0 + per < nb ? b0 + per : nb;
    int s = 0;
    for (int b = b0; b < b1; ++b) s += counts[b];
    part[t] = s;
    __syncthreads();
    for (int d = 1; d < 1024; d <<= 1) {
        const int v = t >= d ? part[t - d] : 0;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    int run = part[t] - s;
    for (int b = b0; b < b1; ++b) { offs[b] = run; run += counts[b]; }
    if (t == 1023) *total = part[1023];
}

// dst [planes][n_m] <- x[plane][mask], in index order.  grid = (ceil(n / 2048), planes), 256 lanes; offs from prep_mask_scan.
__global__ __launch_bounds__(256) void prep_mask_scatter(const float* __restrict__ x, long long n, const uint8_t* __restrict__ mask,
                                                         const int* __restrict__ offs, long long n_m, float* __restrict__ dst) {
    __shared__ int before[kPrepMaskRows * 4];                    // masked pixels of the block before wave w of row k, at [4 k + w]
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const long long i0 = (long long)blockIdx.x * kPrepMaskBlock + t;
    const unsigned long long below = (1ull << lane) - 1;
    int rank[kPrepMaskRows];
    unsigned in_mask = 0;
#pragma unroll
    for (int k = 0; k < kPrepMaskRows; ++k) {
        const long long i = i0 + k * 256;
        const bool m = i < n && mask[i] != 0;
        const unsigned long long b = __ballot(m);
        rank[k] = __popcll(b & below);
        in_mask |= (m ? 1u : 0u) << k;
        if (lane == 0) before[4 * k + wave] = __popcll(b);
    }
    __syncthreads();
    if (t < 64) {                                                // exclusive scan of the 32 wave counts in one wave
        const int c = t < kPrepMaskRows * 4 ? before[t] : 0;
        int s = c;
        for (int d = 1; d < 32; d <<= 1) { const int o = __shfl_up(s, d, 64); if (lane >= d) s += o; }
        if (t < kPrepMaskRows * 4) before[t] = s - c;
    }
    __syncthreads();
    const float* p = x + (size_t)blockIdx.y * n;
    float* o = dst + (size_t)blockIdx.y * n_m + offs[blockIdx.x];
#pragma unroll
    for (int k = 0; k < kPrepMaskRows; ++k)
        if (in_mask >> k & 1) o[before[4 * k + wave] + rank[k]] = p[i0 + k * 256];
}

// APPLY: x [planes][n] normalised in place by schemes[plane] (device_tables.h: PrepScheme), a masked row only where mask [n] is set;
// *status |= kPrepStatusRgbRange where an RGB plane holds a sample outside [0, 255] (a NaN is not outside, as in numpy's comparison).
// Not APPLY: schemes, mask and status are not read and x is not written.  Either way lo_hi [planes][2] receives prep_key of the minimum and
// maximum of every plane (of the result when APPLY), preset to {INT_MAX, INT_MIN} by the host.  grid = (ceil(n / 2048), planes), 256 lanes.
template <bool APPLY>
__global__ __launch_bounds__(256) void prep_apply_schemes(float* __restrict__ x, long long n, const PrepScheme* __restrict__ schemes,
                                                          const uint8_t* __restrict__ mask, int* __restrict__ lo_hi, int* __restrict__ status) {
#pragma clang fp contract(off)
    const int plane = blockIdx.y;
    PrepScheme s{kPrepNone, 0, 0.f, 1.f, 0.f, 0.f};
    if (APPLY) s = schemes[plane];
    float* p = x + (size_t)plane * n;
    const long long i0 = (long long)blockIdx.x * (256 * kPrepNormPerLane) + threadIdx.x;
    int lo = 0x7FFFFFFF, hi = (int)0x80000000;
    bool outside = false;
#pragma unroll
    for (int k = 0; k < kPrepNormPerLane; ++k) {
        const long long i = i0 + k * 256;
        if (i < n) {
            float v = p[i];
            if (s.id == kPrepCT) {
                v = v < s.lo ? s.lo : v;
                v = v > s.hi ? s.hi : v;
            }
            if (s.id == kPrepRGB01) outside |= v < 0.f || v > 255.f;
            if (s.id != kPrepNone && (!s.masked || mask[i] != 0)) {
                const float d = v - s.sub;
                v = d / s.div;
                p[i] = v;
            }
            const int key = prep_key(v);
            lo = key < lo ? key : lo; hi = key > hi ? key : hi;
        }
    }
    lo = prep_wave_min(lo); hi = prep_wave_max(hi);
    if (APPLY && __any(outside) && (threadIdx.x & 63) == 0) atomicOr(status, kPrepStatusRgbRange);
    __shared__ int red[8];
    if ((threadIdx.x & 63) == 0) { red[threadIdx.x >> 6] = lo; red[4 + (threadIdx.x >> 6)] = hi; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < 4; ++k) { lo = red[k] < lo ? red[k] : lo; hi = red[4 + k] > hi ? red[4 + k] : hi; }
        atomicMin(lo_hi + 2 * plane, lo); atomicMax(lo_hi + 2 * plane + 1, hi);
    }
}

}  // namespace ts2d
