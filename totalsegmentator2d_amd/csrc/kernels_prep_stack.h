// The planes of kernels_prep.h for a STACK: a 3-D volume [C][Z][H][W] that a 2-D plan takes slice by slice (reference flow
// DefaultPreprocessor.run_case, ts2d/core/inference/prediction_worker.py:194-199, with a volume where ts2d feeds a projection).  nnU-Net crops
// such a volume to ONE box over all three axes and normalises each channel with statistics of the WHOLE cropped volume; only the resample that
// follows is per slice, clipped to each slice's own minimum and maximum.  Three kernels behind ts2d_planes_crop_normalize_stack (prep.hip):
//     prep_nonzero_box3          the box {z0, z1, r0, r1, c0, c1} of the voxels that are non-zero in ANY channel (integer atomics, one pass)
//     prep_compact_box3          the box of every channel copied into a dense [C][Z'][h'][w'] buffer: its flattened index is numpy's
//     prep_apply_schemes_stack<A, M> prep_apply_schemes of kernels_prep_schemes.h with the scheme row of plane / Z': A = true normalises
//                                every slice in place by its CHANNEL's row and leaves the float32 minimum and maximum of each SLICE as integer
//                                keys; A = false leaves the keys of the slices as they are (the minimum and maximum behind Rescale: the host
//                                folds them over a channel's slices, integers again).  M = false reads no mask; M = true normalises a masked row
//                                only inside the volume's hole-filled mask (kernels_prep_fill.h), behind ts2d_planes_crop_normalize_stack_masked
// The sums of the z-score are prep_chunk_sums<0 / 1> of kernels_prep.h, unchanged, over C runs of N = Z' h' w' elements: numpy copies the cropped
// view of a channel into a dense C-ordered array and reduces that, so its chunks of 8192 cross the slice boundaries exactly as these do
// (tests/test_stack_cpu.py).  Arithmetic = the statements of preprocess.py applied to the flattened channel, bit for bit; every subtraction and
// division under `#pragma clang fp contract(off)`, the division the correctly rounded float32 `/`, numpy's clip spelled out with comparisons.
// No float atomics; the result does not depend on the launch shape.  Pure HBM streaming, no MFMA; LDS holds eight integers per workgroup.
#pragma once
#include "kernels_prep_schemes.h"

namespace ts2d {

// box = {first slice, last slice, first row, last row, first column, last column}, preset to {z, -1, h, -1, w, -1} by the host (a volume of zeros
// leaves it so and keeps its whole extent).  `v != 0` as numpy has it: a NaN is not zero, -0.0 is.  x [channels][z][h][w]; one lane per voxel,
// one set of atomics per wave that saw a non-zero voxel.  grid = ceil(z h w / 256), 256 lanes.
__global__ __launch_bounds__(256) void prep_nonzero_box3(const float* __restrict__ x, int channels, int z, int h, int w, int* __restrict__ box) {
    const long long hw = (long long)h * w, n = hw * z, i = (long long)blockIdx.x * 256 + threadIdx.x;
    bool nz = false;
    if (i < n)
        for (int c = 0; c < channels; ++c) nz |= x[(size_t)c * n + i] != 0.f;
    const int sl = (int)(i / hw), in_plane = (int)(i % hw);
    const int row = in_plane / w, col = in_plane % w;
    const int z0 = prep_wave_min(nz ? sl : z), z1 = prep_wave_max(nz ? sl : -1);
    const int r0 = prep_wave_min(nz ? row : h), r1 = prep_wave_max(nz ? row : -1);
    const int c0 = prep_wave_min(nz ? col : w), c1 = prep_wave_max(nz ? col : -1);
    if ((threadIdx.x & 63) == 0 && z1 >= 0) {
        atomicMin(box + 0, z0); atomicMax(box + 1, z1); atomicMin(box + 2, r0); atomicMax(box + 3, r1); atomicMin(box + 4, c0); atomicMax(box + 5, c1);
    }
}

// dst [channels][bz][bh][bw] <- src [channels][z][h][w] at (z0 + ., r0 + ., c0 + .).  grid = (ceil(bh bw / 256), bz, channels), 256 lanes.
__global__ __launch_bounds__(256) void prep_compact_box3(const float* __restrict__ src, int z, int h, int w, int z0, int r0, int c0, int bh, int bw,
                                                         float* __restrict__ dst) {
    const int i = blockIdx.x * 256 + threadIdx.x;               // (bh bw <= 8192^2 = 2^26)
    if (i >= bh * bw) return;
    const int row = i / bw, col = i % bw;
    const size_t from = (((size_t)blockIdx.z * z + z0 + blockIdx.y) * h + r0 + row) * w + c0 + col;
    dst[((size_t)blockIdx.z * gridDim.y + blockIdx.y) * bh * bw + i] = src[from];
}

// prep_apply_schemes for the slices x [channels * slices][n] of a stack: slice `plane` is normalised by schemes[plane / slices] - with MASKED a masked
// row only where mask [slices][n], the mask of the volume that all channels share, is set, the sample itself elsewhere; without it mask is not read;
// lo_hi [channels * slices][2] receives prep_key of each SLICE's minimum and maximum, preset to {INT_MAX, INT_MIN} by the host; *status as there.
// Not APPLY: schemes and status are not read and x is not written.  grid = (ceil(n / 2048), channels * slices), 256 lanes.
template <bool APPLY, bool MASKED>
__global__ __launch_bounds__(256) void prep_apply_schemes_stack(float* __restrict__ x, long long n, int slices, const PrepScheme* __restrict__ schemes,
                                                                const uint8_t* __restrict__ mask, int* __restrict__ lo_hi, int* __restrict__ status) {
#pragma clang fp contract(off)
    const int plane = blockIdx.y;
    PrepScheme s{kPrepNone, 0, 0.f, 1.f, 0.f, 0.f};
    if (APPLY) s = schemes[plane / slices];
    float* p = x + (size_t)plane * n;
    const uint8_t* m = MASKED ? mask + (size_t)(plane % slices) * n : nullptr;
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
            if (s.id != kPrepNone && (!MASKED || !s.masked || m[i] != 0)) {
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
