// Device side of nnU-Net's preprocessing of an input that is 2-D when it arrives (reference flow DefaultPreprocessor.run_case,
// ts2d/core/inference/prediction_worker.py:194-199): crop_to_nonzero's box, the per-channel ZScoreNormalization without mask, and the clip
// bounds of the resample that follows.  Four kernels behind the ts2d_planes handle (prep.hip):
//     prep_nonzero_box      the bounding box of the pixels that are non-zero in ANY plane (integer atomics, one pass over all planes)
//     prep_chunk_sums<P>    numpy's float32 sum of a plane, chunk by chunk (P = 0: of x; P = 1: of fl32(fl32(x - mean)^2))
//     prep_normalise        x <- fl32(fl32(x - mean) / div) in place, and the plane's float32 minimum and maximum
// (the compaction of the box between the first two is a strided device copy).
//
// Arithmetic = preprocess.zscore_f32_statement, bit for bit, which is bit for bit numpy's `img.mean()`, `img.std()`, `img -= mean`,
// `img /= max(std, 1e-8)` on a C-contiguous float32 plane (tests/test_prep_cpu.py).  numpy's add.reduce hands the flattened plane to its
// inner loop in chunks of 8192 elements (its buffer size); the loop adds the PAIRWISE sum of a chunk to the running float32 result,
// which starts at +0.  The pairwise sum of a run of n elements:
//     n < 8      res = 0; res += a[i] one by one
//     n <= 128   eight accumulators r[j] = a[j], r[j] += a[8 i + j] for 8 i + j < n - n % 8, then
//                res = ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7)); res += a[i] for the n % 8 last elements
//     n > 128    n2 = n / 2 - (n / 2) % 8;  pairwise(a, n2) + pairwise(a + n2, n - n2)
// A run of <= 128 elements is a LEAF.  Eight lanes own a leaf, lane j holds r[j]: a wave covers eight leaves and every load instruction
// fetches eight 32-byte groups.  The combination of the eight accumulators is a butterfly over lane bits 0, 1, 2 (float addition
// commutes exactly, so a ^ b order is the statement's order); every lane of the eight then adds the tail and holds the leaf's sum.
// A FULL chunk of 8192 elements is 64 leaves of 128 under a perfect binary tree whose nodes add neighbouring halves: the butterfly
// goes on over lane bits 3, 4, 5 (the eight leaves of a wave) and ends with the eight wave sums of the 512-lane workgroup added by one
// lane in the same tree order.  One workgroup per full chunk writes one float.  The LAST, partial chunk of a plane has a tree of its
// own: the host walks the recursion once per extent and uploads its leaves (offset, length); the workgroup behind the full chunks
// writes one float per leaf and the host folds them along the recursion.  The host then adds the chunk sums in index order and
// computes mean, variance, square root and divisor in float32 (prep_plan.cpp: prep_*), so no reduction order is left to the device.
// No float atomics anywhere; the result does not depend on the launch shape.
//
// Every float32 sum, difference and product is a plain operator under `#pragma clang fp contract(off)` (prep_add, prep_term): hipcc contracts
// d * d + r into v_fmac_f32 by default, which would drop the rounding of the product, and HIP's __fmul_rn / __fadd_rn are plain operators
// that it fuses just the same (tests/test_prep_cpu.py reads the emitted stream of prep_chunk_sums: v_add_f32 / v_mul_f32 / v_sub_f32
// and no fused form, no scratch, no spills).  The division is the
// correctly rounded float32 `/` (hipcc's default, as kernels_fold.h relies on it); float32 denormals are kept.
//
// Pure HBM streaming: the box pass reads every plane once, each sum pass reads the compacted planes once, the normalise pass reads
// and writes them once.  Nothing here uses MFMA; LDS holds eight floats, or two dozen integers, per workgroup.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "device_tables.h"      // kPrepChunk, kPrepLeaf, kPrepMaxTailLeaves, PrepLeaf, PrepNorm

namespace ts2d {

__device__ __forceinline__ float prep_add(float a, float b) {
#pragma clang fp contract(off)
    return a + b;
}

// the value pass P sums: x itself, or the square of its rounded distance from the mean (two roundings, as numpy's x = arr - mean; x * x)
template <int PASS>
__device__ __forceinline__ float prep_term(float x, float mean) {
#pragma clang fp contract(off)
    if (PASS == 0) return x;
    const float d = x - mean;
    return d * d;
}

__device__ __forceinline__ float prep_xor(float v, int mask) { return __shfl_xor(v, mask, 64); }

// The pairwise sum of one leaf a[0 ... len), len <= 128, by the eight lanes that own it (j = lane & 7); every one of them returns it.
template <int PASS>
__device__ __forceinline__ float prep_leaf_sum(const float* __restrict__ a, int len, int j, float mean) {
    if (len < 8) {                                               // (the eight lanes agree on len: no lane is left out of the shuffles below)
        float res = 0.f;
        for (int i = 0; i < len; ++i) res = prep_add(res, prep_term<PASS>(a[i], mean));
        return res;
    }
    const int m = len - (len & 7);
    float r = prep_term<PASS>(a[j], mean);
    if (len == kPrepLeaf) {                                      // the leaves of a full chunk: 15 loads in flight together
        float v[15];
#pragma unroll
        for (int i = 0; i < 15; ++i) v[i] = a[8 * (i + 1) + j];
#pragma unroll
        for (int i = 0; i < 15; ++i) r = prep_add(r, prep_term<PASS>(v[i], mean));
    } else {
        for (int i = 8; i < m; i += 8) r = prep_add(r, prep_term<PASS>(a[i + j], mean));
    }
    r = prep_add(r, prep_xor(r, 1));                             // r0 + r1 | r2 + r3 | r4 + r5 | r6 + r7
    r = prep_add(r, prep_xor(r, 2));                             // (r0 + r1) + (r2 + r3) | (r4 + r5) + (r6 + r7)
    r = prep_add(r, prep_xor(r, 4));
    for (int i = m; i < len; ++i) r = prep_add(r, prep_term<PASS>(a[i], mean));
    return r;
}

// grid = (full chunks + (partial chunk ? 1 : 0), planes), 512 lanes.  x [planes][n]; out [planes][n_out] with n_out = full chunks +
// tail leaves: one float per full chunk, then one per leaf of the partial chunk (leaves[0 ... n_tail_leaves), offsets from the chunk).
template <int PASS>
__global__ __launch_bounds__(512) void prep_chunk_sums(const float* __restrict__ x, long long n, const PrepNorm* __restrict__ norm,
                                                       const PrepLeaf* __restrict__ leaves, int n_tail_leaves, float* __restrict__ out) {
    const int plane = blockIdx.y;
    const long long n_full = n / kPrepChunk;
    const float mean = PASS ? norm[plane].mean : 0.f;
    const float* p = x + (size_t)plane * n + (size_t)blockIdx.x * kPrepChunk;
    float* o = out + (size_t)plane * (n_full + n_tail_leaves);
    const int t = threadIdx.x, j = t & 7;
    if ((long long)blockIdx.x < n_full) {
        float s = prep_leaf_sum<PASS>(p + (t >> 3) * kPrepLeaf, kPrepLeaf, j, mean);
        s = prep_add(s, prep_xor(s, 8));                         // leaves 2 i and 2 i + 1 of the wave, then pairs of pairs, then all eight
        s = prep_add(s, prep_xor(s, 16));
        s = prep_add(s, prep_xor(s, 32));
        __shared__ float wave[8];
        if ((t & 63) == 0) wave[t >> 6] = s;
        __syncthreads();
        if (t == 0)
            o[blockIdx.x] = prep_add(prep_add(prep_add(wave[0], wave[1]), prep_add(wave[2], wave[3])),
                                     prep_add(prep_add(wave[4], wave[5]), prep_add(wave[6], wave[7])));
    } else {
        for (int l = t >> 3; l < n_tail_leaves; l += 64) {       // (a leaf's eight lanes leave the loop together)
            const PrepLeaf lf = leaves[l];
            const float s = prep_leaf_sum<PASS>(p + lf.off, lf.len, j, mean);
            if (j == 0) o[n_full + l] = s;
        }
    }
}

// float32 <-> an integer whose signed order is the float order, -0 below +0 and the NaNs outside the infinities: min / max by integer atomics
__device__ __forceinline__ int prep_key(float f) { const int b = __float_as_int(f); return b < 0 ? b ^ 0x7FFFFFFF : b; }

__device__ __forceinline__ int prep_wave_min(int v) {
    for (int m = 32; m > 0; m >>= 1) { const int o = __shfl_xor(v, m, 64); v = o < v ? o : v; }
    return v;
}
__device__ __forceinline__ int prep_wave_max(int v) {
    for (int m = 32; m > 0; m >>= 1) { const int o = __shfl_xor(v, m, 64); v = o > v ? o : v; }
    return v;
}

// box = {first row, last row, first column, last column} of the pixels that are non-zero in any plane, preset to {h, -1, w, -1} by the host
// (an image of zeros leaves it so and keeps its whole extent).  `v != 0` as numpy has it: a NaN is not zero.  x [planes][h][w]; one lane
// per pixel, one set of atomics per wave that saw a non-zero pixel.
__global__ __launch_bounds__(256) void prep_nonzero_box(const float* __restrict__ x, int n_planes, int h, int w, int* __restrict__ box) {
    const long long n = (long long)h * w, i = (long long)blockIdx.x * 256 + threadIdx.x;
    bool nz = false;
    if (i < n)
        for (int c = 0; c < n_planes; ++c) nz |= x[(size_t)c * n + i] != 0.f;
    const int row = (int)(i / w), col = (int)(i % w);
    const int r0 = prep_wave_min(nz ? row : h), r1 = prep_wave_max(nz ? row : -1);
    const int c0 = prep_wave_min(nz ? col : w), c1 = prep_wave_max(nz ? col : -1);
    if ((threadIdx.x & 63) == 0 && r1 >= 0) { atomicMin(box + 0, r0); atomicMax(box + 1, r1); atomicMin(box + 2, c0); atomicMax(box + 3, c1); }
}

constexpr int kPrepNormPerLane = 8;     // elements of a plane per lane of prep_normalise, 256 lanes apart

// x [planes][n] <- fl32(fl32(x - mean) / div) in place; lo_hi [planes][2]: prep_key of the plane's minimum and maximum, preset to
// {INT_MAX, INT_MIN} by the host.  A non-finite result shows in them (an infinity is a bound, a NaN lies outside the infinities).
// grid = (ceil(n / 2048), planes), 256 lanes.
__global__ __launch_bounds__(256) void prep_normalise(float* __restrict__ x, long long n, const PrepNorm* __restrict__ norm, int* __restrict__ lo_hi) {
#pragma clang fp contract(off)
    const int plane = blockIdx.y;
    const PrepNorm nm = norm[plane];
    float* p = x + (size_t)plane * n;
    const long long i0 = (long long)blockIdx.x * (256 * kPrepNormPerLane) + threadIdx.x;
    int lo = 0x7FFFFFFF, hi = (int)0x80000000;
#pragma unroll
    for (int k = 0; k < kPrepNormPerLane; ++k) {
        const long long i = i0 + k * 256;
        if (i < n) {
            const float d = p[i] - nm.mean;
            const float v = d / nm.div;
            p[i] = v;
            const int key = prep_key(v);
            lo = key < lo ? key : lo; hi = key > hi ? key : hi;
        }
    }
    lo = prep_wave_min(lo); hi = prep_wave_max(hi);
    __shared__ int red[8];
    if ((threadIdx.x & 63) == 0) { red[threadIdx.x >> 6] = lo; red[4 + (threadIdx.x >> 6)] = hi; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < 4; ++k) { lo = red[k] < lo ? red[k] : lo; hi = red[4 + k] > hi ? red[4 + k] : hi; }
        atomicMin(lo_hi + 2 * plane, lo); atomicMax(lo_hi + 2 * plane + 1, hi);
    }
}

}  // namespace ts2d
