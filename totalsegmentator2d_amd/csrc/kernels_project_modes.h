// Every projection mode of the reference's project() along the coronal axis (ts2d/core/util/image.py:46-101): max, min, mean, median, std,
// first (= depth) and slice, behind ts2d_project_coronal_modes.  The volume is addressed as project_coronal (kernels_project.h) addresses
// it - signed element strides and the base of the reoriented view - so no reorientation copy is made.  The host statement of every mode is
// totalsegmentator2d_amd.image.project; tests/test_gpu_projection_modes.py holds these kernels against it bit for bit.
//
//   project_modes_stream   one lane per output pixel (z, x), one pass over the ray in index order for whichever of max, min, mean sum and first
//                          were asked for (max and mean: the arithmetic of project_coronal, statement for statement); the slices are single reads;
//                          std makes a second pass over the same ray with the mean in a register: float64, multiply and add rounded separately
//                          (contraction off), correctly rounded divide and square root.  On a float volume it also looks for a non-finite
//                          sample and reports it in the status word (one integer atomic per lane that found one): such a volume has no
//                          place in the key order below, and the caller takes the host route.
//   project_median_lds     a workgroup takes tile_x adjacent x of one z.  It stages the keys (ray_select.h) of its
//                          [ny][tile_x] samples in LDS in that order, so thread t reads element j * 256 + t in its j-th step - consecutive
//                          addresses across a wave for every tile_x - and the volume is read from HBM once.  The 256 threads are 256 / tile_x
//                          groups of tile_x lanes; group g counts over the rows y = g (mod groups).  Per key bit: every thread counts its
//                          share, the counts meet in LDS (two buffers in turn: one barrier per bit), every thread adds the groups' counts of its
//                          own x and takes the decision of ray_select.h.  The pick goes out with a plain store from group 0.
//   project_median_global  the same selection with one lane per pixel that reads its ray from global memory once per key bit: for the rays
//                          that do not fit in LDS at the narrowest tile.
// No atomics in the median kernels, no flags, nothing waits for another workgroup; every loop bound is a kernel argument or a constant.
//
// LDS budget.  A CU has 160 KiB; a workgroup takes at most half of it, 2 KiB of counts and kPmLdsKeyBytes = 78 KiB of keys, so that two
// workgroups share a CU.  Keys are as wide as the samples.  Longest ray held in LDS, by element size and tile width:
//       element     tile_x = 64     tile_x = 32     tile_x = 16
//       1 byte          1248            2496            4992
//       2 bytes          624            1248            2496
//       4 bytes          312             624            1248
// A longer ray goes to project_median_global, up to kPmRayCap = 8192 samples; above the cap the entry sets TS2D_PROJECT_RAY_TOO_LONG and
// launches nothing.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>

#include "kernels_project.h"
#include "ray_select.h"

namespace ts2d {

enum { kPmMax = 0, kPmMin = 1, kPmMean = 2, kPmMedian = 3, kPmStd = 4, kPmFirst = 5, kPmSlice = 6, kPmKinds = 7 };
constexpr int kPmMaxModes = 16;
constexpr int kPmThreads = 256;
constexpr int kPmLdsCountBytes = 2 * kPmThreads * (int)sizeof(int);
constexpr int kPmLdsKeyBytes = 78 * 1024;
constexpr int kPmRayCap = 8192;
constexpr int kPmStatusNonFinite = 1, kPmStatusRayTooLong = 2;

// the widest tile whose [ny][tile_x] keys of `esize` bytes fit in kPmLdsKeyBytes; 0: none does
inline int pm_tile_x(int ny, int esize) {
    for (int tx = 64; tx >= 16; tx >>= 1)
        if ((long long)ny * tx * esize <= kPmLdsKeyBytes) return tx;
    return 0;
}

struct PmStreamArgs {
    float* out[kPmKinds];               // the plane of a kind, or null when it was not asked for (kPmMedian, kPmSlice: unused here)
    int n_slices;
    int slice_y[kPmMaxModes];
    float* slice_out[kPmMaxModes];
};

template <typename T>
__global__ __launch_bounds__(256) void project_modes_stream(const T* __restrict__ vol, int nz, int ny, int nx, long long sz, long long sy, long long sx,
                                                             long long base, PmStreamArgs a, int* __restrict__ status) {
#pragma clang fp contract(off)
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)nz * nx) return;
    const int x = (int)(i % nx), z = (int)(i / nx);
    const T* p = vol + base + z * sz + x * sx;
    double mean;
    if constexpr (std::is_floating_point<T>::value) {
        float mx = (float)p[0], mn = mx, first = mx; double s = 0.0;
        bool found = false, bad = false;
        for (int y = 0; y < ny; ++y) {
            const float v = (float)p[y * sy];
            bad |= (__float_as_uint(v) & 0x7F800000u) == 0x7F800000u;
            mx = v > mx ? v : mx; mn = v < mn ? v : mn; s += (double)v;
            if (!found && v != 0.f) { first = v; found = true; }
        }
        if (bad) atomicOr(status, kPmStatusNonFinite);
        mean = s / ny;
        if (a.out[kPmMax]) a.out[kPmMax][i] = mx;
        if (a.out[kPmMin]) a.out[kPmMin][i] = mn;
        if (a.out[kPmMean]) a.out[kPmMean][i] = (float)mean;
        if (a.out[kPmFirst]) a.out[kPmFirst][i] = first;
    } else {                                                       // integer volume: exact sum, real-valued mean
        long long mx = (long long)p[0], mn = mx, first = mx, s = 0;
        bool found = false;
        for (int y = 0; y < ny; ++y) {
            const long long v = (long long)p[y * sy];
            mx = v > mx ? v : mx; mn = v < mn ? v : mn; s += v;
            if (!found && v != 0) { first = v; found = true; }
        }
        mean = (double)s / (double)ny;
        if (a.out[kPmMax]) a.out[kPmMax][i] = (float)mx;
        if (a.out[kPmMin]) a.out[kPmMin][i] = (float)mn;
        if (a.out[kPmMean]) a.out[kPmMean][i] = (float)mean;
        if (a.out[kPmFirst]) a.out[kPmFirst][i] = (float)first;
    }
    for (int k = 0; k < a.n_slices; ++k) a.slice_out[k][i] = (float)p[a.slice_y[k] * sy];
    if (a.out[kPmStd]) {                                           // sample standard deviation: second pass, the mean in a register
        double sq = 0.0;
        for (int y = 0; y < ny; ++y) { const double d = (double)p[y * sy] - mean; const double dd = d * d; sq = sq + dd; }
        a.out[kPmStd][i] = (float)sqrt(sq / (double)(ny - 1));
    }
}

// grid = (tiles_x * nz); dynamic LDS = kPmLdsCountBytes + ny * tile_x keys; tile_x = 1 << lg_tile_x in {16, 32, 64}; n_full = ny * tile_x / 256 (rounded down)
template <typename T>
__global__ __launch_bounds__(256) void project_median_lds(const T* __restrict__ vol, int nz, int ny, int nx, long long sz, long long sy, long long sx,
                                                           long long base, int lg_tile_x, int tiles_x, int n_full, float* __restrict__ out) {
    typedef typename RsKey<T>::type K;
    extern __shared__ __attribute__((aligned(16))) unsigned char pm_smem[];
    int* cnt = reinterpret_cast<int*>(pm_smem);                    // [2][256]
    K* keys = reinterpret_cast<K*>(pm_smem + kPmLdsCountBytes);    // [ny][tile_x]
    const int tile_x = 1 << lg_tile_x, groups = kPmThreads >> lg_tile_x;
    const int t = threadIdx.x, x = t & (tile_x - 1);
    const int z = (int)(blockIdx.x / tiles_x), gx = (int)(blockIdx.x % tiles_x) * tile_x + x;
    const bool live = gx < nx;
    const int total = ny * tile_x;
    const T* p = vol + base + z * sz + (live ? gx : 0) * sx;      // a lane beyond nx stages column 0 again: a valid address, its pick is not stored
    // n_full steps in which every thread has an element (no guard: the loads of a step group are in flight together), then at most one more
    const int tail = n_full * kPmThreads + t;
#pragma unroll 4
    for (int j = 0; j < n_full; ++j) {
        const int idx = j * kPmThreads + t;
        keys[idx] = rs_key(p[(idx >> lg_tile_x) * sy]);
    }
    if (tail < total) keys[tail] = rs_key(p[(tail >> lg_tile_x) * sy]);
    __syncthreads();
    uint32_t prefix = 0, sel = 0;
    int k = ny / 2;
    for (int b = RsKey<T>::bits - 1; b >= 0; --b) {
        const uint32_t bit = 1u << b;
        sel |= bit;
        int c = 0;
#pragma unroll 8
        for (int j = 0; j < n_full; ++j) c += rs_counts((uint32_t)keys[j * kPmThreads + t], sel, prefix);
        if (tail < total) c += rs_counts((uint32_t)keys[tail], sel, prefix);
        int* cb = cnt + (b & 1) * kPmThreads;                      // the buffer written two bits ago: every thread has passed a barrier since it read it
        cb[t] = c;
        __syncthreads();
        int clear = 0;
        for (int g = 0; g < groups; ++g) clear += cb[(g << lg_tile_x) + x];
        rs_decide(clear, bit, &k, &prefix);
    }
    if (t < tile_x && live) out[(long long)z * nx + gx] = (float)rs_unkey<T>((K)prefix);
}

template <typename T>
__global__ __launch_bounds__(256) void project_median_global(const T* __restrict__ vol, int nz, int ny, int nx, long long sz, long long sy, long long sx,
                                                              long long base, float* __restrict__ out) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)nz * nx) return;
    const int x = (int)(i % nx), z = (int)(i / nx);
    out[i] = (float)rs_select_kth_samples<T>(vol + base + z * sz + x * sx, ny, sy, ny / 2);
}

// zs_apply (kernels_project.h) with the non-zero box PER PLANE: grid = (ceil(n / 256), planes), box = [planes][4], each {min row, max row, min col,
// max col} from {nz, -1, nx, -1}.  The host forms the union over the planes of one sub-model's channel set.
__global__ void zs_apply_planes(const float* __restrict__ x, long long n, int nx, const double* __restrict__ stats, float* __restrict__ out,
                                int* __restrict__ box) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int c = blockIdx.y;
    const float v = x[(long long)c * n + i];
    const double sd = stats[2 * c + 1] > 1e-8 ? stats[2 * c + 1] : 1e-8;
    out[(long long)c * n + i] = (float)(((double)v - stats[2 * c]) / sd);
    if (v != 0.f) {
        const int row = (int)(i / nx), col = (int)(i % nx);
        int* b = box + 4 * c;
        atomicMin(b + 0, row); atomicMax(b + 1, row); atomicMin(b + 2, col); atomicMax(b + 3, col);
    }
}

}  // namespace ts2d
