// Per-label statistics of a segmentation behind ts2d_label_statistics: voxel count, bounding box, index sums and, per intensity channel, minimum,
// maximum, float64 sum and sum of squared deviations.  The statement is totalsegmentator2d_amd.statistics.label_statistics_statement;
// tests/test_gpu_statistics.py holds these kernels against it bit for bit, the float64 sums included.  A volume is R = Z * H rows of W samples.
//
//   stats_rows<1>      one wave per (label, row): lanes stride the row, read the mask byte, keep count, sum, minimum and maximum of x in
//                      registers and meet across lanes; lane 0 writes the row's integer partial.  A row without a sample of the label is done
//                      there (its float partials are +0.0 and the empty keys: what the tree gives for it).  Otherwise, per channel, the lane sums
//                      of stats_tree.h (st_lane_sum), the halving, the keys; a non-finite sample under the label sets the status word
//                      (one integer atomicOr per wave that found one).
//   stats_combine<1>   one wave per label over its row partials: integers and box, then per channel the level-2 tree, minimum, maximum and
//                      mean = sum / count (IEEE divide) into the label's result.
//   stats_rows<2>      the same walk with the label's mean in a register: the squared deviations (st_lane_ssq), into the slot of the sum.
//   stats_combine<2>   the level-2 tree over them, std = sqrt(ssq / count) (IEEE divide and square root).
// Plain vector stores of partials; no floating-point atomics, no flags, nothing waits for another wave: a phase finds what it needs behind the
// launch boundary.  Indices are int32 (the entry refuses more than 2^31 - 1 voxels and sizes a label chunk so that its partials stay below that
// too); a plane or channel is reached through its own base pointer.
//
// Result layout (also the entry's): out_int [K][kStInts] int64 = count, index sum along z, y, x, then min z, max z, min y, max y, min x, max x
// (an empty label: sums 0, minima the extents, maxima -1); out_f64 [K][C][kStF64s] = sum, ssq, mean, std, min, max (an empty label: all +0.0).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "stats_tree.h"

namespace ts2d {

constexpr int kStInts = 10, kStF64s = 6;
constexpr int kStStatusNonfinite = 1;

// the row partials of one chunk of L labels: [L][R] integers, [L][C][R] per channel
struct StScratch {
    int* cnt; int* minx; int* maxx; long long* sumx;
    double* fsum; uint32_t* kmin; uint32_t* kmax;
};

// the halving of stats_tree.h across the 64 lanes of a wave: lane l takes v[l] + v[l + off] for off = 32, 16, ..., 1; lane 0 holds the result
// (the lanes at and above `off` add a value of no consequence).
__device__ __forceinline__ double st_wave_halve(double v) {
#pragma clang fp contract(off)
    for (int off = kStLanes / 2; off >= 1; off >>= 1) v = v + __shfl_down(v, off, kStLanes);
    return v;
}
__device__ __forceinline__ long long st_wave_sum(long long v) {
    for (int off = kStLanes / 2; off >= 1; off >>= 1) v += __shfl_down(v, off, kStLanes);
    return v;
}
__device__ __forceinline__ int st_wave_min(int v) {
    for (int off = kStLanes / 2; off >= 1; off >>= 1) { const int o = __shfl_down(v, off, kStLanes); v = o < v ? o : v; }
    return v;
}
__device__ __forceinline__ int st_wave_max(int v) {
    for (int off = kStLanes / 2; off >= 1; off >>= 1) { const int o = __shfl_down(v, off, kStLanes); v = o > v ? o : v; }
    return v;
}
__device__ __forceinline__ uint32_t st_wave_umin(uint32_t v) {
    for (int off = kStLanes / 2; off >= 1; off >>= 1) { const uint32_t o = (uint32_t)__shfl_down((int)v, off, kStLanes); v = o < v ? o : v; }
    return v;
}
__device__ __forceinline__ uint32_t st_wave_umax(uint32_t v) {
    for (int off = kStLanes / 2; off >= 1; off >>= 1) { const uint32_t o = (uint32_t)__shfl_down((int)v, off, kStLanes); v = o > v ? o : v; }
    return v;
}

// grid = (R, L), block = 64; where R * 64 passes 2^32 the rows fold along z (entry_util.h: fold_grid), row = blockIdx.z * gridDim.x + blockIdx.x.
// seg: planes [K][n] or one label map [n] with values [K]; label k0 + blockIdx.y; x: [C][n] float32;
// result: the labels' out_f64 (PASS 2 reads the mean there).
template <int PASS>
__global__ __launch_bounds__(64) void stats_rows(const uint8_t* __restrict__ seg, int kind, const uint8_t* __restrict__ values, int k0, int R, int W,
                                                 long long n, const float* __restrict__ x, int C, StScratch s, const double* __restrict__ result,
                                                 int* __restrict__ status) {
    const long long row = (long long)blockIdx.z * gridDim.x + blockIdx.x;
    if (row >= R) return;                                          // (the whole wave: the last fold of a folded grid)
    const int r = (int)row, l = (int)blockIdx.y, k = k0 + l, lane = (int)threadIdx.x;
    const uint8_t* m = seg + (kind == kStPlanes ? (long long)k * n : 0ll) + (long long)r * W;
    const uint8_t value = kind == kStLabelMap ? values[k] : (uint8_t)0;
    const int slot = l * R + r;
    if (PASS == 1) {
        int cnt = 0, mn = 0x7FFFFFFF, mx = -1;
        long long sx = 0;
        const int trips = st_lane_trips(W, lane);
        for (int j = 0; j < trips; ++j) {
            const int i = lane + j * kStLanes;
            if (st_masked(m[i], kind, value)) { ++cnt; sx += i; mn = i < mn ? i : mn; mx = i; }
        }
        cnt = (int)st_wave_sum((long long)cnt); sx = st_wave_sum(sx); mn = st_wave_min(mn); mx = st_wave_max(mx);
        if (lane == 0) { s.cnt[slot] = cnt; s.sumx[slot] = sx; s.minx[slot] = mn; s.maxx[slot] = mx; }
        cnt = __shfl(cnt, 0, kStLanes);
        for (int c = 0; c < C; ++c) {
            const long long fslot = ((long long)l * C + c) * R + r;
            if (cnt == 0) {
                if (lane == 0) { s.fsum[fslot] = 0.0; s.kmin[fslot] = 0xFFFFFFFFu; s.kmax[fslot] = 0u; }
                continue;
            }
            uint32_t lo = 0xFFFFFFFFu, hi = 0u;
            int bad = 0;
            double v = st_lane_sum(m, kind, value, x + (long long)c * n + (long long)r * W, W, lane, &lo, &hi, &bad);
            v = st_wave_halve(v); lo = st_wave_umin(lo); hi = st_wave_umax(hi); bad = st_wave_max(bad);
            if (lane == 0) {
                s.fsum[fslot] = v; s.kmin[fslot] = lo; s.kmax[fslot] = hi;
                if (bad) atomicOr(status, kStStatusNonfinite);
            }
        }
    } else {
        const int cnt = s.cnt[slot];
        for (int c = 0; c < C; ++c) {
            const long long fslot = ((long long)l * C + c) * R + r;
            if (cnt == 0) {
                if (lane == 0) s.fsum[fslot] = 0.0;
                continue;
            }
            const double mean = result[((long long)k * C + c) * kStF64s + 2];
            double v = st_lane_ssq(m, kind, value, x + (long long)c * n + (long long)r * W, W, lane, mean);
            v = st_wave_halve(v);
            if (lane == 0) s.fsum[fslot] = v;
        }
    }
}

// grid = L, block = 64.  out_int [K][kStInts], out_f64 [K][C][kStF64s] on the device.
template <int PASS>
__global__ __launch_bounds__(64) void stats_combine(int k0, int R, int H, int Z, int W, int C, StScratch s, long long* __restrict__ out_int,
                                                    double* __restrict__ out_f64) {
#pragma clang fp contract(off)
    const int l = (int)blockIdx.x, k = k0 + l, lane = (int)threadIdx.x;
    const int trips = st_lane_trips(R, lane);
    long long count;
    if (PASS == 1) {
        long long cn = 0, sz = 0, sy = 0, sx = 0;
        int mnz = Z, mxz = -1, mny = H, mxy = -1, mnx = W, mxx = -1;
        for (int j = 0; j < trips; ++j) {
            const int r = lane + j * kStLanes, slot = l * R + r, c = s.cnt[slot];
            if (c == 0) continue;
            const int z = r / H, y = r - z * H;
            cn += c; sz += (long long)z * c; sy += (long long)y * c; sx += s.sumx[slot];
            mnz = z < mnz ? z : mnz; mxz = z > mxz ? z : mxz; mny = y < mny ? y : mny; mxy = y > mxy ? y : mxy;
            const int a = s.minx[slot], b = s.maxx[slot];
            mnx = a < mnx ? a : mnx; mxx = b > mxx ? b : mxx;
        }
        cn = st_wave_sum(cn); sz = st_wave_sum(sz); sy = st_wave_sum(sy); sx = st_wave_sum(sx);
        mnz = st_wave_min(mnz); mxz = st_wave_max(mxz); mny = st_wave_min(mny); mxy = st_wave_max(mxy); mnx = st_wave_min(mnx); mxx = st_wave_max(mxx);
        if (lane == 0) {
            long long* o = out_int + (long long)k * kStInts;
            o[0] = cn; o[1] = sz; o[2] = sy; o[3] = sx; o[4] = mnz; o[5] = mxz; o[6] = mny; o[7] = mxy; o[8] = mnx; o[9] = mxx;
        }
        count = __shfl(cn, 0, kStLanes);
    } else {
        count = out_int[(long long)k * kStInts];
    }
    for (int c = 0; c < C; ++c) {
        const long long base = ((long long)l * C + c) * R;
        double v = st_wave_halve(st_lane_rows(s.fsum + base, R, lane));
        double* o = out_f64 + ((long long)k * C + c) * kStF64s;
        if (PASS == 1) {
            uint32_t lo = 0xFFFFFFFFu, hi = 0u;
            for (int j = 0; j < trips; ++j) {
                const long long i = base + lane + j * kStLanes;
                const uint32_t a = s.kmin[i], b = s.kmax[i];
                lo = a < lo ? a : lo; hi = b > hi ? b : hi;
            }
            lo = st_wave_umin(lo); hi = st_wave_umax(hi);
            if (lane == 0) {
                o[0] = v;
                o[2] = count ? v / (double)count : 0.0;
                o[4] = count ? (double)rs_unkey<float>(lo) : 0.0;
                o[5] = count ? (double)rs_unkey<float>(hi) : 0.0;
            }
        } else if (lane == 0) {
            o[1] = v;
            o[3] = count ? sqrt(v / (double)count) : 0.0;
        }
    }
}

}  // namespace ts2d
