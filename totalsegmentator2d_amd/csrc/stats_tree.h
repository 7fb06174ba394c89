// The arithmetic of the per-label statistics (kernels_stats.h) that the statement, totalsegmentator2d_amd/statistics.py, fixes bit for bit: which
// samples belong to a label, the terms of the float64 sums and the ORDER in which they are added.  Its own header, host and device:
// tests/test_statistics_cpu.py compiles it into a stand-alone program and holds st_tree_label against the statement.
//
// The tree.  A label's samples are `rows` rows of W samples.  A term is the sample's value (first pass) or its squared deviation from the mean
// (second pass) where the sample belongs to the label, +0.0 where it does not.
//   level 1, per row    lane l of 64 adds the terms at x = l, l + 64, ... in increasing x, starting from +0.0; the 64 lane values are halved:
//                       v[l] + v[l + 32] for l < 32, then + 16, ... down to + 1.  v[0] is the row's partial.
//   level 2, per label  the row partials meet the same way: lane l adds the partials of rows l, l + 64, ..., then the halving.
// The shape is a function of (rows, W) alone, so neither the number of workgroups nor the order in which they finish shows in a bit.  A sum that
// starts at +0.0 never becomes -0.0 (x + -0.0 = x, +0.0 + -0.0 = +0.0), so adding +0.0 for a sample outside the label equals skipping it.
// Every product and sum is rounded on its own (contraction off): no fused multiply-add on either side.
//
// Minimum and maximum are taken on the order-preserving keys of ray_select.h (-0.0 < +0.0); a non-finite sample under a label is reported, the
// caller then computes nothing.
#pragma once
#include <stdint.h>
#include <string.h>

#include "ray_select.h"

namespace ts2d {

constexpr int kStLanes = 64;
enum { kStPlanes = 0, kStLabelMap = 1 };      // TS2D_STATS_PLANES, TS2D_STATS_LABELMAP

// does a segmentation sample belong to the label?  planes: the label's own plane > 0; label map: the sample equals the label's value
TS2D_RS_HD bool st_masked(uint8_t s, int kind, uint8_t value) { return kind == kStLabelMap ? s == value : s > 0; }

// the x of lane `lane` in a row of W samples: lane, lane + 64, ...; their number (no sum that could pass 2^31)
TS2D_RS_HD int st_lane_trips(int W, int lane) { return lane < W ? (W - 1 - lane) / kStLanes + 1 : 0; }

TS2D_RS_HD bool st_nonfinite(float v) {
    uint32_t u;
    memcpy(&u, &v, sizeof(u));
    return (u & 0x7F800000u) == 0x7F800000u;
}

// Level 1, first pass: lane `lane`'s sum over its samples of the row.  Also the smallest and largest key among its samples of the label
// (kmin from 0xFFFFFFFF, kmax from 0) and whether one of them is not finite.
TS2D_RS_HD double st_lane_sum(const uint8_t* m, int kind, uint8_t value, const float* x, int W, int lane, uint32_t* kmin, uint32_t* kmax,
                              int* bad) {
#pragma clang fp contract(off)
    double s = 0.0;
    uint32_t lo = *kmin, hi = *kmax;
    int b = *bad;
    const int trips = st_lane_trips(W, lane);
    for (int j = 0; j < trips; ++j) {
        const int i = lane + j * kStLanes;
        const bool in = st_masked(m[i], kind, value);
        const float v = x[i];
        const double t = in ? (double)v : 0.0;
        s = s + t;
        if (in) {
            const uint32_t key = rs_key(v);
            lo = key < lo ? key : lo;
            hi = key > hi ? key : hi;
            b |= st_nonfinite(v) ? 1 : 0;
        }
    }
    *kmin = lo; *kmax = hi; *bad = b;
    return s;
}

// Level 1, second pass: the squared deviations from `mean`, difference, product and sum each rounded on its own.
TS2D_RS_HD double st_lane_ssq(const uint8_t* m, int kind, uint8_t value, const float* x, int W, int lane, double mean) {
#pragma clang fp contract(off)
    double s = 0.0;
    const int trips = st_lane_trips(W, lane);
    for (int j = 0; j < trips; ++j) {
        const int i = lane + j * kStLanes;
        const double d = (double)x[i] - mean;
        const double dd = d * d;
        const double t = st_masked(m[i], kind, value) ? dd : 0.0;
        s = s + t;
    }
    return s;
}

// Level 2: lane `lane`'s sum over the row partials l, l + 64, ...
TS2D_RS_HD double st_lane_rows(const double* partial, int rows, int lane) {
#pragma clang fp contract(off)
    double s = 0.0;
    const int trips = st_lane_trips(rows, lane);
    for (int j = 0; j < trips; ++j) s = s + partial[lane + j * kStLanes];
    return s;
}

#if !defined(__HIP_DEVICE_COMPILE__)
// The halving of 64 lane values, spelled over an array (the kernels do it with cross-lane moves: st_wave_halve, kernels_stats.h).
inline double st_halve(double* v) {
    for (int n = kStLanes / 2; n >= 1; n >>= 1)
        for (int l = 0; l < n; ++l) v[l] = v[l] + v[l + n];
    return v[0];
}

// The whole tree of one label on the host: what stats_rows and stats_combine compute together.  second = 0: the sum (kmin, kmax, bad as
// st_lane_sum leaves them over all samples); second = 1: the sum of squared deviations from `mean`.  `partial`: rows doubles of scratch.
inline double st_tree_label(const uint8_t* m, int kind, uint8_t value, const float* x, int rows, int W, int second, double mean, double* partial,
                            uint32_t* kmin, uint32_t* kmax, int* bad) {
    double v[kStLanes];
    for (int r = 0; r < rows; ++r) {
        const uint8_t* mr = m + (size_t)r * W;
        const float* xr = x + (size_t)r * W;
        for (int l = 0; l < kStLanes; ++l)
            v[l] = second ? st_lane_ssq(mr, kind, value, xr, W, l, mean) : st_lane_sum(mr, kind, value, xr, W, l, kmin, kmax, bad);
        partial[r] = st_halve(v);
    }
    for (int l = 0; l < kStLanes; ++l) v[l] = st_lane_rows(partial, rows, l);
    return st_halve(v);
}
#endif

}  // namespace ts2d
