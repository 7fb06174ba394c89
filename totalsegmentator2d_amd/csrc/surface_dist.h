// The arithmetic of the boundary distances and their profile (kernels_evaluate.h, kernels_evaluate_profile.h) that the statements of
// totalsegmentator2d_amd/evaluate.py fix bit for bit: which samples are border pixels, the squared distance of a border pixel of one mask to the
// border of the other, and the sum and the order statistics of those distances.  Its own header, host and device: tests/test_evaluate_cpu.py and
// tests/test_evaluate_profile_cpu.py compile it into stand-alone programs and hold its ONE host walk, sd_label_profile (sd_label: the call of it
// without the profile), against the statements.
//
// Border.  A border pixel of a mask is a foreground pixel with at least one of its four neighbours background; outside the image is background.
//
// Distance.  For a border pixel p of A,
//     d2(p) = min over border pixels q of B of ((|py - qy| * sy) * (|py - qy| * sy) + (|px - qx| * sx) * (|px - qx| * sx))
// in float64, both products of a term and the sum each rounded on their own (contraction off), +inf where B has no border.
//
// The two passes and why they are exact.  Write f(n, s) = (n * s) * (n * s) for an integer n >= 0 and a spacing s > 0, with its two roundings.
//   - n -> n * s is monotone (rounding to nearest is monotone and n * s grows with n), and r -> r * r is monotone for r >= 0 for the same reason:
//     f(n, s) <= f(n + 1, s), bits included.
//   - u -> u + v with one rounding is monotone in u for a fixed v.
// Fix a column x' of B.  Among its border pixels (y', x') the term of the column offset, f(|px - x'|, sx), is the same, and the term of the row
// offset is monotone in |py - y'|: the candidate of the NEAREST row, |py - y'| = g(py, x'), is the smallest of the column (or ties with it).  So
//     d2(p) = min over x' with a border pixel of f(g(py, x'), sy) + f(|px - x'|, sx),
// the same set minimum over fewer candidates: equal bit for bit to the brute force, and independent of the order in which the columns are met.
//   pass 1, per column    g(y, x') = min |y - y'| over the border rows y' of column x': a downward scan (nearest at or above) and an upward
//                         scan (nearest at or below); kSdNone where the column has no border pixel
//   pass 2, per border pixel of the row    the minimum over x' of sd_candidate(g(py, x'), |px - x'|)
//
// The distance profile (ts2d_surface_distance_profile; the statement: evaluate.distance_profile_statement) keeps every border pixel's d2.
//   Sum.  The term of pixel (y, x) is sd_sqrt(d2) where it is a border pixel of the direction's own side, +0.0 elsewhere, and the terms meet in
//   the tree of stats_tree.h over (H, W): per row lane l of 64 adds the terms at x = l, l + 64, ... in increasing x from +0.0, the lanes are
//   halved, and the row partials meet the same way.  No term is negative, so an infinite term makes the sum +inf and never a NaN.
//   Order statistics.  The root is monotone, so the distance at sorted position r is the root of the d2 at sorted position r, and d2 >= +0.0 orders
//   as its key (sd_key) does.  The key at position r is built from its top digit down, eight rounds of eight bits (rs_decide of ray_select.h
//   generalised to a digit): with the digits above decided (`prefix`), a round counts per digit value the candidates - the keys that agree with
//   the prefix on those digits -; the digit is the first whose running count passes r, and the count below it is taken off r.  Integers only.
//   Ranks.  For percentile q among n >= 1 sorted values: h = (n - 1) * (q / 100), i = min(floor(h), n - 1), j = min(i + 1, n - 1), t = h - i, each
//   operation an IEEE float64 one (sd_percentile_ranks); the caller interpolates between the roots of the two selected d2.
//
// VOLUMES (ts2d_volume_surface_distances, kernels_evaluate_volume.h; the statements: evaluate.volume_surface_statement and
// evaluate.volume_distance_profile_statement; the host walk: sd_volume_label_profile, held against them by tests/test_evaluate_volume_cpu.py).
// Border (sd_border3).  A border voxel of a mask [Z][H][W] is a foreground voxel with at least one of its SIX face neighbours background; outside
// the volume is background.  (With Z = 1 every foreground voxel is one: that is this definition, not the 2-D border.)
// Distance.  For a border voxel p of A,
//     d2(p) = min over border voxels q of B of ((f(|pz - qz|, sz) + f(|py - qy|, sy)) + f(|px - qx|, sx))
// in float64, that association, every operation rounded on its own, +inf where B has no border.
// The three passes and why they are exact.  f(n, s) is monotone in n and u -> fl(u + v) is monotone in u (above).
//   pass 1, per line (y', x') along z    the integer g(z, y', x') = min |z - z'| over the border voxels of the line (two scans), or kSdNone
//   pass 2, per (z, y, x')               h(z, y, x') = min over y' of (f(g(z, y', x'), sz) + f(|y - y'|, sy)), +inf without a candidate
//   pass 3, per border voxel p of A      d2(p) = min over x' of (h(pz, py, x') + f(|px - x'|, sx))      (sd_candidate_h)
// Fix a line (y', x') of B.  Its candidates for p differ in the z term alone, f(|pz - z'|, sz), and (u + f(dy)) + f(dx) is monotone in u by two
// applications of the second fact: the line's NEAREST voxel gives its smallest candidate.  Fix x'.  The candidates of its lines are
// u(y') + f(|px - x'|, sx) with u(y') = f(g, sz) + f(|py - y'|, sy), monotone in u: the smallest u - that is h - gives the smallest candidate,
// so the minimum over y' commutes with adding the x term.  The three passes therefore take the same set minimum over fewer candidates: equal
// to the brute force over all border pairs bit for bit, whatever the order in which lines and columns are met.
// The sum of a volume's profile meets in the tree of stats_tree.h over (Z * H, W): row z * H + y, lane x % 64.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "stats_tree.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define TS2D_SD_HD __host__ __device__ __forceinline__
#else
#define TS2D_SD_HD inline
#endif

namespace ts2d {

constexpr uint16_t kSdNone = 0xFFFFu;          // g of a column without a border pixel (H <= kSdMaxExtent keeps every real g below it)
constexpr int kSdMaxExtent = 32767;
constexpr int kSdMaxTolerances = 8;            // TS2D_EVAL_MAX_TOLERANCES
constexpr int kSdMaxPercentiles = 8;           // TS2D_EVAL_MAX_PERCENTILES
constexpr int kSdMaxRanks = 2 * kSdMaxPercentiles;      // a percentile selects two sorted positions
constexpr uint64_t kSdNoKey = ~0ull;           // in a key buffer: not a border pixel (the bits of a NaN: no d2 has them)
constexpr int kSdRounds = 8, kSdDigits = 256;  // a 64-bit key in 8-bit digits, the top one first

// is (y, x) a border pixel of the label's mask m [H][W]?  (the kinds and st_masked, who belongs to the label: stats_tree.h)
TS2D_SD_HD bool sd_border(const uint8_t* m, int kind, uint8_t value, int H, int W, int y, int x) {
    if (!st_masked(m[(long long)y * W + x], kind, value)) return false;
    const bool up = y > 0 && st_masked(m[(long long)(y - 1) * W + x], kind, value);
    const bool down = y + 1 < H && st_masked(m[(long long)(y + 1) * W + x], kind, value);
    const bool left = x > 0 && st_masked(m[(long long)y * W + x - 1], kind, value);
    const bool right = x + 1 < W && st_masked(m[(long long)y * W + x + 1], kind, value);
    return !(up && down && left && right);
}

// is (z, y, x) a border voxel of the label's mask m [Z][H][W]?  (six face neighbours)
TS2D_SD_HD bool sd_border3(const uint8_t* m, int kind, uint8_t value, int Z, int H, int W, int z, int y, int x) {
    const long long HW = (long long)H * W, i = (long long)z * HW + (long long)y * W + x;
    if (!st_masked(m[i], kind, value)) return false;
    const bool before = z > 0 && st_masked(m[i - HW], kind, value);
    const bool after = z + 1 < Z && st_masked(m[i + HW], kind, value);
    const bool up = y > 0 && st_masked(m[i - W], kind, value);
    const bool down = y + 1 < H && st_masked(m[i + W], kind, value);
    const bool left = x > 0 && st_masked(m[i - 1], kind, value);
    const bool right = x + 1 < W && st_masked(m[i + 1], kind, value);
    return !(before && after && up && down && left && right);
}

TS2D_SD_HD double sd_inf() {
    const uint64_t u = 0x7FF0000000000000ull;
    double d;
    memcpy(&d, &u, sizeof(d));
    return d;
}

// the candidate of column x' for a border pixel: row distance g (kSdNone: no border in the column), column distance dx
TS2D_SD_HD double sd_candidate(uint16_t g, int dx, double sy, double sx) {
#pragma clang fp contract(off)
    if (g == kSdNone) return sd_inf();
    const double ry = (double)(int)g * sy;
    const double ry2 = ry * ry;
    const double rx = (double)dx * sx;
    const double rx2 = rx * rx;
    return ry2 + rx2;
}

// f(n, s) = (n * s) * (n * s), its two roundings
TS2D_SD_HD double sd_f(int n, double s) {
#pragma clang fp contract(off)
    const double r = (double)n * s;
    return r * r;
}

// volumes, pass 2: the candidate of line (y', x') for the voxels of row y at its z - line distance g (kSdNone: no border on the line)
TS2D_SD_HD double sd_candidate_line(uint16_t g, int dy, double sz, double sy) {
#pragma clang fp contract(off)
    if (g == kSdNone) return sd_inf();
    const double a = sd_f((int)g, sz);
    const double b = sd_f(dy, sy);
    return a + b;
}

// volumes, pass 3: the candidate of column x' for a border voxel - h of the column at the voxel's (z, y) (+inf: no candidate), column distance dx
TS2D_SD_HD double sd_candidate_h(double h, int dx, double sx) {
#pragma clang fp contract(off)
    const double c = sd_f(dx, sx);
    return h + c;
}

// d2 >= +0.0 or +inf: the bit pattern of such a float64, read as an unsigned integer, orders as the values do
TS2D_SD_HD uint64_t sd_key(double d2) {
    uint64_t u;
    memcpy(&u, &d2, sizeof(u));
    return u;
}

TS2D_SD_HD double sd_unkey(uint64_t key) {
    double d;
    memcpy(&d, &key, sizeof(d));
    return d;
}

// the distance of a d2: the correctly rounded root, np.sqrt's bits (IEEE on the host; the device's double sqrt is correctly rounded without
// fast-math, and tests/test_gpu_evaluate_profile.py holds it against np.sqrt on the values the distances take)
TS2D_SD_HD double sd_sqrt(double d2) { return sqrt(d2); }

// the sorted positions i <= j and the weight t of percentile q (0 ... 100) among n >= 1 values
TS2D_SD_HD void sd_percentile_ranks(long long n, double q, long long* i, long long* j, double* t) {
#pragma clang fp contract(off)
    const double f = q / 100.0;
    const double h = (double)(n - 1) * f;
    long long lo = (long long)floor(h);
    lo = lo < n - 1 ? lo : n - 1;
    *i = lo;
    *j = lo + 1 < n - 1 ? lo + 1 : n - 1;
    *t = h - (double)lo;
}

// round rnd (0 ... 7) looks at the bits [shift, shift + 8) of a key
TS2D_SD_HD int sd_round_shift(int rnd) { return 8 * (kSdRounds - 1 - rnd); }
// does a key agree with the prefix on the digits decided before round rnd?
TS2D_SD_HD bool sd_digit_candidate(uint64_t key, uint64_t prefix, int rnd) {
    return rnd == 0 || (key >> (sd_round_shift(rnd) + 8)) == (prefix >> (sd_round_shift(rnd) + 8));
}
TS2D_SD_HD int sd_digit(uint64_t key, int rnd) { return (int)((key >> sd_round_shift(rnd)) & 0xFFu); }

// One decision over FOUR adjacent digit values d0 ... d0 + 3 with c[] candidates each, `below` candidates under d0: where sorted position *rank
// falls among them, the digit goes into the prefix, the candidates under it come off the rank, and the result is true.
TS2D_SD_HD bool sd_decide_quad(const uint32_t* c, int d0, long long below, int rnd, long long* rank, uint64_t* prefix) {
    long long r = *rank - below;
    if (r < 0) return false;
    for (int j = 0; j < 4; ++j) {
        if (r < (long long)c[j]) {
            *rank = r;
            *prefix |= (uint64_t)(d0 + j) << sd_round_shift(rnd);
            return true;
        }
        r -= (long long)c[j];
    }
    return false;
}

#if !defined(__HIP_DEVICE_COMPILE__)
// Pass 1 of one column on the host: g[y * W + x] for y = 0 ... H - 1 from the border bytes of the column.
inline void sd_column(const uint8_t* border, int H, int W, int x, uint16_t* g) {
    int last = -1;
    for (int y = 0; y < H; ++y) {
        if (border[(size_t)y * W + x]) last = y;
        g[(size_t)y * W + x] = last < 0 ? kSdNone : (uint16_t)(y - last);
    }
    last = -1;
    for (int y = H - 1; y >= 0; --y) {
        if (border[(size_t)y * W + x]) last = y;
        if (last >= 0 && (uint16_t)(last - y) < g[(size_t)y * W + x]) g[(size_t)y * W + x] = (uint16_t)(last - y);
    }
}

// The key at sorted position rank (0 <= rank < the number of keys other than kSdNoKey) of keys[0 ... n - 1]: what sd_select_hist and
// sd_select_decide compute together.
inline uint64_t sd_select_rank(const uint64_t* keys, size_t n, long long rank) {
    uint64_t prefix = 0;
    for (int rnd = 0; rnd < kSdRounds; ++rnd) {
        uint32_t bins[kSdDigits] = {0};
        for (size_t i = 0; i < n; ++i)
            if (keys[i] != kSdNoKey && sd_digit_candidate(keys[i], prefix, rnd)) ++bins[sd_digit(keys[i], rnd)];
        long long below = 0;
        for (int d0 = 0; d0 < kSdDigits; d0 += 4) {
            if (sd_decide_quad(bins + d0, d0, below, rnd, &rank, &prefix)) break;
            below += (long long)bins[d0] + bins[d0 + 1] + bins[d0 + 2] + bins[d0 + 3];
        }
    }
    return prefix;
}

// One label and one direction on the host, what sd_columns, sd_rows, sd_profile_combine and the selection kernels compute together: the border
// count of `own`, the largest d2 as a key (0 for an empty border: the caller reports -inf), per tolerance the border pixels with d2 <= tol_sq[t];
// with `partial` (H of scratch; else null) the sum of the distances in the tree over (H, W), +0.0 for an empty border; with `keys` (H * W of
// scratch; else null, and P = 0) per percentile q[p] the keys at the two sorted positions (rank_keys [P][2]) and the weight (weights [P]), which
// an empty border leaves alone.  border_own, border_other: H * W bytes of scratch each; g: H * W.
inline long long sd_label_profile(const uint8_t* own, int kind_own, const uint8_t* other, int kind_other, uint8_t value, int H, int W, double sy,
                                  double sx, const double* tol_sq, int T, const double* q, int P, uint8_t* border_own, uint8_t* border_other,
                                  uint16_t* g, uint64_t* keys, double* partial, uint64_t* key_max, long long* within, double* dist_sum,
                                  uint64_t* rank_keys, double* weights) {
#pragma clang fp contract(off)
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            border_own[(size_t)y * W + x] = sd_border(own, kind_own, value, H, W, y, x) ? 1 : 0;
            border_other[(size_t)y * W + x] = sd_border(other, kind_other, value, H, W, y, x) ? 1 : 0;
        }
    for (int x = 0; x < W; ++x) sd_column(border_other, H, W, x, g);
    long long n = 0;
    *key_max = 0;
    for (int t = 0; t < T; ++t) within[t] = 0;
    double v[kStLanes];
    for (int y = 0; y < H; ++y) {
        for (int l = 0; l < kStLanes; ++l) v[l] = 0.0;
        for (int x = 0; x < W; ++x) {
            if (keys) keys[(size_t)y * W + x] = kSdNoKey;
            if (!border_own[(size_t)y * W + x]) continue;
            double d2 = sd_inf();
            for (int xo = 0; xo < W; ++xo) {
                const double c = sd_candidate(g[(size_t)y * W + xo], xo > x ? xo - x : x - xo, sy, sx);
                d2 = c < d2 ? c : d2;
            }
            ++n;
            const uint64_t key = sd_key(d2);
            if (keys) keys[(size_t)y * W + x] = key;
            *key_max = key > *key_max ? key : *key_max;
            for (int t = 0; t < T; ++t) within[t] += d2 <= tol_sq[t] ? 1 : 0;
            if (partial) v[x % kStLanes] = v[x % kStLanes] + sd_sqrt(d2);          // increasing x: lane x % 64 meets its terms in order
        }
        if (partial) partial[y] = st_halve(v);
    }
    if (partial) {
        for (int l = 0; l < kStLanes; ++l) v[l] = st_lane_rows(partial, H, l);
        *dist_sum = st_halve(v);
    }
    for (int p = 0; p < P && n > 0; ++p) {
        long long i, j;
        sd_percentile_ranks(n, q[p], &i, &j, weights + p);
        rank_keys[2 * p] = sd_select_rank(keys, (size_t)H * W, i);
        rank_keys[2 * p + 1] = sd_select_rank(keys, (size_t)H * W, j);
    }
    return n;
}

// ... without the profile: what ts2d_surface_distances reports
inline long long sd_label(const uint8_t* own, int kind_own, const uint8_t* other, int kind_other, uint8_t value, int H, int W, double sy, double sx,
                          const double* tol_sq, int T, uint8_t* border_own, uint8_t* border_other, uint16_t* g, uint64_t* key_max, long long* within) {
    return sd_label_profile(own, kind_own, other, kind_other, value, H, W, sy, sx, tol_sq, T, nullptr, 0, border_own, border_other, g, nullptr, nullptr,
                            key_max, within, nullptr, nullptr, nullptr);
}
// Pass 1 of one line (y, x) along z on the host: g[z * H * W + i] for z = 0 ... Z - 1 from the border bytes of the line (i = y * W + x).
inline void sd_line(const uint8_t* border, int Z, size_t HW, size_t i, uint16_t* g) {
    int last = -1;
    for (int z = 0; z < Z; ++z) {
        if (border[(size_t)z * HW + i]) last = z;
        g[(size_t)z * HW + i] = last < 0 ? kSdNone : (uint16_t)(z - last);
    }
    last = -1;
    for (int z = Z - 1; z >= 0; --z) {
        if (border[(size_t)z * HW + i]) last = z;
        if (last >= 0 && (uint16_t)(last - z) < g[(size_t)z * HW + i]) g[(size_t)z * HW + i] = (uint16_t)(last - z);
    }
}

// One label and one direction of a VOLUME on the host, what sdv_lines, sdv_planes, sdv_rows, sdv_profile_combine and the selection kernels
// compute together (they inside the label's box, this over the whole extent: outside the box everything is background).  The results and the
// optional parts as sd_label_profile has them; the tree of the sum is over (Z * H, W).  border_own, border_other: Z * H * W bytes of scratch
// each; g: Z * H * W; h: Z * H * W; keys: Z * H * W or null; partial: Z * H or null.
inline long long sd_volume_label_profile(const uint8_t* own, int kind_own, const uint8_t* other, int kind_other, uint8_t value, int Z, int H, int W,
                                         double sz, double sy, double sx, const double* tol_sq, int T, const double* q, int P, uint8_t* border_own,
                                         uint8_t* border_other, uint16_t* g, double* h, uint64_t* keys, double* partial, uint64_t* key_max,
                                         long long* within, double* dist_sum, uint64_t* rank_keys, double* weights) {
#pragma clang fp contract(off)
    const size_t HW = (size_t)H * W, n_all = (size_t)Z * HW;
    for (int z = 0; z < Z; ++z)
        for (int y = 0; y < H; ++y)
            for (int x = 0; x < W; ++x) {
                const size_t i = (size_t)z * HW + (size_t)y * W + x;
                border_own[i] = sd_border3(own, kind_own, value, Z, H, W, z, y, x) ? 1 : 0;
                border_other[i] = sd_border3(other, kind_other, value, Z, H, W, z, y, x) ? 1 : 0;
            }
    for (size_t i = 0; i < HW; ++i) sd_line(border_other, Z, HW, i, g);
    for (int z = 0; z < Z; ++z)
        for (int y = 0; y < H; ++y)
            for (int x = 0; x < W; ++x) {
                double best = sd_inf();
                for (int yo = 0; yo < H; ++yo) {
                    const double c = sd_candidate_line(g[(size_t)z * HW + (size_t)yo * W + x], yo > y ? yo - y : y - yo, sz, sy);
                    best = c < best ? c : best;
                }
                h[(size_t)z * HW + (size_t)y * W + x] = best;
            }
    long long n = 0;
    *key_max = 0;
    for (int t = 0; t < T; ++t) within[t] = 0;
    double v[kStLanes];
    for (size_t r = 0; r < (size_t)Z * H; ++r) {                    // row r = z * H + y
        for (int l = 0; l < kStLanes; ++l) v[l] = 0.0;
        for (int x = 0; x < W; ++x) {
            if (keys) keys[r * W + x] = kSdNoKey;
            if (!border_own[r * W + x]) continue;
            double d2 = sd_inf();
            for (int xo = 0; xo < W; ++xo) {
                const double c = sd_candidate_h(h[r * W + xo], xo > x ? xo - x : x - xo, sx);
                d2 = c < d2 ? c : d2;
            }
            ++n;
            const uint64_t key = sd_key(d2);
            if (keys) keys[r * W + x] = key;
            *key_max = key > *key_max ? key : *key_max;
            for (int t = 0; t < T; ++t) within[t] += d2 <= tol_sq[t] ? 1 : 0;
            if (partial) v[x % kStLanes] = v[x % kStLanes] + sd_sqrt(d2);
        }
        if (partial) partial[r] = st_halve(v);
    }
    if (partial) {
        for (int l = 0; l < kStLanes; ++l) v[l] = st_lane_rows(partial, Z * H, l);
        *dist_sum = st_halve(v);
    }
    for (int p = 0; p < P && n > 0; ++p) {
        long long i, j;
        sd_percentile_ranks(n, q[p], &i, &j, weights + p);
        rank_keys[2 * p] = sd_select_rank(keys, n_all, i);
        rank_keys[2 * p + 1] = sd_select_rank(keys, n_all, j);
    }
    return n;
}

// ... without the profile: the plain form of ts2d_volume_surface_distances
inline long long sd_volume_label(const uint8_t* own, int kind_own, const uint8_t* other, int kind_other, uint8_t value, int Z, int H, int W, double sz,
                                 double sy, double sx, const double* tol_sq, int T, uint8_t* border_own, uint8_t* border_other, uint16_t* g, double* h,
                                 uint64_t* key_max, long long* within) {
    return sd_volume_label_profile(own, kind_own, other, kind_other, value, Z, H, W, sz, sy, sx, tol_sq, T, nullptr, 0, border_own, border_other, g, h,
                                   nullptr, nullptr, key_max, within, nullptr, nullptr, nullptr);
}
#endif

}  // namespace ts2d
