// The arithmetic of the boundary distances (kernels_evaluate.h) that the statement, totalsegmentator2d_amd/evaluate.py, fixes bit for bit: which
// samples belong to a label, which of them are border pixels, and the squared distance of a border pixel of one mask to the border of the other.
// Its own header, host and device: tests/test_evaluate_cpu.py compiles it into a stand-alone program and holds sd_label against the statement.
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
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define TS2D_SD_HD __host__ __device__ __forceinline__
#else
#define TS2D_SD_HD inline
#endif

namespace ts2d {

enum { kSdPlanes = 0, kSdLabelMap = 1 };      // TS2D_STATS_PLANES, TS2D_STATS_LABELMAP
constexpr uint16_t kSdNone = 0xFFFFu;          // g of a column without a border pixel (H <= kSdMaxExtent keeps every real g below it)
constexpr int kSdMaxExtent = 32767;
constexpr int kSdMaxTolerances = 8;            // TS2D_EVAL_MAX_TOLERANCES

// does a segmentation sample belong to the label?  planes: the label's own plane > 0; label map: the sample equals the label's value
TS2D_SD_HD bool sd_masked(uint8_t s, int kind, uint8_t value) { return kind == kSdLabelMap ? s == value : s > 0; }

// is (y, x) a border pixel of the label's mask m [H][W]?
TS2D_SD_HD bool sd_border(const uint8_t* m, int kind, uint8_t value, int H, int W, int y, int x) {
    if (!sd_masked(m[(long long)y * W + x], kind, value)) return false;
    const bool up = y > 0 && sd_masked(m[(long long)(y - 1) * W + x], kind, value);
    const bool down = y + 1 < H && sd_masked(m[(long long)(y + 1) * W + x], kind, value);
    const bool left = x > 0 && sd_masked(m[(long long)y * W + x - 1], kind, value);
    const bool right = x + 1 < W && sd_masked(m[(long long)y * W + x + 1], kind, value);
    return !(up && down && left && right);
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

// d2 >= +0.0 or +inf: the bit pattern of such a float64, read as an unsigned integer, orders as the values do
TS2D_SD_HD uint64_t sd_key(double d2) {
    uint64_t u;
    memcpy(&u, &d2, sizeof(u));
    return u;
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

// One label and one direction on the host, what the kernels compute together: the border count of `own`, the largest d2 as a key (0 for an empty
// border: the caller reports -inf) and per tolerance the border pixels with d2 <= tol_sq[t].  border_own, border_other: H * W bytes of scratch
// each; g: H * W.
inline long long sd_label(const uint8_t* own, int kind_own, const uint8_t* other, int kind_other, uint8_t value, int H, int W, double sy, double sx,
                          const double* tol_sq, int T, uint8_t* border_own, uint8_t* border_other, uint16_t* g, uint64_t* key_max, long long* within) {
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            border_own[(size_t)y * W + x] = sd_border(own, kind_own, value, H, W, y, x) ? 1 : 0;
            border_other[(size_t)y * W + x] = sd_border(other, kind_other, value, H, W, y, x) ? 1 : 0;
        }
    for (int x = 0; x < W; ++x) sd_column(border_other, H, W, x, g);
    long long n = 0;
    *key_max = 0;
    for (int t = 0; t < T; ++t) within[t] = 0;
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            if (!border_own[(size_t)y * W + x]) continue;
            double d2 = sd_inf();
            for (int xo = 0; xo < W; ++xo) {
                const double c = sd_candidate(g[(size_t)y * W + xo], xo > x ? xo - x : x - xo, sy, sx);
                d2 = c < d2 ? c : d2;
            }
            ++n;
            const uint64_t key = sd_key(d2);
            *key_max = key > *key_max ? key : *key_max;
            for (int t = 0; t < T; ++t) within[t] += d2 <= tol_sq[t] ? 1 : 0;
        }
    return n;
}
#endif

}  // namespace ts2d
