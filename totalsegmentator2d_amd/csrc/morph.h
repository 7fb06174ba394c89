// The arithmetic of the label morphology (kernels_morph.h, behind ts2d_label_morphology) that the statement, totalsegmentator2d_amd/morphology.py,
// fixes byte for byte: grow, shrink, open and close a mask by a radius in the unit of the spacing, with an exact Euclidean disc.  Its own header,
// host and device: tests/test_morphology_cpu.py compiles it into a stand-alone program (tests/morph_driver.cpp) and holds its ONE host walk,
// mo_label, against the statement.
//
// The disc.  r2 = r * r in float64, one rounding.  Offset (dy, dx) belongs to the disc iff sd_candidate(|dy|, |dx|, sy, sx) <= r2 (surface_dist.h:
// (|dy| * sy)^2 + (|dx| * sx)^2, every operation rounded on its own); a pixel exactly on the circle belongs.
//   dilate   D(M) = the pixels p inside the image with some q in M and p - q in the disc
//   erode    E(M) = ~D(~M), the complement taken INSIDE the image: outside the image is neither background nor foreground, so a mask that touches
//            an edge is not eaten from that edge
//   open     D(E(M));  close  E(D(M))
//
// The table.  sd_candidate is monotone in both integers, bits included (surface_dist.h argues that), so per row offset n the admitted column
// offsets are 0 ... cover[n], and cover is not increasing in n: cover[n] = the largest dx in [0, W - 1] with sd_candidate(n, dx) <= r2, for
// n = 0, 1, ... up to the first n that admits no dx, or H.  cover[0] exists (0 <= r2), so the table has 1 ... H entries.  It carries everything the
// float64 comparison decides: behind it no step holds a floating-point number.
//
// The scan form.  g(y, x') = the row distance from y to the nearest pixel of M in column x' (pass 1 of surface_dist.h over foreground), capped at
// the table's length T, which also stands for "no pixel in the column".  Column x' covers, in row y, the interval [x' - c, x' + c] with
// c = cover[g] (nothing where g >= T): among the column's pixels the nearest row admits the widest interval.  So
//     D(M)(y, x)  iff  max over x' <= x of (x' + c) >= x   or   min over x' >= x of (x' - c) <= x,
// one prefix maximum and one suffix minimum along the row.  A row is walked in chunks of 64 pixels, the running value carried from chunk to chunk;
// inside a chunk the 64 values meet in six doubling steps (kernels: cross-lane moves; host: mo_chunk_prefix_max / mo_chunk_suffix_min spell the
// same steps over an array).  Maximum and minimum of integers: whatever the order, the same number.
#pragma once
#include "surface_dist.h"

namespace ts2d {

enum { kMoDilate = 0, kMoErode = 1, kMoOpen = 2, kMoClose = 3 };      // TS2D_MORPH_DILATE ... TS2D_MORPH_CLOSE
constexpr int kMoCounters = 4;                  // TS2D_MORPH_COUNTERS: pixels before, after, added, removed
constexpr int kMoMaxExtent = kSdMaxExtent;      // g, the table's length and a cover are uint16; x + cover stays far below 2^31
constexpr int kMoNoReach = -1;                  // the right end of a column that covers nothing: left of every pixel
constexpr int kMoFar = 0x7FFFFFFF;              // ... and its left end: right of every pixel

// the two steps of an operation: is step s (0, 1) taken on the complement (an erosion)?  dilate and erode have one step
TS2D_SD_HD int mo_steps(int op) { return op == kMoOpen || op == kMoClose ? 2 : 1; }
TS2D_SD_HD bool mo_step_erodes(int op, int s) { return op == kMoErode || (op == kMoOpen && s == 0) || (op == kMoClose && s == 1); }
TS2D_SD_HD bool mo_grows(int op) { return op == kMoDilate || op == kMoClose; }

// does a sample belong to the set a step dilates?  the label's mask (st_masked), or its complement for an erosion
TS2D_SD_HD bool mo_member(uint8_t s, int kind, uint8_t value, bool complement) { return st_masked(s, kind, value) != complement; }

// g of a pixel whose nearest member of the column is d rows away (none: d < 0)
TS2D_SD_HD uint16_t mo_g(int d, int T) { return (uint16_t)(d < 0 || d > T ? T : d); }

// the ends of the interval column x covers where its row distance is g
TS2D_SD_HD int mo_reach_right(const uint16_t* cover, int T, int g, int x) { return g < T ? x + (int)cover[g] : kMoNoReach; }
TS2D_SD_HD int mo_reach_left(const uint16_t* cover, int T, int g, int x) { return g < T ? x - (int)cover[g] : kMoFar; }

// the byte of a plane's pixel after an operation: a pixel that stays set keeps its byte, a new one becomes 1, a cleared one 0
TS2D_SD_HD uint8_t mo_plane_byte(uint8_t before, bool after) { return after ? (before ? before : (uint8_t)1) : (uint8_t)0; }

#if !defined(__HIP_DEVICE_COMPILE__)
// The table: cover[0 ... T - 1] (room for H entries), T returned.  radius >= 0, spacings > 0, all finite: the entry checks that.
inline int mo_cover_table(double radius, double sy, double sx, int H, int W, uint16_t* cover) {
#pragma clang fp contract(off)
    const double r2 = radius * radius;
    int dx = W - 1, T = 0;
    for (int n = 0; n < H; ++n) {                       // cover does not grow with n: dx only walks down, H + W steps in all
        while (dx >= 0 && !(sd_candidate((uint16_t)n, dx, sy, sx) <= r2)) --dx;
        if (dx < 0) break;
        cover[T++] = (uint16_t)dx;
    }
    return T;
}

// Pass 1 of one column on the host: g[y * W + x] for every y, over the members of the column.
inline void mo_column(const uint8_t* src, int kind, uint8_t value, bool complement, int H, int W, int x, int T, uint16_t* g) {
    int last = -1;
    for (int y = 0; y < H; ++y) {
        if (mo_member(src[(size_t)y * W + x], kind, value, complement)) last = y;
        g[(size_t)y * W + x] = mo_g(last < 0 ? -1 : y - last, T);
    }
    last = -1;
    for (int y = H - 1; y >= 0; --y) {
        if (mo_member(src[(size_t)y * W + x], kind, value, complement)) last = y;
        const uint16_t d = mo_g(last < 0 ? -1 : last - y, T);
        if (d < g[(size_t)y * W + x]) g[(size_t)y * W + x] = d;
    }
}

// The six doubling steps of a chunk, spelled over an array (the kernels: mo_wave_prefix_max, mo_wave_suffix_min).
inline void mo_chunk_prefix_max(int* v) {
    for (int d = 1; d < kStLanes; d <<= 1)
        for (int l = kStLanes - 1; l >= d; --l) v[l] = v[l - d] > v[l] ? v[l - d] : v[l];
}
inline void mo_chunk_suffix_min(int* v) {
    for (int d = 1; d < kStLanes; d <<= 1)
        for (int l = 0; l + d < kStLanes; ++l) v[l] = v[l + d] < v[l] ? v[l + d] : v[l];
}

// Pass 2 of one row on the host: dst[x] = 1 where the row's pixel is covered (erodes: where it is NOT), else 0.
inline void mo_row(const uint16_t* g, int W, const uint16_t* cover, int T, bool erodes, uint8_t* dst) {
    const int chunks = (W + kStLanes - 1) / kStLanes;
    int v[kStLanes];
    int carry = kMoNoReach;
    for (int c = 0; c < chunks; ++c) {
        for (int l = 0; l < kStLanes; ++l) {
            const int x = c * kStLanes + l;
            v[l] = x < W ? mo_reach_right(cover, T, g[x], x) : kMoNoReach;
        }
        mo_chunk_prefix_max(v);
        for (int l = 0; l < kStLanes; ++l) v[l] = v[l] > carry ? v[l] : carry;
        carry = v[kStLanes - 1];
        for (int l = 0; l < kStLanes && c * kStLanes + l < W; ++l) dst[c * kStLanes + l] = v[l] >= c * kStLanes + l ? 1 : 0;
    }
    carry = kMoFar;
    for (int c = chunks - 1; c >= 0; --c) {
        for (int l = 0; l < kStLanes; ++l) {
            const int x = c * kStLanes + l;
            v[l] = x < W ? mo_reach_left(cover, T, g[x], x) : kMoFar;
        }
        mo_chunk_suffix_min(v);
        for (int l = 0; l < kStLanes; ++l) v[l] = v[l] < carry ? v[l] : carry;
        carry = v[0];
        for (int l = 0; l < kStLanes && c * kStLanes + l < W; ++l) {
            const int x = c * kStLanes + l;
            const bool covered = dst[x] != 0 || v[l] <= x;
            dst[x] = covered != erodes ? 1 : 0;
        }
    }
}

// One label on the host, what mo_columns and mo_rows compute together: res[H * W] = 1 where the operation leaves the pixel set, else 0.
// g: H * W of scratch; mid: H * W bytes of scratch (open and close; else unused).
inline void mo_label(const uint8_t* seg, int kind, uint8_t value, int H, int W, int op, const uint16_t* cover, int T, uint16_t* g, uint8_t* mid,
                     uint8_t* res) {
    const int steps = mo_steps(op);
    for (int s = 0; s < steps; ++s) {
        const uint8_t* src = s == 0 ? seg : mid;
        const int src_kind = s == 0 ? kind : (int)kStPlanes;
        uint8_t* dst = s + 1 == steps ? res : mid;
        const bool erodes = mo_step_erodes(op, s);
        for (int x = 0; x < W; ++x) mo_column(src, src_kind, value, erodes, H, W, x, T, g);
        for (int y = 0; y < H; ++y) mo_row(g + (size_t)y * W, W, cover, T, erodes, dst + (size_t)y * W);
    }
}
#endif

}  // namespace ts2d
