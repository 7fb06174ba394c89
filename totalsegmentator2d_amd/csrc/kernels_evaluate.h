// Scoring a segmentation against a reference, behind ts2d_project_labels_coronal, ts2d_label_overlap and the two passes of the boundary
// distances of ts2d_surface_distances and ts2d_surface_distance_profile (what the profile adds behind them: kernels_evaluate_profile.h).  The
// statements are totalsegmentator2d_amd.evaluate.project_labels, overlap_statement, surface_statement and distance_profile_statement;
// tests/test_gpu_evaluate.py and tests/test_gpu_evaluate_profile.py hold these kernels against them byte for byte and bit for bit, the float64
// bits of the largest squared distance included.
//
//   project_labels_stream  the reference's project(..., 'multiclass:<num>') along the coronal axis (ts2d/core/util/image.py:164-194) in ONE pass
//                          over the volume whatever num is.  The volume is addressed as project_modes_stream (kernels_project_modes.h) addresses
//                          it - signed element strides and the base of the reoriented view, output pixels (z, x) in flat order over the lanes - so
//                          no reorientation copy is made and the loads of a wave coalesce as they do there.  A lane takes FOUR adjacent output
//                          pixels and keeps per pixel a num-bit set in NW = ceil(num / 32) registers (the word is chosen by a static loop over
//                          the words: no dynamically indexed private array).  Then plane k gets bit k of the four sets as one 4-byte store where
//                          nz * nx is a multiple of 4 (every plane then starts on a 4-byte boundary), else as byte stores.  A sample outside
//                          0 ... num sets the status word (one integer atomic per lane that found one).
//   overlap_count          per label the samples on side A, on side B and on both: lanes stride the samples, 16 bytes per load where the sample
//                          count is a multiple of 16 (every plane then starts on a 16-byte boundary), compare four bytes at a time with integer
//                          bit work, add up in registers, meet across the wave, and one lane per wave adds to the label's three int64 counters.
//   sd_columns             pass 1 of surface_dist.h, one lane per (label, side, column): the border byte of every pixel of the column and, by a
//                          downward and an upward scan, its row distance g to the nearest border pixel of the column.
//   sd_rows                pass 2, one wave per (label, direction, row): the wave finds the border pixels of its row 64 columns at a time (a
//                          ballot), and for each of them its lanes stride the columns x' of the other side's g, take the minimum of
//                          sd_candidate in registers and meet across the wave.  Lane 0 counts the border pixels, those within each tolerance, and
//                          keeps the largest d2 as its key; per wave one integer add per counter and one integer max.
//                          ONE body in two compile-time forms.  sd_rows<false> (ts2d_surface_distances) is that and no more.  sd_rows<true>
//                          (ts2d_surface_distance_profile) keeps every border pixel's d2: the minimum of border pixel px goes to every lane,
//                          and lane px - x0 keeps it.  After the 64 columns of a chunk every lane stores its key to the key buffer (kSdNoKey
//                          where it has no border pixel: one coalesced store per chunk) and adds sd_sqrt of its d2 to its own float64 sum -
//                          one root per lane and chunk, all lanes at once.  The chunks come in increasing x0, so lane l adds the terms at
//                          x = l, l + 64, ... in increasing x from +0.0: level 1 of the tree of stats_tree.h.  At the end of the row the lanes
//                          are halved (st_wave_halve, kernels_stats.h) and lane 0 stores the row's partial.  Compile-time, not a null check
//                          at run time: the plain form then carries no broadcast, no per-lane key and no sum, and keeps its 35 registers
//                          (the profile form needs 46) without anyone having to measure that a branch on null costs nothing.
//                          The body is sd_row_walk, which the rows of a volume's boxes share (sdv_rows, kernels_evaluate_volume.h).
// Integer atomics only (sums and a maximum of non-negative keys: the result does not depend on their order), no flags, nothing waits for another
// wave (a workgroup of sd_columns and sd_rows is ONE wave); contraction off; every loop bound is a kernel argument, the grid's extent, 64 or a
// constant.  Indices into a plane are int32 or long long as the entry's limits need.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels_stats.h"
#include "surface_dist.h"

namespace ts2d {

constexpr int kPlThreads = 128;
constexpr int kPlStatusRange = 1;
constexpr int kOvThreads = 256;
constexpr int kOvMaxBlocks = 512;

// grid = ceil(ceil(nz * nx / 4) / kPlThreads).  out: uint8 [num][nz][nx]; vec: nz * nx is a multiple of 4.
template <typename T, int NW>
__global__ __launch_bounds__(kPlThreads) void project_labels_stream(const T* __restrict__ vol, int nz, int ny, int nx, long long sz, long long sy,
                                                                    long long sx, long long base, int num, int vec, uint8_t* __restrict__ out,
                                                                    int* __restrict__ status) {
    const long long N = (long long)nz * nx;
    const long long i0 = ((long long)blockIdx.x * kPlThreads + threadIdx.x) * 4;
    if (i0 >= N) return;
    const T* p[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const long long i = i0 + j < N ? i0 + j : i0;             // a pixel beyond the plane walks pixel i0 again: a valid address, nothing of it is stored
        const long long z = i / nx, x = i - z * nx;
        p[j] = vol + base + z * sz + x * sx;
    }
    uint32_t w[4][NW];
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int n = 0; n < NW; ++n) w[j][n] = 0u;
    bool bad = false;
    for (int y = 0; y < ny; ++y) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const long long v = (long long)p[j][y * sy];
            const bool in = v > 0 && v <= num;
            bad |= v < 0 || v > num;
            const uint32_t b = (uint32_t)(v - 1), word = b >> 5, bit = 1u << (b & 31u);
#pragma unroll
            for (int n = 0; n < NW; ++n) w[j][n] |= (in && word == (uint32_t)n) ? bit : 0u;
        }
    }
    if (bad) atomicOr(status, kPlStatusRange);
#pragma unroll
    for (int n = 0; n < NW; ++n) {
        const int bits = num - n * 32 < 32 ? num - n * 32 : 32;
        for (int b = 0; b < bits; ++b) {
            uint8_t* o = out + (long long)(n * 32 + b) * N + i0;
            if (vec) {
                const uint32_t four = ((w[0][n] >> b) & 1u) | (((w[1][n] >> b) & 1u) << 8) | (((w[2][n] >> b) & 1u) << 16) | (((w[3][n] >> b) & 1u) << 24);
                *reinterpret_cast<uint32_t*>(o) = four;
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (i0 + j < N) o[j] = (uint8_t)((w[j][n] >> b) & 1u);
            }
        }
    }
}

// the high bit of every byte of x that belongs to the label: planes - the byte is not 0; label map - the byte equals the value (v4: it in all four bytes)
__device__ __forceinline__ uint32_t ov_bytes(uint32_t x, int kind, uint32_t v4) {
    const uint32_t y = kind == kStLabelMap ? x ^ v4 : x;
    const uint32_t nonzero = (((y & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | y) & 0x80808080u;
    return kind == kStLabelMap ? nonzero ^ 0x80808080u : nonzero;
}

// grid = (blocks, K), block = kOvThreads.  a, b: planes [K][n] or one label map [n]; values [K]; out: [K][3] = n_a, n_b, n_both, zero before the launch.
__global__ __launch_bounds__(kOvThreads) void overlap_count(const uint8_t* __restrict__ a, int kind_a, const uint8_t* __restrict__ b, int kind_b,
                                                            const uint8_t* __restrict__ values, long long n, int vec,
                                                            unsigned long long* __restrict__ out) {
    const int k = (int)blockIdx.y;
    const uint8_t* pa = a + (kind_a == kStPlanes ? (long long)k * n : 0ll);
    const uint8_t* pb = b + (kind_b == kStPlanes ? (long long)k * n : 0ll);
    const uint8_t value = values[k];
    const long long first = (long long)blockIdx.x * kOvThreads + threadIdx.x, step = (long long)gridDim.x * kOvThreads;
    int ca = 0, cb = 0, cab = 0;
    if (vec) {
        const uint32_t v4 = (uint32_t)value * 0x01010101u;
        const uint4* qa = reinterpret_cast<const uint4*>(pa);
        const uint4* qb = reinterpret_cast<const uint4*>(pb);
        const long long groups = n >> 4;
        for (long long g = first; g < groups; g += step) {
            const uint4 va = qa[g], vb = qb[g];
            const uint32_t xa[4] = {va.x, va.y, va.z, va.w}, xb[4] = {vb.x, vb.y, vb.z, vb.w};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const uint32_t ma = ov_bytes(xa[j], kind_a, v4), mb = ov_bytes(xb[j], kind_b, v4);
                ca += __popc(ma); cb += __popc(mb); cab += __popc(ma & mb);
            }
        }
    } else {
        for (long long i = first; i < n; i += step) {
            const bool ma = st_masked(pa[i], kind_a, value), mb = st_masked(pb[i], kind_b, value);
            ca += ma ? 1 : 0; cb += mb ? 1 : 0; cab += (ma && mb) ? 1 : 0;
        }
    }
    for (int off = 32; off >= 1; off >>= 1) {
        ca += __shfl_down(ca, off, 64); cb += __shfl_down(cb, off, 64); cab += __shfl_down(cab, off, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        unsigned long long* o = out + (long long)k * 3;
        if (ca) atomicAdd(o + 0, (unsigned long long)ca);
        if (cb) atomicAdd(o + 1, (unsigned long long)cb);
        if (cab) atomicAdd(o + 2, (unsigned long long)cab);
    }
}

// grid = (ceil(W / 64), 2, L), block = 64.  a, b: planes [K][H * W] or one label map; label k0 + blockIdx.z; border: uint8 [L][2][H * W], g: uint16
// [L][2][H * W] (side 0: A, side 1: B).
__global__ __launch_bounds__(64) void sd_columns(const uint8_t* __restrict__ a, int kind_a, const uint8_t* __restrict__ b, int kind_b,
                                                 const uint8_t* __restrict__ values, int k0, int H, int W, uint8_t* __restrict__ border,
                                                 uint16_t* __restrict__ g) {
    const int x = (int)blockIdx.x * 64 + (int)threadIdx.x;
    if (x >= W) return;
    const int side = (int)blockIdx.y, l = (int)blockIdx.z, k = k0 + l;
    const long long HW = (long long)H * W;
    const int kind = side == 0 ? kind_a : kind_b;
    const uint8_t* m = (side == 0 ? a : b) + (kind == kStPlanes ? (long long)k * HW : 0ll);
    const uint8_t value = values[k];
    uint8_t* bo = border + ((long long)l * 2 + side) * HW;
    uint16_t* go = g + ((long long)l * 2 + side) * HW;
    int last = -1;
    for (int y = 0; y < H; ++y) {
        const long long i = (long long)y * W + x;
        const bool bd = sd_border(m, kind, value, H, W, y, x);
        bo[i] = bd ? 1 : 0;
        if (bd) last = y;
        go[i] = last < 0 ? kSdNone : (uint16_t)(y - last);
    }
    last = -1;
    for (int y = H - 1; y >= 0; --y) {
        const long long i = (long long)y * W + x;
        if (bo[i]) last = y;
        if (last >= 0 && (uint16_t)(last - y) < go[i]) go[i] = (uint16_t)(last - y);
    }
}

struct SdTolerances { double sq[kSdMaxTolerances]; };

// The ONE walk over the border pixels of a row, behind sd_rows (2-D planes) and sdv_rows (volumes: kernels_evaluate_volume.h), in compile-time
// forms: PROFILE as above; VOLUME chooses the candidate of column x' - sd_candidate(go[x'], dx) from the row distances of the other side, or
// sd_candidate_h(ho[x'], dx) from pass 2 of a volume - and where the row starts: a volume's row is a row of the label's BOX, whose column 0 is
// column x_first of the full extent, and the sum's lane of a term is its FULL-extent x % 64 (stats_tree.h over (Z * H, W)), so the chunks of 64
// start at `first` = -(x_first % 64) and lane l walks the box columns first + l, first + l + 64, ...: the terms of full-extent lane
// (x_first + x) % 64 = l in increasing x.  The columns a row skips that way, and those outside the box, have the term +0.0, which leaves the
// bits of a non-negative sum as they are.  The ballot, the broadcast, the key store, the per-lane root sums and the counters exist once.
// bo: the border bytes of the row (W of them); go / ho: g or h of the other side's row; counts: the (label, direction)'s [1 + T]; key_top: its
// largest key; key_row: the row's W keys (null: none kept); row_slot: the row's partial (null: no sum).
template <bool PROFILE, bool VOLUME>
__device__ __forceinline__ void sd_row_walk(const uint8_t* __restrict__ bo, const uint16_t* __restrict__ go, const double* __restrict__ ho, int first,
                                            int W, double sy, double sx, const SdTolerances& tol, int T, unsigned long long* __restrict__ counts,
                                            unsigned long long* __restrict__ key_top, uint64_t* __restrict__ key_row, double* __restrict__ row_slot,
                                            int lane) {
#pragma clang fp contract(off)
    int cnt = 0;
    int within[kSdMaxTolerances];
#pragma unroll
    for (int t = 0; t < kSdMaxTolerances; ++t) within[t] = 0;
    uint64_t key_max = 0;
    double acc = 0.0;                                              // (PROFILE)
    for (int x0 = VOLUME ? first : 0; x0 < W; x0 += 64) {
        const int x = x0 + lane;
        const bool in = VOLUME ? (x >= 0 && x < W) : x < W;
        unsigned long long todo = __ballot(in && bo[x] != 0);
        uint64_t mine = kSdNoKey;                                  // (PROFILE)
        while (todo) {                                             // at most 64 rounds; the mask is the same in every lane
            const int src = __ffsll((long long)todo) - 1, px = x0 + src;
            todo &= todo - 1;
            double best = sd_inf();
            for (int xo = lane; xo < W; xo += 64) {
                double c;
                if constexpr (VOLUME) c = sd_candidate_h(ho[xo], xo > px ? xo - px : px - xo, sx);
                else c = sd_candidate(go[xo], xo > px ? xo - px : px - xo, sy, sx);
                best = c < best ? c : best;
            }
            for (int off = 32; off >= 1; off >>= 1) { const double o = __shfl_down(best, off, 64); best = o < best ? o : best; }
            if constexpr (PROFILE) best = __shfl(best, 0, 64);     // lane 0 holds the minimum: now every lane does
            ++cnt;                                                 // (plain: the other lanes' tallies are not used)
            const uint64_t key = sd_key(best);
            key_max = key > key_max ? key : key_max;
#pragma unroll
            for (int t = 0; t < kSdMaxTolerances; ++t) within[t] += (t < T && best <= tol.sq[t]) ? 1 : 0;
            if constexpr (PROFILE) mine = lane == src ? key : mine;
        }
        if constexpr (PROFILE) {
            if (key_row && in) key_row[x] = mine;
            if (row_slot) acc = acc + (mine != kSdNoKey ? sd_sqrt(sd_unkey(mine)) : 0.0);      // (+0.0 for no border pixel: the sum stays as it is)
        }
    }
    if constexpr (PROFILE) {
        if (row_slot) {
            acc = st_wave_halve(acc);
            if (lane == 0) *row_slot = acc;
        }
    }
    if (lane == 0 && cnt) {
        atomicAdd(counts, (unsigned long long)cnt);
#pragma unroll
        for (int t = 0; t < kSdMaxTolerances; ++t)
            if (t < T && within[t]) atomicAdd(counts + 1 + t, (unsigned long long)within[t]);
        atomicMax(key_top, (unsigned long long)key_max);
    }
}

// grid = (H, 2, L), block = 64.  Direction 0: the border pixels of A against g of B; direction 1: the other way.  counts: [K][2][1 + T] (border
// pixels, then those within each tolerance), keys: [K][2] (the largest d2 as sd_key), both zero before the first launch.  PROFILE: also key_buf
// uint64 [L][2][H * W] (null: no keys are kept) and row_sum float64 [L][2][H] (null: no sum); the plain form reads neither argument.
template <bool PROFILE>
__global__ __launch_bounds__(64) void sd_rows(const uint8_t* __restrict__ border, const uint16_t* __restrict__ g, int k0, int H, int W, double sy,
                                              double sx, SdTolerances tol, int T, unsigned long long* __restrict__ counts,
                                              unsigned long long* __restrict__ keys, uint64_t* __restrict__ key_buf, double* __restrict__ row_sum) {
    const int y = (int)blockIdx.x, dir = (int)blockIdx.y, l = (int)blockIdx.z, k = k0 + l, lane = (int)threadIdx.x;
    const long long HW = (long long)H * W;
    const long long own = ((long long)l * 2 + dir) * HW + (long long)y * W;
    sd_row_walk<PROFILE, false>(border + own, g + ((long long)l * 2 + (1 - dir)) * HW + (long long)y * W, nullptr, 0, W, sy, sx, tol, T,
                                counts + ((long long)k * 2 + dir) * (1 + T), keys + (long long)k * 2 + dir,
                                PROFILE && key_buf ? key_buf + own : nullptr, PROFILE && row_sum ? row_sum + ((long long)l * 2 + dir) * H + y : nullptr,
                                lane);
}

}  // namespace ts2d
