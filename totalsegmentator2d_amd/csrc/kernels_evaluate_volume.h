// The boundary distances of VOLUMES behind ts2d_volume_surface_distances: six-neighbour borders and the exact three-pass squared Euclidean
// distance of surface_dist.h (which has the argument), with the profile of kernels_evaluate_profile.h on request.  The statements are
// totalsegmentator2d_amd.evaluate.volume_surface_statement and volume_distance_profile_statement; tests/test_gpu_evaluate_volume.py holds these
// kernels against them bit for bit.
//
// EVERYTHING AFTER THE BOX KERNEL WORKS INSIDE A LABEL'S JOINT BOUNDING BOX: the inclusive box of the label over BOTH sides.  A voxel outside
// it is background for the label on either side, so it is no border voxel, lies on no line, and is no candidate of any minimum: the three
// passes restricted to the box take the definition's minima over the definition's candidates, bit for bit.  (The border predicate itself reads
// the full volume - a box face inside the volume has background behind it either way.)  A label empty on both sides has no box and costs
// nothing.  The host plans the scratch from the K x 6 box integers (evaluate_plan.h).  Per label and BOX voxel: 2 bytes of border (1 per
// side), 4 of g (uint16 per side), 16 of h (float64 per side); with percentiles 16 more (the keys of both directions, dense over the box,
// kSdNoKey off the border); with the sum 16 bytes per box ROW (z, y).  In a chunk's arrays label l starts at element 2 * vox of every per-voxel
// array, side or direction s at + s * nb (nb = bz * by * bx), voxel (zb, yb, xb) of the box at (zb * by + yb) * bx + xb; its row partials at
// 2 * row + s * bz * by.
//
//   sdv_box             per label the inclusive box over both sides: lanes stride the voxels (16 bytes per load where the voxel count is a multiple
//                       of 16, the byte tests of overlap_count), keep the smallest and largest z, y, x of the label's voxels in registers, meet
//                       across the wave, and one lane per wave that found a voxel does three integer atomicMin and three integer atomicMax.
//   sdv_lines           pass 1, one lane per (label, side, y, x) of the box: the border byte of every voxel of its line along z (sd_border3) and, by
//                       a forward and a backward scan, the line distance g.  Adjacent lanes hold adjacent x: the stores and the scans' reads
//                       coalesce.
//   sdv_planes          pass 2 and the hot path, O(box x by): a wave holds 64 adjacent columns x' of one z and kSdvRows output rows y of them in
//                       registers.  It strides y' over the box: ONE coalesced load of g(z, y', x') per y' (2 bytes a lane), f(g, sz) once, and
//                       per output row the candidate f(g, sz) + f(|y - y'|, sy) and the minimum - the second term is the same in every lane.
//                       g of a (z, x') column is read by / kSdvRows times, from cache after the first.  h is stored as float64, coalesced.
//                       No LDS: a lane's candidates come from its own column, there is nothing to share across the lanes but the uniform
//                       second term, which is two multiplies.
//   sdv_rows            pass 3, one wave per (label, direction, z, y) row of the box: sd_row_walk of kernels_evaluate.h - the body of sd_rows - with
//                       the candidate h + f(dx, sx), the chunks of 64 aligned to the FULL-extent x so that the sum's lanes are the tree's.
//   sdv_profile_combine level 2 of the sum over the FULL extent's Z * H rows from the box's rows alone: the partial of box row (zb, yb) is the
//                       partial of full-extent row r = (z0 + zb) * H + y0 + yb, whose lane is r % 64; lane l walks the rows with r % 64 = l in
//                       increasing r (z-slab after z-slab, within a slab from its first such row in steps of 64).  The rows outside the box,
//                       and a row's columns outside it, hold no border voxel: their terms and partials are +0.0, and adding +0.0 to a sum that
//                       started at +0.0 and has only non-negative terms leaves its bits (stats_tree.h), so skipping them equals adding them.
//   The selection runs on the box's dense key buffer with sd_select_init / sd_select_hist / sd_select_decide of kernels_evaluate_profile.h
//   unchanged (a key's place does not matter to a selection), one launch per label with a box.
//
// Integer atomics only (sums, min / max of integers, the max of the bits of non-negative float64), no flags, nothing waits for another wave (a
// workgroup of every kernel but sdv_box is ONE wave, and sdv_box's waves do not talk); contraction off; plain vector stores.  Every loop bound
// is a kernel argument, the grid's extent, 64, a constant or an extent of the label's descriptor, which the host wrote before the launch.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "evaluate_plan.h"
#include "kernels_evaluate.h"
#include "kernels_stats.h"

namespace ts2d {

constexpr int kSdvBoxThreads = 256;
constexpr int kSdvBoxMaxBlocks = 512;
constexpr int kSdvRows = 8;                    // output rows of a wave of sdv_planes

struct SdvCorners { uint32_t lo[3]; int hi[3]; };      // z, y, x

__device__ __forceinline__ void sdv_note(uint32_t i, uint32_t HW, uint32_t W, SdvCorners& c) {
    const uint32_t z = i / HW, r = i - z * HW, y = r / W, x = r - y * W;
    c.lo[0] = z < c.lo[0] ? z : c.lo[0]; c.lo[1] = y < c.lo[1] ? y : c.lo[1]; c.lo[2] = x < c.lo[2] ? x : c.lo[2];
    c.hi[0] = (int)z > c.hi[0] ? (int)z : c.hi[0]; c.hi[1] = (int)y > c.hi[1] ? (int)y : c.hi[1]; c.hi[2] = (int)x > c.hi[2] ? (int)x : c.hi[2];
}

// grid = (blocks, K), block = kSdvBoxThreads.  a, b: planes [K][n] or one label map [n], n = Z * H * W <= 2^31 - 1; vec: n is a multiple of 16.
// box: [K][6] = the smallest z, y, x as uint32 (every byte 0xFF before the launch) and the largest as int32 (-1 before the launch: the same bytes).
__global__ __launch_bounds__(kSdvBoxThreads) void sdv_box(const uint8_t* __restrict__ a, int kind_a, const uint8_t* __restrict__ b, int kind_b,
                                                          const uint8_t* __restrict__ values, long long n, int H, int W, int vec,
                                                          uint32_t* __restrict__ box) {
    const int k = (int)blockIdx.y;
    const uint8_t* pa = a + (kind_a == kStPlanes ? (long long)k * n : 0ll);
    const uint8_t* pb = b + (kind_b == kStPlanes ? (long long)k * n : 0ll);
    const uint8_t value = values[k];
    const uint32_t uW = (uint32_t)W, uHW = (uint32_t)H * (uint32_t)W;      // (H * W <= n < 2^31)
    const long long first = (long long)blockIdx.x * kSdvBoxThreads + threadIdx.x, step = (long long)gridDim.x * kSdvBoxThreads;
    SdvCorners c = {{0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu}, {-1, -1, -1}};
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
                const uint32_t m = ov_bytes(xa[j], kind_a, v4) | ov_bytes(xb[j], kind_b, v4);      // bit 8 t + 7: byte t belongs to the label
                if (m == 0u) continue;
#pragma unroll
                for (int t = 0; t < 4; ++t)
                    if (m & (0x80u << (8 * t))) sdv_note((uint32_t)(g * 16 + j * 4 + t), uHW, uW, c);
            }
        }
    } else {
        for (long long i = first; i < n; i += step)
            if (st_masked(pa[i], kind_a, value) || st_masked(pb[i], kind_b, value)) sdv_note((uint32_t)i, uHW, uW, c);
    }
#pragma unroll
    for (int d = 0; d < 3; ++d)
        for (int off = 32; off >= 1; off >>= 1) {
            const uint32_t lo = __shfl_down(c.lo[d], off, 64);
            const int hi = __shfl_down(c.hi[d], off, 64);
            c.lo[d] = lo < c.lo[d] ? lo : c.lo[d];
            c.hi[d] = hi > c.hi[d] ? hi : c.hi[d];
        }
    if ((threadIdx.x & 63) == 0 && c.hi[0] >= 0) {
        uint32_t* o = box + (long long)k * 6;
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            atomicMin(o + d, c.lo[d]);
            atomicMax(reinterpret_cast<int*>(o) + 3 + d, c.hi[d]);
        }
    }
}

// grid = (ceil(max by * bx / 64), 2, labels of the chunk), block = 64.  labels: the chunk's descriptors, label k0 + blockIdx.z first to last;
// border: uint8, g: uint16, laid out as the head of this file says (side 0: A, side 1: B).
__global__ __launch_bounds__(64) void sdv_lines(const uint8_t* __restrict__ a, int kind_a, const uint8_t* __restrict__ b, int kind_b,
                                                const uint8_t* __restrict__ values, const SdvLabel* __restrict__ labels, int k0, int Z, int H, int W,
                                                uint8_t* __restrict__ border, uint16_t* __restrict__ g) {
    const SdvLabel d = labels[blockIdx.z];
    const long long plane = (long long)d.by * d.bx, i = (long long)blockIdx.x * 64 + (long long)threadIdx.x;
    if (i >= plane) return;                                        // (an empty label: plane = 0)
    const int side = (int)blockIdx.y, k = k0 + (int)blockIdx.z;
    const int yb = (int)(i / d.bx), xb = (int)(i - (long long)yb * d.bx), y = d.y0 + yb, x = d.x0 + xb;
    const long long n = (long long)Z * H * W, nb = plane * d.bz;
    const int kind = side == 0 ? kind_a : kind_b;
    const uint8_t* m = (side == 0 ? a : b) + (kind == kStPlanes ? (long long)k * n : 0ll);
    const uint8_t value = values[k];
    uint8_t* bo = border + 2 * d.vox + side * nb + i;
    uint16_t* go = g + 2 * d.vox + side * nb + i;
    int last = -1;
    for (int zb = 0; zb < d.bz; ++zb) {
        const bool bd = sd_border3(m, kind, value, Z, H, W, d.z0 + zb, y, x);
        bo[zb * plane] = bd ? 1 : 0;
        if (bd) last = zb;
        go[zb * plane] = last < 0 ? kSdNone : (uint16_t)(zb - last);
    }
    last = -1;
    for (int zb = d.bz - 1; zb >= 0; --zb) {
        if (bo[zb * plane]) last = zb;
        if (last >= 0 && (uint16_t)(last - zb) < go[zb * plane]) go[zb * plane] = (uint16_t)(last - zb);
    }
}

// grid = (max over the chunk of ceil(bx / 64) * ceil(by / kSdvRows) * bz, 2, labels of the chunk), block = 64.  g as sdv_lines left it;
// h: float64 in the same layout.
__global__ __launch_bounds__(64) void sdv_planes(const uint16_t* __restrict__ g, const SdvLabel* __restrict__ labels, double sz, double sy,
                                                 double* __restrict__ h) {
#pragma clang fp contract(off)
    const SdvLabel d = labels[blockIdx.z];
    const int xt = (d.bx + 63) / 64, yt = (d.by + kSdvRows - 1) / kSdvRows;
    const long long blocks = (long long)xt * yt * d.bz, bi = (long long)blockIdx.x;
    if (bi >= blocks) return;
    const int xi = (int)(bi % xt), yi = (int)((bi / xt) % yt), zb = (int)(bi / ((long long)xt * yt));
    const int xb = xi * 64 + (int)threadIdx.x, y_first = yi * kSdvRows;
    if (xb >= d.bx) return;                                        // (the lanes do not talk: no cross-lane move follows)
    const long long plane = (long long)d.by * d.bx, nb = plane * d.bz, at = 2 * d.vox + (long long)blockIdx.y * nb + zb * plane + xb;
    const uint16_t* gc = g + at;
    double best[kSdvRows];
#pragma unroll
    for (int j = 0; j < kSdvRows; ++j) best[j] = sd_inf();
    for (int yo = 0; yo < d.by; ++yo) {
        const uint16_t gg = gc[(long long)yo * d.bx];
#pragma unroll
        for (int j = 0; j < kSdvRows; ++j) {
            const int dy = y_first + j > yo ? y_first + j - yo : yo - (y_first + j);
            const double c = sd_candidate_line(gg, dy, sz, sy);
            best[j] = c < best[j] ? c : best[j];
        }
    }
    double* ho = h + at;
#pragma unroll
    for (int j = 0; j < kSdvRows; ++j)
        if (y_first + j < d.by) ho[(long long)(y_first + j) * d.bx] = best[j];
}

// grid = (max over the chunk of bz * by, 2, labels of the chunk), block = 64.  Direction 0: the border voxels of A against h of B; direction 1:
// the other way.  counts, keys: as sd_rows.  PROFILE: key_buf uint64 dense over the boxes (null: no keys are kept), row_sum float64 per box
// row (null: no sum).
template <bool PROFILE>
__global__ __launch_bounds__(64) void sdv_rows(const uint8_t* __restrict__ border, const double* __restrict__ h, const SdvLabel* __restrict__ labels,
                                               int k0, double sx, SdTolerances tol, int T, unsigned long long* __restrict__ counts,
                                               unsigned long long* __restrict__ keys, uint64_t* __restrict__ key_buf, double* __restrict__ row_sum) {
    const SdvLabel d = labels[blockIdx.z];
    const long long rows = (long long)d.bz * d.by, row = (long long)blockIdx.x;
    if (row >= rows) return;                                       // (the whole wave)
    const int dir = (int)blockIdx.y, k = k0 + (int)blockIdx.z;
    const long long nb = rows * d.bx, own = 2 * d.vox + dir * nb + row * d.bx, other = 2 * d.vox + (1 - dir) * nb + row * d.bx;
    sd_row_walk<PROFILE, true>(border + own, nullptr, h + other, -(d.x0 % 64), d.bx, 0.0, sx, tol, T, counts + ((long long)k * 2 + dir) * (1 + T),
                               keys + (long long)k * 2 + dir, PROFILE && key_buf ? key_buf + own : nullptr,
                               PROFILE && row_sum ? row_sum + 2 * d.row + dir * rows + row : nullptr, (int)threadIdx.x);
}

// grid = (2, labels of the chunk), block = 64.  row_sum as sdv_rows left it -> sums [K][2] (zero before the first launch: an empty label's stay).
__global__ __launch_bounds__(64) void sdv_profile_combine(const double* __restrict__ row_sum, const SdvLabel* __restrict__ labels, int k0, int H,
                                                          double* __restrict__ sums) {
#pragma clang fp contract(off)
    const SdvLabel d = labels[blockIdx.y];
    if (d.bz == 0) return;
    const int dir = (int)blockIdx.x, lane = (int)threadIdx.x;
    const double* rs = row_sum + 2 * d.row + (long long)dir * d.bz * d.by;
    double acc = 0.0;
    for (int zb = 0; zb < d.bz; ++zb) {
        const long long r0 = (long long)(d.z0 + zb) * H + d.y0;   // the full-extent row of box row (zb, 0)
        const int j0 = (lane - (int)(r0 % 64) + 64) % 64;          // the first box row of the slab whose full-extent row has this lane
        for (int j = j0; j < d.by; j += 64) acc = acc + rs[(long long)zb * d.by + j];
    }
    acc = st_wave_halve(acc);
    if (lane == 0) sums[(long long)(k0 + (int)blockIdx.y) * 2 + dir] = acc;
}

}  // namespace ts2d
