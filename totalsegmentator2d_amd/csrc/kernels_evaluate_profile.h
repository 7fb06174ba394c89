// What the distance profile of ts2d_surface_distance_profile adds behind the two passes of the boundary distances: per (label, direction) the sum
// of the distances in the fixed tree and their exact order statistics at requested percentiles.  The statement is
// totalsegmentator2d_amd.evaluate.distance_profile_statement; tests/test_gpu_evaluate_profile.py holds these kernels against it bit for bit.
// The arithmetic - root, ranks, digits, decision - is surface_dist.h.  The passes themselves, sd_columns and sd_rows<true> - which leaves the key
// buffer and the row partials these kernels read - are kernels_evaluate.h: there is ONE walk over the border pixels.
//
//   sd_profile_combine  one wave per (label, direction): level 2 over the H row partials (st_lane_rows, then the halving).
//   sd_select_init      per (label, direction, percentile) the two sorted positions and the weight from the border count that sd_rows has
//                       just left behind (sd_percentile_ranks); an empty border gets position -1: nothing is selected.
//   sd_select_hist      one round of the selection: a wave per slice of a (label, direction)'s key buffer counts, per selection, the digit of the
//                       keys that agree with the selection's prefix - into an LDS histogram with integer atomics, then its non-zero bins into the
//                       global bins with integer adds.  All selections of a (label, direction) share ONE read of the keys per round.
//   sd_select_decide    one wave per selection: lane l holds the bins of the digits 4 l ... 4 l + 3, a running sum across the wave gives every
//                       lane the candidates below its digits, and the one lane the position falls to decides (sd_decide_quad).  The wave leaves
//                       the bins zero for the next round.
//
// The key buffer is DENSE, uint64 [L][2][H * W]: a pixel's key lies at the pixel's place.  Compacting it per row would save the selection's
// bandwidth (borders are a few percent of the pixels) but needs every row's count and an exclusive scan before pass 2 so that a key's place does
// not depend on the order of arrival - a further pass over the border bytes and a launch per chunk - while the dense reads are coalesced 8-byte
// loads of which all but the border keys are dropped after one compare.  A (label, direction) with an empty border reads nothing at all.
//
// Integer atomics only (sums: the result does not depend on their order), no floating-point atomics, no flags, nothing waits for another wave
// (a workgroup is ONE wave throughout; the barriers of sd_select_hist order that wave's own LDS traffic); every loop bound is a kernel argument,
// the grid's extent, 64 or a constant; plain C++ stores.  A plane's index is a long long.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels_evaluate.h"
#include "stats_tree.h"

namespace ts2d {

constexpr int kSpHistMaxBlocks = 256;

struct SdPercentiles { double q[kSdMaxPercentiles]; };

// grid = (2, L), block = 64.  row_sum [L][2][H] -> sums [K][2].
__global__ __launch_bounds__(64) void sd_profile_combine(const double* __restrict__ row_sum, int k0, int H, double* __restrict__ sums) {
    const int dir = (int)blockIdx.x, l = (int)blockIdx.y, lane = (int)threadIdx.x;
    const double v = st_wave_halve(st_lane_rows(row_sum + ((long long)l * 2 + dir) * H, H, lane));
    if (lane == 0) sums[(long long)(k0 + l) * 2 + dir] = v;
}

// grid = L, block = 64.  counts [K][2][1 + T] -> sel_rank int64 [K][2][P][2] (-1: an empty border), sel_prefix uint64 [K][2][P][2] = 0,
// weights float64 [K][2][P] (+0.0 for an empty border).
__global__ __launch_bounds__(64) void sd_select_init(const unsigned long long* __restrict__ counts, int k0, int T, SdPercentiles pc, int P,
                                                     long long* __restrict__ sel_rank, uint64_t* __restrict__ sel_prefix,
                                                     double* __restrict__ weights) {
    const int k = k0 + (int)blockIdx.x;
    for (int s = (int)threadIdx.x; s < 2 * P; s += 64) {
        const int dir = s / P, p = s - dir * P;
        const long long n = (long long)counts[((long long)k * 2 + dir) * (1 + T)];
        long long i = -1, j = -1;
        double t = 0.0;
        if (n > 0) {
            double q = pc.q[0];
#pragma unroll
            for (int u = 1; u < kSdMaxPercentiles; ++u) q = u == p ? pc.q[u] : q;      // (no dynamically indexed kernel argument)
            sd_percentile_ranks(n, q, &i, &j, &t);
        }
        const long long at = ((long long)k * 2 + dir) * P + p;
        sel_rank[2 * at] = i; sel_rank[2 * at + 1] = j;
        sel_prefix[2 * at] = 0; sel_prefix[2 * at + 1] = 0;
        weights[at] = t;
    }
}

// grid = (blocks, 2, L), block = 64.  key_buf [L][2][HW]; R = 2 P selections per (label, direction); sel_rank, sel_prefix [K][2][R];
// bins uint32 [L][2][R][256], zero before the launch.
__global__ __launch_bounds__(64) void sd_select_hist(const uint64_t* __restrict__ key_buf, int k0, long long HW, int R, int rnd,
                                                     const long long* __restrict__ sel_rank, const uint64_t* __restrict__ sel_prefix,
                                                     uint32_t* __restrict__ bins) {
    __shared__ uint32_t hist[kSdMaxRanks * kSdDigits];
    __shared__ uint64_t prefix[kSdMaxRanks];
    __shared__ int active[kSdMaxRanks];
    const int dir = (int)blockIdx.y, l = (int)blockIdx.z, lane = (int)threadIdx.x;
    const long long state = ((long long)(k0 + l) * 2 + dir) * R;
    for (int i = lane; i < R * kSdDigits; i += 64) hist[i] = 0u;
    if (lane < R) { prefix[lane] = sel_prefix[state + lane]; active[lane] = sel_rank[state + lane] >= 0 ? 1 : 0; }
    __syncthreads();
    if (!active[0]) return;                                        // an empty border: every selection of the (label, direction) is idle
    const uint64_t* kb = key_buf + ((long long)l * 2 + dir) * HW;
    for (long long i = (long long)blockIdx.x * 64 + lane; i < HW; i += (long long)gridDim.x * 64) {
        const uint64_t key = kb[i];
        if (key == kSdNoKey) continue;
        const uint32_t digit = (uint32_t)sd_digit(key, rnd);
        for (int r = 0; r < R; ++r)
            if (sd_digit_candidate(key, prefix[r], rnd)) atomicAdd(&hist[r * kSdDigits + digit], 1u);
    }
    __syncthreads();
    uint32_t* gb = bins + (((long long)l * 2 + dir) * R) * kSdDigits;
    for (int i = lane; i < R * kSdDigits; i += 64)
        if (hist[i]) atomicAdd(&gb[i], hist[i]);
}

// grid = (R, 2, L), block = 64.  Decides digit rnd of one selection and leaves its bins zero.
__global__ __launch_bounds__(64) void sd_select_decide(int k0, int R, int rnd, long long* __restrict__ sel_rank, uint64_t* __restrict__ sel_prefix,
                                                       uint32_t* __restrict__ bins) {
    const int r = (int)blockIdx.x, dir = (int)blockIdx.y, l = (int)blockIdx.z, lane = (int)threadIdx.x;
    const long long state = ((long long)(k0 + l) * 2 + dir) * R + r;
    long long rank = sel_rank[state];
    if (rank < 0) return;                                          // nothing was counted: the bins are zero already
    uint32_t* b = bins + ((((long long)l * 2 + dir) * R + r) * kSdDigits) + lane * 4;
    const uint32_t c[4] = {b[0], b[1], b[2], b[3]};
    const long long own = (long long)c[0] + c[1] + c[2] + c[3];
    long long upto = own;                                          // the candidates of the digits of lanes 0 ... lane
    for (int off = 1; off < 64; off <<= 1) { const long long o = __shfl_up(upto, off, 64); upto += lane >= off ? o : 0; }
    uint64_t prefix = sel_prefix[state];
    if (sd_decide_quad(c, lane * 4, upto - own, rnd, &rank, &prefix)) { sel_rank[state] = rank; sel_prefix[state] = prefix; }
    b[0] = 0u; b[1] = 0u; b[2] = 0u; b[3] = 0u;
}

}  // namespace ts2d
