// Percentiles of the intensities under a label behind ts2d_label_percentiles: per (label, channel, percentile) the float32 samples at the two
// sorted positions numpy's linear percentile interpolates between.  The statement is totalsegmentator2d_amd.statistics.label_percentiles_statement;
// tests/test_gpu_statistics_percentiles.py holds these kernels against it bit for bit.  The arithmetic - keys, ranks, digits, decision - is
// label_select.h and surface_dist.h.  Counts and boxes come from stats_rows<1> / stats_combine<1> of kernels_stats.h with C = 0: the label's
// row of out_int (count; min z, max z, min y, max y, min x, max x) is READ ON THE DEVICE by the kernels below, behind the launch boundary - no
// box is downloaded, and the grids are sized from the extents alone.
//
//   ls_select_init     per (label, channel, percentile) the two sorted positions (sd_percentile_ranks) with prefix 0, per (label, percentile) the
//                      weight; an empty label gets position -1: nothing is selected.
//   ls_select_hist     one round, one 8-bit digit of the 32-bit key, the top one first.  A wave walks rows of the label's BOX (box row
//                      blockIdx.x, + gridDim.x, ...) between the box's first and last column; a block beyond the box's rows, and every block of
//                      an empty label, ends before it reads a sample.  Per sample the segmentation byte and, for members only, the intensity;
//                      the key is formed in registers - there is no key buffer.  Per selection the digit of the keys that agree with the prefix
//                      is counted into an LDS histogram (R x 256 uint32) with integer atomics, then the non-zero bins go to the global bins with
//                      integer adds.  All R = 2 P selections of a (label, channel) share ONE read per round.  In round 0 every sample is a
//                      candidate of every selection, so ONE histogram is counted and added to the bins of all R.  Round 0 also reports a
//                      non-finite sample under the label (one integer atomicOr per wave that found one); the entry then downloads nothing.
//   ls_select_decide   one wave per selection, the body of sd_select_decide over (label, channel): four bins per lane, a running sum across
//                      the wave, the decision of sd_decide_quad; the wave leaves its bins zero for the next round.
//   ls_select_write    after round 3: the four decided digits back into the float32 (ls_unkey) into the result; an empty label gets +0.0.
//
// Integer atomics only (sums of counts: the result does not depend on the order of arrival), no floating-point atomics, no flags, nothing waits
// for another wave (a workgroup is ONE wave; the barriers of ls_select_hist order that wave's own LDS traffic); a loop bound is a kernel
// argument, the grid's extent, a constant or the label's box clamped to the extents - the finished result of an earlier launch -; plain C++
// stores.  Indices are int32 under the entry's 2^31 - 1 bound on the voxels; a plane or channel is reached through its own base pointer.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels_stats.h"
#include "label_select.h"

namespace ts2d {

constexpr int kLsHistMaxBlocks = 256;          // the histogram blocks of a (label, channel): block b walks the box rows b, b + 256, ...

struct LsPercentiles { double q[kSdMaxPercentiles]; };

// grid = L, block = 64.  out_int [K][kStInts] (stats_combine<1>) -> sel_rank int64 [L][C][P][2] (-1: an empty label), sel_prefix uint64
// [L][C][P][2] = 0, weights float64 [K][P] (+0.0 for an empty label).
__global__ __launch_bounds__(64) void ls_select_init(const long long* __restrict__ out_int, int k0, int C, LsPercentiles pc, int P,
                                                     long long* __restrict__ sel_rank, uint64_t* __restrict__ sel_prefix,
                                                     double* __restrict__ weights) {
    const int l = (int)blockIdx.x, k = k0 + l;
    const long long n = out_int[(long long)k * kStInts];
    for (int s = (int)threadIdx.x; s < C * P; s += 64) {
        const int c = s / P, p = s - c * P;
        long long i = -1, j = -1;
        double t = 0.0;
        if (n > 0) {
            double q = pc.q[0];
#pragma unroll
            for (int u = 1; u < kSdMaxPercentiles; ++u) q = u == p ? pc.q[u] : q;      // (no dynamically indexed kernel argument)
            sd_percentile_ranks(n, q, &i, &j, &t);
        }
        const long long at = ((long long)l * C + c) * P + p;
        sel_rank[2 * at] = i; sel_rank[2 * at + 1] = j;
        sel_prefix[2 * at] = 0; sel_prefix[2 * at + 1] = 0;
        if (c == 0) weights[(long long)k * P + p] = t;
    }
}

// grid = (blocks, C, L), block = 64, R * 256 * 4 bytes of dynamic LDS.  seg: planes [K][n] or one label map [n] with values [K]; x [C][n];
// out_int [K][kStInts]; sel_prefix [L][C][R]; bins uint32 [L][C][R][256], zero before the launch.
__global__ __launch_bounds__(64) void ls_select_hist(const uint8_t* __restrict__ seg, int kind, const uint8_t* __restrict__ values, int k0, int Z, int H,
                                                     int W, long long n, const float* __restrict__ x, const long long* __restrict__ out_int, int R,
                                                     int rnd, const uint64_t* __restrict__ sel_prefix, uint32_t* __restrict__ bins,
                                                     int* __restrict__ status) {
    extern __shared__ uint32_t ls_hist[];
    __shared__ uint64_t prefix[kSdMaxRanks];
    const int c = (int)blockIdx.y, l = (int)blockIdx.z, k = k0 + l, lane = (int)threadIdx.x, C = (int)gridDim.y;
    const long long* box = out_int + (long long)k * kStInts;
    if (box[0] == 0) return;                                       // an empty label: every selection is idle
    // the box, clamped to the extents: whatever the integers hold, no index leaves the volume
    const int z0 = box[4] > 0 ? (int)box[4] : 0, z1 = box[5] < Z - 1 ? (int)box[5] : Z - 1;
    const int y0 = box[6] > 0 ? (int)box[6] : 0, y1 = box[7] < H - 1 ? (int)box[7] : H - 1;
    const int x0 = box[8] > 0 ? (int)box[8] : 0, x1 = box[9] < W - 1 ? (int)box[9] : W - 1;
    if (z1 < z0 || y1 < y0 || x1 < x0) return;
    const int by = y1 - y0 + 1, box_rows = (z1 - z0 + 1) * by;      // (at most Z * H: an int32)
    if ((int)blockIdx.x >= box_rows) return;                       // a block beyond the box's rows
    const int Rc = rnd == 0 ? 1 : R;                               // round 0: one histogram serves every selection
    const long long state = ((long long)l * C + c) * R;
    for (int i = lane; i < Rc * kSdDigits; i += 64) ls_hist[i] = 0u;
    if (lane < R) prefix[lane] = sel_prefix[state + lane];
    __syncthreads();
    const uint8_t* m = seg + (kind == kStPlanes ? (long long)k * n : 0ll);
    const uint8_t value = kind == kStLabelMap ? values[k] : (uint8_t)0;
    const float* xc = x + (long long)c * n;
    int bad = 0;
    // trip counts, not running ends: an index never steps past the last one it uses, so none passes 2^31 - 1
    const int row_trips = (box_rows - 1 - (int)blockIdx.x) / (int)gridDim.x + 1, x_trips = st_lane_trips(x1 - x0 + 1, lane);
    for (int t = 0; t < row_trips; ++t) {
        const int i = (int)blockIdx.x + t * (int)gridDim.x;
        const int bz = i / by, row = ((z0 + bz) * H + y0 + (i - bz * by)) * W;      // (row + x < n <= 2^31 - 1)
        for (int j = 0; j < x_trips; ++j) {
            const int xx = x0 + lane + j * kStLanes;
            if (!st_masked(m[row + xx], kind, value)) continue;
            const float v = xc[row + xx];
            bad |= st_nonfinite(v) ? 1 : 0;
            const uint64_t key = ls_key(v);
            const uint32_t digit = (uint32_t)sd_digit(key, rnd);
            for (int r = 0; r < Rc; ++r)
                if (sd_digit_candidate(key, prefix[r], rnd)) atomicAdd(&ls_hist[r * kSdDigits + digit], 1u);
        }
    }
    __syncthreads();
    uint32_t* gb = bins + state * kSdDigits;
    for (int i = lane; i < R * kSdDigits; i += 64) {
        const uint32_t v = ls_hist[rnd == 0 ? (i & (kSdDigits - 1)) : i];
        if (v) atomicAdd(&gb[i], v);
    }
    if (rnd == 0) {
        bad = st_wave_max(bad);
        if (lane == 0 && bad) atomicOr(status, kStStatusNonfinite);
    }
}

// grid = (R, C, L), block = 64.  Decides digit rnd of one selection and leaves its bins zero.
__global__ __launch_bounds__(64) void ls_select_decide(int R, int rnd, long long* __restrict__ sel_rank, uint64_t* __restrict__ sel_prefix,
                                                       uint32_t* __restrict__ bins) {
    const int r = (int)blockIdx.x, c = (int)blockIdx.y, l = (int)blockIdx.z, lane = (int)threadIdx.x, C = (int)gridDim.y;
    const long long state = ((long long)l * C + c) * R + r;
    long long rank = sel_rank[state];
    if (rank < 0) return;                                          // nothing was counted: the bins are zero already
    uint32_t* b = bins + state * kSdDigits + lane * 4;
    const uint32_t cnt[4] = {b[0], b[1], b[2], b[3]};
    const long long own = (long long)cnt[0] + cnt[1] + cnt[2] + cnt[3];
    long long upto = own;                                          // the candidates of the digits of lanes 0 ... lane
    for (int off = 1; off < 64; off <<= 1) { const long long o = __shfl_up(upto, off, 64); upto += lane >= off ? o : 0; }
    uint64_t prefix = sel_prefix[state];
    if (sd_decide_quad(cnt, lane * 4, upto - own, rnd, &rank, &prefix)) { sel_rank[state] = rank; sel_prefix[state] = prefix; }
    b[0] = 0u; b[1] = 0u; b[2] = 0u; b[3] = 0u;
}

// grid = L, block = 64.  sel_prefix [L][C][R] -> out_rank float32 [K][C][R] (R = 2 P: [P][2]).
__global__ __launch_bounds__(64) void ls_select_write(const long long* __restrict__ out_int, int k0, int C, int R, const uint64_t* __restrict__ sel_prefix,
                                                      float* __restrict__ out_rank) {
    const int l = (int)blockIdx.x, k = k0 + l;
    const bool any = out_int[(long long)k * kStInts] > 0;
    for (int s = (int)threadIdx.x; s < C * R; s += 64)
        out_rank[(long long)k * C * R + s] = any ? ls_unkey(sel_prefix[(long long)l * C * R + s]) : 0.0f;
}

}  // namespace ts2d
