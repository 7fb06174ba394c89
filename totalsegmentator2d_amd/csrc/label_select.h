// The arithmetic of the percentiles of the intensities under a label (kernels_stats_select.h, ts2d_label_percentiles) that the statement,
// totalsegmentator2d_amd.statistics.label_percentiles_statement, fixes bit for bit: which sample of a label stands at a sorted position.  Its own
// header, host and device: tests/test_statistics_percentiles_cpu.py compiles it into a stand-alone program and holds its host walk,
// ls_label_percentiles, against the statement.
//
// Order.  The float32 samples of a channel under a label are ordered by their keys (rs_key of ray_select.h: -0.0 right below +0.0, the
// subnormals between the zeros and the normals, equal values repeated).  A NaN has no place in that order: the entry reports a non-finite
// sample under a label and writes nothing.
// Ranks.  Percentile q among n >= 1 samples selects the sorted positions i <= j and the weight t of sd_percentile_ranks (surface_dist.h), called
// as it is; the caller interpolates between the two selected samples on the host.
// Selection.  A 32-bit key is widened into the top half of a 64-bit key (ls_key), so the digits, the candidates and the decision of the
// boundary distances' selection (sd_digit, sd_digit_candidate, sd_decide_quad) serve unchanged: rounds 0 ... 3 of their eight look at the four
// bytes of the key, the top one first, and after round 3 the top half of the prefix is the key at the sorted position (ls_unkey).  Integers only.
#pragma once
#include <stdint.h>

#include "surface_dist.h"

namespace ts2d {

constexpr int kLsRounds = 4;                   // a 32-bit key in 8-bit digits: the rounds 0 ... 3 of sd_round_shift

TS2D_SD_HD uint64_t ls_key(float v) { return (uint64_t)rs_key(v) << 32; }
TS2D_SD_HD float ls_unkey(uint64_t prefix) { return rs_unkey<float>((uint32_t)(prefix >> 32)); }

#if !defined(__HIP_DEVICE_COMPILE__)
// The sample of the label at sorted position rank (0 <= rank < the label's samples) among m[0 ... n - 1], x[0 ... n - 1]: what ls_select_hist
// and ls_select_decide compute together in four rounds.
inline float ls_select_rank(const uint8_t* m, int kind, uint8_t value, const float* x, size_t n, long long rank) {
    uint64_t prefix = 0;
    for (int rnd = 0; rnd < kLsRounds; ++rnd) {
        uint32_t bins[kSdDigits] = {0};
        for (size_t i = 0; i < n; ++i) {
            if (!st_masked(m[i], kind, value)) continue;
            const uint64_t key = ls_key(x[i]);
            if (sd_digit_candidate(key, prefix, rnd)) ++bins[sd_digit(key, rnd)];
        }
        long long below = 0;
        for (int d0 = 0; d0 < kSdDigits; d0 += 4) {
            if (sd_decide_quad(bins + d0, d0, below, rnd, &rank, &prefix)) break;
            below += (long long)bins[d0] + bins[d0 + 1] + bins[d0 + 2] + bins[d0 + 3];
        }
    }
    return ls_unkey(prefix);
}

// One label and one channel on the host, what the kernels of kernels_stats_select.h compute together: the label's samples (the result), per
// percentile q[p] the samples at the two sorted positions (rank_values [P][2]) and the weight (weights [P]) - all +0.0 for an empty label -, and
// in *bad whether a sample under the label is not finite (the entry then writes nothing; here the selection still runs, on the keys).
inline long long ls_label_percentiles(const uint8_t* m, int kind, uint8_t value, const float* x, size_t n, const double* q, int P, float* rank_values,
                                      double* weights, int* bad) {
    long long count = 0;
    *bad = 0;
    for (size_t i = 0; i < n; ++i)
        if (st_masked(m[i], kind, value)) { ++count; *bad |= st_nonfinite(x[i]) ? 1 : 0; }
    for (int p = 0; p < P; ++p) {
        rank_values[2 * p] = 0.0f; rank_values[2 * p + 1] = 0.0f; weights[p] = 0.0;
        if (count == 0) continue;
        long long i, j;
        sd_percentile_ranks(count, q[p], &i, &j, weights + p);
        rank_values[2 * p] = ls_select_rank(m, kind, value, x, n, i);
        rank_values[2 * p + 1] = ls_select_rank(m, kind, value, x, n, j);
    }
    return count;
}
#endif

}  // namespace ts2d
