// Per-label statistics of a segmentation, which need no engine: ts2d_label_statistics (kernels_stats.h; the tree of its float64 sums:
// stats_tree.h; the statement: totalsegmentator2d_amd/statistics.py) and ts2d_label_percentiles (kernels_stats_select.h; the arithmetic:
// label_select.h; the chunks: stats_plan.cpp).  Host pointers in and out, one call = one upload, every label on the
// device in chunks of labels whose row partials stay below max_scratch_bytes, one download; every device buffer of the call is one DevMem,
// so HIP_TRY may return wherever it fails.
#include "engine_internal.h"
#include "entry_util.h"
#include "kernels_stats.h"
#include "kernels_stats_select.h"
#include "stats_plan.h"

#include <cstring>
#include <vector>

using namespace ts2d;

static_assert(kStStatusNonfinite == TS2D_STATS_NONFINITE, "the status bit speaks the C header's number");
static_assert(kStPlanes == TS2D_STATS_PLANES && kStLabelMap == TS2D_STATS_LABELMAP, "the kinds speak the C header's numbers");
static_assert(kStInts == TS2D_STATS_INTS && kStF64s == TS2D_STATS_F64S, "the result layout is the C header's");

int ts2d_label_statistics(int device, const uint8_t* seg, int kind, const uint8_t* values, int K, int Z, int H, int W, const float* intensities,
                          int C, size_t max_scratch_bytes, int64_t* out_int, double* out_f64, int* status) {
    const char* const entry = "ts2d_label_statistics";
    if (!seg || !out_int || !status) return fail(TS2D_ERR_INVALID, "%s: null argument", entry);
    *status = 0;
    if (!label_kind(kind)) return fail(TS2D_ERR_INVALID, "%s: kind %d is neither planes (0) nor label map (1)", entry, kind);
    TRY(check_label_count(entry, K));
    if (!volume_fits_int32(Z, H, W)) return fail(TS2D_ERR_INVALID, "%s: %d x %d x %d is empty or more than 2^31 - 1 voxels", entry, Z, H, W);
    if (C < 0 || C > TS2D_STATS_MAX_CHANNELS) return fail(TS2D_ERR_INVALID, "%s: C = %d channels outside 0 ... %d", entry, C, TS2D_STATS_MAX_CHANNELS);
    if (C > 0 && (!intensities || !out_f64)) return fail(TS2D_ERR_INVALID, "%s: C = %d channels without intensities or out_f64", entry, C);
    if (kind == kStLabelMap) TRY(check_label_values(entry, values, K));
    const size_t n = (size_t)Z * H * W, R = (size_t)Z * H;
    // a label's row partials and the labels of a chunk: stats_plan.cpp
    size_t L = 0, per_label = 0, budget = 0;
    const int planned = st_plan(K, C, (long long)R, max_scratch_bytes, &L, &per_label, &budget);
    if (planned == -1)
        return fail(TS2D_ERR_INVALID, "%s: the row partials of ONE label (%zu rows, %d channels) take %zu bytes, above max_scratch_bytes = %zu", entry,
                    R, C, per_label, budget);
    if (planned != 0) return fail(TS2D_ERR_INVALID, "%s: %zu rows x %d channels are more partial slots than an int32 index reaches", entry, R, C);

    HIP_TRY(hipSetDevice(device));
    const size_t seg_bytes = kind == kStPlanes ? (size_t)K * n : n;
    // [status | values || out_int | out_f64 || segmentation | intensities | partials of a chunk]: what starts as zero, what is downloaded, the rest
    ArenaLayout lay;
    const size_t o_status = lay.add(sizeof(int)), o_val = lay.add((size_t)K);
    const size_t o_int = lay.add((size_t)K * kStInts * sizeof(long long)), o_f64 = lay.add((size_t)K * C * kStF64s * sizeof(double));
    const size_t o_seg = lay.add(seg_bytes), o_x = lay.add((size_t)C * n * sizeof(float));
    const size_t o_cnt = lay.add(L * R * 4), o_minx = lay.add(L * R * 4), o_maxx = lay.add(L * R * 4), o_sumx = lay.add(L * R * 8);
    const size_t o_fsum = lay.add(L * C * R * 8), o_kmin = lay.add(L * C * R * 4), o_kmax = lay.add(L * C * R * 4);
    DevMem d;
    HIP_TRY(d.alloc(lay.total()));
    HIP_TRY(hipMemset(d.as<char>(), 0, o_int));
    if (kind == kStLabelMap) HIP_TRY(hipMemcpy(d.as<char>(o_val), values, (size_t)K, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d.as<char>(o_seg), seg, seg_bytes, hipMemcpyHostToDevice));
    if (C > 0) HIP_TRY(hipMemcpy(d.as<char>(o_x), intensities, (size_t)C * n * sizeof(float), hipMemcpyHostToDevice));
    int* const d_status = d.as<int>(o_status);
    const uint8_t* const d_values = d.as<const uint8_t>(o_val);
    long long* const d_int = d.as<long long>(o_int);
    double* const d_f64 = d.as<double>(o_f64);
    const uint8_t* const d_seg = d.as<const uint8_t>(o_seg);
    const float* const d_x = d.as<const float>(o_x);
    const StScratch s = {d.as<int>(o_cnt), d.as<int>(o_minx), d.as<int>(o_maxx), d.as<long long>(o_sumx),
                         d.as<double>(o_fsum), d.as<uint32_t>(o_kmin), d.as<uint32_t>(o_kmax)};
    for (int k0 = 0; k0 < K; k0 += (int)L) {
        const unsigned labels = (unsigned)(K - k0 < (int)L ? K - k0 : (int)L);
        const FoldedGrid fg = fold_grid((long long)R, kStLanes);      // (R * 64 threads pass 2^32 from R = 2^26 on)
        const dim3 rows(fg.x, labels, fg.fold), block(kStLanes);
        hipLaunchKernelGGL(stats_rows<1>, rows, block, 0, 0, d_seg, kind, d_values, k0, (int)R, W, (long long)n, d_x, C, s, d_f64, d_status);
        hipLaunchKernelGGL(stats_combine<1>, dim3(labels), block, 0, 0, k0, (int)R, H, Z, W, C, s, d_int, d_f64);
        if (C > 0) {
            hipLaunchKernelGGL(stats_rows<2>, rows, block, 0, 0, d_seg, kind, d_values, k0, (int)R, W, (long long)n, d_x, C, s, d_f64, d_status);
            hipLaunchKernelGGL(stats_combine<2>, dim3(labels), block, 0, 0, k0, (int)R, H, Z, W, C, s, d_int, d_f64);
        }
        HIP_TRY(hipGetLastError());
    }
    int st = 0;
    HIP_TRY(hipMemcpy(&st, d_status, sizeof(st), hipMemcpyDeviceToHost));      // (waits for the launches: the default stream orders them)
    if (st) { *status = st; return TS2D_OK; }                                    // a non-finite intensity under a label: the outputs stay as they were
    // one download: out_int and out_f64 lie next to each other (the gap of the alignment goes along)
    std::vector<char> host(o_seg - o_int);
    HIP_TRY(hipMemcpy(host.data(), d.as<char>(o_int), host.size(), hipMemcpyDeviceToHost));
    memcpy(out_int, host.data(), (size_t)K * kStInts * sizeof(int64_t));
    if (C > 0) memcpy(out_f64, host.data() + (o_f64 - o_int), (size_t)K * C * kStF64s * sizeof(double));
    return TS2D_OK;
}

static_assert(kSdMaxPercentiles == TS2D_STATS_MAX_PERCENTILES, "the percentile limit speaks the C header's number");

int ts2d_label_percentiles(int device, const uint8_t* seg, int kind, const uint8_t* values, int K, int Z, int H, int W, const float* intensities,
                           int C, const double* percentiles, int P, size_t max_scratch_bytes, int64_t* out_count, float* out_rank_f32,
                           double* out_weight_f64, int* status) {
    const char* const entry = "ts2d_label_percentiles";
    if (!seg || !intensities || !percentiles || !out_count || !out_rank_f32 || !out_weight_f64 || !status)
        return fail(TS2D_ERR_INVALID, "%s: null argument", entry);
    *status = 0;
    if (!label_kind(kind)) return fail(TS2D_ERR_INVALID, "%s: kind %d is neither planes (0) nor label map (1)", entry, kind);
    TRY(check_label_count(entry, K));
    if (!volume_fits_int32(Z, H, W)) return fail(TS2D_ERR_INVALID, "%s: %d x %d x %d is empty or more than 2^31 - 1 voxels", entry, Z, H, W);
    if (C < 1 || C > TS2D_STATS_MAX_CHANNELS) return fail(TS2D_ERR_INVALID, "%s: C = %d channels outside 1 ... %d", entry, C, TS2D_STATS_MAX_CHANNELS);
    if (P < 1 || P > kSdMaxPercentiles) return fail(TS2D_ERR_INVALID, "%s: P = %d percentiles outside 1 ... %d", entry, P, kSdMaxPercentiles);
    LsPercentiles pc = {};
    for (int p = 0; p < P; ++p) {
        if (!(percentiles[p] >= 0.0 && percentiles[p] <= 100.0))
            return fail(TS2D_ERR_INVALID, "%s: percentiles[%d] = %g outside 0 ... 100", entry, p, percentiles[p]);
        pc.q[p] = percentiles[p];
    }
    if (kind == kStLabelMap) TRY(check_label_values(entry, values, K));
    const size_t n = (size_t)Z * H * W, rows = (size_t)Z * H;
    const int R = 2 * P;
    std::vector<LsChunk> chunks;
    size_t need = 0, budget = 0;
    if (ls_plan(K, C, P, (long long)rows, max_scratch_bytes, &chunks, &need, &budget) != 0)
        return fail(TS2D_ERR_INVALID, "%s: the state of ONE label (%zu rows, %d channels, %d percentiles) takes %zu bytes, above max_scratch_bytes = %zu",
                    entry, rows, C, P, need, budget);
    const size_t L = (size_t)(chunks[0].k1 - chunks[0].k0);          // the largest chunk: the first

    HIP_TRY(hipSetDevice(device));
    const size_t seg_bytes = kind == kStPlanes ? (size_t)K * n : n;
    // [status | values || counts and boxes | rank values | weights || segmentation | intensities | state of a chunk]: the first three parts start
    // as zero, the middle is downloaded
    ArenaLayout lay;
    const size_t o_status = lay.add(sizeof(int)), o_val = lay.add((size_t)K);
    const size_t o_int = lay.add((size_t)K * kStInts * sizeof(long long)), o_rank = lay.add((size_t)K * C * R * sizeof(float));
    const size_t o_wgt = lay.add((size_t)K * P * sizeof(double));
    const size_t o_seg = lay.add(seg_bytes), o_x = lay.add((size_t)C * n * sizeof(float));
    const size_t o_cnt = lay.add(L * rows * 4), o_minx = lay.add(L * rows * 4), o_maxx = lay.add(L * rows * 4), o_sumx = lay.add(L * rows * 8);
    const size_t o_sel = lay.add(L * C * R * sizeof(long long)), o_pre = lay.add(L * C * R * sizeof(uint64_t));
    const size_t o_bins = lay.add(L * C * R * kSdDigits * sizeof(uint32_t));
    DevMem d;
    HIP_TRY(d.alloc(lay.total()));
    HIP_TRY(hipMemset(d.as<char>(), 0, o_seg));
    HIP_TRY(hipMemset(d.as<char>(o_bins), 0, lay.total() - o_bins));
    if (kind == kStLabelMap) HIP_TRY(hipMemcpy(d.as<char>(o_val), values, (size_t)K, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d.as<char>(o_seg), seg, seg_bytes, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d.as<char>(o_x), intensities, (size_t)C * n * sizeof(float), hipMemcpyHostToDevice));
    int* const d_status = d.as<int>(o_status);
    const uint8_t* const d_values = d.as<const uint8_t>(o_val);
    long long* const d_int = d.as<long long>(o_int);
    const uint8_t* const d_seg = d.as<const uint8_t>(o_seg);
    const float* const d_x = d.as<const float>(o_x);
    long long* const d_sel = d.as<long long>(o_sel);
    uint64_t* const d_pre = d.as<uint64_t>(o_pre);
    uint32_t* const d_bins = d.as<uint32_t>(o_bins);
    const StScratch s = {d.as<int>(o_cnt), d.as<int>(o_minx), d.as<int>(o_maxx), d.as<long long>(o_sumx), nullptr, nullptr, nullptr};
    const unsigned hist_blocks = (unsigned)(rows < (size_t)kLsHistMaxBlocks ? rows : (size_t)kLsHistMaxBlocks);
    const size_t hist_lds = (size_t)R * kSdDigits * sizeof(uint32_t);
    for (const LsChunk& ch : chunks) {
        const unsigned labels = (unsigned)(ch.k1 - ch.k0);
        const dim3 block(kStLanes);
        const FoldedGrid fg = fold_grid((long long)rows, kStLanes);
        // counts and boxes: the counting pass of ts2d_label_statistics without a channel
        hipLaunchKernelGGL(stats_rows<1>, dim3(fg.x, labels, fg.fold), block, 0, 0, d_seg, kind, d_values, ch.k0, (int)rows, W, (long long)n,
                           (const float*)nullptr, 0, s, (const double*)nullptr, d_status);
        hipLaunchKernelGGL(stats_combine<1>, dim3(labels), block, 0, 0, ch.k0, (int)rows, H, Z, W, 0, s, d_int, (double*)nullptr);
        hipLaunchKernelGGL(ls_select_init, dim3(labels), block, 0, 0, d_int, ch.k0, C, pc, P, d_sel, d_pre, d.as<double>(o_wgt));
        for (int rnd = 0; rnd < kLsRounds; ++rnd) {
            hipLaunchKernelGGL(ls_select_hist, dim3(hist_blocks, (unsigned)C, labels), block, hist_lds, 0, d_seg, kind, d_values, ch.k0, Z, H, W,
                               (long long)n, d_x, d_int, R, rnd, d_pre, d_bins, d_status);
            hipLaunchKernelGGL(ls_select_decide, dim3((unsigned)R, (unsigned)C, labels), block, 0, 0, R, rnd, d_sel, d_pre, d_bins);
        }
        hipLaunchKernelGGL(ls_select_write, dim3(labels), block, 0, 0, d_int, ch.k0, C, R, d_pre, d.as<float>(o_rank));
        HIP_TRY(hipGetLastError());
    }
    int st = 0;
    HIP_TRY(hipMemcpy(&st, d_status, sizeof(st), hipMemcpyDeviceToHost));      // (waits for the launches: the default stream orders them)
    if (st) { *status = st; return TS2D_OK; }                                    // a non-finite intensity under a label: the outputs stay as they were
    // one download: counts and boxes, rank values and weights lie next to each other (the gaps of the alignment go along)
    std::vector<char> host(o_seg - o_int);
    HIP_TRY(hipMemcpy(host.data(), d.as<char>(o_int), host.size(), hipMemcpyDeviceToHost));
    for (int k = 0; k < K; ++k) memcpy(out_count + k, host.data() + (size_t)k * kStInts * sizeof(int64_t), sizeof(int64_t));
    memcpy(out_rank_f32, host.data() + (o_rank - o_int), (size_t)K * C * R * sizeof(float));
    memcpy(out_weight_f64, host.data() + (o_wgt - o_int), (size_t)K * P * sizeof(double));
    return TS2D_OK;
}
