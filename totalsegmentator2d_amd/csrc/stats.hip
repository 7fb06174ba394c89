// Per-label statistics of a segmentation, which need no engine: ts2d_label_statistics (kernels_stats.h; the tree of its float64 sums:
// stats_tree.h; the statement: totalsegmentator2d_amd/statistics.py).  Host pointers in and out, one call = one upload, every label on the
// device in chunks of labels whose row partials stay below max_scratch_bytes, one download; every device buffer of the call is one DevMem,
// so HIP_TRY may return wherever it fails.
#include "engine_internal.h"
#include "entry_util.h"
#include "kernels_stats.h"

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
    // a label's row partials: count, min x, max x (int32), sum x (int64), and per channel one float64 and two keys
    const size_t per_label = R * (20 + 16 * (size_t)C);
    size_t budget = 0;
    size_t L = labels_per_chunk(max_scratch_bytes, per_label, K, &budget);
    if (L < 1)
        return fail(TS2D_ERR_INVALID, "%s: the row partials of ONE label (%zu rows, %d channels) take %zu bytes, above max_scratch_bytes = %zu", entry,
                    R, C, per_label, budget);
    const size_t slot_cap = (size_t)0x7FFFFFFF / (R * (size_t)(C > 0 ? C : 1));       // int32 slots: L * C * R stays below 2^31
    if (slot_cap < 1) return fail(TS2D_ERR_INVALID, "%s: %zu rows x %d channels are more partial slots than an int32 index reaches", entry, R, C);
    if (L > slot_cap) L = slot_cap;

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
        const dim3 rows((unsigned)R, labels), block(kStLanes);
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
