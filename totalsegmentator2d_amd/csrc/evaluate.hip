// Scoring a segmentation against a reference, none of which needs an engine: ts2d_project_labels_coronal, ts2d_label_overlap and the boundary
// distances (kernels_evaluate.h; what their profile adds: kernels_evaluate_profile.h).  ts2d_surface_distances and ts2d_surface_distance_profile
// are ONE implementation, surface_distances_impl: the first is the second without percentiles and without the sum.
// ts2d_volume_surface_distances is their counterpart for volumes (kernels_evaluate_volume.h; the plan of its scratch: evaluate_plan.h): the same
// checks (check_distance_request), the same counters, selections and download (DistanceResults).  The arithmetic of the
// distances: surface_dist.h; the statements: totalsegmentator2d_amd/evaluate.py.  ts2d_label_confusion stands beside ts2d_label_overlap: the
// matrix of all label pairs as one integer matrix product (kernels_confusion.h; what a row is as operand bytes: confusion.h).
// Host pointers in and out; a call uploads each input once, works on the device and downloads once; every device buffer of a call is one DevMem
// laid out by an ArenaLayout (entry_util.h), so HIP_TRY may return wherever it fails.
#include "engine_internal.h"
#include "entry_util.h"
#include "kernels_confusion.h"
#include "kernels_evaluate.h"
#include "kernels_evaluate_profile.h"
#include "kernels_evaluate_volume.h"

#include <cstring>
#include <type_traits>
#include <vector>

using namespace ts2d;

static_assert(kStPlanes == TS2D_STATS_PLANES && kStLabelMap == TS2D_STATS_LABELMAP, "the kinds speak the C header's numbers");
static_assert(kPlStatusRange == TS2D_LABELS_RANGE && kSdMaxTolerances == TS2D_EVAL_MAX_TOLERANCES && kSdMaxExtent == TS2D_EVAL_MAX_EXTENT,
              "the status bit and the limits speak the C header's numbers");
static_assert(kSdMaxPercentiles == TS2D_EVAL_MAX_PERCENTILES, "the limits speak the C header's numbers");
static_assert(kCfPlanes == TS2D_STATS_PLANES && kCfLabelMap == TS2D_STATS_LABELMAP, "confusion.h speaks the C header's kinds");
static_assert(kCfChunkMin % 128 == 0 && kCfChunkMin % kCfStep == 0 && kCfStep == 2 * kCfLoad, "a chunk is whole lines and whole steps");

#pragma GCC visibility push(hidden)
namespace {

template <typename T>
void project_labels_launch(const T* d_vol, int nz, int ny, int nx, long long sz, long long sy, long long sx, long long base, int num, uint8_t* d_out,
                           int* d_status) {
    const long long N = (long long)nz * nx, quads = (N + 3) / 4;
    const dim3 grid((unsigned)((quads + kPlThreads - 1) / kPlThreads)), block(kPlThreads);
    const int vec = N % 4 == 0 ? 1 : 0;
    if (num <= 32) hipLaunchKernelGGL((project_labels_stream<T, 1>), grid, block, 0, 0, d_vol, nz, ny, nx, sz, sy, sx, base, num, vec, d_out, d_status);
    else if (num <= 64) hipLaunchKernelGGL((project_labels_stream<T, 2>), grid, block, 0, 0, d_vol, nz, ny, nx, sz, sy, sx, base, num, vec, d_out, d_status);
    else if (num <= 128) hipLaunchKernelGGL((project_labels_stream<T, 4>), grid, block, 0, 0, d_vol, nz, ny, nx, sz, sy, sx, base, num, vec, d_out, d_status);
    else hipLaunchKernelGGL((project_labels_stream<T, 8>), grid, block, 0, 0, d_vol, nz, ny, nx, sz, sy, sx, base, num, vec, d_out, d_status);
}

// the checks the two scoring entries share; *seg_a, *seg_b: the bytes of either input
int check_sides(const char* entry, const void* a, int kind_a, const void* b, int kind_b, const uint8_t* values, int K, size_t n, size_t* seg_a,
                size_t* seg_b) {
    if (!a || !b) return fail(TS2D_ERR_INVALID, "%s: null segmentation", entry);
    if (!label_kind(kind_a) || !label_kind(kind_b))
        return fail(TS2D_ERR_INVALID, "%s: kinds %d, %d are not planes (0) or label map (1)", entry, kind_a, kind_b);
    TRY(check_label_count(entry, K));
    if (kind_a == kStLabelMap || kind_b == kStLabelMap) TRY(check_label_values(entry, values, K));
    *seg_a = kind_a == kStPlanes ? (size_t)K * n : n;
    *seg_b = kind_b == kStPlanes ? (size_t)K * n : n;
    return TS2D_OK;
}

// What the distance entries ask of their tolerances, percentiles and outputs, alike (the extents and the spacings: each its own).
int check_distance_request(const char* E, const double* tol_sq, int T, const double* percentiles, int P, int want_sum, const int64_t* out_i64,
                           const double* out_f64, const double* out_sum_f64, const double* out_rank_f64, const double* out_weight_f64,
                           SdTolerances* tol, SdPercentiles* pc) {
    if (T < 0 || T > kSdMaxTolerances || (T > 0 && !tol_sq)) return fail(TS2D_ERR_INVALID, "%s: T = %d tolerances outside 0 ... %d, or without tol_sq", E, T, kSdMaxTolerances);
    for (int t = 0; t < T; ++t) {
        if (!(tol_sq[t] >= 0.0)) return fail(TS2D_ERR_INVALID, "%s: tol_sq[%d] = %g is negative or not a number", E, t, tol_sq[t]);
        tol->sq[t] = tol_sq[t];
    }
    if (P < 0 || P > kSdMaxPercentiles || (P > 0 && !percentiles))
        return fail(TS2D_ERR_INVALID, "%s: P = %d percentiles outside 0 ... %d, or without percentiles", E, P, kSdMaxPercentiles);
    for (int p = 0; p < P; ++p) {
        if (!(percentiles[p] >= 0.0 && percentiles[p] <= 100.0)) return fail(TS2D_ERR_INVALID, "%s: percentiles[%d] = %g outside 0 ... 100", E, p, percentiles[p]);
        pc->q[p] = percentiles[p];
    }
    if ((P > 0 && (!out_rank_f64 || !out_weight_f64)) || (want_sum && !out_sum_f64))
        return fail(TS2D_ERR_INVALID, "%s: null output for the %s", E, want_sum && !out_sum_f64 ? "sum" : "percentiles");
    return TS2D_OK;
}

// The results of a distance call on the device, [counts | keys | sums | prefixes | weights || ranks | bins]: what is downloaded - in ONE copy,
// the gaps of the alignment go along - then what more starts as zero.  add() puts them at the head of the call's layout.
struct DistanceResults {
    int K, T, P, R, want_sum;
    size_t n_cnt, n_sel, pairs, o_cnt, o_key, o_sum, o_pre, o_wgt, down_bytes, o_rank, o_bins, zero_bytes;
    void add(ArenaLayout& lay, int K_, int T_, int P_, int want_sum_, size_t bins_bytes) {
        K = K_; T = T_; P = P_; R = 2 * P_; want_sum = want_sum_;
        n_cnt = (size_t)K * 2 * (1 + T); n_sel = (size_t)K * 2 * R; pairs = (size_t)K * 2;
        o_cnt = lay.add(n_cnt * sizeof(unsigned long long)); o_key = lay.add(pairs * sizeof(unsigned long long));
        o_sum = lay.add(want_sum ? pairs * sizeof(double) : 0); o_pre = lay.add(n_sel * sizeof(uint64_t));
        o_wgt = lay.add(pairs * P * sizeof(double)); down_bytes = lay.total();
        o_rank = lay.add(n_sel * sizeof(long long)); o_bins = lay.add(bins_bytes);
        zero_bytes = lay.total();
    }
    // the download and the outputs: an empty border reports -inf for its largest d2 and its ranks
    int finish(const DevMem& d, int64_t* out_i64, double* out_f64, double* out_sum_f64, double* out_rank_f64, double* out_weight_f64) const {
        std::vector<char> host(down_bytes);
        HIP_TRY(hipMemcpy(host.data(), d.as<char>(), host.size(), hipMemcpyDeviceToHost));
        memcpy(out_i64, host.data() + o_cnt, n_cnt * sizeof(int64_t));
        const uint64_t minus_inf = 0xFFF0000000000000ull;
        for (size_t i = 0; i < pairs; ++i) {
            long long border;
            uint64_t key;
            memcpy(&border, host.data() + o_cnt + i * (1 + T) * sizeof(int64_t), sizeof(border));
            memcpy(&key, host.data() + o_key + i * sizeof(uint64_t), sizeof(key));
            if (border == 0) key = minus_inf;                                          // an empty border: -inf
            memcpy(out_f64 + i, &key, sizeof(key));
            for (int r = 0; r < R; ++r) {
                memcpy(&key, host.data() + o_pre + (i * R + r) * sizeof(uint64_t), sizeof(key));
                if (border == 0) key = minus_inf;
                memcpy(out_rank_f64 + i * R + r, &key, sizeof(key));
            }
        }
        if (want_sum) memcpy(out_sum_f64, host.data() + o_sum, pairs * sizeof(double));
        if (P) memcpy(out_weight_f64, host.data() + o_wgt, pairs * P * sizeof(double));
        return TS2D_OK;
    }
};

// The selection of one (chunk of) key buffer(s) [L][2][n]: eight rounds of histogram and decision for the labels k0 ... k0 + L - 1.
void select_rounds(const uint64_t* d_kbuf, int k0, unsigned L, long long n, int R, long long* d_rank, uint64_t* d_pre, uint32_t* d_bins) {
    size_t hist_blocks = ((size_t)n + 1023) / 1024;                                  // 16 keys per lane, up to the cap
    if (hist_blocks > (size_t)kSpHistMaxBlocks) hist_blocks = kSpHistMaxBlocks;
    for (int rnd = 0; rnd < kSdRounds; ++rnd) {
        hipLaunchKernelGGL(sd_select_hist, dim3((unsigned)hist_blocks, 2, L), dim3(64), 0, 0, d_kbuf, k0, n, R, rnd, d_rank, d_pre, d_bins);
        hipLaunchKernelGGL(sd_select_decide, dim3((unsigned)R, 2, L), dim3(64), 0, 0, k0, R, rnd, d_rank, d_pre, d_bins);
    }
}

// ts2d_surface_distances (E names it; P = 0, want_sum = 0, the three outputs of the profile null) and ts2d_surface_distance_profile.
int surface_distances_impl(const char* E, int device, const uint8_t* a, int kind_a, const uint8_t* b, int kind_b, const uint8_t* values, int K, int H,
                           int W, double spacing_h, double spacing_w, const double* tol_sq, int T, const double* percentiles, int P, int want_sum,
                           size_t max_scratch_bytes, int64_t* out_i64, double* out_f64, double* out_sum_f64, double* out_rank_f64,
                           double* out_weight_f64) {
    if (!out_i64 || !out_f64) return fail(TS2D_ERR_INVALID, "%s: null output", E);
    if (H < 1 || W < 1 || H > kSdMaxExtent || W > kSdMaxExtent) return fail(TS2D_ERR_INVALID, "%s: %d x %d outside 1 ... %d per axis", E, H, W, kSdMaxExtent);
    if (!(spacing_h > 0.0 && spacing_h < 1e300 && spacing_w > 0.0 && spacing_w < 1e300))
        return fail(TS2D_ERR_INVALID, "%s: spacing %g x %g is not finite and positive", E, spacing_h, spacing_w);
    SdTolerances tol = {};
    SdPercentiles pc = {};
    TRY(check_distance_request(E, tol_sq, T, percentiles, P, want_sum, out_i64, out_f64, out_sum_f64, out_rank_f64, out_weight_f64, &tol, &pc));
    const size_t n = (size_t)H * W;
    size_t bytes_a = 0, bytes_b = 0;
    TRY(check_sides(E, a, kind_a, b, kind_b, values, K, n, &bytes_a, &bytes_b));
    // a label's scratch: the border bytes and the uint16 row distances of both sides; with percentiles the keys of both directions and the bins
    // of its 2 * 2 P selections; with the sum the row partials of both directions
    const int R = 2 * P;
    const size_t bins_label = (size_t)2 * R * kSdDigits * sizeof(uint32_t);
    const size_t per_label = n * 2 * (1 + sizeof(uint16_t)) + (P ? n * 2 * sizeof(uint64_t) + bins_label : 0) + (want_sum ? (size_t)H * 2 * sizeof(double) : 0);
    size_t budget = 0;
    const size_t L = labels_per_chunk(max_scratch_bytes, per_label, K, &budget);
    if (L < 1)
        return fail(TS2D_ERR_INVALID, "%s: the scratch of ONE label (%d x %d) takes %zu bytes, above max_scratch_bytes = %zu", E, H, W, per_label, budget);
    HIP_TRY(hipSetDevice(device));
    // [the results (DistanceResults) | values || a | b | border of a chunk | g | key buffer | row partials]
    ArenaLayout lay;
    DistanceResults res;
    res.add(lay, K, T, P, want_sum, P ? L * bins_label : 0);
    const size_t o_val = lay.add((size_t)K), zero_bytes = lay.total();
    const size_t o_a = lay.add(bytes_a), o_b = lay.add(bytes_b), o_border = lay.add(L * 2 * n), o_g = lay.add(L * 2 * n * sizeof(uint16_t));
    const size_t o_kbuf = lay.add(P ? L * 2 * n * sizeof(uint64_t) : 0), o_rows = lay.add(want_sum ? L * 2 * (size_t)H * sizeof(double) : 0);
    DevMem d;
    HIP_TRY(d.alloc(lay.total()));
    HIP_TRY(hipMemset(d.as<char>(), 0, zero_bytes));
    if (values) HIP_TRY(hipMemcpy(d.as<char>(o_val), values, (size_t)K, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d.as<char>(o_a), a, bytes_a, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d.as<char>(o_b), b, bytes_b, hipMemcpyHostToDevice));
    unsigned long long* const d_cnt = d.as<unsigned long long>(res.o_cnt);
    unsigned long long* const d_key = d.as<unsigned long long>(res.o_key);
    long long* const d_rank = d.as<long long>(res.o_rank);
    uint64_t* const d_pre = d.as<uint64_t>(res.o_pre);
    uint32_t* const d_bins = d.as<uint32_t>(res.o_bins);
    uint64_t* const d_kbuf = P ? d.as<uint64_t>(o_kbuf) : nullptr;
    double* const d_rows = want_sum ? d.as<double>(o_rows) : nullptr;
    const bool profile = P > 0 || want_sum;
    for (int k0 = 0; k0 < K; k0 += (int)L) {
        const unsigned labels = (unsigned)(K - k0 < (int)L ? K - k0 : (int)L);
        hipLaunchKernelGGL(sd_columns, dim3((unsigned)((W + 63) / 64), 2, labels), dim3(64), 0, 0, d.as<const uint8_t>(o_a), kind_a,
                           d.as<const uint8_t>(o_b), kind_b, d.as<const uint8_t>(o_val), k0, H, W, d.as<uint8_t>(o_border), d.as<uint16_t>(o_g));
        hipLaunchKernelGGL(profile ? sd_rows<true> : sd_rows<false>, dim3((unsigned)H, 2, labels), dim3(64), 0, 0, d.as<const uint8_t>(o_border),
                           d.as<const uint16_t>(o_g), k0, H, W, spacing_h, spacing_w, tol, T, d_cnt, d_key, d_kbuf, d_rows);
        if (want_sum) hipLaunchKernelGGL(sd_profile_combine, dim3(2, labels), dim3(64), 0, 0, d_rows, k0, H, d.as<double>(res.o_sum));
        if (P) {
            hipLaunchKernelGGL(sd_select_init, dim3(labels), dim3(64), 0, 0, d_cnt, k0, T, pc, P, d_rank, d_pre, d.as<double>(res.o_wgt));
            select_rounds(d_kbuf, k0, labels, (long long)n, R, d_rank, d_pre, d_bins);
        }
        HIP_TRY(hipGetLastError());
    }
    return res.finish(d, out_i64, out_f64, out_sum_f64, out_rank_f64, out_weight_f64);
}

// ts2d_volume_surface_distances: box, plan, then per chunk of labels the three passes inside the boxes and what the profile adds.
int volume_distances_impl(const char* E, int device, const uint8_t* a, int kind_a, const uint8_t* b, int kind_b, const uint8_t* values, int K, int Z,
                          int H, int W, double spacing_z, double spacing_h, double spacing_w, const double* tol_sq, int T, const double* percentiles,
                          int P, int want_sum, size_t max_scratch_bytes, int64_t* out_i64, double* out_f64, double* out_sum_f64, double* out_rank_f64,
                          double* out_weight_f64) {
    if (!out_i64 || !out_f64) return fail(TS2D_ERR_INVALID, "%s: null output", E);
    if (Z < 1 || H < 1 || W < 1 || Z > kSdMaxExtent || H > kSdMaxExtent || W > kSdMaxExtent)
        return fail(TS2D_ERR_INVALID, "%s: %d x %d x %d outside 1 ... %d per axis", E, Z, H, W, kSdMaxExtent);
    if (!volume_fits_int32(Z, H, W)) return fail(TS2D_ERR_INVALID, "%s: %d x %d x %d is more than 2^31 - 1 voxels", E, Z, H, W);
    if (!(spacing_z > 0.0 && spacing_z < 1e300 && spacing_h > 0.0 && spacing_h < 1e300 && spacing_w > 0.0 && spacing_w < 1e300))
        return fail(TS2D_ERR_INVALID, "%s: spacing %g x %g x %g is not finite and positive", E, spacing_z, spacing_h, spacing_w);
    SdTolerances tol = {};
    SdPercentiles pc = {};
    TRY(check_distance_request(E, tol_sq, T, percentiles, P, want_sum, out_i64, out_f64, out_sum_f64, out_rank_f64, out_weight_f64, &tol, &pc));
    const size_t n = (size_t)Z * H * W;
    size_t bytes_a = 0, bytes_b = 0;
    TRY(check_sides(E, a, kind_a, b, kind_b, values, K, n, &bytes_a, &bytes_b));
    const size_t budget = max_scratch_bytes ? max_scratch_bytes : ((size_t)4 << 30);
    const int R = 2 * P;
    HIP_TRY(hipSetDevice(device));
    // [the results (DistanceResults; ONE label's bins: the selections run label by label) | values || the boxes || a | b]
    ArenaLayout lay;
    DistanceResults res;
    res.add(lay, K, T, P, want_sum, P ? (size_t)2 * R * kSdDigits * sizeof(uint32_t) : 0);
    const size_t o_val = lay.add((size_t)K), zero_bytes = lay.total();
    const size_t box_bytes = (size_t)K * 6 * sizeof(int32_t), o_box = lay.add(box_bytes), o_a = lay.add(bytes_a), o_b = lay.add(bytes_b);
    DevMem d;
    HIP_TRY(d.alloc(lay.total()));
    HIP_TRY(hipMemset(d.as<char>(), 0, zero_bytes));
    HIP_TRY(hipMemset(d.as<char>(o_box), 0xFF, box_bytes));                             // smallest: UINT32_MAX; largest: -1
    if (values) HIP_TRY(hipMemcpy(d.as<char>(o_val), values, (size_t)K, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d.as<char>(o_a), a, bytes_a, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d.as<char>(o_b), b, bytes_b, hipMemcpyHostToDevice));
    const uint8_t* const d_a = d.as<const uint8_t>(o_a);
    const uint8_t* const d_b = d.as<const uint8_t>(o_b);
    const uint8_t* const d_val = d.as<const uint8_t>(o_val);
    {
        const int vec = n % 16 == 0 ? 1 : 0;
        const size_t units = vec ? n / 16 : n;
        size_t blocks = (units + kSdvBoxThreads - 1) / kSdvBoxThreads;
        if (blocks > (size_t)kSdvBoxMaxBlocks) blocks = kSdvBoxMaxBlocks;
        hipLaunchKernelGGL(sdv_box, dim3((unsigned)blocks, (unsigned)K), dim3(kSdvBoxThreads), 0, 0, d_a, kind_a, d_b, kind_b, d_val, (long long)n, H, W,
                           vec, d.as<uint32_t>(o_box));
        HIP_TRY(hipGetLastError());
    }
    std::vector<int32_t> box((size_t)K * 6);
    HIP_TRY(hipMemcpy(box.data(), d.as<char>(o_box), box_bytes, hipMemcpyDeviceToHost));
    std::vector<SdvLabel> labels;
    std::vector<SdvChunk> chunks;
    size_t need = 0;
    const int over = sdv_plan(box.data(), K, P, want_sum, budget, &labels, &chunks, &need);
    if (over >= 0)
        return fail(TS2D_ERR_INVALID, "%s: the scratch of ONE label (label %d, its box %d x %d x %d) takes %zu bytes, above max_scratch_bytes = %zu", E,
                    over, box[(size_t)over * 6 + 3] - box[(size_t)over * 6] + 1, box[(size_t)over * 6 + 4] - box[(size_t)over * 6 + 1] + 1,
                    box[(size_t)over * 6 + 5] - box[(size_t)over * 6 + 2] + 1, need, budget);
    // sdv_planes and sdv_rows run one wave per (group of) box row(s): a box of more than 2^26 - 1 rows (W < 32 at the largest extents) would be a
    // launch of more than 2^32 - 1 threads, which the runtime does not refuse but cuts short
    for (int k = 0; k < K; ++k) {
        const SdvLabel& l = labels[(size_t)k];
        const long long pl = (long long)((l.bx + 63) / 64) * ((l.by + kSdvRows - 1) / kSdvRows) * l.bz, rw = (long long)l.bz * l.by;
        if ((pl > rw ? pl : rw) * 64 > 0xFFFFFFFFll)
            return fail(TS2D_ERR_INVALID, "%s: label %d: its box %d x %d x %d has %lld rows, above the 67108863 rows one launch takes", E, k, l.bz, l.by,
                        l.bx, rw);
    }
    long long max_vox = 0, max_rows = 0;
    for (const SdvChunk& c : chunks) {
        max_vox = c.vox > max_vox ? c.vox : max_vox;
        max_rows = c.rows > max_rows ? c.rows : max_rows;
    }
    // the scratch of the largest chunk: [descriptors | border | g | h | key buffer | row partials]
    ArenaLayout slay;
    const size_t o_lab = slay.add((size_t)K * sizeof(SdvLabel)), o_border = slay.add((size_t)max_vox * 2), o_g = slay.add((size_t)max_vox * 2 * sizeof(uint16_t));
    const size_t o_h = slay.add((size_t)max_vox * 2 * sizeof(double)), o_kbuf = slay.add(P ? (size_t)max_vox * 2 * sizeof(uint64_t) : 0);
    const size_t o_rows = slay.add(want_sum ? (size_t)max_rows * 2 * sizeof(double) : 0);
    DevMem s;
    HIP_TRY(s.alloc(slay.total()));
    HIP_TRY(hipMemcpy(s.as<char>(o_lab), labels.data(), (size_t)K * sizeof(SdvLabel), hipMemcpyHostToDevice));
    unsigned long long* const d_cnt = d.as<unsigned long long>(res.o_cnt);
    unsigned long long* const d_key = d.as<unsigned long long>(res.o_key);
    long long* const d_rank = d.as<long long>(res.o_rank);
    uint64_t* const d_pre = d.as<uint64_t>(res.o_pre);
    uint32_t* const d_bins = d.as<uint32_t>(res.o_bins);
    uint64_t* const d_kbuf = P ? s.as<uint64_t>(o_kbuf) : nullptr;
    double* const d_rows = want_sum ? s.as<double>(o_rows) : nullptr;
    const bool profile = P > 0 || want_sum;
    for (const SdvChunk& c : chunks) {
        if (c.vox == 0) continue;                                  // none of its labels has a voxel on either side: the zeros stand
        const unsigned L = (unsigned)(c.k1 - c.k0);
        const SdvLabel* const d_lab = s.as<const SdvLabel>(o_lab) + c.k0;
        long long lines = 0, planes = 0, rows = 0;                 // the largest grids among the chunk's labels
        for (int k = c.k0; k < c.k1; ++k) {
            const SdvLabel& l = labels[(size_t)k];
            const long long ln = ((long long)l.by * l.bx + 63) / 64;
            const long long pl = (long long)((l.bx + 63) / 64) * ((l.by + kSdvRows - 1) / kSdvRows) * l.bz, rw = (long long)l.bz * l.by;
            lines = ln > lines ? ln : lines; planes = pl > planes ? pl : planes; rows = rw > rows ? rw : rows;
        }
        hipLaunchKernelGGL(sdv_lines, dim3((unsigned)lines, 2, L), dim3(64), 0, 0, d_a, kind_a, d_b, kind_b, d_val, d_lab, c.k0, Z, H, W,
                           s.as<uint8_t>(o_border), s.as<uint16_t>(o_g));
        hipLaunchKernelGGL(sdv_planes, dim3((unsigned)planes, 2, L), dim3(64), 0, 0, s.as<const uint16_t>(o_g), d_lab, spacing_z, spacing_h,
                           s.as<double>(o_h));
        hipLaunchKernelGGL(profile ? sdv_rows<true> : sdv_rows<false>, dim3((unsigned)rows, 2, L), dim3(64), 0, 0, s.as<const uint8_t>(o_border),
                           s.as<const double>(o_h), d_lab, c.k0, spacing_w, tol, T, d_cnt, d_key, d_kbuf, d_rows);
        if (want_sum) hipLaunchKernelGGL(sdv_profile_combine, dim3(2, L), dim3(64), 0, 0, d_rows, d_lab, c.k0, H, d.as<double>(res.o_sum));
        if (P) {
            hipLaunchKernelGGL(sd_select_init, dim3(L), dim3(64), 0, 0, d_cnt, c.k0, T, pc, P, d_rank, d_pre, d.as<double>(res.o_wgt));
            for (int k = c.k0; k < c.k1; ++k) {                    // a label's keys: [2][its box voxels], one "chunk of one" to the selection
                const SdvLabel& l = labels[(size_t)k];
                if (l.bz) select_rounds(d_kbuf + 2 * l.vox, k, 1, (long long)l.bz * l.by * l.bx, R, d_rank, d_pre, d_bins);
            }
        }
        HIP_TRY(hipGetLastError());
    }
    return res.finish(d, out_i64, out_f64, out_sum_f64, out_rank_f64, out_weight_f64);
}

}  // namespace
#pragma GCC visibility pop

extern "C" {

int ts2d_project_labels_coronal(int device, const void* volume, size_t n_elems, int dtype, int nz, int ny, int nx, long long sz, long long sy,
                                long long sx, long long base, int num, uint8_t* planes_u8, int32_t* status) {
    const char* const E = "ts2d_project_labels_coronal";
    if (!volume || !planes_u8 || !status) return fail(TS2D_ERR_INVALID, "%s: null argument", E);
    if (dtype < 0 || dtype > 4 || dtype == 2) return fail(TS2D_ERR_INVALID, "%s: dtype %d is not an integer type (int16 0, uint8 1, uint16 3, int32 4)", E, dtype);
    if (num < 1 || num > 255) return fail(TS2D_ERR_INVALID, "%s: num = %d outside 1 ... 255", E, num);
    if (nz < 1 || ny < 1 || nx < 1) return fail(TS2D_ERR_INVALID, "%s: extents nz %d, ny %d, nx %d below 1", E, nz, ny, nx);
    if ((long long)nz * nx * num > 0x7FFFFFFFll) return fail(TS2D_ERR_INVALID, "%s: %d planes of nz %d x nx %d are more than 2^31 - 1 bytes", E, num, nz, nx);
    TRY(check_strided_view(E, n_elems, base, {nz, ny, nx}, {sz, sy, sx}));
    *status = 0;
    HIP_TRY(hipSetDevice(device));
    const size_t vbytes = n_elems * sample_size(dtype), obytes = (size_t)nz * nx * num;
    ArenaLayout lay;
    const size_t o_status = lay.add(sizeof(int)), o_vol = lay.add(vbytes), o_out = lay.add(obytes);
    DevMem d;
    HIP_TRY(d.alloc(lay.total()));
    int* d_status = d.as<int>(o_status);
    uint8_t* d_out = d.as<uint8_t>(o_out);
    HIP_TRY(hipMemset(d_status, 0, sizeof(int)));
    HIP_TRY(hipMemcpy(d.as<char>(o_vol), volume, vbytes, hipMemcpyHostToDevice));
    by_sample_type(dtype, [&](auto t) {
        using S = typename decltype(t)::type;
        if constexpr (std::is_integral<S>::value)                  // (float32 was refused above: no kernel of it is built)
            project_labels_launch(d.as<const S>(o_vol), nz, ny, nx, sz, sy, sx, base, num, d_out, d_status);
    });
    HIP_TRY(hipGetLastError());
    int st = 0;
    HIP_TRY(hipMemcpy(&st, d_status, sizeof(st), hipMemcpyDeviceToHost));       // (waits for the launch: the default stream orders them)
    if (st) { *status = st; return TS2D_OK; }                                     // a sample outside 0 ... num: the planes are no result
    HIP_TRY(hipMemcpy(planes_u8, d_out, obytes, hipMemcpyDeviceToHost));
    return TS2D_OK;
}

int ts2d_label_overlap(int device, const uint8_t* a, int kind_a, const uint8_t* b, int kind_b, const uint8_t* values, int K, int Z, int H, int W,
                       int64_t* out_i64) {
    const char* const E = "ts2d_label_overlap";
    if (!out_i64) return fail(TS2D_ERR_INVALID, "%s: out_i64 is null", E);
    if (!volume_fits_int32(Z, H, W)) return fail(TS2D_ERR_INVALID, "%s: %d x %d x %d is empty or more than 2^31 - 1 samples", E, Z, H, W);
    const size_t n = (size_t)Z * H * W;
    size_t bytes_a = 0, bytes_b = 0;
    TRY(check_sides(E, a, kind_a, b, kind_b, values, K, n, &bytes_a, &bytes_b));
    HIP_TRY(hipSetDevice(device));
    ArenaLayout lay;
    const size_t o_cnt = lay.add((size_t)K * 3 * sizeof(unsigned long long)), o_val = lay.add((size_t)K);
    const size_t o_a = lay.add(bytes_a), o_b = lay.add(bytes_b);
    DevMem d;
    HIP_TRY(d.alloc(lay.total()));
    HIP_TRY(hipMemset(d.as<char>(), 0, o_a));                      // the counts and the values
    if (values) HIP_TRY(hipMemcpy(d.as<char>(o_val), values, (size_t)K, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d.as<char>(o_a), a, bytes_a, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d.as<char>(o_b), b, bytes_b, hipMemcpyHostToDevice));
    const int vec = n % 16 == 0 ? 1 : 0;
    const size_t units = vec ? n / 16 : n;
    size_t blocks = (units + kOvThreads - 1) / kOvThreads;
    if (blocks > (size_t)kOvMaxBlocks) blocks = kOvMaxBlocks;
    hipLaunchKernelGGL(overlap_count, dim3((unsigned)blocks, (unsigned)K), dim3(kOvThreads), 0, 0, d.as<const uint8_t>(o_a), kind_a,
                       d.as<const uint8_t>(o_b), kind_b, d.as<const uint8_t>(o_val), (long long)n, vec, d.as<unsigned long long>(o_cnt));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(out_i64, d.as<char>(o_cnt), (size_t)K * 3 * sizeof(int64_t), hipMemcpyDeviceToHost));
    return TS2D_OK;
}

int ts2d_label_confusion(int device, const uint8_t* a, int kind_a, const uint8_t* b, int kind_b, const uint8_t* values, int K, int Z, int H, int W,
                         int64_t* out_i64) {
    const char* const E = "ts2d_label_confusion";
    if (!out_i64) return fail(TS2D_ERR_INVALID, "%s: out_i64 is null", E);
    if (!volume_fits_int32(Z, H, W)) return fail(TS2D_ERR_INVALID, "%s: %d x %d x %d is empty or more than 2^31 - 1 samples", E, Z, H, W);
    const size_t n = (size_t)Z * H * W;
    size_t bytes_a = 0, bytes_b = 0;
    TRY(check_sides(E, a, kind_a, b, kind_b, values, K, n, &bytes_a, &bytes_b));
    const bool same = a == b && kind_a == kind_b;                  // ONE array on both sides: one upload, one none plane
    const bool any_map = kind_a == kStLabelMap || kind_b == kStLabelMap;
    uint32_t set[8] = {};
    if (any_map) cf_set_build(values, K, set);
    HIP_TRY(hipSetDevice(device));
    // [the matrix | values | the set of the values || a | b | none of a | none of b]
    const size_t rows = (size_t)K + 2, cnt_bytes = rows * rows * sizeof(unsigned long long);
    ArenaLayout lay;
    const size_t o_cnt = lay.add(cnt_bytes), o_val = lay.add((size_t)K), o_set = lay.add(sizeof(set));
    const size_t o_a = lay.add(bytes_a), o_b = same ? o_a : lay.add(bytes_b), o_na = lay.add(n), o_nb = same ? o_na : lay.add(n);
    DevMem d;
    HIP_TRY(d.alloc(lay.total()));
    HIP_TRY(hipMemset(d.as<char>(), 0, o_set));                    // the matrix and the values
    if (values) HIP_TRY(hipMemcpy(d.as<char>(o_val), values, (size_t)K, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d.as<char>(o_set), set, sizeof(set), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d.as<char>(o_a), a, bytes_a, hipMemcpyHostToDevice));
    if (!same) HIP_TRY(hipMemcpy(d.as<char>(o_b), b, bytes_b, hipMemcpyHostToDevice));
    const int aligned = n % kCfLoad == 0 ? 1 : 0;                  // every region starts on a 256-byte boundary: plane k on one of 16 iff n is a multiple
    // Neither launch comes near the 2^32 lanes of one axis, where a grid would have to be folded (entry_util.h, fold_grid): n <= 2^31 - 1, a lane
    // of cf_none takes 16 samples (at most 2^27 lanes along x) and a wave of cf_product at least kCfChunkMin = 1024 (at most 2^21 waves, 2^27 lanes;
    // along y the at most 81 tile pairs).
    const unsigned none_blocks = (unsigned)(((n + kCfLoad - 1) / kCfLoad + kCfNoneThreads - 1) / kCfNoneThreads);
    hipLaunchKernelGGL(cf_none, dim3(none_blocks), dim3(kCfNoneThreads), 0, 0, d.as<const uint8_t>(o_a), kind_a, K, (long long)n, aligned,
                       d.as<const uint32_t>(o_set), d.as<uint8_t>(o_na));
    if (!same)
        hipLaunchKernelGGL(cf_none, dim3(none_blocks), dim3(kCfNoneThreads), 0, 0, d.as<const uint8_t>(o_b), kind_b, K, (long long)n, aligned,
                           d.as<const uint32_t>(o_set), d.as<uint8_t>(o_nb));
    HIP_TRY(hipGetLastError());
    const int tiles = (int)((rows + kCfTile - 1) / kCfTile), pairs = tiles * tiles;
    const long long per_pair = kCfWavesAim / pairs > 0 ? kCfWavesAim / pairs : 1;
    long long chunk = ((long long)n + per_pair - 1) / per_pair;
    chunk = chunk < kCfChunkMin ? kCfChunkMin : (chunk + 127) / 128 * 128;
    hipLaunchKernelGGL(cf_product, dim3((unsigned)(((long long)n + chunk - 1) / chunk), (unsigned)pairs), dim3(64), 0, 0, d.as<const uint8_t>(o_a), kind_a, d.as<const uint8_t>(o_na),
                       d.as<const uint8_t>(o_b), kind_b, d.as<const uint8_t>(o_nb), d.as<const uint8_t>(o_val), K, (long long)n, chunk, tiles, aligned,
                       aligned, d.as<unsigned long long>(o_cnt));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(out_i64, d.as<char>(o_cnt), cnt_bytes, hipMemcpyDeviceToHost));
    return TS2D_OK;
}


int ts2d_surface_distances(int device, const uint8_t* a, int kind_a, const uint8_t* b, int kind_b, const uint8_t* values, int K, int H, int W,
                           double spacing_h, double spacing_w, const double* tol_sq, int T, size_t max_scratch_bytes, int64_t* out_i64,
                           double* out_f64) {
    return surface_distances_impl("ts2d_surface_distances", device, a, kind_a, b, kind_b, values, K, H, W, spacing_h, spacing_w, tol_sq, T, nullptr, 0, 0,
                                  max_scratch_bytes, out_i64, out_f64, nullptr, nullptr, nullptr);
}

int ts2d_surface_distance_profile(int device, const uint8_t* a, int kind_a, const uint8_t* b, int kind_b, const uint8_t* values, int K, int H,
                                  int W, double spacing_h, double spacing_w, const double* tol_sq, int T, const double* percentiles, int P,
                                  int want_sum, size_t max_scratch_bytes, int64_t* out_i64, double* out_f64, double* out_sum_f64,
                                  double* out_rank_f64, double* out_weight_f64) {
    return surface_distances_impl("ts2d_surface_distance_profile", device, a, kind_a, b, kind_b, values, K, H, W, spacing_h, spacing_w, tol_sq, T,
                                  percentiles, P, want_sum, max_scratch_bytes, out_i64, out_f64, out_sum_f64, out_rank_f64, out_weight_f64);
}

int ts2d_volume_surface_distances(int device, const uint8_t* a, int kind_a, const uint8_t* b, int kind_b, const uint8_t* values, int K, int Z,
                                  int H, int W, double spacing_z, double spacing_h, double spacing_w, const double* tol_sq, int T,
                                  const double* percentiles, int P, int want_sum, size_t max_scratch_bytes, int64_t* out_i64, double* out_f64,
                                  double* out_sum_f64, double* out_rank_f64, double* out_weight_f64) {
    return volume_distances_impl("ts2d_volume_surface_distances", device, a, kind_a, b, kind_b, values, K, Z, H, W, spacing_z, spacing_h, spacing_w, tol_sq,
                                 T, percentiles, P, want_sum, max_scratch_bytes, out_i64, out_f64, out_sum_f64, out_rank_f64, out_weight_f64);
}

}  // extern "C"
