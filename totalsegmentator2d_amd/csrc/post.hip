// The output side behind the export of libts2d_engine.so, which needs no engine: nnU-Net's largest-component postprocessing of a decided label map
// (kernels_post_cc.h), and the components of every label of a segmentation at once with their clean-up rule (kernels_components.h).  One upload,
// every step on the device, one download; every device buffer of a call is a DevMem, so HIP_TRY may return wherever it fails.
#include "engine_internal.h"
#include "entry_util.h"
#include "kernels_components.h"
#include "kernels_post_cc.h"

#include <algorithm>
#include <vector>

using namespace ts2d;

static_assert(kCcStatusGiveUp == TS2D_CC_GIVE_UP, "the status bit speaks the C header's number");
static_assert(sizeof(ts2d_cc_step) == 257, "a step is its 256-byte table and the background byte");

int ts2d_keep_largest_components(int device, uint8_t* seg, int Z, int H, int W, const ts2d_cc_step* steps, int n_steps, int64_t* stats, int* status) {
    const char* const entry = "ts2d_keep_largest_components";
    if (!seg || !status || (!steps && n_steps > 0)) return fail(TS2D_ERR_INVALID, "%s: null argument", entry);
    *status = 0;
    if (Z < 1 || H < 1 || W < 1) return fail(TS2D_ERR_INVALID, "%s: extents %d x %d x %d must be positive", entry, Z, H, W);
    if (!volume_fits_int32(Z, H, W))
        return fail(TS2D_ERR_INVALID, "%s: %d x %d x %d are more voxels than one call takes (2^31 - 1: the indices are int32)", entry, Z, H, W);
    if (n_steps < 0) return fail(TS2D_ERR_INVALID, "%s: %d steps", entry, n_steps);
    if (n_steps == 0) return TS2D_OK;
    HIP_TRY(hipSetDevice(device));
    const size_t n = (size_t)Z * H * W;
    const int ww = (W + 63) >> 6;
    const long long words = (long long)Z * H * ww;
    // [status, counters of every step | the steps | seg | bit words | parent | count]
    const size_t ctr_ints = 1 + (size_t)n_steps * kCcCounters;
    ArenaLayout lay;
    const size_t o_ctr = lay.add(ctr_ints * sizeof(int)), o_steps = lay.add((size_t)n_steps * sizeof(ts2d_cc_step)), o_seg = lay.add(n);
    const size_t o_bits = lay.add((size_t)words * sizeof(cc_word)), o_parent = lay.add(n * sizeof(int)), o_count = lay.add(n * sizeof(int));
    DevMem d;
    HIP_TRY(d.alloc(lay.total()));
    int* const d_status = d.as<int>(o_ctr);
    uint8_t* const d_seg = d.as<uint8_t>(o_seg);
    cc_word* const d_bits = d.as<cc_word>(o_bits);
    int* const d_parent = d.as<int>(o_parent);
    int* const d_count = d.as<int>(o_count);
    HIP_TRY(hipMemset(d_status, 0, ctr_ints * sizeof(int)));
    HIP_TRY(hipMemcpy(d.as<char>(o_steps), steps, (size_t)n_steps * sizeof(ts2d_cc_step), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_seg, seg, n, hipMemcpyHostToDevice));
    const FoldedGrid fg = fold_grid((words + 3) / 4, 256);
    const dim3 grid(fg.x, 1, fg.fold), block(256);
    for (int s = 0; s < n_steps; ++s) {          // each launch sees the one before it: the default stream orders them
        const uint8_t* member = d.as<const uint8_t>(o_steps + (size_t)s * sizeof(ts2d_cc_step));
        int* ctr = d_status + 1 + (size_t)s * kCcCounters;
        hipLaunchKernelGGL(cc_mask_init, grid, block, 0, 0, d_seg, member, W, words, d_bits, d_parent, d_count, ctr);
        hipLaunchKernelGGL(cc_link, grid, block, 0, 0, d_bits, d_parent, H, W, words, d_status);
        hipLaunchKernelGGL(cc_flatten, grid, block, 0, 0, d_parent, W, words, ctr, d_status);
        hipLaunchKernelGGL(cc_count, grid, block, 0, 0, d_parent, W, words, d_count);
        hipLaunchKernelGGL(cc_max, grid, block, 0, 0, d_parent, d_count, W, words, ctr);
        hipLaunchKernelGGL(cc_apply, grid, block, 0, 0, d_seg, d_parent, d_count, W, words, steps[s].background, ctr, d_status);
        HIP_TRY(hipGetLastError());
    }
    std::vector<int> ctr(ctr_ints);
    HIP_TRY(hipMemcpy(ctr.data(), d_status, ctr_ints * sizeof(int), hipMemcpyDeviceToHost));
    if (ctr[0]) { *status = ctr[0]; return TS2D_OK; }            // a bounded loop reached its cap: the caller's buffer and stats stay as they are
    HIP_TRY(hipMemcpy(seg, d_seg, n, hipMemcpyDeviceToHost));
    if (stats)
        for (size_t k = 0; k < (size_t)n_steps * kCcCounters; ++k) stats[k] = ctr[1 + k];
    return TS2D_OK;
}

static_assert(kLcStatusGiveUp == TS2D_COMP_GIVE_UP && kLcStatusListFull == TS2D_COMP_LIST_FULL, "the status bits speak the C header's numbers");
static_assert(kLcCounters == TS2D_COMP_COUNTERS, "the counters are the C header's");
static_assert(kLcPlanes == TS2D_STATS_PLANES && kLcLabelMap == TS2D_STATS_LABELMAP, "the kinds speak the C header's numbers");
static_assert(kLcFull == TS2D_COMP_FULL && kLcFaces == TS2D_COMP_FACES, "the connectivities speak the C header's numbers");

int ts2d_label_components(int device, const uint8_t* seg, int kind, const uint8_t* values, int K, int Z, int H, int W, int connectivity,
                          int keep_largest, const int64_t* min_voxels, size_t max_scratch_bytes, uint8_t* out_seg, int64_t* out_counters,
                          int64_t* out_components, int64_t capacity, int64_t* out_n_components, int* status) {
    const char* const entry = "ts2d_label_components";
    if (!seg || !out_counters || !out_n_components || !status) return fail(TS2D_ERR_INVALID, "%s: null argument", entry);
    if (!label_kind(kind)) return fail(TS2D_ERR_INVALID, "%s: kind %d is neither planes (0) nor label map (1)", entry, kind);
    if (connectivity != kLcFull && connectivity != kLcFaces)
        return fail(TS2D_ERR_INVALID, "%s: connectivity %d is neither full (0) nor faces (1)", entry, connectivity);
    TRY(check_label_count(entry, K));
    if (!volume_fits_int32(Z, H, W)) return fail(TS2D_ERR_INVALID, "%s: %d x %d x %d is empty or more than 2^31 - 1 voxels", entry, Z, H, W);
    uint8_t table[256] = {};
    if (kind == kLcLabelMap) {
        TRY(check_label_values(entry, values, K));
        for (int k = 0; k < K; ++k) {
            if (table[values[k]]) return fail(TS2D_ERR_INVALID, "%s: values[%d] = %d repeats values[%d]", entry, k, values[k], table[values[k]] - 1);
            table[values[k]] = (uint8_t)(k + 1);
        }
    }
    std::vector<long long> minv((size_t)K, 0);
    for (int k = 0; min_voxels && k < K; ++k) {
        if (min_voxels[k] < 0) return fail(TS2D_ERR_INVALID, "%s: min_voxels[%d] = %lld is negative", entry, k, (long long)min_voxels[k]);
        minv[(size_t)k] = min_voxels[k];
    }
    if (capacity < 0) return fail(TS2D_ERR_INVALID, "%s: capacity %lld is negative", entry, (long long)capacity);
    if (capacity > 0 && !out_components) return fail(TS2D_ERR_INVALID, "%s: capacity %lld without a list to fill", entry, (long long)capacity);
    const size_t n = (size_t)Z * H * W;
    const int ww = (W + 63) >> 6;
    const long long words = (long long)Z * H * ww;
    // the state of one set: cls, the eq words, parent and count - 9 1/8 bytes per voxel.  A label map is one set whatever K is.
    const size_t per_set = n + (size_t)words * sizeof(cc_word) + 2 * n * sizeof(int);
    const size_t budget = max_scratch_bytes ? max_scratch_bytes : ((size_t)1 << 30);
    if (per_set > budget)
        return fail(TS2D_ERR_INVALID, "%s: the state of ONE label (%zu voxels) takes %zu bytes, above max_scratch_bytes = %zu", entry, n, per_set, budget);
    const int sets = kind == kLcLabelMap ? 1 : (int)(budget / per_set < (size_t)K ? budget / per_set : (size_t)K);
    const size_t n_sets = (size_t)(kind == kLcLabelMap ? 1 : K);
    const unsigned long long cap = (unsigned long long)capacity < (unsigned long long)n_sets * n ? (unsigned long long)capacity : (unsigned long long)n_sets * n;

    HIP_TRY(hipSetDevice(device));
    const size_t seg_bytes = n_sets * n;
    // [status, cursor, counters || table | thresholds | segmentation | state of a chunk | list]: the first part starts as zero
    const size_t ctr_ints = 4 + (size_t)K * kLcCounters;            // status at int 0, the 64-bit cursor at ints 2 and 3
    ArenaLayout lay;
    const size_t o_ctr = lay.add(ctr_ints * sizeof(int)), o_table = lay.add(256), o_min = lay.add((size_t)K * sizeof(long long)), o_seg = lay.add(seg_bytes);
    const size_t o_cls = lay.add((size_t)sets * n), o_eq = lay.add((size_t)sets * (size_t)words * sizeof(cc_word));
    const size_t o_parent = lay.add((size_t)sets * n * sizeof(int)), o_count = lay.add((size_t)sets * n * sizeof(int));
    const size_t o_list = lay.add((size_t)cap * 3 * sizeof(int));
    DevMem d;
    HIP_TRY(d.alloc(lay.total()));
    int* const d_status = d.as<int>(o_ctr);
    unsigned long long* const d_cursor = d.as<unsigned long long>(o_ctr + 2 * sizeof(int));
    int* const d_ctr = d_status + 4;
    uint8_t* const d_seg = d.as<uint8_t>(o_seg);
    HIP_TRY(hipMemset(d_status, 0, ctr_ints * sizeof(int)));
    HIP_TRY(hipMemcpy(d.as<char>(o_table), table, 256, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d.as<char>(o_min), minv.data(), (size_t)K * sizeof(long long), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_seg, seg, seg_bytes, hipMemcpyHostToDevice));
    LcState s = {d.as<uint8_t>(o_cls), d.as<cc_word>(o_eq), d.as<int>(o_parent), d.as<int>(o_count), (long long)n, words, W, kind, 0};
    const dim3 block(256);
    const FoldedGrid fg = fold_grid((words + 3) / 4, 256);
    for (int k0 = 0; k0 < (int)n_sets; k0 += sets) {               // each launch sees the one before it: the default stream orders them
        const unsigned now = (unsigned)((int)n_sets - k0 < sets ? (int)n_sets - k0 : sets);
        const dim3 grid(fg.x, now, fg.fold);
        s.k0 = k0;
        hipLaunchKernelGGL(lc_init, grid, block, 0, 0, d_seg, d.as<const uint8_t>(o_table), s, d_ctr);
        hipLaunchKernelGGL(lc_link, grid, block, 0, 0, s, H, connectivity, d_status);
        hipLaunchKernelGGL(lc_flatten, grid, block, 0, 0, s, d_ctr, d_status);
        hipLaunchKernelGGL(lc_count, grid, block, 0, 0, s);
        hipLaunchKernelGGL(lc_max, grid, block, 0, 0, s, d_ctr);
        hipLaunchKernelGGL(lc_apply, grid, block, 0, 0, d_seg, s, keep_largest ? 1 : 0, d.as<const long long>(o_min), d_ctr, d_status);
        if (cap > 0) hipLaunchKernelGGL(lc_list, grid, block, 0, 0, s, d.as<int>(o_list), cap, d_cursor, d_status);
        HIP_TRY(hipGetLastError());
    }
    std::vector<int> ctr(ctr_ints);
    HIP_TRY(hipMemcpy(ctr.data(), d_status, ctr_ints * sizeof(int), hipMemcpyDeviceToHost));      // (waits for the launches)
    if (ctr[0]) { *status = ctr[0]; return TS2D_OK; }              // a bounded loop reached its cap: every output stays as it is
    int64_t total = 0;
    for (int k = 0; k < K; ++k) total += ctr[4 + (size_t)k * kLcCounters + 1];
    const bool list_full = total > capacity;
    std::vector<int> list;
    if (!list_full && total > 0) {
        list.resize((size_t)total * 3);
        HIP_TRY(hipMemcpy(list.data(), d.as<char>(o_list), list.size() * sizeof(int), hipMemcpyDeviceToHost));
    }
    // the arrival order must not show: (label, size descending, first voxel).  The rows are dealt to their labels, whose places the counters give;
    // inside a label ONE 64-bit key orders them: (2^31 - 1 - size, first)
    std::vector<size_t> at((size_t)K + 1, 0);
    std::vector<unsigned long long> keys;
    if (!list_full && total > 0) {
        for (int k = 0; k < K; ++k) at[(size_t)k + 1] = at[(size_t)k] + (size_t)ctr[4 + (size_t)k * kLcCounters + 1];
        std::vector<size_t> fill(at.begin(), at.end() - 1);
        keys.resize((size_t)total);
        for (size_t r = 0; r < (size_t)total; ++r) {
            const int* const e = list.data() + 3 * r;
            if (e[0] < 0 || e[0] >= K || fill[(size_t)e[0]] >= at[(size_t)e[0] + 1])
                return fail(TS2D_ERR_STATE, "%s: the list and the counters disagree about label %d", entry, e[0]);
            keys[fill[(size_t)e[0]]++] = (unsigned long long)(0x7FFFFFFF - e[2]) << 32 | (unsigned)e[1];
        }
        for (int k = 0; k < K; ++k) std::sort(keys.begin() + (long long)at[(size_t)k], keys.begin() + (long long)at[(size_t)k + 1]);
    }
    if (out_seg) HIP_TRY(hipMemcpy(out_seg, d_seg, seg_bytes, hipMemcpyDeviceToHost));
    for (size_t k = 0; k < (size_t)K * kLcCounters; ++k) out_counters[k] = ctr[4 + k];
    *out_n_components = total;
    *status = list_full ? kLcStatusListFull : 0;
    for (int k = 0; k < K && !keys.empty(); ++k)
        for (size_t r = at[(size_t)k]; r < at[(size_t)k + 1]; ++r) {
            out_components[3 * r] = k;
            out_components[3 * r + 1] = (int64_t)(keys[r] & 0xFFFFFFFFull);
            out_components[3 * r + 2] = 0x7FFFFFFF - (int64_t)(keys[r] >> 32);
        }
    return TS2D_OK;
}
