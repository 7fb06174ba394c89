// ts2d_label_morphology: grow, shrink, open and close every label of a 2-D segmentation by a radius in the unit of the spacing, with an exact
// Euclidean disc (kernels_morph.h; the arithmetic: morph.h; the table and the chunks: morph_plan.cpp; the definition:
// totalsegmentator2d_amd/morphology.py).  Host pointers in and out, one upload, every step on the device, one download; every device buffer of the
// call is one DevMem laid out by an ArenaLayout, so HIP_TRY may return wherever it fails and the scratch is freed on every path.
#include "engine_internal.h"
#include "entry_util.h"
#include "kernels_morph.h"
#include "morph_plan.h"

#include <cmath>
#include <vector>

using namespace ts2d;

static_assert(kMoDilate == TS2D_MORPH_DILATE && kMoErode == TS2D_MORPH_ERODE && kMoOpen == TS2D_MORPH_OPEN && kMoClose == TS2D_MORPH_CLOSE,
              "the operations speak the C header's numbers");
static_assert(kMoCounters == TS2D_MORPH_COUNTERS && kMoMaxExtent == TS2D_EVAL_MAX_EXTENT, "the counters and the limit are the C header's");
static_assert(kStPlanes == TS2D_STATS_PLANES && kStLabelMap == TS2D_STATS_LABELMAP, "the kinds speak the C header's numbers");

int ts2d_label_morphology(int device, const uint8_t* seg, int kind, const uint8_t* values, int K, int H, int W, double sy, double sx, int op,
                          double radius, const uint8_t* select, uint64_t max_scratch_bytes, uint8_t* out_seg, int64_t* out_counters) {
    const char* const entry = "ts2d_label_morphology";
    if (!seg || !out_seg || !out_counters) return fail(TS2D_ERR_INVALID, "%s: null argument", entry);
    if (!label_kind(kind)) return fail(TS2D_ERR_INVALID, "%s: kind %d is neither planes (0) nor label map (1)", entry, kind);
    if (op < kMoDilate || op > kMoClose) return fail(TS2D_ERR_INVALID, "%s: op %d is none of dilate (0), erode (1), open (2), close (3)", entry, op);
    TRY(check_label_count(entry, K));
    if (H < 1 || W < 1 || H > kMoMaxExtent || W > kMoMaxExtent)
        return fail(TS2D_ERR_INVALID, "%s: extents %d x %d outside 1 ... %d", entry, H, W, kMoMaxExtent);
    if (!volume_fits_int32(1, H, W)) return fail(TS2D_ERR_INVALID, "%s: %d x %d is more than 2^31 - 1 pixels", entry, H, W);
    if (!(std::isfinite(radius) && radius >= 0.0)) return fail(TS2D_ERR_INVALID, "%s: radius %g must be finite and not negative", entry, radius);
    if (!(std::isfinite(sy) && std::isfinite(sx) && sy > 0.0 && sx > 0.0))
        return fail(TS2D_ERR_INVALID, "%s: spacing %g x %g must be finite and positive", entry, sy, sx);
    uint8_t table[256] = {};
    if (kind == kStLabelMap) {
        TRY(check_label_values(entry, values, K));
        for (int k = 0; k < K; ++k) {
            if (table[values[k]]) return fail(TS2D_ERR_INVALID, "%s: values[%d] = %d repeats values[%d]", entry, k, values[k], table[values[k]] - 1);
            table[values[k]] = (uint8_t)(k + 1);
        }
    }
    MoPlan plan;
    if (mo_plan(kind, op, H, W, sy, sx, radius, K, (size_t)max_scratch_bytes, &plan) != 0)
        return fail(TS2D_ERR_INVALID, "%s: the scratch of ONE label (%d x %d pixels) takes %zu bytes, above max_scratch_bytes = %zu", entry, H, W,
                    plan.per_label, plan.budget);
    std::vector<int> sel;
    for (int k = 0; k < K; ++k)
        if (!select || select[k]) sel.push_back(k);
    const size_t n = (size_t)H * W, n_planes = kind == kStLabelMap ? 1 : (size_t)K;
    const size_t seg_bytes = n_planes * n;
    const size_t L = plan.labels < sel.size() ? plan.labels : (sel.empty() ? 1 : sel.size());
    const int T = (int)plan.cover.size();
    const int steps = mo_steps(op);
    const bool map = kind == kStLabelMap;

    HIP_TRY(hipSetDevice(device));
    // [counters || table | values | selected labels | cover | segmentation | output | g | intermediate planes | result planes]: the first part starts as zero
    const size_t ctr_ints = (size_t)K * kMoCtr;
    ArenaLayout lay;
    const size_t o_ctr = lay.add(ctr_ints * sizeof(int)), o_table = lay.add(256), o_val = lay.add((size_t)K), o_sel = lay.add(sel.size() * sizeof(int));
    const size_t o_cover = lay.add((size_t)T * sizeof(uint16_t)), o_seg = lay.add(seg_bytes), o_out = lay.add(seg_bytes);
    const size_t o_g = lay.add(L * n * sizeof(uint16_t)), o_mid = lay.add(steps == 2 ? L * n : 0), o_res = lay.add(map ? L * n : 0);
    DevMem d;
    HIP_TRY(d.alloc(lay.total()));
    int* const d_ctr = d.as<int>(o_ctr);
    const uint8_t* const d_seg = d.as<const uint8_t>(o_seg);
    uint8_t* const d_out = d.as<uint8_t>(o_out);
    HIP_TRY(hipMemset(d_ctr, 0, ctr_ints * sizeof(int)));
    HIP_TRY(hipMemcpy(d.as<char>(o_table), table, 256, hipMemcpyHostToDevice));
    if (map) HIP_TRY(hipMemcpy(d.as<char>(o_val), values, (size_t)K, hipMemcpyHostToDevice));
    if (!sel.empty()) HIP_TRY(hipMemcpy(d.as<char>(o_sel), sel.data(), sel.size() * sizeof(int), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d.as<char>(o_cover), plan.cover.data(), (size_t)T * sizeof(uint16_t), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d.as<char>(o_seg), seg, seg_bytes, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_out, d_seg, seg_bytes, hipMemcpyDeviceToDevice));      // unselected planes, and the label map that mo_compose changes
    // Grids: n <= 2^31 - 1 pixels in blocks of 256 are at most 2^23 blocks along x; rows and columns at most 32767; labels at most 255 along y.
    const unsigned pixel_blocks = (unsigned)((n + 255) / 256);
    hipLaunchKernelGGL(mo_before, dim3(pixel_blocks, (unsigned)n_planes), dim3(256), 0, 0, d_seg, kind, d.as<const uint8_t>(o_table), (long long)n, d_ctr);
    const uint16_t* const d_cover = d.as<const uint16_t>(o_cover);
    uint16_t* const d_g = d.as<uint16_t>(o_g);
    uint8_t* const d_mid = d.as<uint8_t>(o_mid);
    uint8_t* const d_res = d.as<uint8_t>(o_res);
    for (size_t c0 = 0; c0 < sel.size(); c0 += L) {                // each launch sees the one before it: the default stream orders them
        const unsigned now = (unsigned)(sel.size() - c0 < L ? sel.size() - c0 : L);
        const MoChunk ch = {d.as<const int>(o_sel) + c0, d.as<const uint8_t>(o_val), (int)now, (long long)n, H, W};
        const dim3 col_grid((unsigned)((W + 63) / 64), now), row_grid((unsigned)((H + 3) / 4), now);
        for (int s = 0; s < steps; ++s) {
            const int erodes = mo_step_erodes(op, s) ? 1 : 0;
            const bool last = s + 1 == steps;
            const uint8_t* const src = s == 0 ? d_seg : d_mid;
            const int src_mode = s == 0 ? (map ? kMoSrcLabelMap : kMoSrcPlanes) : kMoSrcSlots;
            hipLaunchKernelGGL(mo_columns, col_grid, dim3(64), 0, 0, ch, src, src_mode, erodes, T, d_g);
            if (last && !map)
                hipLaunchKernelGGL(mo_rows<true>, row_grid, dim3(256), 0, 0, ch, d_g, d_cover, T, erodes, d_out, 1, d_seg, d_ctr);
            else
                hipLaunchKernelGGL(mo_rows<false>, row_grid, dim3(256), 0, 0, ch, d_g, d_cover, T, erodes, last ? d_res : d_mid, 0, d_seg, d_ctr);
        }
        if (map) hipLaunchKernelGGL(mo_compose, dim3(pixel_blocks), dim3(256), 0, 0, ch, d_seg, d_res, mo_grows(op) ? 1 : 0, d_out, d_ctr);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipGetLastError());
    std::vector<int> ctr(ctr_ints);
    HIP_TRY(hipMemcpy(ctr.data(), d_ctr, ctr_ints * sizeof(int), hipMemcpyDeviceToHost));      // (waits for the launches)
    HIP_TRY(hipMemcpy(out_seg, d_out, seg_bytes, hipMemcpyDeviceToHost));
    for (int k = 0; k < K; ++k) {
        const int64_t before = ctr[(size_t)k * kMoCtr], added = ctr[(size_t)k * kMoCtr + 1], removed = ctr[(size_t)k * kMoCtr + 2];
        int64_t* const o = out_counters + (size_t)k * kMoCounters;
        o[0] = before; o[1] = before + added - removed; o[2] = added; o[3] = removed;
    }
    return TS2D_OK;
}
