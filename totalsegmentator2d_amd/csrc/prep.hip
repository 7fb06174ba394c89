// The input side of libts2d_engine.so, none of which needs an engine: coronal projection + z-score of a volume, its synthetic radiograph and the
// label projection along the radiograph's rays, the order-3 resample to the
// plan spacing, and the ts2d_planes handle (crop box, every normalisation scheme of nnU-Net and resample of native 2-D inputs, and of the slice stacks
// of a volume under a 2-D plan, where they lie on the device).
// The host arithmetic behind them is prep_plan.cpp; every device buffer of a call is a DevMem, so HIP_TRY may return wherever it fails.
#include "engine_internal.h"
#include "entry_util.h"
#include "kernels_project.h"
#include "kernels_project_modes.h"
#include "kernels_project_xr.h"
#include "kernels_resample_in.h"
#include "kernels_prep.h"
#include "kernels_prep_schemes.h"
#include "kernels_prep_stack.h"
#include "kernels_prep_fill.h"

#include <algorithm>
#include <cmath>
#include <type_traits>
#include <vector>

using namespace ts2d;

#pragma GCC visibility push(hidden)
// Planes that stay on the device between the steps of nnU-Net's preprocessing of a native 2-D input (kernels_prep.h): uploaded once,
// cropped, z-scored and resampled where they lie, downloaded once.
struct ts2d_planes {
    int device = 0;
    int n = 0, h = 0, w = 0;
    int z = 1;                  // slices per channel: 1, or those of a stack (ts2d_planes_create_stack), whose n = channels * z planes are its slices
    DevMem d;                   // float [n][h][w]
    DevMem d_lh;                // float [n][2]: float32 minimum and maximum of each plane, valid while has_bounds
    bool has_bounds = false;
};

namespace {

constexpr int kPrepMaxPlanes = 65535;           // (a grid dimension)
constexpr long long kPrepMaxSamples = 1ll << 28;
static_assert(kPrepZScore == TS2D_NORM_ZSCORE && kPrepCT == TS2D_NORM_CT && kPrepRescale01 == TS2D_NORM_RESCALE01 && kPrepRGB01 == TS2D_NORM_RGB01 &&
              kPrepNone == TS2D_NORM_NONE && kPrepStatusRgbRange == TS2D_PLANES_RGB_RANGE && kPrepStatusFillRounds == TS2D_PLANES_FILL_ROUNDS,
              "the scheme table speaks the C header's numbers");

int project_coronal_impl(int device, const void* volume, size_t n_elems, int dtype, int nz, int ny, int nx, long long sz,
                         long long sy, long long sx, long long base, float* out_max, float* out_mean, float* out_norm, double* out_stats, int* out_box) {
    if (!volume || !out_max || !out_mean) return fail(TS2D_ERR_INVALID, "ts2d_project_coronal: null argument");
    if (dtype < 0 || dtype > 4 || nz < 1 || ny < 1 || nx < 1) return fail(TS2D_ERR_INVALID, "ts2d_project_coronal: bad dtype / extents");
    if ((long long)nz * nx > 0x7FFFFFFFll)          // one lane per output pixel: a launch past 2^32 lanes is cut short, not refused, by the runtime
        return fail(TS2D_ERR_INVALID, "ts2d_project_coronal: planes of nz %d x nx %d are more than 2^31 - 1 pixels", nz, nx);
    TRY(check_strided_view("ts2d_project_coronal", n_elems, base, {nz, ny, nx}, {sz, sy, sx}, false));
    HIP_TRY(hipSetDevice(device));
    const size_t vbytes = n_elems * sample_size(dtype), obytes = (size_t)nz * nx * sizeof(float);
    ArenaLayout lay;
    const size_t o_vol = lay.add(vbytes), o_proj = lay.add(2 * obytes);      // max | mean, contiguous: the two channels of the z-score
    const size_t o_norm = lay.add(2 * obytes), o_part = lay.add(2 * kZBlocks * sizeof(double)), o_stats = lay.add(4 * sizeof(double));
    const size_t o_box = lay.add(4 * sizeof(int));
    DevMem d;
    HIP_TRY(d.alloc(lay.total()));
    float* d_max = d.as<float>(o_proj);
    float* d_mean = d_max + (size_t)nz * nx;
    HIP_TRY(hipMemcpy(d.as<char>(o_vol), volume, vbytes, hipMemcpyHostToDevice));
    const unsigned grid = (unsigned)(((long long)nz * nx + 255) / 256);
    by_sample_type(dtype, [&](auto t) {
        using S = typename decltype(t)::type;
        hipLaunchKernelGGL(project_coronal<S>, dim3(grid), dim3(256), 0, 0, d.as<const S>(o_vol), nz, ny, nx, sz, sy, sx, base, d_max, d_mean);
    });
    HIP_TRY(hipGetLastError());
    if (out_norm) {          // per-channel z-score of (max, mean): float64 two-pass statistics, deterministic
        const long long n = (long long)nz * nx;
        float* d_norm = d.as<float>(o_norm);
        double* d_part = d.as<double>(o_part); double* d_stats = d.as<double>(o_stats);
        int* d_box = d.as<int>(o_box);
        const int box0[4] = {nz, -1, nx, -1};
        HIP_TRY(hipMemcpy(d_box, box0, sizeof(box0), hipMemcpyHostToDevice));
        hipLaunchKernelGGL(zs_partial<0>, dim3(kZBlocks, 2), dim3(256), 0, 0, d_max, n, d_stats, d_part);
        hipLaunchKernelGGL(zs_combine<0>, dim3(1), dim3(2), 0, 0, d_part, n, d_stats);
        hipLaunchKernelGGL(zs_partial<1>, dim3(kZBlocks, 2), dim3(256), 0, 0, d_max, n, d_stats, d_part);
        hipLaunchKernelGGL(zs_combine<1>, dim3(1), dim3(2), 0, 0, d_part, n, d_stats);
        hipLaunchKernelGGL(zs_apply, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, d_max, n, nx, 2, d_stats, d_norm, d_box);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpy(out_norm, d_norm, 2 * obytes, hipMemcpyDeviceToHost));
        if (out_stats) HIP_TRY(hipMemcpy(out_stats, d_stats, 4 * sizeof(double), hipMemcpyDeviceToHost));
        if (out_box) HIP_TRY(hipMemcpy(out_box, d_box, 4 * sizeof(int), hipMemcpyDeviceToHost));
    }
    HIP_TRY(hipMemcpy(out_max, d_max, obytes, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(out_mean, d_mean, obytes, hipMemcpyDeviceToHost));
    return TS2D_OK;
}

static_assert(kPmMax == TS2D_PROJECT_MAX && kPmMin == TS2D_PROJECT_MIN && kPmMean == TS2D_PROJECT_MEAN && kPmMedian == TS2D_PROJECT_MEDIAN &&
              kPmStd == TS2D_PROJECT_STD && kPmFirst == TS2D_PROJECT_FIRST && kPmSlice == TS2D_PROJECT_SLICE && kPmMaxModes == TS2D_PROJECT_MAX_MODES &&
              kPmStatusNonFinite == TS2D_PROJECT_NONFINITE && kPmStatusRayTooLong == TS2D_PROJECT_RAY_TOO_LONG && kPmRayCap == TS2D_PROJECT_RAY_CAP,
              "the projection modes speak the C header's numbers");

// The launches of ts2d_project_coronal_modes for one sample type.  d_first[kind]: the first plane asked for of that kind (null: none).
template <typename T>
int project_modes_launch(const T* d_vol, int nz, int ny, int nx, long long sz, long long sy, long long sx, long long base, bool stream,
                         const PmStreamArgs& sa, float* d_median, int* d_status) {
    const long long n = (long long)nz * nx;
    const unsigned grid = (unsigned)((n + 255) / 256);
    if (stream) hipLaunchKernelGGL(project_modes_stream<T>, dim3(grid), dim3(256), 0, 0, d_vol, nz, ny, nx, sz, sy, sx, base, sa, d_status);
    if (d_median) {
        const int tile_x = pm_tile_x(ny, (int)sizeof(T));
        if (tile_x) {
            int lg = 4;
            while ((1 << lg) < tile_x) ++lg;
            const int tiles_x = (nx + tile_x - 1) / tile_x, n_full = ny * tile_x / kPmThreads;
            const size_t smem = kPmLdsCountBytes + align_up((size_t)ny * tile_x * sizeof(T), 16);
            HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(project_median_lds<T>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
            hipLaunchKernelGGL(project_median_lds<T>, dim3((unsigned)((long long)tiles_x * nz)), dim3(kPmThreads), smem, 0, d_vol, nz, ny, nx, sz, sy, sx,
                               base, lg, tiles_x, n_full, d_median);
        } else {
            hipLaunchKernelGGL(project_median_global<T>, dim3(grid), dim3(256), 0, 0, d_vol, nz, ny, nx, sz, sy, sx, base, d_median);
        }
    }
    HIP_TRY(hipGetLastError());
    return TS2D_OK;
}

int project_coronal_modes_impl(int device, const void* volume, size_t n_elems, int dtype, int nz, int ny, int nx, long long sz, long long sy,
                               long long sx, long long base, const int* modes, const int* slice_index, int n_modes, float* out_planes,
                               float* out_norm, double* out_stats, int* out_box, int* status) {
    const char* const E = "ts2d_project_coronal_modes";
    if (!volume) return fail(TS2D_ERR_INVALID, "%s: volume is null", E);
    if (!modes) return fail(TS2D_ERR_INVALID, "%s: modes is null", E);
    if (!slice_index) return fail(TS2D_ERR_INVALID, "%s: slice_index is null", E);
    if (!out_planes) return fail(TS2D_ERR_INVALID, "%s: out_planes is null", E);
    if (!status) return fail(TS2D_ERR_INVALID, "%s: status is null", E);
    if (!out_norm && (out_stats || out_box)) return fail(TS2D_ERR_INVALID, "%s: out_stats / out_box without out_norm", E);
    if (dtype < 0 || dtype > 4) return fail(TS2D_ERR_INVALID, "%s: dtype %d unknown", E, dtype);
    if (n_modes < 1 || n_modes > kPmMaxModes) return fail(TS2D_ERR_INVALID, "%s: n_modes %d outside 1 ... %d", E, n_modes, kPmMaxModes);
    if (nz < 1 || ny < 1 || nx < 1) return fail(TS2D_ERR_INVALID, "%s: extents nz %d, ny %d, nx %d below 1", E, nz, ny, nx);
    if ((long long)nz * nx * n_modes > kPrepMaxSamples)
        return fail(TS2D_ERR_INVALID, "%s: n_modes %d planes of nz %d x nx %d are more than one call takes (2^28 samples)", E, n_modes, nz, nx);
    bool want[kPmKinds] = {};
    for (int m = 0; m < n_modes; ++m) {
        if (modes[m] < 0 || modes[m] >= kPmKinds) return fail(TS2D_ERR_INVALID, "%s: modes[%d] = %d is an unknown mode", E, m, modes[m]);
        if (modes[m] == kPmSlice && (slice_index[m] < 0 || slice_index[m] >= ny))
            return fail(TS2D_ERR_INVALID, "%s: slice_index[%d] = %d outside [0, ny = %d)", E, m, slice_index[m], ny);
        want[modes[m]] = true;
    }
    if (want[kPmStd] && ny < 2) return fail(TS2D_ERR_INVALID, "%s: the std mode needs ny >= 2, found ny %d", E, ny);
    TRY(check_strided_view(E, n_elems, base, {nz, ny, nx}, {sz, sy, sx}));
    *status = 0;
    if (ny > kPmRayCap) { *status = kPmStatusRayTooLong; return TS2D_OK; }     // nothing is launched, nothing is written
    HIP_TRY(hipSetDevice(device));
    const long long n = (long long)nz * nx;
    const size_t vbytes = n_elems * sample_size(dtype), obytes = (size_t)n * sizeof(float);
    ArenaLayout lay;
    const size_t o_vol = lay.add(vbytes), o_proj = lay.add(n_modes * obytes), o_norm = lay.add(n_modes * obytes);
    const size_t o_part = lay.add((size_t)n_modes * kZBlocks * sizeof(double)), o_stats = lay.add((size_t)n_modes * 2 * sizeof(double));
    const size_t o_box = lay.add((size_t)n_modes * 4 * sizeof(int)), o_status = lay.add(sizeof(int));
    DevMem d;
    HIP_TRY(d.alloc(lay.total()));
    float* d_planes = d.as<float>(o_proj);
    int* d_status = d.as<int>(o_status);
    HIP_TRY(hipMemcpy(d.as<char>(o_vol), volume, vbytes, hipMemcpyHostToDevice));
    HIP_TRY(hipMemset(d_status, 0, sizeof(int)));
    // a kind asked for twice is computed once, into its first plane, and copied to the others
    PmStreamArgs sa = {};
    float* d_first[kPmKinds] = {};
    for (int m = 0; m < n_modes; ++m) {
        float* plane = d_planes + (size_t)m * n;
        if (modes[m] == kPmSlice) { sa.slice_y[sa.n_slices] = slice_index[m]; sa.slice_out[sa.n_slices++] = plane; }
        else if (!d_first[modes[m]]) d_first[modes[m]] = plane;
    }
    for (int k = 0; k < kPmKinds; ++k) sa.out[k] = (k == kPmMedian || k == kPmSlice) ? nullptr : d_first[k];
    // a float volume is always streamed: that pass is what finds a non-finite sample
    const bool stream = dtype == 2 || sa.n_slices > 0 || want[kPmMax] || want[kPmMin] || want[kPmMean] || want[kPmStd] || want[kPmFirst];
    TRY(by_sample_type(dtype, [&](auto t) {
        return project_modes_launch(d.as<const typename decltype(t)::type>(o_vol), nz, ny, nx, sz, sy, sx, base, stream, sa, d_first[kPmMedian], d_status);
    }));
    for (int m = 0; m < n_modes; ++m) {
        float* plane = d_planes + (size_t)m * n;
        if (modes[m] != kPmSlice && d_first[modes[m]] != plane) HIP_TRY(hipMemcpy(plane, d_first[modes[m]], obytes, hipMemcpyDeviceToDevice));
    }
    HIP_TRY(hipMemcpy(status, d_status, sizeof(int), hipMemcpyDeviceToHost));
    if (*status) return TS2D_OK;                                   // a non-finite sample: the planes are no result, the caller takes the host route
    if (out_norm) {          // per-plane z-score as behind ts2d_project_coronal_zscore, the non-zero box per plane
        float* d_norm = d.as<float>(o_norm);
        double* d_part = d.as<double>(o_part); double* d_stats = d.as<double>(o_stats);
        int* d_box = d.as<int>(o_box);
        int box0[4 * kPmMaxModes];
        for (int m = 0; m < n_modes; ++m) { box0[4 * m] = nz; box0[4 * m + 1] = -1; box0[4 * m + 2] = nx; box0[4 * m + 3] = -1; }
        HIP_TRY(hipMemcpy(d_box, box0, (size_t)n_modes * 4 * sizeof(int), hipMemcpyHostToDevice));
        hipLaunchKernelGGL(zs_partial<0>, dim3(kZBlocks, n_modes), dim3(256), 0, 0, d_planes, n, d_stats, d_part);
        hipLaunchKernelGGL(zs_combine<0>, dim3(1), dim3(n_modes), 0, 0, d_part, n, d_stats);
        hipLaunchKernelGGL(zs_partial<1>, dim3(kZBlocks, n_modes), dim3(256), 0, 0, d_planes, n, d_stats, d_part);
        hipLaunchKernelGGL(zs_combine<1>, dim3(1), dim3(n_modes), 0, 0, d_part, n, d_stats);
        hipLaunchKernelGGL(zs_apply_planes, dim3((unsigned)((n + 255) / 256), n_modes), dim3(256), 0, 0, d_planes, n, nx, d_stats, d_norm, d_box);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpy(out_norm, d_norm, n_modes * obytes, hipMemcpyDeviceToHost));
        if (out_stats) HIP_TRY(hipMemcpy(out_stats, d_stats, (size_t)n_modes * 2 * sizeof(double), hipMemcpyDeviceToHost));
        if (out_box) HIP_TRY(hipMemcpy(out_box, d_box, (size_t)n_modes * 4 * sizeof(int), hipMemcpyDeviceToHost));
    }
    HIP_TRY(hipMemcpy(out_planes, d_planes, n_modes * obytes, hipMemcpyDeviceToHost));
    return TS2D_OK;
}

// what ts2d_resample_cubic and ts2d_planes_resample_cubic refuse alike: extents outside 2 ... kRsInMaxExtent, more samples than one call takes
int rsin_check(const char* entry, int n_planes, int in_h, int in_w, int out_h, int out_w) {
    if (in_h < 2 || in_w < 2 || out_h < 2 || out_w < 2 || in_h > kRsInMaxExtent || in_w > kRsInMaxExtent || out_h > kRsInMaxExtent || out_w > kRsInMaxExtent)
        return fail(TS2D_ERR_INVALID, "%s: extents %d x %d -> %d x %d outside 2 ... %d", entry, in_h, in_w, out_h, out_w, kRsInMaxExtent);
    if ((long long)n_planes * (in_h + 2 * kRsInPad) * (in_w + 2 * kRsInPad) > (1ll << 28) || (long long)n_planes * out_h * out_w > (1ll << 28))
        return fail(TS2D_ERR_INVALID, "%s: %d planes of %d x %d -> %d x %d are more than one call takes (2^28 samples)", entry, n_planes, in_h, in_w, out_h, out_w);
    return TS2D_OK;
}

// The device part of the order-3 resample, shared by ts2d_resample_cubic (host planes in and out) and ts2d_planes_resample_cubic (planes
// that live on the device): the tables of the plan go to the scratch, then the three rsin_* launches over device pointers.
// d_scratch: pl.bytes; d_src [n_planes][in_h][in_w], d_lh [n_planes][2], d_dst [n_planes][out_h][out_w], all on the device
int rsin_run(const RsInPlan& pl, char* d_scratch, const float* d_src, const float* d_lh, float* d_dst, int n_planes, int in_h, int in_w,
             int out_h, int out_w) {
    double* d_coef = reinterpret_cast<double*>(d_scratch);
    const double* d_pow = reinterpret_cast<const double*>(d_scratch + pl.o_pow);
    const RsInTap* d_taps = reinterpret_cast<const RsInTap*>(d_scratch + pl.o_taps);
    HIP_TRY(hipMemcpy(d_scratch + pl.o_pow, pl.zpow.data(), pl.zpow.size() * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_scratch + pl.o_taps, pl.taps.data(), pl.taps.size() * sizeof(RsInTap), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(rsin_prefilter_cols, dim3((unsigned)(((long long)n_planes * pl.Wp + 63) / 64)), dim3(64), 0, 0,
                       d_src, n_planes, in_h, in_w, pl.ax_h, d_pow, d_coef);
    hipLaunchKernelGGL(rsin_prefilter_rows, dim3((unsigned)(((long long)n_planes * pl.Hp + 63) / 64)), dim3(64), 0, 0,
                       d_coef, n_planes, pl.Hp, pl.Wp, pl.ax_w, d_pow);
    const long long quads = (long long)n_planes * out_h * ((out_w + 3) / 4);
    hipLaunchKernelGGL(rsin_interp_clip, dim3((unsigned)((quads + 255) / 256)), dim3(256), 0, 0,
                       d_coef, n_planes, pl.Hp, pl.Wp, out_h, out_w, d_taps, d_lh, d_dst);
    HIP_TRY(hipGetLastError());
    return TS2D_OK;
}

// Both create entries: n_planes planes of h x w, `slices` of them per channel, uploaded to a new handle.
int planes_create(const char* entry, int device, const float* src, int n_planes, int slices, int h, int w, ts2d_planes** out) {
    if (!src || !out) return fail(TS2D_ERR_INVALID, "%s: null argument", entry);
    *out = nullptr;
    if (n_planes < 1 || n_planes > kPrepMaxPlanes) return fail(TS2D_ERR_INVALID, "%s: %d planes outside 1 ... %d", entry, n_planes, kPrepMaxPlanes);
    if (h < 1 || w < 1 || h > kRsInMaxExtent || w > kRsInMaxExtent)
        return fail(TS2D_ERR_INVALID, "%s: extents %d x %d outside 1 ... %d", entry, h, w, kRsInMaxExtent);
    if ((long long)n_planes * h * w > kPrepMaxSamples)
        return fail(TS2D_ERR_INVALID, "%s: %d planes of %d x %d are more than one handle takes (2^28 samples)", entry, n_planes, h, w);
    HIP_TRY(hipSetDevice(device));
    const size_t bytes = (size_t)n_planes * h * w * sizeof(float);
    DevMem d, d_lh;
    HIP_TRY(d.alloc(bytes));
    HIP_TRY(d_lh.alloc((size_t)n_planes * 2 * sizeof(float)));
    HIP_TRY(hipMemcpy(d.as<float>(), src, bytes, hipMemcpyHostToDevice));
    ts2d_planes* p = new ts2d_planes();
    p->device = device; p->n = n_planes; p->z = slices; p->h = h; p->w = w; p->d = std::move(d); p->d_lh = std::move(d_lh);
    *out = p;
    return TS2D_OK;
}

// crop_to_nonzero of both crop entries: the box of the pixels that are non-zero in any plane, and the planes compacted to it.  d_box: four
// integers of device scratch.  box = {first row, one past the last row, first column, one past the last column}; the handle's clip bounds are dropped.
int planes_crop(const char* entry, ts2d_planes* p, int* d_box, int32_t box[4]) {
    const int n = p->n;
    int hb[4] = {p->h, -1, p->w, -1};
    HIP_TRY(hipMemcpy(d_box, hb, sizeof(hb), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(prep_nonzero_box, dim3((unsigned)(((long long)p->h * p->w + 255) / 256)), dim3(256), 0, 0, p->d.as<float>(), n, p->h, p->w, d_box);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(hb, d_box, sizeof(hb), hipMemcpyDeviceToHost));
    if (hb[1] < 0) { hb[0] = 0; hb[1] = p->h - 1; hb[2] = 0; hb[3] = p->w - 1; }            // nothing but zeros: the whole extent stays
    if (hb[0] < 0 || hb[1] >= p->h || hb[0] > hb[1] || hb[2] < 0 || hb[3] >= p->w || hb[2] > hb[3])
        return fail(TS2D_ERR_HIP, "%s: the device returned the box rows %d ... %d, columns %d ... %d of %d x %d", entry, hb[0], hb[1], hb[2], hb[3], p->h, p->w);
    const int bh = hb[1] - hb[0] + 1, bw = hb[3] - hb[2] + 1;
    // compaction: the flattened index of the dense [n][bh][bw] buffer is numpy's
    if (bh != p->h || bw != p->w) {
        DevMem d_new;
        HIP_TRY(d_new.alloc((size_t)n * bh * bw * sizeof(float)));
        for (int c = 0; c < n; ++c)
            HIP_TRY(hipMemcpy2D(d_new.as<float>() + (size_t)c * bh * bw, (size_t)bw * sizeof(float), p->d.as<float>() + ((size_t)c * p->h + hb[0]) * p->w + hb[2],
                                (size_t)p->w * sizeof(float), (size_t)bw * sizeof(float), (size_t)bh, hipMemcpyDeviceToDevice));
        p->d = std::move(d_new); p->h = bh; p->w = bw;
    }
    p->has_bounds = false;
    box[0] = hb[0]; box[1] = hb[1] + 1; box[2] = hb[2]; box[3] = hb[3] + 1;
    return TS2D_OK;
}

// The z-score statistics of the planes x [n][N] on the device that `want` selects (null: all): the two sums chunk by chunk on the device, their
// fold and the float32 mean, variance, square root and divisor here.  norm [n] (also left at d_norm) and stats [n][2] = (mean, std) are
// written for the selected planes only; *bad is set, and nothing more computed, when a mean or a variance of theirs is not finite.
// d_leaves: kPrepMaxTailLeaves leaves, d_sums: n * (N / kPrepChunk + kPrepMaxTailLeaves) floats of device scratch.
int planes_stats(const char* entry, const float* x, long long N, int n, const uint8_t* want, PrepNorm* d_norm, PrepLeaf* d_leaves, float* d_sums,
                 PrepNorm* norm, float* stats, bool* bad) {
    const long long n_full = N / kPrepChunk;
    std::vector<PrepLeaf> leaves;
    if (N % kPrepChunk) prep_leaves(0, (int)(N % kPrepChunk), &leaves);
    if ((int)leaves.size() > kPrepMaxTailLeaves) return fail(TS2D_ERR_INVALID, "%s: %zu leaves in a partial chunk", entry, leaves.size());
    const size_t n_out = (size_t)n_full + leaves.size();
    const dim3 grid_sums((unsigned)(n_full + (leaves.empty() ? 0 : 1)), (unsigned)n);
    std::vector<float> sums((size_t)n * n_out);
    if (!leaves.empty()) HIP_TRY(hipMemcpy(d_leaves, leaves.data(), leaves.size() * sizeof(PrepLeaf), hipMemcpyHostToDevice));
    for (int pass = 0; pass < 2; ++pass) {
        if (pass == 0) hipLaunchKernelGGL(prep_chunk_sums<0>, grid_sums, dim3(512), 0, 0, x, N, d_norm, d_leaves, (int)leaves.size(), d_sums);
        else hipLaunchKernelGGL(prep_chunk_sums<1>, grid_sums, dim3(512), 0, 0, x, N, d_norm, d_leaves, (int)leaves.size(), d_sums);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpy(sums.data(), d_sums, sums.size() * sizeof(float), hipMemcpyDeviceToHost));
        for (int c = 0; c < n; ++c) {
            if (want && !want[c]) continue;
            // numpy divides the float32 sum by the count in float64 and rounds once to float32 (`ret / rcount` with an intp count)
            const float q = (float)((double)prep_plane_sum(sums.data() + (size_t)c * n_out, N) / (double)N);
            if (!std::isfinite(q)) *bad = true;
            if (pass == 0) { norm[c].mean = q; stats[2 * c] = q; }
            else { const float sd = std::sqrt(q); stats[2 * c + 1] = sd; norm[c].div = 1e-8 > (double)sd ? (float)1e-8 : sd; }   // max(std, 1e-8)
        }
        if (*bad) return TS2D_OK;
        HIP_TRY(hipMemcpy(d_norm, norm, (size_t)n * sizeof(PrepNorm), hipMemcpyHostToDevice));
    }
    return TS2D_OK;
}

// The keys a normalise kernel left at d_keys [n][2] become the handle's clip bounds; *bad is set instead when one of them is not finite.
int planes_keep_bounds(ts2d_planes* p, const int* d_keys, std::vector<int>* keys, bool* bad) {
    const size_t m = (size_t)p->n * 2;
    HIP_TRY(hipMemcpy(keys->data(), d_keys, m * sizeof(int), hipMemcpyDeviceToHost));
    std::vector<float> lh(m);
    for (size_t i = 0; i < m; ++i) { lh[i] = prep_unkey((*keys)[i]); if (!std::isfinite(lh[i])) *bad = true; }
    if (*bad) return TS2D_OK;
    HIP_TRY(hipMemcpy(p->d_lh.as<float>(), lh.data(), m * sizeof(float), hipMemcpyHostToDevice));
    p->has_bounds = true;
    return TS2D_OK;
}

// Both crop entries of a stack.  take_masked: a z-score channel with use_mask is normalised inside the hole-filled mask of the volume
// (kernels_prep_fill.h); without it such a channel is refused by name.
int planes_crop_normalize_stack(const char* entry, bool take_masked, ts2d_planes* p, const int32_t* schemes, const float* params, const uint8_t* use_mask,
                                int32_t box[6], float* stats, int* status) {
    if (!p || !schemes || !params || !use_mask || !box || !stats || !status) return fail(TS2D_ERR_INVALID, "%s: null argument", entry);
    *status = 0;
    const int C = p->n / p->z;
    bool any_plain = false, any_masked = false, any_rescale = false;
    for (int c = 0; c < C; ++c) {
        if (schemes[c] < TS2D_NORM_ZSCORE || schemes[c] > TS2D_NORM_NONE) return fail(TS2D_ERR_INVALID, "%s: channel %d has the unknown scheme %d", entry, c, (int)schemes[c]);
        const bool masked = schemes[c] == TS2D_NORM_ZSCORE && use_mask[c];
        if (masked && !take_masked)
            return fail(TS2D_ERR_INVALID, "%s: channel %d is normalised inside the non-zero mask, which nnU-Net fills in 3-D for a volume: that stays on the host", entry, c);
        if (schemes[c] == TS2D_NORM_CT)
            for (int k = 0; k < 4; ++k)
                if (!std::isfinite(params[4 * c + k]))
                    return fail(TS2D_ERR_INVALID, "%s: channel %d has the non-finite CT parameter %g at [%d] (mean, divisor, lower bound, upper bound)", entry, c, (double)params[4 * c + k], k);
        any_masked |= masked; any_plain |= schemes[c] == TS2D_NORM_ZSCORE && !masked; any_rescale |= schemes[c] == TS2D_NORM_RESCALE01;
    }
    HIP_TRY(hipSetDevice(p->device));
    // scratch, sized for the uncropped extent: [box, -, status, n_m, "a sweep added a bit" | min / max keys of every slice, of the result and of the input | mean, divisor |
    //                                           scheme table | leaves of the partial chunk | chunk and leaf sums of every channel]
    const int n0 = p->n;
    const size_t per_channel = (size_t)((long long)p->z * p->h * p->w / kPrepChunk) + kPrepMaxTailLeaves;
    const size_t o_keys = 256, o_norm = align_up(o_keys + (size_t)n0 * 4 * sizeof(int), 256), o_table = align_up(o_norm + (size_t)C * sizeof(PrepNorm), 256);
    const size_t o_leaves = align_up(o_table + (size_t)C * sizeof(PrepScheme), 256), o_sums = align_up(o_leaves + kPrepMaxTailLeaves * sizeof(PrepLeaf), 256);
    DevMem d;
    HIP_TRY(d.alloc(o_sums + (size_t)C * per_channel * sizeof(float)));
    int* d_box = d.as<int>(); int* d_status = d.as<int>(7 * sizeof(int)); int* d_total = d_status + 1; int* d_added = d_status + 2;
    int* d_keys = d.as<int>(o_keys);
    PrepNorm* d_norm = d.as<PrepNorm>(o_norm); PrepScheme* d_table = d.as<PrepScheme>(o_table);
    // 1. crop_to_nonzero's box over all channels and all three axes (the holes nnU-Net fills in the mask lie inside it: the box is that of the raw mask)
    int hb[6] = {p->z, -1, p->h, -1, p->w, -1};
    const int zero = 0;
    HIP_TRY(hipMemcpy(d_box, hb, sizeof(hb), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_status, &zero, sizeof(int), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(prep_nonzero_box3, dim3((unsigned)(((long long)p->z * p->h * p->w + 255) / 256)), dim3(256), 0, 0, p->d.as<float>(), C, p->z, p->h, p->w, d_box);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(hb, d_box, sizeof(hb), hipMemcpyDeviceToHost));
    if (hb[1] < 0) { hb[0] = 0; hb[1] = p->z - 1; hb[2] = 0; hb[3] = p->h - 1; hb[4] = 0; hb[5] = p->w - 1; }      // nothing but zeros: the whole extent stays
    const int ext[3] = {p->z, p->h, p->w};
    for (int a = 0; a < 3; ++a)
        if (hb[2 * a] < 0 || hb[2 * a + 1] >= ext[a] || hb[2 * a] > hb[2 * a + 1])
            return fail(TS2D_ERR_HIP, "%s: the device returned the box %d ... %d on axis %d of extent %d", entry, hb[2 * a], hb[2 * a + 1], a, ext[a]);
    const int bz = hb[1] - hb[0] + 1, bh = hb[3] - hb[2] + 1, bw = hb[5] - hb[4] + 1;
    // 2. compaction: the flattened index of the dense [C][bz][bh][bw] buffer is numpy's
    if (bz != p->z || bh != p->h || bw != p->w) {
        DevMem d_new;
        HIP_TRY(d_new.alloc((size_t)C * bz * bh * bw * sizeof(float)));
        hipLaunchKernelGGL(prep_compact_box3, dim3((unsigned)((bh * bw + 255) / 256), (unsigned)bz, (unsigned)C), dim3(256), 0, 0,
                           p->d.as<const float>(), p->z, p->h, p->w, hb[0], hb[2], hb[4], bh, bw, d_new.as<float>());
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipDeviceSynchronize());
        p->d = std::move(d_new); p->z = bz; p->h = bh; p->w = bw; p->n = C * bz;
    }
    p->has_bounds = false;
    for (int a = 0; a < 3; ++a) { box[2 * a] = hb[2 * a]; box[2 * a + 1] = hb[2 * a + 1] + 1; }
    const int n = p->n;
    float* const x = p->d.as<float>();
    const long long n_plane = (long long)bh * bw, N = n_plane * bz;
    const dim3 grid_apply((unsigned)((n_plane + 256 * kPrepNormPerLane - 1) / (256 * kPrepNormPerLane)), (unsigned)n);
    int* d_keys_in = d_keys + 2 * (size_t)n;
    std::vector<int> keys((size_t)n * 4);
    for (size_t i = 0; i < keys.size(); i += 2) { keys[i] = 0x7FFFFFFF; keys[i + 1] = (int)0x80000000; }
    HIP_TRY(hipMemcpy(d_keys, keys.data(), keys.size() * sizeof(int), hipMemcpyHostToDevice));
    // 3. with a masked channel: the non-zero mask of the volume with its holes filled in 3-D, shared by all channels - rounds of six sweeps over two
    //    bit planes until one adds nothing - and the masked samples of every channel in index order: numpy's `img[m]`, across the slices
    long long n_m = 0;
    const uint8_t* mask = nullptr;
    DevMem d_bits, d_mask, d_dense;
    if (any_masked) {
        const int ww = (bw + 63) / 64;
        const long long rows = (long long)bz * bh, words = rows * ww;
        HIP_TRY(d_bits.alloc(2 * (size_t)words * sizeof(prep_word)));
        prep_word* const d_bg = d_bits.as<prep_word>(); prep_word* const d_out = d_bg + words;
        hipLaunchKernelGGL(prep_fill_planes, dim3((unsigned)((words + 3) / 4)), dim3(256), 0, 0, x, C, bz, bh, bw, d_bg, d_out);
        HIP_TRY(hipGetLastError());
        const long long lines_z = (long long)bh * ww, lines_y = (long long)bz * ww;
        const dim3 grid_z((unsigned)((lines_z + 63) / 64)), grid_y((unsigned)((lines_y + 63) / 64)), grid_x((unsigned)((rows + 63) / 64));
        int round = 0;
        for (; round < kPrepFillMaxRounds; ++round) {
            int added = 0;
            HIP_TRY(hipMemcpy(d_added, &added, sizeof(int), hipMemcpyHostToDevice));
            for (int dir = 1; dir >= -1; dir -= 2)
                hipLaunchKernelGGL(prep_fill_sweep_words, grid_z, dim3(64), 0, 0, d_bg, d_out, lines_z, lines_z, 0ll, lines_z, bz, dir, d_added);
            for (int dir = 1; dir >= -1; dir -= 2)
                hipLaunchKernelGGL(prep_fill_sweep_words, grid_y, dim3(64), 0, 0, d_bg, d_out, lines_y, (long long)ww, lines_z, (long long)ww, bh, dir, d_added);
            hipLaunchKernelGGL(prep_fill_sweep_rows<true>, grid_x, dim3(64), 0, 0, d_bg, d_out, rows, ww, d_added);
            hipLaunchKernelGGL(prep_fill_sweep_rows<false>, grid_x, dim3(64), 0, 0, d_bg, d_out, rows, ww, d_added);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipMemcpy(&added, d_added, sizeof(int), hipMemcpyDeviceToHost));
            if (!added) break;
        }
        if (round == kPrepFillMaxRounds) { *status = TS2D_PLANES_FILL_ROUNDS; return TS2D_OK; }      // every round still added something: numpy's turn
        const int nb = (int)((N + kPrepMaskBlock - 1) / kPrepMaskBlock);
        const size_t o_counts = align_up((size_t)N, 256), o_offs = align_up(o_counts + (size_t)nb * sizeof(int), 256);
        HIP_TRY(d_mask.alloc(o_offs + (size_t)nb * sizeof(int)));
        mask = d_mask.as<uint8_t>();
        hipLaunchKernelGGL(prep_fill_mask_counts, dim3((unsigned)nb), dim3(256), 0, 0, d_out, bw, N, d_mask.as<uint8_t>(), d_mask.as<int>(o_counts));
        hipLaunchKernelGGL(prep_mask_scan, dim3(1), dim3(1024), 0, 0, d_mask.as<int>(o_counts), nb, d_mask.as<int>(o_offs), d_total);
        HIP_TRY(hipGetLastError());
        int total = 0;
        HIP_TRY(hipMemcpy(&total, d_total, sizeof(int), hipMemcpyDeviceToHost));
        if (total < 0 || total > N) return fail(TS2D_ERR_HIP, "%s: the device counted %d masked voxels of %lld", entry, total, N);
        if (total == 0) { *status = TS2D_PLANES_EMPTY_MASK; return TS2D_OK; }      // a volume of zeros: numpy takes the mean of nothing
        n_m = total;
        HIP_TRY(d_dense.alloc((size_t)C * n_m * sizeof(float)));
        hipLaunchKernelGGL(prep_mask_scatter, dim3((unsigned)nb, (unsigned)C), dim3(256), 0, 0, x, N, mask, d_mask.as<int>(o_offs), n_m, d_dense.as<float>());
        HIP_TRY(hipGetLastError());
    }
    // 4. the parameters of every channel, over its WHOLE cropped volume: the z-score statistics of a run of N = bz bh bw samples (numpy's chunks
    //    cross the slices) - of the n_m masked ones for a masked channel -, the minimum and maximum behind Rescale folded over the channel's
    //    slices, the caller's for CT
    std::vector<PrepNorm> norm((size_t)C, PrepNorm{0.f, 1.f});
    std::vector<uint8_t> want((size_t)C);
    bool bad = false;
    if (any_plain) {
        for (int c = 0; c < C; ++c) want[c] = schemes[c] == TS2D_NORM_ZSCORE && !use_mask[c];
        TRY(planes_stats(entry, x, N, C, want.data(), d_norm, d.as<PrepLeaf>(o_leaves), d.as<float>(o_sums), norm.data(), stats, &bad));
    }
    if (any_masked && !bad) {
        for (int c = 0; c < C; ++c) want[c] = schemes[c] == TS2D_NORM_ZSCORE && use_mask[c];
        TRY(planes_stats(entry, d_dense.as<float>(), n_m, C, want.data(), d_norm, d.as<PrepLeaf>(o_leaves), d.as<float>(o_sums), norm.data(), stats, &bad));
    }
    if (any_rescale && !bad) {
        hipLaunchKernelGGL((prep_apply_schemes_stack<false, false>), grid_apply, dim3(256), 0, 0, x, n_plane, bz, nullptr, nullptr, d_keys_in, nullptr);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpy(keys.data() + 2 * (size_t)n, d_keys_in, (size_t)n * 2 * sizeof(int), hipMemcpyDeviceToHost));
    }
    std::vector<PrepScheme> table((size_t)C);
    for (int c = 0; c < C && !bad; ++c) {
        PrepScheme& s = table[c];
        s = PrepScheme{(int)schemes[c], 0, 0.f, 1.f, 0.f, 0.f};
        if (s.id == kPrepZScore) { s.masked = use_mask[c] ? 1 : 0; s.sub = norm[c].mean; s.div = norm[c].div; continue; }      // (stats: mean and std, written above)
        if (s.id == kPrepCT) { s.sub = params[4 * c]; s.div = params[4 * c + 1]; s.lo = params[4 * c + 2]; s.hi = params[4 * c + 3]; }
        if (s.id == kPrepRGB01) s.div = 255.f;
        if (s.id == kPrepRescale01) {
            int klo = 0x7FFFFFFF, khi = (int)0x80000000;
            for (int k = 0; k < bz; ++k) {
                const int* kk = keys.data() + 2 * (size_t)n + 2 * ((size_t)c * bz + k);
                klo = std::min(klo, kk[0]); khi = std::max(khi, kk[1]);
            }
            const float mn = prep_unkey(klo), mx = prep_unkey(khi);
            if (!std::isfinite(mn) || !std::isfinite(mx)) { bad = true; break; }
            // numpy's min() of a volume that holds zeros of both signs and nothing below them returns either: not decided here
            if (mn == 0.f && std::signbit(mn)) *status |= TS2D_PLANES_ZERO_SIGN;
            s.sub = mn; s.div = prep_rescale_div(mn, mx);
        }
        stats[2 * c] = s.sub; stats[2 * c + 1] = s.div;
    }
    if (bad) *status |= TS2D_PLANES_NONFINITE;                     // a non-finite sample (or an overflowing sum)
    if (*status) return TS2D_OK;                                   // nothing is normalised
    // 5. normalise in place by the channel's row (a masked one inside the mask only); the minimum and maximum of each resulting SLICE are the clip bounds of the resample
    HIP_TRY(hipMemcpy(d_table, table.data(), table.size() * sizeof(PrepScheme), hipMemcpyHostToDevice));
    if (any_masked) hipLaunchKernelGGL((prep_apply_schemes_stack<true, true>), grid_apply, dim3(256), 0, 0, x, n_plane, bz, d_table, mask, d_keys, d_status);
    else hipLaunchKernelGGL((prep_apply_schemes_stack<true, false>), grid_apply, dim3(256), 0, 0, x, n_plane, bz, d_table, nullptr, d_keys, d_status);
    HIP_TRY(hipGetLastError());
    TRY(planes_keep_bounds(p, d_keys, &keys, &bad));
    HIP_TRY(hipMemcpy(status, d_status, sizeof(int), hipMemcpyDeviceToHost));
    if (bad) *status |= TS2D_PLANES_NONFINITE;                     // (a quotient overflowed, or a channel that is not normalised holds a non-finite sample)
    if (*status) p->has_bounds = false;                            // (an RGB sample out of range: the slices are no result, nothing resamples them)
    return TS2D_OK;
}

static_assert(kXrStatusNonFinite == TS2D_XR_NONFINITE && kXrStatusRange == TS2D_LABELS_RANGE, "the radiograph entries speak the C header's numbers");

// What ts2d_project_xr and ts2d_project_labels_xr share.  xr_check: every refusal of the view and the geometry, and the ray tables; nothing of the
// device is touched.  xr_upload: the call's one allocation - status word, volume, tables, `out_bytes` of output - with the volume and the tables
// uploaded and the status word cleared.
struct XrCall {
    XrPlan plan;
    XrView view;
    XrTables tb;
    DevMem d;
    int* d_status = nullptr;
    size_t o_vol = 0, o_out = 0;
};

int xr_check(const char* E, const void* volume, size_t n_elems, const XrGeometry& g, long long sz, long long sy, long long sx, long long base, XrCall* c) {
    if (!volume) return fail(TS2D_ERR_INVALID, "%s: volume is null", E);
    TRY(xr_plan(E, g, &c->plan));
    if ((long long)g.nz * g.nx > 0x7FFFFFFFll)          // (the scan: one lane per (z, x) column)
        return fail(TS2D_ERR_INVALID, "%s: planes of nz %d x nx %d are more than 2^31 - 1 samples", E, g.nz, g.nx);
    TRY(check_strided_view(E, n_elems, base, {g.nz, g.ny, g.nx}, {sz, sy, sx}));
    c->view = XrView{g.nz, g.ny, g.nx, sz, sy, sx, base};
    return TS2D_OK;
}

int xr_upload(int device, const void* volume, size_t vbytes, size_t out_bytes, XrCall* c) {
    const XrPlan& pl = c->plan;
    HIP_TRY(hipSetDevice(device));
    ArenaLayout lay;
    const size_t o_status = lay.add(sizeof(int));
    c->o_vol = lay.add(vbytes);
    const size_t nt = pl.t.size(), nu = pl.a.size(), nv = pl.b.size();
    const size_t o_t = lay.add(nt * sizeof(double)), o_a = lay.add(nu * sizeof(double)), o_cx = lay.add(nu * sizeof(double));
    const size_t o_b = lay.add(nv * sizeof(double)), o_cz = lay.add(nv * sizeof(double));
    c->o_out = lay.add(out_bytes);
    HIP_TRY(c->d.alloc(lay.total()));
    c->d_status = c->d.as<int>(o_status);
    HIP_TRY(hipMemset(c->d_status, 0, sizeof(int)));
    HIP_TRY(hipMemcpy(c->d.as<char>(c->o_vol), volume, vbytes, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(c->d.as<char>(o_t), pl.t.data(), nt * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(c->d.as<char>(o_a), pl.a.data(), nu * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(c->d.as<char>(o_cx), pl.cx.data(), nu * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(c->d.as<char>(o_b), pl.b.data(), nv * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(c->d.as<char>(o_cz), pl.cz.data(), nv * sizeof(double), hipMemcpyHostToDevice));
    c->tb = XrTables{c->d.as<const double>(o_t), c->d.as<const double>(o_a), c->d.as<const double>(o_cx), c->d.as<const double>(o_b),
                     c->d.as<const double>(o_cz), pl.nu, pl.nv};
    return TS2D_OK;
}

int project_xr_impl(int device, const void* volume, size_t n_elems, int dtype, const XrGeometry& g, long long sz, long long sy, long long sx,
                    long long base, double air, double water, int clip, double density_max, double* out_sum, float* out_xr, int* status) {
    const char* const E = "ts2d_project_xr";
    if (!status) return fail(TS2D_ERR_INVALID, "%s: status is null", E);
    if (!out_sum && !out_xr) return fail(TS2D_ERR_INVALID, "%s: out_sum_f64 and out_xr_f32 are both null", E);
    if (dtype < 0 || dtype > 4) return fail(TS2D_ERR_INVALID, "%s: dtype %d unknown", E, dtype);
    if (!(std::isfinite(air) && std::isfinite(water))) return fail(TS2D_ERR_INVALID, "%s: air = %g, water = %g are not finite", E, air, water);
    if (water == air) return fail(TS2D_ERR_INVALID, "%s: water == air = %g: no sample value has density 1", E, air);
    if (clip != 0 && clip != 1) return fail(TS2D_ERR_INVALID, "%s: clip %d is neither 0 nor 1", E, clip);
    if (clip && !(density_max >= 0.0)) return fail(TS2D_ERR_INVALID, "%s: density_max = %g is not a number >= 0", E, density_max);
    XrCall c;
    TRY(xr_check(E, volume, n_elems, g, sz, sy, sx, base, &c));
    *status = 0;
    const long long n = (long long)g.nu * g.nv;
    TRY(xr_upload(device, volume, n_elems * sample_size(dtype), (size_t)n * sizeof(double), &c));
    const XrDensity dn = {air, 1.0 / (water - air), clip ? density_max : 0.0, clip};
    double* d_sum = c.d.as<double>(c.o_out);
    by_sample_type(dtype, [&](auto t) {
        using S = typename decltype(t)::type;
        const S* d_vol = c.d.as<const S>(c.o_vol);
        if constexpr (!std::is_integral<S>::value)       // the streaming pre-pass of a float volume: a non-finite sample is a status, not a result
            hipLaunchKernelGGL(xr_scan<S>, dim3((unsigned)(((long long)g.nz * g.nx + kXrThreads - 1) / kXrThreads)), dim3(kXrThreads), 0, 0, d_vol, c.view,
                               -1, c.d_status);
        hipLaunchKernelGGL(project_xr_rays<S>, dim3((unsigned)((n + kXrThreads - 1) / kXrThreads)), dim3(kXrThreads), 0, 0, d_vol, c.view, dn, c.tb, d_sum);
    });
    HIP_TRY(hipGetLastError());
    int st = 0;
    HIP_TRY(hipMemcpy(&st, c.d_status, sizeof(st), hipMemcpyDeviceToHost));       // (waits for the launches: the default stream orders them)
    if (st) { *status = kXrStatusNonFinite; return TS2D_OK; }                      // the sums are no result: the outputs stay untouched
    std::vector<double> own;
    double* sum = out_sum;
    if (!sum) { own.resize((size_t)n); sum = own.data(); }
    HIP_TRY(hipMemcpy(sum, d_sum, (size_t)n * sizeof(double), hipMemcpyDeviceToHost));
    if (out_xr) xr_finish(c.plan, sum, out_xr);
    return TS2D_OK;
}

template <typename T>
void project_labels_xr_launch(const T* d_vol, const XrCall& c, int num, uint8_t* d_out) {
    const long long n = (long long)c.tb.nu * c.tb.nv;
    const dim3 grid((unsigned)((n + kXrThreads - 1) / kXrThreads)), block(kXrThreads);
    hipLaunchKernelGGL(xr_scan<T>, dim3((unsigned)(((long long)c.view.nz * c.view.nx + kXrThreads - 1) / kXrThreads)), block, 0, 0, d_vol, c.view, num,
                       c.d_status);
    if (num <= 32) hipLaunchKernelGGL((project_labels_xr_rays<T, 1>), grid, block, 0, 0, d_vol, c.view, c.tb, num, d_out);
    else if (num <= 64) hipLaunchKernelGGL((project_labels_xr_rays<T, 2>), grid, block, 0, 0, d_vol, c.view, c.tb, num, d_out);
    else if (num <= 128) hipLaunchKernelGGL((project_labels_xr_rays<T, 4>), grid, block, 0, 0, d_vol, c.view, c.tb, num, d_out);
    else hipLaunchKernelGGL((project_labels_xr_rays<T, 8>), grid, block, 0, 0, d_vol, c.view, c.tb, num, d_out);
}

int project_labels_xr_impl(int device, const void* volume, size_t n_elems, int dtype, const XrGeometry& g, long long sz, long long sy, long long sx,
                           long long base, int num, uint8_t* planes, int* status) {
    const char* const E = "ts2d_project_labels_xr";
    if (!planes) return fail(TS2D_ERR_INVALID, "%s: planes_u8 is null", E);
    if (!status) return fail(TS2D_ERR_INVALID, "%s: status is null", E);
    if (dtype < 0 || dtype > 4 || dtype == 2)
        return fail(TS2D_ERR_INVALID, "%s: dtype %d is not an integer type (int16 0, uint8 1, uint16 3, int32 4)", E, dtype);
    if (num < 1 || num > 255) return fail(TS2D_ERR_INVALID, "%s: num = %d outside 1 ... 255", E, num);
    XrCall c;
    TRY(xr_check(E, volume, n_elems, g, sz, sy, sx, base, &c));
    const long long n = (long long)g.nu * g.nv;
    if (n * num > 0x7FFFFFFFll) return fail(TS2D_ERR_INVALID, "%s: %d planes of nv %d x nu %d are more than 2^31 - 1 bytes", E, num, g.nv, g.nu);
    *status = 0;
    const size_t obytes = (size_t)n * num;
    TRY(xr_upload(device, volume, n_elems * sample_size(dtype), obytes, &c));
    uint8_t* d_out = c.d.as<uint8_t>(c.o_out);
    by_sample_type(dtype, [&](auto t) {
        using S = typename decltype(t)::type;
        if constexpr (std::is_integral<S>::value)                  // (float32 was refused above: no kernel of it is built)
            project_labels_xr_launch(c.d.as<const S>(c.o_vol), c, num, d_out);
    });
    HIP_TRY(hipGetLastError());
    int st = 0;
    HIP_TRY(hipMemcpy(&st, c.d_status, sizeof(st), hipMemcpyDeviceToHost));
    if (st) { *status = kXrStatusRange; return TS2D_OK; }                         // a sample outside 0 ... num: no plane is written
    HIP_TRY(hipMemcpy(planes, d_out, obytes, hipMemcpyDeviceToHost));
    return TS2D_OK;
}

}  // namespace
#pragma GCC visibility pop

extern "C" {

int ts2d_project_coronal(int device, const void* volume, size_t n_elems, int dtype, int nz, int ny, int nx, long long sz,
                         long long sy, long long sx, long long base, float* out_max, float* out_mean) {
    return project_coronal_impl(device, volume, n_elems, dtype, nz, ny, nx, sz, sy, sx, base, out_max, out_mean, nullptr, nullptr, nullptr);
}

int ts2d_project_coronal_zscore(int device, const void* volume, size_t n_elems, int dtype, int nz, int ny, int nx, long long sz,
                                long long sy, long long sx, long long base, float* out_max, float* out_mean, float* out_norm,
                                double* out_stats, int32_t* out_box) {
    if (!out_norm) return fail(TS2D_ERR_INVALID, "ts2d_project_coronal_zscore: null argument");
    return project_coronal_impl(device, volume, n_elems, dtype, nz, ny, nx, sz, sy, sx, base, out_max, out_mean, out_norm, out_stats, out_box);
}

int ts2d_project_coronal_modes(int device, const void* volume, size_t n_elems, int dtype, int nz, int ny, int nx, long long sz, long long sy,
                               long long sx, long long base, const int32_t* modes, const int32_t* slice_index, int n_modes, float* out_planes,
                               float* out_norm, double* out_stats, int32_t* out_box, int32_t* status) {
    return project_coronal_modes_impl(device, volume, n_elems, dtype, nz, ny, nx, sz, sy, sx, base, modes, slice_index, n_modes, out_planes, out_norm,
                                      out_stats, out_box, status);
}

int ts2d_project_xr(int device, const void* volume, size_t n_elems, int dtype, int nz, int ny, int nx, long long sz, long long sy, long long sx,
                    long long base, double spacing_x, double spacing_y, double spacing_z, double source_detector_mm, double source_center_mm,
                    int view_pa, int parallel, double du, double dv, int nu, int nv, double air, double water, int clip, double density_max,
                    double* out_sum_f64, float* out_xr_f32, int32_t* status) {
    const XrGeometry g = {nz, ny, nx, spacing_x, spacing_y, spacing_z, source_detector_mm, source_center_mm, view_pa, parallel, du, dv, nu, nv};
    return project_xr_impl(device, volume, n_elems, dtype, g, sz, sy, sx, base, air, water, clip, density_max, out_sum_f64, out_xr_f32, status);
}

int ts2d_project_labels_xr(int device, const void* volume, size_t n_elems, int dtype, int nz, int ny, int nx, long long sz, long long sy,
                           long long sx, long long base, double spacing_x, double spacing_y, double spacing_z, double source_detector_mm,
                           double source_center_mm, int view_pa, int parallel, double du, double dv, int nu, int nv, int num, uint8_t* planes_u8,
                           int32_t* status) {
    const XrGeometry g = {nz, ny, nx, spacing_x, spacing_y, spacing_z, source_detector_mm, source_center_mm, view_pa, parallel, du, dv, nu, nv};
    return project_labels_xr_impl(device, volume, n_elems, dtype, g, sz, sy, sx, base, num, planes_u8, status);
}

int ts2d_resample_cubic(int device, const float* src, int n_planes, int in_h, int in_w, int out_h, int out_w, const float* lo_hi, float* dst) {
    if (!src || !lo_hi || !dst) return fail(TS2D_ERR_INVALID, "ts2d_resample_cubic: null argument");
    if (n_planes < 1) return fail(TS2D_ERR_INVALID, "ts2d_resample_cubic: %d planes", n_planes);
    TRY(rsin_check("ts2d_resample_cubic", n_planes, in_h, in_w, out_h, out_w));
    for (int p = 0; p < n_planes; ++p)
        if (!std::isfinite(lo_hi[2 * p]) || !std::isfinite(lo_hi[2 * p + 1]) || lo_hi[2 * p] > lo_hi[2 * p + 1])
            return fail(TS2D_ERR_INVALID, "ts2d_resample_cubic: plane %d has non-finite or inverted clip bounds [%g, %g] (a plane with a non-finite sample is not computed here)",
                        p, (double)lo_hi[2 * p], (double)lo_hi[2 * p + 1]);
    RsInPlan pl;
    TRY(rsin_plan("ts2d_resample_cubic", n_planes, in_h, in_w, out_h, out_w, &pl));
    HIP_TRY(hipSetDevice(device));
    const size_t n_src = (size_t)n_planes * in_h * in_w, n_dst = (size_t)n_planes * out_h * out_w;
    // [scratch of the plan | source | clip bounds | result]
    const size_t o_src = pl.bytes, o_lh = align_up(o_src + n_src * sizeof(float), 256);
    const size_t o_dst = align_up(o_lh + (size_t)n_planes * 2 * sizeof(float), 256);
    DevMem d;
    HIP_TRY(d.alloc(o_dst + n_dst * sizeof(float)));
    HIP_TRY(hipMemcpy(d.as<char>(o_src), src, n_src * sizeof(float), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d.as<char>(o_lh), lo_hi, (size_t)n_planes * 2 * sizeof(float), hipMemcpyHostToDevice));
    TRY(rsin_run(pl, d.as<char>(), d.as<const float>(o_src), d.as<const float>(o_lh), d.as<float>(o_dst), n_planes, in_h, in_w, out_h, out_w));
    HIP_TRY(hipMemcpy(dst, d.as<float>(o_dst), n_dst * sizeof(float), hipMemcpyDeviceToHost));
    return TS2D_OK;
}

// ---------------------------------------------------------------------------------------------------------------- ts2d_planes
int ts2d_planes_create(int device, const float* src, int n_planes, int h, int w, ts2d_planes** out) {
    return planes_create("ts2d_planes_create", device, src, n_planes, 1, h, w, out);
}

int ts2d_planes_create_stack(int device, const float* src, int channels, int slices, int h, int w, ts2d_planes** out) {
    const char* const entry = "ts2d_planes_create_stack";
    if (out) *out = nullptr;
    if (channels < 1 || slices < 1 || (long long)channels * slices > kPrepMaxPlanes)
        return fail(TS2D_ERR_INVALID, "%s: %d channels of %d slices outside 1 ... %d planes", entry, channels, slices, kPrepMaxPlanes);
    return planes_create(entry, device, src, channels * slices, slices, h, w, out);
}

int ts2d_planes_crop_zscore(ts2d_planes* p, int32_t box[4], float* stats, int* nonfinite) {
    if (!p || !box || !stats || !nonfinite) return fail(TS2D_ERR_INVALID, "ts2d_planes_crop_zscore: null argument");
    *nonfinite = 0;
    if (p->z != 1) return fail(TS2D_ERR_INVALID, "ts2d_planes_crop_zscore: the handle is a stack of %d slices per channel (ts2d_planes_crop_normalize_stack crops and normalises one)", p->z);
    HIP_TRY(hipSetDevice(p->device));
    const int n = p->n;
    // scratch, sized for the uncropped extent: [box | min / max keys | mean, divisor | leaves of the partial chunk | chunk and leaf sums]
    const size_t per_plane = (size_t)((long long)p->h * p->w / kPrepChunk) + kPrepMaxTailLeaves;
    const size_t o_keys = 256, o_norm = align_up(o_keys + (size_t)n * 2 * sizeof(int), 256), o_leaves = align_up(o_norm + (size_t)n * sizeof(PrepNorm), 256);
    const size_t o_sums = align_up(o_leaves + kPrepMaxTailLeaves * sizeof(PrepLeaf), 256);
    DevMem d;
    HIP_TRY(d.alloc(o_sums + (size_t)n * per_plane * sizeof(float)));
    int* d_keys = d.as<int>(o_keys);
    PrepNorm* d_norm = d.as<PrepNorm>(o_norm);
    // 1., 2. crop_to_nonzero's box over all planes and the compaction to it
    TRY(planes_crop("ts2d_planes_crop_zscore", p, d.as<int>(), box));
    float* const x = p->d.as<float>();
    // 3. the two sums of every plane: chunk and leaf sums on the device, their fold and the float32 statistics here
    const long long N = (long long)p->h * p->w;
    std::vector<PrepNorm> norm((size_t)n, PrepNorm{0.f, 1.f});
    bool bad = false;
    TRY(planes_stats("ts2d_planes_crop_zscore", x, N, n, nullptr, d_norm, d.as<PrepLeaf>(o_leaves), d.as<float>(o_sums), norm.data(), stats, &bad));
    if (bad) { *nonfinite = 1; return TS2D_OK; }                   // a non-finite sample (or an overflowing sum): nothing is normalised
    // 4. normalise in place; the minimum and maximum of the result are the clip bounds of the resample
    std::vector<int> keys((size_t)n * 2);
    for (int c = 0; c < n; ++c) { keys[2 * c] = 0x7FFFFFFF; keys[2 * c + 1] = (int)0x80000000; }
    HIP_TRY(hipMemcpy(d_keys, keys.data(), keys.size() * sizeof(int), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(prep_normalise, dim3((unsigned)((N + 256 * kPrepNormPerLane - 1) / (256 * kPrepNormPerLane)), (unsigned)n), dim3(256), 0, 0, x, N, d_norm, d_keys);
    HIP_TRY(hipGetLastError());
    TRY(planes_keep_bounds(p, d_keys, &keys, &bad));
    if (bad) *nonfinite = 1;                                       // (a quotient overflowed: the planes hold it, the caller drops the handle)
    return TS2D_OK;
}

int ts2d_planes_crop_normalize(ts2d_planes* p, const int32_t* schemes, const float* params, const uint8_t* use_mask, int32_t box[4], float* stats,
                               int* status) {
    const char* const entry = "ts2d_planes_crop_normalize";
    if (!p || !schemes || !params || !use_mask || !box || !stats || !status) return fail(TS2D_ERR_INVALID, "%s: null argument", entry);
    *status = 0;
    if (p->z != 1) return fail(TS2D_ERR_INVALID, "%s: the handle is a stack of %d slices per channel (ts2d_planes_crop_normalize_stack crops and normalises one)", entry, p->z);
    const int n = p->n;
    bool any_plain = false, any_masked = false, any_rescale = false;
    for (int c = 0; c < n; ++c) {
        if (schemes[c] < TS2D_NORM_ZSCORE || schemes[c] > TS2D_NORM_NONE) return fail(TS2D_ERR_INVALID, "%s: plane %d has the unknown scheme %d", entry, c, (int)schemes[c]);
        if (schemes[c] == TS2D_NORM_CT)
            for (int k = 0; k < 4; ++k)
                if (!std::isfinite(params[4 * c + k]))
                    return fail(TS2D_ERR_INVALID, "%s: plane %d has the non-finite CT parameter %g at [%d] (mean, divisor, lower bound, upper bound)", entry, c, (double)params[4 * c + k], k);
        const bool masked = schemes[c] == TS2D_NORM_ZSCORE && use_mask[c];
        any_masked |= masked; any_plain |= schemes[c] == TS2D_NORM_ZSCORE && !masked; any_rescale |= schemes[c] == TS2D_NORM_RESCALE01;
    }
    HIP_TRY(hipSetDevice(p->device));
    // scratch, sized for the uncropped extent: [box, n_m, status | min / max keys, of the result and of the input | mean, divisor | scheme table |
    //                                           leaves of the partial chunk | chunk and leaf sums]
    const size_t per_plane = (size_t)((long long)p->h * p->w / kPrepChunk) + kPrepMaxTailLeaves;
    const size_t o_keys = 256, o_norm = align_up(o_keys + (size_t)n * 4 * sizeof(int), 256), o_table = align_up(o_norm + (size_t)n * sizeof(PrepNorm), 256);
    const size_t o_leaves = align_up(o_table + (size_t)n * sizeof(PrepScheme), 256), o_sums = align_up(o_leaves + kPrepMaxTailLeaves * sizeof(PrepLeaf), 256);
    DevMem d, d_mask, d_dense;
    HIP_TRY(d.alloc(o_sums + (size_t)n * per_plane * sizeof(float)));
    int* d_total = d.as<int>(4 * sizeof(int)); int* d_status = d_total + 1;
    int* d_keys = d.as<int>(o_keys); int* d_keys_in = d_keys + 2 * (size_t)n;
    PrepNorm* d_norm = d.as<PrepNorm>(o_norm); PrepScheme* d_table = d.as<PrepScheme>(o_table);
    PrepLeaf* d_leaves = d.as<PrepLeaf>(o_leaves); float* d_sums = d.as<float>(o_sums);
    // 1., 2. crop_to_nonzero's box over all planes and the compaction to it
    TRY(planes_crop(entry, p, d.as<int>(), box));
    float* const x = p->d.as<float>();
    const long long N = (long long)p->h * p->w;
    const dim3 grid_apply((unsigned)((N + 256 * kPrepNormPerLane - 1) / (256 * kPrepNormPerLane)), (unsigned)n);
    std::vector<int> keys((size_t)n * 4);
    for (size_t i = 0; i < keys.size(); i += 2) { keys[i] = 0x7FFFFFFF; keys[i + 1] = (int)0x80000000; }
    const int zero2[2] = {0, 0};
    HIP_TRY(hipMemcpy(d_keys, keys.data(), keys.size() * sizeof(int), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_total, zero2, sizeof(zero2), hipMemcpyHostToDevice));
    // 3. the non-zero mask inside the box (nnU-Net's `seg >= 0` for one slice), shared by all planes, and the masked samples of every plane
    //    in index order: numpy's `img[m]`
    long long n_m = 0;
    const uint8_t* mask = nullptr;
    if (any_masked) {
        const int nb = (int)((N + kPrepMaskBlock - 1) / kPrepMaskBlock);
        const size_t o_counts = align_up((size_t)N, 256), o_offs = align_up(o_counts + (size_t)nb * sizeof(int), 256);
        HIP_TRY(d_mask.alloc(o_offs + (size_t)nb * sizeof(int)));
        mask = d_mask.as<uint8_t>();
        hipLaunchKernelGGL(prep_mask_counts, dim3((unsigned)nb), dim3(256), 0, 0, x, n, N, d_mask.as<uint8_t>(), d_mask.as<int>(o_counts));
        hipLaunchKernelGGL(prep_mask_scan, dim3(1), dim3(1024), 0, 0, d_mask.as<int>(o_counts), nb, d_mask.as<int>(o_offs), d_total);
        HIP_TRY(hipGetLastError());
        int total = 0;
        HIP_TRY(hipMemcpy(&total, d_total, sizeof(int), hipMemcpyDeviceToHost));
        if (total < 0 || total > N) return fail(TS2D_ERR_HIP, "%s: the device counted %d masked pixels of %lld", entry, total, N);
        if (total == 0) { *status = TS2D_PLANES_EMPTY_MASK; return TS2D_OK; }      // an image of zeros: numpy takes the mean of nothing
        n_m = total;
        HIP_TRY(d_dense.alloc((size_t)n * n_m * sizeof(float)));
        hipLaunchKernelGGL(prep_mask_scatter, dim3((unsigned)nb, (unsigned)n), dim3(256), 0, 0, x, N, mask, d_mask.as<int>(o_offs), n_m, d_dense.as<float>());
        HIP_TRY(hipGetLastError());
    }
    // 4. the parameters of every plane: the z-score statistics (of the whole plane, or of its masked samples), the minimum and maximum
    //    behind Rescale, the caller's for CT
    std::vector<PrepNorm> norm((size_t)n, PrepNorm{0.f, 1.f});
    std::vector<uint8_t> want((size_t)n);
    bool bad = false;
    if (any_plain) {
        for (int c = 0; c < n; ++c) want[c] = schemes[c] == TS2D_NORM_ZSCORE && !use_mask[c];
        TRY(planes_stats(entry, x, N, n, want.data(), d_norm, d_leaves, d_sums, norm.data(), stats, &bad));
    }
    if (any_masked && !bad) {
        for (int c = 0; c < n; ++c) want[c] = schemes[c] == TS2D_NORM_ZSCORE && use_mask[c];
        TRY(planes_stats(entry, d_dense.as<float>(), n_m, n, want.data(), d_norm, d_leaves, d_sums, norm.data(), stats, &bad));
    }
    if (any_rescale && !bad) {
        hipLaunchKernelGGL(prep_apply_schemes<false>, grid_apply, dim3(256), 0, 0, x, N, nullptr, nullptr, d_keys_in, nullptr);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpy(keys.data() + 2 * (size_t)n, d_keys_in, (size_t)n * 2 * sizeof(int), hipMemcpyDeviceToHost));
    }
    std::vector<PrepScheme> table((size_t)n);
    for (int c = 0; c < n && !bad; ++c) {
        PrepScheme& s = table[c];
        s = PrepScheme{(int)schemes[c], 0, 0.f, 1.f, 0.f, 0.f};
        if (s.id == kPrepZScore) { s.masked = use_mask[c] ? 1 : 0; s.sub = norm[c].mean; s.div = norm[c].div; continue; }      // (stats: mean and std, written above)
        if (s.id == kPrepCT) { s.sub = params[4 * c]; s.div = params[4 * c + 1]; s.lo = params[4 * c + 2]; s.hi = params[4 * c + 3]; }
        if (s.id == kPrepRGB01) s.div = 255.f;
        if (s.id == kPrepRescale01) {
            const float mn = prep_unkey(keys[2 * (size_t)n + 2 * c]), mx = prep_unkey(keys[2 * (size_t)n + 2 * c + 1]);
            if (!std::isfinite(mn) || !std::isfinite(mx)) { bad = true; break; }
            // numpy's min() of a plane that holds zeros of both signs and nothing below them returns either: not decided here
            if (mn == 0.f && std::signbit(mn)) *status |= TS2D_PLANES_ZERO_SIGN;
            s.sub = mn; s.div = prep_rescale_div(mn, mx);
        }
        stats[2 * c] = s.sub; stats[2 * c + 1] = s.div;
    }
    if (bad) *status |= TS2D_PLANES_NONFINITE;                     // a non-finite sample (or an overflowing sum)
    if (*status) return TS2D_OK;                                   // nothing is normalised
    // 5. normalise in place; the minimum and maximum of the result are the clip bounds of the resample
    HIP_TRY(hipMemcpy(d_table, table.data(), table.size() * sizeof(PrepScheme), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(prep_apply_schemes<true>, grid_apply, dim3(256), 0, 0, x, N, d_table, mask, d_keys, d_status);
    HIP_TRY(hipGetLastError());
    TRY(planes_keep_bounds(p, d_keys, &keys, &bad));
    HIP_TRY(hipMemcpy(status, d_status, sizeof(int), hipMemcpyDeviceToHost));
    if (bad) *status |= TS2D_PLANES_NONFINITE;                     // (a quotient overflowed, or a plane that is not normalised holds a non-finite sample)
    if (*status) p->has_bounds = false;                            // (an RGB sample out of range: the planes are no result, nothing resamples them)
    return TS2D_OK;
}

int ts2d_planes_crop_normalize_stack(ts2d_planes* p, const int32_t* schemes, const float* params, const uint8_t* use_mask, int32_t box[6], float* stats,
                                     int* status) {
    return planes_crop_normalize_stack("ts2d_planes_crop_normalize_stack", false, p, schemes, params, use_mask, box, stats, status);
}

int ts2d_planes_crop_normalize_stack_masked(ts2d_planes* p, const int32_t* schemes, const float* params, const uint8_t* use_mask, int32_t box[6],
                                            float* stats, int* status) {
    return planes_crop_normalize_stack("ts2d_planes_crop_normalize_stack_masked", true, p, schemes, params, use_mask, box, stats, status);
}

int ts2d_planes_resample_cubic(ts2d_planes* p, int out_h, int out_w) {
    if (!p) return fail(TS2D_ERR_INVALID, "ts2d_planes_resample_cubic: null argument");
    const int in_h = p->h, in_w = p->w, n = p->n;
    TRY(rsin_check("ts2d_planes_resample_cubic", n, in_h, in_w, out_h, out_w));
    if (!p->has_bounds)
        return fail(TS2D_ERR_STATE, "ts2d_planes_resample_cubic: the planes carry no clip bounds (ts2d_planes_crop_zscore computes them; a resample uses them up)");
    RsInPlan pl;
    TRY(rsin_plan("ts2d_planes_resample_cubic", n, in_h, in_w, out_h, out_w, &pl));
    HIP_TRY(hipSetDevice(p->device));
    DevMem d_scratch, d_dst;
    HIP_TRY(d_scratch.alloc(pl.bytes));
    HIP_TRY(d_dst.alloc((size_t)n * out_h * out_w * sizeof(float)));
    TRY(rsin_run(pl, d_scratch.as<char>(), p->d.as<float>(), p->d_lh.as<float>(), d_dst.as<float>(), n, in_h, in_w, out_h, out_w));
    HIP_TRY(hipDeviceSynchronize());
    p->d = std::move(d_dst); p->h = out_h; p->w = out_w; p->has_bounds = false;
    return TS2D_OK;
}

int ts2d_planes_extent(const ts2d_planes* p, int* h, int* w) {
    if (!p || !h || !w) return fail(TS2D_ERR_INVALID, "ts2d_planes_extent: null argument");
    *h = p->h; *w = p->w;
    return TS2D_OK;
}

int ts2d_planes_download(const ts2d_planes* p, float* dst) {
    if (!p || !dst) return fail(TS2D_ERR_INVALID, "ts2d_planes_download: null argument");
    HIP_TRY(hipSetDevice(p->device));
    HIP_TRY(hipMemcpy(dst, p->d.as<float>(), (size_t)p->n * p->h * p->w * sizeof(float), hipMemcpyDeviceToHost));
    return TS2D_OK;
}

int ts2d_planes_destroy(ts2d_planes* p) {
    if (!p) return TS2D_OK;
    (void)hipSetDevice(p->device);
    delete p;
    return TS2D_OK;
}

int ts2d_synth_slices(int device, unsigned long long key, unsigned long long first_element, unsigned long long n_elements,
                      float* out_device, void* stream) {
    if (!out_device) return fail(TS2D_ERR_INVALID, "ts2d_synth_slices: null output");
    if (n_elements == 0) return TS2D_OK;
    if (n_elements > (1ull << 40)) return fail(TS2D_ERR_INVALID, "ts2d_synth_slices: %llu elements in one call", n_elements);
    HIP_TRY(hipSetDevice(device));
    const unsigned long long per = 1ull << 30;                      // <= 2^30 elements per launch (grid of 2^22 blocks)
    for (unsigned long long o = 0; o < n_elements; o += per) {
        const unsigned long long m = std::min(per, n_elements - o);
        hipLaunchKernelGGL(synth_normal, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                           out_device + o, key, first_element + o, m);
        HIP_TRY(hipGetLastError());
    }
    return TS2D_OK;
}

}  // extern "C"
