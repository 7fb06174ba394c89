// The input side of libts2d_engine.so, none of which needs an engine: coronal projection + z-score of a volume, the order-3 resample to the
// plan spacing, and the ts2d_planes handle (crop box, z-score and resample of native 2-D inputs where they lie on the device).
// The host arithmetic behind them is prep_plan.cpp; every device buffer of a call is a DevMem, so HIP_TRY may return wherever it fails.
#include "engine_internal.h"
#include "kernels_project.h"
#include "kernels_resample_in.h"
#include "kernels_prep.h"

#include <algorithm>
#include <cmath>
#include <vector>

using namespace ts2d;

#pragma GCC visibility push(hidden)
// Planes that stay on the device between the steps of nnU-Net's preprocessing of a native 2-D input (kernels_prep.h): uploaded once,
// cropped, z-scored and resampled where they lie, downloaded once.
struct ts2d_planes {
    int device = 0;
    int n = 0, h = 0, w = 0;
    DevMem d;                   // float [n][h][w]
    DevMem d_lh;                // float [n][2]: float32 minimum and maximum of each plane, valid while has_bounds
    bool has_bounds = false;
};

namespace {

constexpr int kPrepMaxPlanes = 65535;           // (a grid dimension)
constexpr long long kPrepMaxSamples = 1ll << 28;

int project_coronal_impl(int device, const void* volume, size_t n_elems, int dtype, int nz, int ny, int nx, long long sz,
                         long long sy, long long sx, long long base, float* out_max, float* out_mean, float* out_norm, double* out_stats, int* out_box) {
    if (!volume || !out_max || !out_mean) return fail(TS2D_ERR_INVALID, "ts2d_project_coronal: null argument");
    static const int esize[5] = {2, 1, 4, 2, 4};
    if (dtype < 0 || dtype > 4 || nz < 1 || ny < 1 || nx < 1) return fail(TS2D_ERR_INVALID, "ts2d_project_coronal: bad dtype / extents");
    {   // every element the view can touch must lie inside the buffer
        long long lo = base, hi = base;
        const long long ext[3] = {(long long)(nz - 1) * sz, (long long)(ny - 1) * sy, (long long)(nx - 1) * sx};
        for (int k = 0; k < 3; ++k) { if (ext[k] < 0) lo += ext[k]; else hi += ext[k]; }
        if (lo < 0 || hi >= (long long)n_elems) return fail(TS2D_ERR_INVALID, "ts2d_project_coronal: the strided view leaves the buffer");
    }
    HIP_TRY(hipSetDevice(device));
    const size_t vbytes = n_elems * esize[dtype], obytes = (size_t)nz * nx * sizeof(float);
    // [volume | max | mean (contiguous: the two channels of the z-score) | normalised x 2 | partial sums | stats | box]
    const size_t o_proj = align_up(vbytes, 256), o_norm = align_up(o_proj + 2 * obytes, 256), o_part = align_up(o_norm + 2 * obytes, 256);
    const size_t o_stats = o_part + 2 * kZBlocks * sizeof(double), o_box = o_stats + 4 * sizeof(double);
    DevMem d;
    HIP_TRY(d.alloc(o_box + 4 * sizeof(int)));
    float* d_max = d.as<float>(o_proj);
    float* d_mean = d_max + (size_t)nz * nx;
    HIP_TRY(hipMemcpy(d.as<char>(), volume, vbytes, hipMemcpyHostToDevice));
    const unsigned grid = (unsigned)(((long long)nz * nx + 255) / 256);
    switch (dtype) {
        case 0: hipLaunchKernelGGL(project_coronal<int16_t>, dim3(grid), dim3(256), 0, 0, d.as<const int16_t>(), nz, ny, nx, sz, sy, sx, base, d_max, d_mean); break;
        case 1: hipLaunchKernelGGL(project_coronal<uint8_t>, dim3(grid), dim3(256), 0, 0, d.as<const uint8_t>(), nz, ny, nx, sz, sy, sx, base, d_max, d_mean); break;
        case 2: hipLaunchKernelGGL(project_coronal<float>, dim3(grid), dim3(256), 0, 0, d.as<const float>(), nz, ny, nx, sz, sy, sx, base, d_max, d_mean); break;
        case 3: hipLaunchKernelGGL(project_coronal<uint16_t>, dim3(grid), dim3(256), 0, 0, d.as<const uint16_t>(), nz, ny, nx, sz, sy, sx, base, d_max, d_mean); break;
        default: hipLaunchKernelGGL(project_coronal<int32_t>, dim3(grid), dim3(256), 0, 0, d.as<const int32_t>(), nz, ny, nx, sz, sy, sx, base, d_max, d_mean); break;
    }
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
    if (!src || !out) return fail(TS2D_ERR_INVALID, "ts2d_planes_create: null argument");
    *out = nullptr;
    if (n_planes < 1 || n_planes > kPrepMaxPlanes) return fail(TS2D_ERR_INVALID, "ts2d_planes_create: %d planes outside 1 ... %d", n_planes, kPrepMaxPlanes);
    if (h < 1 || w < 1 || h > kRsInMaxExtent || w > kRsInMaxExtent)
        return fail(TS2D_ERR_INVALID, "ts2d_planes_create: extents %d x %d outside 1 ... %d", h, w, kRsInMaxExtent);
    if ((long long)n_planes * h * w > kPrepMaxSamples)
        return fail(TS2D_ERR_INVALID, "ts2d_planes_create: %d planes of %d x %d are more than one handle takes (2^28 samples)", n_planes, h, w);
    HIP_TRY(hipSetDevice(device));
    const size_t bytes = (size_t)n_planes * h * w * sizeof(float);
    DevMem d, d_lh;
    HIP_TRY(d.alloc(bytes));
    HIP_TRY(d_lh.alloc((size_t)n_planes * 2 * sizeof(float)));
    HIP_TRY(hipMemcpy(d.as<float>(), src, bytes, hipMemcpyHostToDevice));
    ts2d_planes* p = new ts2d_planes();
    p->device = device; p->n = n_planes; p->h = h; p->w = w; p->d = std::move(d); p->d_lh = std::move(d_lh);
    *out = p;
    return TS2D_OK;
}

int ts2d_planes_crop_zscore(ts2d_planes* p, int32_t box[4], float* stats, int* nonfinite) {
    if (!p || !box || !stats || !nonfinite) return fail(TS2D_ERR_INVALID, "ts2d_planes_crop_zscore: null argument");
    *nonfinite = 0;
    HIP_TRY(hipSetDevice(p->device));
    const int n = p->n;
    // scratch, sized for the uncropped extent: [box | min / max keys | mean, divisor | leaves of the partial chunk | chunk and leaf sums]
    const size_t per_plane = (size_t)((long long)p->h * p->w / kPrepChunk) + kPrepMaxTailLeaves;
    const size_t o_keys = 256, o_norm = align_up(o_keys + (size_t)n * 2 * sizeof(int), 256), o_leaves = align_up(o_norm + (size_t)n * sizeof(PrepNorm), 256);
    const size_t o_sums = align_up(o_leaves + kPrepMaxTailLeaves * sizeof(PrepLeaf), 256);
    DevMem d;
    HIP_TRY(d.alloc(o_sums + (size_t)n * per_plane * sizeof(float)));
    int* d_box = d.as<int>(); int* d_keys = d.as<int>(o_keys);
    PrepNorm* d_norm = d.as<PrepNorm>(o_norm); PrepLeaf* d_leaves = d.as<PrepLeaf>(o_leaves);
    float* d_sums = d.as<float>(o_sums);
    // 1. crop_to_nonzero's box over all planes
    int hb[4] = {p->h, -1, p->w, -1};
    HIP_TRY(hipMemcpy(d_box, hb, sizeof(hb), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(prep_nonzero_box, dim3((unsigned)(((long long)p->h * p->w + 255) / 256)), dim3(256), 0, 0, p->d.as<float>(), n, p->h, p->w, d_box);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(hb, d_box, sizeof(hb), hipMemcpyDeviceToHost));
    if (hb[1] < 0) { hb[0] = 0; hb[1] = p->h - 1; hb[2] = 0; hb[3] = p->w - 1; }            // nothing but zeros: the whole extent stays
    if (hb[0] < 0 || hb[1] >= p->h || hb[0] > hb[1] || hb[2] < 0 || hb[3] >= p->w || hb[2] > hb[3])
        return fail(TS2D_ERR_HIP, "ts2d_planes_crop_zscore: the device returned the box rows %d ... %d, columns %d ... %d of %d x %d", hb[0], hb[1], hb[2], hb[3], p->h, p->w);
    const int bh = hb[1] - hb[0] + 1, bw = hb[3] - hb[2] + 1;
    // 2. compaction: the flattened index of the dense [n][bh][bw] buffer is numpy's
    if (bh != p->h || bw != p->w) {
        DevMem d_new;
        HIP_TRY(d_new.alloc((size_t)n * bh * bw * sizeof(float)));
        for (int c = 0; c < n; ++c)
            HIP_TRY(hipMemcpy2D(d_new.as<float>() + (size_t)c * bh * bw, (size_t)bw * sizeof(float), p->d.as<float>() + ((size_t)c * p->h + hb[0]) * p->w + hb[2],
                                (size_t)p->w * sizeof(float), (size_t)bw * sizeof(float), (size_t)bh, hipMemcpyDeviceToDevice));
        p->d = std::move(d_new); p->h = bh; p->w = bw;
    }
    float* const x = p->d.as<float>();
    p->has_bounds = false;
    box[0] = hb[0]; box[1] = hb[1] + 1; box[2] = hb[2]; box[3] = hb[3] + 1;
    // 3. the two sums of every plane: chunk and leaf sums on the device, their fold and the float32 statistics here
    const long long N = (long long)bh * bw, n_full = N / kPrepChunk;
    std::vector<PrepLeaf> leaves;
    if (N % kPrepChunk) prep_leaves(0, (int)(N % kPrepChunk), &leaves);
    if ((int)leaves.size() > kPrepMaxTailLeaves) return fail(TS2D_ERR_INVALID, "ts2d_planes_crop_zscore: %zu leaves in a partial chunk", leaves.size());
    const size_t n_out = (size_t)n_full + leaves.size();
    const dim3 grid_sums((unsigned)(n_full + (leaves.empty() ? 0 : 1)), (unsigned)n);
    std::vector<float> sums((size_t)n * n_out);
    std::vector<PrepNorm> norm((size_t)n, PrepNorm{0.f, 1.f});
    if (!leaves.empty()) HIP_TRY(hipMemcpy(d_leaves, leaves.data(), leaves.size() * sizeof(PrepLeaf), hipMemcpyHostToDevice));
    bool bad = false;
    for (int pass = 0; pass < 2; ++pass) {
        if (pass == 0) hipLaunchKernelGGL(prep_chunk_sums<0>, grid_sums, dim3(512), 0, 0, x, N, d_norm, d_leaves, (int)leaves.size(), d_sums);
        else hipLaunchKernelGGL(prep_chunk_sums<1>, grid_sums, dim3(512), 0, 0, x, N, d_norm, d_leaves, (int)leaves.size(), d_sums);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpy(sums.data(), d_sums, sums.size() * sizeof(float), hipMemcpyDeviceToHost));
        for (int c = 0; c < n; ++c) {
            // numpy divides the float32 sum by the count in float64 and rounds once to float32 (`ret / rcount` with an intp count)
            const float q = (float)((double)prep_plane_sum(sums.data() + (size_t)c * n_out, N) / (double)N);
            if (!std::isfinite(q)) bad = true;
            if (pass == 0) { norm[c].mean = q; stats[2 * c] = q; }
            else { const float sd = std::sqrt(q); stats[2 * c + 1] = sd; norm[c].div = 1e-8 > (double)sd ? (float)1e-8 : sd; }   // max(std, 1e-8)
        }
        if (bad) { *nonfinite = 1; return TS2D_OK; }               // a non-finite sample (or an overflowing sum): nothing is normalised
        HIP_TRY(hipMemcpy(d_norm, norm.data(), norm.size() * sizeof(PrepNorm), hipMemcpyHostToDevice));
    }
    // 4. normalise in place; the minimum and maximum of the result are the clip bounds of the resample
    std::vector<int> keys((size_t)n * 2);
    for (int c = 0; c < n; ++c) { keys[2 * c] = 0x7FFFFFFF; keys[2 * c + 1] = (int)0x80000000; }
    HIP_TRY(hipMemcpy(d_keys, keys.data(), keys.size() * sizeof(int), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(prep_normalise, dim3((unsigned)((N + 256 * kPrepNormPerLane - 1) / (256 * kPrepNormPerLane)), (unsigned)n), dim3(256), 0, 0, x, N, d_norm, d_keys);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(keys.data(), d_keys, keys.size() * sizeof(int), hipMemcpyDeviceToHost));
    std::vector<float> lh((size_t)n * 2);
    for (size_t i = 0; i < lh.size(); ++i) { lh[i] = prep_unkey(keys[i]); if (!std::isfinite(lh[i])) bad = true; }
    if (bad) { *nonfinite = 1; return TS2D_OK; }                   // (a quotient overflowed: the planes hold it, the caller drops the handle)
    HIP_TRY(hipMemcpy(p->d_lh.as<float>(), lh.data(), lh.size() * sizeof(float), hipMemcpyHostToDevice));
    p->has_bounds = true;
    return TS2D_OK;
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
