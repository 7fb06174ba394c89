// The PNG visuals behind Result.save of libts2d_engine.so, which need no engine: the label visual (flatten, nearest resample, colour) and the
// grey visual (order-3 resample, window) of visual.py on the device (kernels_visual.h; host tables: visual_plan.cpp).  Host pointers in and
// out, one call = uploads, a few launches on the default stream, downloads; every device buffer of a call is a DevMem, so HIP_TRY may return
// wherever it fails.
#include "engine_internal.h"
#include "entry_util.h"
#include "kernels_visual.h"

#include <cmath>
#include <cstring>
#include <vector>

using namespace ts2d;

static_assert(kVisStatusNonfinite == TS2D_VISUAL_NONFINITE, "the status bit speaks the C header's number");

namespace {

// what both entries check of the geometry, by name: the extents, the spacings, and that the caller's output extents are the plan's
int visual_geometry(const char* entry, int H, int W, double spacing_h, double spacing_w, int out_h, int out_w) {
    if (H < 1 || W < 1 || H > kVisMaxExtent || W > kVisMaxExtent)
        return fail(TS2D_ERR_INVALID, "%s: extents %d x %d outside 1 ... %d", entry, H, W, kVisMaxExtent);
    if (!(std::isfinite(spacing_h) && std::isfinite(spacing_w) && spacing_h > 0.0 && spacing_w > 0.0))
        return fail(TS2D_ERR_INVALID, "%s: spacing %g x %g must be finite and positive", entry, spacing_h, spacing_w);
    const double m = spacing_h < spacing_w ? spacing_h : spacing_w;
    const int mh = visual_axis_extent(H, spacing_h, m), mw = visual_axis_extent(W, spacing_w, m);
    if (mh < 0 || mw < 0 || (long long)mh * mw > (1ll << 28))
        return fail(TS2D_ERR_INVALID, "%s: %d x %d at spacing %g x %g resamples to more than one call takes (%d per axis, 2^28 pixels)", entry, H, W,
                    spacing_h, spacing_w, kVisMaxOutExtent);
    if (mh != out_h || mw != out_w)
        return fail(TS2D_ERR_INVALID, "%s: out_h x out_w = %d x %d, the resample gives %d x %d", entry, out_h, out_w, mh, mw);
    return TS2D_OK;
}

void visual_tables(int H, int W, double spacing_h, double spacing_w, int out_h, int out_w, std::vector<VisTap>* taps) {
    const double m = spacing_h < spacing_w ? spacing_h : spacing_w;
    taps->resize((size_t)out_h + out_w);
    visual_axis_table(H, spacing_h, m, out_h, taps->data());
    visual_axis_table(W, spacing_w, m, out_w, taps->data() + out_h);
}

float visual_unkey(int key) { const int b = key < 0 ? key ^ 0x7FFFFFFF : key; float f; std::memcpy(&f, &b, 4); return f; }

template <int DT>
void launch_grey_resample(bool cubic, const void* d_src, int H, int W, int out_h, int out_w, const VisAxis& ax_h, const VisAxis& ax_w,
                          const double* d_zpow, double* d_coef, const VisTap* d_taps, int* d_res, VisCtl* d_ctl) {
    const dim3 grid((unsigned)((out_w + 63) / 64), (unsigned)out_h), block(64);
    if (cubic) {
        hipLaunchKernelGGL(visual_prefilter_cols<DT>, dim3((unsigned)((W + 63) / 64)), block, 0, 0, d_src, H, W, ax_h, d_zpow, d_coef, d_ctl);
        hipLaunchKernelGGL(visual_prefilter_rows, dim3((unsigned)((H + 63) / 64)), block, 0, 0, d_coef, H, W, ax_w, d_zpow);
        hipLaunchKernelGGL(visual_interp_cast<DT>, grid, block, 0, 0, d_coef, W, out_h, out_w, d_taps, d_res, d_ctl);
    } else {
        hipLaunchKernelGGL(visual_gather_nearest<DT>, grid, block, 0, 0, d_src, W, out_h, out_w, d_taps, d_res, d_ctl);
    }
}

}  // namespace

int ts2d_visual_labels(int device, const uint8_t* planes, int K, int H, int W, double spacing_h, double spacing_w, const uint8_t* palette,
                       int n_palette, int out_h, int out_w, uint8_t* rgb) {
    const char* const entry = "ts2d_visual_labels";
    if (!planes || !palette || !rgb) return fail(TS2D_ERR_INVALID, "%s: null argument", entry);
    if (K < 1 || K > 255) return fail(TS2D_ERR_INVALID, "%s: K = %d planes outside 1 ... 255 (the index map is uint8)", entry, K);
    if (n_palette < 1 || n_palette > 256) return fail(TS2D_ERR_INVALID, "%s: n_palette = %d colours outside 1 ... 256", entry, n_palette);
    TRY(visual_geometry(entry, H, W, spacing_h, spacing_w, out_h, out_w));
    std::vector<VisTap> taps;
    visual_tables(H, W, spacing_h, spacing_w, out_h, out_w, &taps);
    uint32_t lut[256];
    visual_color_lut(palette, n_palette, lut);
    HIP_TRY(hipSetDevice(device));
    const size_t n = (size_t)H * W, stride = align_up(n, 16), n_out = (size_t)out_h * out_w;
    ArenaLayout lay;
    const size_t o_lut = lay.add(sizeof(lut)), o_taps = lay.add(taps.size() * sizeof(VisTap)), o_idx = lay.add(stride), o_rgb = lay.add(3 * n_out);
    const size_t o_planes = lay.add(K > 1 ? (size_t)K * stride : 0);          // at a stride of a multiple of 16
    DevMem d;
    HIP_TRY(d.alloc(lay.total()));
    HIP_TRY(hipMemcpy(d.as<char>(o_lut), lut, sizeof(lut), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d.as<char>(o_taps), taps.data(), taps.size() * sizeof(VisTap), hipMemcpyHostToDevice));
    uint8_t* const d_idx = d.as<uint8_t>(o_idx);
    if (K > 1) {
        HIP_TRY(hipMemcpy2D(d.as<char>(o_planes), stride, planes, n, n, (size_t)K, hipMemcpyHostToDevice));
        hipLaunchKernelGGL(visual_flatten, dim3((unsigned)((n + 4095) / 4096)), dim3(256), 0, 0, d.as<const uint8_t>(o_planes), K, (long long)n,
                           (long long)stride, d_idx);
    } else {
        HIP_TRY(hipMemcpy(d_idx, planes, n, hipMemcpyHostToDevice));      // K = 1 is a label map: it is its own index map
    }
    hipLaunchKernelGGL(visual_label_rgb, dim3((unsigned)((out_w + 255) / 256), (unsigned)out_h), dim3(64), 0, 0, d_idx, W, out_h, out_w,
                       d.as<const VisTap>(o_taps), d.as<const uint32_t>(o_lut), d.as<uint8_t>(o_rgb));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(rgb, d.as<char>(o_rgb), 3 * n_out, hipMemcpyDeviceToHost));
    return TS2D_OK;
}

int ts2d_visual_grey(int device, const void* plane, int dtype, int H, int W, double spacing_h, double spacing_w, int cubic, double lo, double hi,
                     int auto_lo, int auto_hi, int out_h, int out_w, uint8_t* grey, double* window_used, int* status) {
    const char* const entry = "ts2d_visual_grey";
    if (!plane || !grey || !window_used || !status) return fail(TS2D_ERR_INVALID, "%s: null argument", entry);
    *status = 0;
    if (dtype < 0 || dtype > 4) return fail(TS2D_ERR_INVALID, "%s: dtype %d unknown (0 int16, 1 uint8, 2 float32, 3 uint16, 4 int32)", entry, dtype);
    if (cubic != 0 && cubic != 1) return fail(TS2D_ERR_INVALID, "%s: cubic = %d is neither 0 (nearest) nor 1", entry, cubic);
    if (cubic && dtype == 1) return fail(TS2D_ERR_INVALID, "%s: a uint8 plane takes the nearest path (cubic = 0)", entry);
    if ((!auto_lo && !std::isfinite(lo)) || (!auto_hi && !std::isfinite(hi)))
        return fail(TS2D_ERR_INVALID, "%s: window %g ... %g is not finite", entry, lo, hi);
    TRY(visual_geometry(entry, H, W, spacing_h, spacing_w, out_h, out_w));
    if (cubic && (H < 2 || W < 2)) return fail(TS2D_ERR_INVALID, "%s: the cubic resample needs extents of at least 2, found %d x %d", entry, H, W);
    std::vector<VisTap> taps;
    visual_tables(H, W, spacing_h, spacing_w, out_h, out_w, &taps);
    std::vector<double> zpow((size_t)(H > W ? H : W));
    visual_zpow((int)zpow.size(), zpow.data());
    const VisAxis ax_h = visual_axis_constants(H), ax_w = visual_axis_constants(W);
    HIP_TRY(hipSetDevice(device));
    const size_t n = (size_t)H * W, n_out = (size_t)out_h * out_w;
    ArenaLayout lay;
    const size_t o_ctl = lay.add(sizeof(VisCtl)), o_taps = lay.add(taps.size() * sizeof(VisTap)), o_pow = lay.add(zpow.size() * sizeof(double));
    const size_t o_src = lay.add(n * sample_size(dtype)), o_res = lay.add(n_out * sizeof(int)), o_grey = lay.add(n_out);
    const size_t o_coef = lay.add(cubic ? n * sizeof(double) : 0);
    DevMem d;
    HIP_TRY(d.alloc(lay.total()));
    VisCtl ctl = {0, 0x7FFFFFFF, (int)0x80000000, 0};
    VisCtl* const d_ctl = d.as<VisCtl>(o_ctl);
    HIP_TRY(hipMemcpy(d_ctl, &ctl, sizeof(ctl), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d.as<char>(o_taps), taps.data(), taps.size() * sizeof(VisTap), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d.as<char>(o_pow), zpow.data(), zpow.size() * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d.as<char>(o_src), plane, n * sample_size(dtype), hipMemcpyHostToDevice));
    const void* d_src = d.as<const char>(o_src);
    const VisTap* d_taps = d.as<const VisTap>(o_taps);
    const double* d_zpow = d.as<const double>(o_pow);
    double* d_coef = d.as<double>(o_coef);
    int* d_res = d.as<int>(o_res);
    by_sample_type(dtype, [&](auto t) {
        launch_grey_resample<decltype(t)::dtype>(cubic, d_src, H, W, out_h, out_w, ax_h, ax_w, d_zpow, d_coef, d_taps, d_res, d_ctl);
    });
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(&ctl, d_ctl, sizeof(ctl), hipMemcpyDeviceToHost));      // (waits for the launches: the default stream orders them)
    if (ctl.status) { *status = ctl.status; return TS2D_OK; }                   // a non-finite sample: nothing is written, the caller takes the host route
    const bool is_float = dtype == 2;
    const double w_lo = auto_lo ? (is_float ? (double)visual_unkey(ctl.min_key) : (double)ctl.min_key) : lo;
    const double w_hi = auto_hi ? (is_float ? (double)visual_unkey(ctl.max_key) : (double)ctl.max_key) : hi;
    window_used[0] = w_lo; window_used[1] = w_hi;
    if (w_hi == w_lo) { std::memset(grey, 0, n_out); return TS2D_OK; }          // our definition: an all-zero plane
    const VisWindow win = visual_window(w_lo, w_hi);
    hipLaunchKernelGGL(visual_window, dim3((unsigned)((n_out + 1023) / 1024)), dim3(256), 0, 0, d_res, (long long)n_out, is_float ? 1 : 0, win,
                       d.as<uint8_t>(o_grey));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(grey, d.as<char>(o_grey), n_out, hipMemcpyDeviceToHost));
    return TS2D_OK;
}
