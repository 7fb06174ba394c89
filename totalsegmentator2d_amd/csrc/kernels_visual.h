// Device side of the PNG visuals (visual.py is the statement, visual.hip the two entries, visual_plan.cpp the host tables).
//
// Labels (ts2d_visual_labels):
//     visual_flatten        K uint8 planes [K][n] -> uint8 index map [n]: 1 + the index of the LAST non-zero plane, 0 when all are zero
//     visual_label_rgb      nearest gather through the two axis tables, colour from a 256-entry table in LDS, RGB bytes
// Flatten runs BEFORE the resample, so the K planes are read once whatever the upsampling ratio.
//
// Grey (ts2d_visual_grey):
//     visual_prefilter_cols  source type -> float64, gain, cubic B-spline prefilter with the mirror initialisation along axis 0
//     visual_prefilter_rows  the same filter along axis 1, in place
//     visual_interp_cast     16 float64 taps per output pixel, cast back to the source type, min / max of the result
//     visual_gather_nearest  (uint8, or no resample at all) nearest gather, min / max of the result
//     visual_window          IntensityWindowing to 0 ... 255 and the cast to uint8
// The resampled plane is kept as one 32-bit word per pixel: the value of an integer type, or the bits of a float32.  Its min / max are taken
// on order-preserving int32 keys (the value; for a float32 the bits with the magnitude of negatives inverted) with a wave reduction and one
// integer atomic per wave, so they do not depend on the order of arrival.
//
// The line filter is visual.spline_prefilter_axis0 in the shape of rsin_filter_line (kernels_resample_in.h): one lane per line, the loads of
// 16 samples issued together ahead of the 16 dependent chain steps, every float64 product and sum through rs_mul / rs_add (rs_arith.h) so that
// nothing fuses.  With n the length of the line and g[i] = sample[i] * gain:
//     acc    = g[0] + z^(n-1) * g[n-1];  for i = 1 ... n-2:  acc += zpow[i] * (g[i] + z^(n-1) * g[n-1-i])
//     c[0]   = acc * k0                                        k0 = 1 / (1 - z^(n-1) * z^(n-1))
//     c[i]   = g[i] + z * c[i-1]                               i = 1 ... n-1
//     c[n-1] = (z * c[n-2] + c[n-1]) * k1                      k1 = z / (z*z - 1)
//     c[i]   = z * (c[i+1] - c[i])                             i = n-2 ... 0
// floor, pow and every division are the host's (VisAxis, VisTap, VisWindow, the colour table): the kernels hold none.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "rs_arith.h"           // rs_mul, rs_add
#include "visual_plan.h"        // VisTap, VisAxis, VisWindow

namespace ts2d {

constexpr int kVisBatch = 16;           // samples of a line whose loads are in flight together
constexpr int kVisStatusNonfinite = 1;  // TS2D_VISUAL_NONFINITE
constexpr int kVisFlattenUnroll = 4;    // planes whose loads are in flight together

struct VisCtl { int status, min_key, max_key, pad_; };      // zeroed / seeded by the entry before the first launch

// ------------------------------------------------------------------------------------------------ labels
// high bit of every byte of v that is not zero
__device__ __forceinline__ uint32_t vis_nonzero_bytes(uint32_t v) {
    return (((v & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | v) & 0x80808080u;
}

// 16 consecutive bytes at p as four words; `vec`: p is 16-byte aligned and all 16 are inside; else the first `valid` bytes, one by one
__device__ __forceinline__ uint4 vis_load16(const uint8_t* __restrict__ p, bool vec, int valid) {
    if (vec) return *reinterpret_cast<const uint4*>(p);
    uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int j = 0; j < 16; ++j)
        if (j < valid) w[j >> 2] |= (uint32_t)p[j] << ((j & 3) * 8);
    return make_uint4(w[0], w[1], w[2], w[3]);
}

// bytes of idx where v is non-zero become `label` (a byte broadcast to the four positions)
__device__ __forceinline__ void vis_take(uint4& idx, const uint4 v, uint32_t label) {
    uint32_t m;
    m = (vis_nonzero_bytes(v.x) >> 7) * 0xFFu; idx.x = (idx.x & ~m) | (label & m);
    m = (vis_nonzero_bytes(v.y) >> 7) * 0xFFu; idx.y = (idx.y & ~m) | (label & m);
    m = (vis_nonzero_bytes(v.z) >> 7) * 0xFFu; idx.z = (idx.z & ~m) | (label & m);
    m = (vis_nonzero_bytes(v.w) >> 7) * 0xFFu; idx.w = (idx.w & ~m) | (label & m);
}

// One lane per 16 consecutive pixels of the planes seen as [K][n], plane k at planes + k * stride (the entry uploads them at a stride that is
// a multiple of 16, so every plane of its buffer is aligned).  The loop over the planes is wave-uniform and has no early exit: the planes
// are visited in index order and a later non-zero plane overwrites an earlier one.  A plane whose base is 16-byte aligned is read with one
// 16-byte load per lane (the lane's offset is a multiple of 16), any other plane and the tail of every plane byte by byte.
__global__ __launch_bounds__(256) void visual_flatten(const uint8_t* __restrict__ planes, int K, long long n, long long stride,
                                                      uint8_t* __restrict__ index_map) {
    const long long p0 = ((long long)blockIdx.x * 256 + threadIdx.x) * 16;
    if (p0 >= n) return;
    const int valid = n - p0 < 16 ? (int)(n - p0) : 16;
    const bool full = valid == 16;
    uint4 idx = make_uint4(0u, 0u, 0u, 0u);
    int k = 0;
    for (; k + kVisFlattenUnroll <= K; k += kVisFlattenUnroll) {
        uint4 v[kVisFlattenUnroll];
#pragma unroll
        for (int u = 0; u < kVisFlattenUnroll; ++u) {
            const uint8_t* base = planes + (size_t)(k + u) * (size_t)stride;
            v[u] = vis_load16(base + p0, full && ((uintptr_t)base & 15) == 0, valid);
        }
#pragma unroll
        for (int u = 0; u < kVisFlattenUnroll; ++u) vis_take(idx, v[u], (uint32_t)(k + u + 1) * 0x01010101u);
    }
    for (; k < K; ++k) {
        const uint8_t* base = planes + (size_t)k * (size_t)stride;
        vis_take(idx, vis_load16(base + p0, full && ((uintptr_t)base & 15) == 0, valid), (uint32_t)(k + 1) * 0x01010101u);
    }
    if (full && ((uintptr_t)index_map & 15) == 0) {
        *reinterpret_cast<uint4*>(index_map + p0) = idx;
    } else {
        const uint32_t w[4] = {idx.x, idx.y, idx.z, idx.w};
#pragma unroll
        for (int j = 0; j < 16; ++j)
            if (j < valid) index_map[p0 + j] = (uint8_t)(w[j >> 2] >> ((j & 3) * 8));
    }
}

// One lane per 4 consecutive output X of output row blockIdx.y.  index_map [H][W]; rows at taps[0, out_h), columns at taps[out_h, out_h + out_w);
// lut[256]: the colour of every label value, r | g << 8 | b << 16, staged in LDS; rgb [out_h][out_w][3].  An outside pixel is label 0: black.
__global__ __launch_bounds__(64) void visual_label_rgb(const uint8_t* __restrict__ index_map, int W, int out_h, int out_w,
                                                       const VisTap* __restrict__ taps, const uint32_t* __restrict__ lut, uint8_t* __restrict__ rgb) {
    __shared__ uint32_t s_lut[256];
#pragma unroll
    for (int j = 0; j < 4; ++j) s_lut[threadIdx.x + 64 * j] = lut[threadIdx.x + 64 * j];
    __syncthreads();
    const int Y = blockIdx.y;
    const int X0 = (blockIdx.x * 64 + threadIdx.x) * 4;
    if (X0 >= out_w) return;
    const int ny = taps[Y].nearest;
    const uint8_t* row = index_map + (size_t)(ny < 0 ? 0 : ny) * W;
    uint32_t c[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (X0 + j >= out_w) continue;
        const int nx = taps[out_h + X0 + j].nearest;
        const uint32_t v = (ny < 0 || nx < 0) ? 0u : (uint32_t)row[nx];
        c[j] = s_lut[v];
    }
    uint8_t* o = rgb + ((size_t)Y * out_w + X0) * 3;
    if ((out_w & 3) == 0) {             // 12 bytes at a multiple of 12 from a row start that is a multiple of 4: three aligned words
        uint32_t* o32 = reinterpret_cast<uint32_t*>(o);
        o32[0] = c[0] | (c[1] << 24);
        o32[1] = (c[1] >> 8) | (c[2] << 16);
        o32[2] = (c[2] >> 16) | (c[3] << 8);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (X0 + j >= out_w) continue;
            o[3 * j] = (uint8_t)c[j]; o[3 * j + 1] = (uint8_t)(c[j] >> 8); o[3 * j + 2] = (uint8_t)(c[j] >> 16);
        }
    }
}

// ------------------------------------------------------------------------------------------------ grey: source types and keys
// dtype codes of the C-ABI (those of ts2d_project_coronal): 0 int16, 1 uint8, 2 float32, 3 uint16, 4 int32
template <int DT> struct VisType;
template <> struct VisType<0> { using T = int16_t;  static constexpr bool is_float = false; static constexpr double lo = -32768.0, hi = 32767.0; };
template <> struct VisType<1> { using T = uint8_t;  static constexpr bool is_float = false; static constexpr double lo = 0.0, hi = 255.0; };
template <> struct VisType<2> { using T = float;    static constexpr bool is_float = true;  static constexpr double lo = 0.0, hi = 0.0; };
template <> struct VisType<3> { using T = uint16_t; static constexpr bool is_float = false; static constexpr double lo = 0.0, hi = 65535.0; };
template <> struct VisType<4> { using T = int32_t;  static constexpr bool is_float = false; static constexpr double lo = -2147483648.0, hi = 2147483647.0; };

__device__ __forceinline__ int vis_float_key(int bits) { return bits < 0 ? bits ^ 0x7FFFFFFF : bits; }
__device__ __forceinline__ bool vis_nonfinite(int bits) { return (bits & 0x7F800000) == 0x7F800000; }

// min / max of the keys of a wave's lanes (a lane without a pixel brings INT_MAX / INT_MIN), one atomic each from lane 0.  Every lane of the
// wave must arrive here.
__device__ __forceinline__ void vis_wave_minmax(int kmin, int kmax, VisCtl* __restrict__ ctl) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const int a = __shfl_xor(kmin, off, 64), b = __shfl_xor(kmax, off, 64);
        kmin = a < kmin ? a : kmin;
        kmax = b > kmax ? b : kmax;
    }
    if ((threadIdx.x & 63) == 0) {
        if (kmin != 0x7FFFFFFF) atomicMin(&ctl->min_key, kmin);
        if (kmax != (int)0x80000000) atomicMax(&ctl->max_key, kmax);
    }
}

// ------------------------------------------------------------------------------------------------ grey: the prefilter
template <class L>
__device__ __forceinline__ void visual_filter_line(const L& ln, int n, const VisAxis& ax, const double* __restrict__ zpow) {
    double acc = rs_add(ln.g(0), rs_mul(ax.zn1, ln.g(n - 1)));
    int i = 1;
    for (; i + kVisBatch <= n - 1; i += kVisBatch) {            // terms 1 ... n-2 of the boundary sum
        double a[kVisBatch], b[kVisBatch], zp[kVisBatch];
#pragma unroll
        for (int k = 0; k < kVisBatch; ++k) { a[k] = ln.g(i + k); b[k] = ln.g(n - 1 - i - k); zp[k] = zpow[i + k]; }
#pragma unroll
        for (int k = 0; k < kVisBatch; ++k) acc = rs_add(acc, rs_mul(zp[k], rs_add(a[k], rs_mul(ax.zn1, b[k]))));
    }
    for (; i < n - 1; ++i) acc = rs_add(acc, rs_mul(zpow[i], rs_add(ln.g(i), rs_mul(ax.zn1, ln.g(n - 1 - i)))));
    double prev = rs_mul(acc, ax.k0), before = prev;
    ln.c(0) = prev;
    for (i = 1; i + kVisBatch <= n; i += kVisBatch) {           // causal
        double a[kVisBatch];
#pragma unroll
        for (int k = 0; k < kVisBatch; ++k) a[k] = ln.g(i + k);
#pragma unroll
        for (int k = 0; k < kVisBatch; ++k) { before = prev; prev = rs_add(a[k], rs_mul(ax.z, prev)); ln.c(i + k) = prev; }
    }
    for (; i < n; ++i) { before = prev; prev = rs_add(ln.g(i), rs_mul(ax.z, prev)); ln.c(i) = prev; }
    prev = rs_mul(rs_add(rs_mul(ax.z, before), prev), ax.k1);   // `before` = c[n-2], `prev` = c[n-1] of the causal pass
    ln.c(n - 1) = prev;
    for (i = n - 2; i - kVisBatch + 1 >= 0; i -= kVisBatch) {   // anticausal
        double a[kVisBatch];
#pragma unroll
        for (int k = 0; k < kVisBatch; ++k) a[k] = ln.c(i - k);
#pragma unroll
        for (int k = 0; k < kVisBatch; ++k) { prev = rs_mul(ax.z, rs_add(prev, -a[k])); ln.c(i - k) = prev; }
    }
    for (; i >= 0; --i) { prev = rs_mul(ax.z, rs_add(prev, -ln.c(i))); ln.c(i) = prev; }
}

template <class T> struct VisColumn {       // column x of the source plane; coefficients to the float64 plane
    const T* s; double* cf; int W; double gain;
    __device__ __forceinline__ double g(int i) const { return rs_mul((double)s[(size_t)i * W], gain); }
    __device__ __forceinline__ double& c(int i) const { return cf[(size_t)i * W]; }
};

struct VisRow {                             // row of the coefficient plane, filtered in place
    double* cf; double gain;
    __device__ __forceinline__ double g(int i) const { return rs_mul(cf[i], gain); }
    __device__ __forceinline__ double& c(int i) const { return cf[i]; }
};

// One lane per column x.  src [H][W] of type DT; coef [H][W] float64 (written); zpow[i], i < H.  A float32 column with a non-finite sample
// sets the status bit (its coefficients are then of no use: the entry returns before it reads them).
template <int DT>
__global__ __launch_bounds__(64) void visual_prefilter_cols(const void* __restrict__ src, int H, int W, VisAxis ax, const double* __restrict__ zpow,
                                                            double* __restrict__ coef, VisCtl* __restrict__ ctl) {
    using T = typename VisType<DT>::T;
    const int x = blockIdx.x * 64 + threadIdx.x;
    if (x >= W) return;
    const T* s = static_cast<const T*>(src) + x;
    if (VisType<DT>::is_float) {
        int bad = 0;
        for (int i = 0; i < H; ++i) bad |= vis_nonfinite(__float_as_int((float)s[(size_t)i * W])) ? 1 : 0;
        if (bad) { atomicOr(&ctl->status, kVisStatusNonfinite); return; }
    }
    const VisColumn<T> ln = {s, coef + x, W, ax.gain};
    visual_filter_line(ln, H, ax, zpow);
}

// One lane per row, in place on coef [H][W]; zpow[i], i < W.
__global__ __launch_bounds__(64) void visual_prefilter_rows(double* __restrict__ coef, int H, int W, VisAxis ax, const double* __restrict__ zpow) {
    const int y = blockIdx.x * 64 + threadIdx.x;
    if (y >= H) return;
    const VisRow ln = {coef + (size_t)y * W, ax.gain};
    visual_filter_line(ln, W, ax, zpow);
}

// ------------------------------------------------------------------------------------------------ grey: resample, window
// float64 -> the word of the resampled plane (visual.cast_to_pixel_type): a float32 takes one rounding, an integer type is clamped to its range
// and truncated toward zero
template <int DT> __device__ __forceinline__ int vis_cast_word(double s) {
    if (VisType<DT>::is_float) return __float_as_int(__double2float_rn(s));
    s = s < VisType<DT>::lo ? VisType<DT>::lo : s;
    s = s > VisType<DT>::hi ? VisType<DT>::hi : s;
    return (int)s;
}

// One lane per output pixel (row blockIdx.y): 16 taps - row tap outer, column tap inner - each (c * wy) * wx, summed in that order from 0.
// res [out_h][out_w]: the words of the resampled plane; an outside pixel is 0.
template <int DT>
__global__ __launch_bounds__(64) void visual_interp_cast(const double* __restrict__ coef, int W, int out_h, int out_w, const VisTap* __restrict__ taps,
                                                         int* __restrict__ res, VisCtl* __restrict__ ctl) {
    const int Y = blockIdx.y, X = blockIdx.x * 64 + threadIdx.x;
    int kmin = 0x7FFFFFFF, kmax = (int)0x80000000;
    if (X < out_w) {
        const VisTap ty = taps[Y], tx = taps[out_h + X];
        int word = 0;
        if (ty.inside && tx.inside) {
            double s = 0.0;
#pragma unroll
            for (int a = 0; a < 4; ++a) {
                const double* row = coef + (size_t)ty.idx[a] * W;
#pragma unroll
                for (int b = 0; b < 4; ++b) s = rs_add(s, rs_mul(rs_mul(row[tx.idx[b]], ty.w[a]), tx.w[b]));
            }
            word = vis_cast_word<DT>(s);
        }
        res[(size_t)Y * out_w + X] = word;
        kmin = kmax = VisType<DT>::is_float ? vis_float_key(word) : word;
    }
    vis_wave_minmax(kmin, kmax, ctl);
}

// One lane per output pixel (row blockIdx.y): the nearest sample, 0 outside.  A non-finite float32 sample sets the status bit.
template <int DT>
__global__ __launch_bounds__(64) void visual_gather_nearest(const void* __restrict__ src, int W, int out_h, int out_w, const VisTap* __restrict__ taps,
                                                            int* __restrict__ res, VisCtl* __restrict__ ctl) {
    using T = typename VisType<DT>::T;
    const int Y = blockIdx.y, X = blockIdx.x * 64 + threadIdx.x;
    int kmin = 0x7FFFFFFF, kmax = (int)0x80000000;
    if (X < out_w) {
        const int ny = taps[Y].nearest, nx = taps[out_h + X].nearest;
        int word = 0;
        if (ny >= 0 && nx >= 0) {
            const T v = static_cast<const T*>(src)[(size_t)ny * W + nx];
            word = VisType<DT>::is_float ? __float_as_int((float)v) : (int)v;
            if (VisType<DT>::is_float && vis_nonfinite(word)) atomicOr(&ctl->status, kVisStatusNonfinite);
        }
        res[(size_t)Y * out_w + X] = word;
        kmin = kmax = VisType<DT>::is_float ? vis_float_key(word) : word;
    }
    vis_wave_minmax(kmin, kmax, ctl);
}

// visual.window_u8 of one word: below lo 0, above hi 255, else x * scale + shift (rounded on their own), one rounding to the pixel type (an
// integer type truncates, as the final cast does), then truncation to uint8 kept inside 0 ... 255
__device__ __forceinline__ uint32_t vis_window_one(int word, bool is_float, const VisWindow& w) {
    const double x = is_float ? (double)__int_as_float(word) : (double)word;
    double v = rs_add(rs_mul(x, w.scale), w.shift);
    v = x > w.hi ? 255.0 : v;
    v = x < w.lo ? 0.0 : v;
    if (is_float) v = (double)__double2float_rn(v);
    int u = (int)v;
    u = u < 0 ? 0 : (u > 255 ? 255 : u);
    return (uint32_t)u;
}

// One lane per 4 consecutive pixels of the flat resampled plane res [n] -> grey [n] uint8.
__global__ __launch_bounds__(256) void visual_window(const int* __restrict__ res, long long n, int is_float, VisWindow w, uint8_t* __restrict__ grey) {
    const long long p0 = ((long long)blockIdx.x * 256 + threadIdx.x) * 4;
    if (p0 >= n) return;
    if (p0 + 4 <= n) {
        const int4 r = *reinterpret_cast<const int4*>(res + p0);
        const uint32_t o = vis_window_one(r.x, is_float, w) | (vis_window_one(r.y, is_float, w) << 8) | (vis_window_one(r.z, is_float, w) << 16) |
                           (vis_window_one(r.w, is_float, w) << 24);
        *reinterpret_cast<uint32_t*>(grey + p0) = o;
    } else {
        for (long long p = p0; p < n; ++p) grey[p] = (uint8_t)vis_window_one(res[p], is_float, w);
    }
}

}  // namespace ts2d
