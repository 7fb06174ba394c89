// Device side of the INPUT resample: a case whose spacing is not the plan's has every (channel, slice) plane resampled
// to the plan spacing with skimage's resize(order=3, mode='edge', anti_aliasing=False, clip=True), which is scipy's
// zoom(order=3, mode='nearest', grid_mode=True) followed by a clip to the plane's value range.  Three kernels, each ONE launch for all
// planes of a call (ts2d_resample_cubic, prep.hip):
//     rsin_prefilter_cols   pad by 12 edge samples, widen to float64, gain, cubic B-spline prefilter along axis 0
//     rsin_prefilter_rows   the same filter along axis 1, in place
//     rsin_interp_clip      16 taps per output pixel, one rounding to float32, clip to the plane's [lo, hi]
//
// Arithmetic = preprocess.resize_cubic_f64, bit for bit, which is bit for bit scipy (tests/test_resample_cubic_cpu.py).  The line filter,
// one rounding per product / sum (scipy's apply_filter with the initialisation of modes 'nearest' / 'reflect'), n = padded length:
//     g[i]   = sample[i] * gain
//     acc    = g[0] + z^n * g[n-1];  for i = 1 ... n-1:  acc += zpow[i] * (g[i] + z^n * (i == n-1 ? acc : g[n-1-i]))
//     c[0]   = acc * k0 + g[0]                              k0 = z / (1 - z^n * z^n)
//     c[i]   = g[i] + z * c[i-1]                            i = 1 ... n-1
//     c[n-1] = c[n-1] * k1                                  k1 = z / (z - 1)
//     c[i]   = z * (c[i+1] - c[i])                          i = n-2 ... 0
// (scipy accumulates the boundary sum IN c[0], so its last term reads the accumulator: that is the `i == n-1` case.)  The recursion is
// sequential along a line by nature and is left so: a scan or a truncated sum would change the bits.  Everything that does not depend on
// the line - z, gain, z^n, the running products zpow[i] = z * z * ... (NOT pow(z, i)), k0, k1 - is computed once on the host in float64
// and passed in (RsInAxis), so no pow and no division runs on the device; the interpolation taps (start index, four weights per output
// row / column) come from the host as well (prep_plan.cpp: rsin_axis_taps), so the kernels hold no floor either.  Every float64 product and
// sum is written with rs_mul / rs_add (rs_arith.h: `#pragma clang fp contract(off)`); tests/test_resample_cubic_cpu.py asserts that
// the emitted stream holds v_mul_f64 / v_add_f64 and no fused form, no scratch and no spills.  float64 denormals are kept (the powers
// zpow[i] pass through them on their way to 0 on lines longer than about 560 samples), as on the host.
//
// Shape of the work.  A plane pair of a case is a few MB of float64 coefficients and stays in L2.  The filter is latency-bound: the chain
// of one line is a dependent multiply-add per sample, so the loads of 16 samples are issued together ahead of the 16 chain steps
// (kRsInBatch).  Column pass: one lane per column of the padded plane, neighbouring lanes read neighbouring x: every step is a coalesced
// row read and write.  Row pass: one lane per row; a lane's 16 samples of a batch are 128 consecutive bytes, so a wave reads and writes
// whole cache lines, one per lane, and no line is fetched twice.  64-lane workgroups spread the few dozen waves of a call over the CUs.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "device_tables.h"      // kRsInPad, RsInAxis, RsInTap
#include "rs_arith.h"           // rs_mul, rs_add

namespace ts2d {

constexpr int kRsInBatch = 16;      // samples of a line whose loads are in flight together

// The line filter of one lane.  `L` gives the line: L.g(i) = sample i times the gain, L.c(i) = reference to coefficient i.  Whole batches
// first (their loads carry constant offsets and are issued together), then the remainder sample by sample.
template <class L>
__device__ __forceinline__ void rsin_filter_line(const L& ln, int n, const RsInAxis& ax, const double* __restrict__ zpow) {
    const double g0 = ln.g(0);
    double acc = rs_add(g0, rs_mul(ax.zn, ln.g(n - 1)));
    int i = 1;
    for (; i + kRsInBatch <= n - 1; i += kRsInBatch) {          // terms 1 ... n-2 of the boundary sum
        double a[kRsInBatch], b[kRsInBatch], zp[kRsInBatch];
#pragma unroll
        for (int k = 0; k < kRsInBatch; ++k) { a[k] = ln.g(i + k); b[k] = ln.g(n - 1 - i - k); zp[k] = zpow[i + k]; }
#pragma unroll
        for (int k = 0; k < kRsInBatch; ++k) acc = rs_add(acc, rs_mul(zp[k], rs_add(a[k], rs_mul(ax.zn, b[k]))));
    }
    for (; i < n - 1; ++i) acc = rs_add(acc, rs_mul(zpow[i], rs_add(ln.g(i), rs_mul(ax.zn, ln.g(n - 1 - i)))));
    acc = rs_add(acc, rs_mul(zpow[n - 1], rs_add(ln.g(n - 1), rs_mul(ax.zn, acc))));      // term n-1 reads the accumulator
    double prev = rs_add(rs_mul(acc, ax.k0), g0);
    ln.c(0) = prev;
    for (i = 1; i + kRsInBatch <= n; i += kRsInBatch) {         // causal
        double a[kRsInBatch];
#pragma unroll
        for (int k = 0; k < kRsInBatch; ++k) a[k] = ln.g(i + k);
#pragma unroll
        for (int k = 0; k < kRsInBatch; ++k) { prev = rs_add(a[k], rs_mul(ax.z, prev)); ln.c(i + k) = prev; }
    }
    for (; i < n; ++i) { prev = rs_add(ln.g(i), rs_mul(ax.z, prev)); ln.c(i) = prev; }
    prev = rs_mul(prev, ax.k1);
    ln.c(n - 1) = prev;
    for (i = n - 2; i - kRsInBatch + 1 >= 0; i -= kRsInBatch) { // anticausal
        double a[kRsInBatch];
#pragma unroll
        for (int k = 0; k < kRsInBatch; ++k) a[k] = ln.c(i - k);
#pragma unroll
        for (int k = 0; k < kRsInBatch; ++k) { prev = rs_mul(ax.z, rs_add(prev, -a[k])); ln.c(i - k) = prev; }
    }
    for (; i >= 0; --i) { prev = rs_mul(ax.z, rs_add(prev, -ln.c(i))); ln.c(i) = prev; }
}

struct RsInColumn {         // column x of a padded plane: samples from the float32 source (edge samples repeat: row index clamped)
    const float* s; double* cf; int H, W, Wp; double gain;
    __device__ __forceinline__ double g(int i) const {
        int r = i - kRsInPad; r = r < 0 ? 0 : (r > H - 1 ? H - 1 : r);
        return rs_mul((double)s[(size_t)r * W], gain);
    }
    __device__ __forceinline__ double& c(int i) const { return cf[(size_t)i * Wp]; }
};

struct RsInRow {            // row of a padded plane of coefficients, filtered in place
    double* cf; double gain;
    __device__ __forceinline__ double g(int i) const { return rs_mul(cf[i], gain); }
    __device__ __forceinline__ double& c(int i) const { return cf[i]; }
};

// One lane per column x of one padded plane.  src [planes, H, W] float32; coef [planes, H + 24, W + 24] float64 (written);
// zpow[i], i < H + 24: the running products of the pole.
__global__ __launch_bounds__(64) void rsin_prefilter_cols(const float* __restrict__ src, int n_planes, int H, int W, RsInAxis ax,
                                                          const double* __restrict__ zpow, double* __restrict__ coef) {
    const int Hp = H + 2 * kRsInPad, Wp = W + 2 * kRsInPad;
    const long long t = (long long)blockIdx.x * 64 + threadIdx.x;
    if (t >= (long long)n_planes * Wp) return;
    const int x = (int)(t % Wp), p = (int)(t / Wp);
    int sx = x - kRsInPad; sx = sx < 0 ? 0 : (sx > W - 1 ? W - 1 : sx);
    const RsInColumn ln = {src + (size_t)p * H * W + sx, coef + (size_t)p * Hp * Wp + x, H, W, Wp, ax.gain};
    rsin_filter_line(ln, Hp, ax, zpow);
}

// One lane per row of one padded plane, in place on coef [planes, Hp, Wp]; zpow[i], i < Wp.
__global__ __launch_bounds__(64) void rsin_prefilter_rows(double* __restrict__ coef, int n_planes, int Hp, int Wp, RsInAxis ax,
                                                          const double* __restrict__ zpow) {
    const long long t = (long long)blockIdx.x * 64 + threadIdx.x;
    if (t >= (long long)n_planes * Hp) return;
    const RsInRow ln = {coef + (size_t)t * Wp, ax.gain};
    rsin_filter_line(ln, Wp, ax, zpow);
}

// One lane per 4 consecutive output X of one (plane, Y) row.  taps: rows at [0, out_h), columns at [out_h, out_h + out_w);
// lo_hi [planes][2]: the clip bounds of each plane (its float32 min and max).  dst [planes, out_h, out_w] float32.
__global__ __launch_bounds__(256) void rsin_interp_clip(const double* __restrict__ coef, int n_planes, int Hp, int Wp, int out_h, int out_w,
                                                        const RsInTap* __restrict__ taps, const float* __restrict__ lo_hi,
                                                        float* __restrict__ dst) {
    const int Wq = (out_w + 3) >> 2;
    const long long q = (long long)blockIdx.x * 256 + threadIdx.x;
    if (q >= (long long)n_planes * out_h * Wq) return;
    const int X0 = (int)(q % Wq) * 4; const long long r = q / Wq;
    const int Y = (int)(r % out_h), p = (int)(r / out_h);
    const RsInTap ty = taps[Y];
    const double* c0 = coef + ((size_t)p * Hp + ty.start) * Wp;
    const float lo = lo_hi[2 * p], hi = lo_hi[2 * p + 1];
    const int nx = out_w - X0 < 4 ? out_w - X0 : 4;             // (the last quad of a row whose extent is no multiple of 4)
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    for (int j = 0; j < 4; ++j) {                               // (constant trip count: v[] stays in registers)
        if (j >= nx) continue;
        const RsInTap tx = taps[out_h + X0 + j];
        double s = 0.0;
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            const double* row = c0 + (size_t)a * Wp + tx.start;
#pragma unroll
            for (int b = 0; b < 4; ++b) s = rs_add(s, rs_mul(rs_mul(row[b], ty.w[a]), tx.w[b]));
        }
        float f = __double2float_rn(s);
        f = f < lo ? lo : f;                                    // numpy's clip: a value equal to a bound keeps its own sign of zero
        f = f > hi ? hi : f;
        v[j] = f;
    }
    const size_t o = ((size_t)p * out_h + Y) * out_w + X0;
    if ((out_w & 3) == 0) {
        *reinterpret_cast<float4*>(dst + o) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
        for (int j = 0; j < 4; ++j) if (j < nx) dst[o + j] = v[j];
    }
}

}  // namespace ts2d
