// The synthetic radiograph of a CT volume and the matching perspective projection of a label volume, behind ts2d_project_xr and
// ts2d_project_labels_xr.  The statements are totalsegmentator2d_amd.xray.synthetic_xr_statement and project_labels_xr_statement;
// tests/test_gpu_xray.py holds these kernels against them bit for bit and byte for byte.
//
//   xr_scan                 one pass over the view before the rays: a float volume is searched for a NaN or an infinity, a label volume for a
//                           sample outside 0 ... num.  EVERY sample of the view is looked at, also one no ray meets, because the statements refuse
//                           the volume and not the rays.  One lane per (z, x) column walks y, as project_coronal does: the loads of a wave are
//                           adjacent in x.  A lane that found one sets the status word with one integer atomic OR.
//   project_xr_rays         one lane per detector pixel, the 64 lanes of a wave adjacent in u.  The lane walks the planes y = j in index order and
//                           adds one bilinear sample of the plane's density per plane, in float64 with the statement's roundings (rs_mul / rs_add:
//                           no fused multiply-add).  Sample j lies at x = cx[i] + t[j] * a[i], z = cz[k] + t[j] * b[k] (the tables are the host's:
//                           prep_plan.cpp, xr_plan); the four loads of a step are the corners (z0, x0) ... (z0 + 1, x0 + 1), each adjacent across the
//                           lanes.  A corner outside the plane is +0.0 and is not loaded; a sample outside (-1, nx) x (-1, nz) adds nothing.
//                           The kernel only sums: the step length and the cast to float32 are the host's (xr_finish).
//   project_labels_xr_rays  the same rays with the nearest voxel floor(x + 0.5), floor(z + 0.5); a sample outside the volume is skipped.  A lane
//                           keeps a num-bit set in NW = ceil(num / 32) registers (the word is chosen by a static loop over the words: no
//                           dynamically indexed private array, as project_labels_stream) and stores bit k of it to plane k.
// No inter-lane communication, no flags, nothing waits; the one atomic is xr_scan's integer OR; plain vector stores.  Every index into the volume
// is checked against the view's extents before the load, and every loop bound is a kernel argument.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "rs_arith.h"

namespace ts2d {

constexpr int kXrThreads = 256;
constexpr int kXrStatusNonFinite = 1;      // TS2D_XR_NONFINITE
constexpr int kXrStatusRange = 1;          // TS2D_LABELS_RANGE

struct XrView {             // the reoriented strided view of the volume, in elements
    int nz, ny, nx;
    long long sz, sy, sx, base;
};
struct XrDensity {          // density = max((sample - air) * scale, 0), then min(., dmax) where clip
    double air, scale, dmax;
    int clip;
};
struct XrTables {           // device pointers: t [ny]; a, cx [nu]; b, cz [nv]
    const double *t, *a, *cx, *b, *cz;
    int nu, nv;
};

// grid = ceil(nz * nx / kXrThreads).  num < 0: a float volume, searched for a non-finite sample; else the range 0 ... num of a label volume.
template <typename T>
__global__ __launch_bounds__(kXrThreads) void xr_scan(const T* __restrict__ vol, XrView v, int num, int* __restrict__ status) {
    const long long i = (long long)blockIdx.x * kXrThreads + threadIdx.x;
    if (i >= (long long)v.nz * v.nx) return;
    const long long z = i / v.nx, x = i - z * v.nx;
    const T* p = vol + v.base + z * v.sz + x * v.sx;
    bool bad = false;
    for (int y = 0; y < v.ny; ++y) {
        const T s = p[(long long)y * v.sy];
        if constexpr (!std::is_integral<T>::value) {
            bad |= (__float_as_uint(s) & 0x7F800000u) == 0x7F800000u;
        } else {
            const long long w = (long long)s;
            bad |= w < 0 || w > num;
        }
    }
    if (bad) atomicOr(status, 1);
}

template <typename T>
__device__ __forceinline__ double xr_density(T s, const XrDensity& dn) {
    const double x = rs_mul(rs_add((double)s, -dn.air), dn.scale);
    double d = x > 0.0 ? x : 0.0;
    if (dn.clip) d = d > dn.dmax ? dn.dmax : d;
    return d;
}

// grid = ceil(nu * nv / kXrThreads).  out: float64 [nv][nu], the sums of the rays.
template <typename T>
__global__ __launch_bounds__(kXrThreads) void project_xr_rays(const T* __restrict__ vol, XrView v, XrDensity dn, XrTables tb, double* __restrict__ out) {
    const long long pix = (long long)blockIdx.x * kXrThreads + threadIdx.x;
    if (pix >= (long long)tb.nu * tb.nv) return;
    const int k = (int)(pix / tb.nu), i = (int)(pix - (long long)k * tb.nu);
    const double ai = tb.a[i], cxi = tb.cx[i], bk = tb.b[k], czk = tb.cz[k];
    const double xmax = (double)v.nx, zmax = (double)v.nz;
    double acc = 0.0;
    for (int j = 0; j < v.ny; ++j) {
        const double tj = tb.t[j];
        const double x = rs_add(cxi, rs_mul(tj, ai)), z = rs_add(czk, rs_mul(tj, bk));
        if (!(x > -1.0 && x < xmax && z > -1.0 && z < zmax)) continue;          // (a NaN is outside as well)
        const double xf = floor(x), zf = floor(z);
        const double fx = rs_add(x, -xf), fz = rs_add(z, -zf);
        const int x0 = (int)xf, z0 = (int)zf;                                   // -1 ... nx - 1, -1 ... nz - 1
        const bool xa = x0 >= 0, xb = x0 + 1 < v.nx, za = z0 >= 0, zb = z0 + 1 < v.nz;
        const T* p = vol + v.base + (long long)j * v.sy + (long long)z0 * v.sz + (long long)x0 * v.sx;
        double d00 = 0.0, d01 = 0.0, d10 = 0.0, d11 = 0.0;
        if (za && xa) d00 = xr_density(p[0], dn);
        if (za && xb) d01 = xr_density(p[v.sx], dn);
        if (zb && xa) d10 = xr_density(p[v.sz], dn);
        if (zb && xb) d11 = xr_density(p[v.sz + v.sx], dn);
        const double gx = rs_add(1.0, -fx), gz = rs_add(1.0, -fz);
        const double r0 = rs_add(rs_mul(d00, gx), rs_mul(d01, fx));
        const double r1 = rs_add(rs_mul(d10, gx), rs_mul(d11, fx));
        acc = rs_add(acc, rs_add(rs_mul(r0, gz), rs_mul(r1, fz)));
    }
    out[pix] = acc;
}

// grid = ceil(nu * nv / kXrThreads).  out: uint8 [num][nv][nu].  The volume's samples lie in 0 ... num (xr_scan); one that does not sets no bit.
template <typename T, int NW>
__global__ __launch_bounds__(kXrThreads) void project_labels_xr_rays(const T* __restrict__ vol, XrView v, XrTables tb, int num, uint8_t* __restrict__ out) {
    const long long N = (long long)tb.nu * tb.nv;
    const long long pix = (long long)blockIdx.x * kXrThreads + threadIdx.x;
    if (pix >= N) return;
    const int k = (int)(pix / tb.nu), i = (int)(pix - (long long)k * tb.nu);
    const double ai = tb.a[i], cxi = tb.cx[i], bk = tb.b[k], czk = tb.cz[k];
    const double xmax = (double)v.nx, zmax = (double)v.nz;
    uint32_t w[NW];
#pragma unroll
    for (int n = 0; n < NW; ++n) w[n] = 0u;
    for (int j = 0; j < v.ny; ++j) {
        const double tj = tb.t[j];
        const double x = rs_add(rs_add(cxi, rs_mul(tj, ai)), 0.5), z = rs_add(rs_add(czk, rs_mul(tj, bk)), 0.5);
        if (!(x >= 0.0 && x < xmax && z >= 0.0 && z < zmax)) continue;
        const int xi = (int)x, zi = (int)z;                                     // x, z >= 0: the cast is the floor; 0 ... nx - 1, 0 ... nz - 1
        const long long s = (long long)vol[v.base + (long long)j * v.sy + (long long)zi * v.sz + (long long)xi * v.sx];
        const bool in = s > 0 && s <= num;
        const uint32_t b = (uint32_t)(s - 1), word = b >> 5, bit = 1u << (b & 31u);
#pragma unroll
        for (int n = 0; n < NW; ++n) w[n] |= (in && word == (uint32_t)n) ? bit : 0u;
    }
#pragma unroll
    for (int n = 0; n < NW; ++n) {
        const int bits = num - n * 32 < 32 ? num - n * 32 : 32;
        for (int b = 0; b < bits; ++b) out[(long long)(n * 32 + b) * N + pix] = (uint8_t)((w[n] >> b) & 1u);
    }
}

}  // namespace ts2d
