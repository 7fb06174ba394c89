// Host arithmetic of the PNG visuals (visual.hip): the per-axis tables of resample_uniform, the constants of the mirror prefilter, the window.
// Plain C++: every statement here must match visual.py (numpy float64) bit for bit, so none of it is compiled as HIP code and no product
// feeds a sum unrounded.  floor, pow and every division of the feature live here; the kernels hold none.
#include "visual_plan.h"

#include <cmath>

namespace ts2d {
namespace {

// the float64 nearest to sqrt(3) - 2 (prep_plan.cpp: kRsInPole)
const double kVisPole = -0x1.126145e9ecd56p-2;

int fold_mirror(long long i, int n) {
    if (n == 1) return 0;
    const long long p = 2LL * (n - 1);
    i %= p;
    if (i < 0) i += p;
    return (int)(i > n - 1 ? p - i : i);
}

}  // namespace

int visual_axis_extent(int N, double s, double m) {
#pragma clang fp contract(off)
    const double prod = (double)N * s;
    const double q = prod / m;
    const double v = 0.5 + q;
    if (!(v >= 1.0) || !(v < (double)kVisMaxOutExtent + 1.0)) return -1;
    return (int)v;
}

void visual_axis_table(int N, double s, double m, int M, VisTap* t) {
#pragma clang fp contract(off)
    const double ratio = m / s;
    const double c = (double)(N / 2);
    for (int j = 0; j < M; ++j) {
        const double step = (double)(j - M / 2) * ratio;
        const double x = c + step;
        VisTap& e = t[j];
        e.inside = (x >= -0.5 && x < (double)N - 0.5) ? 1 : 0;
        if (!e.inside) {
            for (int k = 0; k < 4; ++k) { e.w[k] = 0.0; e.idx[k] = 0; }
            e.nearest = -1;
            continue;
        }
        const int up = (int)std::floor(x + 0.5);
        e.nearest = up > N - 1 ? N - 1 : up;         // (x + 0.5 may round up to N just below the upper edge; the kernels read where this points)
        const double f = std::floor(x);
        const double y = x - f, u = 1.0 - y;
        const double yy = y * y, uu = u * u;
        const double a1 = yy * (y - 2.0), a2 = uu * (u - 2.0);
        const double b1 = a1 * 3.0, b2 = a2 * 3.0;
        e.w[1] = (b1 + 4.0) / 6.0;
        e.w[2] = (b2 + 4.0) / 6.0;
        const double u3 = uu * u;
        e.w[0] = u3 / 6.0;
        const double r0 = 1.0 - e.w[0], r1 = r0 - e.w[1];
        e.w[3] = r1 - e.w[2];
        for (int k = 0; k < 4; ++k) e.idx[k] = fold_mirror((long long)f - 1 + k, N);
    }
}

VisAxis visual_axis_constants(int n) {
#pragma clang fp contract(off)
    VisAxis a;
    a.z = kVisPole;
    const double inv = 1.0 / a.z;
    a.gain = (1.0 - a.z) * (1.0 - inv);
    a.zn1 = std::pow(a.z, (double)(n - 1));
    const double zn2 = a.zn1 * a.zn1;
    a.k0 = 1.0 / (1.0 - zn2);
    const double zz = a.z * a.z;
    a.k1 = a.z / (zz - 1.0);
    return a;
}

void visual_zpow(int n, double* zpow) {
#pragma clang fp contract(off)
    if (n > 0) zpow[0] = 1.0;
    if (n > 1) zpow[1] = kVisPole;
    for (int i = 2; i < n; ++i) zpow[i] = zpow[i - 1] * kVisPole;
}

VisWindow visual_window(double lo, double hi) {
#pragma clang fp contract(off)
    VisWindow w;
    w.lo = lo; w.hi = hi;
    w.scale = 255.0 / (hi - lo);
    const double nlo = -lo;
    w.shift = nlo * w.scale;
    return w;
}

void visual_color_lut(const uint8_t* palette, int n, uint32_t lut[256]) {
    lut[0] = 0;
    for (int v = 1; v < 256; ++v) {
        const uint8_t* c = palette + 3 * (v % n);
        lut[v] = (uint32_t)c[0] | ((uint32_t)c[1] << 8) | ((uint32_t)c[2] << 16);
    }
}

}  // namespace ts2d
