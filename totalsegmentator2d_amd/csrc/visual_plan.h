// Host tables of the PNG visuals (visual.hip, kernels_visual.h): what visual.py states per axis - extent, nearest index, cubic taps, inside
// flag - the constants of the mirror prefilter, the window's scale and shift, the colour of every label value.  Plain C++ with no HIP type in
// it, so visual_plan.cpp also compiles into a stand-alone host program (tests/test_visual_cpu.py compares its tables with visual.axis_table).
#pragma once
#include <stdint.h>

#pragma GCC visibility push(hidden)      // (the library exports the C-ABI only)
namespace ts2d {

constexpr int kVisMaxExtent = 8192;         // visual.MAX_EXTENT: per input axis
constexpr int kVisMaxOutExtent = 32768;     // visual.MAX_OUT_EXTENT: per output axis

struct VisTap {             // one output index of one axis
    double w[4];            // cubic B-spline weights of the four taps (0 outside)
    int idx[4];             // their source indices, mirror-folded onto 0 ... N-1 (0 outside)
    int nearest;            // floor(x + 0.5), or -1 outside
    int inside;             // -0.5 <= x < N - 0.5
};
static_assert(sizeof(VisTap) == 56, "VisTap is copied to the device as bytes");

struct VisAxis {            // line-independent constants of the mirror prefilter along an axis of n samples
    double z, gain, zn1;    // pole, gain, z^(n-1) (libm pow on the host)
    double k0, k1;          // 1 / (1 - z^(n-1) * z^(n-1)),  z / (z*z - 1)
};
static_assert(sizeof(VisAxis) == 40, "VisAxis is passed by value");

struct VisWindow {          // IntensityWindowing to 0 ... 255
    double lo, hi, scale, shift;        // scale = 255 / (hi - lo), shift = -lo * scale
};

// int(0.5 + N*s/m), or -1 when that is no extent in 1 ... kVisMaxOutExtent
int visual_axis_extent(int N, double s, double m);
// the M entries of one axis: x_j = (N/2) + (j - M/2) * (m/s) in float64, in that order
void visual_axis_table(int N, double s, double m, int M, VisTap* t);
VisAxis visual_axis_constants(int n);
// zpow[0] = 1, zpow[i] = zpow[i-1] * z: the running products of the pole (they pass through denormals on long lines), NOT pow(z, i)
void visual_zpow(int n, double* zpow);
VisWindow visual_window(double lo, double hi);
// lut[v] = 0 for v = 0, else the colour palette[v % n] packed r | g << 8 | b << 16
void visual_color_lut(const uint8_t* palette, int n, uint32_t lut[256]);

}  // namespace ts2d
#pragma GCC visibility pop
