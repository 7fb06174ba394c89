// Host arithmetic of the input side (prep.hip): the taps and prefilter constants of the order-3 resample, and the fold of numpy's pairwise
// sum behind the z-score.  Plain C++: every statement here must match scipy / numpy bit for bit, so none of it is compiled as HIP code.
#include "engine_internal.h"

#include <algorithm>
#include <cmath>
#include <cstring>

namespace ts2d {
namespace {

// Taps of one axis of the order-3 resample (n_in -> n_out samples; preprocess.cubic_axis_taps is the same statement in numpy, pinned to
// scipy): cc = ((o + 0.5) * (n_in / n_out) - 0.5) + 12 clamped to the padded extent, start = floor(cc) - 1, y = cc - floor(cc), t = 1 - y,
// w1 = (y*y*(y-2)*3 + 4) / 6, w2 = (t*t*(t-2)*3 + 4) / 6, w0 = t*t*t / 6, w3 = 1 - w0 - w1 - w2, one rounding per step.  False if a tap
// would leave the padded line (with this map it cannot: cc lies in [11.5, n_in + 11.5]; checked because the kernel reads where it points).
bool rsin_axis_taps(int n_in, int n_out, RsInTap* t) {
#pragma clang fp contract(off)
    const int n_pad = n_in + 2 * kRsInPad;
    const double zoom = (double)n_in / (double)n_out;
    for (int o = 0; o < n_out; ++o) {
        const double prod = ((double)o + 0.5) * zoom;
        const double shifted = prod - 0.5;
        double cc = shifted + (double)kRsInPad;
        cc = std::min(std::max(cc, 0.0), (double)(n_pad - 1));
        const double f = std::floor(cc);
        const long long start = (long long)f - 1;
        if (start < 0 || start + 3 > n_pad - 1) return false;
        const double y = cc - f, u = 1.0 - y;
        const double yy = y * y, uu = u * u;
        const double a1 = yy * (y - 2.0), a2 = uu * (u - 2.0);
        const double b1 = a1 * 3.0, b2 = a2 * 3.0;
        t[o].w[1] = (b1 + 4.0) / 6.0;
        t[o].w[2] = (b2 + 4.0) / 6.0;
        const double u3 = uu * u;
        t[o].w[0] = u3 / 6.0;
        const double r0 = 1.0 - t[o].w[0], r1 = r0 - t[o].w[1];
        t[o].w[3] = r1 - t[o].w[2];
        t[o].start = (int)start; t[o].pad_ = 0;
    }
    return true;
}

// The float64 nearest to sqrt(3) - 2: what scipy's binary holds for the pole of the cubic prefilter (its compiler folds the constant
// in extended precision).  std::sqrt(3.0) - 2.0 is two units in the last place away and would cost the bit identity.
const double kRsInPole = -0x1.126145e9ecd56p-2;

RsInAxis rsin_axis_constants(int n_pad) {
#pragma clang fp contract(off)
    RsInAxis a;
    a.z = kRsInPole;
    const double inv = 1.0 / a.z;
    a.gain = (1.0 - a.z) * (1.0 - inv);
    a.zn = std::pow(a.z, (double)n_pad);
    const double zn2 = a.zn * a.zn;
    a.k0 = a.z / (1.0 - zn2);
    a.k1 = a.z / (a.z - 1.0);
    return a;
}

// the same recursion as prep_leaves over the leaves' sums: every inner node adds its two halves, rounded to float32
float prep_fold(const float*& leaf, int n) {
#pragma clang fp contract(off)
    if (n <= kPrepLeaf) return *leaf++;
    int n2 = n / 2; n2 -= n2 % 8;
    const float a = prep_fold(leaf, n2);
    const float b = prep_fold(leaf, n - n2);
    return a + b;
}

}  // namespace

int rsin_plan(const char* entry, int n_planes, int in_h, int in_w, int out_h, int out_w, RsInPlan* pl) {
    pl->Hp = in_h + 2 * kRsInPad; pl->Wp = in_w + 2 * kRsInPad;
    pl->taps.resize((size_t)out_h + out_w);
    if (!rsin_axis_taps(in_h, out_h, pl->taps.data()) || !rsin_axis_taps(in_w, out_w, pl->taps.data() + out_h))
        return fail(TS2D_ERR_INVALID, "%s: zoom %d x %d -> %d x %d puts a tap outside the padded plane", entry, in_h, in_w, out_h, out_w);
    pl->zpow.resize((size_t)std::max(pl->Hp, pl->Wp));
    {
#pragma clang fp contract(off)
        pl->zpow[0] = 1.0; pl->zpow[1] = kRsInPole;
        for (size_t i = 2; i < pl->zpow.size(); ++i) pl->zpow[i] = pl->zpow[i - 1] * kRsInPole;
    }
    pl->ax_h = rsin_axis_constants(pl->Hp); pl->ax_w = rsin_axis_constants(pl->Wp);
    pl->o_pow = align_up((size_t)n_planes * pl->Hp * pl->Wp * sizeof(double), 256);
    pl->o_taps = align_up(pl->o_pow + pl->zpow.size() * sizeof(double), 256);
    pl->bytes = align_up(pl->o_taps + pl->taps.size() * sizeof(RsInTap), 256);
    return TS2D_OK;
}

// leaves of numpy's pairwise sum over a run of n elements (the partial chunk of a plane), in the order the recursion visits them
void prep_leaves(int off, int n, std::vector<PrepLeaf>* out) {
    if (n <= kPrepLeaf) { out->push_back(PrepLeaf{off, n}); return; }
    int n2 = n / 2; n2 -= n2 % 8;
    prep_leaves(off, n2, out);
    prep_leaves(off + n2, n - n2, out);
}

// numpy's add.reduce of one plane from what prep_chunk_sums wrote: +0, plus each chunk's pairwise sum in index order
float prep_plane_sum(const float* sums, long long n) {
#pragma clang fp contract(off)
    const long long n_full = n / kPrepChunk;
    float acc = 0.f;
    for (long long c = 0; c < n_full; ++c) acc = acc + sums[c];
    if (n % kPrepChunk) { const float* leaf = sums + n_full; const float tail = prep_fold(leaf, (int)(n % kPrepChunk)); acc = acc + tail; }
    return acc;
}

// RescaleTo01Normalization's divisor from the plane's minimum and maximum: numpy takes `clip(max(img - min), 1e-8, None)`; x -> fl32(x - min)
// is monotone, so that maximum is fl32(max - min), and the clip is `d < lo ? lo : d` with lo = float32(1e-8) (a NaN stays NaN)
float prep_rescale_div(float mn, float mx) {
#pragma clang fp contract(off)
    const float d = mx - mn, lo = (float)1e-8;
    return d < lo ? lo : d;
}

float prep_unkey(int key) { const int b = key < 0 ? key ^ 0x7FFFFFFF : key; float f; std::memcpy(&f, &b, 4); return f; }

}  // namespace ts2d
