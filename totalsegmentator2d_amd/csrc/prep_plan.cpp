// Host arithmetic of the input side (prep.hip): the taps and prefilter constants of the order-3 resample, the fold of numpy's pairwise
// sum behind the z-score, and the ray tables, step lengths and final cast of the synthetic radiograph.  Plain C++: every statement here must match scipy / numpy bit for bit, so none of it is compiled as HIP code.
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

// The ray tables of a synthetic radiograph (totalsegmentator2d_amd/xray.py: xr_tables is the same statement in numpy), one rounding per
// operation.  Refuses, by name, what XRGeometry.resolve refuses; on a refusal the plan is not to be used.
int xr_plan(const char* entry, const XrGeometry& g, XrPlan* pl) {
#pragma clang fp contract(off)
    if (g.nz < 1 || g.ny < 1 || g.nx < 1) return fail(TS2D_ERR_INVALID, "%s: extents nz %d, ny %d, nx %d below 1", entry, g.nz, g.ny, g.nx);
    if (g.pa != 0 && g.pa != 1) return fail(TS2D_ERR_INVALID, "%s: view %d is neither 0 (ap) nor 1 (pa)", entry, g.pa);
    if (g.parallel != 0 && g.parallel != 1) return fail(TS2D_ERR_INVALID, "%s: parallel %d is neither 0 nor 1", entry, g.parallel);
    const struct { const char* name; double v; } positive[] = {{"spacing_x", g.sx}, {"spacing_y", g.sy}, {"spacing_z", g.sz},
        {"source_detector_mm", g.sdd}, {"source_center_mm", g.sod}, {"du", g.du}, {"dv", g.dv}};
    for (const auto& c : positive)
        if (!(std::isfinite(c.v) && c.v > 0.0)) return fail(TS2D_ERR_INVALID, "%s: %s = %g is not finite and positive", entry, c.name, c.v);
    const double half = (double)(g.ny - 1) * g.sy / 2.0;
    if (!(g.sod > half))
        return fail(TS2D_ERR_INVALID, "%s: source_center_mm = %g puts the source inside the slab of plane centres (half depth %g mm)", entry, g.sod, half);
    if (g.sdd - g.sod < half)
        return fail(TS2D_ERR_INVALID, "%s: source_detector_mm - source_center_mm = %g puts the detector inside the slab of plane centres (half depth %g mm)",
                    entry, g.sdd - g.sod, half);
    if (g.nu < 1 || g.nv < 1) return fail(TS2D_ERR_INVALID, "%s: detector size nu %d, nv %d below 1", entry, g.nu, g.nv);
    if ((long long)g.nu * g.nv > 0x7FFFFFFFll)
        return fail(TS2D_ERR_INVALID, "%s: detector size nu %d x nv %d is more than 2^31 - 1 pixels", entry, g.nu, g.nv);
    if (g.parallel && (g.nu != g.nx || g.nv != g.nz || g.du != g.sx || g.dv != g.sz))
        return fail(TS2D_ERR_INVALID, "%s: parallel rays fix the detector to nu = nx, nv = nz, du = spacing_x, dv = spacing_z", entry);
    const double Cx = (double)(g.nx - 1) * g.sx / 2.0, Cy = (double)(g.ny - 1) * g.sy / 2.0, Cz = (double)(g.nz - 1) * g.sz / 2.0;
    const double sign = g.pa ? -1.0 : 1.0;
    const double Sy = Cy - sign * g.sod;
    const double Yd = Sy + sign * g.sdd;
    const double den = Yd - Sy;
    const double hu = (double)(g.nu - 1) / 2.0, hv = (double)(g.nv - 1) / 2.0;
    pl->parallel = g.parallel != 0; pl->sy = g.sy; pl->nu = g.nu; pl->nv = g.nv;
    pl->t.resize((size_t)g.ny);
    pl->a.resize((size_t)g.nu); pl->cx.resize((size_t)g.nu); pl->p.resize((size_t)g.nu);
    pl->b.resize((size_t)g.nv); pl->cz.resize((size_t)g.nv); pl->q.resize((size_t)g.nv);
    for (int j = 0; j < g.ny; ++j) pl->t[(size_t)j] = g.parallel ? 0.0 : ((double)j * g.sy - Sy) / den;
    const double cx = Cx / g.sx, cz = Cz / g.sz;
    for (int i = 0; i < g.nu; ++i) {
        const double U = Cx + ((double)i - hu) * g.du, off = U - Cx;
        pl->a[(size_t)i] = off / g.sx; pl->p[(size_t)i] = off / den; pl->cx[(size_t)i] = g.parallel ? (double)i : cx;
    }
    for (int k = 0; k < g.nv; ++k) {
        const double V = Cz + ((double)k - hv) * g.dv, off = V - Cz;
        pl->b[(size_t)k] = off / g.sz; pl->q[(size_t)k] = off / den; pl->cz[(size_t)k] = g.parallel ? (double)k : cz;
    }
    return TS2D_OK;
}

// the step length of ray (k, i): sy * sqrt((1 + p_i p_i) + q_k q_k), sy for parallel rays
double xr_step(const XrPlan& pl, int k, int i) {
#pragma clang fp contract(off)
    if (pl.parallel) return pl.sy;
    const double p = pl.p[(size_t)i], q = pl.q[(size_t)k];
    const double pp = p * p, qq = q * q;
    const double s = (1.0 + pp) + qq;
    return pl.sy * std::sqrt(s);
}

// the radiograph from the downloaded sums: float32(sum * step)
void xr_finish(const XrPlan& pl, const double* sum, float* out) {
#pragma clang fp contract(off)
    for (int k = 0; k < pl.nv; ++k)
        for (int i = 0; i < pl.nu; ++i) {
            const size_t at = (size_t)k * pl.nu + i;
            const double v = sum[at] * xr_step(pl, k, i);
            out[at] = (float)v;
        }
}

}  // namespace ts2d
