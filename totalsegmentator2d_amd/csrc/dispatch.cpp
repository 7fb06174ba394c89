// Kernel dispatch of libts2d_engine.so: the pixel tiling of a level, which kernel (and which instance of it) serves an op, and what follows
// from that - the activation liveness plan and the layout of the workspace.  Touches no device: a plan can be made on any host.
#include "engine_internal.h"
#include "tile_dims.h"      // kBlock, kBM: the eligibility tests below are written against the kernels' workgroup tile

#include <algorithm>

namespace ts2d {

namespace {

inline int lg_exact(int v) { return (v > 0 && (v & (v - 1)) == 0) ? ilog2(v) : -1; }

inline void tile_finish(TileGeom& g, int B, int Ht, int Wt, int sy, int sx, int taps) {
    const bool p2 = lg_exact(g.TH) >= 0 && lg_exact(g.TW) >= 0;
    g.lgTH = p2 ? ilog2(g.TH) : -1; g.lgTW = p2 ? ilog2(g.TW) : -1;
    if (g.NIMG > 1) { g.tiles_x = 1; g.tiles_y = 1; }
    else { g.tiles_x = (Wt + g.TW - 1) / g.TW; g.tiles_y = (Ht + g.TH - 1) / g.TH; }
    g.n_mtiles = (B + g.NIMG - 1) / g.NIMG * g.tiles_x * g.tiles_y;
    const int halo = (taps == 9) ? 3 : 1;
    g.PH = (g.TH - 1) * sy + halo; g.PW = (g.TW - 1) * sx + halo;
}

// Rounds 1-4: power-of-two tiles (TW = min(32, pow2ceil(Wt)) ...) - complete on 512^2 / 1024^2, idle rows everywhere else.  Kept for
// the first block (level 0 of a real plan is a multiple of 64 or more along both axes) and as the first candidate below.
TileGeom tile_geom_pow2(int B, int Ht, int Wt, int sy, int sx, int taps) {
    TileGeom g{};
    g.TW = std::min(32, pow2ceil(Wt));
    g.TH = std::min(pow2ceil(Ht), kBM / g.TW);
    g.NIMG = std::min(16, kBM / (g.TH * g.TW));
    if (Wt > g.TW || Ht > g.TH) g.NIMG = 1;   // several images share a tile only when a whole image fits in it
    tile_finish(g, B, Ht, Wt, sy, sx, taps);
    return g;
}

// Round 5: the tile shape follows the level's extent (the reference runs whatever patch size plans.json names -
// ts2d/core/inference/prediction_worker.py:76-77 - and nnU-Net patches such as 640 x 384 or 448 x 576 give levels of 80 x 48, 40 x 24,
// 56 x 72, 28 x 36 pixels).  The power-of-two tiling is kept when it is waste-free (bit-compatible with rounds 1-4 on 512^2 / 1024^2);
// otherwise: whole images per tile when at least two fit (any extent: 5 x 6, 10 x 6 ...), else the TH x TW <= 256 with the fewest
// tiles per image whose haloed patch fits the staging budget of EVERY kernel that may serve the op in any precision mode (the
// shape depends on (Ht, Wt, stride) only - never on B or on the mode, so the statistics partials are laid out the same everywhere).
TileGeom tile_geom(int B, int Ht, int Wt, int sy, int sx, int taps) {
    TileGeom g = tile_geom_pow2(B, Ht, Wt, sy, sx, taps);
    const int halo = (taps == 9) ? 3 : 1;
    auto patch = [&](int th, int tw) { return ((th - 1) * sy + halo) * ((tw - 1) * sx + halo); };
    const bool s1 = sy == 1 && sx == 1;
    // staging budgets (patch pixels): conv_mfma_f32 576 / 1296 (ConvCfg::MAXP), conv3x3_f16x3 640, conv3x3s2_f16x3 1536; preferred (one-image
    // kernels): conv3x3_f16x3_one / conv3x3_h32 384, conv3x3s2_f16x3_one 1280
    const int hard = taps == 1 ? (1 << 30) : (s1 ? 576 : 1296), soft = taps == 1 ? (1 << 30) : (s1 ? 384 : 1280);
    // (the power-of-two tile too must fit the budget: 16 images of 2 x 8 are 640 patch pixels, 8 of 1 x 32 are 816 - the kernels stage no more than
    //  their budget and the last images of such a tile read LDS nobody wrote.  tests/test_workspace_plan_cpu.py, W4, found it and holds every tile to it)
    if ((g.NIMG == 1 ? (Ht % g.TH == 0 && Wt % g.TW == 0) : (g.TH == Ht && g.TW == Wt)) && g.NIMG * patch(g.TH, g.TW) <= hard) return g;
    if (Ht * Wt * 2 <= kBM) {
        int n = std::min(16, kBM / (Ht * Wt));
        while (n > 1 && n * patch(Ht, Wt) > hard) --n;
        if (n > 1) { g.TH = Ht; g.TW = Wt; g.NIMG = n; tile_finish(g, B, Ht, Wt, sy, sx, taps); return g; }
    }
    int best_th = 0, best_tw = 0; long best_cost = -1;
    for (int pass = 0; pass < 2 && best_cost < 0; ++pass) {
        const int lim = pass == 0 ? soft : hard;
        for (int tw = std::min(Wt, kBM); tw >= 1; --tw) {
            int th = std::min(Ht, kBM / tw);
            while (th > 1 && patch(th, tw) > lim) --th;
            if (patch(th, tw) > lim) continue;
            th = (Ht + (Ht + th - 1) / th - 1) / ((Ht + th - 1) / th);      // the smallest TH with the same number of tile rows (even tiles)
            const long tiles = (long)((Ht + th - 1) / th) * ((Wt + tw - 1) / tw);
            // fewest tiles; then whole rows of 4 pixels (the 16-byte stores of a lane stay inside a tile row), then the wider tile
            const long cost = tiles * 4 + (tw % 4 ? 1 : 0);
            if (best_cost < 0 || cost < best_cost) { best_cost = cost; best_th = th; best_tw = tw; }
        }
    }
    g.TH = best_th; g.TW = best_tw; g.NIMG = 1;
    tile_finish(g, B, Ht, Wt, sy, sx, taps);
    return g;
}

// Tile of the composed decoder entry on a level that is no multiple of 8 x 32 (conv3x3_upc / conv3x3_upc_h, FLEX instances): TH x TW
// output pixels, both even, <= 256, coarse patch (TH/2 + 2)(TW/2 + 2) <= 128 and skip patch (TH + 2)(TW + 2) <= 384 pixels (the
// kernels' staging units); fewest tiles per image.  ok = false: no shape fills its tiles to 70 %.
TileGeom tile_geom_upc(int B, int Ht, int Wt, bool& ok) {
    ok = false;
    TileGeom g{};
    if (Ht % 2 || Wt % 2) return g;
    int best_th = 0, best_tw = 0; long best = -1;
    for (int tw = std::min(Wt, 128) / 2 * 2; tw >= 2; tw -= 2) {
        int th = std::min(Ht, 256 / tw) / 2 * 2;
        while (th >= 2 && ((th / 2 + 2) * (tw / 2 + 2) > 128 || (th + 2) * (tw + 2) > 384)) th -= 2;
        if (th < 2) continue;
        const int rows = (Ht + th - 1) / th;
        th = ((Ht + rows - 1) / rows + 1) / 2 * 2;            // the smallest even TH with the same number of tile rows
        const long tiles = (long)rows * ((Wt + tw - 1) / tw);
        if (best < 0 || tiles < best) { best = tiles; best_th = th; best_tw = tw; }
    }
    if (best < 0 || (double)Ht * Wt < 0.70 * 256.0 * (double)best) return g;
    ok = true;
    g.TH = best_th; g.TW = best_tw; g.NIMG = 1;
    tile_finish(g, B, Ht, Wt, 1, 1, 9);
    return g;
}

// Output tile of conv3x3s2_v2<.., FLEX> on a level that is no multiple of 8 x 32: TH | Ht, TW | Wt, TW % 4 == 0, TH * TW <= 256, a patch of
// (2 TH + 1) x (2 TW + 2) <= 1122 slots; the largest such tile; ok = false below 3/4 of 256 pixels.
TileGeom tile_geom_s2v2(int B, int Ht, int Wt, bool& ok) {
    ok = false;
    TileGeom g{};
    int best = 0;
    for (int tw = 4; tw <= std::min(Wt, 124); tw += 4) {
        if (Wt % tw) continue;
        for (int th = 1; th <= std::min(Ht, 256 / tw); ++th) {
            if (Ht % th || (2 * th + 1) * (2 * tw + 2) > 1122) continue;
            if (th * tw > best || (th * tw == best && tw > g.TW)) { best = th * tw; g.TH = th; g.TW = tw; }
        }
    }
    if (best < 192) return g;
    ok = true;
    g.NIMG = 1;
    tile_finish(g, B, Ht, Wt, 2, 2, 9);
    return g;
}

// the 8 x 32 / 16 x 32 tilings of the kernels that walk complete tiles of a fixed shape
TileGeom tile_fixed(int B, int Ht, int Wt, int th, int tw, int sy, int sx) {
    TileGeom g{};
    g.TH = th; g.TW = tw; g.NIMG = 1;
    tile_finish(g, B, Ht, Wt, sy, sx, 9);
    return g;
}
// Split-K factor for a split-fp16 conv whose grid would leave most CUs idle (8x8 / 4x4 bottleneck levels).
int choose_ksplit(const Op& op, const TileGeom& g) {
    if (op.type != OP_CONV || !op.split_ok || op.first_direct) return 1;
    // The factor depends on the layer geometry only (never on B), so a slice computes bit-identically alone or in a batch
    // (the whole Choice of the full dispatch, as a property over batches: tests/test_workspace_plan_cpu.py, W5):
    // tiles that hold >= 4 whole images (<= 8x8 pixels per image) leave most CUs idle -> split K as far as 4 chunks/slice.
    if (g.NIMG < 4) return 1;
    const int nchunks = (op.cin + op.cin_skip) / (op.stride == 1 ? 16 : 8);
    int S = 1;
    while (S < 8 && nchunks / (S * 2) >= 4) S *= 2;
    return S;
}

// Small batches (round 6).  TS2D.predict runs tiles x mirrors = 8 slices per sub-model and the reference one (B = 1 per network() call,
// ts2d/core/inference/prediction_worker.py:209): at the <= 32 x 32 levels the persistent / composed kernels then launch 4 ... 64 workgroups on 256 CUs, each
// walking 16 ... 64 channel chunks in series (B = 1: enc5.c0 0.21 ms for 0.6 GMAC).  When the one-image kernel of an op would launch fewer workgroups than
// the chip has CUs, K is split until it does (>= 4 chunks per slice; deterministic two-phase reduction, splitk_reduce_stats), and a composed decoder entry
// runs as transposed conv + conv (the composed kernels have no split-K form).  The factor depends on B: a slice is bit-identical alone or in a batch only
// while both batches take the same path (tests compare across regimes at 2e-6); the same B always gives the same bits.
// Measured (profiles/r06_small_batch.txt, wall time of a forward, split mode): B = 1 2.51 -> 1.90 ms, B = 2 2.77 -> 2.15, B = 4 3.27 -> 2.82, B = 8 4.32 -> 3.98;
// filling to TWO workgroups per CU instead of one: equal (the reduction pass of each further split op costs what its conv gains).
// (kSbkElems, the bound of what this rule splits, and the `full` dispatch flag: engine_internal.h)
int fill_ksplit(const ts2d_engine* e, long long n_wgs, int nchunks, bool full) {
    if (!e->use_sbk || full || e->num_cus > 256) return 1;            // (the bound above assumes <= 256 CUs)
    int S = 1;
    while (S < 8 && n_wgs * S < e->num_cus && nchunks / (S * 2) >= 4) S *= 2;
    return S;
}

// ------------------------------------------------------------------------------------------------------------------ dispatch
// ONE function decides which kernel serves an op for (precision, options, B, H, W).  The activation plan (which tensors exist), the
// workspace sizing and the run (what is launched) all ask it, so they cannot disagree (the eligibility tests
// used to be written at plan time and again inline at launch; round 3's plan / run mismatch came from exactly that).
// The decision is the whole Choice: kernel, instance (split first block, 32-channel chunks, segment length, k-steps) and reported name.
// Nothing outside this file reads an option or the precision mode to pick a kernel; the launchers (engine.hip) add LDS bytes and grid
// sizes only, as arithmetic on Choice, Op and the kernels' own constants.  choose() is also asked for shapes other than the run's
// (workspace sizing), so it depends on its arguments and the engine's options alone - never on workspace pointers.
inline bool fits32(size_t bytes) { return bytes < ((size_t)1 << 31); }      // an image addressed through a 32-bit buffer offset
// the persistent kernels decode a tile number with udiv_magic (kernels.h): exact for tile number x tiles per image < 2^32
inline bool magic_ok(const TileGeom& g) { return (unsigned long long)g.n_mtiles * (unsigned)(g.tiles_x * g.tiles_y) < 0x100000000ull; }

// Thresholds measured on the canonical net at B = 64 (kernel table and the conv3x3_upq paragraph):
constexpr int kUpqMin = 256;      // least coarse channel count served by conv3x3_upq (dec1.c0, Cb = 128: no faster than conv3x3_upc<64>)
constexpr int kH2Min = 64;        // least channel count of a plain 16-bit block served by conv3x3_h2 (enc1-4.c1, dec1-4.c1; below: conv3x3_h32)

// Tiles per workgroup segment of the persistent resident-weight kernels (conv3x3_res32, conv3x3_up0): the largest divisor of an image's
// tiles that still leaves >= 2 workgroups per CU (or all tiles)
int segment_tiles(const ts2d_engine* e, const TileGeom& g) {
    const int tpi = g.tiles_x * g.tiles_y, want = std::min(g.n_mtiles, 2 * e->num_cus);
    int seg = 1;
    for (int d = 1; d <= tpi; ++d) if (tpi % d == 0 && g.n_mtiles / d >= want) seg = d;
    return seg;
}

// Does the first block run as a statistics-only pass, recomputed inside the second block (conv3x3_res32<.., FUSE>)?
bool fuse0_applies(const ts2d_engine* e, int H, int W) {
    // (split mode only.  Measured in the 16-bit mode, B = 64 canonical: 0.30 + 0.94 ms fused against 0.44 + 0.52 ms as two kernels - the
    //  16-bit second block is HBM-bound at a third of the split block's MFMA work, and the recompute is fp32 MFMA work either way)
    //  Round 6, with the recompute on the fp16 matrix path and the statistics pass at 0.25 ms: 0.25 + 0.79 fused against 0.33 + 0.54 - the 16-bit
    //  conversion of the recomputed values (round to fp16 as if stored, normalise, LeakyReLU in fp16) is what the fused kernel is bound by)
    if (!e->use_fuse0 || e->diagnosing || !e->use_res || !e->use_one || e->precision != TS2D_PRECISION_F32_SPLIT_F16X3 || e->ops.size() < 3) return false;
    const Op& o0 = e->ops[0]; const Op& o1 = e->ops[1];
    if (!o0.first_direct || o0.cout != 32 || e->arch.input_channels > 2) return false;
    if (o1.type != OP_CONV || !o1.res_ok || o1.src != o0.dst || o1.skip >= 0) return false;
    for (size_t i = 2; i < e->ops.size(); ++i)       // (a one-conv stage: the tensor is a skip; a residual encoder: the first join adds the stem's output)
        if (e->ops[i].src == o0.dst || e->ops[i].skip == o0.dst || e->ops[i].res == o0.dst) return false;
    if (H % 8 || W % 32) return false;
    return fits32((size_t)H * W * 32 * 4) && fits32((size_t)e->arch.input_channels * H * W * 4);
}

// Which instance of conv3x3s2_v2 serves the op (kernels_s2v2.h)
void s2v2_variant(const ts2d_engine* e, const Op& op, Choice& c) {
    const bool f16 = e->precision == TS2D_PRECISION_F16;
    // 16-bit mode: chunks of 32 channels (the second part of the LDS images = channels 16-31 instead of the split mode's lo parts; K32)
    c.k32 = f16 && e->use_s2k32 && op.cin % 32 == 0;
    c.npp = (f16 && !c.k32) ? 1 : 2; c.nch = op.cin / (c.k32 ? 32 : 16);
    // split mode, 128 columns, fixed tile, weights not resident (two chunks or more): the pipelined instance (kernels_s2v2p.h).  Its conversion is
    // branch-free, so it takes normalised sources only - every stride-2 conv of the supported nets reads one
    c.s2p = e->precision == TS2D_PRECISION_F32_SPLIT_F16X3 && c.bn == 128 && !c.flex && !s2v2_resident(c) && e->use_s2p && e->tensors[op.src].normed;
}

// The decoder block `op` (3x3 conv over cat(up, skip)) as ONE kernel together with its transposed conv (kernels_upc.h ...), or K_NONE.
Kern composed_kernel(const ts2d_engine* e, const Op& op, int B, int H, int W, bool full) {
    if (!op.upc_ok || !e->use_upc || !e->use_one || e->precision == TS2D_PRECISION_F32_EXACT || B < 1) return K_NONE;
    const bool f16 = e->precision == TS2D_PRECISION_F16;
    const Op& up = e->ops[op.up_idx];
    const bool srcs_normed = e->tensors[up.src].normed && e->tensors[op.skip].normed;       // (`normed`, not the scale POINTERS: the plan asks
                                                                                           //  before the workspace - and the pointers - exist)
    if (f16 && (op.cin_skip % 32 || !srcs_normed)) return K_NONE;       // (the 16-bit kernels walk the skip channels in chunks of 32 and normalise both sources)
    const int Ht = H >> op.ly, Wt = W >> op.lx;
    if (!(op.up0_ok && e->use_up0)) {
        // small batch: the two-kernel path when its conv would run with split-K (fill_ksplit) and the upsampled tensor fits the scratch region
        const TileGeom g1 = tile_geom(B, Ht, Wt, 1, 1, 9);
        const int chunk = f16 ? 32 : 16, bn1 = op.cout % 64 == 0 ? 64 : 32;
        const bool two_ok = up.split_ok && (f16 ? op.h32_ok : op.split_ok) && g1.NIMG == 1 && (size_t)B * Ht * Wt * up.cout <= kSbkElems / 2;
        if (two_ok && fill_ksplit(e, (long long)g1.n_mtiles * (op.cout / bn1), ct_total(op) / chunk, full) > 1) return K_NONE;
    }
    if (Ht % 8 || Wt % 32) {                                            // no complete 8 x 32 tiles: tiles that follow the extent (FLEX instances)
        bool ok = false;
        (void)tile_geom_upc(B, Ht, Wt, ok);
        if (!ok || !e->use_flex || !srcs_normed || op.cout % 32) return K_NONE;
        if (!fits32((size_t)Ht * Wt * std::max(op.cout, op.cin_skip) * 4) || !fits32((size_t)(Ht / 2) * (Wt / 2) * up.cin * 4)) return K_NONE;
        return f16 ? K_UPC_H : K_UPC;
    }
    if (op.up0_ok && e->use_up0 && srcs_normed && fits32((size_t)Ht * Wt * 32 * 4)) return K_UP0;
    if (!fits32((size_t)Ht * Wt * std::max(op.cout, op.cin_skip) * 4) || !fits32((size_t)(Ht / 2) * (Wt / 2) * up.cin * 4)) return K_NONE;
    const int bn = op.cout % 64 == 0 ? 64 : 32;

    if (f16) return (e->use_uh2 && bn == 64 && Ht % 16 == 0) ? K_UPC_H2 : K_UPC_H;
    const bool upq = bn == 64 && up.cin >= kUpqMin && Ht % 16 == 0 && srcs_normed && up.cin <= 512 && op.cin_skip <= 512;
    return upq ? K_UPQ : K_UPC;           // (Cb = 128: conv3x3_upq no faster than conv3x3_upc, measured)
}

Choice pick_kernel(const ts2d_engine* e, size_t oi, int B, int H, int W, bool full) {
    const Op& op = e->ops[oi];
    Choice c;
    const bool f16 = e->precision == TS2D_PRECISION_F16, exact = e->precision == TS2D_PRECISION_F32_EXACT;
    if (op.type == OP_PROJ || op.type == OP_JOIN) {
        // Residual blocks (kernels_resblock.h).  The 16-bit mode is opt-in (option "resf16"; without it K_NONE: ts2d_engine_set_precision refuses the
        // mode on such an engine before a forward gets here, and a forward after the option was cleared fails).  Per-pixel work: no pixel tiling,
        // nothing that depends on B or on another option.
        if (f16 && !e->use_resf16) return c;
        c.half = f16;
        c.k = op.type == OP_PROJ ? K_PROJ : K_JOIN;
        c.bn = op.cout % 64 == 0 ? 64 : 32;
        if (op.type == OP_PROJ) {       // tiles of 128 rows of the batch's pixels; partial statistics per tile where an image is a whole number of them
            const int HW = (H >> op.ly) * (W >> op.lx);
            c.fused_stats = HW % 128 == 0;
            c.g.NIMG = 1; c.g.tiles_x = c.fused_stats ? HW / 128 : 1; c.g.tiles_y = 1;
            c.g.n_mtiles = (int)(((long long)B * HW + 127) / 128);
        }
        return c;
    }
    if (op.type == OP_HEAD) {
        const bool hm = op.split_ok && !exact && e->use_one && e->tensors[op.src].C == 32 && (H * W) % 32 == 0 && W % 32 == 0;
        c.k = hm ? K_HEAD_MFMA : K_HEAD_1X1;
        return c;
    }
    if (op.first_direct) {
        c.g = tile_geom_pow2(B, H, W, 1, 1, 9);
        const int kp = (op.cin + 1) / 2, P = c.g.PH * c.g.PW * c.g.NIMG;
        c.fused_stats = c.g.NIMG == 1;
        c.first_full = c.g.NIMG == 1 && c.g.lgTW >= 4 && c.g.lgTH + c.g.lgTW == 8 && H % c.g.TH == 0 && W % c.g.TW == 0 &&
                       P * 2 * kp <= 4 * kBlock && fits32((size_t)H * W * op.cout * 4);
        c.k = fuse0_applies(e, H, W) ? K_FIRST_STATS : K_FIRST;
        // the K = 9 C contraction on the fp16 matrix path (hi / lo split input, one K = 54 product; kernels_first.h SPLIT): every mode but the exact one
        c.first_split = e->use_first_split && !exact && c.first_full && op.cout / 32 == 1 && kp == 1;
        return c;
    }
    const Tensor& src = e->tensors[op.src];
    const int Hin = H >> src.ly, Win = W >> src.lx;
    if (op.type == OP_CONVT) {
        if (oi + 1 < e->ops.size() && e->ops[oi + 1].up_idx == (int)oi && composed_kernel(e, e->ops[oi + 1], B, H, W, full) != K_NONE) {
            c.k = K_FUSED_AWAY;             // composed into the next block: the upsampled tensor is never materialised
            return c;
        }
        c.g = tile_geom(B, Hin, Win, 1, 1, 1);          // (the transposed conv tiles its INPUT pixels)
        const int N = op.sy * op.sx * op.cout;
        if (!(op.split_ok && !exact)) {                 // exact mode, or a kernel other than 2 x 2: the generic kernel in every mode
            if (f16 && op.stride == 2) return c;        // (K_NONE: a 2 x 2 transposed conv without a 16-bit kernel - Cin % 32 != 0)
            c.k = K_EXACT; c.bn = (N % 64 == 0 && op.cout % 64 == 0) ? 64 : 32;
            return c;
        }
        c.bn = 64;                                      // N = 4 * Cout is a multiple of 128; each 32-column tile lies in one (a, b) tap
        c.k = (e->use_one && c.g.NIMG == 1 && fits32((size_t)4 * Hin * Win * op.cout * 4) && fits32((size_t)Hin * Win * op.cin * 4)) ? K_T_ONE : K_T_GENERIC;
        return c;
    }
    const int Ht = H >> op.ly, Wt = W >> op.lx, ct = ct_total(op);
    if (op.up_idx >= 0) {
        const Kern ck = composed_kernel(e, op, B, H, W, full);
        if (ck != K_NONE) {
            c.k = ck; c.fused_stats = true;
            if (ck == K_UP0 && f16) c.ppt = 4;
            c.bn = op.cout % 64 == 0 ? 64 : 32;
            if (Ht % 8 || Wt % 32) { bool ok = false; c.g = tile_geom_upc(B, Ht, Wt, ok); c.flex = true; }
            else c.g = tile_fixed(B, Ht, Wt, (ck == K_UPQ || ck == K_UPC_H2) ? 16 : 8, 32, 1, 1);
            if (ck == K_UPC_H || ck == K_UPC_H2) c.ks = e->ops[op.up_idx].cin % 64 == 0 ? 4 : 2;
            if (ck == K_UP0) {
                c.seg = segment_tiles(e, c.g);
                if (e->u0seg > 0 && (c.g.tiles_x * c.g.tiles_y) % e->u0seg == 0) c.seg = e->u0seg;      // (option "u0seg": tests)
            }
            return c;
        }
    }
    c.bn = op.cout % 64 == 0 ? 64 : 32;
    if (!(op.split_ok && !exact)) {
        if (f16 && op.stride != 3) return c;            // (K_NONE: no 16-bit kernel - channel counts must be multiples of 16)
        c.k = K_EXACT;
        c.g = tile_geom(B, Ht, Wt, op.sy, op.sx, 9);
        c.fused_stats = c.g.NIMG == 1;
        return c;
    }
    const bool img32 = fits32((size_t)Hin * Win * std::max(op.cin, op.cin_skip) * 4) && fits32((size_t)Ht * Wt * op.cout * 4);
    if (op.stride == 2) {
        // small batch: the one-image kernel with split-K where it leaves most CUs idle (fill_ksplit); else the 512-thread kernel
        int s2k = 1;
        {
            const TileGeom g1 = tile_geom(B, Ht, Wt, 2, 2, 9);
            const int P1 = g1.PH * g1.PW * g1.NIMG;
            if (e->use_one && g1.NIMG == 1 && P1 <= 5 * kBlock && img32) s2k = fill_ksplit(e, (long long)g1.n_mtiles * (op.cout / c.bn), op.cin / 8, full);
        }
        if (s2k == 1 && op.s2v2_ok && e->use_s2v2 && e->use_one && Ht % 8 == 0 && Wt % 32 == 0 && img32 && magic_ok(tile_fixed(B, Ht, Wt, 8, 32, 2, 2))) {
            // stride-2 block on complete 8 x 32 output tiles: one 512-thread workgroup per CU, up to 128 output columns
            c.k = K_S2_V2; c.bn = op.bn2; c.fused_stats = true;
            c.g = tile_fixed(B, Ht, Wt, 8, 32, 2, 2);
            s2v2_variant(e, op, c);
            return c;
        }
        if (s2k == 1 && op.s2v2_ok && e->use_s2v2 && e->use_one && e->use_flex2 && img32 && (f16 || e->use_flex2 > 1)) {
            // ... on the tile that divides the level (FLEX instance)
            bool ok = false;
            const TileGeom gs = tile_geom_s2v2(B, Ht, Wt, ok);
            if (ok && magic_ok(gs)) { c.k = K_S2_V2; c.bn = op.bn2; c.fused_stats = true; c.flex = true; c.g = gs; s2v2_variant(e, op, c); return c; }
        }
        c.g = tile_geom(B, Ht, Wt, 2, 2, 9);
        c.ksplit = std::max(choose_ksplit(op, c.g), s2k);
        c.fused_stats = c.g.NIMG == 1 && c.ksplit == 1;
        const int P = c.g.PH * c.g.PW * c.g.NIMG;
        c.k = (e->use_one && c.g.NIMG == 1 && P <= 5 * kBlock && img32) ? K_S2_ONE : K_S2_GENERIC;
        return c;
    }
    if (op.res_ok && e->use_res && e->use_one && src.normed && op.skip < 0 && Ht % 8 == 0 && Wt % 32 == 0 && fits32((size_t)Ht * Wt * 32 * 4)) {
        // 32 -> 32 stride-1 block on complete 8 x 32 tiles: persistent kernel with the layer's weights resident in LDS
        c.k = (oi == 1 && fuse0_applies(e, H, W)) ? K_S1_RES32F : K_S1_RES32;
        c.fused_stats = true;
        c.g = tile_fixed(B, Ht, Wt, 8, 32, 1, 1);
        c.seg = segment_tiles(e, c.g);
        return c;
    }
    c.g = tile_geom(B, Ht, Wt, 1, 1, 9);
    c.ksplit = choose_ksplit(op, c.g);
    c.fused_stats = c.g.NIMG == 1;
    const int P = c.g.PH * c.g.PW * c.g.NIMG;
    const bool srcs_normed = src.normed && (op.skip < 0 || e->tensors[op.skip].normed);
    const bool tiles16 = Ht % 16 == 0 && Wt % 32 == 0 && c.g.NIMG == 1 && img32;          // complete 16 x 32 tiles
    // small batch: split-K on the one-image kernels where they leave most CUs idle (fill_ksplit) - ahead of the 512-thread kernels, which have no split-K form
    if (c.g.NIMG == 1 && img32 && op.cout % c.bn == 0) {
        const bool can = f16 ? (op.h32_ok && P * 4 <= 6 * kBlock) : (e->use_one && P * 2 <= 3 * kBlock);
        const int sk = can ? fill_ksplit(e, (long long)c.g.n_mtiles * (op.cout / c.bn), ct / (f16 ? 32 : 16), full) : 1;
        if (sk > 1) {
            c.ksplit = sk; c.fused_stats = false;
            c.k = f16 ? K_S1_H32 : K_S1_ONE;
            return c;
        }
    }
    if (f16) {
        if (e->use_h2 && tiles16 && op.cout % 64 == 0 && op.skip < 0 && ct % 32 == 0 && src.normed && ct >= kH2Min) {
            c.k = K_S1_H2; c.bn = 64;       // plain C -> C block on 16 x 32 tiles: the skip phase of conv3x3_upc_h2
            c.g = tile_fixed(B, Ht, Wt, 16, 32, 1, 1);
            return c;
        }
        c.k = (op.h32_ok && c.g.NIMG == 1 && P * 4 <= 6 * kBlock && img32) ? K_S1_H32 : K_S1_GENERIC;
        return c;
    }
    const bool one = e->use_one && c.g.NIMG == 1 && P * 2 <= 3 * kBlock && img32;
    if (one && e->use_q && tiles16 && c.bn == 64 && ct >= 64 && srcs_normed && magic_ok(tile_fixed(B, Ht, Wt, 16, 32, 1, 1))) {       // (pays off from 4 chunks on: measured)
        // (round 5: an extent-following variant of this kernel was built and measured - tile = TH x TW <= 512 pixels, row -> pixel by division:
        //  correct, but at 256 registers per wave its two extra address registers spill, and a scratch reload per item in front of the
        //  MFMA stream made it 10-35 % SLOWER than conv3x3_f16x3_one on its extent-following 256-pixel tiles; ragged levels keep that kernel)
        c.k = K_S1_QP;                      // one persistent 512-thread workgroup per CU, patch and weights double-buffered
        c.g = tile_fixed(B, Ht, Wt, 16, 32, 1, 1);
        return c;
    }
    c.k = one ? K_S1_ONE : K_S1_GENERIC;
    return c;
}

// What ts2d_engine_op_kernel reports for the op: the kernel family, with the column tile / chunk width where two instances differ in speed
const char* kernel_name(const Op& op, const Choice& c) {
    const bool b64 = c.bn == 64;
    switch (c.k) {
    case K_NONE: case K_FUSED_AWAY: return "";
    case K_FIRST: return c.first_split ? "conv3x3_first_split" : "conv3x3_first";
    case K_FIRST_STATS: return "conv3x3_first_stats";
    case K_EXACT: return op.type == OP_CONV ? "conv_mfma_f32" : "convT_mfma_f32";
    case K_S1_GENERIC: return "conv3x3_f16x3";
    case K_S1_ONE: return b64 ? "conv3x3_f16x3_one<64>" : "conv3x3_f16x3_one<32>";
    case K_S1_QP: return "conv3x3_f16x3_qp";
    case K_S1_H32: return b64 ? "conv3x3_h32<64>" : "conv3x3_h32<32>";
    case K_S1_H2: return "conv3x3_h2";
    case K_S1_RES32: return "conv3x3_res32";
    case K_S1_RES32F: return "conv3x3_res32f";
    case K_S2_V2: return c.bn == 128 ? (c.k32 ? "conv3x3s2_v2<128,k32>" : "conv3x3s2_v2<128>") : (c.k32 ? "conv3x3s2_v2<64,k32>" : "conv3x3s2_v2<64>");
    case K_S2_ONE: return "conv3x3s2_f16x3_one";
    case K_S2_GENERIC: return "conv3x3s2_f16x3";
    case K_T_ONE: case K_T_GENERIC: return "convT2x2_f16x3";
    case K_UP0: return "conv3x3_up0";
    case K_UPQ: return "conv3x3_upq";
    case K_UPC: return b64 ? "conv3x3_upc<64>" : "conv3x3_upc<32>";
    case K_UPC_H: return b64 ? "conv3x3_upc_h<64>" : "conv3x3_upc_h<32>";
    case K_UPC_H2: return "conv3x3_upc_h2";
    case K_HEAD_MFMA: case K_HEAD_1X1: return "head";
    case K_PROJ: return c.half ? "pool_proj1x1_h" : "pool_proj1x1";
    case K_JOIN: return c.half ? "res_join_h" : "res_join";
    }
    return "";
}

}  // namespace

Choice choose(const ts2d_engine* e, size_t oi, int B, int H, int W, bool full) {
    Choice c = pick_kernel(e, oi, B, H, W, full);
    c.name = kernel_name(e->ops[oi], c);
    return c;
}

std::vector<Choice> choose_all(const ts2d_engine* e, int B, int H, int W, bool full) {
    std::vector<Choice> plan(e->ops.size());
    for (size_t i = 0; i < plan.size(); ++i) plan[i] = choose(e, i, B, H, W, full);
    return plan;
}

// choose_all(), cached per (B, H, W, precision, option generation, full-batch dispatch of the run)
const std::vector<Choice>& planned(ts2d_engine* e, int B, int H, int W, bool full) {
    if (e->plan.size() != e->ops.size() || e->planB != B || e->planH != H || e->planW != W || e->plan_prec != e->precision || e->plan_gen != e->opt_gen ||
        e->plan_full != full) {
        e->plan = choose_all(e, B, H, W, full);
        e->planB = B; e->planH = H; e->planW = W; e->plan_prec = e->precision; e->plan_gen = e->opt_gen; e->plan_full = full;
    }
    return e->plan;
}

namespace {

// The sizing below asks for a (B, H, W) that need not be the cached plan's: it takes the whole plan of that shape, made once per layout.
size_t partial_floats_needed(const ts2d_engine* e, const std::vector<Choice>& plan, int B, int H, int W) {
    size_t mx = 0;
    for (size_t i = 0; i < e->ops.size(); ++i) {
        const Op& op = e->ops[i];
        if (plan[i].ksplit > 1) mx = std::max(mx, (size_t)plan[i].ksplit * B * (H >> op.ly) * (W >> op.lx) * op.cout);
    }
    // a workspace sized for B also serves every smaller batch, whose ops may split K further (fill_ksplit): the bound of that rule
    // (asserted, not only argued: tests/test_workspace_plan_cpu.py, W3, takes every admitted (layout, run) pair of its sweep)
    if (e->use_sbk) mx = std::max(mx, kSbkElems);
    return mx;
}

size_t part_floats_needed(const ts2d_engine* e, const std::vector<Choice>& plan, int B) {
    size_t mx = 0;
    for (size_t i = 0; i < e->ops.size(); ++i) {
        const Op& op = e->ops[i];
        if (op.type != OP_CONV && op.type != OP_PROJ) continue;
        const Choice& c = plan[i];
        if (c.fused_stats) mx = std::max(mx, (size_t)B * c.g.tiles_x * c.g.tiles_y * c.ppt * op.cout * 4);      // (S, Q, K, n) per (tile, channel)
        if (e->use_sbk) mx = std::max(mx, kSbkElems / 256 * 4);      // small-batch split-K (any smaller batch in this workspace): a partial per 256 pixels and channel
    }
    return mx;
}

// Activation plan (round 3): liveness-based reuse.  An activation lives from the op that writes it to the last op that reads it
// (the encoder skips until their decoder block); its bytes then return to a first-fit free list inside ONE arena, sized by
// simulating the program.  Canonical net: 340 -> ~110 MB per slice.  A composed decoder entry (kernels_upc.h) reads the COARSE tensor
// and never materialises `decN.up`, so the plan depends on the precision mode - it is remade when that changes.
// keep_activations: no reuse (every tensor keeps its own buffer for ts2d_engine_debug_tensor / the non-finite diagnosis).
// That no run admitted into a layout writes over a tensor it still reads is tests/test_workspace_plan_cpu.py, W2.
ActPlan plan_activations(const ts2d_engine* e, const std::vector<Choice>& plan, int B, int H, int W, bool keep) {
    const size_t nt = e->tensors.size(), no = e->ops.size();
    ActPlan p; p.off.assign(nt, 0); p.size.assign(nt, 0); p.used.assign(nt, 0); p.reused.assign(nt, 0);
    auto bytes_of = [&](size_t t) { const Tensor& x = e->tensors[t]; return align_up((size_t)B * (H >> x.ly) * (W >> x.lx) * x.C * sizeof(float), 256); };
    // which ops run, what they read
    std::vector<char> skipped(no, 0);
    std::vector<std::vector<int>> reads(no);
    const bool fused0 = plan[0].k == K_FIRST_STATS;        // first block recomputed inside the second: its output tensor is never materialised
    for (size_t i = 0; i < no; ++i) {
        const Op& op = e->ops[i];
        if (fused0 && i == 1) continue;                    // (reads the network input, which is not part of the arena)
        if (plan[i].k == K_FUSED_AWAY) { skipped[i] = 1; continue; }
        if (op.type == OP_CONV && op.up_idx >= 0 && skipped[op.up_idx]) { reads[i] = {e->ops[op.up_idx].src, op.skip}; continue; }
        if (!(op.first_direct)) reads[i].push_back(op.src);
        if (op.skip >= 0) reads[i].push_back(op.skip);
        if (op.res >= 0) reads[i].push_back(op.res);
    }
    std::vector<int> last(nt, -1);
    for (size_t i = 0; i < no; ++i) for (int t : reads[i]) last[t] = (int)i;
    struct Blk { size_t off, size; };
    std::vector<Blk> freel;
    size_t top = 0;
    auto alloc = [&](size_t sz, bool& recycled) {
        int best = -1;
        for (size_t k = 0; k < freel.size(); ++k) if (freel[k].size >= sz && (best < 0 || freel[k].size < freel[best].size)) best = (int)k;
        if (best >= 0) { const size_t o = freel[best].off; freel[best].off += sz; freel[best].size -= sz; if (!freel[best].size) freel.erase(freel.begin() + best); recycled = true; return o; }
        if (!freel.empty() && freel.back().off + freel.back().size == top) {      // grow the arena from a free block at its end
            const size_t o = freel.back().off; top = o + sz; freel.pop_back(); recycled = true; return o;
        }
        const size_t o = top; top += sz; recycled = false; return o;
    };
    auto release = [&](size_t off, size_t sz) {
        size_t k = 0;
        while (k < freel.size() && freel[k].off < off) ++k;
        freel.insert(freel.begin() + k, Blk{off, sz});
        if (k + 1 < freel.size() && freel[k].off + freel[k].size == freel[k + 1].off) { freel[k].size += freel[k + 1].size; freel.erase(freel.begin() + k + 1); }
        if (k > 0 && freel[k - 1].off + freel[k - 1].size == freel[k].off) { freel[k - 1].size += freel[k].size; freel.erase(freel.begin() + k); }
    };
    std::vector<std::pair<size_t, size_t>> live(nt, {0, 0});
    if (!e->ops[0].first_direct) { bool r; p.off[0] = alloc(bytes_of(0), r); p.size[0] = bytes_of(0); p.used[0] = 1; live[0] = {p.off[0], bytes_of(0)}; }
    for (size_t i = 0; i < no; ++i) {
        if (skipped[i]) {
            // keep_activations: a smaller batch inside this workspace may run the entry as two kernels ("sbk", composed_kernel) - its upsampled
            // tensor then gets a buffer of its own instead of the one shared scratch region, so that it is still there after the run
            // (ts2d_engine_debug_tensor, the non-finite diagnosis).  The two-kernel rule bounds the tensor by the scratch region's size.
            if (keep && e->use_sbk) {
                const Op& op = e->ops[i];
                const size_t sz = std::min(bytes_of(op.dst), align_up(kSbkElems / 2 * sizeof(float), 256));
                bool r = false;
                p.off[op.dst] = alloc(sz, r); p.size[op.dst] = sz; p.used[op.dst] = 1; live[op.dst] = {p.off[op.dst], sz};
            }
            continue;
        }
        const Op& op = e->ops[i];
        if (fused0 && i == 0) continue;                      // statistics only: no output tensor
        if (op.dst >= 0) {                                   // the output is placed while the inputs are still allocated: never on top of them
            bool r = false;
            p.off[op.dst] = alloc(bytes_of(op.dst), r); p.size[op.dst] = bytes_of(op.dst); p.used[op.dst] = 1; live[op.dst] = {p.off[op.dst], bytes_of(op.dst)};
            if (last[op.dst] < 0 && !keep) release(live[op.dst].first, live[op.dst].second);       // (never read: e.g. a net whose last tensor feeds nothing)
        }
        if (!keep)
            for (int t : reads[i]) if (last[t] == (int)i && live[t].second) { release(live[t].first, live[t].second); live[t].second = 0; }
    }
    // a tensor's values survive the run unless a LATER tensor overlaps its block
    for (size_t a = 0; a < nt; ++a) {
        if (!p.used[a]) continue;
        for (size_t b2 = 0; b2 < nt; ++b2) {
            if (!p.used[b2] || a == b2) continue;
            const bool later = b2 > a;                       // tensors are numbered in program order of their producers
            if (later && p.off[b2] < p.off[a] + p.size[a] && p.off[a] < p.off[b2] + p.size[b2]) p.reused[a] = 1;
        }
    }
    p.bytes = top;
    return p;
}

}  // namespace

WsLayout workspace_layout(const ts2d_engine* e, int B, int H, int W, bool full) {
    WsLayout L;
    const std::vector<Choice> plan = choose_all(e, B, H, W, full);
    L.plan = plan_activations(e, plan, B, H, W, e->keep_activations);
    for (size_t& o : L.plan.off) o += kWsHeader;          // (the header: owner token of a shared workspace)
    size_t off = align_up(kWsHeader + L.plan.bytes, 256);
    L.o_sc.assign(e->tensors.size(), 0); L.o_sh.assign(e->tensors.size(), 0);
    for (size_t i = 0; i < e->tensors.size(); ++i) {
        const Tensor& t = e->tensors[i];
        if (t.normed) {
            L.o_sc[i] = off; off = align_up(off + (size_t)B * t.C * sizeof(float), 256);
            L.o_sh[i] = off; off = align_up(off + (size_t)B * t.C * sizeof(float), 256);
        }
    }
    L.o_part = off; off = align_up(off + part_floats_needed(e, plan, B) * sizeof(float) + 256, 256);
    L.o_pk = off; off = align_up(off + partial_floats_needed(e, plan, B, H, W) * sizeof(float) + 256, 256);   // split-K partials
    // one upsampled tensor of a small batch's two-kernel decoder entry (composed_kernel): the plan above is the reserved batch's, where that entry is composed
    // (one tenant at a time, read by the next op only, never above the region: tests/test_workspace_plan_cpu.py, W1 and W2)
    L.has_up = e->use_sbk;
    L.o_up = off; if (L.has_up) off = align_up(off + kSbkElems / 2 * sizeof(float) + 256, 256);
    L.bytes = off;
    return L;
}

}  // namespace ts2d
