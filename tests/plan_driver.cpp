// TEST INFRASTRUCTURE (never linked into the product): the host planners behind a main of their own.  Built by tests/test_workspace_plan_cpu.py
// and tests/test_tiled_plan_cpu.py together with csrc/dispatch.cpp, csrc/program.cpp and csrc/tiled_plan.cpp under the address and
// undefined-behaviour sanitizers; touches no device and is never loaded into Python.
//
//     plan_driver ws SPEC [--tamper N] [--show N]       the workspace properties W1-W5 over the sweep that SPEC states
//     plan_driver tiled [--tamper N]         the sliding-window plan properties T1-T4 and the refusals over the scenario table below
//
// The checkers read Op, Tensor, Choice, WsLayout and SwPlan DATA only: every expected figure is restated here from the launcher or kernel
// that consumes the region (file:line beside each), never asked of the planner again.
#include "engine_internal.h"

#include <algorithm>
#include <cinttypes>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <map>
#include <memory>
#include <sstream>
#include <string>
#include <tuple>
#include <vector>

using namespace ts2d;

namespace {

// ------------------------------------------------------------------------------------------------------------------ reporting
struct Report {
    std::map<std::string, long long> n;
    long long show = 8;                 // violations printed per property (--show N)
    std::string where;                  // the case being checked: "net mode=.. H=.. W=.. Bw=.. fw=.. b=.. fr=.. opts"
    void viol(const char* prop, const std::string& msg) {
        if (n[prop]++ < show) std::printf("viol %s %s :: %s\n", prop, where.c_str(), msg.c_str());      // (the first few of a kind name the case; the tally has them all)
    }
};
Report g_rep;

std::string fmt(const char* f, ...) __attribute__((format(printf, 1, 2)));
std::string fmt(const char* f, ...) {
    char buf[512];
    va_list ap; va_start(ap, f); vsnprintf(buf, sizeof(buf), f, ap); va_end(ap);
    return buf;
}

// ------------------------------------------------------------------------------------------------------------------ the engine, minus the device
// What create_engine does before it touches the device (engine.hip:748-756): the caller's descriptor, the padded one, the blocks of a
// residual encoder, the program.
std::unique_ptr<ts2d_engine> make_engine(const ts2d_arch_desc& arch, const int* n_blocks) {
    std::unique_ptr<ts2d_engine> e(new ts2d_engine());
    e->user_arch = arch;
    if (n_blocks) { e->residual = true; for (int s = 0; s < TS2D_MAX_STAGES; ++s) e->n_blocks[s] = n_blocks[s]; }
    e->arch = pad_arch(arch, e->padded);
    if (build_program(e.get()) != TS2D_OK) { std::fprintf(stderr, "build_program: %s\n", last_error()); return nullptr; }
    return e;
}

bool set_option(ts2d_engine* e, const std::string& name, int v) {      // the fields ts2d_engine_set_option sets (engine.hip:818-820)
    struct B { const char* n; bool* p; };
    const B bools[] = {{"one", &e->use_one}, {"s2v2", &e->use_s2v2}, {"q", &e->use_q}, {"h2", &e->use_h2}, {"uh2", &e->use_uh2}, {"first_split", &e->use_first_split},
                       {"sbk", &e->use_sbk}, {"s2k32", &e->use_s2k32}, {"s2p", &e->use_s2p}, {"up0", &e->use_up0}, {"upc", &e->use_upc}, {"res", &e->use_res},
                       {"fuse0", &e->use_fuse0}, {"flex", &e->use_flex}, {"resf16", &e->use_resf16}, {"keep", &e->keep_activations}};
    for (const B& b : bools) if (name == b.n) { *b.p = v != 0; return true; }
    if (name == "flex2") { e->use_flex2 = v; return true; }
    if (name == "u0seg") { e->u0seg = v; return true; }
    if (name == "num_cus") { e->num_cus = v; return true; }
    return false;
}

// ------------------------------------------------------------------------------------------------------------------ the run, as the launchers read it
struct Shape { int b, H, W; };
size_t elems_of(const ts2d_engine* e, int t, const Shape& s) { const Tensor& x = e->tensors[t]; return (size_t)s.b * (s.H >> x.ly) * (s.W >> x.lx) * x.C; }
// Bytes a run writes of tensor t.  Counted at four bytes per element in every mode: the 16-bit mode stores halves (engine.hip:585, ST* out), the
// plan sizes every buffer for floats, and the check holds the plan to what it sizes.
size_t bytes_of(const ts2d_engine* e, int t, const Shape& s) { return elems_of(e, t, s) * sizeof(float); }

bool composed(Kern k) { return k == K_UP0 || k == K_UPQ || k == K_UPC || k == K_UPC_H || k == K_UPC_H2; }
bool runs(const Choice& c) { return c.k != K_NONE && c.k != K_FUSED_AWAY; }

// the activation tensors op i of the run reads (the network input is no part of the arena)
std::vector<int> reads_of(const ts2d_engine* e, const std::vector<Choice>& plan, size_t i) {
    const Op& op = e->ops[i];
    const Kern k = plan[i].k;
    if (!runs(plan[i])) return {};
    if (k == K_FIRST || k == K_FIRST_STATS) return {};                                       // engine.hip:208 (fa.x = r.d_in)
    if (composed(k)) return {e->ops[op.up_idx].src, op.skip};                                // engine.hip:248, 270 (the coarse tensor and the skip)
    if (k == K_S1_RES32F) return {};                                                         // engine.hip:325 (ra.src = nullptr, ra.x0 = r.d_in)
    if (k == K_JOIN) return {op.src, op.res};                                                // engine.hip:388
    if (k == K_S1_RES32 || k == K_PROJ || k == K_HEAD_MFMA || k == K_HEAD_1X1 || k == K_S1_H2) return {op.src};      // engine.hip:312, 368, 340, 484
    std::vector<int> r{op.src};                                                              // engine.hip:507-508 (launch_conv_family)
    if (op.skip >= 0) r.push_back(op.skip);
    return r;
}
// ... and whether it writes its output tensor (the statistics-only first pass stores nothing: engine.hip:219, 229)
bool writes_dst(const ts2d_engine* e, const std::vector<Choice>& plan, size_t i) { return runs(plan[i]) && e->ops[i].dst >= 0 && plan[i].k != K_FIRST_STATS; }

// The documented refusals: a 16-bit mode without a 16-bit kernel for the op (dispatch.cpp names them; here from the Op alone)
bool refusal_expected(const ts2d_engine* e, const Op& op) {
    if (e->precision != TS2D_PRECISION_F16) return false;
    if (op.type == OP_PROJ || op.type == OP_JOIN) return !e->use_resf16;
    if (op.type == OP_CONVT) return !op.split_ok && op.stride == 2;
    if (op.type == OP_CONV) return !op.first_direct && !op.split_ok && op.stride != 3;
    return false;
}

struct Region { std::string name; size_t off, need; };

struct Placed { bool ok = false; bool in_up = false; size_t off = 0, cap = 0; };
// Where the run finds tensor t: its buffer of the layout (engine.hip:88-90) or, for the output of a transposed conv the layout has no buffer
// for, the one scratch region (place_uncomposed_ups, engine.hip:609-621)
Placed place(const ts2d_engine* e, const WsLayout& L, int t, bool convt_out, const Shape& s) {
    Placed p;
    if (L.plan.used[t]) { p.ok = true; p.off = L.plan.off[t]; p.cap = L.plan.size[t]; return p; }
    if (convt_out && L.has_up && elems_of(e, t, s) <= kSbkElems / 2) { p.ok = true; p.in_up = true; p.off = L.o_up; p.cap = kSbkElems / 2 * sizeof(float); }
    return p;
}

// W1, W2, W3 of one admitted (layout, run) pair
void check_pair(const ts2d_engine* e, const WsLayout& L, const std::vector<Choice>& plan, const Shape& s) {
    const size_t no = e->ops.size(), nt = e->tensors.size();
    // ---- W1: a buffer for every output
    std::vector<Placed> at(nt);
    std::vector<int> wrote(nt, -2);                     // op that writes the tensor (-1: the layout change of the input, engine.hip:650-655)
    if (!e->ops[0].first_direct) wrote[0] = -1;
    for (size_t i = 0; i < no; ++i) {
        if (plan[i].k == K_NONE && !refusal_expected(e, e->ops[i])) g_rep.viol("W1", fmt("op %s has no kernel and no documented refusal", e->ops[i].name.c_str()));
        if (writes_dst(e, plan, i)) wrote[e->ops[i].dst] = (int)i;
    }
    for (size_t t = 0; t < nt; ++t) {
        if (wrote[t] == -2) continue;
        const bool convt_out = wrote[t] >= 0 && e->ops[wrote[t]].type == OP_CONVT;
        at[t] = place(e, L, (int)t, convt_out, s);
        if (!at[t].ok) { g_rep.viol("W1", fmt("tensor %s (%zu elements) has no buffer: used=%d has_up=%d", e->tensors[t].name.c_str(), elems_of(e, (int)t, s), (int)L.plan.used[t], (int)L.has_up)); continue; }
        if (at[t].cap < bytes_of(e, (int)t, s)) g_rep.viol("W1", fmt("tensor %s writes %zu bytes into a buffer of %zu", e->tensors[t].name.c_str(), bytes_of(e, (int)t, s), at[t].cap));
    }
    // ---- W2: no live tensor is overwritten
    std::vector<std::vector<int>> reads(no);
    std::vector<int> last(nt, -2);
    for (size_t i = 0; i < no; ++i) { reads[i] = reads_of(e, plan, i); for (int t : reads[i]) last[t] = (int)i; }
    for (size_t i = 0; i < no; ++i)
        for (int t : reads[i]) if (wrote[t] == -2 || wrote[t] >= (int)i) g_rep.viol("W2", fmt("op %s reads %s, which no earlier op of the run wrote", e->ops[i].name.c_str(), e->tensors[t].name.c_str()));
    auto overlap = [&](int a, int b) {
        return at[a].ok && at[b].ok && at[a].off < at[b].off + bytes_of(e, b, s) && at[b].off < at[a].off + bytes_of(e, a, s);
    };
    for (size_t i = 0; i < no; ++i) {
        if (!writes_dst(e, plan, i)) continue;
        const int d = e->ops[i].dst;
        for (size_t t = 0; t < nt; ++t)
            if ((int)t != d && wrote[t] != -2 && wrote[t] < (int)i && last[t] >= (int)i && overlap(d, (int)t))
                g_rep.viol("W2", fmt("op %s writes %s at [%zu, +%zu) over %s at [%zu, +%zu), read last by op %s", e->ops[i].name.c_str(), e->tensors[d].name.c_str(), at[d].off,
                                     bytes_of(e, d, s), e->tensors[t].name.c_str(), at[t].off, bytes_of(e, (int)t, s), e->ops[last[t]].name.c_str()));
        if (at[d].in_up)       // one tenant of the scratch at a time: read by the very next op only
            for (size_t j = 0; j < no; ++j)
                for (int t : reads[j]) if (t == d && j != i + 1) g_rep.viol("W2", fmt("%s lives in the one scratch region and is read by op %s, not only the next op", e->tensors[d].name.c_str(), e->ops[j].name.c_str()));
    }
    if (e->keep_activations)
        for (size_t a = 0; a < nt; ++a)
            for (size_t b = a + 1; b < nt; ++b)
                if (wrote[a] != -2 && wrote[b] != -2 && overlap((int)a, (int)b))
                    g_rep.viol("W2", fmt("keep_activations: %s and %s share bytes", e->tensors[a].name.c_str(), e->tensors[b].name.c_str()));
    // ---- W3: side regions, each with what its consumers touch
    std::vector<Region> side;
    for (size_t t = 0; t < nt; ++t)
        if (e->tensors[t].normed) {      // scale / shift [n * C + c], n < B (kernels.h:417-418, 443-444, 486-487; the join: engine.hip:391)
            side.push_back({e->tensors[t].name + ".scale", L.o_sc[t], (size_t)s.b * e->tensors[t].C * sizeof(float)});
            side.push_back({e->tensors[t].name + ".shift", L.o_sh[t], (size_t)s.b * e->tensors[t].C * sizeof(float)});
        }
    size_t part = 0, pk = 0, up = 0;
    for (size_t i = 0; i < no; ++i) {
        const Op& op = e->ops[i]; const Choice& c = plan[i];
        if (!runs(c)) continue;
        const size_t HW = (size_t)(s.H >> op.ly) * (s.W >> op.lx);
        if (c.ksplit > 1) {
            // K slice k of the conv at d_partial + k * B Ht Wt Cout (engine.hip:555-556); the reduce pass reads S of them (kernels.h:468, 507)
            pk = std::max(pk, (size_t)c.ksplit * s.b * HW * op.cout * sizeof(float));
            // images of a whole number of 256 pixels, more than one: splitk_reduce_part leaves (S, Q, K, n) per (image, 256 pixels, channel)
            // (engine.hip:589-593, kernels.h:528)
            if (HW % 256 == 0 && HW > 256) part = std::max(part, (size_t)s.b * (HW / 256) * op.cout * 4 * sizeof(float));
        } else if (c.fused_stats && (op.type == OP_CONV || op.type == OP_PROJ)) {
            // (S, Q, K, n) per (image, tile lane, channel): written at ((n tpi + tile) Cout + c) * 4 (kernels.h:373), read as n * ntiles * C f32x4 with
            // ntiles = tiles_x tiles_y ppt (engine.hip:596, kernels.h:390)
            part = std::max(part, (size_t)s.b * c.g.tiles_x * c.g.tiles_y * c.ppt * op.cout * 4 * sizeof(float));
        }
        if (writes_dst(e, plan, i) && at[op.dst].in_up) up = std::max(up, bytes_of(e, op.dst, s));
    }
    side.push_back({"part", L.o_part, part});
    side.push_back({"partial", L.o_pk, pk});
    if (L.has_up) side.push_back({"up", L.o_up, up});
    std::sort(side.begin(), side.end(), [](const Region& a, const Region& b) { return a.off < b.off; });
    size_t arena_end = kWsHeader;
    for (size_t t = 0; t < nt; ++t) {
        if (wrote[t] == -2 || !at[t].ok || at[t].in_up) continue;
        if (at[t].off % 256) g_rep.viol("W3", fmt("tensor %s at %zu is not 256-byte aligned", e->tensors[t].name.c_str(), at[t].off));
        if (at[t].off < kWsHeader) g_rep.viol("W3", fmt("tensor %s at %zu lies on the header", e->tensors[t].name.c_str(), at[t].off));      // (engine.hip:713: the token)
        arena_end = std::max(arena_end, at[t].off + bytes_of(e, (int)t, s));
    }
    if (!side.empty() && arena_end > side[0].off) g_rep.viol("W3", fmt("the activations end at %zu, behind the start of %s at %zu", arena_end, side[0].name.c_str(), side[0].off));
    for (size_t k = 0; k < side.size(); ++k) {
        if (side[k].off % 256) g_rep.viol("W3", fmt("%s at %zu is not 256-byte aligned", side[k].name.c_str(), side[k].off));
        const size_t end = k + 1 < side.size() ? side[k + 1].off : L.bytes;
        if (side[k].off + side[k].need > end)
            g_rep.viol("W3", fmt("%s needs [%zu, +%zu) and %s begins at %zu", side[k].name.c_str(), side[k].off, side[k].need, k + 1 < side.size() ? side[k + 1].name.c_str() : "the end", end));
    }
}

// W4: the tile geometry of one plan
struct KernTile { int th, tw; };      // the fixed tile a kernel walks (0: none)
KernTile fixed_tile(const Choice& c) {
    switch (c.k) {
    case K_S1_RES32: case K_S1_RES32F: case K_UP0: return {8, 32};                           // kernels_res32.h:48 (patch 10 x 34), kernels_up0.h:62
    case K_UPC: case K_UPC_H: case K_S2_V2: return c.flex ? KernTile{0, 0} : KernTile{8, 32};      // kernels_upc.h:57, kernels_s2v2.h:80
    case K_UPQ: case K_UPC_H2: case K_S1_H2: case K_S1_QP: return {16, 32};                  // kernels_upq.h:29-30 (patches 10 x 18, 18 x 34), kernels_f16x3_qp.h:38 (18 rows)
    default: return {0, 0};
    }
}
// patch pixels the staging loop of the kernel reaches (0: not a staged-patch kernel of the tile_geom family)
int staging_capacity(const ts2d_engine* e, const Op& op, const Choice& c) {
    (void)e;
    switch (c.k) {
    case K_EXACT: {      // MAXIT = ceil(MAXP * QPP / 256) iterations of 256 threads, QPP = CK / 4 quads per pixel (kernels.h:132-133, 190-201); MAXP = 576 at
                         // stride (1, 1) - the transposed conv is launched with SY = SX = 1, engine.hip:426 - else 1296
        const int maxp = (op.type == OP_CONVT || (op.sy == 1 && op.sx == 1)) ? 576 : 1296, qpp = op.ck / 4;
        return (maxp * qpp + kBlock - 1) / kBlock * kBlock / qpp;
    }
    case K_S1_GENERIC: return 5 * kBlock / 2;      // MAXU = 3 or 5 units per thread, two units per pixel (engine.hip:448-450, kernels_f16x3.h:294-298)
    case K_S1_ONE: return 3 * kBlock / 2;          // MAXU = 3, two units per pixel (kernels_f16x3_one.h:103, 134-138)
    case K_S1_H32: return 6 * kBlock / 4;          // MAXU = 6, four units per pixel (engine.hip:439, kernels_h32.h:78-82)
    case K_S2_ONE: return 5 * kBlock;              // MAXU = 5, one unit per pixel (kernels_f16x3_one.h:268, 297-300)
    case K_S2_GENERIC: return 6 * kBlock;          // MAXU = 5 or 6 (engine.hip:453-455, kernels_f16x3.h:550-553)
    case K_T_ONE: case K_T_GENERIC: return kBlock; // four units per thread, four units per pixel (kernels_f16x3_convt.h:38, 213)
    default: return 0;
    }
}
bool geom_family(Kern k) { return k == K_EXACT || k == K_S1_GENERIC || k == K_S1_ONE || k == K_S1_H32 || k == K_S2_ONE || k == K_S2_GENERIC || k == K_T_ONE || k == K_T_GENERIC; }
bool one_image(Kern k) { return k == K_S1_ONE || k == K_S1_H32 || k == K_S2_ONE || k == K_T_ONE; }

void check_tiles(const ts2d_engine* e, const std::vector<Choice>& plan, const Shape& s) {
    for (size_t i = 0; i < e->ops.size(); ++i) {
        const Op& op = e->ops[i]; const Choice& c = plan[i]; const TileGeom& g = c.g;
        const bool first = c.k == K_FIRST || c.k == K_FIRST_STATS;
        if (!(geom_family(c.k) || fixed_tile(c).th || c.flex || first)) continue;
        const Tensor& src = e->tensors[op.src];
        // the pixels the kernel tiles: a conv's output, a transposed conv's INPUT (engine.hip:502-503)
        const int Ht = op.type == OP_CONVT ? s.H >> src.ly : s.H >> op.ly, Wt = op.type == OP_CONVT ? s.W >> src.lx : s.W >> op.lx;
        const char* nm = op.name.c_str();
        auto bad = [&](const std::string& m) { g_rep.viol("W4", fmt("op %s (%s) tile %d x %d x %d on %d x %d: %s", nm, c.name, g.NIMG, g.TH, g.TW, Ht, Wt, m.c_str())); };
        if (g.NIMG < 1 || g.TH < 1 || g.TW < 1) { bad("empty tile"); continue; }
        if ((long long)g.n_mtiles != (long long)((s.b + g.NIMG - 1) / g.NIMG) * g.tiles_x * g.tiles_y) bad(fmt("n_mtiles %d is not ceil(b / NIMG) * %d * %d", g.n_mtiles, g.tiles_x, g.tiles_y));
        if (g.NIMG == 1) { if ((long long)g.tiles_y * g.TH < Ht || (long long)g.tiles_x * g.TW < Wt) bad(fmt("%d x %d tiles do not cover the level", g.tiles_y, g.tiles_x)); }
        else if (first) {      // the first block's power-of-two slot may exceed its image: rows past it are masked (kernels_first.h:117, 205-207), the patch reads zeros (:103)
            if (g.TH < Ht || g.TW < Wt || g.tiles_x != 1 || g.tiles_y != 1) bad("several images per tile, and an image does not fit its slot");
        } else if (g.TH != Ht || g.TW != Wt || g.tiles_x != 1 || g.tiles_y != 1) bad("several images per tile, and the tile is not the image");
        if ((unsigned long long)g.n_mtiles * (unsigned)(g.tiles_x * g.tiles_y) >= 0x100000000ull) bad("tile number x tiles per image reaches 2^32 (udiv_magic, engine.hip:196-197)");
        const KernTile ft = fixed_tile(c);
        // the rows of the kernel's workgroup: 256 (tile_dims.h:8; kernels.h:345-350, m < 256); the 16 x 32 kernels bring 512 and walk that tile only
        if (!ft.th && g.NIMG * g.TH * g.TW > kBM) bad("more rows than a workgroup's 256");
        if (ft.th) {
            if (g.NIMG != 1 || g.TH != ft.th || g.TW != ft.tw) bad(fmt("the kernel walks %d x %d tiles", ft.th, ft.tw));
            if (Ht % ft.th || Wt % ft.tw) bad("the fixed tile does not divide the level");
            if ((c.k == K_UP0 || c.k == K_S1_RES32 || c.k == K_S1_RES32F) && (c.seg < 1 || g.n_mtiles % c.seg)) bad(fmt("segments of %d tiles do not divide %d (grid = n_tiles / seg, engine.hip:261, 327)", c.seg, g.n_mtiles));
        } else if (c.flex && (c.k == K_UPC || c.k == K_UPC_H)) {      // kernels_upc.h:36, 51-52
            if (g.TH % 2 || g.TW % 2) bad("FLEX composed tile with an odd side");
            if (g.TH * g.TW > 256) bad("FLEX composed tile above 256 pixels");
            if ((g.TH / 2 + 2) * (g.TW / 2 + 2) > 128) bad("FLEX coarse patch above 128 pixels");
            if ((g.TH + 2) * (g.TW + 2) > 384) bad("FLEX skip patch above 384 pixels");
        } else if (c.flex && c.k == K_S2_V2) {                        // kernels_s2v2.h:36, 51, 81
            if (Ht % g.TH || Wt % g.TW) bad("FLEX stride-2 tile does not divide the level");
            if (g.TW % 4) bad("FLEX stride-2 tile: TW % 4 != 0");
            if ((2 * g.TH + 1) * (2 * g.TW + 2) > 17 * 66) bad("FLEX stride-2 patch above 1122 slots");
        } else if (c.flex) bad("a FLEX instance of a kernel that has none");
        if (geom_family(c.k)) {
            const int taps = op.type == OP_CONVT ? 1 : 9, sy = op.type == OP_CONVT ? 1 : op.sy, sx = op.type == OP_CONVT ? 1 : op.sx, halo = taps == 9 ? 3 : 1;
            if (g.PH < (g.TH - 1) * sy + halo || g.PW < (g.TW - 1) * sx + halo) bad(fmt("patch %d x %d does not hold the tile's receptive field", g.PH, g.PW));
            const int cap = staging_capacity(e, op, c);
            if (g.PH * g.PW * g.NIMG > cap) bad(fmt("patch of %d pixels above the %d the kernel stages", g.PH * g.PW * g.NIMG, cap));
            if (one_image(c.k) && g.NIMG != 1) bad("a one-image kernel on a tile of several images");
            if (c.fused_stats && g.NIMG != 1) bad("tile partials on a tile of several images (kernels.h:363)");
        }
        if (first && c.first_full && (g.NIMG != 1 || g.TH * g.TW != 256 || s.H % g.TH || s.W % g.TW)) bad("persistent first block on incomplete tiles (engine.hip:222-223)");
    }
}

// W5: what of a Choice can change a row's bits
typedef std::tuple<int, int, int, int, int, int, bool, bool, bool, int, int, bool, bool, bool, bool> Bits;
Bits bits_of(const Choice& c) {
    return Bits(c.k, c.bn, c.ksplit, c.g.TH, c.g.TW, c.g.NIMG, c.flex, c.k32, c.s2p, c.ks, c.ppt, c.fused_stats, c.first_full, c.first_split, c.half);
}

// ------------------------------------------------------------------------------------------------------------------ the sweep
struct Sweep {
    std::string net, tag;
    std::unique_ptr<ts2d_engine> e;
    std::vector<int> modes, batches;
    std::vector<std::pair<int, int>> pairs;             // (Bw, b); empty: every b <= Bw of `batches`
    std::vector<std::pair<int, int>> extents;
};

int g_tamper = 0;
long long g_tampered = 0;

void run_sweep(Sweep& sw) {
    ts2d_engine* e = sw.e.get();
    static const char* kMode[3] = {"exact", "split", "f16"};
    std::vector<int> bs = sw.batches;
    for (auto& p : sw.pairs) { bs.push_back(p.first); bs.push_back(p.second); }
    std::sort(bs.begin(), bs.end()); bs.erase(std::unique(bs.begin(), bs.end()), bs.end());
    const int divy = 1 << e->lvl_y[e->arch.n_stages - 1], divx = 1 << e->lvl_x[e->arch.n_stages - 1];
    std::map<int, long long> n_layouts, n_pairs, n_refused;
    for (auto& hw : sw.extents) {
        const int H = hw.first, W = hw.second;
        if (H < divy || W < divx || H % divy || W % divx || (H / divy) * (W / divx) <= 1) { std::printf("skip %s %dx%d: not a shape reserve_checked admits\n", sw.net.c_str(), H, W); continue; }      // engine.hip:722-726
        std::map<size_t, std::tuple<int, int, int>> geom;      // op -> tile of the tile_geom family, over every mode and batch of this extent
        for (int mode : sw.modes) {
            e->precision = mode;
            if (!image_extent_ok(e, H, W)) { std::printf("skip %s %dx%d mode=%s: above the per-image limit of reserve_checked\n", sw.net.c_str(), H, W, kMode[mode]); continue; }
            std::map<std::pair<int, int>, WsLayout> layouts;
            std::map<std::pair<int, int>, std::vector<Choice>> plans;
            std::vector<int> ok_b;
            for (int b : bs) {
                if ((long long)b * H * W >= call_pixel_limit(e)) continue;                   // engine.hip: reserve_checked
                ok_b.push_back(b);
                for (int f = 0; f < 2; ++f) {
                    layouts[{b, f}] = workspace_layout(e, b, H, W, f != 0);
                    plans[{b, f}] = choose_all(e, b, H, W, f != 0);
                    ++n_layouts[mode];
                }
            }
            // ---- per plan: W4, the refusals, and the tiles of the tile_geom family across modes and batches
            for (int b : ok_b)
                for (int f = 0; f < 2; ++f) {
                    std::vector<Choice> plan = plans[{b, f}];
                    g_rep.where = fmt("%s mode=%s H=%d W=%d b=%d fr=%d %s", sw.net.c_str(), kMode[mode], H, W, b, f, sw.tag.c_str());
                    if (g_tamper == 5)                                                       // (e) a tile one row short of covering its level
                        for (size_t i = 0; i < plan.size(); ++i) {
                            Choice& c = plan[i];
                            if (geom_family(c.k) && c.g.NIMG == 1 && c.g.TH > 1 && e->ops[i].type == OP_CONV && c.g.tiles_y * c.g.TH == (H >> e->ops[i].ly)) { c.g.TH -= 1; ++g_tampered; break; }
                        }
                    check_tiles(e, plan, Shape{b, H, W});
                    for (size_t i = 0; i < plan.size(); ++i) {
                        if (!geom_family(plan[i].k)) continue;
                        const auto t = std::make_tuple(plan[i].g.TH, plan[i].g.TW, plan[i].g.NIMG);
                        auto it = geom.find(i);
                        if (it == geom.end()) geom[i] = t;
                        else if (it->second != t && g_tamper != 5)
                            g_rep.viol("W5", fmt("op %s: the tile_geom tile %d x %d x %d differs from %d x %d x %d of another mode or batch", e->ops[i].name.c_str(), plan[i].g.NIMG, plan[i].g.TH,
                                                 plan[i].g.TW, std::get<2>(it->second), std::get<0>(it->second), std::get<1>(it->second)));
                    }
                }
            // ---- W5: the full dispatch does not depend on the batch
            for (size_t k = 1; k < ok_b.size(); ++k) {
                std::vector<Choice> p0 = plans[{ok_b[0], 1}];
                const std::vector<Choice>& p1 = plans[{ok_b[k], 1}];
                if (g_tamper == 6 && ok_b[0] == 1)                                           // (f) one op's split factor doubled at b = 1 only
                    for (Choice& c : p0) if (geom_family(c.k)) { c.ksplit *= 2; ++g_tampered; break; }
                g_rep.where = fmt("%s mode=%s H=%d W=%d b=%d vs b=%d fr=1 %s", sw.net.c_str(), kMode[mode], H, W, ok_b[0], ok_b[k], sw.tag.c_str());
                for (size_t i = 0; i < p0.size(); ++i)
                    if (bits_of(p0[i]) != bits_of(p1[i]))
                        g_rep.viol("W5", fmt("op %s: %s S=%d tile %dx%dx%d against %s S=%d tile %dx%dx%d", e->ops[i].name.c_str(), p0[i].name, p0[i].ksplit, p0[i].g.NIMG, p0[i].g.TH, p0[i].g.TW,
                                             p1[i].name, p1[i].ksplit, p1[i].g.NIMG, p1[i].g.TH, p1[i].g.TW));
            }
            // ---- W1-W3 per admitted (layout, run) pair (ensure_workspace, engine.hip:69: wsB >= B, the same extent, mode and keep flag, ws_full || !full)
            auto pair_ok = [&](int Bw, int b) {
                if (b > Bw) return false;
                if (sw.pairs.empty()) return std::find(sw.batches.begin(), sw.batches.end(), Bw) != sw.batches.end() && std::find(sw.batches.begin(), sw.batches.end(), b) != sw.batches.end();
                return std::find(sw.pairs.begin(), sw.pairs.end(), std::make_pair(Bw, b)) != sw.pairs.end();
            };
            for (int Bw : ok_b)
                for (int b : ok_b) {
                    if (!pair_ok(Bw, b)) continue;
                    for (int fw = 0; fw < 2; ++fw)
                        for (int fr = 0; fr <= fw; ++fr) {
                            const std::vector<Choice>& plan = plans[{b, fr}];
                            g_rep.where = fmt("%s mode=%s H=%d W=%d Bw=%d fw=%d b=%d fr=%d %s", sw.net.c_str(), kMode[mode], H, W, Bw, fw, b, fr, sw.tag.c_str());
                            bool refused = false;
                            for (size_t i = 0; i < plan.size(); ++i) refused |= plan[i].k == K_NONE && refusal_expected(e, e->ops[i]);
                            if (refused) { ++n_refused[mode]; continue; }      // (the forward fails with the op's name, engine.hip:664-666)
                            ++n_pairs[mode];
                            if (!g_tamper || g_tamper >= 5) { check_pair(e, layouts[{Bw, fw}], plan, Shape{b, H, W}); continue; }
                            // ---- the damages (a)-(d): to a copy of the planner's DATA, then the same check
                            WsLayout L = layouts[{Bw, fw}];
                            const Shape s{b, H, W};
                            if (g_tamper == 1) {        // (a) the split-K region one 256-byte block shorter than its largest consumer needs
                                size_t pk = 0;
                                for (size_t i = 0; i < plan.size(); ++i) if (runs(plan[i]) && plan[i].ksplit > 1) pk = std::max(pk, (size_t)plan[i].ksplit * b * (H >> e->ops[i].ly) * (W >> e->ops[i].lx) * e->ops[i].cout * sizeof(float));
                                if (pk) { const size_t end = L.o_pk + align_up(pk, 256) - 256; if (L.has_up) L.o_up = end; else L.bytes = end; ++g_tampered; }
                            } else if (g_tamper == 2) { // (b) an output moved onto a tensor that is live at its write
                                for (size_t i = 0; i < plan.size(); ++i) {
                                    const std::vector<int> r = reads_of(e, plan, i);
                                    if (writes_dst(e, plan, i) && !r.empty() && L.plan.used[r[0]] && L.plan.used[e->ops[i].dst]) { L.plan.off[e->ops[i].dst] = L.plan.off[r[0]]; ++g_tampered; break; }
                                }
                            } else if (g_tamper == 3) { // (c) the scratch of an un-composed upsampled tensor gone
                                if (L.has_up) { L.has_up = false; ++g_tampered; }
                            } else if (g_tamper == 4) { // (d) a tensor's buffer one block short of what the run writes
                                for (size_t i = 0; i < plan.size(); ++i)
                                    if (writes_dst(e, plan, i) && L.plan.used[e->ops[i].dst]) { L.plan.size[e->ops[i].dst] = align_up(bytes_of(e, e->ops[i].dst, s), 256) - 256; ++g_tampered; break; }
                            }
                            check_pair(e, L, plan, s);
                        }
                }
        }
    }
    for (int mode : sw.modes)
        std::printf("count %s mode=%s %s extents=%zu layouts=%lld pairs=%lld refused=%lld\n", sw.net.c_str(), kMode[mode], sw.tag.c_str(), sw.extents.size(), n_layouts[mode], n_pairs[mode], n_refused[mode]);
}

// SPEC: whitespace-separated words.
//   net NAME RESIDUAL CIN K N_STAGES  features[n]  n_conv_enc[n]  n_conv_dec[n-1]  strides[n][2]  n_blocks[n] (RESIDUAL = 1 only)
//   tag WORD | set NAME VALUE ... end | modes M ... end | batches B ... end | pairs Bw b ... end | extents H W ... end | run | show MODE H W B FULL
int main_ws(const char* path) {
    std::ifstream f(path);
    if (!f) { std::fprintf(stderr, "cannot read %s\n", path); return 2; }
    Sweep sw;
    ts2d_arch_desc arch{}; int n_blocks[TS2D_MAX_STAGES] = {0}; bool residual = false;
    std::vector<std::pair<std::string, int>> opts;
    std::string w;
    auto ints = [&](std::vector<int>& v) { v.clear(); std::string t; while (f >> t && t != "end") v.push_back(std::atoi(t.c_str())); };
    while (f >> w) {
        if (w == "net") {
            int res = 0;
            arch = ts2d_arch_desc{}; std::memset(n_blocks, 0, sizeof(n_blocks));
            f >> sw.net >> res >> arch.input_channels >> arch.num_classes >> arch.n_stages;
            if (arch.n_stages < 2 || arch.n_stages > TS2D_MAX_STAGES) return 3;
            residual = res != 0;
            for (int s = 0; s < arch.n_stages; ++s) f >> arch.features[s];
            for (int s = 0; s < arch.n_stages; ++s) f >> arch.n_conv_enc[s];
            for (int s = 0; s < arch.n_stages - 1; ++s) f >> arch.n_conv_dec[s];
            for (int s = 0; s < arch.n_stages; ++s) f >> arch.strides[s][0] >> arch.strides[s][1];
            if (residual) for (int s = 0; s < arch.n_stages; ++s) f >> n_blocks[s];
            arch.norm_eps = 1e-5f; arch.leaky_slope = 0.01f;
            opts.clear(); sw.pairs.clear(); sw.tag = "default";
        } else if (w == "tag") { f >> sw.tag; }
        else if (w == "set") { opts.clear(); std::string k; while (f >> k && k != "end") { int v; f >> v; opts.push_back({k, v}); } }
        else if (w == "modes") ints(sw.modes);
        else if (w == "batches") ints(sw.batches);
        else if (w == "pairs") { std::vector<int> v; ints(v); sw.pairs.clear(); for (size_t i = 0; i + 1 < v.size(); i += 2) sw.pairs.push_back({v[i], v[i + 1]}); }
        else if (w == "extents") { std::vector<int> v; ints(v); sw.extents.clear(); for (size_t i = 0; i + 1 < v.size(); i += 2) sw.extents.push_back({v[i], v[i + 1]}); }
        else if (w == "run") {
            sw.e = make_engine(arch, residual ? n_blocks : nullptr);
            if (!sw.e) return 4;
            for (auto& o : opts) if (!set_option(sw.e.get(), o.first, o.second)) { std::fprintf(stderr, "unknown option %s\n", o.first.c_str()); return 5; }
            run_sweep(sw);
            sw.e.reset();
        } else if (w == "show") {      // show MODE H W B FULL: the plan of one run, op by op (to read a violation with)
            int mode, H, W, B, full;
            f >> mode >> H >> W >> B >> full;
            std::unique_ptr<ts2d_engine> e = make_engine(arch, residual ? n_blocks : nullptr);
            if (!e) return 4;
            for (auto& o : opts) set_option(e.get(), o.first, o.second);
            e->precision = mode;
            const std::vector<Choice> plan = choose_all(e.get(), B, H, W, full != 0);
            for (size_t i = 0; i < plan.size(); ++i)
                std::printf("show %s %s S=%d tile %dx%dx%d tiles %dx%d\n", e->ops[i].name.c_str(), plan[i].k == K_FUSED_AWAY ? "(composed away)" : plan[i].name, plan[i].ksplit,
                            plan[i].g.NIMG, plan[i].g.TH, plan[i].g.TW, plan[i].g.tiles_y, plan[i].g.tiles_x);
        } else if (w == "limit") {     // limit MODE H W: the per-image predicate of reserve_checked (engine.hip; program.cpp image_extent_ok) at one extent
            int mode, H, W;
            f >> mode >> H >> W;
            std::unique_ptr<ts2d_engine> e = make_engine(arch, residual ? n_blocks : nullptr);
            if (!e) return 4;
            for (auto& o : opts) set_option(e.get(), o.first, o.second);
            e->precision = mode;
            int t = -1;
            const long long bytes = image_plane_bytes(e.get(), H, W, &t);
            std::printf("limit %s mode=%d H=%d W=%d bytes=%lld widest=%s C=%d ok=%d call=%lld\n", sw.net.c_str(), mode, H, W, bytes, t >= 0 ? e->tensors[t].name.c_str() : "input",
                        t >= 0 ? e->tensors[t].C : e->arch.input_channels, (int)image_extent_ok(e.get(), H, W), call_pixel_limit(e.get()));
        } else if (w == "limits") {    // limits MODE: L1 - along W at many heights, the predicate flips once, exactly where the restated plane passes 2^31 - 1 bytes
            int mode;
            f >> mode;
            std::unique_ptr<ts2d_engine> e = make_engine(arch, residual ? n_blocks : nullptr);
            if (!e) return 4;
            e->precision = mode;
            const int divy = 1 << e->lvl_y[e->arch.n_stages - 1], divx = 1 << e->lvl_x[e->arch.n_stages - 1];
            // restated from the consumers, not asked of program.cpp: a record count (int)(pixels * C * sizeof(ST)) per activation tensor (kernels_f16x3.h:218
            // and its siblings), handed an op only under fits32(pixels * C * 4) in every mode (dispatch.cpp:165, 229-233, 271, 292, 320, 349);
            // (int)(C0 * H * W * 4) for the network input (kernels_res32.h:144-145, dispatch.cpp:195)
            auto plane = [&](long long H, long long W) {
                unsigned __int128 worst = (unsigned __int128)H * W * e->arch.input_channels * 4;
                for (const Tensor& x : e->tensors) worst = std::max(worst, (unsigned __int128)(H >> x.ly) * (W >> x.lx) * x.C * 4);
                return worst;
            };
            long long n = 0;
            for (long long H = divy; H <= (1LL << 30); H = H * 3 / 2 / divy * divy + divy) {
                g_rep.where = fmt("%s mode=%d H=%lld", sw.net.c_str(), mode, H);
                long long lo = 0, hi = ((1LL << 31) - 1) / H / divx + 1;      // in units of divx: ok(lo) (or lo = 0), not ok(hi) - there H * W reaches 2^31 pixels
                if (image_extent_ok(e.get(), (int)H, (int)std::min(hi * divx, (long long)INT32_MAX / divx * divx))) g_rep.viol("L1", "accepted at 2^31 pixels");
                while (hi - lo > 1) { const long long mid = (lo + hi) / 2; (image_extent_ok(e.get(), (int)H, (int)(mid * divx)) ? lo : hi) = mid; }
                for (long long k = std::max(1LL, lo - 3); k <= std::min(hi + 3, ((1LL << 31) - 1) / divx); ++k) {
                    const bool ok = image_extent_ok(e.get(), (int)H, (int)(k * divx)), want = (unsigned __int128)H * (k * divx) < ((unsigned __int128)1 << 31) && plane(H, k * divx) <= (unsigned __int128)kImagePlaneMax;
                    if (ok != want) g_rep.viol("L1", fmt("W=%lld: the predicate says %d, the restated plane %d", k * divx, (int)ok, (int)want));
                    ++n;
                }
                if (lo >= 1 && plane(H, lo * divx) > (unsigned __int128)kImagePlaneMax) g_rep.viol("L1", fmt("W=%lld accepted with a plane above the limit", lo * divx));
            }
            std::printf("limits %s mode=%d checked=%lld viol=%lld\n", sw.net.c_str(), mode, n, g_rep.n["L1"]);
        } else { std::fprintf(stderr, "unknown word %s\n", w.c_str()); return 6; }
    }
    std::printf("tally");
    for (const char* p : {"W1", "W2", "W3", "W4", "W5"}) std::printf(" %s=%lld", p, g_rep.n[p]);
    std::printf(" tampered=%lld\n", g_tampered);
    return 0;
}

}  // namespace

int main_tiled();

int main(int argc, char** argv) {
    for (int i = 1; i + 1 < argc; ++i) {
        if (!std::strcmp(argv[i], "--tamper")) g_tamper = std::atoi(argv[i + 1]);
        if (!std::strcmp(argv[i], "--show")) g_rep.show = std::atoll(argv[i + 1]);
    }
    if (argc >= 3 && !std::strcmp(argv[1], "ws")) return main_ws(argv[2]);
    if (argc >= 2 && !std::strcmp(argv[1], "tiled")) return main_tiled();
    std::fprintf(stderr, "usage: plan_driver ws SPEC [--tamper N] | plan_driver tiled [--tamper N]\n");
    return 2;
}


// ================================================================================================================== the sliding-window plan
namespace {

enum Kind { kNone, kExport, kLabelmap, kRegions, kProb, kProbRuns };
struct Rect { int src_y, src_x, src_h, src_w, out_h, out_w, full_h, full_w, box_y, box_x; uint8_t* u8; float* f32; };
struct Call {
    int kind = kNone, F = 1, ph = 32, pw = 32, mirror = 0, mode = 0;
    bool name_images = true;
    std::vector<ts2d_tiled_image> images;
    std::vector<Rect> rects;                                   // one per image (kProbRuns: one per RUN)
    std::vector<ts2d_tiled_probabilities_run> runs;
    std::vector<uint8_t> order;
};

SwTail tail_of(const Call& c) {
    const int n = (int)c.images.size();
    SwTail t((SwTail::Kind)c.kind, c.kind == kNone ? 0 : n);
    t.mode = c.mode;
    t.class_order = c.kind == kRegions || (c.kind >= kProb && c.mode == kProbRegions) ? c.order.data() : nullptr;
    auto image = [](const Rect& q) { return SwTail::Image{q.src_y, q.src_x, q.src_h, q.src_w, q.out_h, q.out_w, q.full_h, q.full_w, q.box_y, q.box_x, q.u8, q.f32}; };
    if (c.kind == kProbRuns) {
        t.runs = c.runs.data(); t.n_runs = (int)c.runs.size(); t.run_of.resize((size_t)n);
        for (size_t r = 0; r < c.runs.size(); ++r)
            for (int s = 0; s < c.runs[r].n_slices; ++s) { const size_t i = (size_t)c.runs[r].first_image + s; t.images[i] = image(c.rects[r]); t.run_of[i] = (int)r; }
        return t;
    }
    for (size_t i = 0; i < t.images.size(); ++i) t.images[i] = image(c.rects[i]);
    return t;
}

// ---- the scenarios of scripts/tiled_plan_record.py, restated: four image extents (Hp, Wp, tiles; the last has more rows than a chunk holds, the third a
// row pitch that is no multiple of 4), their rectangles (the second and the fourth un-resampled), and two more extents for a chunk that fills exactly
float g_px[8];
uint8_t g_u8[8];
std::vector<std::unique_ptr<std::vector<int32_t>>> g_tiles;      // (kept alive: the images point into them)
const int kExtents[6][3] = {{40, 32, 2}, {32, 48, 2}, {50, 70, 6}, {90, 100, 40}, {64, 64, 8}, {48, 36, 16}};
const int kRects[6][6] = {{4, 0, 30, 32, 45, 20}, {0, 8, 32, 33, 32, 33}, {1, 2, 48, 60, 17, 90}, {3, 5, 80, 90, 80, 90}, {0, 0, 64, 64, 100, 37}, {2, 4, 40, 32, 40, 32}};
ts2d_tiled_image image(int Hp, int Wp, int n_tiles, bool l16, bool seg, int ph, int pw) {
    g_tiles.emplace_back(new std::vector<int32_t>()); std::vector<int32_t>& ty = *g_tiles.back();
    g_tiles.emplace_back(new std::vector<int32_t>()); std::vector<int32_t>& tx = *g_tiles.back();
    for (int t = 0; t < n_tiles; ++t) { ty.push_back((t * 7) % (Hp - ph + 1 > 0 ? Hp - ph + 1 : 1)); tx.push_back((t * 5) % (Wp - pw + 1 > 0 ? Wp - pw + 1 : 1)); }
    return ts2d_tiled_image{g_px, Hp, Wp, n_tiles, ty.data(), tx.data(), l16 ? reinterpret_cast<uint16_t*>(g_px) : nullptr, seg ? g_u8 : nullptr, 0};
}
Rect rect(int i, bool u8, bool f32) {
    const int* q = kRects[i];
    return Rect{q[0], q[1], q[2], q[3], q[4], q[5], q[4] + 7 + i, q[5] + 3, 2 + i, 1, u8 ? g_u8 : nullptr, f32 ? g_px : nullptr};
}
// a / b: the kind's two outputs - export: uint8 / float; label map and regions: the plane / -; probabilities: the decided map / the planes
Call make(int kind, const std::vector<int>& idx, bool a, bool b, int mode = 0, bool padded = false, int ph = 32, int pw = 32) {
    Call c;
    c.kind = kind; c.mode = mode; c.order = {3, 1, 2}; c.ph = ph; c.pw = pw;
    for (int i : idx) {
        c.images.push_back(image(kExtents[i][0], kExtents[i][1], kExtents[i][2], kind == kNone || padded, padded, ph, pw));
        if (kind != kNone && kind != kProbRuns) c.rects.push_back(rect(i, a, b));
    }
    return c;
}
Call make_runs(const std::vector<int>& slices, int ext, bool dec, int mode) {       // runs of `slices` images, all of extent `ext`
    Call c;
    c.kind = kProbRuns; c.mode = mode; c.order = {3, 1, 2};
    int first = 0;
    for (size_t r = 0; r < slices.size(); ++r) {
        for (int s = 0; s < slices[r]; ++s) c.images.push_back(image(kExtents[ext][0], kExtents[ext][1], kExtents[ext][2], false, false, 32, 32));
        const Rect q = rect(ext, dec, true);
        c.rects.push_back(q);
        const long long plane = (long long)q.full_h * q.full_w * slices[r];
        c.runs.push_back(ts2d_tiled_probabilities_run{q.src_y, q.src_x, q.src_h, q.src_w, q.out_h, q.out_w, q.full_h, q.full_w, q.box_y, q.box_x, first, slices[r],
                                                      q.f32, plane + 11, q.u8, plane});
        first += slices[r];
    }
    return c;
}

struct TReport {
    std::map<std::string, long long> n;
    std::string where;
    void viol(const char* prop, const std::string& msg) { if (n[prop]++ < g_rep.show) std::printf("viol %s %s :: %s\n", prop, where.c_str(), msg.c_str()); }
} g_t;
long long g_plans = 0, g_refused = 0, g_lanes = 0, g_replayed = 0;
std::map<std::tuple<int, int, int>, bool> g_taps_printed;

long long blocks(long long lanes) { return (lanes + 255) / 256; }      // 256 lanes per block (kernels_sw.h:40, 45)

// the owner of a block as the kernels find it (kernels_sw.h:27-35, kernels_resample.h:27-36), on any list of first blocks
int find_owner(const std::vector<unsigned>& first, unsigned blk) {
    int lo = 0, hi = (int)first.size() - 1;
    while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (first[mid] <= blk) lo = mid; else hi = mid - 1; }
    return lo;
}

struct Span { const char* name; size_t off, need; };

void check_plan(const ts2d_engine* e, const Call& c, const SwTail& tail, SwPlan& pl) {
    const int C = e->arch.input_channels, K = e->arch.num_classes, V = pl.V, F = c.F, ph = c.ph, pw = c.pw;
    const int n_images = (int)c.images.size();
    const size_t plane = (size_t)ph * pw;
    // ---------------------------------------------------------------------------------------------------------------- T2: rows
    if (V != ((c.mirror & 3) == 3 ? 4 : (c.mirror & 3) ? 2 : 1)) g_t.viol("T2", fmt("V = %d for mirror mask %d", V, c.mirror));
    if (pl.cap_rows > kSwChunkRows) g_t.viol("T2", fmt("cap_rows %d above kSwChunkRows", pl.cap_rows));
    std::vector<int> next_row(n_images, 0), last_chunk(n_images, -1), agg_chunk(n_images, -1);
    size_t seg_i = 0;
    size_t log_need_rows = 0;
    for (size_t ci = 0; ci < pl.chunks.size(); ++ci) {
        const SwChunk& ck = pl.chunks[ci];
        if (ck.seg0 != (int)seg_i || ck.n_segs < 1 || seg_i + ck.n_segs > pl.segs.size()) { g_t.viol("T2", fmt("chunk %zu: segments [%d, +%d) do not follow %zu", ci, ck.seg0, ck.n_segs, seg_i)); return; }
        if (ck.rows < 1 || ck.rows > pl.cap_rows) g_t.viol("T2", fmt("chunk %zu: %d rows, cap_rows %d", ci, ck.rows, pl.cap_rows));
        unsigned g0 = 0, a0 = 0; int rows = 0;
        std::vector<unsigned> gfirst, afirst;
        for (int j = 0; j < ck.n_segs; ++j) {
            const SwSeg& sg = pl.segs[seg_i + j];
            const int im = sg.image;
            if (im < 0 || im >= n_images) { g_t.viol("T2", fmt("segment %zu names image %d", seg_i + j, im)); return; }
            if (sg.Hp != c.images[im].Hp || sg.Wp != c.images[im].Wp || sg.n_tiles != c.images[im].n_tiles) g_t.viol("T2", fmt("segment %zu is not image %d", seg_i + j, im));
            if (sg.row0 != next_row[im] || sg.n_rows < 1) g_t.viol("T2", fmt("image %d: rows [%d, +%d) where row %d is next", im, sg.row0, sg.n_rows, next_row[im]));
            next_row[im] = sg.row0 + sg.n_rows;
            if (sg.batch_row != rows) g_t.viol("T2", fmt("segment %zu: batch_row %d, %d rows before it", seg_i + j, sg.batch_row, rows));
            if (sg.batch_row + sg.n_rows > pl.cap_rows) g_t.viol("T2", fmt("segment %zu: rows [%d, +%d) leave the batch of %d", seg_i + j, sg.batch_row, sg.n_rows, pl.cap_rows));
            rows += sg.n_rows;
            // the network writes row r of the chunk to logit row ck.log_row + r (tiled.hip:134); the aggregate reads tile t, variant v of the image at
            // sg.log_row + t V + v (kernels_sw.h:114, 120): the image's row 0 must be where the chunk put it
            if (ck.log_row + sg.batch_row - sg.row0 != sg.log_row) g_t.viol("T2", fmt("segment %zu: log_row %d, the chunk writes its row 0 to %d", seg_i + j, sg.log_row, ck.log_row + sg.batch_row - sg.row0));
            if (sg.gblock0 != g0 || sg.ablock0 != a0) g_t.viol("T2", fmt("segment %zu: first blocks %u / %u, prefix sums %u / %u", seg_i + j, sg.gblock0, sg.ablock0, g0, a0));
            gfirst.push_back(sg.gblock0); afirst.push_back(sg.ablock0);
            g0 += (unsigned)blocks((long long)sg.n_rows * C * ph * ((pw + 3) / 4));                  // kernels_sw.h:44-46
            a0 += (unsigned)blocks((long long)K * sg.Hp * ((sg.Wp + 3) / 4));                        // kernels_sw.h:93-94
            last_chunk[im] = (int)ci;
            if (ck.aggregate) { if (agg_chunk[im] >= 0) g_t.viol("T2", fmt("image %d is aggregated twice", im)); agg_chunk[im] = (int)ci; }
        }
        if (rows != ck.rows) g_t.viol("T2", fmt("chunk %zu: %d rows, its segments hold %d", ci, ck.rows, rows));
        if (ck.gblocks != g0 || ck.ablocks != a0) g_t.viol("T2", fmt("chunk %zu: %u / %u blocks, its segments need %u / %u", ci, ck.gblocks, ck.ablocks, g0, a0));
        for (size_t j = 1; j < gfirst.size(); ++j) if (gfirst[j] <= gfirst[j - 1] || afirst[j] <= afirst[j - 1]) g_t.viol("T2", fmt("chunk %zu: first blocks do not increase", ci));
        // the search of the kernels finds the owner of every block
        if (g0 + a0 < 200000) {
            for (unsigned b = 0; b < g0; ++b) { const int o = find_owner(gfirst, b); const unsigned end = o + 1 < (int)gfirst.size() ? gfirst[o + 1] : g0; if (b < gfirst[o] || b >= end) g_t.viol("T2", fmt("chunk %zu: gather block %u lands in segment %d", ci, b, o)); }
            for (unsigned b = 0; b < a0; ++b) { const int o = find_owner(afirst, b); const unsigned end = o + 1 < (int)afirst.size() ? afirst[o + 1] : a0; if (b < afirst[o] || b >= end) g_t.viol("T2", fmt("chunk %zu: aggregate block %u lands in segment %d", ci, b, o)); }
        }
        log_need_rows = std::max(log_need_rows, (size_t)ck.log_row + ck.rows);
        seg_i += ck.n_segs;
    }
    if (seg_i != pl.segs.size()) g_t.viol("T2", fmt("%zu segments, the chunks hold %zu", pl.segs.size(), seg_i));
    for (int i = 0; i < n_images; ++i) {
        if (next_row[i] != c.images[i].n_tiles * V) g_t.viol("T2", fmt("image %d: %d of its %d rows are in chunks", i, next_row[i], c.images[i].n_tiles * V));
        if (agg_chunk[i] != last_chunk[i]) g_t.viol("T2", fmt("image %d: aggregated in chunk %d, its last rows are in chunk %d", i, agg_chunk[i], last_chunk[i]));
        log_need_rows = std::max(log_need_rows, (size_t)c.images[i].n_tiles * V);
    }
    // ---------------------------------------------------------------------------------------------------------------- T1: layout
    size_t img_end = 0, out_end = 0;
    {
        std::vector<std::pair<long long, long long>> imgs, outs;
        for (const SwSeg& sg : pl.segs) {
            imgs.push_back({sg.img_off, sg.img_off + (long long)C * sg.Hp * sg.Wp}); outs.push_back({sg.out_off, sg.out_off + (long long)K * sg.Hp * sg.Wp});
            if (sg.img_off % 4 || sg.out_off % 8) g_t.viol("T1", fmt("image %d: img_off %lld / out_off %lld not a multiple of 4 / 8", sg.image, sg.img_off, sg.out_off));
            img_end = std::max(img_end, (size_t)imgs.back().second); out_end = std::max(out_end, (size_t)outs.back().second);
        }
        for (size_t a = 0; a < pl.segs.size(); ++a)
            for (size_t b = a + 1; b < pl.segs.size(); ++b) {
                if (pl.segs[a].image == pl.segs[b].image) { if (imgs[a] != imgs[b] || outs[a] != outs[b]) g_t.viol("T1", fmt("image %d has two places", pl.segs[a].image)); continue; }
                if (imgs[a].first < imgs[b].second && imgs[b].first < imgs[a].second) g_t.viol("T1", fmt("images %d and %d share input floats", pl.segs[a].image, pl.segs[b].image));
                if (outs[a].first < outs[b].second && outs[b].first < outs[a].second) g_t.viol("T3", fmt("images %d and %d share output elements", pl.segs[a].image, pl.segs[b].image));
            }
        // the host copies image i to the running sum of align_up(C Hp Wp, 64) floats and reads its outputs at that of align_up(K Hp Wp, 256) (tiled.hip:122-127, 157-163)
        long long io = 0, oo = 0;
        for (int i = 0; i < n_images; ++i) {
            for (const SwSeg& sg : pl.segs) if (sg.image == i && (sg.img_off != io || sg.out_off != oo)) g_t.viol("T1", fmt("image %d: planned at %lld / %lld, copied at %lld / %lld", i, sg.img_off, sg.out_off, io, oo));
            io += (long long)align_up((size_t)C * c.images[i].Hp * c.images[i].Wp, 64); oo += (long long)align_up((size_t)K * c.images[i].Hp * c.images[i].Wp, 256);
        }
        if ((size_t)pl.out_elems < out_end) g_t.viol("T1", fmt("out_elems %lld, the last image ends at %zu", pl.out_elems, out_end));
    }
    size_t rs8 = 0, rs32 = 0, prob = 0;       // elements the tail kernels write (below, T4)
    // ---------------------------------------------------------------------------------------------------------------- T4: the tail
    const RsTap* taps = reinterpret_cast<const RsTap*>(pl.tab.data() + pl.tab_rtaps);
    const size_t n_taps = (pl.tab_order - pl.tab_rtaps) / sizeof(RsTap);
    if (tail.kind != SwTail::kNone) {
        if ((int)pl.rsegs.size() != n_images) g_t.viol("T4", fmt("%zu tail segments for %d images", pl.rsegs.size(), n_images));
        unsigned b0 = 0;
        std::vector<std::pair<long long, long long>> dst, pdst, ddst;
        const int D = tail.mode == kProbMultilabel ? K : 1;
        for (size_t i = 0; i < pl.rsegs.size() && (int)i < n_images; ++i) {
            const RsSeg& rs = pl.rsegs[i]; const SwTail::Image& ex = tail.images[i];
            if (rs.block0 != b0) g_t.viol("T4", fmt("image %zu: block0 %u, prefix sum %u", i, rs.block0, b0));
            if (rs.Hp != c.images[i].Hp || rs.Wp != c.images[i].Wp || rs.out_h != ex.out_h || rs.out_w != ex.out_w) g_t.viol("T4", fmt("image %zu: the segment is not the image's", i));
            const bool untapped = tail.kind != SwTail::kExport && ex.out_h == ex.src_h && ex.out_w == ex.src_w;
            if ((rs.tap0 == -1) != untapped) g_t.viol("T4", fmt("image %zu: tap0 %d, un-resampled %d", i, rs.tap0, (int)untapped));
            long long src0 = -1;
            for (const SwSeg& sg : pl.segs) if (sg.image == (int)i) src0 = sg.out_off;
            if (untapped) {      // src_off points at the rectangle's first sample (kernels_labelmap.h:45, kernels_prob.h q.ident)
                if (rs.src_off != src0 + (long long)ex.src_y * rs.Wp + ex.src_x) g_t.viol("T4", fmt("image %zu: src_off %lld is not its rectangle's first sample", i, rs.src_off));
            } else {
                if (rs.src_off != src0) g_t.viol("T4", fmt("image %zu: src_off %lld, its half planes are at %lld", i, rs.src_off, src0));
                if (rs.tap0 < 0 || (size_t)rs.tap0 + ex.out_h + ex.out_w > n_taps) { g_t.viol("T4", fmt("image %zu: taps [%d, +%d) leave the table of %zu", i, rs.tap0, ex.out_h + ex.out_w, n_taps)); continue; }
                for (int ax = 0; ax < 2; ++ax) {
                    const int n_in = ax ? ex.src_w : ex.src_h, n_out = ax ? ex.out_w : ex.out_h, origin = ax ? ex.src_x : ex.src_y;
                    const RsTap* t = taps + rs.tap0 + (ax ? ex.out_h : 0);
                    for (int o = 0; o < n_out; ++o) {
                        RsTap tp; std::memcpy(&tp, t + o, sizeof(tp));
                        if (tp.i0 < origin || tp.i0 >= origin + n_in || tp.i1 < origin || tp.i1 >= origin + n_in) g_t.viol("T4", fmt("image %zu axis %d tap %d: indices %d, %d leave [%d, +%d)", i, ax, o, tp.i0, tp.i1, origin, n_in));
                        if (tp.w0 + tp.w1 != 1.0) g_t.viol("T4", fmt("image %zu axis %d tap %d: weights %a + %a", i, ax, o, tp.w0, tp.w1));
                        // the coordinate is not clamped: below the first sample it is negative and floor() leaves w1 in [0, 1) all the same
                        if (!(tp.w1 >= 0.0 && tp.w1 < 1.0)) g_t.viol("T4", fmt("image %zu axis %d tap %d: w1 = %a", i, ax, o, tp.w1));
                    }
                    if (!g_taps_printed[std::make_tuple(n_in, n_out, origin)]) {       // for the bit-for-bit comparison with preprocess.linear_axis_taps
                        g_taps_printed[std::make_tuple(n_in, n_out, origin)] = true;
                        std::printf("taps %d %d %d", n_in, n_out, origin);
                        for (int o = 0; o < n_out; ++o) {
                            RsTap tp; std::memcpy(&tp, t + o, sizeof(tp));
                            uint64_t a, b; std::memcpy(&a, &tp.w0, 8); std::memcpy(&b, &tp.w1, 8);
                            std::printf(" %016" PRIx64 " %016" PRIx64 " %d %d", a, b, tp.i0, tp.i1);
                        }
                        std::printf("\n");
                    }
                }
            }
            if (tail.prob()) {
                b0 += (unsigned)blocks((long long)ex.full_h * ((ex.full_w + 3) / 4));             // kernels_prob.h:104-106
                long long po, d_o, ps, ds;
                int fh, fw;
                if (tail.kind == SwTail::kProbRuns) { const ProbStackSeg& q = pl.pssegs[i]; po = q.prob_off; d_o = q.dec_off; ps = q.prob_stride; ds = q.dec_stride; fh = q.full_h; fw = q.full_w; }
                else { const ProbSeg& q = pl.psegs[i]; po = q.prob_off; d_o = q.dec_off; fh = q.full_h; fw = q.full_w; ps = ds = (long long)fh * fw; }
                if (fh != ex.full_h || fw != ex.full_w) g_t.viol("T4", fmt("image %zu: full extent %d x %d, the descriptor says %d x %d", i, fh, fw, ex.full_h, ex.full_w));
                for (int k = 0; k < K; ++k) pdst.push_back({po + k * ps, po + k * ps + (long long)fh * fw});       // head k at prob_off + k * prob_stride (kernels_prob.h:95, 113)
                for (int k = 0; k < D; ++k) ddst.push_back({d_o + k * ds, d_o + k * ds + (long long)fh * fw});
                if ((fw & 3) == 0 && (po % 4 || d_o % 4 || ps % 4 || ds % 4)) g_t.viol("T4", fmt("image %zu: vector stores at offsets that are no multiples of 4", i));      // kernels_prob.h:110
            } else {
                const int planes = tail.kind == SwTail::kExport ? K : 1;
                b0 += (unsigned)blocks((long long)planes * ex.out_h * ((ex.out_w + 3) / 4));      // kernels_resample.h:45-47, kernels_labelmap.h:33-35
                dst.push_back({rs.dst_off, rs.dst_off + (long long)planes * ex.out_h * ex.out_w});
                if ((ex.out_w & 3) == 0 && rs.dst_off % 4) g_t.viol("T4", fmt("image %zu: dst_off %lld is no multiple of 4", i, rs.dst_off));      // kernels_resample.h:66-72
            }
        }
        if ((long long)b0 != pl.rs_blocks) g_t.viol("T4", fmt("rs_blocks %lld, the segments need %u", pl.rs_blocks, b0));
        auto disjoint = [&](std::vector<std::pair<long long, long long>>& v, const char* what, size_t* end) {
            std::sort(v.begin(), v.end());
            for (size_t k = 0; k < v.size(); ++k) {
                if (v[k].first < 0) g_t.viol("T4", fmt("%s: a negative place", what));
                if (k && v[k].first < v[k - 1].second) g_t.viol("T4", fmt("%s: places [%lld, %lld) and [%lld, %lld) overlap", what, v[k - 1].first, v[k - 1].second, v[k].first, v[k].second));
                *end = std::max(*end, (size_t)v[k].second);
            }
        };
        size_t dst_end = 0, dec_end = 0;
        disjoint(dst, "resampled outputs", &dst_end); disjoint(pdst, "probabilities", &prob); disjoint(ddst, "decided maps", &dec_end);
        if (tail.prob()) { rs8 = pl.any_rs8 ? dec_end : 0; if ((size_t)pl.prob_elems < prob) g_t.viol("T4", fmt("prob_elems %lld, the last place ends at %zu", pl.prob_elems, prob)); }
        else { rs8 = pl.any_rs8 ? dst_end : 0; rs32 = pl.any_rs32 ? dst_end : 0; }
    }
    // ---------------------------------------------------------------------------------------------------------------- T1: the regions
    {
        const Span spans[] = {
            {"tab", pl.o_tab, pl.tab.size()},                                                      // tiled.hip:118
            {"gaussian", pl.o_g, plane * 2},                                                       // tiled.hip:119
            {"images", pl.o_imgs, img_end * 4},                                                    // tiled.hip:123-127
            {"batch", pl.o_batch, (size_t)pl.cap_rows * C * plane * 4},                            // tiled.hip:101, 132, 134 (the fold reserves cap_rows)
            {"logits", pl.o_log, log_need_rows * K * plane * 4},                                   // tiled.hip:134; kernels_sw.h:114
            {"half outputs", pl.o_o16, pl.any16 ? ((size_t)(F - 1) * pl.out_elems + out_end) * 2 : 0},      // tiled.hip:138 (fold f at f * out_elems)
            {"uint8 outputs", pl.o_seg, pl.anyseg ? out_end : 0},                                  // tiled.hip:115, 138
            {"flags", pl.o_flag, (size_t)F * n_images * 4},                                        // tiled.hip:120
            {"resampled uint8", pl.o_rs8, rs8}, {"resampled float", pl.o_rs32, rs32 * 4}, {"probabilities", pl.o_prob, prob * 4}};      // tiled.hip:151-152
        const size_t ns = sizeof(spans) / sizeof(spans[0]);
        for (size_t k = 0; k < ns; ++k) {
            if (spans[k].off % 256) g_t.viol("T1", fmt("%s at %zu is not 256-byte aligned", spans[k].name, spans[k].off));
            const size_t end = k + 1 < ns ? spans[k + 1].off : pl.bytes;
            if (spans[k].off + spans[k].need > end) g_t.viol("T1", fmt("%s needs [%zu, +%zu), the next region begins at %zu", spans[k].name, spans[k].off, spans[k].need, end));
        }
        for (const SwChunk& ck : pl.chunks) if (ck.rows > pl.cap_rows) g_t.viol("T1", fmt("a chunk of %d rows in a batch of %d", ck.rows, pl.cap_rows));
        // the table: [segments | tile_y | tile_x | tail segments | taps | class order | probabilities segments]
        const size_t nt = (size_t)pl.n_tiles_all;
        const bool regions = tail.class_order != nullptr;
        if (pl.tab_segs != pl.segs.size() * sizeof(SwSeg)) g_t.viol("T1", "tab_segs is not the segments' bytes");      // tiled.hip:112 (tile_y begins there)
        if (pl.tab_rsegs < pl.tab_segs + 2 * nt * 4 || pl.tab_rsegs % 8) g_t.viol("T1", "tab_rsegs lies on the tile origins or is not 8-byte aligned");
        if (pl.tab_rtaps < pl.tab_rsegs + pl.rsegs.size() * sizeof(RsSeg) || pl.tab_rtaps % 8) g_t.viol("T1", "tab_rtaps lies on the tail segments or is not 8-byte aligned");
        if (pl.tab_order < pl.tab_rtaps) g_t.viol("T1", "tab_order in front of the taps");
        if (tail.prob() && (pl.tab_psegs < pl.tab_order + (regions ? (size_t)K : 0) || pl.tab_psegs % 8)) g_t.viol("T1", "tab_psegs lies on the class order or is not 8-byte aligned");
        const size_t tab_end = tail.prob() ? pl.tab_psegs + (tail.kind == SwTail::kProbRuns ? pl.pssegs.size() * sizeof(ProbStackSeg) : pl.psegs.size() * sizeof(ProbSeg))
                                           : pl.tab_order + (regions ? (size_t)K : 0);
        if (tab_end > pl.tab.size()) g_t.viol("T1", fmt("the table holds %zu bytes, its parts end at %zu", pl.tab.size(), tab_end));
        const int32_t* ty = reinterpret_cast<const int32_t*>(pl.tab.data() + pl.tab_segs);
        size_t t0 = 0;
        for (int i = 0; i < n_images && tab_end <= pl.tab.size(); ++i) {
            for (const SwSeg& sg : pl.segs) if (sg.image == i && sg.tile0 != (int)t0) g_t.viol("T1", fmt("image %d: tile0 %d, %zu tiles before it", i, sg.tile0, t0));
            if (std::memcmp(ty + t0, c.images[i].tile_y, (size_t)c.images[i].n_tiles * 4) || std::memcmp(ty + nt + t0, c.images[i].tile_x, (size_t)c.images[i].n_tiles * 4))
                g_t.viol("T1", fmt("image %d: the table does not hold its tile origins", i));
            t0 += c.images[i].n_tiles;
        }
    }
    // ---------------------------------------------------------------------------------------------------------------- T3: addressing replay
    long long lanes = 0;
    for (const SwChunk& ck : pl.chunks) lanes += ((long long)ck.gblocks + (ck.aggregate ? ck.ablocks : 0)) * 256;
    g_lanes += lanes;
    if (lanes > 400000 || g_t.n["T1"] || g_t.n["T2"]) return;
    ++g_replayed;
    const int32_t* tys = reinterpret_cast<const int32_t*>(pl.tab.data() + pl.tab_segs); const int32_t* txs = tys + pl.n_tiles_all;
    const int pwq = (pw + 3) >> 2;
    std::vector<uint8_t> out_written(out_end, 0);
    for (const SwChunk& ck : pl.chunks) {
        std::vector<unsigned> gfirst, afirst;
        for (int j = 0; j < ck.n_segs; ++j) { gfirst.push_back(pl.segs[ck.seg0 + j].gblock0); afirst.push_back(pl.segs[ck.seg0 + j].ablock0); }
        // ---- sw_gather (kernels_sw.h:40-66)
        std::vector<uint8_t> bw((size_t)ck.rows * C * plane, 0);
        for (unsigned blk = 0; blk < ck.gblocks; ++blk) {
            const SwSeg& sg = pl.segs[ck.seg0 + find_owner(gfirst, blk)];
            for (int tid = 0; tid < 256; ++tid) {
                const long long q = (long long)(blk - sg.gblock0) * 256 + tid;
                if (q >= (long long)sg.n_rows * C * ph * pwq) continue;
                const int x0 = (int)(q % pwq) * 4; long long r = q / pwq;
                const int y = (int)(r % ph); r /= ph;
                const int ch = (int)(r % C); const int lrow = (int)(r / C);
                const int row = sg.row0 + lrow, t = row / V, f = (pl.vflips >> (8 * (row % V))) & 3;
                if (t >= sg.n_tiles) { g_t.viol("T3", fmt("gather: row %d of image %d is tile %d of %d", row, sg.image, t, sg.n_tiles)); continue; }
                const int ty = tys[sg.tile0 + t], tx = txs[sg.tile0 + t];
                const int sy = (f & 1) ? ph - 1 - y : y;
                const long long lo = sg.img_off, hi = sg.img_off + (long long)C * sg.Hp * sg.Wp;
                const long long src = sg.img_off + ((long long)ch * sg.Hp + ty + sy) * sg.Wp + tx;
                const long long dst = (((long long)(sg.batch_row + lrow) * C + ch) * ph + y) * pw + x0;
                const bool vec = ((pw | sg.Wp | tx) & 3) == 0;
                for (int j = 0; j < 4; ++j) {
                    const int x = x0 + j;
                    if (!vec && x >= pw) continue;
                    const long long s1 = vec ? ((f & 2) ? src + pw - 4 - x0 + j : src + x0 + j) : src + ((f & 2) ? pw - 1 - x : x);
                    if (s1 < lo || s1 >= hi) g_t.viol("T3", fmt("gather: image %d lane %lld reads float %lld outside [%lld, %lld)", sg.image, q, s1, lo, hi));
                    if (dst + j < (long long)sg.batch_row * C * (long long)plane || dst + j >= (long long)(sg.batch_row + sg.n_rows) * C * (long long)plane || (size_t)(dst + j) >= bw.size())
                        g_t.viol("T3", fmt("gather: image %d lane %lld writes batch float %lld outside its rows", sg.image, q, dst + j));
                    else if (bw[(size_t)(dst + j)]++) g_t.viol("T3", fmt("gather: batch float %lld written twice", dst + j));
                }
                if (vec) {
                    const long long s0 = (f & 2) ? src + pw - 4 - x0 : src + x0;
                    if ((pl.o_imgs + 4 * s0) % 16 || (pl.o_batch + 4 * dst) % 16) g_t.viol("T3", fmt("gather: image %d lane %lld: a 16-byte access at a place that is not 16-byte aligned", sg.image, q));
                }
            }
        }
        for (size_t k = 0; k < bw.size(); ++k) if (bw[k] != 1) { g_t.viol("T3", fmt("gather: batch float %zu of the chunk written %d times", k, bw[k])); break; }
        if (!ck.aggregate) continue;
        // ---- sw_aggregate (kernels_sw.h:87-174)
        for (unsigned blk = 0; blk < ck.ablocks; ++blk) {
            const SwSeg& sg = pl.segs[ck.seg0 + find_owner(afirst, blk)];
            const int Hp = sg.Hp, Wp = sg.Wp, Wq = (Wp + 3) >> 2;
            const long long total = (long long)K * Hp * Wq;
            for (int tid = 0; tid < 256; ++tid) {
                const long long q = (long long)(blk - sg.ablock0) * 256 + tid;
                if (q >= total) continue;
                const int X0 = (int)(q % Wq) * 4; const long long r = q / Wq;
                const int Y = (int)(r % Hp), k = (int)(r / Hp);
                for (int t = 0; t < sg.n_tiles; ++t) {
                    const int ty = tys[sg.tile0 + t], tx = txs[sg.tile0 + t];
                    const int yy = Y - ty, xx0 = X0 - tx;
                    if (yy < 0 || yy >= ph || xx0 + 3 < 0 || xx0 >= pw) continue;
                    const long long row_lo = sg.log_row, row_hi = (long long)sg.log_row + (long long)sg.n_tiles * V;
                    const bool vec = ((tx | pw) & 3) == 0;
                    for (int v = 0; v < V; ++v) {
                        const int f = (pl.vflips >> (8 * v)) & 3;
                        const long long lrow = (long long)sg.log_row + (long long)t * V + v;
                        if (lrow < row_lo || lrow >= row_hi || (size_t)lrow >= log_need_rows) g_t.viol("T3", fmt("aggregate: image %d reads logit row %lld outside its rows", sg.image, lrow));
                        const int sy = (v && (f & 1)) ? ph - 1 - yy : yy;
                        for (int j = 0; j < 4; ++j) {
                            const int xx = xx0 + j;
                            if (!vec && (xx < 0 || xx >= pw)) continue;
                            const long long at = vec ? ((v && (f & 2)) ? (long long)sy * pw + pw - 4 - xx0 + j : (long long)sy * pw + xx0 + j)
                                                     : (long long)sy * pw + ((v && (f & 2)) ? pw - 1 - xx : xx);
                            if (at < 0 || at >= (long long)plane) g_t.viol("T3", fmt("aggregate: image %d lane %lld reads element %lld of a %d x %d tile plane", sg.image, q, at, ph, pw));
                        }
                        if (vec) {
                            const long long a0 = (v && (f & 2)) ? (long long)sy * pw + pw - 4 - xx0 : (long long)sy * pw + xx0;
                            if ((pl.o_log + 4 * ((lrow * K + k) * (long long)plane + a0)) % 16) g_t.viol("T3", fmt("aggregate: image %d lane %lld: a 16-byte read that is not 16-byte aligned", sg.image, q));
                            if ((pl.o_g + 2 * ((long long)yy * pw + xx0)) % 8) g_t.viol("T3", fmt("aggregate: image %d lane %lld: an 8-byte gaussian read that is not 8-byte aligned", sg.image, q));
                        }
                    }
                }
                const int nx = Wp - X0 < 4 ? Wp - X0 : 4;
                const long long o = sg.out_off + ((long long)k * Hp + Y) * Wp + X0;
                const int nw = (Wp & 3) == 0 ? 4 : nx;
                for (int j = 0; j < nw; ++j) {
                    if (o + j < sg.out_off || o + j >= sg.out_off + (long long)K * Hp * Wp || (size_t)(o + j) >= out_written.size()) g_t.viol("T3", fmt("aggregate: image %d lane %lld writes output %lld outside its planes", sg.image, q, o + j));
                    else if (out_written[(size_t)(o + j)]++) g_t.viol("T3", fmt("aggregate: output %lld written twice", o + j));
                }
                if ((Wp & 3) == 0 && ((pl.o_o16 + 2 * o) % 8 || (pl.o_seg + o) % 4)) g_t.viol("T3", fmt("aggregate: image %d lane %lld: a vector store that is not aligned", sg.image, q));
            }
        }
    }
    for (const SwSeg& sg : pl.segs)
        for (long long o = sg.out_off; o < sg.out_off + (long long)K * sg.Hp * sg.Wp; ++o)
            if (out_written[(size_t)o] != 1) { g_t.viol("T3", fmt("image %d: output %lld written %d times", sg.image, o, out_written[(size_t)o])); break; }
}

void go(const char* name, const ts2d_engine* e, Call c, int F, int mirror) {
    c.F = F; c.mirror = mirror;
    SwPlan pl;
    const SwTail tail = tail_of(c);
    const int rc = plan_tiled(e, c.F, c.images.data(), tail, (int)c.images.size(), c.ph, c.pw, c.mirror, c.name_images, "entry", &pl);
    g_t.where = fmt("plan %lld '%s' kind=%d F=%d mirror=%d patch=%dx%d n=%zu", g_plans, name, c.kind, F, mirror, c.ph, c.pw, c.images.size());
    if (rc != TS2D_OK) { g_t.viol("T0", fmt("refused: %s", last_error())); return; }
    ++g_plans;
    if (g_tamper == 7) pl.cap_rows -= 1;                                                   // a batch one row short of the largest chunk
    if (g_tamper == 8 && pl.segs.size() > 1) pl.segs.back().out_off -= 8;                  // the last image's outputs moved onto the one before
    if (g_tamper == 9 && !pl.chunks.empty()) pl.chunks.back().aggregate = false;           // the last image never aggregated
    if (g_tamper == 10) pl.o_log -= 256;                                                   // the logits one block into the batch
    check_plan(e, c, tail, pl);
}

void refuse(const char* name, const ts2d_engine* e, const Call& c) {
    SwPlan pl;
    const SwTail tail = tail_of(c);
    const int rc = plan_tiled(e, c.F, c.images.data(), tail, (int)c.images.size(), c.ph, c.pw, c.mirror, c.name_images, "entry", &pl);
    ++g_refused;
    std::printf("refused|%s|%d|%d|%d|%zu|%s\n", name, c.kind, (int)c.name_images, rc, pl.chunks.size(), rc ? last_error() : "");
}

}  // namespace

int main_tiled() {
    std::unique_ptr<ts2d_engine> eng(new ts2d_engine());
    eng->arch.input_channels = 2; eng->arch.num_classes = 3;
    const ts2d_engine* e = eng.get();
    // {1, 3} and {3}: every image un-resampled - a label-map, regions or probabilities tail without a single tap; {4, 4} under both mirrors: 2 x 32 rows
    // fill a chunk exactly, {5} alone is 16 x 4 = 64 rows, {3} has 160
    const std::vector<std::vector<int>> sets = {{0}, {0, 1, 2}, {3}, {2, 3, 0, 1, 1}, {1, 3}, {4, 4}, {4, 4, 0}, {5}, {5, 0, 5}};
    for (const auto& idx : sets)
        for (int F : {1, 3})
            for (int mirror : {0, 1, 2, 3}) {
                go("none logits", e, make(kNone, idx, false, false), F, mirror);
                go("none both", e, make(kNone, idx, false, false, 0, true), F, mirror);
                go("export u8", e, make(kExport, idx, true, false), F, mirror);
                go("export f32", e, make(kExport, idx, false, true), F, mirror);
                go("export both padded", e, make(kExport, idx, true, true, 0, true), F, mirror);
                go("labelmap", e, make(kLabelmap, idx, true, false), F, mirror);
                go("regions", e, make(kRegions, idx, true, false), F, mirror);
                for (int mode = 0; mode < 3; ++mode) {
                    go("probabilities", e, make(kProb, idx, false, true, mode), F, mirror);
                    go("probabilities decided", e, make(kProb, idx, true, true, mode, mode == 1), F, mirror);
                }
            }
    for (int F : {1, 3})
        for (int mode = 0; mode < 3; ++mode)
            for (int dec = 0; dec < 2; ++dec) {
                go("runs 1", e, make_runs({1}, 0, dec, mode), F, 3);
                go("runs 3+1+2", e, make_runs({3, 1, 2}, 2, dec, mode), F, 3);
                go("runs that split over chunks", e, make_runs({2, 3}, 3, dec, mode), F, 3);
            }
    // patches other than 32 x 32: 24 x 40, and 32 x 31 / 30 x 26 whose width is no multiple of 4 (the per-pixel paths of both kernels)
    for (int mirror : {0, 1, 2, 3}) {
        go("export patch 24x40", e, make(kExport, {2, 3}, true, true, 0, false, 24, 40), 1, mirror);
        go("labelmap patch 32x31", e, make(kLabelmap, {0, 1}, true, false, 0, true, 32, 31), 1, mirror);
        go("none patch 30x26", e, make(kNone, {0, 2, 1}, false, false, 0, true, 30, 26), 3, mirror);
        go("none patch 32x32 on a pitch of 70", e, make(kNone, {2}, false, false, 0, true), 1, mirror);
    }
    if (g_tamper) {
        std::printf("tally");
        for (const char* p : {"T0", "T1", "T2", "T3", "T4"}) std::printf(" %s=%lld", p, g_t.n[p]);
        std::printf(" plans=%lld replayed=%lld\n", g_plans, g_replayed);
        return 0;
    }
    // ---- the refused calls of the record script (scripts/tiled_plan_record.py), every one of them for every kind it runs them for: one fault, then two at
    // once (which message wins).  A fault in a field the kind does not read (the full extent and the box of a tail that is no probabilities tail, the
    // padded outputs of a call with a tail, the output the kind does not have) leaves the call accepted: recorded with rc 0 and its chunks.
    for (int kind = kNone; kind <= kProb; ++kind)
        for (int named = 0; named < 2; ++named) {
            const bool a = kind != kNone, b = kind == kExport || kind == kProb;
            auto base = [&]() { Call c = make(kind, {0, 1, 2}, a, b, kind == kProb ? 2 : 0); c.name_images = named != 0; return c; };
            Call c = base(); c.ph = 0; refuse("bad patch", e, c);
            c = base(); c.images[1].image = nullptr; refuse("null image", e, c);
            c = base(); c.images[1].tile_x = nullptr; refuse("null tiles", e, c);
            c = base(); c.images[2].logits_f16 = nullptr; c.images[2].seg_u8 = nullptr; refuse("no padded output", e, c);
            c = base(); c.images[1].n_tiles = 0; refuse("no tiles", e, c);
            c = base(); c.images[0].Hp = 31; refuse("patch above image", e, c);
            c = base(); c.images[1].Hp = 1 << 15; c.images[1].Wp = 1 << 15; refuse("2^31 elements", e, c);
            c = base(); const_cast<int32_t*>(c.images[2].tile_y)[1] = 50 - 31; refuse("tile leaves", e, c);
            c = base(); c.images[0].n_tiles = 1 << 20; c.images[0].tile_y = nullptr; refuse("null tiles and too many", e, c);
            c = base(); c.images[0].n_tiles = (1 << 20) + 1; refuse("too many tiles", e, c);
            if (kind == kNone) continue;
            c = base(); c.rects[1].u8 = nullptr; c.rects[1].f32 = nullptr; refuse("null outputs", e, c);
            c = base(); c.rects[1].u8 = nullptr; refuse("null first output", e, c);
            c = base(); c.rects[1].f32 = nullptr; refuse("null second output", e, c);
            c = base(); c.rects[2].src_h = 50; refuse("rect leaves", e, c);
            c = base(); c.rects[0].src_x = -1; refuse("rect negative", e, c);
            c = base(); c.rects[0].src_w = 0; refuse("rect empty", e, c);
            c = base(); c.rects[1].out_h = 0; refuse("bad out extent", e, c);
            c = base(); c.rects[1].out_h = 1 << 15; c.rects[1].out_w = 1 << 15; c.rects[1].full_h = 1 << 16; c.rects[1].full_w = 1 << 16; refuse("2^30 outputs", e, c);
            c = base(); c.rects[1].out_h = 1 << 16; c.rects[1].out_w = 1 << 15; c.rects[1].full_h = 1 << 17; c.rects[1].full_w = 1 << 16; refuse("2^31 outputs", e, c);
            c = base(); c.rects[0].out_h = 1 << 25; c.rects[0].out_w = 1; c.rects[1].out_h = 1 << 25; c.rects[1].out_w = 2; c.rects[0].full_h = c.rects[1].full_h = 1 << 26;
            refuse("2^26 taps", e, c);
            c = base(); c.rects[1].box_y = -1; refuse("box negative", e, c);
            c = base(); c.rects[1].full_w = c.rects[1].out_w; refuse("box leaves", e, c);
            c = base(); c.rects[1].full_h = 0; refuse("full empty", e, c);
            c = base(); c.rects[2].full_h = 1 << 15; c.rects[2].full_w = 1 << 15; refuse("2^31 full", e, c);
            // two at once
            c = base(); c.rects[1].u8 = nullptr; c.rects[1].f32 = nullptr; c.rects[1].src_h = 99; refuse("null outputs + rect leaves", e, c);
            c = base(); c.rects[0].src_h = 99; c.rects[1].u8 = nullptr; c.rects[1].f32 = nullptr; refuse("rect leaves at 0 + null outputs at 1", e, c);
            c = base(); c.images[1].n_tiles = 0; c.rects[0].out_w = -4; refuse("bad out at 0 + no tiles at 1", e, c);
            c = base(); c.images[0].n_tiles = 0; c.rects[0].out_w = -4; refuse("no tiles + bad out, both at 0", e, c);
            c = base(); c.rects[1].out_h = 0; c.rects[1].full_h = 0; refuse("bad out + full empty", e, c);
            c = base(); c.rects[1].src_y = 100; c.rects[1].box_x = -2; refuse("rect leaves + box negative", e, c);
            c = base(); c.ph = -1; c.rects[0].u8 = nullptr; c.rects[0].f32 = nullptr; refuse("bad patch + null outputs", e, c);
        }
    for (int named = 0; named < 2; ++named) {
        auto base = [&]() { Call c = make_runs({2, 1}, 1, true, 0); c.name_images = named != 0; return c; };
        Call c = base(); c.images[1].image = nullptr; refuse("runs null image", e, c);
        c = base(); c.rects[1].src_h = 40; c.runs[1].src_h = 40; refuse("runs rect leaves", e, c);
        c = base(); c.rects[0].full_h = 0; c.runs[0].full_h = 0; refuse("runs full empty", e, c);
        c = base(); c.rects[1].box_y = 900; c.runs[1].box_y = 900; c.images[0].n_tiles = 0; refuse("runs no tiles at 0 + box leaves in run 1", e, c);
    }
    {   // 64 images of 2^20 tiles (one shared tile list) x 4 mirror variants: 2^28 network rows in one call
        Call c = make(kLabelmap, {0}, true, false);
        c.mirror = 3;
        std::vector<int32_t> zeros((size_t)1 << 20, 0);
        c.images[0].n_tiles = 1 << 20; c.images[0].tile_y = c.images[0].tile_x = zeros.data();
        c.images.resize(64, c.images[0]); c.rects.resize(64, c.rects[0]);
        refuse("2^28 network rows", e, c);
        c.images.resize(63); c.rects.resize(63); c.rects[62].src_h = 0;
        refuse("rect empty at 62 (below 2^28 rows)", e, c);
    }
    std::printf("tally");
    for (const char* p : {"T0", "T1", "T2", "T3", "T4"}) std::printf(" %s=%lld", p, g_t.n[p]);
    std::printf(" plans=%lld replayed=%lld lanes=%lld refused=%lld\n", g_plans, g_replayed, g_lanes, g_refused);
    return 0;
}
