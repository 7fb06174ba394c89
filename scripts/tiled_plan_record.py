"""Plan record of the sliding window's device-free front (csrc/tiled_plan.cpp: plan_tiled, rs_plan_segment) behind a main of its own, under the
address and undefined-behaviour sanitizers: for every kind of tail, what the plan refuses (``rc|message``) and, for an accepted call, every
offset and count of the SwPlan, its chunks and a hash of the table blob.  No GPU and no built library needed.

    python scripts/tiled_plan_record.py OUT.txt [--root OTHER_CHECKOUT]

The record of two commits is compared byte for byte (``cmp a.txt b.txt``): a refactor of the planning must leave it identical.  The driver is
the same for both; the ONE adapter that spells the call is chosen by what the checkout's engine_internal.h declares (a tail descriptor, or the
four arguments a call had before it)."""
import os
import subprocess
import sys
import tempfile

HIPCC = '/opt/rocm/bin/hipcc'

DRIVER = r'''
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
static char g_msg[1024];
namespace ts2d {
int fail(int code, const char* fmt, ...) {                   // the library's is program.cpp: here the message is kept for the record
    va_list ap;
    va_start(ap, fmt);
    std::vsnprintf(g_msg, sizeof(g_msg), fmt, ap);
    va_end(ap);
    return code;
}
const char* last_error() { return g_msg; }
}
using namespace ts2d;

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

// ---------------------------------------------------------------- the adapter: the one place that differs between the two sides
#ifdef TS2D_TAIL_API
static SwTail tail_of(const Call& c, bool one = false) {
    const int n = one ? 1 : (int)c.images.size();
    SwTail t((SwTail::Kind)c.kind, c.kind == kNone ? 0 : n);
    t.mode = c.mode;
    t.class_order = c.kind == kRegions || (c.kind >= kProb && c.mode == kProbRegions) ? c.order.data() : nullptr;
    if (c.kind == kProbRuns) {
        t.runs = c.runs.data(); t.n_runs = (int)c.runs.size(); t.run_of.resize((size_t)n);
        for (size_t r = 0; r < c.runs.size(); ++r)
            for (int s = 0; s < c.runs[r].n_slices; ++s) {
                const Rect& q = c.rects[r];
                const size_t i = (size_t)c.runs[r].first_image + s;
                t.images[i] = SwTail::Image{q.src_y, q.src_x, q.src_h, q.src_w, q.out_h, q.out_w, q.full_h, q.full_w, q.box_y, q.box_x, q.u8, q.f32};
                t.run_of[i] = (int)r;
            }
        return t;
    }
    for (size_t i = 0; i < t.images.size(); ++i) {
        const Rect& q = c.rects[i];
        t.images[i] = SwTail::Image{q.src_y, q.src_x, q.src_h, q.src_w, q.out_h, q.out_w, q.full_h, q.full_w, q.box_y, q.box_x, q.u8, q.f32};
    }
    return t;
}
static int call_plan(const ts2d_engine* e, const Call& c, SwPlan* pl) {
    return plan_tiled(e, c.F, c.images.data(), tail_of(c), (int)c.images.size(), c.ph, c.pw, c.mirror, c.name_images, "entry", pl);
}
static void call_segment(const Call& c, int K, int Hp, int Wp, long long src_off, std::vector<RsSeg>* rsegs, std::vector<RsTap>* rtaps, long long* blocks,
                         long long* elems) {
    rs_plan_segment(tail_of(c, true), 0, K, Hp, Wp, src_off, rsegs, rtaps, blocks, elems);
}
#else
static int call_plan(const ts2d_engine* e, const Call& c, SwPlan* pl) {
    const size_t n = c.images.size();
    std::vector<ts2d_tiled_export> ex(n);
    std::vector<ts2d_tiled_probabilities> pd(n);
    std::vector<int> run_of(n);
    const bool prob = c.kind >= kProb;
    auto put = [&](size_t i, const Rect& q) {
        ex[i] = ts2d_tiled_export{q.src_y, q.src_x, q.src_h, q.src_w, q.out_h, q.out_w, prob ? reinterpret_cast<uint8_t*>(q.f32) : q.u8, c.kind == kExport ? q.f32 : nullptr};
        pd[i] = ts2d_tiled_probabilities{q.src_y, q.src_x, q.src_h, q.src_w, q.out_h, q.out_w, q.full_h, q.full_w, q.box_y, q.box_x, q.f32, q.u8};
    };
    if (c.kind == kProbRuns) {
        for (size_t r = 0; r < c.runs.size(); ++r)
            for (int s = 0; s < c.runs[r].n_slices; ++s) { put((size_t)c.runs[r].first_image + s, c.rects[r]); run_of[(size_t)c.runs[r].first_image + s] = (int)r; }
    } else if (c.kind != kNone) {
        for (size_t i = 0; i < n; ++i) put(i, c.rects[i]);
    }
    ProbCall pc{pd.data(), c.mode};
    if (c.kind == kProbRuns) { pc.runs = c.runs.data(); pc.n_runs = (int)c.runs.size(); pc.run_of = run_of.data(); }
    const uint8_t* order = c.kind == kRegions || (prob && c.mode == kProbRegions) ? c.order.data() : nullptr;
    return plan_tiled(e, c.F, c.images.data(), c.kind == kNone ? nullptr : ex.data(), c.kind >= kLabelmap, order, prob ? &pc : nullptr, (int)n, c.ph, c.pw,
                      c.mirror, c.name_images, "entry", pl);
}
static void call_segment(const Call& c, int K, int Hp, int Wp, long long src_off, std::vector<RsSeg>* rsegs, std::vector<RsTap>* rtaps, long long* blocks,
                         long long* elems) {
    const Rect& q = c.rects[0];
    const ts2d_tiled_export ex{q.src_y, q.src_x, q.src_h, q.src_w, q.out_h, q.out_w, q.u8, nullptr};
    const int full_hw[2] = {q.full_h, q.full_w};
    rs_plan_segment(c.kind >= kLabelmap, K, Hp, Wp, ex, src_off, rsegs, rtaps, blocks, c.kind >= kProb ? nullptr : elems, c.kind >= kProb ? full_hw : nullptr);
}
#endif

// ---------------------------------------------------------------- the record
static unsigned long long fnv(const void* p, size_t n) {
    unsigned long long h = 1469598103934665603ull;
    for (size_t i = 0; i < n; ++i) { h ^= static_cast<const unsigned char*>(p)[i]; h *= 1099511628211ull; }
    return h;
}
static int g_cases = 0, g_refused = 0;
static void record(const char* name, const ts2d_engine* e, const Call& c) {
    SwPlan pl;
    g_msg[0] = 0;
    const int rc = call_plan(e, c, &pl);
    ++g_cases; g_refused += rc != 0;
    std::printf("%s F=%d n=%zu mirror=%d named=%d\n  %d|%s\n", name, c.F, c.images.size(), c.mirror, (int)c.name_images, rc, rc ? g_msg : "");
    if (rc) return;
    std::printf("  V=%d vflips=%d cap_rows=%d tiles=%lld out_elems=%lld rs_blocks=%lld any=%d%d%d%d prob_elems=%lld n=%zu/%zu/%zu/%zu/%zu\n", pl.V, pl.vflips,
                pl.cap_rows, pl.n_tiles_all, pl.out_elems, pl.rs_blocks, pl.any16, pl.anyseg, pl.any_rs8, pl.any_rs32, pl.prob_elems, pl.segs.size(),
                pl.chunks.size(), pl.rsegs.size(), pl.psegs.size(), pl.pssegs.size());
    std::printf("  tab %zu: %zu %zu %zu %zu %zu hash %016llx\n", pl.tab.size(), pl.tab_segs, pl.tab_rsegs, pl.tab_rtaps, pl.tab_order, pl.tab_psegs,
                fnv(pl.tab.data(), pl.tab.size()));
    std::printf("  scratch %zu: %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", pl.bytes, pl.o_tab, pl.o_g, pl.o_imgs, pl.o_batch, pl.o_log, pl.o_o16, pl.o_seg,
                pl.o_flag, pl.o_rs8, pl.o_rs32, pl.o_prob);
    for (const SwChunk& k : pl.chunks)
        std::printf("  chunk seg0=%d n=%d rows=%d log_row=%d agg=%d g=%u a=%u\n", k.seg0, k.n_segs, k.rows, k.log_row, (int)k.aggregate, k.gblocks, k.ablocks);
    for (const RsSeg& r : pl.rsegs) std::printf("  rseg %016llx\n", fnv(&r, sizeof(r)));
    for (const ProbSeg& p : pl.psegs) std::printf("  pseg %016llx\n", fnv(&p, sizeof(p)));
    for (const ProbStackSeg& p : pl.pssegs) std::printf("  psseg %016llx\n", fnv(&p, sizeof(p)));
}

static float g_px[8];
static uint8_t g_u8[8];
static std::vector<std::vector<int32_t>> g_ty, g_tx;         // (kept alive: the images point into them)
static ts2d_tiled_image image(int Hp, int Wp, int n_tiles, bool l16, bool seg, int ph = 32, int pw = 32) {
    std::vector<int32_t> ty, tx;
    for (int t = 0; t < n_tiles; ++t) { ty.push_back((t * 7) % (Hp - ph + 1 > 0 ? Hp - ph + 1 : 1)); tx.push_back((t * 5) % (Wp - pw + 1 > 0 ? Wp - pw + 1 : 1)); }
    g_ty.push_back(ty); g_tx.push_back(tx);
    return ts2d_tiled_image{g_px, Hp, Wp, n_tiles, g_ty.back().data(), g_tx.back().data(), l16 ? reinterpret_cast<uint16_t*>(g_px) : nullptr,
                            seg ? g_u8 : nullptr, 0};
}
static const int kExtents[4][3] = {{40, 32, 2}, {32, 48, 2}, {50, 70, 6}, {90, 100, 40}};        // Hp, Wp, tiles (the last: more rows than a chunk)
static const int kRects[4][6] = {{4, 0, 30, 32, 45, 20}, {0, 8, 32, 33, 32, 33}, {1, 2, 48, 60, 17, 90}, {3, 5, 80, 90, 80, 90}};
static Rect rect(int i, bool u8, bool f32) {
    const int* q = kRects[i];
    return Rect{q[0], q[1], q[2], q[3], q[4], q[5], q[4] + 7 + i, q[5] + 3, 2 + i, 1, u8 ? g_u8 : nullptr, f32 ? g_px : nullptr};
}
static Call make(int kind, const std::vector<int>& idx, bool a, bool b, int mode = 0, bool padded = false) {
    // a / b: the kind's two outputs - export: uint8 / float; label map and regions: the plane / -; probabilities: the decided map / the planes
    Call c;
    c.kind = kind; c.mode = mode; c.order = {3, 1, 2};
    for (int i : idx) {
        c.images.push_back(image(kExtents[i][0], kExtents[i][1], kExtents[i][2], kind == kNone || padded, padded));
        if (kind != kNone && kind != kProbRuns) c.rects.push_back(rect(i, a, b));
    }
    return c;
}
static Call make_runs(const std::vector<int>& slices, int ext, bool dec, int mode) {       // runs of `slices` images, all of extent `ext`
    Call c;
    c.kind = kProbRuns; c.mode = mode; c.order = {3, 1, 2};
    int first = 0;
    for (size_t r = 0; r < slices.size(); ++r) {
        for (int s = 0; s < slices[r]; ++s) c.images.push_back(image(kExtents[ext][0], kExtents[ext][1], kExtents[ext][2], false, false));
        const Rect q = rect(ext, dec, true);
        c.rects.push_back(q);
        const long long plane = (long long)q.full_h * q.full_w * slices[r];
        c.runs.push_back(ts2d_tiled_probabilities_run{q.src_y, q.src_x, q.src_h, q.src_w, q.out_h, q.out_w, q.full_h, q.full_w, q.box_y, q.box_x, first, slices[r],
                                                      q.f32, plane + 11, q.u8, plane});
        first += slices[r];
    }
    return c;
}

int main() {
    static ts2d_engine eng;
    eng.arch.input_channels = 2; eng.arch.num_classes = 3;
    const ts2d_engine* e = &eng;
    const std::vector<std::vector<int>> sets = {{0}, {0, 1, 2}, {3}, {2, 3, 0, 1, 1}};
    // ---- accepted calls: every kind x image set x folds x mirror mask
    for (const auto& idx : sets)
        for (int F : {1, 2})
            for (int mirror : {0, 1, 2, 3}) {
                auto go = [&](const char* name, Call c) { c.F = F; c.mirror = mirror; record(name, e, c); };
                go("none logits", make(kNone, idx, false, false));
                go("none both", make(kNone, idx, false, false, 0, true));
                go("export u8", make(kExport, idx, true, false));
                go("export f32", make(kExport, idx, false, true));
                go("export both padded", make(kExport, idx, true, true, 0, true));
                go("labelmap", make(kLabelmap, idx, true, false));
                go("regions", make(kRegions, idx, true, false));
                for (int mode = 0; mode < 3; ++mode) {
                    go("probabilities", make(kProb, idx, false, true, mode));
                    go("probabilities decided", make(kProb, idx, true, true, mode, mode == 1));
                }
            }
    for (int F : {1, 2})
        for (int mode = 0; mode < 3; ++mode)
            for (int dec = 0; dec < 2; ++dec) {
                auto go = [&](const char* name, Call c) { c.F = F; c.mirror = 3; record(name, e, c); };
                go("runs 1", make_runs({1}, 0, dec, mode));
                go("runs 3+1+2", make_runs({3, 1, 2}, 2, dec, mode));
                go("runs that split over chunks", make_runs({2, 3}, 3, dec, mode));
            }
    {   // patches other than 32 x 32, and a gaussian-sized scratch that follows them
        Call c = make(kExport, {2, 3}, true, true);
        c.ph = 24; c.pw = 40;
        record("export patch 24x40", e, c);
        c = make(kLabelmap, {0, 1}, true, false); c.ph = 32; c.pw = 31;
        record("labelmap patch 32x31", e, c);
    }
    // ---- the refusals, each kind: one fault, then two at once (which message wins)
    for (int kind = kNone; kind <= kProb; ++kind)
        for (int named = 0; named < 2; ++named) {
            const bool a = kind != kNone, b = kind == kExport || kind == kProb;
            auto base = [&]() { Call c = make(kind, {0, 1, 2}, a, b, kind == kProb ? 2 : 0); c.name_images = named != 0; return c; };
            char tag[64];
            auto go = [&](const char* what, const Call& c) { std::snprintf(tag, sizeof(tag), "refuse kind=%d %s", kind, what); record(tag, e, c); };
            Call c = base(); c.ph = 0; go("bad patch", c);
            c = base(); c.images[1].image = nullptr; go("null image", c);
            c = base(); c.images[1].tile_x = nullptr; go("null tiles", c);
            c = base(); c.images[2].logits_f16 = nullptr; c.images[2].seg_u8 = nullptr; go("no padded output", c);
            c = base(); c.images[1].n_tiles = 0; go("no tiles", c);
            c = base(); c.images[0].Hp = 31; go("patch above image", c);
            c = base(); c.images[1].Hp = 1 << 15; c.images[1].Wp = 1 << 15; go("2^31 elements", c);
            c = base(); g_ty[g_ty.size() - 1][1] = 50 - 31; go("tile leaves", c);
            c = base(); c.images[0].n_tiles = 1 << 20; c.images[0].tile_y = nullptr; go("null tiles and too many", c);
            c = base(); c.images[0].n_tiles = (1 << 20) + 1; go("too many tiles", c);
            if (kind == kNone) continue;
            c = base(); c.rects[1].u8 = nullptr; c.rects[1].f32 = nullptr; go("null outputs", c);
            c = base(); c.rects[1].u8 = nullptr; go("null first output", c);
            c = base(); c.rects[1].f32 = nullptr; go("null second output", c);
            c = base(); c.rects[2].src_h = 50; go("rect leaves", c);
            c = base(); c.rects[0].src_x = -1; go("rect negative", c);
            c = base(); c.rects[0].src_w = 0; go("rect empty", c);
            c = base(); c.rects[1].out_h = 0; go("bad out extent", c);
            c = base(); c.rects[1].out_h = 1 << 15; c.rects[1].out_w = 1 << 15; c.rects[1].full_h = 1 << 16; c.rects[1].full_w = 1 << 16; go("2^30 outputs", c);
            c = base(); c.rects[1].out_h = 1 << 16; c.rects[1].out_w = 1 << 15; c.rects[1].full_h = 1 << 17; c.rects[1].full_w = 1 << 16; go("2^31 outputs", c);
            c = base(); c.rects[0].out_h = 1 << 25; c.rects[0].out_w = 1; c.rects[1].out_h = 1 << 25; c.rects[1].out_w = 2; c.rects[0].full_h = c.rects[1].full_h = 1 << 26;
            go("2^26 taps", c);
            c = base(); c.rects[1].box_y = -1; go("box negative", c);
            c = base(); c.rects[1].full_w = c.rects[1].out_w; go("box leaves", c);
            c = base(); c.rects[1].full_h = 0; go("full empty", c);
            c = base(); c.rects[2].full_h = 1 << 15; c.rects[2].full_w = 1 << 15; go("2^31 full", c);
            // two at once
            c = base(); c.rects[1].u8 = nullptr; c.rects[1].f32 = nullptr; c.rects[1].src_h = 99; go("null outputs + rect leaves", c);
            c = base(); c.rects[0].src_h = 99; c.rects[1].u8 = nullptr; c.rects[1].f32 = nullptr; go("rect leaves at 0 + null outputs at 1", c);
            c = base(); c.images[1].n_tiles = 0; c.rects[0].out_w = -4; go("bad out at 0 + no tiles at 1", c);
            c = base(); c.images[0].n_tiles = 0; c.rects[0].out_w = -4; go("no tiles + bad out, both at 0", c);
            c = base(); c.rects[1].out_h = 0; c.rects[1].full_h = 0; go("bad out + full empty", c);
            c = base(); c.rects[1].src_y = 100; c.rects[1].box_x = -2; go("rect leaves + box negative", c);
            c = base(); c.ph = -1; c.rects[0].u8 = nullptr; c.rects[0].f32 = nullptr; go("bad patch + null outputs", c);
        }
    for (int named = 0; named < 2; ++named) {
        auto base = [&]() { Call c = make_runs({2, 1}, 1, true, 0); c.name_images = named != 0; return c; };
        Call c = base(); c.images[1].image = nullptr; record("refuse runs null image", e, c);
        c = base(); c.rects[1].src_h = 40; c.runs[1].src_h = 40; record("refuse runs rect leaves", e, c);
        c = base(); c.rects[0].full_h = 0; c.runs[0].full_h = 0; record("refuse runs full empty", e, c);
        c = base(); c.rects[1].box_y = 900; c.runs[1].box_y = 900; c.images[0].n_tiles = 0; record("refuse runs no tiles at 0 + box leaves in run 1", e, c);
    }
    {   // 64 images of 2^20 tiles (one shared tile list) x 4 mirror variants: 2^28 network rows in one call
        Call c = make(kLabelmap, {0}, true, false);
        c.mirror = 3;
        std::vector<int32_t> zeros((size_t)1 << 20, 0);
        c.images[0].n_tiles = 1 << 20; c.images[0].tile_y = c.images[0].tile_x = zeros.data();
        c.images.resize(64, c.images[0]); c.rects.resize(64, c.rects[0]);
        record("refuse 2^28 network rows", e, c);
        c.images.resize(63); c.rects.resize(63); c.rects[62].src_h = 0;
        record("refuse rect empty at 62 (below 2^28 rows)", e, c);
    }
    // ---- rs_plan_segment as the *_from_logits entries call it: one image, no plan around it
    for (int kind = kLabelmap; kind <= kProb; ++kind)
        for (int i = 0; i < 4; ++i)
            for (long long src_off : {0LL, 7680LL}) {
                Call c = make(kind, {i}, true, kind == kProb);
                std::vector<RsSeg> rsegs; std::vector<RsTap> rtaps;
                long long blocks = 5, elems = 512;
                call_segment(c, 3, kExtents[i][0], kExtents[i][1], src_off, &rsegs, &rtaps, &blocks, &elems);
                call_segment(c, 3, kExtents[i][0], kExtents[i][1], src_off + 256, &rsegs, &rtaps, &blocks, &elems);
                ++g_cases;
                std::printf("segment kind=%d image=%d src_off=%lld: blocks=%lld elems=%lld taps=%zu %016llx segs %016llx %016llx\n", kind, i, src_off, blocks, elems,
                            rtaps.size(), fnv(rtaps.data(), rtaps.size() * sizeof(RsTap)), fnv(&rsegs[0], sizeof(RsSeg)), fnv(&rsegs[1], sizeof(RsSeg)));
            }
    std::printf("%d cases, %d refused\n", g_cases, g_refused);
    return 0;
}
'''


def main():
    out = sys.argv[1]
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if '--root' in sys.argv:
        root = os.path.abspath(sys.argv[sys.argv.index('--root') + 1])
    csrc = os.path.join(root, 'totalsegmentator2d_amd', 'csrc')
    tail_api = 'struct SwTail' in open(os.path.join(csrc, 'engine_internal.h')).read()
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, 'plan_record.cpp')
        with open(src, 'w') as f:
            f.write(f'#include "{os.path.join(csrc, "engine_internal.h")}"\n' + DRIVER)
        exe = os.path.join(d, 'plan_record')
        inc = os.path.join(os.path.dirname(os.path.dirname(HIPCC)), 'include')
        subprocess.check_call([HIPCC, '-x', 'c++', '-D__HIP_PLATFORM_AMD__', '-I' + inc, '-O1', '-g', '-std=c++17', '-Wall', '-Wno-unused-function',
                               '-fsanitize=address,undefined'] + (['-DTS2D_TAIL_API'] if tail_api else [])
                              + ['-o', exe, src, os.path.join(csrc, 'tiled_plan.cpp')])
        res = subprocess.run([exe], capture_output=True, text=True)
    sys.stderr.write(res.stderr)
    if res.returncode != 0:
        raise SystemExit(f'the driver ended with status {res.returncode}')
    with open(out, 'w') as f:
        f.write(res.stdout)
    import hashlib
    print(f'adapter: {"tail" if tail_api else "quadruple"}; {res.stdout.splitlines()[-1]}; sanitizers silent: {not res.stderr.strip()} -> {out}')
    print('sha256', hashlib.sha256(res.stdout.encode()).hexdigest())


if __name__ == '__main__':
    main()
