// The device-free front of the sliding window (tiled.hip: predict_tiled_impl): argument checks, the rows (tile x mirror variant) of the
// images packed into chunks of at most kSwChunkRows, the export's segments and taps, the table blob and the scratch layout.  Plain C++:
// the taps must match numpy bit for bit, so this arithmetic is not compiled as HIP code.  (Every plan of a scenario table, its rows, regions,
// lane addresses and taps: tests/test_tiled_plan_cpu.py.)
#include "engine_internal.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>

namespace ts2d {
namespace {

long long blocks_of(long long lanes) { return (lanes + 255) / 256; }

// Taps of one axis of the order-1 resample (n_in -> n_out samples; preprocess.linear_axis_taps is the same statement in numpy, pinned
// to scipy): cc = (o + 0.5) * (n_in / n_out) - 0.5, i0 = floor(cc), w1 = cc - i0, all in float64; the coordinate is not clamped, the
// two INDICES are (scipy extends the array by its edge samples).  `origin` shifts the indices to the padded plane.
// No contraction: a fused (o + 0.5) * zoom - 0.5 would round differently from numpy on a host build that has FMA (-march=native).
void rs_axis_taps(int n_in, int n_out, int origin, RsTap* t) {
#pragma clang fp contract(off)
    const double zoom = (double)n_in / (double)n_out;
    for (int o = 0; o < n_out; ++o) {
        const double prod = ((double)o + 0.5) * zoom;
        const double cc = prod - 0.5;
        const double f = std::floor(cc);
        const long long i0 = (long long)f;
        t[o].w1 = cc - f; t[o].w0 = 1.0 - t[o].w1;
        t[o].i0 = origin + (int)std::min<long long>(std::max<long long>(i0, 0), n_in - 1);
        t[o].i1 = origin + (int)std::min<long long>(std::max<long long>(i0 + 1, 0), n_in - 1);
    }
}

// every image (and its part of the tail, under the tail's name) on its own; the totals that bound the tables
int check_images(int F, int C, int K, const ts2d_tiled_image* images, const SwTail& tail, int n_images, int ph, int pw, bool name_images,
                 const char* entry, SwPlan* pl) {
    long long n_taps_all = 0;
    const char* what = tail.what();
    pl->any16 = F > 1;      // (the mean is taken over the half buffers)
    for (int i = 0; i < n_images; ++i) {
        const ts2d_tiled_image& im = images[i];
        char pre[48] = "";
        if (name_images && tail.kind == SwTail::kProbRuns) snprintf(pre, sizeof(pre), "run %d: image %d: ", tail.run_of[i], i);
        else if (name_images) snprintf(pre, sizeof(pre), "image %d: ", i);
        if (!im.image || !im.tile_y || !im.tile_x) return fail(TS2D_ERR_INVALID, "%snull image or tile pointer", pre);
        if (tail.kind == SwTail::kNone && !im.logits_f16 && !im.seg_u8) return fail(TS2D_ERR_INVALID, "%sboth outputs are null", pre);
        if (im.n_tiles < 1 || im.n_tiles > (1 << 20) || im.Hp < 1 || im.Wp < 1 || ph > im.Hp || pw > im.Wp)
            return fail(TS2D_ERR_INVALID, "%sbad tiling: %d tiles of %dx%d on %dx%d", pre, im.n_tiles, ph, pw, im.Hp, im.Wp);
        if ((long long)K * im.Hp * im.Wp >= (1LL << 31) || (long long)C * im.Hp * im.Wp >= (1LL << 31))
            return fail(TS2D_ERR_INVALID, "%s%dx%d exceeds 2^31 elements per image", pre, im.Hp, im.Wp);
        for (int t = 0; t < im.n_tiles; ++t)
            if (im.tile_y[t] < 0 || im.tile_x[t] < 0 || im.tile_y[t] + ph > im.Hp || im.tile_x[t] + pw > im.Wp)
                return fail(TS2D_ERR_INVALID, "%stile %d at (%d,%d) leaves the %dx%d image", pre, t, im.tile_y[t], im.tile_x[t], im.Hp, im.Wp);
        pl->n_tiles_all += im.n_tiles;
        pl->any16 |= im.logits_f16 != nullptr; pl->anyseg |= im.seg_u8 != nullptr;
        if (tail.kind == SwTail::kNone) continue;
        const SwTail::Image& ex = tail.images[i];
        if (tail.no_output(ex)) return fail(TS2D_ERR_INVALID, tail.kind == SwTail::kExport ? "%s%s: both outputs are null" : "%s%s: the output is null", pre, what);
        if (ex.src_h < 1 || ex.src_w < 1 || ex.src_y < 0 || ex.src_x < 0 || ex.src_h > im.Hp - ex.src_y || ex.src_w > im.Wp - ex.src_x)
            return fail(TS2D_ERR_INVALID, "%s%s: source rectangle %dx%d at (%d,%d) is empty or leaves the %dx%d image", pre, what, ex.src_h, ex.src_w,
                        ex.src_y, ex.src_x, im.Hp, im.Wp);
        if (ex.out_h < 1 || ex.out_w < 1) return fail(TS2D_ERR_INVALID, "%s%s: bad output extent %dx%d", pre, what, ex.out_h, ex.out_w);
        if ((long long)tail.planes(K) * ex.out_h * ex.out_w >= (1LL << 31))
            return fail(TS2D_ERR_INVALID, "%s%s: %dx%d exceeds 2^31 output elements", pre, what, ex.out_h, ex.out_w);
        n_taps_all += (long long)ex.out_h + ex.out_w;         // (each < 2^31 by the check above; bounded before any table is allocated)
        if (n_taps_all >= (1LL << 26)) return fail(TS2D_ERR_INVALID, "%s%s: more than 2^26 output rows + columns in one call", pre, what);
        pl->any16 = true;
        pl->any_rs8 |= ex.u8 != nullptr;
        if (!tail.prob()) { pl->any_rs32 |= ex.f32 != nullptr; continue; }
        if (ex.full_h < 1 || ex.full_w < 1 || ex.box_y < 0 || ex.box_x < 0 || ex.out_h > ex.full_h - ex.box_y || ex.out_w > ex.full_w - ex.box_x)
            return fail(TS2D_ERR_INVALID, "%s%s: the %dx%d output at (%d,%d) leaves the full extent %dx%d", pre, what, ex.out_h, ex.out_w, ex.box_y,
                        ex.box_x, ex.full_h, ex.full_w);
        if ((long long)K * ex.full_h * ex.full_w >= (1LL << 31))
            return fail(TS2D_ERR_INVALID, "%s%s: %d x %dx%d exceeds 2^31 output elements", pre, what, K, ex.full_h, ex.full_w);
    }
    if (pl->n_tiles_all * pl->V >= (1LL << 28)) return fail(TS2D_ERR_INVALID, "%s: %lld network rows in one call", entry, pl->n_tiles_all * pl->V);
    return TS2D_OK;
}

// Row packing: whole images, greedily, into chunks of at most kSwChunkRows rows; a larger image takes chunks of its own.
// img_floats / log_rows: floats of the image area, rows of the tile-logit buffer.
int pack_rows(int F, int C, int K, const ts2d_tiled_image* images, int n_images, int ph, int pw, const char* entry, SwPlan* pl,
              long long* img_floats, long long* log_rows) {
    const int pwq = (pw + 3) / 4;
    int tile0 = 0;
    SwChunk cur{0, 0, 0, 0, true, 0, 0};
    auto flush = [&]() { if (cur.n_segs) pl->chunks.push_back(cur); cur = SwChunk{(int)pl->segs.size(), 0, 0, 0, true, 0, 0}; };
    for (int i = 0; i < n_images; ++i) {
        const ts2d_tiled_image& im = images[i];
        const int rows = im.n_tiles * pl->V;
        SwSeg sg{};
        sg.img_off = *img_floats; sg.out_off = pl->out_elems; sg.Hp = im.Hp; sg.Wp = im.Wp; sg.tile0 = tile0; sg.n_tiles = im.n_tiles; sg.image = i;
        const long long ablocks = blocks_of((long long)K * im.Hp * ((im.Wp + 3) / 4));
        if (rows > kSwChunkRows) {
            flush();
            for (int r0 = 0; r0 < rows; r0 += kSwChunkRows) {
                const int nb = std::min(kSwChunkRows, rows - r0);
                sg.row0 = r0; sg.n_rows = nb; sg.batch_row = 0; sg.log_row = 0; sg.gblock0 = 0; sg.ablock0 = 0;
                pl->segs.push_back(sg);
                cur.n_segs = 1; cur.rows = nb; cur.log_row = r0; cur.aggregate = r0 + nb == rows;
                cur.gblocks = (unsigned)blocks_of((long long)nb * C * ph * pwq); cur.ablocks = (unsigned)ablocks;
                flush();
            }
        } else {
            if (cur.rows + rows > kSwChunkRows) flush();
            sg.row0 = 0; sg.n_rows = rows; sg.batch_row = cur.rows; sg.log_row = cur.rows; sg.gblock0 = cur.gblocks; sg.ablock0 = cur.ablocks;
            pl->segs.push_back(sg);
            cur.n_segs++; cur.rows += rows;
            cur.gblocks += (unsigned)blocks_of((long long)rows * C * ph * pwq); cur.ablocks += (unsigned)ablocks;
        }
        pl->cap_rows = std::max(pl->cap_rows, std::min(rows, kSwChunkRows)); *log_rows = std::max<long long>(*log_rows, rows);
        tile0 += im.n_tiles;
        *img_floats += (long long)align_up((size_t)C * im.Hp * im.Wp, 64);
        pl->out_elems += (long long)align_up((size_t)K * im.Hp * im.Wp, 256);
    }
    flush();
    for (const SwChunk& c : pl->chunks) {
        pl->cap_rows = std::max(pl->cap_rows, c.rows);
        if ((long long)c.gblocks >= (1LL << 31) || (long long)c.ablocks >= (1LL << 31)) return fail(TS2D_ERR_INVALID, "%s: a chunk exceeds 2^31 blocks", entry);
    }
    *log_rows = std::max<long long>(*log_rows, pl->cap_rows);
    if (F > 1 && blocks_of(pl->out_elems >> 3) >= (1LL << 31)) return fail(TS2D_ERR_INVALID, "%s: the fold mean exceeds 2^31 blocks", entry);
    return TS2D_OK;
}

// The tail: one segment per image (its half logits are segs' out_off), the taps of its rows then of its columns.
// rs_elems: elements of the resampled uint8 outputs (the decided maps of a probabilities tail).
// A probabilities tail: beside every RsSeg goes a ProbSeg with the image's places in the float outputs (prob_elems) and in the decided maps
// (rs_elems); of runs a ProbStackSeg, the places being those of the image's slice in its run.
int plan_export(int K, const ts2d_tiled_image* images, const SwTail& tail, int n_images, const char* entry, SwPlan* pl, std::vector<RsTap>* rtaps,
                long long* rs_elems) {
    long long oo = 0;
    const int D = tail.decided_planes(K);
    // runs: the outputs of a run are [K][n_slices][full_h][full_w] (one contiguous piece per head), its taps are planned with its first slice
    // and every other slice's segment is that one at its own half planes and blocks
    for (int r = 0; r < tail.n_runs; ++r) {
        const ts2d_tiled_probabilities_run& rn = tail.runs[r];
        const long long fplane = (long long)rn.full_h * rn.full_w, run_plane = fplane * rn.n_slices;
        const size_t first = pl->rsegs.size();
        const long long oo_first = oo;
        for (int s = 0; s < rn.n_slices; ++s) {
            const int i = rn.first_image + s;
            pl->pssegs.push_back(ProbStackSeg{pl->prob_elems + s * fplane, *rs_elems + s * fplane, run_plane, run_plane, rn.full_h, rn.full_w, rn.box_y, rn.box_x});
            if (s == 0) {
                rs_plan_segment(tail, i, K, images[i].Hp, images[i].Wp, oo, &pl->rsegs, rtaps, &pl->rs_blocks, nullptr);
            } else {
                RsSeg rs = pl->rsegs[first];
                rs.src_off += oo - oo_first; rs.block0 = (unsigned)pl->rs_blocks;
                pl->rsegs.push_back(rs);
                pl->rs_blocks += blocks_of((long long)rn.full_h * ((rn.full_w + 3) / 4));
            }
            oo += (long long)align_up((size_t)K * images[i].Hp * images[i].Wp, 256);
        }
        pl->prob_elems += (long long)align_up((size_t)K * run_plane, 256);
        *rs_elems += (long long)align_up((size_t)D * run_plane, 256);
    }
    for (int i = 0; i < n_images && tail.kind != SwTail::kProbRuns; ++i) {
        rs_plan_segment(tail, i, K, images[i].Hp, images[i].Wp, oo, &pl->rsegs, rtaps, &pl->rs_blocks, rs_elems);
        if (tail.prob()) {
            const SwTail::Image& pd = tail.images[i];
            const size_t fplane = (size_t)pd.full_h * pd.full_w;
            pl->psegs.push_back(ProbSeg{pl->prob_elems, *rs_elems, pd.full_h, pd.full_w, pd.box_y, pd.box_x});
            pl->prob_elems += (long long)align_up((size_t)K * fplane, 256);
            *rs_elems += (long long)align_up((size_t)D * fplane, 256);
        }
        oo += (long long)align_up((size_t)K * images[i].Hp * images[i].Wp, 256);
    }
    if (pl->rs_blocks >= (1LL << 31)) return fail(TS2D_ERR_INVALID, "%s: the %s exceeds 2^31 blocks", entry, tail.what());
    return TS2D_OK;
}

}  // namespace

void rs_plan_segment(const SwTail& tail, int i, int K, int Hp, int Wp, long long src_off, std::vector<RsSeg>* rsegs, std::vector<RsTap>* rtaps,
                     long long* blocks, long long* rs_elems) {
    const SwTail::Image& ex = tail.images[(size_t)i];
    const bool labelmap = tail.kind != SwTail::kExport, full = tail.prob();
    const int planes = tail.planes(K);          // of the output: the label map is ONE plane, its lanes walk the K source planes
    RsSeg rs{};
    rs.src_off = src_off; rs.dst_off = full ? 0 : *rs_elems; rs.Hp = Hp; rs.Wp = Wp; rs.out_h = ex.out_h; rs.out_w = ex.out_w;
    rs.block0 = (unsigned)*blocks;
    if (labelmap && ex.out_h == ex.src_h && ex.out_w == ex.src_w) {      // the host route does not resample then: no taps, no weights
        rs.tap0 = -1; rs.src_off += (long long)ex.src_y * Wp + ex.src_x;
    } else {
        rs.tap0 = (int)rtaps->size();
        rtaps->resize(rtaps->size() + ex.out_h + ex.out_w);
        rs_axis_taps(ex.src_h, ex.out_h, ex.src_y, rtaps->data() + rs.tap0);
        rs_axis_taps(ex.src_w, ex.out_w, ex.src_x, rtaps->data() + rs.tap0 + ex.out_h);
    }
    rsegs->push_back(rs);
    if (full) { *blocks += blocks_of((long long)ex.full_h * ((ex.full_w + 3) / 4)); return; }      // (its outputs: the caller's ProbSeg)
    *blocks += blocks_of((long long)planes * ex.out_h * ((ex.out_w + 3) / 4));
    *rs_elems += (long long)align_up((size_t)planes * ex.out_h * ex.out_w, 256);
}

int plan_tiled(const ts2d_engine* e, int F, const ts2d_tiled_image* images, const SwTail& tail, int n_images, int ph, int pw, int mirror_mask,
               bool name_images, const char* entry, SwPlan* pl) {
    if (ph < 1 || pw < 1) return fail(TS2D_ERR_INVALID, "%s: bad patch %dx%d", entry, ph, pw);
    const int C = e->arch.input_channels, K = e->arch.num_classes;
    int vflip[4] = {0, 0, 0, 0};
    if ((mirror_mask & 3) == 3) { vflip[1] = 1; vflip[2] = 2; vflip[3] = 3; pl->V = 4; }
    else if (mirror_mask & 1) { vflip[1] = 1; pl->V = 2; }
    else if (mirror_mask & 2) { vflip[1] = 2; pl->V = 2; }
    pl->vflips = vflip[0] | (vflip[1] << 8) | (vflip[2] << 16) | (vflip[3] << 24);
    long long img_floats = 0, log_rows = 0, rs_elems = 0;
    std::vector<RsTap> rtaps;
    const bool regions = tail.class_order != nullptr, exports = tail.kind != SwTail::kNone;
    TRY(check_images(F, C, K, images, tail, n_images, ph, pw, name_images, entry, pl));
    TRY(pack_rows(F, C, K, images, n_images, ph, pw, entry, pl, &img_floats, &log_rows));
    if (exports) TRY(plan_export(K, images, tail, n_images, entry, pl, &rtaps, &rs_elems));
    // ---- the descriptor table and every tile origin
    const size_t n_tiles = (size_t)pl->n_tiles_all;
    pl->tab_segs = pl->segs.size() * sizeof(SwSeg); pl->tab_rsegs = align_up(pl->tab_segs + 2 * n_tiles * 4, 8);
    pl->tab_rtaps = pl->tab_rsegs + pl->rsegs.size() * sizeof(RsSeg);
    pl->tab_order = pl->tab_rtaps + rtaps.size() * sizeof(RsTap);
    pl->tab_psegs = align_up(pl->tab_order + (regions ? (size_t)K : 0), 8);
    pl->tab.resize(tail.prob() ? pl->tab_psegs + pl->psegs.size() * sizeof(ProbSeg) + pl->pssegs.size() * sizeof(ProbStackSeg) : pl->tab_order + (regions ? (size_t)K : 0));
    if (tail.kind == SwTail::kProbRuns) memcpy(pl->tab.data() + pl->tab_psegs, pl->pssegs.data(), pl->pssegs.size() * sizeof(ProbStackSeg));
    else if (tail.prob()) memcpy(pl->tab.data() + pl->tab_psegs, pl->psegs.data(), pl->psegs.size() * sizeof(ProbSeg));
    if (regions) memcpy(pl->tab.data() + pl->tab_order, tail.class_order, (size_t)K);      // (K == n_order: the entry has checked it)
    memcpy(pl->tab.data(), pl->segs.data(), pl->tab_segs);
    if (exports) {
        memcpy(pl->tab.data() + pl->tab_rsegs, pl->rsegs.data(), pl->rsegs.size() * sizeof(RsSeg));
        if (!rtaps.empty()) memcpy(pl->tab.data() + pl->tab_rtaps, rtaps.data(), rtaps.size() * sizeof(RsTap));      // (no taps: no pointer to copy from)
    }
    int32_t* ty = reinterpret_cast<int32_t*>(pl->tab.data() + pl->tab_segs); int32_t* tx = ty + n_tiles;
    for (int i = 0; i < n_images; ++i) {
        memcpy(ty, images[i].tile_y, (size_t)images[i].n_tiles * 4); memcpy(tx, images[i].tile_x, (size_t)images[i].n_tiles * 4);
        ty += images[i].n_tiles; tx += images[i].n_tiles;
    }
    // ---- the scratch (SwPlan names its parts)
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t o = off; off = align_up(off + bytes, 256); return o; };
    pl->o_tab = take(pl->tab.size()); pl->o_g = take((size_t)ph * pw * 2); pl->o_imgs = take((size_t)img_floats * 4);
    pl->o_batch = take((size_t)pl->cap_rows * C * ph * pw * 4); pl->o_log = take((size_t)log_rows * K * ph * pw * 4);
    pl->o_o16 = take(pl->any16 ? (size_t)F * pl->out_elems * 2 : 0); pl->o_seg = take(pl->anyseg ? (size_t)pl->out_elems : 0);
    pl->o_flag = take((size_t)F * n_images * 4);
    pl->o_rs8 = take(pl->any_rs8 ? (size_t)rs_elems : 0); pl->o_rs32 = take(pl->any_rs32 ? (size_t)rs_elems * 4 : 0);
    pl->o_prob = take((size_t)pl->prob_elems * 4);
    pl->bytes = off;
    return TS2D_OK;
}

}  // namespace ts2d
