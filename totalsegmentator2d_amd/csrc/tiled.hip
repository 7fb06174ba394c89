// The sliding window of libts2d_engine.so: tile gather, aggregation, the mean of an ensemble's folds and the TAIL of a call (SwTail,
// engine_internal.h: what becomes of the aggregated half logits - the export's resample-back, a label map, regions, probabilities), around
// the engine's forward (engine.hip: reserve_checked, run_forward).  The C entries ts2d_engine_predict_tiled*, ts2d_ensemble_predict_tiled_*
// (predict_tiled_impl, which runs the tail once: run_tail) and ts2d_{labelmap,regions,probabilities}_from_logits (tail_from_logits: the same
// run_tail on half planes of the caller's).
#include "engine_internal.h"
#include "entry_util.h"
#include "kernels_sw.h"
#include "kernels_fold.h"
#include "kernels_resample.h"
#include "kernels_labelmap.h"
#include "kernels_regions.h"
#include "kernels_prob.h"

#include <string>
#include <vector>

using namespace ts2d;

#pragma GCC visibility push(hidden)
namespace {

int name_fold(int rc, bool name_folds, int f) {
    if (rc == TS2D_OK || !name_folds) return rc;
    const std::string msg = last_error();
    return fail(rc, "fold %d: %s", f, msg.c_str());
}

// Where the tables and the outputs of a tail lie on the device, and the host's copy of the segments (the places of the outputs).
struct TailTables {
    const RsSeg* d_rsegs; const RsTap* d_rtaps; const uint8_t* d_order; const void* d_psegs;       // d_order: null without a class order
    uint8_t* d_rs8; float* d_rs32; float* d_prob;                                                  // d_rs8 / d_rs32: null where no image asks
    long long blocks;
    const RsSeg* rsegs; const ProbSeg* psegs; const ProbStackSeg* pssegs;
};

// THE tail: the one kernel of the tail's kind on the half logits d_o16, then that kind's device-to-host copies, all enqueued on `st`.
int run_tail(const SwTail& t, int K, const TailTables& tt, const __half* d_o16, hipStream_t st) {
    const int n = (int)t.images.size();
    const dim3 grid((unsigned)tt.blocks), block(256);
    switch (t.kind) {
    case SwTail::kNone: return TS2D_OK;
    case SwTail::kExport:
        hipLaunchKernelGGL(sw_resample_threshold, grid, block, 0, st, d_o16, tt.d_rsegs, n, K, tt.d_rtaps, tt.d_rs8, tt.d_rs32, kSigmoidHalfThreshold);
        break;
    case SwTail::kLabelmap: hipLaunchKernelGGL(sw_labelmap, grid, block, 0, st, d_o16, tt.d_rsegs, n, K, tt.d_rtaps, tt.d_rs8); break;
    case SwTail::kRegions:
        hipLaunchKernelGGL(sw_regions, grid, block, 0, st, d_o16, tt.d_rsegs, n, K, tt.d_rtaps, tt.d_order, tt.d_rs8, kSigmoidHalfThreshold);
        break;
    case SwTail::kProbRuns:                                   // (named before kProb: the order of the two instantiations in the code object)
        hipLaunchKernelGGL(sw_probabilities<ProbStackSeg>, grid, block, 0, st, d_o16, tt.d_rsegs, static_cast<const ProbStackSeg*>(tt.d_psegs), n, K,
                           tt.d_rtaps, t.mode, tt.d_order, tt.d_prob, tt.d_rs8, kSigmoidHalfThreshold);
        break;
    case SwTail::kProb:
        hipLaunchKernelGGL(sw_probabilities<ProbSeg>, grid, block, 0, st, d_o16, tt.d_rsegs, static_cast<const ProbSeg*>(tt.d_psegs), n, K, tt.d_rtaps,
                           t.mode, tt.d_order, tt.d_prob, tt.d_rs8, kSigmoidHalfThreshold);
        break;
    }
    HIP_TRY(hipGetLastError());
    const size_t D = (size_t)t.decided_planes(K);
    for (int r = 0; r < t.n_runs; ++r) {                      // (kProbRuns) a head of a run is one piece on both sides
        const ts2d_tiled_probabilities_run& rn = t.runs[r];
        const ProbStackSeg& ps = tt.pssegs[(size_t)rn.first_image];
        const size_t run_plane = (size_t)ps.prob_stride;
        for (int k = 0; k < K; ++k)
            HIP_TRY(hipMemcpyAsync(rn.prob_f32 + (long long)k * rn.prob_head_stride, tt.d_prob + ps.prob_off + (size_t)k * run_plane, run_plane * 4, hipMemcpyDeviceToHost, st));
        for (size_t k = 0; rn.decided_u8 && k < D; ++k)
            HIP_TRY(hipMemcpyAsync(rn.decided_u8 + (long long)k * rn.decided_head_stride, tt.d_rs8 + ps.dec_off + k * run_plane, run_plane, hipMemcpyDeviceToHost, st));
    }
    for (int i = 0; i < n && t.kind != SwTail::kProbRuns; ++i) {
        const SwTail::Image& ti = t.images[(size_t)i];
        if (t.kind == SwTail::kProb) {
            const size_t fplane = (size_t)ti.full_h * ti.full_w;
            HIP_TRY(hipMemcpyAsync(ti.f32, tt.d_prob + tt.psegs[i].prob_off, (size_t)K * fplane * 4, hipMemcpyDeviceToHost, st));
            if (ti.u8) HIP_TRY(hipMemcpyAsync(ti.u8, tt.d_rs8 + tt.psegs[i].dec_off, D * fplane, hipMemcpyDeviceToHost, st));
            continue;
        }
        const size_t ne = (size_t)t.planes(K) * ti.out_h * ti.out_w;
        if (ti.u8) HIP_TRY(hipMemcpyAsync(ti.u8, tt.d_rs8 + tt.rsegs[i].dst_off, ne, hipMemcpyDeviceToHost, st));
        if (ti.f32) HIP_TRY(hipMemcpyAsync(ti.f32, tt.d_rs32 + tt.rsegs[i].dst_off, ne * 4, hipMemcpyDeviceToHost, st));
    }
    return TS2D_OK;
}

// The sliding window of every C entry (include/ts2d_engine.h): N images as ONE engine batch; ts2d_engine_predict_tiled is N = 1.
// plan_tiled (tiled_plan.cpp) validates everything, packs the rows (tile x mirror variant) of the images into chunks of at most
// kSwChunkRows and lays the scratch out; here every host-to-device copy is enqueued, then per chunk one sw_gather, one forward and
// (where an image ends in the chunk) one sw_aggregate, then the tail and every device-to-host copy, ONE stream synchronise and the result check.
// `full` is the whole difference between the entries' results: the batch entry asks for the full-batch dispatch (a row's bits must not
// depend on its batch-mates), the single-image entry for the size-dependent one.  `name_images`: a message names the image it is about.
// `engines[0 .. F)` (the ts2d_ensemble_* entries; the others are F = 1): the folds of an ensemble, one after the other on
// the FIRST engine's stream and in its scratch - the chunk loop once per fold, sw_aggregate into the fold's own half slot and inf
// flags, then ONE sw_fold_mean (kernels_fold.h) into slot 0, on which the tail runs as it does on a single fold's logits.  Only
// the half slots and the flags exist F times.  `name_folds`: a fold's failed reserve or result check is reported as "fold <f>: ...".
int predict_tiled_impl(ts2d_engine* const* engines, int F, ts2d_tiled_image* images, const SwTail& tail, int n_images, int ph, int pw, int mirror_mask,
                       const uint16_t* gaussian_f16, bool full, bool name_images, bool name_folds, const char* entry) {
    ts2d_engine* e = engines[0];
    SwPlan pl;
    TRY(plan_tiled(e, F, images, tail, n_images, ph, pw, mirror_mask, name_images, entry, &pl));
    const int C = e->arch.input_channels, K = e->arch.num_classes, V = pl.V;
    for (int f = 0; f < F; ++f) TRY(name_fold(reserve_checked(engines[f], pl.cap_rows, ph, pw, full), name_folds, f));
    HIP_TRY(hipSetDevice(e->device));
    hipStream_t st = e->stream;
    if (pl.bytes > e->sw_bytes) {                             // grown before the first launch only
        HIP_TRY(hipStreamSynchronize(st));
        if (e->d_sw) { HIP_TRY(hipFree(e->d_sw)); e->d_sw = nullptr; e->sw_bytes = 0; }
        HIP_TRY(hipMalloc(reinterpret_cast<void**>(&e->d_sw), pl.bytes));
        e->sw_bytes = pl.bytes;
    }
    char* b = e->d_sw;
    const SwSeg* d_segs = reinterpret_cast<const SwSeg*>(b + pl.o_tab);
    const int* d_ty = reinterpret_cast<const int*>(b + pl.o_tab + pl.tab_segs); const int* d_tx = d_ty + pl.n_tiles_all;
    __half* d_g = reinterpret_cast<__half*>(b + pl.o_g); float* d_imgs = reinterpret_cast<float*>(b + pl.o_imgs);
    float* d_batch = reinterpret_cast<float*>(b + pl.o_batch); float* d_log = reinterpret_cast<float*>(b + pl.o_log);
    __half* d_o16 = pl.any16 ? reinterpret_cast<__half*>(b + pl.o_o16) : nullptr; uint8_t* d_seg = pl.anyseg ? reinterpret_cast<uint8_t*>(b + pl.o_seg) : nullptr;
    int* d_flag = reinterpret_cast<int*>(b + pl.o_flag);
    for (int i = 0; i < n_images; ++i) images[i].inf_flag = 0;
    HIP_TRY(hipMemcpyAsync(b + pl.o_tab, pl.tab.data(), pl.tab.size(), hipMemcpyHostToDevice, st));
    if (gaussian_f16) HIP_TRY(hipMemcpyAsync(d_g, gaussian_f16, (size_t)ph * pw * 2, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(d_flag, 0, (size_t)F * n_images * 4, st));
    {
        long long io = 0;
        for (int i = 0; i < n_images; ++i) {
            const size_t nf = (size_t)C * images[i].Hp * images[i].Wp;
            HIP_TRY(hipMemcpyAsync(d_imgs + io, images[i].image, nf * 4, hipMemcpyHostToDevice, st));
            io += (long long)align_up(nf, 64);
        }
    }
    for (int f = 0; f < F; ++f)
        for (size_t ci = 0; ci < pl.chunks.size(); ++ci) {
            const SwChunk& c = pl.chunks[ci];
            hipLaunchKernelGGL(sw_gather, dim3(c.gblocks), dim3(256), 0, st, d_imgs, d_segs + c.seg0, c.n_segs, C, ph, pw, V, pl.vflips, d_ty, d_tx, d_batch);
            HIP_TRY(hipGetLastError());
            TRY(run_forward(engines[f], d_batch, c.rows, ph, pw, d_log + (size_t)c.log_row * K * ph * pw, nullptr, st, ci == 0, full));
            if (!c.aggregate) continue;
            // (an ensemble's uint8 output is the predicate on the MEAN: sw_fold_mean writes it)
            hipLaunchKernelGGL(sw_aggregate, dim3(c.ablocks), dim3(256), 0, st, d_log, d_segs + c.seg0, c.n_segs, K, ph, pw, V, pl.vflips, d_ty, d_tx,
                               gaussian_f16 ? d_g : nullptr, d_o16 ? d_o16 + (size_t)f * pl.out_elems : nullptr, F > 1 ? nullptr : d_seg,
                               kSigmoidHalfThreshold, d_flag + (size_t)f * n_images, e->tile_half);
            HIP_TRY(hipGetLastError());
        }
    if (F > 1) {          // every slot up to the end of the last image (the alignment gaps between the images ride along unread)
        const long long n_mean = pl.segs.back().out_off + (long long)K * pl.segs.back().Hp * pl.segs.back().Wp;
        hipLaunchKernelGGL(sw_fold_mean, dim3((unsigned)(((n_mean >> 3) + (n_mean & 7) + 255) / 256)), dim3(256), 0, st, d_o16, pl.out_elems, F, n_mean,
                           d_seg, kSigmoidHalfThreshold);
        HIP_TRY(hipGetLastError());
    }
    const char* tab = b + pl.o_tab;
    TRY(run_tail(tail, K, TailTables{reinterpret_cast<const RsSeg*>(tab + pl.tab_rsegs), reinterpret_cast<const RsTap*>(tab + pl.tab_rtaps),
                                     tail.class_order ? reinterpret_cast<const uint8_t*>(tab + pl.tab_order) : nullptr, tab + pl.tab_psegs,
                                     pl.any_rs8 ? reinterpret_cast<uint8_t*>(b + pl.o_rs8) : nullptr, pl.any_rs32 ? reinterpret_cast<float*>(b + pl.o_rs32) : nullptr,
                                     reinterpret_cast<float*>(b + pl.o_prob), pl.rs_blocks, pl.rsegs.data(), pl.psegs.data(), pl.pssegs.data()},
                 d_o16, st));
    std::vector<int> flags((size_t)F * n_images, 0);
    HIP_TRY(hipMemcpyAsync(flags.data(), d_flag, (size_t)F * n_images * 4, hipMemcpyDeviceToHost, st));
    {
        long long oo = 0;
        for (int i = 0; i < n_images; ++i) {
            const size_t ne = (size_t)K * images[i].Hp * images[i].Wp;
            if (images[i].logits_f16) HIP_TRY(hipMemcpyAsync(images[i].logits_f16, d_o16 + oo, ne * 2, hipMemcpyDeviceToHost, st));
            if (images[i].seg_u8) HIP_TRY(hipMemcpyAsync(images[i].seg_u8, d_seg + oo, ne, hipMemcpyDeviceToHost, st));
            oo += (long long)align_up(ne, 256);
        }
    }
    HIP_TRY(hipStreamSynchronize(st));
    for (int f = 0; f < F; ++f) {         // upstream looks for inf in every fold's aggregated array, not in the mean
        engines[f]->tiled_inf = 0;
        for (int i = 0; i < n_images; ++i) {
            const int inf = flags[(size_t)f * n_images + i] != 0;
            images[i].inf_flag = f ? (images[i].inf_flag | inf) : inf;
            engines[f]->tiled_inf |= inf;
        }
    }
    for (int f = 0; f < F; ++f) TRY(name_fold(ts2d_engine_check(engines[f]), name_folds, f));
    return TS2D_OK;
}

// The prologue of every ensemble entry, before any device work: the handles, the image array, folds that differ where they must agree, the
// entry's own per-image descriptor array (`no_descs`: it is null).  *todo: the images to run (0: the call returns TS2D_OK and does nothing)
int check_folds(const char* entry, ts2d_engine* const* engines, int n_engines, const ts2d_tiled_image* images, int n_images, bool no_descs, int* todo) {
    if (!engines) return fail(TS2D_ERR_INVALID, "%s: %d engines at a null pointer", entry, n_engines);
    if (n_engines < 1 || n_engines > kMaxFolds) return fail(TS2D_ERR_INVALID, "%s: n_engines = %d is outside 1..%d", entry, n_engines, kMaxFolds);
    for (int f = 0; f < n_engines; ++f)
        if (!engines[f]) return fail(TS2D_ERR_INVALID, "%s: engine %d is null", entry, f);
    if (n_images < 0 || (n_images > 0 && !images)) return fail(TS2D_ERR_INVALID, "%s: %d images at a null pointer", entry, n_images);
    *todo = n_images;
    if (n_images == 0) return TS2D_OK;
    const ts2d_engine* e0 = engines[0];
    for (int f = 0; f < n_engines; ++f) {
        const ts2d_engine* e = engines[f];
        if (!e->weights_ready) return fail(TS2D_ERR_STATE, "%s: fold %d: weights not loaded", entry, f);
        if (e->device != e0->device) return fail(TS2D_ERR_INVALID, "%s: fold %d is on device %d, fold 0 on device %d", entry, f, e->device, e0->device);
        if (e->arch.input_channels != e0->arch.input_channels)
            return fail(TS2D_ERR_INVALID, "%s: fold %d has %d input channels, fold 0 has %d", entry, f, e->arch.input_channels, e0->arch.input_channels);
        if (e->arch.num_classes != e0->arch.num_classes)
            return fail(TS2D_ERR_INVALID, "%s: fold %d has num_classes %d, fold 0 has %d", entry, f, e->arch.num_classes, e0->arch.num_classes);
        if (e->precision != e0->precision)
            return fail(TS2D_ERR_INVALID, "%s: fold %d runs precision mode %d, fold 0 mode %d", entry, f, e->precision, e0->precision);
        if (e->tile_half != e0->tile_half)
            return fail(TS2D_ERR_INVALID, "%s: fold %d blends with tile dtype %d, fold 0 with %d", entry, f, e->tile_half, e0->tile_half);
    }
    if (no_descs) return fail(TS2D_ERR_INVALID, "%s: %d images at a null pointer", entry, n_images);
    return TS2D_OK;
}

// the tail of an export call (null: a call without one)
SwTail export_tail(const ts2d_tiled_export* exports, int n_images) {
    SwTail t(exports ? SwTail::kExport : SwTail::kNone, exports ? n_images : 0);
    for (size_t i = 0; i < t.images.size(); ++i) t.images[i] = SwTail::rect_of(exports[i], exports[i].seg_u8, exports[i].logits_f32);
    return t;
}

// the tail of a label-map or region call: ONE uint8 plane per image
SwTail one_plane_tail(SwTail::Kind kind, const ts2d_tiled_labelmap* maps, int n_images, const uint8_t* class_order) {
    SwTail t(kind, n_images);
    t.class_order = class_order;
    for (int i = 0; i < n_images; ++i) t.images[(size_t)i] = SwTail::rect_of(maps[i], maps[i].label_u8, nullptr);
    return t;
}

// what the *_from_logits entries refuse alike of their planes, rectangle and output extent
int check_from_logits(const char* entry, int K, int H, int W, const SwTail::Image& ex) {
    if (K < 1 || K > 256) return fail(TS2D_ERR_INVALID, "%s: %d heads outside 1 ... 256", entry, K);
    if (H < 1 || W < 1 || (long long)K * H * W >= (1LL << 31)) return fail(TS2D_ERR_INVALID, "%s: bad extent %d x %d x %d (2^31 elements at most)", entry, K, H, W);
    if (ex.src_h < 1 || ex.src_w < 1 || ex.src_y < 0 || ex.src_x < 0 || ex.src_h > H - ex.src_y || ex.src_w > W - ex.src_x)
        return fail(TS2D_ERR_INVALID, "%s: source rectangle %dx%d at (%d,%d) is empty or leaves the %dx%d image", entry, ex.src_h, ex.src_w, ex.src_y,
                    ex.src_x, H, W);
    if (ex.out_h < 1 || ex.out_w < 1) return fail(TS2D_ERR_INVALID, "%s: bad output extent %dx%d", entry, ex.out_h, ex.out_w);
    if ((long long)ex.out_h * ex.out_w >= (1LL << 31) || (long long)ex.out_h + ex.out_w >= (1LL << 26))
        return fail(TS2D_ERR_INVALID, "%s: %dx%d exceeds 2^31 output elements or 2^26 output rows + columns", entry, ex.out_h, ex.out_w);
    return TS2D_OK;
}

// The ts2d_*_from_logits entries: the tail of ONE image (t.images[0]; the entry has refused its null pointers) on half planes of the caller's.
int tail_from_logits(const char* entry, int device, const uint16_t* logits_f16, int K, int H, int W, const SwTail& t) {
    const SwTail::Image& ti = t.images[0];
    TRY(check_from_logits(entry, K, H, W, ti));
    if (t.prob()) {
        if (ti.full_h < 1 || ti.full_w < 1 || ti.box_y < 0 || ti.box_x < 0 || ti.out_h > ti.full_h - ti.box_y || ti.out_w > ti.full_w - ti.box_x)
            return fail(TS2D_ERR_INVALID, "%s: probabilities: the %dx%d output at (%d,%d) leaves the full extent %dx%d", entry, ti.out_h, ti.out_w, ti.box_y,
                        ti.box_x, ti.full_h, ti.full_w);
        if ((long long)K * ti.full_h * ti.full_w >= (1LL << 31))
            return fail(TS2D_ERR_INVALID, "%s: probabilities: %d x %dx%d exceeds 2^31 output elements", entry, K, ti.full_h, ti.full_w);
    }
    std::vector<RsSeg> segs; std::vector<RsTap> rtaps;
    long long blocks = 0, elems = 0;
    rs_plan_segment(t, 0, K, H, W, 0, &segs, &rtaps, &blocks, &elems);
    if (blocks >= (1LL << 31)) return fail(TS2D_ERR_INVALID, t.prob() ? "%s: the %s exceed 2^31 blocks" : "%s: the %s exceeds 2^31 blocks", entry, t.what());
    const ProbSeg ps{0, 0, ti.full_h, ti.full_w, ti.box_y, ti.box_x};
    HIP_TRY(hipSetDevice(device));
    const size_t n_src = (size_t)K * H * W, n_prob = t.prob() ? (size_t)K * ti.full_h * ti.full_w : 0;
    const size_t n_u8 = !ti.u8 ? 0 : t.prob() ? (size_t)t.decided_planes(K) * ti.full_h * ti.full_w : (size_t)elems;
    ArenaLayout lay;
    const size_t o_seg = lay.add(sizeof(RsSeg)), o_ps = lay.add(t.prob() ? sizeof(ProbSeg) : 0), o_taps = lay.add(rtaps.size() * sizeof(RsTap));
    const size_t o_order = lay.add(t.class_order ? (size_t)K : 0), o_src = lay.add(n_src * 2), o_prob = lay.add(n_prob * 4), o_u8 = lay.add(n_u8);
    DevMem d;
    HIP_TRY(d.alloc(lay.total()));
    HIP_TRY(hipMemcpy(d.as<char>(o_seg), segs.data(), sizeof(RsSeg), hipMemcpyHostToDevice));
    if (t.prob()) HIP_TRY(hipMemcpy(d.as<char>(o_ps), &ps, sizeof(ProbSeg), hipMemcpyHostToDevice));
    if (!rtaps.empty()) HIP_TRY(hipMemcpy(d.as<char>(o_taps), rtaps.data(), rtaps.size() * sizeof(RsTap), hipMemcpyHostToDevice));
    if (t.class_order) HIP_TRY(hipMemcpy(d.as<char>(o_order), t.class_order, (size_t)K, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d.as<char>(o_src), logits_f16, n_src * 2, hipMemcpyHostToDevice));
    TRY(run_tail(t, K, TailTables{d.as<const RsSeg>(o_seg), d.as<const RsTap>(o_taps), t.class_order ? d.as<const uint8_t>(o_order) : nullptr,
                                  d.as<const char>(o_ps), ti.u8 ? d.as<uint8_t>(o_u8) : nullptr, nullptr, d.as<float>(o_prob), blocks, segs.data(), &ps, nullptr},
                 d.as<const __half>(o_src), 0));
    HIP_TRY(hipStreamSynchronize(0));         // the outputs are the caller's (and `d` goes) when the entry returns
    return TS2D_OK;
}

// what the probabilities entries refuse of the mode and its class order (n_order: of an engine's call; the from_logits entry has none to check)
int check_prob_mode(const char* entry, int mode, int K, const uint8_t* class_order, const int* n_order = nullptr) {
    if (mode != kProbMultilabel && mode != kProbLabelmap && mode != kProbRegions)
        return fail(TS2D_ERR_INVALID, "%s: probabilities: unknown mode %d", entry, mode);
    if (mode == kProbRegions && !class_order) return fail(TS2D_ERR_INVALID, "%s: probabilities: the class order is null", entry);
    if (K < 1 || K > 256) return fail(TS2D_ERR_INVALID, "%s: probabilities: %d heads outside 1 ... 256", entry, K);      // (every mode: the twin's limit)
    if (n_order && mode == kProbRegions && *n_order != K)
        return fail(TS2D_ERR_INVALID, "%s: probabilities: %d class values for a model of %d heads", entry, *n_order, K);
    return TS2D_OK;
}

}  // namespace
#pragma GCC visibility pop

extern "C" {

int ts2d_engine_predict_tiled(ts2d_engine* e, const float* image, int Hp, int Wp, int ph, int pw, int n_tiles,
                              const int32_t* tile_y, const int32_t* tile_x, int mirror_mask, const uint16_t* gaussian_f16,
                              uint16_t* logits_f16, uint8_t* seg_u8) {
    if (!e || !image || !tile_y || !tile_x) return fail(TS2D_ERR_INVALID, "ts2d_engine_predict_tiled: null argument");
    if (!e->weights_ready) return fail(TS2D_ERR_STATE, "ts2d_engine_predict_tiled: weights not loaded");
    if (!logits_f16 && !seg_u8) return fail(TS2D_ERR_INVALID, "ts2d_engine_predict_tiled: both outputs are null");
    ts2d_tiled_image one{image, Hp, Wp, n_tiles, tile_y, tile_x, logits_f16, seg_u8, 0};
    return predict_tiled_impl(&e, 1, &one, SwTail(), 1, ph, pw, mirror_mask, gaussian_f16, kBySize, false, false, "ts2d_engine_predict_tiled");
}

int ts2d_engine_predict_tiled_batch(ts2d_engine* e, ts2d_tiled_image* images, int n_images, int ph, int pw, int mirror_mask,
                                    const uint16_t* gaussian_f16) {
    if (!e) return fail(TS2D_ERR_INVALID, "ts2d_engine_predict_tiled_batch: null engine");
    if (n_images < 0 || (n_images > 0 && !images)) return fail(TS2D_ERR_INVALID, "ts2d_engine_predict_tiled_batch: %d images at a null pointer", n_images);
    if (n_images == 0) return TS2D_OK;
    if (!e->weights_ready) return fail(TS2D_ERR_STATE, "ts2d_engine_predict_tiled_batch: weights not loaded");
    return predict_tiled_impl(&e, 1, images, SwTail(), n_images, ph, pw, mirror_mask, gaussian_f16, kFullBatch, true, false, "ts2d_engine_predict_tiled_batch");
}

int ts2d_engine_predict_tiled_export(ts2d_engine* e, ts2d_tiled_image* images, const ts2d_tiled_export* exports, int n_images, int ph, int pw,
                                     int mirror_mask, const uint16_t* gaussian_f16, int full_batch) {
    if (!e) return fail(TS2D_ERR_INVALID, "ts2d_engine_predict_tiled_export: null engine");
    if (n_images < 0 || (n_images > 0 && !(images && exports)))
        return fail(TS2D_ERR_INVALID, "ts2d_engine_predict_tiled_export: %d images at a null pointer", n_images);
    if (n_images == 0) return TS2D_OK;
    if (!e->weights_ready) return fail(TS2D_ERR_STATE, "ts2d_engine_predict_tiled_export: weights not loaded");
    return predict_tiled_impl(&e, 1, images, export_tail(exports, n_images), n_images, ph, pw, mirror_mask, gaussian_f16, full_batch ? kFullBatch : kBySize, true, false,
                              "ts2d_engine_predict_tiled_export");
}

int ts2d_ensemble_predict_tiled_export(ts2d_engine* const* engines, int n_engines, ts2d_tiled_image* images, const ts2d_tiled_export* exports,
                                       int n_images, int ph, int pw, int mirror_mask, const uint16_t* gaussian_f16, int full_batch) {
    static const char* entry = "ts2d_ensemble_predict_tiled_export";
    int todo = 0;
    TRY(check_folds(entry, engines, n_engines, images, n_images, false, &todo));
    if (!todo) return TS2D_OK;
    return predict_tiled_impl(engines, n_engines, images, export_tail(exports, n_images), n_images, ph, pw, mirror_mask, gaussian_f16, full_batch ? kFullBatch : kBySize,
                              true, true, entry);
}

int ts2d_ensemble_predict_tiled_labelmap(ts2d_engine* const* engines, int n_engines, ts2d_tiled_image* images, const ts2d_tiled_labelmap* labelmaps,
                                         int n_images, int ph, int pw, int mirror_mask, const uint16_t* gaussian_f16, int full_batch) {
    static const char* entry = "ts2d_ensemble_predict_tiled_labelmap";
    int todo = 0;
    TRY(check_folds(entry, engines, n_engines, images, n_images, !labelmaps, &todo));
    if (!todo) return TS2D_OK;
    return predict_tiled_impl(engines, n_engines, images, one_plane_tail(SwTail::kLabelmap, labelmaps, n_images, nullptr), n_images, ph, pw, mirror_mask,
                              gaussian_f16, full_batch ? kFullBatch : kBySize, true, true, entry);
}

int ts2d_ensemble_predict_tiled_regions(ts2d_engine* const* engines, int n_engines, ts2d_tiled_image* images, const ts2d_tiled_labelmap* maps,
                                        int n_images, int ph, int pw, int mirror_mask, const uint16_t* gaussian_f16, int full_batch,
                                        const uint8_t* class_order, int n_order) {
    static const char* entry = "ts2d_ensemble_predict_tiled_regions";
    int todo = 0;
    TRY(check_folds(entry, engines, n_engines, images, n_images, !maps, &todo));
    if (!todo) return TS2D_OK;
    if (!class_order) return fail(TS2D_ERR_INVALID, "%s: regions: the class order is null", entry);
    const int K = engines[0]->arch.num_classes;
    if (n_order != K) return fail(TS2D_ERR_INVALID, "%s: regions: %d class values for a model of %d heads", entry, n_order, K);
    if (K > 256) return fail(TS2D_ERR_INVALID, "%s: regions: %d heads outside 1 ... 256", entry, K);
    return predict_tiled_impl(engines, n_engines, images, one_plane_tail(SwTail::kRegions, maps, n_images, class_order), n_images, ph, pw, mirror_mask,
                              gaussian_f16, full_batch ? kFullBatch : kBySize, true, true, entry);
}

int ts2d_labelmap_from_logits(int device, const uint16_t* logits_f16, int K, int H, int W, const int32_t rect[4], int out_h, int out_w,
                              uint8_t* label_u8) {
    static const char* entry = "ts2d_labelmap_from_logits";
    if (!logits_f16 || !rect || !label_u8) return fail(TS2D_ERR_INVALID, "%s: null argument", entry);
    SwTail t(SwTail::kLabelmap, 1);
    t.images[0] = SwTail::Image{rect[0], rect[1], rect[2], rect[3], out_h, out_w, 0, 0, 0, 0, label_u8, nullptr};
    return tail_from_logits(entry, device, logits_f16, K, H, W, t);
}

int ts2d_regions_from_logits(int device, const uint16_t* logits_f16, int K, int H, int W, const int32_t rect[4], int out_h, int out_w,
                             const uint8_t* class_order, uint8_t* label_u8) {
    static const char* entry = "ts2d_regions_from_logits";
    if (!logits_f16 || !rect) return fail(TS2D_ERR_INVALID, "%s: null argument", entry);
    if (!class_order) return fail(TS2D_ERR_INVALID, "%s: regions: the class order is null", entry);
    if (!label_u8) return fail(TS2D_ERR_INVALID, "%s: regions: the output is null", entry);
    SwTail t(SwTail::kRegions, 1);
    t.class_order = class_order;
    t.images[0] = SwTail::Image{rect[0], rect[1], rect[2], rect[3], out_h, out_w, 0, 0, 0, 0, label_u8, nullptr};
    return tail_from_logits(entry, device, logits_f16, K, H, W, t);
}

int ts2d_ensemble_predict_tiled_probabilities(ts2d_engine* const* engines, int n_engines, ts2d_tiled_image* images,
                                              const ts2d_tiled_probabilities* probabilities, int n_images, int ph, int pw, int mirror_mask,
                                              const uint16_t* gaussian_f16, int full_batch, int mode, const uint8_t* class_order, int n_order) {
    static const char* entry = "ts2d_ensemble_predict_tiled_probabilities";
    int todo = 0;
    TRY(check_folds(entry, engines, n_engines, images, n_images, !probabilities, &todo));
    if (!todo) return TS2D_OK;
    TRY(check_prob_mode(entry, mode, engines[0]->arch.num_classes, class_order, &n_order));
    SwTail t(SwTail::kProb, n_images);
    t.mode = mode; t.class_order = mode == kProbRegions ? class_order : nullptr;
    for (int i = 0; i < n_images; ++i) t.images[(size_t)i] = SwTail::full_of(probabilities[i], probabilities[i].decided_u8, probabilities[i].prob_f32);
    return predict_tiled_impl(engines, n_engines, images, t, n_images, ph, pw, mirror_mask, gaussian_f16, full_batch ? kFullBatch : kBySize, true, true, entry);
}

int ts2d_ensemble_predict_tiled_probabilities_stack(ts2d_engine* const* engines, int n_engines, ts2d_tiled_image* images, int n_images,
                                                    const ts2d_tiled_probabilities_run* runs, int n_runs, int ph, int pw, int mirror_mask,
                                                    const uint16_t* gaussian_f16, int full_batch, int mode, const uint8_t* class_order, int n_order) {
    static const char* entry = "ts2d_ensemble_predict_tiled_probabilities_stack";
    int todo = 0;
    TRY(check_folds(entry, engines, n_engines, images, n_images, false, &todo));
    if (!todo) return TS2D_OK;
    if (!runs || n_runs < 1) return fail(TS2D_ERR_INVALID, "%s: %d runs at a null pointer", entry, n_runs);
    TRY(check_prob_mode(entry, mode, engines[0]->arch.num_classes, class_order, &n_order));
    // the runs cover the images once, in order; every image gets what the sibling entry's descriptor holds: its run's geometry, its own slice of the outputs
    SwTail t(SwTail::kProbRuns, n_images);
    t.mode = mode; t.class_order = mode == kProbRegions ? class_order : nullptr; t.runs = runs; t.n_runs = n_runs; t.run_of.resize((size_t)n_images);
    int next = 0;
    for (int r = 0; r < n_runs; ++r) {
        const ts2d_tiled_probabilities_run& rn = runs[r];
        if (rn.n_slices < 1) return fail(TS2D_ERR_INVALID, "%s: run %d: probabilities: %d slices", entry, r, rn.n_slices);
        if (rn.first_image > next)
            return fail(TS2D_ERR_INVALID, "%s: run %d: probabilities: begins at image %d and leaves a gap behind image %d", entry, r, rn.first_image, next - 1);
        if (rn.first_image < next)
            return fail(TS2D_ERR_INVALID, "%s: run %d: probabilities: begins at image %d and overlaps the run before it, which ends at image %d", entry, r,
                        rn.first_image, next - 1);
        if (rn.n_slices > n_images - next)
            return fail(TS2D_ERR_INVALID, "%s: run %d: probabilities: %d slices from image %d leave the call's %d images", entry, r, rn.n_slices, rn.first_image, n_images);
        if (!rn.prob_f32) return fail(TS2D_ERR_INVALID, "%s: run %d: probabilities: the output is null", entry, r);
        const bool extent = rn.full_h >= 1 && rn.full_w >= 1;         // (a bad one is refused below, with the image named, in the sibling's words)
        const long long fplane = extent ? (long long)rn.full_h * rn.full_w : 0;
        if (extent && rn.prob_head_stride < fplane * rn.n_slices)
            return fail(TS2D_ERR_INVALID, "%s: run %d: probabilities: head stride %lld is below %d slices of %dx%d", entry, r, (long long)rn.prob_head_stride,
                        rn.n_slices, rn.full_h, rn.full_w);
        if (extent && rn.decided_u8 && mode == kProbMultilabel && rn.decided_head_stride < fplane * rn.n_slices)
            return fail(TS2D_ERR_INVALID, "%s: run %d: probabilities: decided head stride %lld is below %d slices of %dx%d", entry, r,
                        (long long)rn.decided_head_stride, rn.n_slices, rn.full_h, rn.full_w);
        for (int s = 0; s < rn.n_slices; ++s) {
            const int i = next + s;
            if (images[i].Hp != images[next].Hp || images[i].Wp != images[next].Wp)
                return fail(TS2D_ERR_INVALID, "%s: run %d: image %d: probabilities: the padded extent %dx%d differs from %dx%d of the run's first image", entry, r, i,
                            images[i].Hp, images[i].Wp, images[next].Hp, images[next].Wp);
            t.images[(size_t)i] = SwTail::full_of(rn, rn.decided_u8 ? rn.decided_u8 + s * fplane : nullptr, rn.prob_f32 + s * fplane);
            t.run_of[(size_t)i] = r;
        }
        next += rn.n_slices;
    }
    if (next != n_images) return fail(TS2D_ERR_INVALID, "%s: probabilities: the %d runs end at image %d and leave a gap to the call's %d images", entry, n_runs, next - 1, n_images);
    return predict_tiled_impl(engines, n_engines, images, t, n_images, ph, pw, mirror_mask, gaussian_f16, full_batch ? kFullBatch : kBySize, true, true, entry);
}

int ts2d_probabilities_from_logits(int device, const uint16_t* logits_f16, int K, int H, int W, const int32_t rect[4], int out_h, int out_w,
                                   int full_h, int full_w, int box_y, int box_x, int mode, const uint8_t* class_order, float* prob_f32,
                                   uint8_t* decided_u8) {
    static const char* entry = "ts2d_probabilities_from_logits";
    if (!logits_f16 || !rect) return fail(TS2D_ERR_INVALID, "%s: null argument", entry);
    if (!prob_f32) return fail(TS2D_ERR_INVALID, "%s: probabilities: the output is null", entry);
    TRY(check_prob_mode(entry, mode, K, class_order));
    SwTail t(SwTail::kProb, 1);
    t.mode = mode; t.class_order = mode == kProbRegions ? class_order : nullptr;
    t.images[0] = SwTail::Image{rect[0], rect[1], rect[2], rect[3], out_h, out_w, full_h, full_w, box_y, box_x, decided_u8, prob_f32};
    return tail_from_logits(entry, device, logits_f16, K, H, W, t);
}

int ts2d_engine_tiled_inf_flag(const ts2d_engine* e) { return e ? (e->tiled_inf != 0) : 0; }

}  // extern "C"
