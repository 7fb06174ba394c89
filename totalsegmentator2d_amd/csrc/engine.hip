// libts2d_engine.so - host side of the MI355X-native 2-D U-Net engine + the C-ABI of include/ts2d_engine.h.
// Replaces the network-forward part of nnUNetPredictor (reference seam: ts2d/core/inference/prediction_worker.py:209,
// network built at ts2d/core/inference/nnu.py:164-165).  gfx950 only; no CPU fallback exists in this library.
// This unit is the network: workspace, launchers, forward, result check.  The sliding window around it is tiled.hip, the input side prep.hip.
#include "engine_internal.h"
#include "kernels.h"
#include "kernels_f16x3.h"
#include "kernels_f16x3_convt.h"
#include "kernels_h32.h"
#include "kernels_head.h"
#include "kernels_f16x3_one.h"
#include "kernels_f16x3_qp.h"
#include "kernels_first.h"
#include "kernels_res32.h"
#include "kernels_s2v2.h"
#include "kernels_s2v2p.h"
#include "kernels_upc.h"
#include "kernels_up0.h"
#include "kernels_upq.h"
#include "kernels_upc_h.h"
#include "kernels_upc_h2.h"
#include "kernels_resblock.h"

#include <atomic>
#include <cstdio>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <string>
#include <type_traits>
#include <vector>

using namespace ts2d;

namespace {

// Generation counter of runs inside caller-provided (shared) workspaces: every such run stamps the workspace header with a fresh token
// and remembers it; an engine whose token is no longer in the header knows that ANOTHER engine of the set has overwritten its
// activations since (ts2d_engine_debug_tensor / ts2d_engine_check must not read them as its own - ADVICE r4).
std::atomic<uint32_t> g_ws_generation{0};

int upload_weights(ts2d_engine* e, const float* blob, size_t n_floats) {
    // (pack_weights also records the per-layer split scale in the op table)
    if (n_floats != e->user_blob_floats)
        return fail(TS2D_ERR_INVALID, "weight blob has %zu floats, architecture needs %zu", n_floats, e->user_blob_floats);
    std::vector<float> staging, wide;
    try {
        staging.resize(e->weight_floats);
        if (e->padded) { expand_blob(e->user_arch, e->arch, e->residual ? e->n_blocks : nullptr, blob, wide); blob = wide.data(); }
    } catch (...) { return fail(TS2D_ERR_NOMEM, "host staging allocation failed"); }
    pack_weights(e, blob, staging.data());
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipMemcpy(e->d_weights, staging.data(), e->weight_floats * sizeof(float), hipMemcpyHostToDevice));
    e->weights_ready = true;
    return TS2D_OK;
}

// `full`: the run takes the full-batch dispatch whatever its size (ts2d_engine_predict_tiled_batch).  Its activation plan keeps the coarse
// tensor of every composed decoder entry alive until that entry has run; the plan of a small batch under "sbk" (transposed conv + conv)
// releases it one op earlier, so a layout made for such a batch cannot serve a full-dispatch run and is re-made here - inside the same
// memory when it fits (checked below, never assumed).  The reverse holds: a full-dispatch layout serves every "sbk" run of the same or a
// smaller batch (the upsampled tensor of its two-kernel entries goes to the d_up scratch, as for any batch below the reserved one), so
// the layout stays and a following predict_tiled / forward finds it unchanged.
// What this reuse rests on - a buffer for every output, no live tensor overwritten, side regions that hold what their kernels touch - is
// checked for every admitted (layout, run) pair of a sweep on the CPU (tests/test_workspace_plan_cpu.py, W1-W3) and run at a few pairs on
// the card (tests/test_gpu_workspace_reuse.py).
int ensure_workspace(ts2d_engine* e, int B, int H, int W, bool full) {
    const bool keep = e->keep_activations;
    if (e->d_ws && e->wsB >= B && e->wsH == H && e->wsW == W && e->ws_precision == e->precision && e->ws_keep == keep && (e->ws_full || !full)) return TS2D_OK;
    HIP_TRY(hipSetDevice(e->device));
    if (e->d_ws && e->wsH == H && e->wsW == W && e->wsB > B && !e->ws_external) B = e->wsB;      // same geometry, another mode: keep the larger batch capacity
    const WsLayout L = workspace_layout(e, B, H, W, full);
    if (e->d_ws) {      // the old workspace may still be in use by a run on ANY stream: wait for its end-of-run event
        if (e->ws_busy) { HIP_TRY(hipEventSynchronize(e->ws_event)); e->ws_busy = false; }
        HIP_TRY(hipStreamSynchronize(e->stream));
    }
    if (e->ws_external) {      // caller-provided memory (ts2d_engine_set_workspace): never allocated or freed here
        if (e->ws_bytes < L.bytes)
            return fail(TS2D_ERR_NOMEM, "the workspace given to ts2d_engine_set_workspace holds %zu bytes, B=%d H=%d W=%d needs %zu "
                        "(ts2d_engine_workspace_bytes)", e->ws_bytes, B, H, W, L.bytes);
    } else {
        if (e->d_ws && e->ws_bytes < L.bytes) { HIP_TRY(hipFree(e->d_ws)); e->d_ws = nullptr; e->ws_bytes = 0; }      // (a mode change that fits re-maps the same memory)
        if (!e->d_ws) { HIP_TRY(hipMalloc(reinterpret_cast<void**>(&e->d_ws), L.bytes)); e->ws_bytes = L.bytes; }
    }
    e->wsB = B; e->wsH = H; e->wsW = W; e->ws_precision = e->precision; e->ws_keep = keep; e->ws_full = full;
    for (size_t i = 0; i < e->tensors.size(); ++i) {
        Tensor& t = e->tensors[i];
        t.data = L.plan.used[i] ? reinterpret_cast<float*>(e->d_ws + L.plan.off[i]) : nullptr;
        t.resident = L.plan.used[i] && !L.plan.reused[i];
        t.bytes = L.plan.used[i] ? L.plan.size[i] : 0;
        t.scale = t.normed ? reinterpret_cast<float*>(e->d_ws + L.o_sc[i]) : nullptr;
        t.shift = t.normed ? reinterpret_cast<float*>(e->d_ws + L.o_sh[i]) : nullptr;
    }
    e->d_part = reinterpret_cast<float*>(e->d_ws + L.o_part);
    e->d_partial = reinterpret_cast<float*>(e->d_ws + L.o_pk);
    e->d_up = L.has_up ? reinterpret_cast<float*>(e->d_ws + L.o_up) : nullptr;
    return TS2D_OK;
}

// Staging memory of the HOST-buffer forward (input, logits, masks of one batch): allocated on the first such call only - a caller
// that passes device pointers (the bench, the multi-GPU stream, SubModelSet) never pays for it (1.3 GB at B = 64, K = 18).
int ensure_staging(ts2d_engine* e, int B, int H, int W) {
    const int K = e->arch.num_classes;
    size_t off = 0;
    const size_t o_in = off; off = align_up(off + (size_t)B * e->arch.input_channels * H * W * sizeof(float), 256);
    const size_t o_lg = off; off = align_up(off + (size_t)B * K * H * W * sizeof(float), 256);
    const size_t o_mk = off; off = align_up(off + (size_t)B * K * H * ((W + 31) / 32) * sizeof(uint32_t), 256);
    if (off > e->stage_bytes) {
        HIP_TRY(hipSetDevice(e->device));
        if (e->ws_busy) { HIP_TRY(hipEventSynchronize(e->ws_event)); e->ws_busy = false; }
        HIP_TRY(hipStreamSynchronize(e->stream));
        if (e->d_stage) { HIP_TRY(hipFree(e->d_stage)); e->d_stage = nullptr; e->stage_bytes = 0; }
        HIP_TRY(hipMalloc(reinterpret_cast<void**>(&e->d_stage), off));
        e->stage_bytes = off;
    }
    e->d_in_stage = reinterpret_cast<float*>(e->d_stage + o_in);
    e->d_logit_stage = reinterpret_cast<float*>(e->d_stage + o_lg);
    e->d_mask_stage = reinterpret_cast<uint32_t*>(e->d_stage + o_mk);
    return TS2D_OK;
}

// (the profiled name is op + suffix: put together only when profiling - a forward at B = 1 is 62 launches in 1.9 ms)
int prof_begin(ts2d_engine* e, const std::string& op, const char* suffix, hipStream_t st) {
    if (!e->profiling) return TS2D_OK;
    const std::string name = op + suffix;
    if (e->n_launched >= e->launches.size()) {
        Launch l; l.name = name;
        HIP_TRY(hipEventCreate(&l.e0)); HIP_TRY(hipEventCreate(&l.e1));
        e->launches.push_back(l);
    }
    e->launches[e->n_launched].name = name;
    e->launches[e->n_launched].kernel.clear();
    e->launches[e->n_launched].ksplit = 1;
    HIP_TRY(hipEventRecord(e->launches[e->n_launched].e0, st));
    return TS2D_OK;
}
// which kernel served the op being profiled (ts2d_engine_op_kernel): called between prof_begin and prof_end
void prof_kernel(ts2d_engine* e, const char* kernel) {
    if (e->profiling && e->n_launched < e->launches.size()) e->launches[e->n_launched].kernel = kernel;
}
// ... and the split-K factor it ran with (ts2d_engine_op_ksplit)
void prof_ksplit(ts2d_engine* e, int ksplit) {
    if (e->profiling && e->n_launched < e->launches.size()) e->launches[e->n_launched].ksplit = ksplit;
}
int prof_end(ts2d_engine* e, hipStream_t st) {
    if (!e->profiling) return TS2D_OK;
    HIP_TRY(hipEventRecord(e->launches[e->n_launched].e1, st));
    e->n_launched++;
    return TS2D_OK;
}

// ------------------------------------------------------------------------------------------------------------------ launching
// hipFuncAttributeMaxDynamicSharedMemorySize is a per-DEVICE property of a kernel: one process may drive engines on several GPUs
// (include/ts2d_engine.h: handles are independent), so the "already set" state is a bit per device, not one flag per process.
inline hipError_t allow_max_lds(const void* kern, std::atomic<uint64_t>& done) {
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    const uint64_t bit = 1ull << (dev & 63);
    if (done.load(std::memory_order_acquire) & bit) return hipSuccess;
    e = hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    if (e == hipSuccess) done.fetch_or(bit, std::memory_order_release);
    return e;
}

// A kernel instantiation that may ask for more dynamic LDS than the default limit: owns the per-device bits of ITS attribute, then launches.
template <auto KERN, typename... A>
hipError_t launch_max_lds(dim3 grid, dim3 block, size_t smem, hipStream_t st, const A&... args) {
    static std::atomic<uint64_t> done{0};
    if (hipError_t e = allow_max_lds(reinterpret_cast<const void*>(KERN), done); e != hipSuccess) return e;
    hipLaunchKernelGGL(KERN, grid, block, smem, st, args...);
    return hipGetLastError();
}
// ... and one that stays below it
template <auto KERN, typename... A>
hipError_t launch_kernel(dim3 grid, dim3 block, size_t smem, hipStream_t st, const A&... args) {
    hipLaunchKernelGGL(KERN, grid, block, smem, st, args...);
    return hipGetLastError();
}

// Storage type of the activations and the fp16 products per value that go with it: (float, 3) in the fp32 modes, (_Float16, 1) in the 16-bit
// mode.  with_storage(f16, f) calls the generic f with the tag of the run - the one place where the run's storage type picks an instantiation.
template <typename ST, int NP> struct Storage { using type = ST; static constexpr int np = NP; };
template <typename F> auto with_storage(bool f16, F&& f) { return f16 ? f(Storage<_Float16, 1>{}) : f(Storage<float, 3>{}); }

// What a forward runs on: the caller's tensors, the batch, the stream and the storage type of the precision mode
struct Run { const float* d_in; float* d_logits; uint32_t* d_mask; int B, H, W; hipStream_t st; bool f16; };

int hip_failed(const Op& op, hipError_t le) { return fail(TS2D_ERR_HIP, "launch of %s failed: %s", op.name.c_str(), hipGetErrorString(le)); }

// ConvArgs fields that describe the pixel tiling / the (tile, column tile) grid
inline void set_tiling(ConvArgs& ca, const TileGeom& g, int n_ctiles) {
    ca.TH = g.TH; ca.TW = g.TW; ca.NIMG = g.NIMG; ca.lgTH = g.lgTH; ca.lgTW = g.lgTW;
    ca.inv_tw = 1.0f / (float)g.TW; ca.inv_thw = 1.0f / (float)(g.TH * g.TW);
    ca.tiles_x = g.tiles_x; ca.tiles_y = g.tiles_y; ca.n_mtiles = g.n_mtiles; ca.n_ctiles = n_ctiles;
    auto magic = [](int d) { return d <= 1 ? 0u : (unsigned)((0x100000000ull + (unsigned)d - 1) / (unsigned)d); };
    ca.mg_tx = magic(g.tiles_x); ca.mg_tpi = magic(g.tiles_x * g.tiles_y);
    ca.PH = g.PH; ca.PW = g.PW;
}

unsigned long long* prof_slots(const ts2d_engine* e, size_t oi) { return (e->dbg == 256 && e->d_prof) ? e->d_prof + 512 * oi : nullptr; }

// ---- first block (kernels_first.h): reads the NCHW boundary tensor
int launch_first(ts2d_engine* e, size_t oi, const Choice& c, const Run& r) {
    const Op& op = e->ops[oi];
    const TileGeom& g = c.g;
    FirstArgs fa{};
    fa.x = r.d_in; fa.w = e->d_weights + op.dev_wraw; fa.bias = e->d_weights + op.dev_b; fa.dst = e->tensors[op.dst].data;
    fa.part = c.fused_stats ? e->d_part : nullptr;
    fa.B = r.B; fa.C = op.cin; fa.H = r.H; fa.W = r.W; fa.Cout = op.cout;
    fa.lgTH = g.lgTH; fa.lgTW = g.lgTW; fa.lgNIMG = ilog2(g.NIMG); fa.tiles_x = g.tiles_x; fa.tiles_y = g.tiles_y;
    fa.n_mtiles = g.n_mtiles; fa.PH = g.PH; fa.PW = g.PW;
    const int kp = (op.cin + 1) / 2, nt = op.cout / 32, P = g.PH * g.PW * g.NIMG;
    size_t smem = std::max((size_t)P * (2 * kp + 1) * sizeof(float), (size_t)4 * op.cout * 4 * sizeof(float));
    if (r.f16 && c.first_full && nt == 1) {          // per-wave transpose regions of the 16-byte-store epilogue (kernels_first.h)
        fa.tr_off = (int)align_up(smem, 16);
        smem = fa.tr_off + 4 * kFirstTr;
    }
    const bool stats_only = c.k == K_FIRST_STATS;      // the block is recomputed inside the second one (implies first_full, nt == 1, kp == 1)
    if (stats_only && !(c.first_full && c.fused_stats)) return fail(TS2D_ERR_INVALID, "internal: fused first block on a geometry without complete tiles");
    if (c.first_split) smem = (size_t)first_split_lds(P, r.f16 && !stats_only);
    // complete one-image 256-pixel tiles everywhere: persistent workgroups (4 per CU) with the next tile's patch in flight
    const dim3 grid(c.first_full ? std::min(g.n_mtiles, e->num_cus * (nt == 1 ? 4 : 2)) : g.n_mtiles), block(kBlock);
    bool served = true;
    const hipError_t launch = with_storage(r.f16, [&](auto s) {
        using ST = typename decltype(s)::type;
        if (c.first_split) return stats_only ? launch_kernel<conv3x3_first_split<ST, false>>(grid, block, smem, r.st, fa)
                                             : launch_kernel<conv3x3_first_split<ST, true>>(grid, block, smem, r.st, fa);
        if (stats_only) return launch_kernel<conv3x3_first<1, 1, ST, true, false>>(grid, block, smem, r.st, fa);
        const bool full = c.first_full;
        if (nt == 1 && kp == 1) return full ? launch_kernel<conv3x3_first<1, 1, ST, true>>(grid, block, smem, r.st, fa) : launch_kernel<conv3x3_first<1, 1, ST, false>>(grid, block, smem, r.st, fa);
        if (nt == 1 && kp == 2) return full ? launch_kernel<conv3x3_first<1, 2, ST, true>>(grid, block, smem, r.st, fa) : launch_kernel<conv3x3_first<1, 2, ST, false>>(grid, block, smem, r.st, fa);
        if (nt == 2 && kp == 1) return full ? launch_kernel<conv3x3_first<2, 1, ST, true>>(grid, block, smem, r.st, fa) : launch_kernel<conv3x3_first<2, 1, ST, false>>(grid, block, smem, r.st, fa);
        if (nt == 2 && kp == 2) return full ? launch_kernel<conv3x3_first<2, 2, ST, true>>(grid, block, smem, r.st, fa) : launch_kernel<conv3x3_first<2, 2, ST, false>>(grid, block, smem, r.st, fa);
        served = false;
        return hipSuccess;
    });
    if (!served) return fail(TS2D_ERR_INVALID, "first block: unsupported Cout %d / Cin %d", op.cout, op.cin);
    if (stats_only) e->fused_away[0] = 1;
    HIP_TRY(launch);
    return TS2D_OK;
}

// ---- decoder entry composed with its transposed conv (kernels_upc.h, _upq.h, _upc_h.h, _upc_h2.h; level 0: kernels_up0.h)
int launch_up0(ts2d_engine* e, size_t oi, const Choice& c, const Run& r) {
    // persistent, resident skip weights, 16x16x32 transposed product
    const Op& op = e->ops[oi]; const Op& up = e->ops[op.up_idx];
    const Tensor& xc = e->tensors[up.src]; const Tensor& sk = e->tensors[op.skip];
    const float* wts = e->d_weights;
    Up0Args u0{};
    u0.xc = xc.data; u0.scc = xc.scale; u0.shc = xc.shift; u0.xs = sk.data; u0.scs = sk.scale; u0.shs = sk.shift;
    u0.wc0 = wts + op.dev_w0c; u0.wk0 = wts + op.dev_w0k; u0.bvar = wts + op.dev_bvar; u0.oscale = wts + op.dev_wcs;
    u0.dst = e->tensors[op.dst].data; u0.part = e->d_part;
    u0.B = r.B; u0.H = r.H >> op.ly; u0.W = r.W >> op.lx; u0.tiles_x = c.g.tiles_x; u0.tiles_y = c.g.tiles_y; u0.n_tiles = c.g.n_mtiles;
    u0.slope = e->arch.leaky_slope;
    u0.prof = prof_slots(e, oi);
    u0.seg = c.seg;
    const hipError_t launch = with_storage(r.f16, [&](auto s) {
        using S = decltype(s);
        const size_t smem = 9 * (S::np == 3 ? 2 : 1) * 4 * 512 + 8 * kResPS;      // resident skip weights (hi, lo in the fp32 modes) + patch planes
        return launch_max_lds<conv3x3_up0<typename S::type, S::np>>(dim3(u0.n_tiles / u0.seg), dim3(kBlock), smem, r.st, u0);
    });
    HIP_TRY(launch);
    return TS2D_OK;
}

int launch_composed(ts2d_engine* e, size_t oi, const Choice& c, const Run& r) {
    if (c.k == K_UP0) return launch_up0(e, oi, c, r);
    const Op& op = e->ops[oi]; const Op& up = e->ops[op.up_idx];
    const Tensor& xc = e->tensors[up.src]; const Tensor& sk = e->tensors[op.skip];
    const TileGeom& g = c.g;
    const float* wts = e->d_weights;
    const int bn = c.bn;
    UpcArgs ua{};
    ua.xc = xc.data; ua.scc = xc.scale; ua.shc = xc.shift; ua.Cb = up.cin;
    ua.xs = sk.data; ua.scs = sk.scale; ua.shs = sk.shift; ua.Cs = op.cin_skip;
    ua.wc = wts + op.dev_wc; ua.wk = wts + op.dev_wk; ua.bvar = wts + op.dev_bvar; ua.oscale = wts + op.dev_wcs;
    ua.dst = e->tensors[op.dst].data; ua.part = e->d_part;
    ua.B = r.B; ua.H = r.H >> op.ly; ua.W = r.W >> op.lx; ua.Cout = op.cout;
    ua.tiles_x = g.tiles_x; ua.tiles_y = g.tiles_y; ua.n_mtiles = g.n_mtiles; ua.n_ctiles = op.cout / bn;
    ua.TH = g.TH; ua.TW = g.TW; ua.inv_twc = 1.0f / (float)(g.TW / 2);
    ua.slope = e->arch.leaky_slope;
    ua.prof = prof_slots(e, oi); ua.dbg = e->dbg;
    const dim3 grid((ua.n_mtiles + 7) / 8 * 8 * ua.n_ctiles), block(kBlock);
    const bool b64 = bn == 64, flex = c.flex;       // flex: extent-following tile (the level is no multiple of 8 x 32): masked, division-addressed instance
    hipError_t launch;
    if (c.k == K_UPC_H2) {             // 16-bit mode on 16 x 32 tiles: four M tiles per wave, skip-half weights by DMA
        launch = c.ks == 4 ? launch_max_lds<conv3x3_upc_h2<4>>(grid, block, kUh2Lds, r.st, ua) : launch_max_lds<conv3x3_upc_h2<2>>(grid, block, kUh2Lds, r.st, ua);
    } else if (c.k == K_UPC_H) {       // 16-bit mode: fp16 storage, one product
        const size_t smem = std::max((size_t)c.ks * 2 * kUcPlane, (size_t)4 * kUsPlane + (size_t)2 * 9 * 2 * bn * 16);
        auto inst = [&](auto bn_, auto ks_) {
            constexpr int BN = decltype(bn_)::value, KS = decltype(ks_)::value;
            return flex ? launch_max_lds<conv3x3_upc_h<BN, KS, true>>(grid, block, smem, r.st, ua) : launch_max_lds<conv3x3_upc_h<BN, KS>>(grid, block, smem, r.st, ua);
        };
        using I32 = std::integral_constant<int, 32>; using I64 = std::integral_constant<int, 64>;
        using K2 = std::integral_constant<int, 2>; using K4 = std::integral_constant<int, 4>;
        launch = b64 ? (c.ks == 4 ? inst(I64{}, K4{}) : inst(I64{}, K2{})) : (c.ks == 4 ? inst(I32{}, K4{}) : inst(I32{}, K2{}));
    } else if (c.k == K_UPQ) {         // 16 x 32 tiles, one 512-thread workgroup per CU, double-buffered staging
        launch = launch_max_lds<conv3x3_upq>(grid, dim3(kUqThreads), kUqLds, r.st, ua);
    } else {
        const size_t smem = std::max((size_t)8 * kUcPlane, (size_t)4 * kUsPlane + (size_t)9 * 4 * bn * 16);
        if (b64) launch = flex ? launch_max_lds<conv3x3_upc<64, true>>(grid, block, smem, r.st, ua) : launch_max_lds<conv3x3_upc<64, false>>(grid, block, smem, r.st, ua);
        else launch = flex ? launch_max_lds<conv3x3_upc<32, true>>(grid, block, smem, r.st, ua) : launch_max_lds<conv3x3_upc<32, false>>(grid, block, smem, r.st, ua);
    }
    HIP_TRY(launch);
    return TS2D_OK;
}

// ---- 32 -> 32 stride-1 block with the layer's weights resident in LDS (kernels_res32.h)
int launch_res32(ts2d_engine* e, size_t oi, const Choice& c, const Run& r) {
    const Op& op = e->ops[oi];
    const Tensor& src = e->tensors[op.src];
    const float* wts = e->d_weights;
    Res32Args ra{};
    ra.src = src.data; ra.sc = src.scale; ra.sh = src.shift; ra.wres = wts + op.dev_wres; ra.bias = wts + op.dev_b;
    ra.oscale = wts + op.dev_ws; ra.dst = e->tensors[op.dst].data; ra.part = e->d_part;
    ra.B = r.B; ra.H = r.H >> op.ly; ra.W = r.W >> op.lx; ra.tiles_x = c.g.tiles_x; ra.tiles_y = c.g.tiles_y; ra.n_tiles = c.g.n_mtiles;
    ra.slope = e->arch.leaky_slope;
    ra.prof = prof_slots(e, oi);
    ra.seg = c.seg;
    const bool fuse0 = c.k == K_S1_RES32F;       // the first block was a statistics-only pass: recompute it here
    if (fuse0) {
        if (!e->fused_away[0]) return fail(TS2D_ERR_INVALID, "internal: fused second block without the statistics-only first pass");
        const Op& o0 = e->ops[0];
        ra.src = nullptr; ra.x0 = r.d_in; ra.C0 = o0.cin; ra.w0 = wts + o0.dev_wraw; ra.b0 = wts + o0.dev_b;
    }
    const dim3 grid(ra.n_tiles / ra.seg), block(kBlock);
    const hipError_t launch = with_storage(r.f16, [&](auto s) {
        using S = decltype(s); using ST = typename S::type;
        const size_t smem = S::np == 3 ? 9 * 2 * 4 * 512 + 8 * kResPS : 9 * 4 * 512 + 4 * kResPS + 1536;
        return fuse0 ? launch_max_lds<conv3x3_res32<ST, S::np, true>>(grid, block, smem, r.st, ra) : launch_max_lds<conv3x3_res32<ST, S::np, false>>(grid, block, smem, r.st, ra);
    });
    HIP_TRY(launch);
    return TS2D_OK;
}

// ---- head (kernels_head.h, kernels.h head_1x1)
int launch_head(ts2d_engine* e, size_t oi, const Choice& c, const Run& r) {
    const Op& op = e->ops[oi];
    const Tensor& src = e->tensors[op.src];
    const float* wts = e->d_weights;
    HeadArgs ha{};
    ha.src = src.data; ha.sc = src.scale; ha.sh = src.shift; ha.w = wts + op.dev_w; ha.bias = wts + op.dev_b;
    ha.logits = r.d_logits; ha.mask = r.d_mask; ha.C = src.C; ha.K = op.cout; ha.HW = r.H * r.W;
    ha.total = (long long)r.B * r.H * r.W; ha.slope = e->arch.leaky_slope; ha.nonfinite = e->d_flags;
    if (c.k == K_HEAD_MFMA) {      // matrix-core head (split / f16 modes)
        ha.wph = wts + op.dev_wh; ha.oscale = wts + op.dev_ws;
        const int bpw = 16;          // (4 ... 128 measured: 16 is as good as any - fewer, longer waves lose DRAM locality)
        const long long nblk = ha.total / 32;
        const dim3 grid((unsigned)((nblk + 4 * bpw - 1) / (4 * bpw)));
        const hipError_t launch = with_storage(r.f16, [&](auto s) { using S = decltype(s); return launch_kernel<head_mfma32<typename S::type, S::np>>(grid, dim3(256), 0, r.st, ha, bpw); });
        HIP_TRY(launch);
        return TS2D_OK;
    }
    const dim3 grid((unsigned)((ha.total + 255) / 256));
    const size_t smem = ((size_t)256 * (src.C + 1) + (size_t)op.cout * src.C + op.cout) * sizeof(float);
    const hipError_t launch = with_storage(r.f16, [&](auto s) {
        using ST = typename decltype(s)::type;
        return src.C == 32 ? launch_max_lds<head_1x1<32, ST>>(grid, dim3(256), smem, r.st, ha) : launch_max_lds<head_1x1<64, ST>>(grid, dim3(256), smem, r.st, ha);
    });
    HIP_TRY(launch);
    return TS2D_OK;
}

// ---- residual blocks (kernels_resblock.h): the skip path's pooled 1x1 projection and the join
int launch_proj(ts2d_engine* e, size_t oi, const Choice& c, const Run& r) {
    const Op& op = e->ops[oi];
    const Tensor& src = e->tensors[op.src];
    ProjArgs pa{};
    pa.src = src.data; pa.sc = src.scale; pa.sh = src.shift; pa.w = e->d_weights + op.dev_w; pa.wh = e->d_weights + op.dev_wh; pa.dst = e->tensors[op.dst].data;
    pa.part = c.fused_stats ? e->d_part : nullptr;
    pa.Cin = src.C; pa.Cout = op.cout; pa.sy = op.sy; pa.sx = op.sx;
    pa.Wt = r.W >> op.lx; pa.HW = (r.H >> op.ly) * pa.Wt; pa.Win = r.W >> src.lx; pa.M = r.B * pa.HW;
    pa.slope = e->arch.leaky_slope; pa.inv_n = 1.0f / (float)(op.sy * op.sx);
    if (!src.normed || src.linear || src.C % 32 || op.cout % c.bn || (r.H >> src.ly) != (r.H >> op.ly) * op.sy || pa.Win != pa.Wt * op.sx)
        return fail(TS2D_ERR_INVALID, "internal: op %s: source of the projection is not an activated tensor of %d x the output's extent", op.name.c_str(), op.sy * op.sx);
    if (c.fused_stats && (pa.HW % kProjBM || c.g.tiles_x != pa.HW / kProjBM))
        return fail(TS2D_ERR_INVALID, "internal: op %s: partial statistics on tiles that span images", op.name.c_str());
    const dim3 grid((unsigned)((pa.M + kProjBM - 1) / kProjBM), op.cout / c.bn), block(256);
    if (c.half != r.f16) return fail(TS2D_ERR_INVALID, "internal: op %s: the plan's storage is not the run's", op.name.c_str());
    if (r.f16) HIP_TRY(c.bn == 64 ? launch_kernel<pool_proj1x1_h<64>>(grid, block, 0, r.st, pa) : launch_kernel<pool_proj1x1_h<32>>(grid, block, 0, r.st, pa));
    else HIP_TRY(c.bn == 64 ? launch_kernel<pool_proj1x1<64>>(grid, block, 0, r.st, pa) : launch_kernel<pool_proj1x1<32>>(grid, block, 0, r.st, pa));
    return TS2D_OK;
}

int launch_join(ts2d_engine* e, size_t oi, const Choice& c, const Run& r) {
    const Op& op = e->ops[oi];
    const Tensor& c2 = e->tensors[op.src]; const Tensor& rs = e->tensors[op.res]; const Tensor& dst = e->tensors[op.dst];
    JoinArgs ja{};
    ja.raw2 = c2.data; ja.sc2 = c2.scale; ja.sh2 = c2.shift; ja.r = rs.data; ja.scr = rs.scale; ja.shr = rs.shift;
    ja.dst = dst.data; ja.dsc = dst.scale; ja.dsh = dst.shift;
    ja.linear = rs.linear ? 1 : 0; ja.sy = op.sy; ja.sx = op.sx;
    ja.Wt = r.W >> op.lx; ja.HW = (r.H >> op.ly) * ja.Wt; ja.Win = r.W >> rs.lx; ja.C = op.cout; ja.npix = r.B * ja.HW;
    ja.slope = e->arch.leaky_slope; ja.inv_n = 1.0f / (float)(op.sy * op.sx);
    if (!c2.normed || !rs.normed || c2.C != op.cout || rs.C != op.cout || op.cout % 32 || (r.H >> rs.ly) != (r.H >> op.ly) * op.sy || ja.Win != ja.Wt * op.sx ||
        (rs.linear && (op.sy != 1 || op.sx != 1)))
        return fail(TS2D_ERR_INVALID, "internal: op %s: the join's sources do not match its output", op.name.c_str());
    if (c.half != r.f16) return fail(TS2D_ERR_INVALID, "internal: op %s: the plan's storage is not the run's", op.name.c_str());
    if (r.f16 && op.cout > 2048) return fail(TS2D_ERR_INVALID, "op %s: the 16-bit join serves at most 2048 channels", op.name.c_str());
    // fp32 storage: 32 pixels x 32 channels per block; fp16 storage: 256 / (C / 8) whole pixels per block (a lane owns 16 bytes of a pixel)
    const int ppb = r.f16 ? 256 / (op.cout / 8) : 32;
    const dim3 grid((unsigned)((ja.npix + ppb - 1) / ppb), r.f16 ? 1 : op.cout / 32), block(256);
    HIP_TRY(with_storage(r.f16, [&](auto s) { return launch_kernel<res_join<typename decltype(s)::type>>(grid, block, 0, r.st, ja); }));
    return TS2D_OK;
}

// ---- every kernel that takes ConvArgs
// The generic implicit-GEMM kernel: the whole exact mode (fp32 storage), and - in every mode - the stages whose stride is neither
// (1, 1) nor (2, 2) (f16 = fp16 storage with the 16-bit mode's operand rounding).
template <int TAPS, int SY, int SX, int CK, int EPI, typename ST = float>
hipError_t launch_exact_bn(bool b64, const ConvArgs& a, dim3 grid, size_t smem, hipStream_t st) {
    return b64 ? launch_max_lds<conv_mfma_f32<TAPS, SY, SX, CK, 64, EPI, ST>>(grid, dim3(kBlock), smem, st, a)
               : launch_max_lds<conv_mfma_f32<TAPS, SY, SX, CK, 32, EPI, ST>>(grid, dim3(kBlock), smem, st, a);
}
hipError_t launch_exact(int taps, int sy, int sx, int ck, int bn, bool f16, const ConvArgs& a, dim3 grid, size_t smem, hipStream_t st) {
    const bool b64 = bn == 64;
    if (bn != 32 && bn != 64) return hipErrorInvalidConfiguration;
    if (taps == 9 && sy == 1 && sx == 1 && !f16) {
        if (ck == 16) return launch_exact_bn<9, 1, 1, 16, 0>(b64, a, grid, smem, st);
        if (ck == 8) return launch_exact_bn<9, 1, 1, 8, 0>(b64, a, grid, smem, st);
    }
    if (taps == 9 && sy == 2 && sx == 2 && ck == 8 && !f16) return launch_exact_bn<9, 2, 2, 8, 0>(b64, a, grid, smem, st);
    if (taps == 9 && sy == 2 && sx == 1 && ck == 8) return f16 ? launch_exact_bn<9, 2, 1, 8, 0, _Float16>(b64, a, grid, smem, st) : launch_exact_bn<9, 2, 1, 8, 0>(b64, a, grid, smem, st);
    if (taps == 9 && sy == 1 && sx == 2 && ck == 8) return f16 ? launch_exact_bn<9, 1, 2, 8, 0, _Float16>(b64, a, grid, smem, st) : launch_exact_bn<9, 1, 2, 8, 0>(b64, a, grid, smem, st);
    if (taps == 1 && ck == 16)       // transposed conv, kernel = stride = (a.KA, a.KB)
        return f16 ? launch_exact_bn<1, 1, 1, 16, 1, _Float16>(b64, a, grid, smem, st) : launch_exact_bn<1, 1, 1, 16, 1>(b64, a, grid, smem, st);
    return hipErrorInvalidConfiguration;
}

// One (tile, column tile) workgroup per grid entry, K slices along grid.y: conv3x3_f16x3(_one), conv3x3s2_f16x3(_one), conv3x3_h32
hipError_t launch_tiled(Kern k, bool f16, int bn, int P, const ConvArgs& a, int grid_x, size_t smem, hipStream_t st) {
    const dim3 grid(grid_x, a.ksplit), block(kBlock);
    const bool b64 = bn == 64;
    if (bn != 32 && bn != 64) return hipErrorInvalidConfiguration;
    switch (k) {
    case K_S1_ONE:           // tile inside one image: lean staging path (BN = 32: 3 workgroups per CU, no room for the prefetched scale/shift)
        return b64 ? launch_max_lds<conv3x3_f16x3_one<64, true>>(grid, block, smem, st, a) : launch_max_lds<conv3x3_f16x3_one<32, false>>(grid, block, smem, st, a);
    case K_S1_H32:           // fp16 storage: 32-channel chunks, one product
        return b64 ? launch_max_lds<conv3x3_h32<64, 6>>(grid, block, smem, st, a) : launch_max_lds<conv3x3_h32<32, 6>>(grid, block, smem, st, a);
    default: break;
    }
    return with_storage(f16, [&](auto s) {
        using S = decltype(s); using ST = typename S::type;
        if (k == K_S2_ONE)       // (measured: prefetching the scale/shift vectors or double-buffering the fragments costs registers and gains nothing here)
            return b64 ? launch_max_lds<conv3x3s2_f16x3_one<64, false, false, ST, S::np>>(grid, block, smem, st, a)
                       : launch_max_lds<conv3x3s2_f16x3_one<32, false, false, ST, S::np>>(grid, block, smem, st, a);
        if (k == K_S1_GENERIC) {
            if (P * 2 <= 3 * kBlock)      // units per thread of the staging loop (2-chunk prefetch measured slower)
                return b64 ? launch_max_lds<conv3x3_f16x3<64, 3, 1, ST, S::np>>(grid, block, smem, st, a) : launch_max_lds<conv3x3_f16x3<32, 3, 1, ST, S::np>>(grid, block, smem, st, a);
            return b64 ? launch_max_lds<conv3x3_f16x3<64, 5, 1, ST, S::np>>(grid, block, smem, st, a) : launch_max_lds<conv3x3_f16x3<32, 5, 1, ST, S::np>>(grid, block, smem, st, a);
        }
        if (k == K_S2_GENERIC) {
            if (P <= 5 * kBlock)
                return b64 ? launch_max_lds<conv3x3s2_f16x3<64, 5, ST, S::np>>(grid, block, smem, st, a) : launch_max_lds<conv3x3s2_f16x3<32, 5, ST, S::np>>(grid, block, smem, st, a);
            return b64 ? launch_max_lds<conv3x3s2_f16x3<64, 6, ST, S::np>>(grid, block, smem, st, a) : launch_max_lds<conv3x3s2_f16x3<32, 6, ST, S::np>>(grid, block, smem, st, a);
        }
        return hipErrorInvalidConfiguration;
    });
}

// conv3x3s2_v2 (kernels_s2v2.h): persistent, one workgroup per CU walks its tiles; every chunk's weights resident in LDS when they fit beside the patch
hipError_t launch_s2v2(const ts2d_engine* e, const Choice& c, bool f16, const ConvArgs& ca, int grid_x, hipStream_t st) {
    const size_t wchunk = s2v2_wchunk(c);
    const bool resw = s2v2_resident(c);
    const dim3 grid(std::min(grid_x, 8 * ca.n_ctiles * std::max(1, e->num_cus / (8 * ca.n_ctiles)))), block(kS2Threads);
    const size_t smem = (size_t)c.npp * 2 * kS2Plane + (resw ? (size_t)c.nch : 1) * wchunk;
    if (c.s2p) return launch_max_lds<conv3x3s2_v2p>(grid, block, kS2pLds, st, ca);      // two patch buffers, weights from L2 (dispatch.cpp: s2v2_variant)
    auto inst = [&](auto bn_, auto s, auto k32_) {
        using S = decltype(s); using ST = typename S::type;
        constexpr int BN = decltype(bn_)::value; constexpr bool K32 = decltype(k32_)::value;
        if (resw) return c.flex ? launch_max_lds<conv3x3s2_v2<BN, ST, S::np, true, true, K32>>(grid, block, smem, st, ca)
                                : launch_max_lds<conv3x3s2_v2<BN, ST, S::np, true, false, K32>>(grid, block, smem, st, ca);
        return c.flex ? launch_max_lds<conv3x3s2_v2<BN, ST, S::np, false, true, K32>>(grid, block, smem, st, ca)
                      : launch_max_lds<conv3x3s2_v2<BN, ST, S::np, false, false, K32>>(grid, block, smem, st, ca);
    };
    using B128 = std::integral_constant<int, 128>; using B64 = std::integral_constant<int, 64>;
    using H1 = Storage<_Float16, 1>; using F3 = Storage<float, 3>;
    if (c.bn == 128) return c.k32 ? inst(B128{}, H1{}, std::true_type{}) : f16 ? inst(B128{}, H1{}, std::false_type{}) : inst(B128{}, F3{}, std::false_type{});
    return c.k32 ? inst(B64{}, H1{}, std::true_type{}) : f16 ? inst(B64{}, H1{}, std::false_type{}) : inst(B64{}, F3{}, std::false_type{});
}

// 16-bit mode, plain C -> C block on 16 x 32 tiles: the skip phase of conv3x3_upc_h2 (four M tiles per wave, weights by LDS-DMA)
hipError_t launch_h2(ts2d_engine* e, const Op& op, const Choice& c, const Run& r) {
    const Tensor& src = e->tensors[op.src];
    const float* wts = e->d_weights;
    UpcArgs ua{};
    ua.xs = src.data; ua.scs = src.scale; ua.shs = src.shift; ua.Cs = src.C;
    ua.wk = wts + op.dev_wp; ua.bvar = wts + op.dev_b; ua.oscale = wts + op.dev_ws;
    ua.dst = e->tensors[op.dst].data; ua.part = e->d_part;
    ua.B = r.B; ua.H = r.H >> op.ly; ua.W = r.W >> op.lx; ua.Cout = op.cout;
    ua.tiles_x = c.g.tiles_x; ua.tiles_y = c.g.tiles_y; ua.n_mtiles = c.g.n_mtiles; ua.n_ctiles = op.cout / 64;
    ua.slope = e->arch.leaky_slope; ua.dbg = e->dbg;
    return launch_max_lds<conv3x3_upc_h2<4, false>>(dim3((ua.n_mtiles + 7) / 8 * 8 * ua.n_ctiles), dim3(kBlock), kUh2Lds, r.st, ua);
}

int launch_conv_family(ts2d_engine* e, size_t oi, const Choice& c, const Run& r) {
    const Op& op = e->ops[oi];
    const Tensor& src = e->tensors[op.src];
    const TileGeom& g = c.g;
    const float* wts = e->d_weights;
    const bool conv = op.type == OP_CONV;
    const int Hin = r.H >> src.ly, Win = r.W >> src.lx;
    const int Ht = conv ? (r.H >> op.ly) : Hin, Wt = conv ? (r.W >> op.lx) : Win;
    const int taps = conv ? 9 : 1, bn = c.bn;
    ConvArgs ca{};
    ca.ksplit = 1; ca.dbg = e->dbg; ca.prof = prof_slots(e, oi);
    ca.src0 = src.data; ca.sc0 = src.scale; ca.sh0 = src.shift; ca.C0 = src.C;
    if (op.skip >= 0) { const Tensor& sk = e->tensors[op.skip]; ca.src1 = sk.data; ca.sc1 = sk.scale; ca.sh1 = sk.shift; ca.C1 = sk.C; }
    ca.wp = wts + op.dev_w; ca.bias = wts + op.dev_b; ca.dst = e->tensors[op.dst].data;
    ca.part = (conv && c.fused_stats) ? e->d_part : nullptr;
    ca.B = r.B; ca.Hin = Hin; ca.Win = Win; ca.Ht = Ht; ca.Wt = Wt;
    ca.KA = conv ? 1 : op.sy; ca.KB = conv ? 1 : op.sx;
    ca.N = conv ? op.cout : op.sy * op.sx * op.cout; ca.Cout = op.cout;
    set_tiling(ca, g, ca.N / bn);
    ca.slope = e->arch.leaky_slope;
    const int P = g.PH * g.PW * g.NIMG;
    const int grid = (g.n_mtiles + 7) / 8 * 8 * ca.n_ctiles;
    hipError_t le = hipSuccess;
    switch (c.k) {
    case K_S2_V2:
        ca.wph = wts + op.dev_w2; ca.oscale = wts + op.dev_ws;
        le = launch_s2v2(e, c, r.f16, ca, grid, r.st);
        break;
    case K_T_ONE: case K_T_GENERIC: {
        ca.wph = wts + op.dev_wh; ca.oscale = wts + op.dev_ws;
        const size_t smem = (size_t)2 * g.TH * g.TW * g.NIMG * kRec + (size_t)2 * 64 * kRec;
        le = with_storage(r.f16, [&](auto s) {
            using S = decltype(s); using ST = typename S::type;
            return c.k == K_T_ONE ? launch_kernel<convT2x2_f16x3_one<ST, S::np>>(dim3(grid), dim3(kBlock), smem, r.st, ca)
                                  : launch_kernel<convT2x2_f16x3<64, ST, S::np>>(dim3(grid), dim3(kBlock), smem, r.st, ca);
        });
        break;
    }
    case K_S1_H2:
        le = launch_h2(e, op, c, r);
        break;
    case K_S1_QP: {
        // complete 16 x 32 tiles x 64 columns, normalised sources: one 512-thread workgroup per CU, patch and weights
        // double-buffered (weights by LDS-DMA), one barrier per chunk
        ca.wph = wts + op.dev_wp; ca.oscale = wts + op.dev_ws;
        const int gridp = std::min(grid, 8 * ca.n_ctiles * std::max(1, e->num_cus / (8 * ca.n_ctiles)));     // one persistent workgroup per CU
        le = launch_max_lds<conv3x3_f16x3_qp>(dim3(gridp), dim3(kQThreads), kQpLds, r.st, ca);
        break;
    }
    default: {
        const bool s2 = op.stride == 2;
        size_t smem = std::max((size_t)(((P * (op.ck + 4) + 3) & ~3) + taps * (op.ck / 8) * bn * 8) * sizeof(float),
                               (size_t)4 * bn * 4 * sizeof(float));
        if (c.k != K_EXACT) {
            smem = !s2 ? (size_t)P * kRec + (size_t)9 * bn * kRec : (size_t)P * kRec8 + (size_t)5 * bn * kRec;
            smem = std::max(smem, (size_t)4 * bn * 4 * sizeof(float));
            ca.wph = wts + (c.k == K_S1_H32 ? op.dev_wh32 : op.dev_wh); ca.oscale = wts + op.dev_ws;
        }
        if (c.ksplit > 1) {
            ca.ksplit = c.ksplit; ca.kslice_stride = (long long)r.B * Ht * Wt * op.cout;
            ca.dst = e->d_partial; ca.part = nullptr;
        }
        if (smem > 160 * 1024) return fail(TS2D_ERR_INVALID, "op %s: LDS tile of %zu bytes exceeds 160 KiB", op.name.c_str(), smem);
        if (c.k == K_EXACT) {      // the whole exact mode; in every mode the stages whose stride is neither (1, 1) nor (2, 2)
            const bool aniso = conv ? op.stride == 3 : op.stride != 2;
            le = launch_exact(taps, conv ? op.sy : 1, conv ? op.sx : 1, op.ck, bn, r.f16 && aniso, ca, dim3(grid), smem, r.st);
        } else le = launch_tiled(c.k, r.f16, bn, P, ca, grid, smem, r.st);
        break;
    }
    }
    if (le != hipSuccess) return hip_failed(op, le);
    return TS2D_OK;
}

// ---- InstanceNorm scale / shift of a conv's output: the launches of an op end with it.  Three sources - the partials a kernel's epilogue left per
// tile (fused_stats), the K slices of a split-K conv (reduced to the output on the way), or the output itself.
int launch_stats(ts2d_engine* e, size_t oi, const Choice& c, const Run& r) {
    const Op& op = e->ops[oi];
    Tensor& dst = e->tensors[op.dst];
    const float* wts = e->d_weights;
    const float *bias = wts + op.dev_b, *gamma = wts + op.dev_g, *beta = wts + op.dev_be;
    const float eps = e->arch.norm_eps;
    const int B = r.B, C = op.cout, HW = (r.H >> op.ly) * (r.W >> op.lx);
    const hipStream_t st = r.st;
    const dim3 per_image(B, C / 32);
    int ntiles = 0;           // per-tile partials in d_part that finalize_stats_t combines
    TRY(prof_begin(e, op.name, ".stats", st)); prof_kernel(e, "finalize_stats");
    with_storage(r.f16, [&](auto s) {
        using ST = typename decltype(s)::type;
        ST* out = reinterpret_cast<ST*>(dst.data);
        const long long stride = (long long)B * HW * C;      // of a K slice
        if (c.ksplit > 1 && HW == 256)            // one block of 32 pixel lanes per (image, 32 channels): output + scale / shift in one launch
            hipLaunchKernelGGL((splitk_reduce_stats<ST, 32>), per_image, dim3(1024), 0, st, e->d_partial, c.ksplit, stride, bias, C, HW, gamma, beta, eps, out, dst.scale, dst.shift);
        else if (c.ksplit > 1 && HW % 256 == 0 && HW > 256) {
            // images of >= 256 pixels (the small-batch rule): one block per 256 pixels writes the output and a shifted partial, finalize_stats
            // combines them - the one-block-per-image kernel below would walk the image 8 pixels per memory round trip
            ntiles = HW / 256;
            hipLaunchKernelGGL(splitk_reduce_part<ST>, dim3(ntiles, C / 32, B), dim3(256), 0, st, e->d_partial, c.ksplit, stride, bias, C, HW, out, e->d_part);
        } else if (c.ksplit > 1)
            hipLaunchKernelGGL(splitk_reduce_stats<ST>, per_image, dim3(256), 0, st, e->d_partial, c.ksplit, stride, bias, C, HW, gamma, beta, eps, out, dst.scale, dst.shift);
        else if (c.fused_stats) ntiles = c.g.tiles_x * c.g.tiles_y * c.ppt;      // the tile-lane count depends on the layer geometry only (never on B)
        else hipLaunchKernelGGL(stats_direct<ST>, per_image, dim3(256), 0, st, out, C, HW, gamma, beta, eps, dst.scale, dst.shift);
        return 0;
    });
    // (8-channel blocks - four times the grid for the 32- / 64-channel levels - measured no faster: 13.2 vs 12.5 us)
    if (ntiles >= 128) hipLaunchKernelGGL(finalize_stats_t<32>, per_image, dim3(1024), 0, st, e->d_part, ntiles, C, B, HW, gamma, beta, eps, dst.scale, dst.shift);
    else if (ntiles) hipLaunchKernelGGL(finalize_stats_t<8>, per_image, dim3(256), 0, st, e->d_part, ntiles, C, B, HW, gamma, beta, eps, dst.scale, dst.shift);
    HIP_TRY(hipGetLastError());
    return prof_end(e, st);
}

// A transposed conv that runs on its own although the workspace's plan (made for the reserved batch) composed it away: its output goes to the
// scratch region (small batches, composed_kernel; one such tensor is alive at a time - it is read by the very next op only)
int place_uncomposed_ups(ts2d_engine* e, const std::vector<Choice>& plan, int B, int H, int W) {
    for (size_t oi = 0; oi < e->ops.size(); ++oi) {
        const Op& op = e->ops[oi];
        if (op.type != OP_CONVT || plan[oi].k == K_FUSED_AWAY) continue;
        Tensor& t = e->tensors[op.dst];
        if (t.data != nullptr && t.data != e->d_up) {
            if ((size_t)B * (H >> t.ly) * (W >> t.lx) * t.C * sizeof(float) > t.bytes)
                return fail(TS2D_ERR_STATE, "internal: op %s writes more than its buffer in the workspace plan holds", op.name.c_str());
            continue;
        }
        if (!e->d_up || (size_t)B * (H >> t.ly) * (W >> t.lx) * t.C > kSbkElems / 2)
            return fail(TS2D_ERR_STATE, "internal: op %s has no output buffer in the workspace plan", op.name.c_str());
        t.data = e->d_up; t.resident = false;
    }
    return TS2D_OK;
}

int launch_op(ts2d_engine* e, size_t oi, const Choice& c, const Run& r) {
    switch (c.k) {
    case K_FIRST: case K_FIRST_STATS: return launch_first(e, oi, c, r);
    case K_UP0: case K_UPQ: case K_UPC: case K_UPC_H: case K_UPC_H2: return launch_composed(e, oi, c, r);
    case K_S1_RES32: case K_S1_RES32F: return launch_res32(e, oi, c, r);
    case K_HEAD_MFMA: case K_HEAD_1X1: return launch_head(e, oi, c, r);
    case K_PROJ: return launch_proj(e, oi, c, r);
    case K_JOIN: return launch_join(e, oi, c, r);
    default: return launch_conv_family(e, oi, c, r);
    }
}

// The forward: per op the kernel the plan names (dispatch.cpp decides, nothing here reads an option), then the statistics of its output
int run_forward_impl(ts2d_engine* e, const float* d_in, int B, int H, int W, float* d_logits, uint32_t* d_mask, hipStream_t st, bool full) {
    e->n_launched = 0;
    e->fused_away.assign(e->ops.size(), 0);
    // (the input is scanned by ts2d_engine_check only when it lives in the engine's own staging memory)
    e->last_input = ((e->d_in_stage && d_in == e->d_in_stage) || (e->d_sw && reinterpret_cast<const char*>(d_in) >= e->d_sw &&
                                               reinterpret_cast<const char*>(d_in) < e->d_sw + e->sw_bytes)) ? d_in : nullptr;
    e->lastB = B; e->lastH = H; e->lastW = W; e->last_stream = st; e->last_full = full;
    const bool f16 = e->precision == TS2D_PRECISION_F16;      // fp16 storage, one fp16 MFMA product, fp32 accumulate/statistics
    e->last_f16 = f16;
    const Run r{d_in, d_logits, d_mask, B, H, W, st, f16};
    if (f16 && !e->ops[0].first_direct) return fail(TS2D_ERR_INVALID, "fp16 mode needs <= 4 input channels");
    if (!e->ops[0].first_direct) {   // boundary layout change NCHW -> NHWC (channels zero-padded to 8); > 4 input channels only
        const long long total = (long long)B * H * W;
        TRY(prof_begin(e, "input.nhwc", "", st));
        prof_kernel(e, "nchw_to_nhwc_pad");
        hipLaunchKernelGGL(nchw_to_nhwc_pad, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st,
                           d_in, e->arch.input_channels, H * W, total, e->cin_pad, e->tensors[0].data);
        HIP_TRY(hipGetLastError());
        TRY(prof_end(e, st));
    }
    const std::vector<Choice>& plan = planned(e, B, H, W, full);
    TRY(place_uncomposed_ups(e, plan, B, H, W));
    for (size_t oi = 0; oi < e->ops.size(); ++oi) {
        const Op& op = e->ops[oi];
        const Choice& c = plan[oi];
        if (c.k == K_NONE && e->residual && !e->use_resf16)      // (the option was cleared with the mode still set: no silent change of mode)
            return fail(TS2D_ERR_INVALID, "op %s: TS2D_PRECISION_F16 is not supported on a residual-encoder engine", op.name.c_str());
        if (c.k == K_NONE) return fail(TS2D_ERR_INVALID, "op %s has no fp16 kernel (channel counts must be multiples of 16)", op.name.c_str());
        if (c.k == K_FUSED_AWAY) { e->fused_away[oi] = 1; continue; }      // composed into the next block (kernels_upc.h): the upsampled tensor is never materialised
        TRY(prof_begin(e, op.name, "", st));
        prof_kernel(e, c.name);
        if (c.ksplit > 1) prof_ksplit(e, c.ksplit);
        TRY(launch_op(e, oi, c, r));
        TRY(prof_end(e, st));
        if (op.type == OP_CONV || op.type == OP_PROJ) TRY(launch_stats(e, oi, c, r));
    }
    return TS2D_OK;
}

// Order this run after the previous user of the workspace if that one ran on a different stream.
int workspace_acquire(ts2d_engine* e, hipStream_t st) {
    if (e->ws_busy && e->ws_stream != st) HIP_TRY(hipStreamWaitEvent(st, e->ws_event, 0));
    return TS2D_OK;
}
int workspace_release(ts2d_engine* e, hipStream_t st) {
    HIP_TRY(hipEventRecord(e->ws_event, st));
    e->ws_stream = st; e->ws_busy = true;
    return TS2D_OK;
}

// clear_flags: first batch of a call.  The non-finite flag is cleared HERE, behind workspace_acquire: the previous run's head kernel
// (possibly on another stream) sets it with atomicOr, and a memset issued before the stream is ordered behind that run could wipe
// or pre-empt it.  ts2d_engine_predict_tiled clears it once per call, not per chunk, so an earlier chunk's inf / NaN survives.
// Is the activation memory still this engine's?  Always for an allocation of its own; a shared workspace carries the token of the last
// run of ANY engine inside it.  (Synchronises: debug / diagnosis paths only.)
bool workspace_is_mine(ts2d_engine* e) {
    if (!e->ws_external) return true;
    if (!e->d_ws || !e->ws_token) return false;
    // Another engine of the set may have ENQUEUED a run on a caller's stream that has not executed yet (its stamp is a stream-ordered
    // memset): this engine's own event says nothing about that, so the token is read behind everything outstanding on the device.
    // (A fresh host thread's current device is 0: select the engine's own first.)
    if (hipSetDevice(e->device) != hipSuccess || hipDeviceSynchronize() != hipSuccess) return false;
    uint32_t tok = 0;
    if (hipMemcpy(&tok, e->d_ws, sizeof(tok), hipMemcpyDeviceToHost) != hipSuccess) return false;
    return tok == e->ws_token;
}

}  // namespace

int ts2d::run_forward(ts2d_engine* e, const float* d_in, int B, int H, int W, float* d_logits, uint32_t* d_mask, hipStream_t st, bool clear_flags, bool full) {
    TRY(workspace_acquire(e, st));
    if (e->ws_external) {           // stamp the shared workspace: whatever another engine of the set left in it is gone after this run
        e->ws_token = ++g_ws_generation;
        if (!e->ws_token) e->ws_token = ++g_ws_generation;
        HIP_TRY(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(e->d_ws), (int)e->ws_token, 1, st));
    }
    if (clear_flags) HIP_TRY(hipMemsetAsync(e->d_flags, 0, 2 * sizeof(int), st));
    const int rc = run_forward_impl(e, d_in, B, H, W, d_logits, d_mask, st, full);
    const int rc2 = workspace_release(e, st);       // also after a failed launch: earlier kernels of the run may be in flight
    return rc != TS2D_OK ? rc : rc2;
}

int ts2d::reserve_checked(ts2d_engine* e, int B, int H, int W, bool full) {
    const int divy = 1 << e->lvl_y[e->arch.n_stages - 1], divx = 1 << e->lvl_x[e->arch.n_stages - 1];
    if (B < 1 || H < divy || W < divx || H % divy || W % divx)
        return fail(TS2D_ERR_INVALID, "shape B=%d H=%d W=%d: H and W must be positive multiples of %d and %d", B, H, W, divy, divx);
    if ((H / divy) * (W / divx) <= 1)   // torch InstanceNorm2d raises "Expected more than 1 spatial element" here too
        return fail(TS2D_ERR_INVALID, "shape %dx%d leaves a single bottleneck pixel: InstanceNorm needs more than 1 spatial element", H, W);
    if ((long long)B * H * W >= (1LL << 31)) return fail(TS2D_ERR_INVALID, "B*H*W = %lld exceeds 2^31 pixels per call", (long long)B * H * W);
    if ((long long)B * H * W >= call_pixel_limit(e))
        return fail(TS2D_ERR_INVALID, "B*H*W = %lld exceeds the 2^29 - 32 pixels per call of a residual-encoder engine (res_join launches 8 threads per pixel)", (long long)B * H * W);
    // one image: every plane the kernels address through a per-image buffer resource stays below 2^31 bytes (program.cpp: image_plane_bytes)
    if (!image_extent_ok(e, H, W)) {
        int t = -1;
        const long long bytes = image_plane_bytes(e, H, W, &t);
        const int C = t >= 0 ? e->tensors[t].C : e->arch.input_channels;
        const int ly = t >= 0 ? e->tensors[t].ly : 0, lx = t >= 0 ? e->tensors[t].lx : 0;
        return fail(TS2D_ERR_INVALID, "image extent %dx%d exceeds the per-image limit: %s holds %lld bytes per image (%d channels of 4 bytes at %dx%d), the limit is "
                    "%lld bytes (2^31 - 1), %lld pixels at that width", H, W, t >= 0 ? e->tensors[t].name.c_str() : "the input", bytes, C, H >> ly, W >> lx,
                    kImagePlaneMax, kImagePlaneMax / ((long long)C * 4));
    }
    return ensure_workspace(e, B, H, W, full);
}

// ------------------------------------------------------------------------------------------------- C-ABI
extern "C" {

int ts2d_abi_version(void) { return 9; }

const char* ts2d_last_error(void) { return last_error(); }

static int create_engine(const char* entry, const ts2d_arch_desc* arch, const ts2d_residual_desc* res, const float* weights, size_t n_floats, int device,
                         ts2d_engine** out) {
    if (!arch || !out) return fail(TS2D_ERR_INVALID, "%s: null argument", entry);
    *out = nullptr;
    if (res) for (int v : res->reserved) if (v) return fail(TS2D_ERR_INVALID, "%s: ts2d_residual_desc.reserved must be zero", entry);
    int ndev = 0;
    HIP_TRY(hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev) return fail(TS2D_ERR_INVALID, "device %d out of range (%d HIP devices visible)", device, ndev);
    ts2d_engine* e = new (std::nothrow) ts2d_engine();
    if (!e) return fail(TS2D_ERR_NOMEM, "host allocation failed");
    e->user_arch = *arch; e->device = device;
    if (res) { e->residual = true; for (int s = 0; s < TS2D_MAX_STAGES; ++s) e->n_blocks[s] = res->n_blocks[s]; }
    if (arch->n_stages >= 2 && arch->n_stages <= TS2D_MAX_STAGES) e->arch = pad_arch(*arch, e->padded); else e->arch = *arch;
    {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0) e->num_cus = prop.multiProcessorCount;
        if (getenv("TS2D_DBG")) e->dbg = atoi(getenv("TS2D_DBG"));
    }
    int rc = build_program(e);
    if (rc != TS2D_OK) { delete e; return rc; }
    hipError_t he = hipSetDevice(device);
    if (he == hipSuccess) he = hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking);
    if (he == hipSuccess) he = hipEventCreateWithFlags(&e->ws_event, hipEventDisableTiming);
    if (he == hipSuccess) he = hipMalloc(reinterpret_cast<void**>(&e->d_flags), 2 * sizeof(int));
    if (he == hipSuccess) he = hipMemset(e->d_flags, 0, 2 * sizeof(int));
    if (he == hipSuccess && e->dbg == 256) he = hipMalloc(reinterpret_cast<void**>(&e->d_prof), 512 * 128 * sizeof(unsigned long long));
    if (he == hipSuccess && e->d_prof) he = hipMemset(e->d_prof, 0, 512 * 128 * sizeof(unsigned long long));
    if (he == hipSuccess) he = hipMalloc(reinterpret_cast<void**>(&e->d_weights), e->weight_floats * sizeof(float));
    if (he != hipSuccess) {
        rc = fail(he == hipErrorOutOfMemory ? TS2D_ERR_NOMEM : TS2D_ERR_HIP, "engine setup failed: %s", hipGetErrorString(he));
        ts2d_engine_destroy(e);
        return rc;
    }
    if (weights) {
        rc = upload_weights(e, weights, n_floats);
        if (rc != TS2D_OK) { ts2d_engine_destroy(e); return rc; }
    }
    *out = e;
    return TS2D_OK;
}

int ts2d_engine_create(const ts2d_arch_desc* arch, const float* weights, size_t n_floats, int device, ts2d_engine** out) {
    return create_engine("ts2d_engine_create", arch, nullptr, weights, n_floats, device, out);
}

int ts2d_engine_create_residual(const ts2d_arch_desc* arch, const ts2d_residual_desc* residual, const float* weights, size_t n_floats, int device,
                                ts2d_engine** out) {
    if (!residual) return fail(TS2D_ERR_INVALID, "ts2d_engine_create_residual: null argument");
    return create_engine("ts2d_engine_create_residual", arch, residual, weights, n_floats, device, out);
}

int ts2d_engine_load_weights(ts2d_engine* e, const float* weights, size_t n_floats) {
    if (!e || !weights) return fail(TS2D_ERR_INVALID, "ts2d_engine_load_weights: null argument");
    HIP_TRY(hipSetDevice(e->device));
    if (e->ws_busy) { HIP_TRY(hipEventSynchronize(e->ws_event)); e->ws_busy = false; }     // a run on any stream may still read the old weights
    HIP_TRY(hipStreamSynchronize(e->stream));
    return upload_weights(e, weights, n_floats);
}

int ts2d_engine_weight_buffer(ts2d_engine* e, void** dev_ptr, size_t* n_bytes) {
    if (!e || !dev_ptr || !n_bytes) return fail(TS2D_ERR_INVALID, "ts2d_engine_weight_buffer: null argument");
    *dev_ptr = e->d_weights; *n_bytes = e->weight_floats * sizeof(float);
    return TS2D_OK;
}

int ts2d_engine_set_precision(ts2d_engine* e, int mode) {
    if (!e) return fail(TS2D_ERR_INVALID, "ts2d_engine_set_precision: null engine");
    if (mode != TS2D_PRECISION_F32_EXACT && mode != TS2D_PRECISION_F32_SPLIT_F16X3 && mode != TS2D_PRECISION_F16)
        return fail(TS2D_ERR_INVALID, "unknown precision mode %d", mode);
    if (mode == TS2D_PRECISION_F16 && e->residual && !e->use_resf16)      // (opt-in, option "resf16": the contract of a residual block is a definition of its own - ts2d_engine.h)
        return fail(TS2D_ERR_INVALID, "TS2D_PRECISION_F16 is not supported on a residual-encoder engine (TS2D_PRECISION_F32_SPLIT_F16X3 and "
                    "TS2D_PRECISION_F32_EXACT are); the mode is unchanged");
    e->precision = mode;
    return TS2D_OK;
}

int ts2d_engine_set_option(ts2d_engine* e, const char* name, int value) {
    if (!e || !name) return fail(TS2D_ERR_INVALID, "ts2d_engine_set_option: null argument");
    struct B { const char* n; bool* p; };
    struct I { const char* n; int* p; int lo, hi; };
    const B bools[] = {{"one", &e->use_one}, {"s2v2", &e->use_s2v2}, {"q", &e->use_q}, {"h2", &e->use_h2},  {"uh2", &e->use_uh2},
                       {"first_split", &e->use_first_split}, {"sbk", &e->use_sbk}, {"s2k32", &e->use_s2k32}, {"s2p", &e->use_s2p}, {"up0", &e->use_up0}, {"upc", &e->use_upc}, {"res", &e->use_res}, {"fuse0", &e->use_fuse0}, {"flex", &e->use_flex}, {"resf16", &e->use_resf16}};
    const I ints[] = {{"u0seg", &e->u0seg, 0, 1 << 20}, {"flex2", &e->use_flex2, 0, 2}};
    bool found = false;
    for (const B& b : bools) if (!strcmp(name, b.n)) { *b.p = value != 0; found = true; }
    for (const I& i : ints) if (!strcmp(name, i.n)) {
        if (value < i.lo || value > i.hi) return fail(TS2D_ERR_INVALID, "option %s = %d out of range [%d, %d]", name, value, i.lo, i.hi);
        *i.p = value; found = true;
    }
    if (!found) return fail(TS2D_ERR_INVALID, "unknown option '%s' (one s2v2 q h2 uh2 up0 u0seg upc res fuse0 flex flex2 first_split sbk s2k32 s2p resf16)", name);
    e->ws_precision = -1;         // which ops compose (and with it the activation plan) depends on the options: re-plan at the next reserve / forward
    ++e->opt_gen;
    return TS2D_OK;
}

int ts2d_engine_set_keep_activations(ts2d_engine* e, int enable) {
    if (!e) return fail(TS2D_ERR_INVALID, "ts2d_engine_set_keep_activations: null engine");
    e->keep_activations = enable != 0;          // takes effect at the next reserve / forward (the workspace is re-planned)
    return TS2D_OK;
}

int ts2d_engine_set_tile_dtype(ts2d_engine* e, int mode) {
    if (!e) return fail(TS2D_ERR_INVALID, "ts2d_engine_set_tile_dtype: null engine");
    if (mode != TS2D_TILE_F32 && mode != TS2D_TILE_F16) return fail(TS2D_ERR_INVALID, "unknown tile dtype %d", mode);
    e->tile_half = mode == TS2D_TILE_F16;
    return TS2D_OK;
}

int ts2d_engine_weights_ready(ts2d_engine* e) {
    if (!e) return fail(TS2D_ERR_INVALID, "ts2d_engine_weights_ready: null engine");
    e->weights_ready = true;
    return TS2D_OK;
}

int ts2d_engine_reserve(ts2d_engine* e, int B, int H, int W) {
    if (!e) return fail(TS2D_ERR_INVALID, "ts2d_engine_reserve: null engine");
    return reserve_checked(e, B, H, W, kBySize);
}

int ts2d_engine_workspace_bytes(ts2d_engine* e, int B, int H, int W, size_t* n_bytes) {
    if (!e || !n_bytes) return fail(TS2D_ERR_INVALID, "ts2d_engine_workspace_bytes: null argument");
    const int divy = 1 << e->lvl_y[e->arch.n_stages - 1], divx = 1 << e->lvl_x[e->arch.n_stages - 1];
    if (B < 1 || H < divy || W < divx || H % divy || W % divx)
        return fail(TS2D_ERR_INVALID, "shape B=%d H=%d W=%d: H and W must be positive multiples of %d and %d", B, H, W, divy, divx);
    *n_bytes = workspace_layout(e, B, H, W, kBySize).bytes;
    return TS2D_OK;
}

int ts2d_engine_set_workspace(ts2d_engine* e, void* dev_ptr, size_t n_bytes) {
    if (!e) return fail(TS2D_ERR_INVALID, "ts2d_engine_set_workspace: null engine");
    if (dev_ptr && (reinterpret_cast<uintptr_t>(dev_ptr) & 255)) return fail(TS2D_ERR_INVALID, "ts2d_engine_set_workspace: the pointer must be 256-byte aligned");
    HIP_TRY(hipSetDevice(e->device));
    if (e->ws_busy) { HIP_TRY(hipEventSynchronize(e->ws_event)); e->ws_busy = false; }      // a run may still use the old memory
    HIP_TRY(hipStreamSynchronize(e->stream));
    if (e->d_ws && !e->ws_external) HIP_TRY(hipFree(e->d_ws));
    e->d_ws = reinterpret_cast<char*>(dev_ptr); e->ws_bytes = dev_ptr ? n_bytes : 0; e->ws_external = dev_ptr != nullptr;
    e->ws_precision = -1; e->wsB = 0;           // re-plan inside the new memory at the next reserve / forward
    for (Tensor& t : e->tensors) { t.data = nullptr; t.bytes = 0; t.resident = false; }
    e->lastB = 0;
    return TS2D_OK;
}

int ts2d_engine_forward(ts2d_engine* e, const float* input, int B, int H, int W, float* logits, uint32_t* mask_packed,
                        int on_device, void* stream) {
    if (!e || !input) return fail(TS2D_ERR_INVALID, "ts2d_engine_forward: null argument");
    if (!e->weights_ready) return fail(TS2D_ERR_STATE, "ts2d_engine_forward: weights not loaded (create with weights, or broadcast + ts2d_engine_weights_ready)");
    if (!logits && !mask_packed) return fail(TS2D_ERR_INVALID, "ts2d_engine_forward: both outputs are null");
    if (mask_packed && (W % 32 || (H * W) % 64)) return fail(TS2D_ERR_INVALID, "packed mask output needs W %% 32 == 0 (W = %d)", W);
    TRY(ts2d_engine_reserve(e, B, H, W));
    HIP_TRY(hipSetDevice(e->device));
    hipStream_t st = stream ? reinterpret_cast<hipStream_t>(stream) : e->stream;
    const int K = e->arch.num_classes;
    if (on_device) return run_forward(e, input, B, H, W, logits, mask_packed, st, true, kBySize);
    // host buffers: staged on the device, synchronous
    TRY(ensure_staging(e, B, H, W));
    HIP_TRY(hipMemcpyAsync(e->d_in_stage, input, (size_t)B * e->arch.input_channels * H * W * sizeof(float), hipMemcpyHostToDevice, st));
    TRY(run_forward(e, e->d_in_stage, B, H, W, logits ? e->d_logit_stage : nullptr, mask_packed ? e->d_mask_stage : nullptr, st, true, kBySize));
    if (logits) HIP_TRY(hipMemcpyAsync(logits, e->d_logit_stage, (size_t)B * K * H * W * sizeof(float), hipMemcpyDeviceToHost, st));
    if (mask_packed) HIP_TRY(hipMemcpyAsync(mask_packed, e->d_mask_stage, (size_t)B * K * H * (W / 32) * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return ts2d_engine_check(e);          // never a silent inf / NaN (asynchronous device-pointer calls: the caller runs the check)
}

int ts2d_engine_check(ts2d_engine* e) {
    if (!e) return fail(TS2D_ERR_INVALID, "ts2d_engine_check: null engine");
    if (!e->lastB) return TS2D_OK;
    HIP_TRY(hipSetDevice(e->device));
    if (e->ws_busy) HIP_TRY(hipEventSynchronize(e->ws_event));
    int flags[2] = {0, 0};
    HIP_TRY(hipMemcpy(flags, e->d_flags, sizeof(flags), hipMemcpyDeviceToHost));
    if (!flags[0]) return TS2D_OK;
    // Diagnosis (slow path, the activations of the run are still resident): the first tensor in program order that holds inf / NaN.
    auto has_nonfinite = [&](const void* p, size_t n, bool half) -> int {
        if (hipMemset(e->d_flags + 1, 0, sizeof(int)) != hipSuccess) return -1;
        const unsigned grid = (unsigned)std::min<size_t>((n + 255) / 256, 4096);
        if (half) hipLaunchKernelGGL(scan_nonfinite<_Float16>, dim3(grid), dim3(256), 0, 0, reinterpret_cast<const _Float16*>(p), n, e->d_flags + 1);
        else hipLaunchKernelGGL(scan_nonfinite<float>, dim3(grid), dim3(256), 0, 0, reinterpret_cast<const float*>(p), n, e->d_flags + 1);
        int f = 0;
        if (hipMemcpy(&f, e->d_flags + 1, sizeof(int), hipMemcpyDeviceToHost) != hipSuccess) return -1;
        return f;
    };
    const int B = e->lastB, H = e->lastH, W = e->lastW;
    // (only the LAST batch of the call is still resident: after a multi-chunk ts2d_engine_predict_tiled an earlier chunk's inf / NaN
    //  is reported, but located only if the last chunk shows it too)
    std::string where = "the head (or an earlier batch of the same call: the diagnosis sees the last batch only)";
    bool input_bad = false, named = false;
    if (e->last_input && has_nonfinite(e->last_input, (size_t)B * e->arch.input_channels * H * W, false) == 1) { where = "the network input"; input_bad = true; }
    float* d_copy = nullptr;
    const bool was_keep = e->keep_activations;
    const bool mine = workspace_is_mine(e);        // a shared workspace may hold ANOTHER engine's activations by now: nothing in it is scanned then
    if (!mine && !input_bad)
        return fail(TS2D_ERR_INVALID, "non-finite logits (inf / NaN) in the last forward; its activations cannot be scanned for the first bad layer: the "
                    "shared workspace (ts2d_engine_set_workspace) has been overwritten by another engine's run since - re-run this engine with a "
                    "workspace of its own (ts2d_engine_set_workspace(e, NULL, 0)) to localise");
    // (shared workspace: the diagnostic re-run with one buffer per tensor needs ~3x the memory the caller sized - skipped; the surviving
    //  tensors of this engine's own last run are scanned below)
    if (!input_bad && !was_keep && e->last_input && !e->ws_external) {
        // activations share buffers by liveness: most of the run has been overwritten.  The input of a synchronous call is still
        // there - run it once more with one buffer per tensor (slow path, taken only after an inf / NaN was flagged).
        const size_t nb = (size_t)B * e->arch.input_channels * H * W * sizeof(float);
        if (hipMalloc(reinterpret_cast<void**>(&d_copy), nb) == hipSuccess && hipMemcpy(d_copy, e->last_input, nb, hipMemcpyDeviceToDevice) == hipSuccess) {
            e->keep_activations = true;
            e->diagnosing = true; ++e->opt_gen;      // (the first block as its own kernel: its output can be scanned and named)
            hipStream_t st = e->last_stream ? e->last_stream : e->stream;
            const bool prof = e->profiling; e->profiling = false;
            const size_t n_launched = e->n_launched;      // (the launch table keeps describing the caller's run: ts2d_engine_op_kernel / _op_ksplit after the error)
            if (ensure_workspace(e, B, H, W, e->last_full) != TS2D_OK || run_forward(e, d_copy, B, H, W, nullptr, nullptr, st, false, e->last_full) != TS2D_OK ||
                hipStreamSynchronize(st) != hipSuccess) { /* keep the generic message */ }
            e->profiling = prof; e->n_launched = n_launched;
            e->diagnosing = false; ++e->opt_gen;
            e->last_input = nullptr;
        }
    }
    if (!input_bad)
        for (const Op& op : e->ops) {
            if (op.dst < 0) continue;
            const size_t oi = (size_t)(&op - e->ops.data());
            if (oi < e->fused_away.size() && e->fused_away[oi]) continue;        // not materialised in the last run
            const Tensor& t = e->tensors[op.dst];
            if (!t.resident || !t.data) continue;                              // overwritten by a later activation of the run
            const size_t n = (size_t)B * (H >> t.ly) * (W >> t.lx) * t.C;
            const int f = has_nonfinite(t.data, n, e->last_f16);
            const int g = (f == 0 && t.normed) ? has_nonfinite(t.scale, (size_t)B * t.C, false) : 0;
            // (a linear tensor - conv2 / projection of a residual block - and a join's sum are scanned as stored, like every other: no activation is applied here)
            if (f == 1 || g == 1) { where = "layer " + op.name + (f == 1 ? "" : " (InstanceNorm statistics)"); named = true; break; }
        }
    if (d_copy) {
        (void)hipFree(d_copy);
        // the diagnostic re-run grew the workspace to one buffer per tensor (~3x): give it back, the next forward re-plans the shared arena
        if (e->ws_busy) { (void)hipEventSynchronize(e->ws_event); e->ws_busy = false; }
        if (e->d_ws && !e->ws_external) { (void)hipFree(e->d_ws); e->d_ws = nullptr; e->ws_bytes = 0; }
        e->ws_precision = -1;     // (re-plan at the next forward)
        for (Tensor& t : e->tensors) { t.data = nullptr; t.bytes = 0; t.resident = false; }
        e->lastB = 0;             // (nothing of that run is readable any more)
    }
    e->keep_activations = was_keep;
    if (named && !was_keep && !d_copy)
        // asynchronous device-pointer call: the input is the caller's, no re-run with private buffers was possible, and most
        // activations of the run have been recycled - the tensor named below is only the first SURVIVING one
        return fail(TS2D_ERR_INVALID, "non-finite logits: first surviving tensor with inf / NaN: %s (earlier activations were recycled; call "
                    "ts2d_engine_set_keep_activations(e, 1) and re-run to localise)%s", where.c_str(), "");
    return fail(TS2D_ERR_INVALID, "non-finite logits: inf / NaN first appears in %s%s", where.c_str(),
                e->precision == TS2D_PRECISION_F32_EXACT ? "" :
                " (the fp16 products of this precision mode need |activation| < 65504 at every conv input: "
                "an overflowing activation - e.g. an un-normalised transposed-conv output - becomes inf; use TS2D_PRECISION_F32_EXACT for such weights)");
}

int ts2d_engine_set_profiling(ts2d_engine* e, int enable) {
    if (!e) return fail(TS2D_ERR_INVALID, "ts2d_engine_set_profiling: null engine");
    e->profiling = enable != 0;
    return TS2D_OK;
}

int ts2d_engine_num_ops(ts2d_engine* e) { return e ? (int)e->n_launched : 0; }

const char* ts2d_engine_op_kernel(ts2d_engine* e, int op) {
    if (!e || op < 0 || (size_t)op >= e->n_launched) return "";
    return e->launches[op].kernel.c_str();
}

int ts2d_engine_op_ksplit(ts2d_engine* e, int op) {
    if (!e || op < 0 || (size_t)op >= e->n_launched) return 0;
    return e->launches[op].ksplit;
}

const char* ts2d_engine_op_name(ts2d_engine* e, int op) {
    if (!e || op < 0 || (size_t)op >= e->n_launched) return "";
    return e->launches[op].name.c_str();
}

int ts2d_engine_op_times(ts2d_engine* e, float* ms, int n_ops) {
    if (!e || !ms) return fail(TS2D_ERR_INVALID, "ts2d_engine_op_times: null argument");
    if (e->d_prof) {        // TS2D_DBG=256: print and reset the in-kernel phase counters (cycles of wave 0, averaged over workgroups)
        std::vector<unsigned long long> raw(512 * 128), hp(8 * 128, 0);
        HIP_TRY(hipDeviceSynchronize());
        HIP_TRY(hipMemcpy(raw.data(), e->d_prof, raw.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
        HIP_TRY(hipMemset(e->d_prof, 0, raw.size() * sizeof(unsigned long long)));
        for (size_t oi = 0; oi < 128; ++oi) for (int k = 0; k < 64; ++k) for (int i = 0; i < 8; ++i) hp[8 * oi + i] += raw[512 * oi + 8 * k + i];
        for (size_t oi = 0; oi < e->ops.size() && oi < 128; ++oi)
            if (hp[8 * oi + 7]) {
                const double n = (double)hp[8 * oi + 7];
                // conv3x3_upc: 0/1 phase-1 staging / MFMAs, 2/3 phase 2, 4 stores, 5 / 6 barriers.  p / s2v2: 0 staging (barrier to barrier), 1 MFMAs
                // (+ wait at the next barrier), 3 last MFMAs, 4 bias + stores, 5 statistics.  q: 0 barrier wait, 1 chunk body, 3-5 as p.
                fprintf(stderr, "[phases] %-8s wgs %6.0f  cycles/wg: [0] %8.0f  [1] %8.0f  [2] %8.0f  [3] %8.0f  [4] %8.0f  [5] %8.0f  [6] %8.0f\n",
                        e->ops[oi].name.c_str(), n, hp[8 * oi] / n, hp[8 * oi + 1] / n, hp[8 * oi + 2] / n, hp[8 * oi + 3] / n, hp[8 * oi + 4] / n, hp[8 * oi + 5] / n, hp[8 * oi + 6] / n);
            }
    }
    if ((size_t)n_ops > e->n_launched) n_ops = (int)e->n_launched;
    for (int i = 0; i < n_ops; ++i) {
        HIP_TRY(hipEventSynchronize(e->launches[i].e1));
        HIP_TRY(hipEventElapsedTime(&ms[i], e->launches[i].e0, e->launches[i].e1));
    }
    return TS2D_OK;
}

int ts2d_engine_debug_tensor(ts2d_engine* e, const char* name, float* out, size_t capacity, int32_t dims[4]) {
    if (!e || !name || !out || !dims) return fail(TS2D_ERR_INVALID, "ts2d_engine_debug_tensor: null argument");
    const int ti = tensor_index(e, name);
    if (ti < 0) return fail(TS2D_ERR_INVALID, "no tensor '%s'", name);
    if (!e->lastB) return fail(TS2D_ERR_STATE, "no forward has run on this engine (or its workspace was replaced since): nothing to read for '%s'", name);
    if (!workspace_is_mine(e))
        return fail(TS2D_ERR_STATE, "tensor '%s': the shared workspace (ts2d_engine_set_workspace) has been overwritten by another engine's forward "
                    "since this engine's last run - run this engine last, or give it a workspace of its own", name);
    const Tensor& t = e->tensors[ti];
    if (t.data && !t.resident)
        return fail(TS2D_ERR_STATE, "tensor '%s' was overwritten by a later activation of the same run (buffers are shared by liveness): "
                    "call ts2d_engine_set_keep_activations(e, 1) before the forward", name);
    for (size_t oi = 0; oi < e->ops.size() && oi < e->fused_away.size(); ++oi)
        if (e->fused_away[oi] && e->ops[oi].dst == ti && oi == 0)
            return fail(TS2D_ERR_INVALID, "tensor '%s' was not materialised by the last run: the first block is recomputed inside the second "
                        "(ts2d_engine_set_option(e, \"fuse0\", 0) runs it as its own kernel)", name);
    for (size_t oi = 0; oi < e->ops.size() && oi < e->fused_away.size(); ++oi)
        if (e->fused_away[oi] && e->ops[oi].dst == ti)
            return fail(TS2D_ERR_INVALID, "tensor '%s' was not materialised by the last run: the transposed conv is composed into the next block "
                        "(ts2d_engine_set_option(e, \"upc\", 0) runs it as its own kernel)", name);
    const int B = e->lastB, h = e->lastH >> t.ly, w = e->lastW >> t.lx, C = t.C, Cu = t.Cu;      // (the caller's channels; C - Cu added ones hold zeros)
    dims[0] = B; dims[1] = Cu; dims[2] = h; dims[3] = w;
    const size_t n = (size_t)B * C * h * w;
    if (capacity < (size_t)B * Cu * h * w) return fail(TS2D_ERR_INVALID, "tensor '%s' needs %zu floats, capacity is %zu", name, (size_t)B * Cu * h * w, capacity);
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipStreamSynchronize(e->last_stream ? e->last_stream : e->stream));
    std::vector<float> raw(n), sc, sh;
    if (e->last_f16) {
        std::vector<uint16_t> rh(n);
        HIP_TRY(hipMemcpy(rh.data(), t.data, n * sizeof(uint16_t), hipMemcpyDeviceToHost));
        for (size_t i = 0; i < n; ++i) raw[i] = f16_to_f32(rh[i]);
    } else {
        HIP_TRY(hipMemcpy(raw.data(), t.data, n * sizeof(float), hipMemcpyDeviceToHost));
    }
    if (t.normed) {
        sc.resize((size_t)B * C); sh.resize((size_t)B * C);
        HIP_TRY(hipMemcpy(sc.data(), t.scale, sc.size() * sizeof(float), hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(sh.data(), t.shift, sh.size() * sizeof(float), hipMemcpyDeviceToHost));
    }
    for (int b = 0; b < B; ++b)
        for (int p = 0; p < h * w; ++p)
            for (int c = 0; c < Cu; ++c) {
                float v = raw[((size_t)b * h * w + p) * C + c];
                if (t.linear) v = std::fmaf(sc[(size_t)b * C + c], v, sh[(size_t)b * C + c]);      // conv2 / projection of a residual block: normalised, not activated - the join's own fused form
                else if (t.normed) { v = v * sc[(size_t)b * C + c] + sh[(size_t)b * C + c]; v = v > 0.f ? v : v * e->arch.leaky_slope; }
                out[((size_t)b * Cu + c) * h * w + p] = v;
            }
    return TS2D_OK;
}

size_t ts2d_engine_device_bytes(ts2d_engine* e) {
    return e ? e->weight_floats * sizeof(float) + (e->ws_external ? 0 : e->ws_bytes) + e->stage_bytes + e->sw_bytes : 0;
}

int ts2d_engine_destroy(ts2d_engine* e) {
    if (!e) return TS2D_OK;
    (void)hipSetDevice(e->device);
    if (e->ws_busy) (void)hipEventSynchronize(e->ws_event);
    if (e->stream) (void)hipStreamSynchronize(e->stream);
    if (e->ws_event) (void)hipEventDestroy(e->ws_event);
    for (Launch& l : e->launches) { if (l.e0) (void)hipEventDestroy(l.e0); if (l.e1) (void)hipEventDestroy(l.e1); }
    if (e->d_ws && !e->ws_external) (void)hipFree(e->d_ws);
    if (e->d_stage) (void)hipFree(e->d_stage);
    if (e->d_flags) (void)hipFree(e->d_flags);
    if (e->d_prof) (void)hipFree(e->d_prof);
    if (e->d_sw) (void)hipFree(e->d_sw);
    if (e->d_weights) (void)hipFree(e->d_weights);
    if (e->stream) (void)hipStreamDestroy(e->stream);
    delete e;
    return TS2D_OK;
}

}  // extern "C"

