// libts2d_engine.so - host side of the MI355X-native 2-D U-Net engine + the C-ABI of include/ts2d_engine.h.
// Replaces the network-forward part of nnUNetPredictor (reference seam: ts2d/core/inference/prediction_worker.py:209,
// network built at ts2d/core/inference/nnu.py:164-165).  gfx950 only; no CPU fallback exists in this library.
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
#include "kernels_upc.h"
#include "kernels_up0.h"
#include "kernels_upq.h"
#include "kernels_upc_h.h"
#include "kernels_upc_h2.h"
#include "kernels_sw.h"
#include "kernels_fold.h"
#include "kernels_resample.h"
#include "kernels_resample_in.h"
#include "kernels_project.h"
#include "kernels_prep.h"

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

#define HIP_TRY(expr)                                                                                     \
    do {                                                                                                  \
        hipError_t _e = (expr);                                                                           \
        if (_e != hipSuccess)                                                                             \
            return fail(_e == hipErrorOutOfMemory ? TS2D_ERR_NOMEM : TS2D_ERR_HIP, "%s failed: %s (%s:%d)", \
                        #expr, hipGetErrorString(_e), __FILE__, __LINE__);                                \
    } while (0)
#define TRY(expr) do { int _rc = (expr); if (_rc != TS2D_OK) return _rc; } while (0)

int upload_weights(ts2d_engine* e, const float* blob, size_t n_floats) {
    // (pack_weights also records the per-layer split scale in the op table)
    if (n_floats != e->user_blob_floats)
        return fail(TS2D_ERR_INVALID, "weight blob has %zu floats, architecture needs %zu", n_floats, e->user_blob_floats);
    std::vector<float> staging, wide;
    try {
        staging.resize(e->weight_floats);
        if (e->padded) { expand_blob(e->user_arch, e->arch, blob, wide); blob = wide.data(); }
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
    const size_t wchunk = (size_t)9 * c.npp * 2 * c.bn * 16;
    const bool resw = (size_t)c.npp * 2 * kS2Plane + (size_t)c.nch * wchunk <= (size_t)160 * 1024;
    const dim3 grid(std::min(grid_x, 8 * ca.n_ctiles * std::max(1, e->num_cus / (8 * ca.n_ctiles)))), block(kS2Threads);
    const size_t smem = (size_t)c.npp * 2 * kS2Plane + (resw ? (size_t)c.nch : 1) * wchunk;
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
        if (c.k == K_NONE) return fail(TS2D_ERR_INVALID, "op %s has no fp16 kernel (channel counts must be multiples of 16)", op.name.c_str());
        if (c.k == K_FUSED_AWAY) { e->fused_away[oi] = 1; continue; }      // composed into the next block (kernels_upc.h): the upsampled tensor is never materialised
        TRY(prof_begin(e, op.name, "", st));
        prof_kernel(e, c.name);
        if (c.ksplit > 1) prof_ksplit(e, c.ksplit);
        TRY(launch_op(e, oi, c, r));
        TRY(prof_end(e, st));
        if (op.type == OP_CONV) TRY(launch_stats(e, oi, c, r));
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

int run_forward(ts2d_engine* e, const float* d_in, int B, int H, int W, float* d_logits, uint32_t* d_mask, hipStream_t st, bool clear_flags, bool full) {
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

}  // namespace

// ------------------------------------------------------------------------------------------------- C-ABI
extern "C" {

int ts2d_abi_version(void) { return 9; }

const char* ts2d_last_error(void) { return last_error(); }

int ts2d_engine_create(const ts2d_arch_desc* arch, const float* weights, size_t n_floats, int device, ts2d_engine** out) {
    if (!arch || !out) return fail(TS2D_ERR_INVALID, "ts2d_engine_create: null argument");
    *out = nullptr;
    int ndev = 0;
    HIP_TRY(hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev) return fail(TS2D_ERR_INVALID, "device %d out of range (%d HIP devices visible)", device, ndev);
    ts2d_engine* e = new (std::nothrow) ts2d_engine();
    if (!e) return fail(TS2D_ERR_NOMEM, "host allocation failed");
    e->user_arch = *arch; e->device = device;
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
    e->precision = mode;
    return TS2D_OK;
}

int ts2d_engine_set_option(ts2d_engine* e, const char* name, int value) {
    if (!e || !name) return fail(TS2D_ERR_INVALID, "ts2d_engine_set_option: null argument");
    struct B { const char* n; bool* p; };
    struct I { const char* n; int* p; int lo, hi; };
    const B bools[] = {{"one", &e->use_one}, {"s2v2", &e->use_s2v2}, {"q", &e->use_q}, {"h2", &e->use_h2},  {"uh2", &e->use_uh2},
                       {"first_split", &e->use_first_split}, {"sbk", &e->use_sbk}, {"s2k32", &e->use_s2k32}, {"up0", &e->use_up0}, {"upc", &e->use_upc}, {"res", &e->use_res}, {"fuse0", &e->use_fuse0}, {"flex", &e->use_flex}};
    const I ints[] = {{"u0seg", &e->u0seg, 0, 1 << 20}, {"flex2", &e->use_flex2, 0, 2}};
    bool found = false;
    for (const B& b : bools) if (!strcmp(name, b.n)) { *b.p = value != 0; found = true; }
    for (const I& i : ints) if (!strcmp(name, i.n)) {
        if (value < i.lo || value > i.hi) return fail(TS2D_ERR_INVALID, "option %s = %d out of range [%d, %d]", name, value, i.lo, i.hi);
        *i.p = value; found = true;
    }
    if (!found) return fail(TS2D_ERR_INVALID, "unknown option '%s' (one s2v2 q h2 uh2 up0 u0seg upc res fuse0 flex flex2 first_split sbk s2k32)", name);
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

static int reserve_checked(ts2d_engine* e, int B, int H, int W, bool full) {
    const int divy = 1 << e->lvl_y[e->arch.n_stages - 1], divx = 1 << e->lvl_x[e->arch.n_stages - 1];
    if (B < 1 || H < divy || W < divx || H % divy || W % divx)
        return fail(TS2D_ERR_INVALID, "shape B=%d H=%d W=%d: H and W must be positive multiples of %d and %d", B, H, W, divy, divx);
    if ((H / divy) * (W / divx) <= 1)   // torch InstanceNorm2d raises "Expected more than 1 spatial element" here too
        return fail(TS2D_ERR_INVALID, "shape %dx%d leaves a single bottleneck pixel: InstanceNorm needs more than 1 spatial element", H, W);
    if ((long long)B * H * W >= (1LL << 31)) return fail(TS2D_ERR_INVALID, "B*H*W = %lld exceeds 2^31 pixels per call", (long long)B * H * W);
    return ensure_workspace(e, B, H, W, full);
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

// The sliding window of both C entries (include/ts2d_engine.h): N images as ONE engine batch; ts2d_engine_predict_tiled is N = 1.
// Host side: validate everything, pack the rows (tile x mirror variant) of the images into chunks of at most kSwChunkRows, lay the
// scratch out, enqueue every host-to-device copy, then per chunk one sw_gather, one forward and (where an image ends in the chunk)
// one sw_aggregate, then every device-to-host copy, ONE stream synchronise and the result check.
// `full` is the whole difference between the entries' results: the batch entry asks for the full-batch dispatch (a row's bits must not
// depend on its batch-mates), the single-image entry for the size-dependent one.  `name_images`: a message names the image it is about.
// `exports` (ts2d_engine_predict_tiled_export; else null): one descriptor per image - behind the last aggregate ONE sw_resample_threshold
// launch resamples every image's half logits to its export extent where they lie in the scratch.
// `engines[0 .. F)` (ts2d_ensemble_predict_tiled_export; the other entries are F = 1): the folds of an ensemble, one after the other on
// the FIRST engine's stream and in its scratch - the chunk loop once per fold, sw_aggregate into the fold's own half slot and inf
// flags, then ONE sw_fold_mean (kernels_fold.h) into slot 0, on which the tail below runs as it does on a single fold's logits.  Only
// the half slots and the flags exist F times.  `name_folds`: a fold's failed reserve or result check is reported as "fold <f>: ...".
constexpr int kSwChunkRows = 64;
constexpr int kMaxFolds = 32;

static int name_fold(int rc, bool name_folds, int f) {
    if (rc == TS2D_OK || !name_folds) return rc;
    const std::string msg = last_error();
    return fail(rc, "fold %d: %s", f, msg.c_str());
}

// Taps of one axis of the order-1 resample (n_in -> n_out samples; preprocess.linear_axis_taps is the same statement in numpy, pinned
// to scipy): cc = (o + 0.5) * (n_in / n_out) - 0.5, i0 = floor(cc), w1 = cc - i0, all in float64; the coordinate is not clamped, the
// two INDICES are (scipy extends the array by its edge samples).  `origin` shifts the indices to the padded plane.
// No contraction: a fused (o + 0.5) * zoom - 0.5 would round differently from numpy on a host build that has FMA (-march=native).
static void rs_axis_taps(int n_in, int n_out, int origin, RsTap* t) {
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

static int predict_tiled_impl(ts2d_engine* const* engines, int F, ts2d_tiled_image* images, const ts2d_tiled_export* exports, int n_images,
                              int ph, int pw, int mirror_mask, const uint16_t* gaussian_f16, bool full, bool name_images, bool name_folds,
                              const char* entry) {
    ts2d_engine* e = engines[0];
    if (ph < 1 || pw < 1) return fail(TS2D_ERR_INVALID, "%s: bad patch %dx%d", entry, ph, pw);
    const int C = e->arch.input_channels, K = e->arch.num_classes;
    int vflip[4] = {0, 0, 0, 0}, V = 1;
    if ((mirror_mask & 3) == 3) { vflip[1] = 1; vflip[2] = 2; vflip[3] = 3; V = 4; }
    else if (mirror_mask & 1) { vflip[1] = 1; V = 2; }
    else if (mirror_mask & 2) { vflip[1] = 2; V = 2; }
    const int vflips = vflip[0] | (vflip[1] << 8) | (vflip[2] << 16) | (vflip[3] << 24);
    long long n_tiles_all = 0, n_taps_all = 0;
    bool any16 = F > 1, anyseg = false, any_rs8 = false, any_rs32 = false;      // (the mean is taken over the half buffers)
    for (int i = 0; i < n_images; ++i) {
        const ts2d_tiled_image& im = images[i];
        char pre[24] = "";
        if (name_images) snprintf(pre, sizeof(pre), "image %d: ", i);
        if (!im.image || !im.tile_y || !im.tile_x) return fail(TS2D_ERR_INVALID, "%snull image or tile pointer", pre);
        if (!exports && !im.logits_f16 && !im.seg_u8) return fail(TS2D_ERR_INVALID, "%sboth outputs are null", pre);
        if (im.n_tiles < 1 || im.n_tiles > (1 << 20) || im.Hp < 1 || im.Wp < 1 || ph > im.Hp || pw > im.Wp)
            return fail(TS2D_ERR_INVALID, "%sbad tiling: %d tiles of %dx%d on %dx%d", pre, im.n_tiles, ph, pw, im.Hp, im.Wp);
        if ((long long)K * im.Hp * im.Wp >= (1LL << 31) || (long long)C * im.Hp * im.Wp >= (1LL << 31))
            return fail(TS2D_ERR_INVALID, "%s%dx%d exceeds 2^31 elements per image", pre, im.Hp, im.Wp);
        for (int t = 0; t < im.n_tiles; ++t)
            if (im.tile_y[t] < 0 || im.tile_x[t] < 0 || im.tile_y[t] + ph > im.Hp || im.tile_x[t] + pw > im.Wp)
                return fail(TS2D_ERR_INVALID, "%stile %d at (%d,%d) leaves the %dx%d image", pre, t, im.tile_y[t], im.tile_x[t], im.Hp, im.Wp);
        n_tiles_all += im.n_tiles;
        any16 |= im.logits_f16 != nullptr; anyseg |= im.seg_u8 != nullptr;
        if (!exports) continue;
        const ts2d_tiled_export& ex = exports[i];
        if (!ex.seg_u8 && !ex.logits_f32) return fail(TS2D_ERR_INVALID, "%sexport: both outputs are null", pre);
        if (ex.src_h < 1 || ex.src_w < 1 || ex.src_y < 0 || ex.src_x < 0 || ex.src_h > im.Hp - ex.src_y || ex.src_w > im.Wp - ex.src_x)
            return fail(TS2D_ERR_INVALID, "%sexport: source rectangle %dx%d at (%d,%d) is empty or leaves the %dx%d image", pre, ex.src_h, ex.src_w,
                        ex.src_y, ex.src_x, im.Hp, im.Wp);
        if (ex.out_h < 1 || ex.out_w < 1) return fail(TS2D_ERR_INVALID, "%sexport: bad output extent %dx%d", pre, ex.out_h, ex.out_w);
        if ((long long)K * ex.out_h * ex.out_w >= (1LL << 31))
            return fail(TS2D_ERR_INVALID, "%sexport: %dx%d exceeds 2^31 output elements", pre, ex.out_h, ex.out_w);
        n_taps_all += (long long)ex.out_h + ex.out_w;         // (each < 2^31 by the check above; bounded before any table is allocated)
        if (n_taps_all >= (1LL << 26)) return fail(TS2D_ERR_INVALID, "%sexport: more than 2^26 output rows + columns in one call", pre);
        any16 = true; any_rs8 |= ex.seg_u8 != nullptr; any_rs32 |= ex.logits_f32 != nullptr;
    }
    if (n_tiles_all * V >= (1LL << 28)) return fail(TS2D_ERR_INVALID, "%s: %lld network rows in one call", entry, n_tiles_all * V);
    // ---- row packing: whole images, greedily, into chunks of at most kSwChunkRows rows; a larger image takes chunks of its own
    struct Chunk { int seg0, n_segs, rows, log_row; bool aggregate; unsigned gblocks, ablocks; };
    std::vector<SwSeg> segs;
    std::vector<Chunk> chunks;
    std::vector<size_t> o_img(n_images);
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t o = off; off = align_up(off + bytes, 256); return o; };
    const int pwq = (pw + 3) / 4;
    auto blocks_of = [](long long lanes) { return (lanes + 255) / 256; };
    long long out_elems = 0, img_floats = 0;
    int tile0 = 0, cap_rows = 0;
    long long log_rows = 0;
    Chunk cur{0, 0, 0, 0, true, 0, 0};
    auto flush = [&]() { if (cur.n_segs) chunks.push_back(cur); cur = Chunk{(int)segs.size(), 0, 0, 0, true, 0, 0}; };
    for (int i = 0; i < n_images; ++i) {
        const ts2d_tiled_image& im = images[i];
        const int rows = im.n_tiles * V;
        SwSeg sg{};
        sg.img_off = img_floats; sg.out_off = out_elems; sg.Hp = im.Hp; sg.Wp = im.Wp; sg.tile0 = tile0; sg.n_tiles = im.n_tiles; sg.image = i;
        const long long ablocks = blocks_of((long long)K * im.Hp * ((im.Wp + 3) / 4));
        if (rows > kSwChunkRows) {
            flush();
            for (int r0 = 0; r0 < rows; r0 += kSwChunkRows) {
                const int nb = std::min(kSwChunkRows, rows - r0);
                sg.row0 = r0; sg.n_rows = nb; sg.batch_row = 0; sg.log_row = 0; sg.gblock0 = 0; sg.ablock0 = 0;
                segs.push_back(sg);
                cur.n_segs = 1; cur.rows = nb; cur.log_row = r0; cur.aggregate = r0 + nb == rows;
                cur.gblocks = (unsigned)blocks_of((long long)nb * C * ph * pwq); cur.ablocks = (unsigned)ablocks;
                flush();
            }
        } else {
            if (cur.rows + rows > kSwChunkRows) flush();
            sg.row0 = 0; sg.n_rows = rows; sg.batch_row = cur.rows; sg.log_row = cur.rows; sg.gblock0 = cur.gblocks; sg.ablock0 = cur.ablocks;
            segs.push_back(sg);
            cur.n_segs++; cur.rows += rows;
            cur.gblocks += (unsigned)blocks_of((long long)rows * C * ph * pwq); cur.ablocks += (unsigned)ablocks;
        }
        cap_rows = std::max(cap_rows, std::min(rows, kSwChunkRows)); log_rows = std::max<long long>(log_rows, rows);
        tile0 += im.n_tiles;
        img_floats += (long long)align_up((size_t)C * im.Hp * im.Wp, 64);
        out_elems += (long long)align_up((size_t)K * im.Hp * im.Wp, 256);
    }
    flush();
    for (const Chunk& c : chunks) {
        cap_rows = std::max(cap_rows, c.rows);
        if ((long long)c.gblocks >= (1LL << 31) || (long long)c.ablocks >= (1LL << 31)) return fail(TS2D_ERR_INVALID, "%s: a chunk exceeds 2^31 blocks", entry);
    }
    log_rows = std::max<long long>(log_rows, cap_rows);
    if (F > 1 && blocks_of(out_elems >> 3) >= (1LL << 31)) return fail(TS2D_ERR_INVALID, "%s: the fold mean exceeds 2^31 blocks", entry);
    // ---- the export: one segment per image (its half logits are segs' out_off), the taps of its rows then of its columns
    std::vector<RsSeg> rsegs;
    std::vector<RsTap> rtaps;
    long long rs_elems = 0, rs_blocks = 0;
    if (exports) {
        long long oo = 0;
        for (int i = 0; i < n_images; ++i) {
            const ts2d_tiled_image& im = images[i]; const ts2d_tiled_export& ex = exports[i];
            RsSeg rs{};
            rs.src_off = oo; rs.dst_off = rs_elems; rs.Hp = im.Hp; rs.Wp = im.Wp; rs.out_h = ex.out_h; rs.out_w = ex.out_w;
            rs.tap0 = (int)rtaps.size(); rs.block0 = (unsigned)rs_blocks;
            rsegs.push_back(rs);
            rtaps.resize(rtaps.size() + ex.out_h + ex.out_w);
            rs_axis_taps(ex.src_h, ex.out_h, ex.src_y, rtaps.data() + rs.tap0);
            rs_axis_taps(ex.src_w, ex.out_w, ex.src_x, rtaps.data() + rs.tap0 + ex.out_h);
            rs_blocks += blocks_of((long long)K * ex.out_h * ((ex.out_w + 3) / 4));
            rs_elems += (long long)align_up((size_t)K * ex.out_h * ex.out_w, 256);
            oo += (long long)align_up((size_t)K * im.Hp * im.Wp, 256);
        }
        if (rs_blocks >= (1LL << 31)) return fail(TS2D_ERR_INVALID, "%s: the export exceeds 2^31 blocks", entry);
    }
    for (int f = 0; f < F; ++f) TRY(name_fold(reserve_checked(engines[f], cap_rows, ph, pw, full), name_folds, f));
    HIP_TRY(hipSetDevice(e->device));
    hipStream_t st = e->stream;
    // ---- the descriptor table and every tile origin: one host blob, one copy
    const size_t tab_segs = segs.size() * sizeof(SwSeg), tab_rsegs = align_up(tab_segs + 2 * (size_t)n_tiles_all * 4, 8);
    const size_t tab_rtaps = tab_rsegs + rsegs.size() * sizeof(RsSeg), tab_bytes = tab_rtaps + rtaps.size() * sizeof(RsTap);
    std::vector<char> tab(tab_bytes);
    memcpy(tab.data(), segs.data(), tab_segs);
    if (exports) { memcpy(tab.data() + tab_rsegs, rsegs.data(), rsegs.size() * sizeof(RsSeg)); memcpy(tab.data() + tab_rtaps, rtaps.data(), rtaps.size() * sizeof(RsTap)); }
    {
        int32_t* ty = reinterpret_cast<int32_t*>(tab.data() + tab_segs); int32_t* tx = ty + n_tiles_all;
        for (int i = 0; i < n_images; ++i) {
            memcpy(ty, images[i].tile_y, (size_t)images[i].n_tiles * 4); memcpy(tx, images[i].tile_x, (size_t)images[i].n_tiles * 4);
            ty += images[i].n_tiles; tx += images[i].n_tiles;
        }
    }
    // ---- scratch: [table | gaussian | images | one chunk's batch | tile logits | half outputs x F | uint8 outputs | flags x F | resampled uint8 | resampled float]
    const size_t o_tab = take(tab_bytes), o_g = take((size_t)ph * pw * 2), o_imgs = take((size_t)img_floats * 4);
    const size_t o_batch = take((size_t)cap_rows * C * ph * pw * 4), o_log = take((size_t)log_rows * K * ph * pw * 4);
    const size_t o_o16 = take(any16 ? (size_t)F * out_elems * 2 : 0), o_seg = take(anyseg ? (size_t)out_elems : 0), o_flag = take((size_t)F * n_images * 4);
    const size_t o_rs8 = take(any_rs8 ? (size_t)rs_elems : 0), o_rs32 = take(any_rs32 ? (size_t)rs_elems * 4 : 0);
    if (off > e->sw_bytes) {                                  // grown before the first launch only
        HIP_TRY(hipStreamSynchronize(st));
        if (e->d_sw) { HIP_TRY(hipFree(e->d_sw)); e->d_sw = nullptr; e->sw_bytes = 0; }
        HIP_TRY(hipMalloc(reinterpret_cast<void**>(&e->d_sw), off));
        e->sw_bytes = off;
    }
    char* b = e->d_sw;
    const SwSeg* d_segs = reinterpret_cast<const SwSeg*>(b + o_tab);
    const int* d_ty = reinterpret_cast<const int*>(b + o_tab + tab_segs); const int* d_tx = d_ty + n_tiles_all;
    __half* d_g = reinterpret_cast<__half*>(b + o_g); float* d_imgs = reinterpret_cast<float*>(b + o_imgs);
    float* d_batch = reinterpret_cast<float*>(b + o_batch); float* d_log = reinterpret_cast<float*>(b + o_log);
    __half* d_o16 = any16 ? reinterpret_cast<__half*>(b + o_o16) : nullptr; uint8_t* d_seg = anyseg ? reinterpret_cast<uint8_t*>(b + o_seg) : nullptr;
    int* d_flag = reinterpret_cast<int*>(b + o_flag);
    for (int i = 0; i < n_images; ++i) images[i].inf_flag = 0;
    HIP_TRY(hipMemcpyAsync(b + o_tab, tab.data(), tab_bytes, hipMemcpyHostToDevice, st));
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
        for (size_t ci = 0; ci < chunks.size(); ++ci) {
            const Chunk& c = chunks[ci];
            hipLaunchKernelGGL(sw_gather, dim3(c.gblocks), dim3(256), 0, st, d_imgs, d_segs + c.seg0, c.n_segs, C, ph, pw, V, vflips, d_ty, d_tx, d_batch);
            HIP_TRY(hipGetLastError());
            TRY(run_forward(engines[f], d_batch, c.rows, ph, pw, d_log + (size_t)c.log_row * K * ph * pw, nullptr, st, ci == 0, full));
            if (!c.aggregate) continue;
            // (an ensemble's uint8 output is the predicate on the MEAN: sw_fold_mean writes it)
            hipLaunchKernelGGL(sw_aggregate, dim3(c.ablocks), dim3(256), 0, st, d_log, d_segs + c.seg0, c.n_segs, K, ph, pw, V, vflips, d_ty, d_tx,
                               gaussian_f16 ? d_g : nullptr, d_o16 ? d_o16 + (size_t)f * out_elems : nullptr, F > 1 ? nullptr : d_seg,
                               kSigmoidHalfThreshold, d_flag + (size_t)f * n_images, e->tile_half);
            HIP_TRY(hipGetLastError());
        }
    if (F > 1) {          // every slot up to the end of the last image (the alignment gaps between the images ride along unread)
        const long long n_mean = segs.back().out_off + (long long)K * segs.back().Hp * segs.back().Wp;
        hipLaunchKernelGGL(sw_fold_mean, dim3((unsigned)blocks_of((n_mean >> 3) + (n_mean & 7))), dim3(256), 0, st, d_o16, out_elems, F, n_mean,
                           d_seg, kSigmoidHalfThreshold);
        HIP_TRY(hipGetLastError());
    }
    uint8_t* d_rs8 = any_rs8 ? reinterpret_cast<uint8_t*>(b + o_rs8) : nullptr; float* d_rs32 = any_rs32 ? reinterpret_cast<float*>(b + o_rs32) : nullptr;
    if (exports) {
        hipLaunchKernelGGL(sw_resample_threshold, dim3((unsigned)rs_blocks), dim3(256), 0, st, d_o16, reinterpret_cast<const RsSeg*>(b + o_tab + tab_rsegs),
                           n_images, K, reinterpret_cast<const RsTap*>(b + o_tab + tab_rtaps), d_rs8, d_rs32, kSigmoidHalfThreshold);
        HIP_TRY(hipGetLastError());
        for (int i = 0; i < n_images; ++i) {
            const size_t ne = (size_t)K * exports[i].out_h * exports[i].out_w;
            if (exports[i].seg_u8) HIP_TRY(hipMemcpyAsync(exports[i].seg_u8, d_rs8 + rsegs[i].dst_off, ne, hipMemcpyDeviceToHost, st));
            if (exports[i].logits_f32) HIP_TRY(hipMemcpyAsync(exports[i].logits_f32, d_rs32 + rsegs[i].dst_off, ne * 4, hipMemcpyDeviceToHost, st));
        }
    }
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

int ts2d_engine_predict_tiled(ts2d_engine* e, const float* image, int Hp, int Wp, int ph, int pw, int n_tiles,
                              const int32_t* tile_y, const int32_t* tile_x, int mirror_mask, const uint16_t* gaussian_f16,
                              uint16_t* logits_f16, uint8_t* seg_u8) {
    if (!e || !image || !tile_y || !tile_x) return fail(TS2D_ERR_INVALID, "ts2d_engine_predict_tiled: null argument");
    if (!e->weights_ready) return fail(TS2D_ERR_STATE, "ts2d_engine_predict_tiled: weights not loaded");
    if (!logits_f16 && !seg_u8) return fail(TS2D_ERR_INVALID, "ts2d_engine_predict_tiled: both outputs are null");
    ts2d_tiled_image one{image, Hp, Wp, n_tiles, tile_y, tile_x, logits_f16, seg_u8, 0};
    return predict_tiled_impl(&e, 1, &one, nullptr, 1, ph, pw, mirror_mask, gaussian_f16, kBySize, false, false, "ts2d_engine_predict_tiled");
}

int ts2d_engine_predict_tiled_batch(ts2d_engine* e, ts2d_tiled_image* images, int n_images, int ph, int pw, int mirror_mask,
                                    const uint16_t* gaussian_f16) {
    if (!e) return fail(TS2D_ERR_INVALID, "ts2d_engine_predict_tiled_batch: null engine");
    if (n_images < 0 || (n_images > 0 && !images)) return fail(TS2D_ERR_INVALID, "ts2d_engine_predict_tiled_batch: %d images at a null pointer", n_images);
    if (n_images == 0) return TS2D_OK;
    if (!e->weights_ready) return fail(TS2D_ERR_STATE, "ts2d_engine_predict_tiled_batch: weights not loaded");
    return predict_tiled_impl(&e, 1, images, nullptr, n_images, ph, pw, mirror_mask, gaussian_f16, kFullBatch, true, false, "ts2d_engine_predict_tiled_batch");
}

int ts2d_engine_predict_tiled_export(ts2d_engine* e, ts2d_tiled_image* images, const ts2d_tiled_export* exports, int n_images, int ph, int pw,
                                     int mirror_mask, const uint16_t* gaussian_f16, int full_batch) {
    if (!e) return fail(TS2D_ERR_INVALID, "ts2d_engine_predict_tiled_export: null engine");
    if (n_images < 0 || (n_images > 0 && !(images && exports)))
        return fail(TS2D_ERR_INVALID, "ts2d_engine_predict_tiled_export: %d images at a null pointer", n_images);
    if (n_images == 0) return TS2D_OK;
    if (!e->weights_ready) return fail(TS2D_ERR_STATE, "ts2d_engine_predict_tiled_export: weights not loaded");
    return predict_tiled_impl(&e, 1, images, exports, n_images, ph, pw, mirror_mask, gaussian_f16, full_batch ? kFullBatch : kBySize, true, false,
                              "ts2d_engine_predict_tiled_export");
}

int ts2d_ensemble_predict_tiled_export(ts2d_engine* const* engines, int n_engines, ts2d_tiled_image* images, const ts2d_tiled_export* exports,
                                       int n_images, int ph, int pw, int mirror_mask, const uint16_t* gaussian_f16, int full_batch) {
    static const char* entry = "ts2d_ensemble_predict_tiled_export";
    if (!engines) return fail(TS2D_ERR_INVALID, "%s: %d engines at a null pointer", entry, n_engines);
    if (n_engines < 1 || n_engines > kMaxFolds) return fail(TS2D_ERR_INVALID, "%s: n_engines = %d is outside 1..%d", entry, n_engines, kMaxFolds);
    for (int f = 0; f < n_engines; ++f)
        if (!engines[f]) return fail(TS2D_ERR_INVALID, "%s: engine %d is null", entry, f);
    if (n_images < 0 || (n_images > 0 && !images)) return fail(TS2D_ERR_INVALID, "%s: %d images at a null pointer", entry, n_images);
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
    return predict_tiled_impl(engines, n_engines, images, exports, n_images, ph, pw, mirror_mask, gaussian_f16, full_batch ? kFullBatch : kBySize,
                              true, true, entry);
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

int ts2d_engine_tiled_inf_flag(const ts2d_engine* e) { return e ? (e->tiled_inf != 0) : 0; }

static int project_coronal_impl(int device, const void* volume, size_t n_elems, int dtype, int nz, int ny, int nx, long long sz,
                                long long sy, long long sx, long long base, float* out_max, float* out_mean, float* out_norm, double* out_stats, int* out_box) {
    if (!volume || !out_max || !out_mean) return fail(TS2D_ERR_INVALID, "ts2d_project_coronal: null argument");
    static const int esize[5] = {2, 1, 4, 2, 4};
    if (dtype < 0 || dtype > 4 || nz < 1 || ny < 1 || nx < 1) return fail(TS2D_ERR_INVALID, "ts2d_project_coronal: bad dtype / extents");
    {   // every element the view can touch must lie inside the buffer
        long long lo = base, hi = base;
        const long long ext[3] = {(long long)(nz - 1) * sz, (long long)(ny - 1) * sy, (long long)(nx - 1) * sx};
        for (int k = 0; k < 3; ++k) { if (ext[k] < 0) lo += ext[k]; else hi += ext[k]; }
        if (lo < 0 || hi >= (long long)n_elems) return fail(TS2D_ERR_INVALID, "ts2d_project_coronal: the strided view leaves the buffer");
    }
    HIP_TRY(hipSetDevice(device));
    const size_t vbytes = n_elems * esize[dtype], obytes = (size_t)nz * nx * sizeof(float);
    char* d = nullptr;
    // [volume | max | mean (contiguous: the two channels of the z-score) | normalised x 2 | partial sums | stats | box]
    const size_t o_proj = align_up(vbytes, 256), o_norm = align_up(o_proj + 2 * obytes, 256), o_part = align_up(o_norm + 2 * obytes, 256);
    const size_t o_stats = o_part + 2 * kZBlocks * sizeof(double), o_box = o_stats + 4 * sizeof(double);
    HIP_TRY(hipMalloc(reinterpret_cast<void**>(&d), o_box + 4 * sizeof(int)));
    float* d_max = reinterpret_cast<float*>(d + o_proj);
    float* d_mean = d_max + (size_t)nz * nx;
    hipError_t he = hipMemcpy(d, volume, vbytes, hipMemcpyHostToDevice);
    if (he == hipSuccess) {
        const unsigned grid = (unsigned)(((long long)nz * nx + 255) / 256);
        switch (dtype) {
            case 0: hipLaunchKernelGGL(project_coronal<int16_t>, dim3(grid), dim3(256), 0, 0, reinterpret_cast<const int16_t*>(d), nz, ny, nx, sz, sy, sx, base, d_max, d_mean); break;
            case 1: hipLaunchKernelGGL(project_coronal<uint8_t>, dim3(grid), dim3(256), 0, 0, reinterpret_cast<const uint8_t*>(d), nz, ny, nx, sz, sy, sx, base, d_max, d_mean); break;
            case 2: hipLaunchKernelGGL(project_coronal<float>, dim3(grid), dim3(256), 0, 0, reinterpret_cast<const float*>(d), nz, ny, nx, sz, sy, sx, base, d_max, d_mean); break;
            case 3: hipLaunchKernelGGL(project_coronal<uint16_t>, dim3(grid), dim3(256), 0, 0, reinterpret_cast<const uint16_t*>(d), nz, ny, nx, sz, sy, sx, base, d_max, d_mean); break;
            default: hipLaunchKernelGGL(project_coronal<int32_t>, dim3(grid), dim3(256), 0, 0, reinterpret_cast<const int32_t*>(d), nz, ny, nx, sz, sy, sx, base, d_max, d_mean); break;
        }
        he = hipGetLastError();
    }
    if (he == hipSuccess && out_norm) {          // per-channel z-score of (max, mean): float64 two-pass statistics, deterministic
        const long long n = (long long)nz * nx;
        float* d_norm = reinterpret_cast<float*>(d + o_norm);
        double* d_part = reinterpret_cast<double*>(d + o_part); double* d_stats = reinterpret_cast<double*>(d + o_stats);
        int* d_box = reinterpret_cast<int*>(d + o_box);
        const int box0[4] = {nz, -1, nx, -1};
        he = hipMemcpy(d_box, box0, sizeof(box0), hipMemcpyHostToDevice);
        if (he == hipSuccess) {
            hipLaunchKernelGGL(zs_partial<0>, dim3(kZBlocks, 2), dim3(256), 0, 0, d_max, n, d_stats, d_part);
            hipLaunchKernelGGL(zs_combine<0>, dim3(1), dim3(2), 0, 0, d_part, n, d_stats);
            hipLaunchKernelGGL(zs_partial<1>, dim3(kZBlocks, 2), dim3(256), 0, 0, d_max, n, d_stats, d_part);
            hipLaunchKernelGGL(zs_combine<1>, dim3(1), dim3(2), 0, 0, d_part, n, d_stats);
            hipLaunchKernelGGL(zs_apply, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, d_max, n, nx, 2, d_stats, d_norm, d_box);
            he = hipGetLastError();
        }
        if (he == hipSuccess) he = hipMemcpy(out_norm, d_norm, 2 * obytes, hipMemcpyDeviceToHost);
        if (he == hipSuccess && out_stats) he = hipMemcpy(out_stats, d_stats, 4 * sizeof(double), hipMemcpyDeviceToHost);
        if (he == hipSuccess && out_box) he = hipMemcpy(out_box, d_box, 4 * sizeof(int), hipMemcpyDeviceToHost);
    }
    if (he == hipSuccess) he = hipMemcpy(out_max, d_max, obytes, hipMemcpyDeviceToHost);
    if (he == hipSuccess) he = hipMemcpy(out_mean, d_mean, obytes, hipMemcpyDeviceToHost);
    (void)hipFree(d);
    if (he != hipSuccess) return fail(TS2D_ERR_HIP, "ts2d_project_coronal failed: %s", hipGetErrorString(he));
    return TS2D_OK;
}

int ts2d_project_coronal(int device, const void* volume, size_t n_elems, int dtype, int nz, int ny, int nx, long long sz,
                         long long sy, long long sx, long long base, float* out_max, float* out_mean) {
    return project_coronal_impl(device, volume, n_elems, dtype, nz, ny, nx, sz, sy, sx, base, out_max, out_mean, nullptr, nullptr, nullptr);
}

int ts2d_project_coronal_zscore(int device, const void* volume, size_t n_elems, int dtype, int nz, int ny, int nx, long long sz,
                                long long sy, long long sx, long long base, float* out_max, float* out_mean, float* out_norm,
                                double* out_stats, int32_t* out_box) {
    if (!out_norm) return fail(TS2D_ERR_INVALID, "ts2d_project_coronal_zscore: null argument");
    return project_coronal_impl(device, volume, n_elems, dtype, nz, ny, nx, sz, sy, sx, base, out_max, out_mean, out_norm, out_stats, out_box);
}
// Taps of one axis of the order-3 resample (n_in -> n_out samples; preprocess.cubic_axis_taps is the same statement in numpy, pinned to
// scipy): cc = ((o + 0.5) * (n_in / n_out) - 0.5) + 12 clamped to the padded extent, start = floor(cc) - 1, y = cc - floor(cc), t = 1 - y,
// w1 = (y*y*(y-2)*3 + 4) / 6, w2 = (t*t*(t-2)*3 + 4) / 6, w0 = t*t*t / 6, w3 = 1 - w0 - w1 - w2, one rounding per step.  False if a tap
// would leave the padded line (with this map it cannot: cc lies in [11.5, n_in + 11.5]; checked because the kernel reads where it points).
static bool rsin_axis_taps(int n_in, int n_out, RsInTap* t) {
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
static const double kRsInPole = -0x1.126145e9ecd56p-2;
constexpr int kRsInMaxExtent = 8192;          // preprocess.CUBIC_MAX_EXTENT

static RsInAxis rsin_axis_constants(int n_pad) {
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

// The device part of the order-3 resample, shared by ts2d_resample_cubic (host planes in and out) and ts2d_planes_resample_cubic (planes that
// live on the device): the host tables of one (in_h, in_w) -> (out_h, out_w) zoom and the layout of the scratch they go to,
// [coefficients | powers | taps], then the three rsin_* launches over device pointers.
struct RsInPlan {
    int Hp = 0, Wp = 0;
    std::vector<RsInTap> taps;          // rows at [0, out_h), columns at [out_h, out_h + out_w)
    std::vector<double> zpow;           // running products of the pole, as scipy forms them (z_i *= z)
    RsInAxis ax_h, ax_w;
    size_t o_pow = 0, o_taps = 0, bytes = 0;
};

// false: a tap would leave the padded plane
static bool rsin_plan(int n_planes, int in_h, int in_w, int out_h, int out_w, RsInPlan* pl) {
    pl->Hp = in_h + 2 * kRsInPad; pl->Wp = in_w + 2 * kRsInPad;
    pl->taps.resize((size_t)out_h + out_w);
    if (!rsin_axis_taps(in_h, out_h, pl->taps.data()) || !rsin_axis_taps(in_w, out_w, pl->taps.data() + out_h)) return false;
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
    return true;
}

// d_scratch: pl.bytes; d_src [n_planes][in_h][in_w], d_lh [n_planes][2], d_dst [n_planes][out_h][out_w], all on the device
static hipError_t rsin_run(const RsInPlan& pl, char* d_scratch, const float* d_src, const float* d_lh, float* d_dst, int n_planes, int in_h,
                           int in_w, int out_h, int out_w) {
    double* d_coef = reinterpret_cast<double*>(d_scratch);
    const double* d_pow = reinterpret_cast<const double*>(d_scratch + pl.o_pow);
    const RsInTap* d_taps = reinterpret_cast<const RsInTap*>(d_scratch + pl.o_taps);
    hipError_t he = hipMemcpy(d_scratch + pl.o_pow, pl.zpow.data(), pl.zpow.size() * sizeof(double), hipMemcpyHostToDevice);
    if (he == hipSuccess) he = hipMemcpy(d_scratch + pl.o_taps, pl.taps.data(), pl.taps.size() * sizeof(RsInTap), hipMemcpyHostToDevice);
    if (he != hipSuccess) return he;
    hipLaunchKernelGGL(rsin_prefilter_cols, dim3((unsigned)(((long long)n_planes * pl.Wp + 63) / 64)), dim3(64), 0, 0,
                       d_src, n_planes, in_h, in_w, pl.ax_h, d_pow, d_coef);
    hipLaunchKernelGGL(rsin_prefilter_rows, dim3((unsigned)(((long long)n_planes * pl.Hp + 63) / 64)), dim3(64), 0, 0,
                       d_coef, n_planes, pl.Hp, pl.Wp, pl.ax_w, d_pow);
    const long long quads = (long long)n_planes * out_h * ((out_w + 3) / 4);
    hipLaunchKernelGGL(rsin_interp_clip, dim3((unsigned)((quads + 255) / 256)), dim3(256), 0, 0,
                       d_coef, n_planes, pl.Hp, pl.Wp, out_h, out_w, d_taps, d_lh, d_dst);
    return hipGetLastError();
}

int ts2d_resample_cubic(int device, const float* src, int n_planes, int in_h, int in_w, int out_h, int out_w, const float* lo_hi, float* dst) {
    if (!src || !lo_hi || !dst) return fail(TS2D_ERR_INVALID, "ts2d_resample_cubic: null argument");
    if (n_planes < 1) return fail(TS2D_ERR_INVALID, "ts2d_resample_cubic: %d planes", n_planes);
    if (in_h < 2 || in_w < 2 || out_h < 2 || out_w < 2 || in_h > kRsInMaxExtent || in_w > kRsInMaxExtent || out_h > kRsInMaxExtent || out_w > kRsInMaxExtent)
        return fail(TS2D_ERR_INVALID, "ts2d_resample_cubic: extents %d x %d -> %d x %d outside 2 ... %d", in_h, in_w, out_h, out_w, kRsInMaxExtent);
    const int Hp = in_h + 2 * kRsInPad, Wp = in_w + 2 * kRsInPad;
    if ((long long)n_planes * Hp * Wp > (1ll << 28) || (long long)n_planes * out_h * out_w > (1ll << 28))
        return fail(TS2D_ERR_INVALID, "ts2d_resample_cubic: %d planes of %d x %d -> %d x %d are more than one call takes (2^28 samples)", n_planes, in_h, in_w, out_h, out_w);
    for (int p = 0; p < n_planes; ++p)
        if (!std::isfinite(lo_hi[2 * p]) || !std::isfinite(lo_hi[2 * p + 1]) || lo_hi[2 * p] > lo_hi[2 * p + 1])
            return fail(TS2D_ERR_INVALID, "ts2d_resample_cubic: plane %d has non-finite or inverted clip bounds [%g, %g] (a plane with a non-finite sample is not computed here)",
                        p, (double)lo_hi[2 * p], (double)lo_hi[2 * p + 1]);
    RsInPlan pl;
    if (!rsin_plan(n_planes, in_h, in_w, out_h, out_w, &pl))
        return fail(TS2D_ERR_INVALID, "ts2d_resample_cubic: zoom %d x %d -> %d x %d puts a tap outside the padded plane", in_h, in_w, out_h, out_w);
    HIP_TRY(hipSetDevice(device));
    const size_t n_src = (size_t)n_planes * in_h * in_w, n_dst = (size_t)n_planes * out_h * out_w;
    // [scratch of the plan | source | clip bounds | result]
    const size_t o_src = pl.bytes, o_lh = align_up(o_src + n_src * sizeof(float), 256);
    const size_t o_dst = align_up(o_lh + (size_t)n_planes * 2 * sizeof(float), 256);
    char* d = nullptr;
    HIP_TRY(hipMalloc(reinterpret_cast<void**>(&d), o_dst + n_dst * sizeof(float)));
    float* d_dst = reinterpret_cast<float*>(d + o_dst);
    hipError_t he = hipMemcpy(d + o_src, src, n_src * sizeof(float), hipMemcpyHostToDevice);
    if (he == hipSuccess) he = hipMemcpy(d + o_lh, lo_hi, (size_t)n_planes * 2 * sizeof(float), hipMemcpyHostToDevice);
    if (he == hipSuccess)
        he = rsin_run(pl, d, reinterpret_cast<const float*>(d + o_src), reinterpret_cast<const float*>(d + o_lh), d_dst, n_planes, in_h, in_w, out_h, out_w);
    if (he == hipSuccess) he = hipMemcpy(dst, d_dst, n_dst * sizeof(float), hipMemcpyDeviceToHost);
    (void)hipFree(d);
    if (he != hipSuccess) return fail(TS2D_ERR_HIP, "ts2d_resample_cubic failed: %s", hipGetErrorString(he));
    return TS2D_OK;
}

// ---------------------------------------------------------------------------------------------------------------- ts2d_planes
// Planes that stay on the device between the steps of nnU-Net's preprocessing of a native 2-D input (kernels_prep.h): uploaded once,
// cropped, z-scored and resampled where they lie, downloaded once.
struct ts2d_planes {
    int device = 0;
    int n = 0, h = 0, w = 0;
    float* d = nullptr;         // [n][h][w]
    float* d_lh = nullptr;      // [n][2]: float32 minimum and maximum of each plane, valid while has_bounds
    bool has_bounds = false;
};

constexpr int kPrepMaxPlanes = 65535;           // (a grid dimension)
constexpr long long kPrepMaxSamples = 1ll << 28;

// leaves of numpy's pairwise sum over a run of n elements (the partial chunk of a plane), in the order the recursion visits them
static void prep_leaves(int off, int n, std::vector<PrepLeaf>* out) {
    if (n <= kPrepLeaf) { out->push_back(PrepLeaf{off, n}); return; }
    int n2 = n / 2; n2 -= n2 % 8;
    prep_leaves(off, n2, out);
    prep_leaves(off + n2, n - n2, out);
}

// the same recursion over the leaves' sums: every inner node adds its two halves, rounded to float32
static float prep_fold(const float*& leaf, int n) {
#pragma clang fp contract(off)
    if (n <= kPrepLeaf) return *leaf++;
    int n2 = n / 2; n2 -= n2 % 8;
    const float a = prep_fold(leaf, n2);
    const float b = prep_fold(leaf, n - n2);
    return a + b;
}

// numpy's add.reduce of one plane from what prep_chunk_sums wrote: +0, plus each chunk's pairwise sum in index order
static float prep_plane_sum(const float* sums, long long n) {
#pragma clang fp contract(off)
    const long long n_full = n / kPrepChunk;
    float acc = 0.f;
    for (long long c = 0; c < n_full; ++c) acc = acc + sums[c];
    if (n % kPrepChunk) { const float* leaf = sums + n_full; const float tail = prep_fold(leaf, (int)(n % kPrepChunk)); acc = acc + tail; }
    return acc;
}

static float prep_unkey(int key) { const int b = key < 0 ? key ^ 0x7FFFFFFF : key; float f; std::memcpy(&f, &b, 4); return f; }

int ts2d_planes_create(int device, const float* src, int n_planes, int h, int w, ts2d_planes** out) {
    if (!src || !out) return fail(TS2D_ERR_INVALID, "ts2d_planes_create: null argument");
    *out = nullptr;
    if (n_planes < 1 || n_planes > kPrepMaxPlanes) return fail(TS2D_ERR_INVALID, "ts2d_planes_create: %d planes outside 1 ... %d", n_planes, kPrepMaxPlanes);
    if (h < 1 || w < 1 || h > kRsInMaxExtent || w > kRsInMaxExtent)
        return fail(TS2D_ERR_INVALID, "ts2d_planes_create: extents %d x %d outside 1 ... %d", h, w, kRsInMaxExtent);
    if ((long long)n_planes * h * w > kPrepMaxSamples)
        return fail(TS2D_ERR_INVALID, "ts2d_planes_create: %d planes of %d x %d are more than one handle takes (2^28 samples)", n_planes, h, w);
    HIP_TRY(hipSetDevice(device));
    const size_t bytes = (size_t)n_planes * h * w * sizeof(float);
    float* d = nullptr; float* d_lh = nullptr;
    HIP_TRY(hipMalloc(reinterpret_cast<void**>(&d), bytes));
    hipError_t he = hipMalloc(reinterpret_cast<void**>(&d_lh), (size_t)n_planes * 2 * sizeof(float));
    if (he == hipSuccess) he = hipMemcpy(d, src, bytes, hipMemcpyHostToDevice);
    if (he != hipSuccess) {
        (void)hipFree(d); if (d_lh) (void)hipFree(d_lh);
        return fail(he == hipErrorOutOfMemory ? TS2D_ERR_NOMEM : TS2D_ERR_HIP, "ts2d_planes_create failed: %s", hipGetErrorString(he));
    }
    ts2d_planes* p = new ts2d_planes();
    p->device = device; p->n = n_planes; p->h = h; p->w = w; p->d = d; p->d_lh = d_lh;
    *out = p;
    return TS2D_OK;
}

int ts2d_planes_crop_zscore(ts2d_planes* p, int32_t box[4], float* stats, int* nonfinite) {
    if (!p || !box || !stats || !nonfinite) return fail(TS2D_ERR_INVALID, "ts2d_planes_crop_zscore: null argument");
    *nonfinite = 0;
    HIP_TRY(hipSetDevice(p->device));
    const int n = p->n;
    // scratch, sized for the uncropped extent: [box | min / max keys | mean, divisor | leaves of the partial chunk | chunk and leaf sums]
    const size_t per_plane = (size_t)((long long)p->h * p->w / kPrepChunk) + kPrepMaxTailLeaves;
    const size_t o_keys = 256, o_norm = align_up(o_keys + (size_t)n * 2 * sizeof(int), 256), o_leaves = align_up(o_norm + (size_t)n * sizeof(PrepNorm), 256);
    const size_t o_sums = align_up(o_leaves + kPrepMaxTailLeaves * sizeof(PrepLeaf), 256);
    char* d = nullptr;
    HIP_TRY(hipMalloc(reinterpret_cast<void**>(&d), o_sums + (size_t)n * per_plane * sizeof(float)));
    int* d_box = reinterpret_cast<int*>(d); int* d_keys = reinterpret_cast<int*>(d + o_keys);
    PrepNorm* d_norm = reinterpret_cast<PrepNorm*>(d + o_norm); PrepLeaf* d_leaves = reinterpret_cast<PrepLeaf*>(d + o_leaves);
    float* d_sums = reinterpret_cast<float*>(d + o_sums);
    float* d_new = nullptr;                                     // the compacted planes, until the handle owns them
    auto done = [&](hipError_t he) {
        (void)hipFree(d); if (d_new) (void)hipFree(d_new);
        if (he != hipSuccess) return fail(he == hipErrorOutOfMemory ? TS2D_ERR_NOMEM : TS2D_ERR_HIP, "ts2d_planes_crop_zscore failed: %s", hipGetErrorString(he));
        return (int)TS2D_OK;
    };
    // 1. crop_to_nonzero's box over all planes
    int hb[4] = {p->h, -1, p->w, -1};
    hipError_t he = hipMemcpy(d_box, hb, sizeof(hb), hipMemcpyHostToDevice);
    if (he != hipSuccess) return done(he);
    hipLaunchKernelGGL(prep_nonzero_box, dim3((unsigned)(((long long)p->h * p->w + 255) / 256)), dim3(256), 0, 0, p->d, n, p->h, p->w, d_box);
    he = hipGetLastError();
    if (he == hipSuccess) he = hipMemcpy(hb, d_box, sizeof(hb), hipMemcpyDeviceToHost);
    if (he != hipSuccess) return done(he);
    if (hb[1] < 0) { hb[0] = 0; hb[1] = p->h - 1; hb[2] = 0; hb[3] = p->w - 1; }            // nothing but zeros: the whole extent stays
    if (hb[0] < 0 || hb[1] >= p->h || hb[0] > hb[1] || hb[2] < 0 || hb[3] >= p->w || hb[2] > hb[3]) {
        (void)done(hipSuccess);
        return fail(TS2D_ERR_HIP, "ts2d_planes_crop_zscore: the device returned the box rows %d ... %d, columns %d ... %d of %d x %d", hb[0], hb[1], hb[2], hb[3], p->h, p->w);
    }
    const int bh = hb[1] - hb[0] + 1, bw = hb[3] - hb[2] + 1;
    // 2. compaction: the flattened index of the dense [n][bh][bw] buffer is numpy's
    if (bh != p->h || bw != p->w) {
        he = hipMalloc(reinterpret_cast<void**>(&d_new), (size_t)n * bh * bw * sizeof(float));
        for (int c = 0; c < n && he == hipSuccess; ++c)
            he = hipMemcpy2D(d_new + (size_t)c * bh * bw, (size_t)bw * sizeof(float), p->d + ((size_t)c * p->h + hb[0]) * p->w + hb[2],
                             (size_t)p->w * sizeof(float), (size_t)bw * sizeof(float), (size_t)bh, hipMemcpyDeviceToDevice);
        if (he != hipSuccess) return done(he);
        (void)hipFree(p->d);
        p->d = d_new; d_new = nullptr; p->h = bh; p->w = bw;
    }
    p->has_bounds = false;
    box[0] = hb[0]; box[1] = hb[1] + 1; box[2] = hb[2]; box[3] = hb[3] + 1;
    // 3. the two sums of every plane: chunk and leaf sums on the device, their fold and the float32 statistics here
    const long long N = (long long)bh * bw, n_full = N / kPrepChunk;
    std::vector<PrepLeaf> leaves;
    if (N % kPrepChunk) prep_leaves(0, (int)(N % kPrepChunk), &leaves);
    if ((int)leaves.size() > kPrepMaxTailLeaves) { (void)done(hipSuccess); return fail(TS2D_ERR_INVALID, "ts2d_planes_crop_zscore: %zu leaves in a partial chunk", leaves.size()); }
    const size_t n_out = (size_t)n_full + leaves.size();
    const dim3 grid_sums((unsigned)(n_full + (leaves.empty() ? 0 : 1)), (unsigned)n);
    std::vector<float> sums((size_t)n * n_out);
    std::vector<PrepNorm> norm((size_t)n, PrepNorm{0.f, 1.f});
    if (!leaves.empty()) he = hipMemcpy(d_leaves, leaves.data(), leaves.size() * sizeof(PrepLeaf), hipMemcpyHostToDevice);
    if (he != hipSuccess) return done(he);
    bool bad = false;
    for (int pass = 0; pass < 2; ++pass) {
        if (pass == 0) hipLaunchKernelGGL(prep_chunk_sums<0>, grid_sums, dim3(512), 0, 0, p->d, N, d_norm, d_leaves, (int)leaves.size(), d_sums);
        else hipLaunchKernelGGL(prep_chunk_sums<1>, grid_sums, dim3(512), 0, 0, p->d, N, d_norm, d_leaves, (int)leaves.size(), d_sums);
        he = hipGetLastError();
        if (he == hipSuccess) he = hipMemcpy(sums.data(), d_sums, sums.size() * sizeof(float), hipMemcpyDeviceToHost);
        if (he != hipSuccess) return done(he);
        for (int c = 0; c < n; ++c) {
            // numpy divides the float32 sum by the count in float64 and rounds once to float32 (`ret / rcount` with an intp count)
            const float q = (float)((double)prep_plane_sum(sums.data() + (size_t)c * n_out, N) / (double)N);
            if (!std::isfinite(q)) bad = true;
            if (pass == 0) { norm[c].mean = q; stats[2 * c] = q; }
            else { const float sd = std::sqrt(q); stats[2 * c + 1] = sd; norm[c].div = 1e-8 > (double)sd ? (float)1e-8 : sd; }   // max(std, 1e-8)
        }
        if (bad) { *nonfinite = 1; return done(hipSuccess); }      // a non-finite sample (or an overflowing sum): nothing is normalised
        he = hipMemcpy(d_norm, norm.data(), norm.size() * sizeof(PrepNorm), hipMemcpyHostToDevice);
        if (he != hipSuccess) return done(he);
    }
    // 4. normalise in place; the minimum and maximum of the result are the clip bounds of the resample
    std::vector<int> keys((size_t)n * 2);
    for (int c = 0; c < n; ++c) { keys[2 * c] = 0x7FFFFFFF; keys[2 * c + 1] = (int)0x80000000; }
    he = hipMemcpy(d_keys, keys.data(), keys.size() * sizeof(int), hipMemcpyHostToDevice);
    if (he != hipSuccess) return done(he);
    hipLaunchKernelGGL(prep_normalise, dim3((unsigned)((N + 256 * kPrepNormPerLane - 1) / (256 * kPrepNormPerLane)), (unsigned)n), dim3(256), 0, 0, p->d, N, d_norm, d_keys);
    he = hipGetLastError();
    if (he == hipSuccess) he = hipMemcpy(keys.data(), d_keys, keys.size() * sizeof(int), hipMemcpyDeviceToHost);
    if (he != hipSuccess) return done(he);
    std::vector<float> lh((size_t)n * 2);
    for (size_t i = 0; i < lh.size(); ++i) { lh[i] = prep_unkey(keys[i]); if (!std::isfinite(lh[i])) bad = true; }
    if (bad) { *nonfinite = 1; return done(hipSuccess); }          // (a quotient overflowed: the planes hold it, the caller drops the handle)
    he = hipMemcpy(p->d_lh, lh.data(), lh.size() * sizeof(float), hipMemcpyHostToDevice);
    if (he != hipSuccess) return done(he);
    p->has_bounds = true;
    return done(hipSuccess);
}

int ts2d_planes_resample_cubic(ts2d_planes* p, int out_h, int out_w) {
    if (!p) return fail(TS2D_ERR_INVALID, "ts2d_planes_resample_cubic: null argument");
    const int in_h = p->h, in_w = p->w, n = p->n;
    if (in_h < 2 || in_w < 2 || out_h < 2 || out_w < 2 || in_h > kRsInMaxExtent || in_w > kRsInMaxExtent || out_h > kRsInMaxExtent || out_w > kRsInMaxExtent)
        return fail(TS2D_ERR_INVALID, "ts2d_planes_resample_cubic: extents %d x %d -> %d x %d outside 2 ... %d", in_h, in_w, out_h, out_w, kRsInMaxExtent);
    if ((long long)n * (in_h + 2 * kRsInPad) * (in_w + 2 * kRsInPad) > (1ll << 28) || (long long)n * out_h * out_w > (1ll << 28))
        return fail(TS2D_ERR_INVALID, "ts2d_planes_resample_cubic: %d planes of %d x %d -> %d x %d are more than one call takes (2^28 samples)", n, in_h, in_w, out_h, out_w);
    if (!p->has_bounds)
        return fail(TS2D_ERR_STATE, "ts2d_planes_resample_cubic: the planes carry no clip bounds (ts2d_planes_crop_zscore computes them; a resample uses them up)");
    RsInPlan pl;
    if (!rsin_plan(n, in_h, in_w, out_h, out_w, &pl))
        return fail(TS2D_ERR_INVALID, "ts2d_planes_resample_cubic: zoom %d x %d -> %d x %d puts a tap outside the padded plane", in_h, in_w, out_h, out_w);
    HIP_TRY(hipSetDevice(p->device));
    char* d_scratch = nullptr; float* d_dst = nullptr;
    HIP_TRY(hipMalloc(reinterpret_cast<void**>(&d_scratch), pl.bytes));
    hipError_t he = hipMalloc(reinterpret_cast<void**>(&d_dst), (size_t)n * out_h * out_w * sizeof(float));
    if (he == hipSuccess) he = rsin_run(pl, d_scratch, p->d, p->d_lh, d_dst, n, in_h, in_w, out_h, out_w);
    if (he == hipSuccess) he = hipDeviceSynchronize();
    (void)hipFree(d_scratch);
    if (he != hipSuccess) {
        if (d_dst) (void)hipFree(d_dst);
        return fail(he == hipErrorOutOfMemory ? TS2D_ERR_NOMEM : TS2D_ERR_HIP, "ts2d_planes_resample_cubic failed: %s", hipGetErrorString(he));
    }
    (void)hipFree(p->d);
    p->d = d_dst; p->h = out_h; p->w = out_w; p->has_bounds = false;
    return TS2D_OK;
}

int ts2d_planes_extent(const ts2d_planes* p, int* h, int* w) {
    if (!p || !h || !w) return fail(TS2D_ERR_INVALID, "ts2d_planes_extent: null argument");
    *h = p->h; *w = p->w;
    return TS2D_OK;
}

int ts2d_planes_download(const ts2d_planes* p, float* dst) {
    if (!p || !dst) return fail(TS2D_ERR_INVALID, "ts2d_planes_download: null argument");
    HIP_TRY(hipSetDevice(p->device));
    HIP_TRY(hipMemcpy(dst, p->d, (size_t)p->n * p->h * p->w * sizeof(float), hipMemcpyDeviceToHost));
    return TS2D_OK;
}

int ts2d_planes_destroy(ts2d_planes* p) {
    if (!p) return TS2D_OK;
    (void)hipSetDevice(p->device);
    if (p->d) (void)hipFree(p->d);
    if (p->d_lh) (void)hipFree(p->d_lh);
    delete p;
    return TS2D_OK;
}
int ts2d_synth_slices(int device, unsigned long long key, unsigned long long first_element, unsigned long long n_elements,
                      float* out_device, void* stream) {
    if (!out_device) return fail(TS2D_ERR_INVALID, "ts2d_synth_slices: null output");
    if (n_elements == 0) return TS2D_OK;
    if (n_elements > (1ull << 40)) return fail(TS2D_ERR_INVALID, "ts2d_synth_slices: %llu elements in one call", n_elements);
    HIP_TRY(hipSetDevice(device));
    const unsigned long long per = 1ull << 30;                      // <= 2^30 elements per launch (grid of 2^22 blocks)
    for (unsigned long long o = 0; o < n_elements; o += per) {
        const unsigned long long m = std::min(per, n_elements - o);
        hipLaunchKernelGGL(synth_normal, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                           out_device + o, key, first_element + o, m);
        HIP_TRY(hipGetLastError());
    }
    return TS2D_OK;
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
                if (t.normed) { v = v * sc[(size_t)b * C + c] + sh[(size_t)b * C + c]; v = v > 0.f ? v : v * e->arch.leaky_slope; }
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

