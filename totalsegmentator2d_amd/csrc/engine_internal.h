// Host-side internals of libts2d_engine.so, shared by the plain C++ files (program.cpp, pack_weights.cpp, dispatch.cpp, tiled_plan.cpp,
// prep_plan.cpp) and the seven device units: the program (tensors, ops), the kernel choice of an op, the workspace layout, the engine
// handle, the plans of the sliding window and of the input side.  Not installed, not part of the ABI (include/ts2d_engine.h is).
// (What the entries that need no engine share of their call scaffolding is entry_util.h beside it.)
// No device code here or in the .cpp files: they build without an offload pass.  Kernels live in engine.hip (the network), tiled.hip
// (the sliding window, fold mean and export), prep.hip (projection, input resample, native 2-D planes), post.hip (largest-component
// postprocessing), visual.hip (the PNG visuals; its host tables, visual_plan.cpp, have a header of their own), stats.hip (the per-label
// statistics of a segmentation), evaluate.hip (scoring a segmentation against a reference) and morph.hip (grow, shrink, open and close every
// label by a radius in mm), each kernel in exactly one.
#pragma once
#include "../../include/ts2d_engine.h"
#include <hip/hip_runtime_api.h>
#include "device_tables.h"
#include "tile_dims.h"

#include <atomic>
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#pragma GCC visibility push(hidden)      // (the library exports the C-ABI only)
namespace ts2d {

// thread-local last error (ts2d_last_error): ONE definition for every object of the library (program.cpp)
int fail(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));
const char* last_error();

#define HIP_TRY(expr)                                                                                     \
    do {                                                                                                  \
        hipError_t _e = (expr);                                                                           \
        if (_e != hipSuccess)                                                                             \
            return fail(_e == hipErrorOutOfMemory ? TS2D_ERR_NOMEM : TS2D_ERR_HIP, "%s failed: %s (%s:%d)", \
                        #expr, hipGetErrorString(_e), __FILE__, __LINE__);                                \
    } while (0)
#define TRY(expr) do { int _rc = (expr); if (_rc != TS2D_OK) return _rc; } while (0)

// Owner of one hipMalloc on the input side (prep.hip): freed when it leaves its scope, so an early HIP_TRY return leaks nothing; a
// handle (ts2d_planes) takes a buffer over by move.  The engine's long-lived buffers are not these: ts2d_engine_destroy frees them.
class DevMem {
public:
    DevMem() = default;
    DevMem(DevMem&& o) noexcept : p_(o.release()) {}
    DevMem& operator=(DevMem&& o) noexcept { if (this != &o) { reset(); p_ = o.release(); } return *this; }
    ~DevMem() { reset(); }
    hipError_t alloc(size_t bytes) { reset(); return hipMalloc(&p_, bytes); }
    template <class T> T* as(size_t byte_off = 0) const { return reinterpret_cast<T*>(static_cast<char*>(p_) + byte_off); }
    void* release() { void* p = p_; p_ = nullptr; return p; }
    void reset() { if (p_) (void)hipFree(p_); p_ = nullptr; }
private:
    void* p_ = nullptr;
};

constexpr size_t kWsHeader = 256;         // bytes in front of the activation plan: [0] = token of the last run inside this memory

enum OpType { OP_CONV = 0, OP_CONVT = 1, OP_HEAD = 2,
              OP_PROJ = 3,      // residual skip path: average pool over the block's stride + 1x1 conv (no bias) + statistics (kernels_resblock.h)
              OP_JOIN = 4 };    // residual join: norm2(conv2) + residual, stored before the LeakyReLU with scale 1 / shift 0

struct Tensor {            // an activation tensor of the program (NHWC fp32)
    std::string name;
    int C = 0, level = 0;
    int Cu = 0;            // channels of the CALLER's architecture (C is the width the kernels run: rounded up to 32 - pad_arch)
    int ly = 0, lx = 0;    // log2 of the cumulative stride along H / W: extent (H >> ly, W >> lx) (per-axis strides, ABI 7)
    bool normed = false;   // raw conv output that carries InstanceNorm scale/shift
    bool linear = false;   // normalised but never activated (conv2 and the projection of a residual block): only the join reads it
    float* data = nullptr; float* scale = nullptr; float* shift = nullptr;
    size_t bytes = 0;      // of its buffer in the workspace plan (0: none)
    bool resident = false; // its buffer still holds the values of the last run (no later tensor of the run was placed on it)
};

struct Op {
    OpType type; std::string name;
    int src, skip, dst;           // tensor indices (skip = -1 if none)
    int res = -1;                 // third source (-1 if none): the residual a join adds - the block's input, or its projection
    int cin, cin_skip, cout, stride, level;      // stride: 1 = (1, 1), 2 = (2, 2) - the dedicated kernels; 3 = anisotropic (generic kernel only)
    int sy = 1, sx = 1;           // stride along H / W (conv: of the conv; transposed conv: kernel = stride of the upsampling)
    int ly = 0, lx = 0;           // shifts of the op's level (= of its output tensor; the head: level 0)
    int ck;                       // Cin chunk of the packed weight layout
    size_t blob_w, blob_b, blob_g, blob_be;     // offsets (floats) into the PyTorch-layout blob
    size_t dev_w, dev_b, dev_g, dev_be;         // offsets (floats) into the device weight arena
    size_t dev_w_floats;
    bool split_ok = false;        // eligible for the split-fp16 kernel (3x3, stride 1, Cin % 16 == 0, not the net input)
    size_t dev_wh = 0;            // offset (floats) of the split-fp16 weights in the arena
    size_t dev_wh32 = 0;          // offset (floats) of the fp16 weights in 32-channel chunks (precision mode f16, kernels_h32.h)
    bool h32_ok = false;
    size_t dev_ws = 0;            // offset (floats) of 1 / (power-of-two pre-scale of the split weights)
    size_t dev_wp = 0;            // offset (floats) of the split-fp16 weights in plane order [chunk16][column tile][tap][hi,lo][h][column][8 halves]
                                  // (conv3x3_f16x3_qp; stride-1 split_ok convs)
    bool s2v2_ok = false;         // stride-2 block: 512-thread kernel of kernels_s2v2.h
    size_t dev_w2 = 0;            // offset (floats) of its weight image [chunk16][column tile][tap][hi,lo][h][column][8 halves]
    int bn2 = 0;                  // its column tile (128 or 64)
    bool res_ok = false;          // 32 -> 32 stride-1 block: resident-weight persistent kernel (kernels_res32.h)
    size_t dev_wres = 0;          // offset (floats) of its weight image [tap][hi,lo][g][cout][8 halves]
    bool upc_ok = false;          // decoder c0 block whose "up" half is composed with the preceding ConvTranspose2d (kernels_upc.h)
    int up_idx = -1;              // ... index of that transposed conv in the program
    size_t dev_wc = 0;            // composed weights [chunk Cb/16][column tile][16 = (A,B,dI,dJ)][hi,lo][h][column][8 halves]
    size_t dev_wk = 0;            // skip half of the 3x3 weights [chunk Cs/16][column tile][tap][hi,lo][h][column][8 halves]
    size_t dev_wcs = 0;           // 1 / (their common power-of-two pre-scale)
    size_t dev_bvar = 0;          // [9 = (ry, rx)][Cout] bias variants
    bool up0_ok = false;          // ... with 64 coarse, 32 skip and 32 output channels (level 0 of the canonical net): kernels_up0.h
    size_t dev_w0c = 0;           // composed weights in fragment order [parity 4][k-step 8][hi,lo][cb 2][lane 64][8 halves]
    size_t dev_w0k = 0;           // skip half, resident image [tap 9][hi,lo][g 4][cout 32][8 halves]
    bool first_direct = false;    // first conv block handled by conv3x3_first (reads the NCHW boundary tensor)
    size_t dev_wraw = 0;
};

struct Launch { std::string name, kernel; int ksplit = 1; hipEvent_t e0 = nullptr, e1 = nullptr; };

inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// Pixel tiling of one level: tile = NIMG images x TH x TW pixels, NIMG * TH * TW <= 256 (a workgroup's 256 GEMM rows).
struct TileGeom { int TH, TW, NIMG, lgTH, lgTW, tiles_x, tiles_y, n_mtiles, PH, PW; };

enum Kern { K_NONE = 0, K_FUSED_AWAY, K_FIRST, K_FIRST_STATS, K_EXACT, K_S1_GENERIC, K_S1_ONE, K_S1_QP, K_S1_H32, K_S1_H2, K_S1_RES32, K_S1_RES32F,
            K_S2_V2, K_S2_ONE, K_S2_GENERIC, K_T_ONE, K_T_GENERIC, K_UP0, K_UPQ, K_UPC, K_UPC_H, K_UPC_H2, K_HEAD_MFMA, K_HEAD_1X1, K_PROJ, K_JOIN };

struct Choice {
    Kern k = K_NONE;
    TileGeom g{};               // the pixel tiling the kernel walks
    int bn = 0;                 // output columns per workgroup
    int ksplit = 1;
    bool fused_stats = false;   // per-tile partial statistics come out of the kernel's epilogue (else stats_direct / splitk_reduce_stats)
    int ppt = 1;                // ... partials per tile and channel (conv3x3_up0: one per wave)
    bool first_full = false;    // (K_FIRST*) complete one-image 256-pixel tiles: the persistent variant
    bool flex = false;          // (K_UPC / K_UPC_H / K_S2_V2) the level is no multiple of 8 x 32: the FLEX instance on the tile c.g
    bool first_split = false;   // (K_FIRST*) the K = 9 C contraction as one fp16 hi / lo split product (kernels_first.h SPLIT; else the exact fp32 MFMA)
    bool k32 = false;           // (K_S2_V2) 16-bit mode: chunks of 32 channels (kernels_s2v2.h K32)
    int npp = 0, nch = 0;       // (K_S2_V2) LDS planes per (tap, k half), channel chunks
    bool s2p = false;           // (K_S2_V2) the pipelined split-mode instance conv3x3s2_v2p (kernels_s2v2p.h); same reported name, same bits
    int seg = 0;                // (K_UP0 / K_S1_RES32*) tiles per workgroup segment (segment_tiles)
    int ks = 0;                 // (K_UPC_H / K_UPC_H2) coarse k-steps per staged chunk
    bool half = false;          // (K_PROJ / K_JOIN) the fp16-storage instance (16-bit mode, option "resf16")
    const char* name = "";      // what ts2d_engine_op_kernel reports for the op (tests and scripts/pmc_traffic.py key on these strings)
};

inline int pow2ceil(int v) { int p = 1; while (p < v) p <<= 1; return p; }
inline int ilog2(int v) { int l = 0; while ((1 << l) < v) ++l; return l; }
inline int ct_total(const Op& op) { return op.cin + op.cin_skip; }
// (K_S2_V2) every chunk's weight block of the column tile stays in LDS beside the patch
inline size_t s2v2_wchunk(const Choice& c) { return (size_t)9 * c.npp * 2 * c.bn * 16; }
inline bool s2v2_resident(const Choice& c) { return (size_t)c.npp * 2 * kS2PlaneBytes + (size_t)c.nch * s2v2_wchunk(c) <= (size_t)kS2LdsMax; }

}  // namespace ts2d

#pragma GCC visibility pop

struct ts2d_engine {
    ts2d_arch_desc arch{};
    int lvl_y[TS2D_MAX_STAGES] = {0}, lvl_x[TS2D_MAX_STAGES] = {0};      // per stage: log2 of the cumulative stride along H / W
    int device = 0;
    int cin_pad = 8;
    std::vector<ts2d::Tensor> tensors;
    std::vector<ts2d::Op> ops;
    size_t blob_floats = 0;
    ts2d_arch_desc user_arch{};        // the descriptor the caller gave; `arch` is what the kernels run (pad_arch)
    bool residual = false;             // ResidualEncoderUNet (ts2d_engine_create_residual): stem + BasicBlockD stages; n_conv_enc is ignored
    int n_blocks[TS2D_MAX_STAGES] = {0};      // ... blocks per stage
    bool padded = false;
    size_t user_blob_floats = 0;       // floats of the caller's blob (== blob_floats unless padded)
    float* d_weights = nullptr; size_t weight_floats = 0;
    bool weights_ready = false;
    int precision = TS2D_PRECISION_F32_SPLIT_F16X3;
    int num_cus = 256;
    int tile_half = 0;            // sliding-window blend order (ts2d_engine_set_tile_dtype): 0 = fp32 tile (reference CPU path)
    int tiled_inf = 0;            // the last predict_tiled produced an infinite aggregated logit (ts2d_engine_tiled_inf_flag)
    // Kernel-dispatch options (ts2d_engine_set_option; ABI 6).  Each selects between two complete, parity-tested kernels for the ops it
    // names; the defaults are the measured-fastest ones.  They are per-HANDLE state set through the C-ABI - the caller's environment
    // never changes which kernel runs.
    bool use_one = true;          // "one": one-image-tile kernels (0: the generic ones; also switches every kernel built on them off)
    bool use_s2v2 = true;         // "s2v2": 512-thread stride-2 kernel
    bool use_q = true;            // "q": persistent 512-thread double-buffered stride-1 kernel on 16 x 32 tiles (0: conv3x3_f16x3_one)
    bool use_h2 = true;           // "h2": 16-bit plain C -> C blocks on 16 x 32 tiles (0: conv3x3_h32)
    bool use_uh2 = true;          // "uh2": 16-bit composed block on 16 x 32 tiles (0: conv3x3_upc_h)
    bool use_s2k32 = true;        // "s2k32": 16-bit mode - the 512-thread stride-2 kernel on 32-channel chunks (0: 16-channel chunks)
    bool use_s2p = true;          // "s2p": split mode - the pipelined instance of the 512-thread stride-2 kernel at 128 columns (0: conv3x3s2_v2<128> itself, its bit-identical twin)
    bool use_sbk = true;          // "sbk": small batches - split-K (and the two-kernel decoder entry) where the preferred kernel would leave most CUs idle (fill_ksplit)
    bool use_first_split = true;  // "first_split": the first block's contraction as one fp16 hi / lo split product (kernels_first.h SPLIT; 0: exact fp32 MFMA)
    bool use_up0 = true;          // "up0": dedicated persistent kernel of the level-0 composed block (0: conv3x3_upc<32>)
    int u0seg = 0;                // "u0seg": tiles per workgroup segment of conv3x3_up0 (0: chosen from the grid; tests force segments that end inside an image)
    bool use_upc = true;          // "upc": decoder c0 blocks composed with their transposed conv (0: two kernels)
    bool use_res = true;          // "res": resident-weight kernel of the 32 -> 32 blocks
    bool use_fuse0 = true;        // "fuse0": first block recomputed inside the second (statistics-only pre-pass + conv3x3_res32 fused variant)
    bool diagnosing = false;      // the re-run of ts2d_engine_check: the first block as its own kernel whatever "fuse0" says (its output can be scanned and named)
    int use_flex2 = 2;            // "flex2": conv3x3s2_v2 on level-dividing tiles where the level is no multiple of 8 x 32 (0: off, 1: 16-bit mode only, 2: both)
    bool use_resf16 = false;      // "resf16": the 16-bit mode on a residual-encoder engine (opt-in: 0 refuses TS2D_PRECISION_F16 there, as before the mode existed)
    bool use_flex = true;         // "flex": the composed decoder entry on extent-following tiles at levels that are no multiple of 8 x 32 (0: two kernels there)
    int dbg = 0;                  // TS2D_DBG (the one environment switch left): timing ablations / in-kernel phase stamps of diagnostic runs
    unsigned long long* d_prof = nullptr;     // TS2D_DBG=256: in-kernel phase counters, 8 per op (diagnostic)
    std::vector<char> fused_away; // per op of the last run: 1 = its output tensor was not materialised (composed into the next op)
    // workspace
    char* d_ws = nullptr; size_t ws_bytes = 0; int wsB = 0, wsH = 0, wsW = 0;
    bool ws_external = false;     // d_ws is the caller's memory (ts2d_engine_set_workspace): shared by the engines of a sub-model set
    uint32_t ws_token = 0;        // ... token this engine's last run wrote into its header (g_ws_generation)
    // the kernel choices of the last (B, H, W, precision, options): a forward of the same shape does not search tile shapes again
    // (62 launches per forward: at B = 1 the host side is a visible part of the 2.5 ms)
    std::vector<ts2d::Choice> plan; int planB = 0, planH = 0, planW = 0, plan_prec = -1; unsigned plan_gen = 0, opt_gen = 1; bool plan_full = false;
    char* d_stage = nullptr; size_t stage_bytes = 0;      // host-buffer forwards only (ensure_staging)
    bool ws_full = false;         // the activation plan of the workspace is the full-batch dispatch's (ensure_workspace)
    bool last_full = false;       // the last run took the full-batch dispatch (ts2d_engine_check re-runs it the same way)
    int ws_precision = -1; bool ws_keep = false;      // the activation plan of the workspace was made for this mode (composition depends on it)
    bool keep_activations = false;                    // ts2d_engine_set_keep_activations: one buffer per tensor (debug access, full diagnosis)
    float* d_part = nullptr;
    float* d_partial = nullptr;   // split-K partial outputs
    float* d_up = nullptr;        // scratch for ONE upsampled tensor (small batches: a decoder entry that the reserved batch's plan composes runs as two kernels)
    float* d_in_stage = nullptr; float* d_logit_stage = nullptr; uint32_t* d_mask_stage = nullptr;
    hipStream_t stream = nullptr;
    bool profiling = false;
    std::vector<ts2d::Launch> launches; size_t n_launched = 0;
    int lastB = 0, lastH = 0, lastW = 0; hipStream_t last_stream = nullptr; bool last_f16 = false;
    char* d_sw = nullptr; size_t sw_bytes = 0;     // sliding-window scratch (image, batch, tile logits, outputs)
    // The activation workspace is shared by every call on this handle, whatever stream the caller passes: the end of each run
    // is marked with an event, and a run issued on ANOTHER stream first waits for it (no host synchronisation).
    hipEvent_t ws_event = nullptr; hipStream_t ws_stream = nullptr; bool ws_busy = false;
    int* d_flags = nullptr;       // [0]: a logit of the last run was inf / NaN (set by the head kernels); [1]: scratch of the diagnosis
    bool checked_input = false; const float* last_input = nullptr;      // (synchronous paths: the staged input can be scanned too)
};

#pragma GCC visibility push(hidden)
namespace ts2d {

// ---- program.cpp: the descriptor as a program of ops over tensors, and the device weight arena's layout
ts2d_arch_desc pad_arch(const ts2d_arch_desc& a, bool& padded);
// n_blocks: the blocks per stage of a residual encoder, or null for a plain one
void expand_blob(const ts2d_arch_desc& ua, const ts2d_arch_desc& pa, const int* n_blocks, const float* ub, std::vector<float>& pb);
int build_program(ts2d_engine* e);
int tensor_index(ts2d_engine* e, const std::string& name);      // -1: no such tensor
// The per-image limit of a forward (reserve_checked refuses beyond it): bytes of the largest plane one image occupies - the widest activation tensor
// or the NCHW input, at four bytes per element in every mode - and the bound the kernels' per-image buffer resources and 32-bit in-image byte
// offsets set for it.  `widest`: index of that tensor (-1: the input).  Host arithmetic only: swept on the CPU by tests/plan_driver.cpp.
constexpr long long kImagePlaneMax = (1LL << 31) - 1;
long long image_plane_bytes(const ts2d_engine* e, int H, int W, int* widest);
bool image_extent_ok(const ts2d_engine* e, int H, int W);
long long call_pixel_limit(const ts2d_engine* e);      // B * H * W of a call stays below it: 2^31, or 2^29 - 31 on a residual encoder (res_join's launch)

// ---- pack_weights.cpp: PyTorch-layout blob -> packed device layouts (host staging buffer `out`, weight_floats long)
void pack_weights(const ts2d_engine* e, const float* blob, float* out);
float f16_to_f32(uint16_t hb);

// ---- dispatch.cpp: which kernel serves an op, and the workspace that follows from it
// Small-batch split-K (fill_ksplit): S x B x HW x Cout of any op the rule splits (n_wgs S < 2 x 256 CUs, <= 256 pixels x 64 columns each).
// The bound is asserted against every split op of a sweep of nets, extents and batches: tests/test_workspace_plan_cpu.py, W3.
constexpr size_t kSbkElems = (size_t)2 * 256 * 256 * 64;
// `full`: the run asks for the full-batch dispatch whatever its size (ts2d_engine_predict_tiled_batch: a row's bits must not depend on its batch).
// No default anywhere: every caller names the dispatch it means.
constexpr bool kBySize = false, kFullBatch = true;

Choice choose(const ts2d_engine* e, size_t oi, int B, int H, int W, bool full);
std::vector<Choice> choose_all(const ts2d_engine* e, int B, int H, int W, bool full);
const std::vector<Choice>& planned(ts2d_engine* e, int B, int H, int W, bool full);

struct ActPlan { std::vector<size_t> off, size; std::vector<char> used, reused; size_t bytes = 0; };
// Layout of the activation workspace for (B, H, W) under the engine's current precision mode, options and keep flag.
struct WsLayout {
    ActPlan plan; std::vector<size_t> o_sc, o_sh; size_t o_part = 0, o_pk = 0, o_up = 0, bytes = 0;
    bool has_up = false;      // the scratch of one upsampled tensor exists at o_up (small batches: a decoder entry the reserved batch's plan composes)
};
WsLayout workspace_layout(const ts2d_engine* e, int B, int H, int W, bool full);

// ---- engine.hip: what the sliding window (tiled.hip) needs of the engine
int reserve_checked(ts2d_engine* e, int B, int H, int W, bool full);      // shape checks of a forward, then the workspace for it
int run_forward(ts2d_engine* e, const float* d_in, int B, int H, int W, float* d_logits, uint32_t* d_mask, hipStream_t st, bool clear_flags, bool full);

// ---- tiled_plan.cpp: everything of a sliding-window call that is decided before the device is touched
struct SwChunk { int seg0, n_segs, rows, log_row; bool aggregate; unsigned gblocks, ablocks; };      // one gather + forward (+ aggregate)
struct SwPlan {
    int V = 1, vflips = 0;                  // mirror variants per tile and their flips, 8 bits each
    int cap_rows = 0;                       // rows of the largest chunk: the batch every fold reserves
    long long n_tiles_all = 0, out_elems = 0, rs_blocks = 0;
    bool any16 = false, anyseg = false, any_rs8 = false, any_rs32 = false;
    std::vector<SwSeg> segs; std::vector<SwChunk> chunks; std::vector<RsSeg> rsegs;
    std::vector<ProbSeg> psegs; long long prob_elems = 0;      // a probabilities call: one per image beside its RsSeg; elements of the float outputs
    std::vector<ProbStackSeg> pssegs;       // ... of runs (ts2d_ensemble_predict_tiled_probabilities_stack): these in the place of psegs, at tab_psegs too
    std::vector<char> tab;                  // [segments | tile_y | tile_x | export (or label-map) segments | their taps | class order | probabilities segments (ProbSeg, or ProbStackSeg of runs)]: one host blob, one copy
    size_t tab_segs = 0, tab_rsegs = 0, tab_rtaps = 0, tab_order = 0, tab_psegs = 0;
    // scratch: [table | gaussian | images | one chunk's batch | tile logits | half outputs x F | uint8 outputs | flags x F | resampled uint8 (or label maps, or decided maps) | resampled float | probabilities]
    size_t o_tab = 0, o_g = 0, o_imgs = 0, o_batch = 0, o_log = 0, o_o16 = 0, o_seg = 0, o_flag = 0, o_rs8 = 0, o_rs32 = 0, o_prob = 0, bytes = 0;
};
// The TAIL of a sliding-window call: what becomes of the aggregated half logits (the mean's, of an ensemble) behind the last sw_aggregate
// or sw_fold_mean.  One kernel per kind, then that kind's device-to-host copies (tiled.hip: run_tail):
//   kNone        nothing: the padded outputs of the images are the call's results
//   kExport      sw_resample_threshold: K uint8 and / or K float planes [out_h, out_w] per image (u8 = seg_u8, f32 = logits_f32)
//   kLabelmap    sw_labelmap: ONE uint8 plane per image (u8 = label_u8)
//   kRegions     sw_regions: the same plan and plane, painted by `class_order`, which rides in the table blob at tab_order
//   kProb        sw_probabilities<ProbSeg>: K float planes of the pre-crop extent per image (f32 = prob_f32), the decided map beside them (u8 =
//                decided_u8, or null); `mode` is a ProbMode = TS2D_PROB_* and `class_order` that of its regions mode (else null); a segment's
//                lanes walk the full extent and the ProbSegs go behind the class order at tab_psegs
//   kProbRuns    sw_probabilities<ProbStackSeg>: the outputs are those of `runs` of slices, head-major in the caller's strided volumes; `images`
//                is the entry's per-image expansion of them (a run's geometry, the slice's place in the caller's arrays) and run_of[i] the run of
//                image i.  The entry has checked that the runs cover the images once, in order, and that a run's images share (Hp, Wp).
struct SwTail {
    enum Kind { kNone, kExport, kLabelmap, kRegions, kProb, kProbRuns };
    struct Image { int src_y, src_x, src_h, src_w, out_h, out_w, full_h, full_w, box_y, box_x; uint8_t* u8; float* f32; };
    Kind kind = kNone;
    std::vector<Image> images;              // one per image of the call (kNone: none)
    int mode = 0; const uint8_t* class_order = nullptr;
    const ts2d_tiled_probabilities_run* runs = nullptr; int n_runs = 0; std::vector<int> run_of;

    SwTail() = default;
    SwTail(Kind k, int n_images) : kind(k), images((size_t)n_images, Image{}) {}
    bool prob() const { return kind == kProb || kind == kProbRuns; }
    const char* what() const { return prob() ? "probabilities" : kind == kRegions ? "regions" : kind == kLabelmap ? "labelmap" : "export"; }      // in a message
    int planes(int K) const { return kind == kExport ? K : 1; }         // of an image's resampled uint8 output
    int decided_planes(int K) const { return mode == kProbMultilabel ? K : 1; }      // ... of its decided map (prob())
    bool no_output(const Image& t) const { return kind == kExport ? !t.u8 && !t.f32 : prob() ? !t.f32 : !t.u8; }
    // the six numbers every descriptor begins with (ts2d_tiled_export, _labelmap, _probabilities, _probabilities_run)
    template <class D> static Image rect_of(const D& d, uint8_t* u8, float* f32) {
        return Image{d.src_y, d.src_x, d.src_h, d.src_w, d.out_h, d.out_w, 0, 0, 0, 0, u8, f32};
    }
    template <class D> static Image full_of(const D& d, uint8_t* u8, float* f32) {      // ... and the four of a probabilities descriptor
        Image t = rect_of(d, u8, f32);
        t.full_h = d.full_h; t.full_w = d.full_w; t.box_y = d.box_y; t.box_x = d.box_x;
        return t;
    }
};
int plan_tiled(const ts2d_engine* e, int F, const ts2d_tiled_image* images, const SwTail& tail, int n_images, int ph, int pw, int mirror_mask,
               bool name_images, const char* entry, SwPlan* pl);
// Image i's segment and taps of the tail's resample (checked extents): appended to rsegs / rtaps, `blocks` and `rs_elems` advanced.
// src_off: elements to the image's [K, Hp, Wp] half planes.  (Also what the ts2d_*_from_logits entries plan their one image with.)
// A probabilities segment: the lanes walk the full extent, 4 X each, and rs_elems is left alone (it may be null).
void rs_plan_segment(const SwTail& tail, int i, int K, int Hp, int Wp, long long src_off, std::vector<RsSeg>* rsegs, std::vector<RsTap>* rtaps,
                     long long* blocks, long long* rs_elems);

// ---- prep_plan.cpp: the host arithmetic of the input side, bit for bit numpy's / scipy's
// The host tables of one (in_h, in_w) -> (out_h, out_w) order-3 zoom and the layout of the scratch they go to: [coefficients | powers | taps]
struct RsInPlan {
    int Hp = 0, Wp = 0;
    std::vector<RsInTap> taps;          // rows at [0, out_h), columns at [out_h, out_h + out_w)
    std::vector<double> zpow;           // running products of the pole, as scipy forms them (z_i *= z)
    RsInAxis ax_h, ax_w;
    size_t o_pow = 0, o_taps = 0, bytes = 0;
};
int rsin_plan(const char* entry, int n_planes, int in_h, int in_w, int out_h, int out_w, RsInPlan* pl);      // fails if a tap would leave the padded plane
void prep_leaves(int off, int n, std::vector<PrepLeaf>* out);
float prep_plane_sum(const float* sums, long long n);
float prep_rescale_div(float mn, float mx);
float prep_unkey(int key);
// The geometry of a synthetic radiograph as its two entries take it, and the float64 ray tables made of it (xray.xr_tables in numpy): sample j of
// ray (k, i) lies at x = cx[i] + t[j] * a[i], z = cz[k] + t[j] * b[k]; p and q give the ray's step length (xr_step).
struct XrGeometry {
    int nz, ny, nx; double sx, sy, sz, sdd, sod; int pa, parallel; double du, dv; int nu, nv;
};
struct XrPlan {
    std::vector<double> t, a, cx, p, b, cz, q;      // t [ny]; a, cx, p [nu]; b, cz, q [nv]
    double sy = 0.0; bool parallel = false; int nu = 0, nv = 0;
};
int xr_plan(const char* entry, const XrGeometry& g, XrPlan* pl);      // refuses, by name, what xray.XRGeometry.resolve refuses
double xr_step(const XrPlan& pl, int k, int i);
void xr_finish(const XrPlan& pl, const double* sum, float* out);       // out [nv][nu] = float32(sum * step)

}  // namespace ts2d
#pragma GCC visibility pop
