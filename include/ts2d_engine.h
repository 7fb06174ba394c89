/* ts2d_engine.h - C-ABI of the MI355X-native 2-D U-Net inference engine (libts2d_engine.so).
 *
 * Drop-in boundary.  The reference has no FFI: its seam is the duck-typed predictor object
 * consumed by `_run_predict` (reference ts2d/core/inference/prediction_worker.py:177-242).  These entry points are
 * what a ctypes/cffi binding placed at that seam binds; each cites the reference interface it replaces.
 * Plain pointers and sizes only - no torch / HIP types in any signature (streams travel as void*).
 *
 * Error convention (replaces Python exceptions, reference prediction_worker.py:183-242 / nnu.py:217-219): every
 * function returns 0 on success or a negative ts2d_status; ts2d_last_error() returns a thread-local message that
 * the Python layer converts to RuntimeError.  The library never aborts the process.
 *
 * Threading: one caller thread per engine handle (reference: one worker process per sub-model, one task at a
 * time, prediction_worker.py:127-165).  Handles are independent (different sub-models / GPUs).
 */
#ifndef TS2D_ENGINE_H
#define TS2D_ENGINE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TS2D_MAX_STAGES 16

typedef enum {
    TS2D_OK = 0,
    TS2D_ERR_INVALID = -1,     /* bad argument / unsupported architecture or shape */
    TS2D_ERR_HIP = -2,         /* a HIP runtime call or kernel launch failed */
    TS2D_ERR_NOMEM = -3,       /* device or host allocation failed */
    TS2D_ERR_STATE = -4        /* engine not initialised (e.g. weights not yet broadcast) */
} ts2d_status;

/* Architecture descriptor = the `arch_kwargs` of nnU-Net's PlainConvUNet that
 * `nnUNetPredictor.initialize_from_trained_model_folder` (reference call site ts2d/core/inference/nnu.py:165) reads
 * from plans.json.  Supported subset: Conv2d 3x3, stride (1, 1) in the first stage and 1 or 2 PER AXIS afterwards (nnU-Net's
 * planner pools each axis separately: (2, 2) until one axis is exhausted, then (2, 1) / (1, 2)), InstanceNorm2d(affine), LeakyReLU,
 * ConvTranspose2d upsampling with kernel = stride = the stride of the stage below, 1x1 head.  features[]: any positive width, features[0] <= 64; a width that
 * is not a multiple of 32 runs rounded up to one with zero weights in the added channels (exact; the weight blob keeps the caller's layout).
 * (2, 2) stages run the dedicated kernels; any other stride runs a generic implicit-GEMM kernel (correct, not tuned). */
typedef struct {
    int32_t input_channels;                 /* C: len(dataset_json['channel_names']) (prediction_worker.py:78) */
    int32_t num_classes;                    /* K: number of segmentation heads (multilabel: one per label) */
    int32_t n_stages;
    int32_t features[TS2D_MAX_STAGES];
    int32_t n_conv_enc[TS2D_MAX_STAGES];
    int32_t n_conv_dec[TS2D_MAX_STAGES];    /* n_stages-1 entries, bottom-up (decoder.stages.{j}) */
    float norm_eps;                         /* InstanceNorm2d eps (1e-5) */
    float leaky_slope;                      /* LeakyReLU negative_slope (0.01) */
    int32_t strides[TS2D_MAX_STAGES][2];    /* ABI 7: arch_kwargs['strides'][s] = (along H, along W), 1 or 2 each; [0] = (1, 1).
                                             * An all-zero entry s >= 1 reads as (2, 2) (descriptors written for ABI <= 6). */
} ts2d_arch_desc;

/* Arithmetic of the dense 3x3 contractions (storage, accumulation, statistics and I/O are fp32 in both modes):
 *   TS2D_PRECISION_F32_EXACT       v_mfma_f32_32x32x2_f32: bit-for-bit an fp32 FMA chain (157 TFLOP/s peak).
 *   TS2D_PRECISION_F32_SPLIT_F16X3 (default) operands split into fp16 hi + lo (22 significant bits) and multiplied
 *       as hi*hi + hi*lo + lo*hi on v_mfma_f32_32x32x16_f16 with fp32 accumulation; measured as close to the fp64
 *       truth as ATen's native fp32 conv on the canonical net.  Activations must stay below
 *       65504 in magnitude (always true after InstanceNorm for |gamma| < 127). */
#define TS2D_PRECISION_F32_EXACT 0
#define TS2D_PRECISION_F32_SPLIT_F16X3 1
/*   TS2D_PRECISION_F16  "mixed fp16" (BASELINE configs 3 and 5): activations stored as fp16 in HBM (half the traffic), weights
 *       rounded to fp16, ONE fp16 MFMA product per MAC, fp32 accumulation and fp32 InstanceNorm statistics; logits are
 *       still returned as fp32.  NOT within the fp32 parity tolerance (logit error ~1e-2); selected explicitly.
 *   Residual blocks under TS2D_PRECISION_F16 (ts2d_engine_create_residual; opt-in: option "resf16").  h(.) rounds to IEEE half and back,
 *   act16(y) = max(y, h(y * h(slope))) for a half y - what every 16-bit consumer does at load time.
 *     stem, conv1, decoder blocks: as every plain block of the mode (the stem's weights are not rounded, like the first block of a plain
 *       net); the operand the next op multiplies is a = act16(h(scale * stored + shift)).
 *     conv2: stored y2 = h(conv(a, h(w)) + b); statistics in fp32 over the stored values; n2 = fma(scale, y2, shift) stays fp32 in the join.
 *     residual r, fp32: the identity skip r = a (the half conv1 multiplies); a pooled skip the fp32 sum of the window's a in row-major
 *       order, times 1 / n; a projection p = h(conv1x1(h(pool(a)), h(w))) (no bias), statistics in fp32 over the stored p,
 *       r = fma(scale_p, p, shift_p), not rounded.
 *     join: t = h(n2 + r) - ONE rounding, on the store - kept as half with scale 1 / shift 0, so that every consumer's load gives act16(t).
 *     ts2d_engine_debug_tensor shows the storage view of a join as of every tensor: leaky_relu(t) in fp32. */
#define TS2D_PRECISION_F16 2

typedef struct ts2d_engine ts2d_engine;

/* Create an engine on HIP device `device`.
 * Replaces: nnUNetPredictor(...).initialize_from_trained_model_folder(model, folds, checkpoint) for ONE fold
 * (reference nnu.py:164-165): network construction + load_state_dict.
 * `weights`: host pointer to the fp32 blob = every parameter tensor in PyTorch layout, concatenated in program order
 * (encoder.stages.{s}.0.convs.{i}.{conv.weight,conv.bias,norm.weight,norm.bias} ..., decoder.transpconvs.{j}.{weight,
 * bias}, decoder.stages.{j}.convs.{i}..., decoder.seg_layers.{n-2}.{weight,bias}); n_floats must match exactly.
 * `weights` may be NULL: the engine is then created with uninitialised device weights that MUST be filled by a
 * broadcast into ts2d_engine_weight_buffer() followed by ts2d_engine_weights_ready() (multi-GPU replicas). */
int ts2d_engine_create(const ts2d_arch_desc* arch, const float* weights, size_t n_floats, int device,
                       ts2d_engine** out);

/* nnU-Net's ResidualEncoderUNet (the nnUNetResEncUNet{M,L,XL}Plans presets; 2-D, `block` = BasicBlockD): what it adds to the descriptor.
 * The encoder is a stem (Conv 3x3 stride 1 + bias, InstanceNorm, LeakyReLU: input_channels -> features[0]) and per stage s n_blocks[s]
 * blocks out = lrelu(conv2(conv1(x)) + skip(x)): conv1 = Conv 3x3 (block 0: the stage's stride) + bias, norm, LeakyReLU; conv2 = Conv 3x3 +
 * bias, norm, NO non-linearity; skip = the identity, or AvgPool2d(kernel = stride) where the block has a stride, followed by Conv 1x1
 * WITHOUT bias + norm (no non-linearity) where the block changes the width.  Decoder and head are those of ts2d_arch_desc. */
typedef struct {
    int32_t n_blocks[TS2D_MAX_STAGES];      /* arch_kwargs['n_blocks_per_stage'], >= 1 each */
    int32_t reserved[16];                   /* must be zero */
} ts2d_residual_desc;

/* ts2d_engine_create for a ResidualEncoderUNet.  `arch`: as above, its n_conv_enc is ignored.  Not supported (TS2D_ERR_INVALID):
 * bottleneck blocks, squeeze-excitation, a stem width other than features[0], conv_bias = False - the descriptor cannot even name them;
 * the caller (arch.py: UNetArch.from_plans) refuses such plans.
 * Blob order (PyTorch layouts, n_floats must match exactly):
 *   encoder.stem.convs.0.{conv.weight, conv.bias, norm.weight, norm.bias};
 *   per stage s and block b: encoder.stages.{s}.blocks.{b}.conv1.{conv.weight, conv.bias, norm.weight, norm.bias}, then
 *   ...conv2.{conv.weight, conv.bias, norm.weight, norm.bias}, then - only where features[s - 1] != features[s], b = 0 - the projection
 *   ...skip.{i}.{conv.weight [Cout, Cin, 1, 1], norm.weight, norm.bias} (i = 1 behind an AvgPool2d, else 0);
 *   then the decoder and the head exactly as for ts2d_engine_create.
 * Every entry that takes an engine takes this one.  TS2D_PRECISION_F32_SPLIT_F16X3 and TS2D_PRECISION_F32_EXACT are supported;
 * ts2d_engine_set_precision(e, TS2D_PRECISION_F16) returns TS2D_ERR_INVALID and leaves the mode unchanged unless the option "resf16" is
 * set on the handle (ts2d_engine_set_option; the contract of a residual block in that mode: TS2D_PRECISION_F16 above).
 * ts2d_engine_debug_tensor names: "stem", "enc{s}.b{b}.c1", "enc{s}.b{b}.c2" and "enc{s}.b{b}.proj" (normalised, NOT activated - as the
 * join reads them) and "enc{s}.b{b}" (the block's output); the decoder's names are unchanged. */
int ts2d_engine_create_residual(const ts2d_arch_desc* arch, const ts2d_residual_desc* residual, const float* weights, size_t n_floats,
                                int device, ts2d_engine** out);

/* Replace the weights of an existing engine (fold switch: `network.load_state_dict(params)` in
 * predict_logits_from_preprocessed_data, reference call site prediction_worker.py:209). */
int ts2d_engine_load_weights(ts2d_engine* e, const float* weights, size_t n_floats);

/* Select the arithmetic mode (see TS2D_PRECISION_*); takes effect at the next forward. */
int ts2d_engine_set_precision(ts2d_engine* e, int mode);

/* Kernel-dispatch options (ABI 6; replaces the TS2D_* environment switches of ABI <= 5 - a product library must not change kernels
 * because of its caller's environment).  Several ops have two complete, parity-tested kernels (e.g. the decoder entry composed
 * with its ConvTranspose2d, or as two kernels); an option picks one for THIS handle, takes effect at the next reserve / forward and
 * never changes results beyond fp32 summation order (every switch has a parity test on each of its sides).  Names (value 0 / 1 unless noted):
 *   "upc" composed decoder entry | "up0" dedicated level-0 composed kernel | "u0seg" (int) its tiles per workgroup segment, 0 = automatic | "q" persistent 16x32-tile stride-1 kernel |
 *   "one" one-image-tile kernels | "res" resident-weight 32 -> 32 kernel | "fuse0" first block recomputed inside the second |
 *   "s2v2" 512-thread stride-2 kernel | "s2p" its pipelined split-mode instance at 128 output columns (two patch buffers, weights from L2;
 *   0: the single-buffered instance, bit-identical - test scaffolding) | "h2", "uh2", "s2k32": the 16-bit mode's variants | "flex" the composed decoder
 *   entry on tiles that follow the level's extent where it is no multiple of 8 x 32 pixels (0: transposed conv + conv there) |
 *   "flex2" (int) the 512-thread stride-2 kernel on tiles that divide such a level (0: off, 1: 16-bit mode only, 2: every mode) |
 *   "first_split" the first block's K = 9 C contraction as one fp16 hi / lo split product (0: exact fp32 MFMA) |
 *   "sbk" the small-batch dispatch: where the preferred kernel of an op would launch fewer workgroups than the device has CUs (the
 *   <= 32 x 32 levels of one ... eight slices - what TS2D.predict and the reference's B = 1 loop run), K is split over more workgroups
 *   (deterministic two-phase reduction) and a composed decoder entry runs as transposed conv + conv.  With "sbk" on (the default) a
 *   slice's result is bit-identical between two batches only if both take the same path (e.g. any two batches >= 32 of the canonical
 *   net); across paths it agrees to fp32 summation order (3e-5 on the logits).  The same batch always reproduces its bits.
 *   "resf16" (default 0) the 16-bit mode on a residual-encoder engine: with 1, ts2d_engine_set_precision(e, TS2D_PRECISION_F16) succeeds there
 *   and the residual blocks run their fp16-storage kernels (res_join<_Float16>, pool_proj1x1_h).  Cleared while such an engine is in the
 *   16-bit mode, the next forward fails (the mode is never changed silently).  No effect on a plain engine.  Not test scaffolding: the opt-in
 *   of a mode whose results differ from the fp32 modes'.
 * Most of these have had one measured winner for rounds ("q", "res", "one", "s2v2", "up0" ...): they are test scaffolding -
 * the way the parity suite reaches the second kernel of an op - not tuning knobs of the product.
 * Unknown names and out-of-range values return TS2D_ERR_INVALID.  The reference has no counterpart (one code path through torch:
 * ts2d/core/inference/prediction_worker.py:209); the callers are this repo's tests and A/B scripts. */
int ts2d_engine_set_option(ts2d_engine* e, const char* name, int value);

/* Weight-broadcast hook: device pointer + byte size of the packed weight arena.  Rank 0 creates with
 * weights, the other ranks with NULL; all ranks broadcast this buffer (RCCL, root 0), then call
 * ts2d_engine_weights_ready(). */
int ts2d_engine_weight_buffer(ts2d_engine* e, void** dev_ptr, size_t* n_bytes);
int ts2d_engine_weights_ready(ts2d_engine* e);

/* One batched forward pass = `network(x)` (reference: nnUNetPredictor.network.__call__ inside
 * _internal_maybe_mirror_and_predict; the reference always uses B = 1).
 *   input        [B, C, H, W] fp32 NCHW (what `data[None]` is in the reference), host or device memory
 *   logits       [B, K, H, W] fp32 NCHW or NULL
 *   mask_packed  [B, K, H, W/32] uint32 or NULL: bit (x & 31) of word x>>5 = (sigmoid(float(logit)) > 0.5), the
 *                multilabel export predicate (reference export_prediction_from_logits, prediction_worker.py:215-221)
 *   H, W         multiples of the product of the strides along their axis (2^(n_stages-1) for an isotropic plan); W multiple of 32
 *                when mask_packed != NULL
 *   on_device    nonzero: input/logits/mask_packed are device pointers; zero: host pointers (staged by the engine)
 *   stream       hipStream_t as void* (NULL = the engine's own stream).  The call is asynchronous when on_device
 *                != 0 (caller synchronises the stream) and synchronous otherwise.
 * Size limits, both refused by name with TS2D_ERR_INVALID before any workspace is allocated (ts2d_engine_reserve and the sliding-window
 * entries, whose forwards run on the patch extent, inherit them):
 *   per call     B * H * W < 2^31 pixels; on a residual-encoder engine B * H * W <= 2^29 - 32 (the join launches 256 threads per 32 pixels).
 *   per image    no plane of ONE image may pass 2^31 - 1 bytes, counted at four bytes per element in every precision mode: the widest
 *                activation tensor, (H >> ly) * (W >> lx) * C * 4 over the levels of the net with C the stage's width rounded up to a
 *                multiple of 32, and the input, C_in * H * W * 4.  For a net whose widest plane is level 0 at width 32 that is
 *                H * W <= 16 777 215 pixels (4094 x 4096 passes, 4096 x 4096 is refused); (32, 512) on two stages is bound by level 1:
 *                H * W <= 4 194 303.  Reason: the kernels address an image through 32-bit byte offsets ("32-bit
 *                quantities of the forward path"). */
int ts2d_engine_forward(ts2d_engine* e, const float* input, int B, int H, int W, float* logits,
                        uint32_t* mask_packed, int on_device, void* stream);

/* Result check of the LAST forward / predict_tiled (synchronises it): TS2D_OK, or TS2D_ERR_INVALID when a logit came out inf / NaN,
 * with ts2d_last_error() naming the first layer (program order) whose output holds a non-finite value.  The split and f16 modes
 * multiply fp16 operands: an activation of magnitude >= 65504 at a conv input (impossible after InstanceNorm for |gamma| < 127,
 * possible for an un-normalised transposed-conv output with adversarial weights) overflows to inf - this check turns that into an
 * error instead of a silent inf; TS2D_PRECISION_F32_EXACT has no such limit.  (The network INPUT is not under that limit: the first block
 * checks every tile's input inside its kernel and computes a tile that holds |x| >= 262 016, an inf or a NaN with the exact fp32
 * MFMAs - same result, slower.)  Host-buffer forwards and ts2d_engine_predict_tiled
 * run it themselves; after an asynchronous device-pointer forward the caller may.  (Reference convention: a failing prediction
 * raises, ts2d/core/inference/prediction_worker.py:211-212; upstream nnU-Net only checks the aggregated array for inf.) */
int ts2d_engine_check(ts2d_engine* e);

/* Sliding-window inference of ONE preprocessed 2-D image on the device (replaces the body of nnU-Net's
 * predict_sliding_window_return_logits + _internal_maybe_mirror_and_predict for one fold: reference call site
 * ts2d/core/inference/prediction_worker.py:209; SURVEY.md rows A3-A5, and A7 for `seg`).
 *   image          host [C, Hp, Wp] fp32, already padded to at least the patch (pad_nd_image is the caller's job)
 *   tile_y/tile_x  host, n_tiles tile origins in upstream order (compute_steps_for_sliding_window)
 *   mirror_mask    bit 0: mirror spatial axis 0 (H), bit 1: axis 1 (W); variants run in upstream order H, W, HW
 *   gaussian_f16   host [patch_h, patch_w] IEEE half bits (compute_gaussian), or NULL for no weighting
 *   logits_f16     host [K, Hp, Wp] half bits: aggregated logits / n_predictions in upstream's float16 buffers (rounding
 *                  order: ts2d_engine_set_tile_dtype; equal bit for bit to the repo's ATen-pinned oracle); may be NULL
 *   seg_u8         host [K, Hp, Wp]: sigmoid(float(logit)) > 0.5 of the aggregated logits (multilabel export); may be NULL
 * All tiles x mirror variants go through the network as one batch (chunks of at most 64 rows).  Synchronous.
 * This is ts2d_engine_predict_tiled_batch with one image - the same host code and kernels - except for the dispatch of the network:
 * here it depends on the batch size (option "sbk"), there it never does (the determinism rule below). */
int ts2d_engine_predict_tiled(ts2d_engine* e, const float* image, int Hp, int Wp, int patch_h, int patch_w, int n_tiles,
                              const int32_t* tile_y, const int32_t* tile_x, int mirror_mask, const uint16_t* gaussian_f16,
                              uint16_t* logits_f16, uint8_t* seg_u8);

/* Sliding-window inference of N preprocessed 2-D images as ONE engine batch (ABI 8).  Replaces the reference's way of driving several
 * inputs at once - `apply` submits every input to its worker pool before it waits for any (ts2d/core/inference/nnu.py:194-216) and each
 * worker runs predict_logits_from_preprocessed_data per input (ts2d/core/inference/prediction_worker.py:209) - by one call: the rows
 * (tile x mirror variant) of all images travel through the network together, so a folder of cases, or the z slices of a stack, pay one
 * stream synchronise per call and run at the large-batch rate of the kernels.
 *   images         n_images descriptors.  Extents and tile counts may differ per image; patch, mirror_mask, gaussian_f16 and the tile
 *                  dtype (ts2d_engine_set_tile_dtype) are shared.  Per image: `image`, Hp, Wp, n_tiles, tile_y, tile_x, logits_f16 and
 *                  seg_u8 mean what they mean in ts2d_engine_predict_tiled (at least one output non-NULL); inf_flag is written by the
 *                  call: 1 if this image's aggregated logits hold an inf.  ts2d_engine_tiled_inf_flag() is the OR over the images.
 *   n_images == 0  returns TS2D_OK and does nothing.
 * Every argument is validated before any device work; an error names the image ("image 3: tile 1 at (..) leaves ..") and nothing is written.
 * Determinism rule: inside ts2d_engine_predict_tiled_batch the network always takes the full-batch dispatch (no "sbk" split-K, composed
 * decoder entries stay composed), whatever the size of a chunk.  A row's logits are then a function of its own pixels and the weights
 * only: a case's logits_f16 / seg_u8 bytes are identical whatever its batch-mates, its position in the batch and the batch size, and
 * identical, bit for bit, to ts2d_engine_predict_tiled on an engine with option "sbk" = 0.  Against the default single-case path ("sbk"
 * on) they agree to fp32 summation order: a few float16 ulps at most on the aggregated logits (each rounding into the half buffer may flip).  The handle's options are not touched.
 * (A batch of ONE small case is slower this way than ts2d_engine_predict_tiled - 4.3 against 4.0 ms at 8 rows of the canonical net.)
 * Row packing: the n_tiles x V rows of an image are consecutive; chunks of at most 64 rows are filled greedily with whole images; an
 * image with more than 64 rows takes chunks of its own, split in 64s.  Per chunk: one gather launch, one forward, one aggregate launch.
 * Device scratch (grown before the first launch, kept by the handle): R x (K + C) x patch_h x patch_w x 4 bytes with
 * R = max(rows of the fullest chunk <= 64, rows of the largest image) - NOT n_images x rows - plus, summed over the images,
 * C x Hp x Wp x 4 (inputs) and K x Hp x Wp x 3 (half + uint8 outputs, each only if some image asks for it), plus 64 bytes per
 * (image, chunk) pair and 8 per tile.  Canonical net (K = 26, C = 2, 512 x 512 patch), 8 cases of 512 x 768: 64 rows -> 1.88 GB of tile
 * logits + batch, 0.27 GB of inputs and outputs.  Synchronous: one stream synchronise per call, then ts2d_engine_check. */
typedef struct {
    const float*   image;        /* host [C, Hp, Wp] fp32, already padded to at least the patch */
    int32_t        Hp, Wp;
    int32_t        n_tiles;
    const int32_t* tile_y;       /* host, n_tiles origins in upstream order */
    const int32_t* tile_x;
    uint16_t*      logits_f16;   /* host [K, Hp, Wp] half bits, or NULL */
    uint8_t*       seg_u8;       /* host [K, Hp, Wp], or NULL */
    int32_t        inf_flag;     /* out: this image's aggregated logits hold an inf */
} ts2d_tiled_image;

int ts2d_engine_predict_tiled_batch(ts2d_engine* e, ts2d_tiled_image* images, int n_images, int patch_h, int patch_w,
                                    int mirror_mask, const uint16_t* gaussian_f16);

/* The sliding window of ts2d_engine_predict_tiled_batch followed, on the device, by the export's resample-back and threshold.  Replaces
 * `export_prediction_from_logits` (reference call site ts2d/core/inference/prediction_worker.py:215-221) up to the crop-insert: nnU-Net
 * resamples the logits of a case whose spacing is not the plan's back to the extent the case had before preprocessing
 * (`resampling_fn_probabilities`: skimage resize, order 1, mode 'edge', per plane for the 2-D configurations) and thresholds them
 * (multilabel: sigmoid(float(logit)) > 0.5).  Here one kernel (csrc/kernels_resample.h) does both where the aggregation left the half
 * logits, so K uint8 planes of the ORIGINAL extent travel to the host instead of K float16 planes of the network's extent that the host
 * widens, interpolates and thresholds.
 *   exports        n_images descriptors, one per image.  (src_y, src_x, src_h, src_w): the rectangle of the aggregated [K, Hp, Wp] logits
 *                  that is the prediction - what pad_nd_image's revert slices cut out; (out_h, out_w): the extent after resampling
 *                  (`shape_after_cropping_and_before_resampling`, in plane).  seg_u8 [K, out_h, out_w]: float32(value) > 1.5 * 2^-24, the
 *                  predicate of seg_u8 in ts2d_engine_predict_tiled; logits_f32 [K, out_h, out_w]: the resampled logits themselves.  At least
 *                  one of the two is non-NULL.  Arithmetic: per axis cc = (o + 0.5) * (n_in / n_out) - 0.5, i0 = floor(cc), w1 = cc - i0,
 *                  w0 = 1 - w1 in float64 on the host, the two indices i0 and i0 + 1 clamped to [0, n_in - 1] (not the coordinate); per
 *                  pixel (((a00*wy0)*wx0 + (a01*wy0)*wx1) + (a10*wy1)*wx0) + (a11*wy1)*wx1 in float64 without FMA, ONE rounding to
 *                  float32 - bit for bit what scipy's zoom(order=1, mode='nearest', grid_mode=True) returns (skimage's resize calls it),
 *                  +-inf samples included; restated in numpy as totalsegmentator2d_amd.preprocess.resize_linear_f64.  With out extent
 *                  == src extent the taps degenerate to weights 1 / 0 and seg_u8 equals the un-resampled seg_u8 of the rectangle.
 *   images         as in ts2d_engine_predict_tiled_batch, except that logits_f16 and seg_u8 of an image may both be NULL: the half
 *                  buffer then lives in the scratch only.  inf_flag is written as there.
 *   full_batch     0: the size-dependent dispatch of ts2d_engine_predict_tiled; nonzero: the full-batch dispatch and with it the
 *                  determinism rule of ts2d_engine_predict_tiled_batch (an image's bytes do not depend on its batch-mates).
 * Every argument is validated before any device work, the image named in the message (an empty source rectangle or one that leaves
 * the image, a non-positive output extent, both export outputs NULL, 2^31 or more output elements, 2^26 or more output rows + columns
 * in one call); nothing is written then.
 * Device scratch: that of ts2d_engine_predict_tiled_batch (the half outputs always) plus, summed over the images,
 * K x out_h x out_w bytes (x 5 with logits_f32 asked for) and 24 bytes per output row and column (the tap tables) + 40 per image.
 * Synchronous: ONE stream synchronise per call, then ts2d_engine_check.  n_images == 0 returns TS2D_OK and does nothing.
 * (Added under ABI 9: new symbols only, no existing signature or structure changes, so ts2d_abi_version() stays 9.) */
typedef struct {
    int32_t  src_y, src_x, src_h, src_w;   /* rectangle of the aggregated [K, Hp, Wp] logits that is the prediction (un-padded) */
    int32_t  out_h, out_w;                 /* extent after resampling back */
    uint8_t* seg_u8;                       /* host [K, out_h, out_w], or NULL */
    float*   logits_f32;                   /* host [K, out_h, out_w], or NULL */
} ts2d_tiled_export;

int ts2d_engine_predict_tiled_export(ts2d_engine* e, ts2d_tiled_image* images, const ts2d_tiled_export* exports, int n_images,
                                     int patch_h, int patch_w, int mirror_mask, const uint16_t* gaussian_f16, int full_batch);

/* ts2d_engine_predict_tiled_export for a FOLD ENSEMBLE: the folds of a model folder (reference: `folds` of model.json go straight into the
 * predictor, ts2d/core/inference/nnu.py:31-33,146-165) as one call, the mean of their logits taken on the device.  Replaces upstream's
 * predict_logits_from_preprocessed_data (reached from ts2d/core/inference/prediction_worker.py:209) - per fold load the parameters and
 * `prediction += predict_sliding_window_return_logits(data)`, then `prediction /= n` when n > 1, in the float16 of the aggregated
 * logits - and the export behind it, so that neither F x K half planes per case travel to the host nor numpy adds halves there.
 *   engines        n_engines handles (1..32), one per fold, in fold order; all on one device, with the same input channels, num_classes,
 *                  precision mode and tile dtype, weights ready.  The other layers may differ.
 *   per fold f     exactly the sliding window ts2d_engine_predict_tiled_export(engines[f], ...) runs: the same row packing, the same
 *                  chunks of at most 64 rows, the same dispatch (`full_batch` and its determinism rule mean what they mean there), so
 *                  fold f's aggregated half logits are byte for byte what the single-engine entries give for that engine.
 *   the mean       one kernel (csrc/kernels_fold.h) over the F half buffers, per element and in fold order:
 *                  acc = x[0]; acc = half(float(acc) + float(x[f])) for f = 1 .. F-1; acc = half(float(acc) / float(half(F))) - the fp32
 *                  add and the correctly rounded fp32 division of numpy's float16 `+` and `/`, each rounded to nearest even, bit for bit
 *                  (+-inf, subnormals and signed zeros as IEEE has them; a NaN stays a NaN).  n_engines == 1: no mean kernel - the
 *                  call is byte-identical to ts2d_engine_predict_tiled_export on that engine (`exports` NULL, full_batch != 0: to
 *                  ts2d_engine_predict_tiled_batch); upstream divides only when n > 1.
 *   outputs        of the MEAN: images[i].logits_f16 and seg_u8 (the predicate on the mean), exports[i].seg_u8 and logits_f32 (the mean
 *                  resampled back) as in the single-engine entry.  `exports` may be NULL: every image then names at least one output.
 *   inf_flag       images[i].inf_flag is the OR over the folds of fold f's flag for image i - upstream looks at every fold's aggregated
 *                  array, not at the mean; ts2d_engine_tiled_inf_flag(engines[f]) is fold f's own OR over the images.
 * Every argument is validated before any device work and nothing is written on an error: a null array, n_engines outside 1..32, a
 * null handle ("engine 2 is null"), a fold whose weights are not ready (TS2D_ERR_STATE, "fold 1: weights not loaded"), folds on
 * different devices or differing in input channels, num_classes, precision mode or tile dtype (the fold and the property named), and
 * per image everything ts2d_engine_predict_tiled_export rejects, in the same words.  n_images == 0 returns TS2D_OK and does nothing.
 * The folds run one after the other on the FIRST engine's stream, and engines[0] holds all scratch: that of
 * ts2d_engine_predict_tiled_export ONCE (tile logits and gathered batch, R x (K + C) x patch_h x patch_w x 4 bytes, the uploaded inputs,
 * the export's outputs) - only the half outputs exist per fold: n_engines x K x Hp x Wp x 2 bytes summed over the images, plus
 * 4 bytes per (fold, image).  Each fold keeps its own activation workspace; the caller may give the folds a shared one with
 * ts2d_engine_set_workspace, which is legal here because they run on one stream.
 * Synchronous: ONE stream synchronise per call, then ts2d_engine_check for every fold; a failure is reported as "fold <f>: <message>".
 * (Added under ABI 9: a new symbol only, so ts2d_abi_version() stays 9.) */
int ts2d_ensemble_predict_tiled_export(ts2d_engine* const* engines, int n_engines, ts2d_tiled_image* images, const ts2d_tiled_export* exports,
                                       int n_images, int patch_h, int patch_w, int mirror_mask, const uint16_t* gaussian_f16, int full_batch);

/* ts2d_ensemble_predict_tiled_export for a LABEL-MAP model - the ordinary nnU-Net head: len(labels) heads with background at 0, whose export
 * is "resample the logits back, then take the argmax over the heads" (`export_prediction_from_logits`, reference call site
 * ts2d/core/inference/prediction_worker.py:215-221, without the multilabel fork's sigmoid).  One kernel (csrc/kernels_labelmap.h) does
 * both where the aggregation (or the mean of the folds) left the half logits, so ONE uint8 plane of the ORIGINAL extent travels to the
 * host instead of K float16 planes of the network's extent that the host widens, interpolates and compares.
 *   engines        as in ts2d_ensemble_predict_tiled_export: n_engines handles (1..32) in fold order, the same sliding window per fold,
 *                  the same mean.  n_engines == 1 is the single-model case: no mean kernel, as there.
 *   labelmaps      n_images descriptors, one per image.  (src_y, src_x, src_h, src_w) and (out_h, out_w) mean what they mean in
 *                  ts2d_tiled_export; label_u8 [out_h, out_w] (not NULL): per pixel the index of the head with the largest value.
 *                  The value compared per head is that of ts2d_tiled_export.logits_f32, bit for bit (float64 products and sums without
 *                  FMA, ONE rounding to float32) - except where (out_h, out_w) == (src_h, src_w): the host route does not resample then,
 *                  and the value is the widened half itself (no taps: an infinite logit stays infinite instead of meeting a zero weight).
 *                  The comparison is numpy's argmax on float32: the first index of the maximum wins, +0 and -0 are equal, a NaN beats
 *                  every number and the first NaN wins.  Restated in numpy as totalsegmentator2d_amd.export.labelmap_statement.
 *   images         as in ts2d_engine_predict_tiled_export: logits_f16 and seg_u8 of an image may both be NULL; logits_f16 asked for in
 *                  the same call are the (mean) half logits the label map was taken from.  inf_flag is written as in the ensemble entry
 *                  (the OR over the folds); ts2d_engine_tiled_inf_flag(engines[f]) is fold f's own.
 *   full_batch     as in ts2d_engine_predict_tiled_export (nonzero: an image's bytes do not depend on its batch-mates).
 * Every argument is validated before any device work and nothing is written on an error: what ts2d_ensemble_predict_tiled_export
 * refuses of the engines, in the same words; per image what ts2d_engine_predict_tiled_export refuses, the image named, with "labelmap:"
 * where it says "export:" (an empty source rectangle or one that leaves the image, a non-positive output extent, a NULL label_u8, 2^31 or
 * more output elements, 2^26 or more output rows + columns in one call).  n_images == 0 returns TS2D_OK and does nothing.
 * Device scratch, all held by engines[0]: that of ts2d_ensemble_predict_tiled_export without its resampled outputs (tile logits and
 * gathered batch once, the half outputs n_engines x K x Hp x Wp x 2 bytes summed over the images, 4 bytes per (fold, image)) plus, summed
 * over the images, out_h x out_w bytes (the label maps) and 24 bytes per output row and column of an image that resamples + 40 per image.
 * Synchronous: ONE stream synchronise per call, then ts2d_engine_check for every fold; a failure is reported as "fold <f>: <message>".
 * (Added under ABI 9: new symbols only, no existing signature or structure changes, so ts2d_abi_version() stays 9.) */
typedef struct {
    int32_t  src_y, src_x, src_h, src_w;   /* rectangle of the aggregated [K, Hp, Wp] logits that is the prediction (un-padded) */
    int32_t  out_h, out_w;                 /* extent after resampling back */
    uint8_t* label_u8;                     /* host [out_h, out_w] */
} ts2d_tiled_labelmap;

int ts2d_ensemble_predict_tiled_labelmap(ts2d_engine* const* engines, int n_engines, ts2d_tiled_image* images, const ts2d_tiled_labelmap* labelmaps,
                                         int n_images, int patch_h, int patch_w, int mirror_mask, const uint16_t* gaussian_f16, int full_batch);

/* The label-map kernel of ts2d_ensemble_predict_tiled_labelmap on half planes the CALLER supplies (so that it can be tested on values no
 * network produces: ties, signed zeros, subnormals, infinities, NaN): logits_f16 host [K, H, W] half bits, rect = {src_y, src_x, src_h,
 * src_w} inside [H, W], label_u8 host [out_h, out_w].  Same arithmetic, same comparator, same identity rule.  Host pointers in and out,
 * synchronous, scratch of the call's own, freed on every path.  TS2D_ERR_INVALID, by name, before any device work: null pointers, K
 * outside 1 ... 256, a non-positive extent or 2^31 or more elements, a rectangle that is empty or leaves the planes, a bad output extent.
 * (A new symbol of ABI 9: nothing that existed changed.) */
int ts2d_labelmap_from_logits(int device, const uint16_t* logits_f16, int K, int H, int W, const int32_t rect[4], int out_h, int out_w,
                              uint8_t* label_u8);

/* ts2d_ensemble_predict_tiled_labelmap for a REGION-BASED model - nnU-Net's third label convention: the label values of dataset.json are
 * lists of labels (nested or overlapping regions, BraTS style), the network has one head per foreground region, and the export is
 * "resample the logits back, sigmoid in float32, then paint the regions in order" [UPSTREAM-RECALL: LabelManager.has_regions,
 * convert_probabilities_to_segmentation]:
 *     seg = 0;  for i, c in enumerate(regions_class_order): seg[prob[i] > 0.5] = c
 * One kernel (csrc/kernels_regions.h) does all of it where the aggregation (or the mean of the folds) left the half logits, so ONE uint8
 * plane of the ORIGINAL extent travels to the host.  Everything is as in ts2d_ensemble_predict_tiled_labelmap - engines, images, the
 * descriptors (`maps`: label_u8 [out_h, out_w], not NULL), the fold mean, inf_flag, full_batch and its determinism rule, logits_f16 of
 * an image asked for in the same call, the device scratch (+ n_order bytes in the call's table) - except the decision:
 *   class_order    n_order class values (0 ... 255; they may repeat and may be 0), one per head, n_order == num_classes of the engines.
 *   label_u8       per pixel class_order[i] of the HIGHEST head i whose value exceeds 1.5 * 2^-24 - the predicate of seg_u8 in
 *                  ts2d_engine_predict_tiled: sigmoid(float32 v) > 0.5 - or 0 where no head does.  NaN is not above it, +inf is.  The value
 *                  per head is that of ts2d_tiled_export.logits_f32, bit for bit, except where (out_h, out_w) == (src_h, src_w): the
 *                  widened half itself, as in the label-map entry (so a zero weight on an infinite sample - NaN, not painted - arises
 *                  only where the call resamples).  Restated in numpy as totalsegmentator2d_amd.export.regions_statement.
 * Every argument is validated before any device work and nothing is written on an error: everything the label-map entry refuses, with
 * "regions:" where that says "labelmap:"; a NULL class_order ("regions: the class order is null"); n_order != num_classes ("regions: 3
 * class values for a model of 4 heads").  n_images == 0 returns TS2D_OK and does nothing.
 * (Added under ABI 9: new symbols only, no existing signature or structure changes, so ts2d_abi_version() stays 9.) */
int ts2d_ensemble_predict_tiled_regions(ts2d_engine* const* engines, int n_engines, ts2d_tiled_image* images, const ts2d_tiled_labelmap* maps,
                                        int n_images, int patch_h, int patch_w, int mirror_mask, const uint16_t* gaussian_f16, int full_batch,
                                        const uint8_t* class_order, int n_order);

/* The region kernel of ts2d_ensemble_predict_tiled_regions on half planes the CALLER supplies - the twin of ts2d_labelmap_from_logits,
 * with the same arguments and the same refusals, plus class_order: K class values, one per head (NULL: "regions: the class order is
 * null"; a NULL label_u8: "regions: the output is null").  Same arithmetic, same predicate, same identity rule.
 * (A new symbol of ABI 9: nothing that existed changed.) */
int ts2d_regions_from_logits(int device, const uint16_t* logits_f16, int K, int H, int W, const int32_t rect[4], int out_h, int out_w,
                             const uint8_t* class_order, uint8_t* label_u8);

/* The PROBABILITIES of the export - `save_probabilities=True` of the reference's predictor (ts2d/core/inference/predictor.py:99-111, passed to
 * export_prediction_from_logits, prediction_worker.py:215-221) - from the device, for every label convention, with the decided map of
 * the same pass: upstream resamples the logits back (order 1), applies the inference non-linearity in float32 - the sigmoid per head for a
 * multilabel or region-based model, the softmax over the heads for a label-map model - and reverts the crop on the probabilities: outside
 * the crop box they are 0, except head 0 of a label-map model, which is 1 [UPSTREAM-RECALL: LabelManager.apply_inference_nonlin,
 * revert_cropping_on_probabilities].  One kernel (csrc/kernels_prob.h) does all of it where the aggregation (or the mean of the folds)
 * left the half logits and writes the planes of the PRE-CROP extent, fill included.
 *   engines, images, full_batch, the fold mean, inf_flag: as in ts2d_ensemble_predict_tiled_labelmap.
 *   mode           TS2D_PROB_MULTILABEL (sigmoid; decided_u8 [K, full_h, full_w]: value > 1.5 * 2^-24 per head), TS2D_PROB_LABELMAP
 *                  (softmax; decided_u8 [full_h, full_w]: the label map of ts2d_ensemble_predict_tiled_labelmap) or TS2D_PROB_REGIONS
 *                  (sigmoid; decided_u8 [full_h, full_w]: the painted regions of ts2d_ensemble_predict_tiled_regions, class_order and
 *                  n_order as there; both are ignored in the other modes).
 *   probabilities  n_images descriptors.  (src_y, src_x, src_h, src_w) and (out_h, out_w) mean what they mean in ts2d_tiled_export;
 *                  (full_h, full_w): the extent before cropping; (box_y, box_x): where the [out_h, out_w] rectangle sits in it.
 *                  prob_f32 [K, full_h, full_w], not NULL.  The value v per head is that of ts2d_tiled_export.logits_f32, bit for bit,
 *                  except where (out_h, out_w) == (src_h, src_w): the widened half itself, as in the label-map entry.  Sigmoid:
 *                  1 / (1 + exp(-v)); softmax: exp(v - max) / sum_k exp(v_k - max), the sum in head order; float32 with a correctly
 *                  rounded add and division, exp the float64 function rounded once to float32.  A NaN logit gives a NaN probability; the
 *                  softmax of a pixel with a +inf or NaN head is NaN in every head, a -inf head gives 0 (torch.softmax on the CPU).  Outside
 *                  the box: 0, or 1 in head 0 of TS2D_PROB_LABELMAP.  Not bit for bit the host route's values (another exp): within a few
 *                  float32 units of them (tests/test_gpu_probabilities.py); restated in numpy as export.probabilities_statement.
 *                  decided_u8, or NULL: decided on the LOGIT value with the predicate / comparator of the entries named above, never on
 *                  the probability - byte for byte what those entries write into the box - and 0 outside the box.
 * Every argument is validated before any device work and nothing is written on an error: what the label-map and region entries refuse,
 * in the same words with "probabilities:" where they say "labelmap:" / "regions:"; a rectangle that leaves the full extent; a NULL
 * prob_f32 ("probabilities: the output is null"); an unknown mode; K x full_h x full_w of 2^31 or more; fewer than 1 or more than 256 heads, in
 * every mode and in both entries ("probabilities: 300 heads outside 1 ... 256").  n_images == 0 returns TS2D_OK and does nothing.
 * Device scratch, all held by engines[0]: that of ts2d_ensemble_predict_tiled_labelmap without its label maps plus, summed over the images,
 * K x full_h x full_w x 4 bytes (the probabilities), full_h x full_w bytes (x K multilabel) where decided_u8 is asked for, 24 bytes per output
 * row and column of an image that resamples + 72 per image, n_order bytes.
 * Synchronous: ONE stream synchronise per call, then ts2d_engine_check for every fold; a failure is reported as "fold <f>: <message>".
 * (Added under ABI 9: new symbols only, no existing signature or structure changes, so ts2d_abi_version() stays 9.) */
#define TS2D_PROB_MULTILABEL 0
#define TS2D_PROB_LABELMAP 1
#define TS2D_PROB_REGIONS 2
typedef struct {
    int32_t  src_y, src_x, src_h, src_w;   /* rectangle of the aggregated [K, Hp, Wp] logits that is the prediction (un-padded) */
    int32_t  out_h, out_w;                 /* extent after resampling back */
    int32_t  full_h, full_w;               /* extent before cropping: what is written */
    int32_t  box_y, box_x;                 /* origin of the [out_h, out_w] rectangle in it */
    float*   prob_f32;                     /* host [K, full_h, full_w] */
    uint8_t* decided_u8;                   /* host [full_h, full_w] (multilabel: [K, full_h, full_w]), or NULL */
} ts2d_tiled_probabilities;

int ts2d_ensemble_predict_tiled_probabilities(ts2d_engine* const* engines, int n_engines, ts2d_tiled_image* images,
                                              const ts2d_tiled_probabilities* probabilities, int n_images, int patch_h, int patch_w,
                                              int mirror_mask, const uint16_t* gaussian_f16, int full_batch, int mode,
                                              const uint8_t* class_order, int n_order);

/* ts2d_ensemble_predict_tiled_probabilities for SLICE STACKS - a 3-D volume [C, Z, H, W] that a 2-D model takes slice by slice, whose
 * probabilities are ONE array [K, Z0, full_h, full_w]: the outputs are described per RUN, not per image.  A run is n_slices consecutive
 * images of the call, images[first_image ... first_image + n_slices), that share one geometry - the ten numbers of
 * ts2d_tiled_probabilities and the padded extent (Hp, Wp) - and are consecutive slices of one volume:
 *   prob_f32       host, head 0 of the run's first slice.  Head k of slice s lies at prob_f32 + k * prob_head_stride + s * full_h * full_w
 *                  (elements): with prob_head_stride = Z0 * full_h * full_w the run writes slices [z, z + n_slices) of the caller's
 *                  [K, Z0, full_h, full_w] where prob_f32 points at [0, z].  prob_head_stride >= n_slices * full_h * full_w.  Not NULL.
 *   decided_u8     host or NULL, the same scheme: slice s of the decided map at decided_u8 + s * full_h * full_w, multilabel head k at
 *                  + k * decided_head_stride (>= n_slices * full_h * full_w there; ignored in the other modes: one plane per slice).
 * The runs of a call cover its images exactly once, in order: run 0 begins at image 0, every run where the one before it ended, the last
 * ends at n_images.  A volume that is split over several calls contributes one run to each, at different slice offsets of the same arrays;
 * slices outside every run (those outside the crop box along z) are the caller's to fill.
 * Everything else - engines, images, full_batch and its determinism rule, the fold mean, inf_flag, mode, class_order, the arithmetic, the
 * fill around the box, the identity rule, the decision - is the sibling entry's: a run of one slice with prob_head_stride = full_h * full_w
 * writes that entry's bytes.  On the device the outputs of a run live as [K][n_slices][full_h][full_w], so a run is downloaded in K
 * contiguous copies (+ K, or 1, for the decided map), and the taps of a run that resamples are built and uploaded once, not per slice
 * (csrc/kernels_prob.h: sw_probabilities<ProbStackSeg>, the sibling's lanes with a head stride).
 * Every argument is validated before any device work and nothing is written on an error: everything the sibling entry refuses, in its
 * words with the run named ("run 1: image 3: probabilities: bad output extent 0x5"); runs at a NULL pointer or n_runs < 1 for n_images
 * > 0; a run of fewer than 1 slices; a run that begins behind the end of the one before it ("run 1: probabilities: begins at image 3
 * and leaves a gap behind image 2"), before it ("... begins at image 1 and overlaps the run before it, which ends at image 2"), or leaves the
 * call's images; runs that end before n_images; a NULL prob_f32 ("run 0: probabilities: the output is null"); a head stride below
 * n_slices * full_h * full_w ("run 0: probabilities: head stride 100 is below 3 slices of 6x7"; "decided head stride" likewise); an
 * image of a run whose padded extent differs from the run's first.  n_images == 0 returns TS2D_OK and does nothing.
 * Device scratch, all held by engines[0]: that of the sibling entry, with the outputs summed over the RUNS - K x n_slices x full_h x full_w
 * x 4 bytes, n_slices x full_h x full_w bytes (x K multilabel) where decided_u8 is asked for, each rounded up to 256 elements - 24 bytes per
 * output row and column of a RUN that resamples + 88 per image, n_order bytes.
 * (Added under ABI 9: new symbols only, no existing signature or structure changes, so ts2d_abi_version() stays 9.) */
typedef struct {
    int32_t  src_y, src_x, src_h, src_w;   /* as in ts2d_tiled_probabilities, for every slice of the run */
    int32_t  out_h, out_w;
    int32_t  full_h, full_w;
    int32_t  box_y, box_x;
    int32_t  first_image, n_slices;        /* images[first_image ... first_image + n_slices) */
    float*   prob_f32;                     /* host: head 0 of the run's first slice */
    int64_t  prob_head_stride;             /* elements between the heads of a slice */
    uint8_t* decided_u8;                   /* host: the run's first slice of the decided map, or NULL */
    int64_t  decided_head_stride;          /* multilabel: elements between the heads of a slice; else ignored */
} ts2d_tiled_probabilities_run;

int ts2d_ensemble_predict_tiled_probabilities_stack(ts2d_engine* const* engines, int n_engines, ts2d_tiled_image* images, int n_images,
                                                    const ts2d_tiled_probabilities_run* runs, int n_runs, int patch_h, int patch_w,
                                                    int mirror_mask, const uint16_t* gaussian_f16, int full_batch, int mode,
                                                    const uint8_t* class_order, int n_order);

/* The kernel of ts2d_ensemble_predict_tiled_probabilities on half planes the CALLER supplies - the twin of ts2d_labelmap_from_logits and
 * ts2d_regions_from_logits, with their arguments and their refusals ("probabilities:" in the place of "regions:"), plus the full extent, the
 * box origin and the mode: logits_f16 host [K, H, W] half bits, rect = {src_y, src_x, src_h, src_w}, prob_f32 host [K, full_h, full_w] (not
 * NULL), decided_u8 host as in the descriptor above (or NULL), class_order K class values (TS2D_PROB_REGIONS only; NULL there: "probabilities:
 * the class order is null").  Same arithmetic, same fill, same identity rule.  Host pointers in and out, synchronous, scratch of the call's
 * own, freed on every path.  (A new symbol of ABI 9: nothing that existed changed.) */
int ts2d_probabilities_from_logits(int device, const uint16_t* logits_f16, int K, int H, int W, const int32_t rect[4], int out_h, int out_w,
                                   int full_h, int full_w, int box_y, int box_x, int mode, const uint8_t* class_order, float* prob_f32,
                                   uint8_t* decided_u8);

/* Blend order of ts2d_engine_predict_tiled (upstream `prediction *= gaussian; predicted_logits[sl] += prediction` with
 * float16 `predicted_logits`; reached from ts2d/core/inference/prediction_worker.py:209):
 *   TS2D_TILE_F32 (default) the reference's CPU path (nnu.py:161-163: device=cpu when torch.cuda.is_available() is false - no autocast): the tile prediction is
 *       fp32, the product is fp32 x float(half gaussian) in fp32, the sum is a float add with ONE rounding into the half buffer;
 *   TS2D_TILE_F16 the reference's CUDA path (fp16 autocast): the tile is half, the product and the sum each round to half. */
#define TS2D_TILE_F32 0
#define TS2D_TILE_F16 1
int ts2d_engine_set_tile_dtype(ts2d_engine* e, int mode);

/* Activation memory (ABI 5).  By default the activations of a forward share one arena by LIVENESS: a tensor's bytes are reused once
 * its last reader has run (the encoder skips live until their decoder block) - ~110 instead of ~340 MB per 2x512x512 slice of the
 * canonical net.  enable != 0 gives every tensor its own buffer again: needed before a forward whose intermediate tensors are to be
 * read back with ts2d_engine_debug_tensor (a reused tensor reports TS2D_ERR_STATE there).  ts2d_engine_check needs no switch: when a
 * synchronous call flagged inf / NaN it re-runs that input once with private buffers to name the first bad layer.  Takes effect at
 * the next ts2d_engine_reserve / forward.  (The reference keeps every intermediate alive only as long as torch's autograd-free
 * forward does: ts2d/core/inference/prediction_worker.py:209.) */
int ts2d_engine_set_keep_activations(ts2d_engine* e, int enable);

/* 1 if the last ts2d_engine_predict_tiled / ts2d_engine_predict_tiled_batch / ts2d_engine_predict_tiled_export call (the OR over its images; after
 * ts2d_ensemble_predict_tiled_export: this fold's own) produced an infinite
 * aggregated float16 logit - upstream's
 * "Encountered inf in predicted array" check of predict_sliding_window_return_logits (reached from
 * ts2d/core/inference/prediction_worker.py:209), evaluated on the device instead of a host pass over the array. */
int ts2d_engine_tiled_inf_flag(const ts2d_engine* e);

/* Coronal maximum + mean projection of a volume on the device (reference ts2d/tool.py:152-160 -> ts2d/core/util/image.py:46-101).
 *   volume     host pointer to the ORIGINAL contiguous buffer of `n_elems` elements of type `dtype`
 *              (0 = int16, 1 = uint8, 2 = float32, 3 = uint16, 4 = int32)
 *   nz, ny, nx extents of the REORIENTED view [z][y][x] (DICOMOrient 'RAI'); sz, sy, sx its signed ELEMENT strides and `base` the
 *              element offset of view[0][0][0] in the buffer (so axis flips / permutations need no host copy)
 *   out_max, out_mean  host [nz][nx] float32: projections along y.  The mean is real-valued for every input type: the sum in index
 *              order (exact for integer volumes) divided in double, rounded once to float - ITK's MeanProjectionImageFilter followed by
 *              the reference's Cast to Float32 (ts2d/tool.py:182-185); the reference's pre-projected sample assets pin it
 *              (oracle/input_oracle.py).  Synchronous.
 * TS2D_ERR_INVALID, by name: nz * nx above 2^31 - 1 output pixels (one lane per pixel: a launch past 2^32 lanes is not refused by the runtime
 * but cut short), and a view that leaves the buffer. */
int ts2d_project_coronal(int device, const void* volume, size_t n_elems, int dtype, int nz, int ny, int nx, long long sz,
                         long long sy, long long sx, long long base, float* out_max, float* out_mean);

/* The same projection followed, on the device, by the per-channel z-score nnU-Net applies to the 2-channel (max, mean) image
 * before the network (ZScoreNormalization without mask: (x - mean) / max(std, 1e-8), population std; reference flow
 * ts2d/tool.py:152-160,182-185 -> DefaultPreprocessor.run_case, ts2d/core/inference/prediction_worker.py:194-199): mean and std in
 * float64, two passes, fixed summation order.  out_norm = [2][nz][nx] float (the network input when nz, nx need no padding),
 * out_stats = {mean_max, std_max, mean_mean, std_mean} (may be NULL), out_box = {first, last non-zero row, first, last non-zero
 * column} over both channels (may be NULL): nnU-Net crops to that box BEFORE normalising, so the caller uses out_norm only when
 * the box is the whole image.  (ABI 4) */
int ts2d_project_coronal_zscore(int device, const void* volume, size_t n_elems, int dtype, int nz, int ny, int nx, long long sz,
                                long long sy, long long sx, long long base, float* out_max, float* out_mean, float* out_norm,
                                double* out_stats, int32_t* out_box);

/* Every projection mode of the reference's project() along the coronal axis (ts2d/core/util/image.py:46-101; a TS2D sub-model's channel NAMES are
 * projection modes, ts2d/tool.py:156-158), on the device, with the addressing of ts2d_project_coronal (volume ... base as there).
 *   modes        [n_modes] TS2D_PROJECT_* codes, 1 <= n_modes <= TS2D_PROJECT_MAX_MODES; a code may occur more than once
 *   slice_index  [n_modes]: for a TS2D_PROJECT_SLICE entry the index along y, in [0, ny); ignored for the other codes (never null)
 *   out_planes   host [n_modes][nz][nx] float32, plane m in mode modes[m].  What a plane holds is stated by totalsegmentator2d_amd.image.project,
 *                followed by its cast to float32:
 *                  MAX, MEAN   bit for bit the planes of ts2d_project_coronal
 *                  MIN         the minimum
 *                  MEDIAN      the value at index ny / 2 of the sorted ray (the upper median: no averaging), picked in the input type
 *                  STD         sqrt(sum((v - mean)^2) / (ny - 1)): float64, two passes in index order, multiply and add rounded separately,
 *                              correctly rounded divide and square root, one rounding to float32; needs ny >= 2
 *                  FIRST       the first sample != 0 in index order, the sample at index 0 when there is none
 *                  SLICE       the sample at slice_index[m]
 *   out_norm     host [n_modes][nz][nx] float32, or NULL: every plane z-scored by itself, as behind ts2d_project_coronal_zscore
 *   out_stats    host [n_modes][2] float64 {mean, std} of each plane, or NULL (needs out_norm)
 *   out_box      host [n_modes][4] {first, last non-zero row, first, last non-zero column} of EACH plane ({nz, -1, nx, -1} for a plane of
 *                zeros), or NULL (needs out_norm): the caller forms the union over the planes that make up one network input
 *   status       a bit word, 0 when the outputs are the result.  TS2D_PROJECT_NONFINITE: a float32 volume holds a NaN or an infinity;
 *                TS2D_PROJECT_RAY_TOO_LONG: ny > TS2D_PROJECT_RAY_CAP (nothing was launched).  With a bit set the call still returns TS2D_OK,
 *                the outputs are unspecified and the caller must not use them: it takes the host route.
 * Every argument is checked before any device work and refused by name with TS2D_ERR_INVALID: a null pointer, an unknown mode, a slice index
 * outside [0, ny), n_modes outside its range, an extent below 1, a view that leaves the buffer.  Nothing is written then.
 * Host pointers in and out; synchronous; the call owns its device scratch and frees it on every path.  (ABI 9, optional symbol) */
#define TS2D_PROJECT_MAX 0
#define TS2D_PROJECT_MIN 1
#define TS2D_PROJECT_MEAN 2
#define TS2D_PROJECT_MEDIAN 3
#define TS2D_PROJECT_STD 4
#define TS2D_PROJECT_FIRST 5
#define TS2D_PROJECT_SLICE 6
#define TS2D_PROJECT_MAX_MODES 16
#define TS2D_PROJECT_RAY_CAP 8192
#define TS2D_PROJECT_NONFINITE 1
#define TS2D_PROJECT_RAY_TOO_LONG 2
int ts2d_project_coronal_modes(int device, const void* volume, size_t n_elems, int dtype, int nz, int ny, int nx, long long sz, long long sy,
                               long long sx, long long base, const int32_t* modes, const int32_t* slice_index, int n_modes, float* out_planes,
                               float* out_norm, double* out_stats, int32_t* out_box, int32_t* status);

/* The synthetic radiograph of a CT volume, and the projection of a 3-D label volume along the radiograph's rays, on the device.  The statements
 * are totalsegmentator2d_amd/xray.py (xr_tables, synthetic_xr_statement, project_labels_xr_statement; numpy); the two entries reproduce them bit
 * for bit and byte for byte.  Both take the strided view of ts2d_project_coronal_modes (volume, n_elems, dtype, extents, element strides and base
 * as there) and then the geometry as plain numbers:
 *   spacing_x, spacing_y, spacing_z   the spacings of the view's x, y and z in mm
 *   source_detector_mm, source_center_mm   sdd and sod: the source's distance to the detector and to the centre of the volume
 *   view_pa      0: 'ap', the source in front of the patient (at y below the volume); 1: 'pa', behind it.  Rows and columns keep their directions.
 *   parallel     1: parallel rays (then nu = nx, nv = nz, du = spacing_x, dv = spacing_z are required); 0: a cone beam
 *   du, dv, nu, nv   the detector's pixel spacings in mm and its size; pixel (k, i) of [nv][nu] sits at Cx + (i - (nu - 1) / 2) du,
 *                Cz + (k - (nv - 1) / 2) dv, C the centre ((nx - 1) spacing_x / 2, (ny - 1) spacing_y / 2, (nz - 1) spacing_z / 2)
 * Rays run along y; every ray has one sample per plane y = j, taken in index order for both views.
 *
 * ts2d_project_xr: the five sample types.  The density of a sample v is max((double(v) - air) * (1 / (water - air)), 0), then min(., density_max)
 * where clip is 1; each sample of a ray is the bilinear interpolation of the plane's density (+0.0 outside the plane), in float64, every
 * operation rounded on its own.
 *   out_sum_f64  host [nv][nu] float64, the sums of the rays, or NULL
 *   out_xr_f32   host [nv][nu] float32 = float32(sum * step), step the ray's length between two planes in mm: the line integral of the density
 *                in millimetres of water (no exponential is applied); or NULL.  Not both NULL.
 *   status       0, or TS2D_XR_NONFINITE: a float32 volume holds a NaN or an infinity; the outputs are not written, and the caller raises.
 *                The call returns TS2D_OK.
 *
 * ts2d_project_labels_xr: integer sample types (dtype 2, float, is refused).  planes_u8 [num][nv][nu]: plane k is 1 where any sample of the ray
 * - the NEAREST voxel floor(x + 0.5), floor(z + 0.5); a sample outside the volume is skipped - equals k + 1, else 0; num 1 ... 255.
 *   status       0, or TS2D_LABELS_RANGE: a sample of the volume (met by a ray or not) lies outside 0 ... num; planes_u8 is not written, and
 *                the caller raises.  The call returns TS2D_OK.
 *
 * Every argument is checked before any device work and refused by name with TS2D_ERR_INVALID, the outputs untouched: a null pointer, an unknown
 * dtype, an extent below 1, a view that leaves the buffer, nz * nx above 2^31 - 1; a spacing or distance that is not finite and positive;
 * source_center_mm <= (ny - 1) spacing_y / 2 (the source inside the slab of plane centres); source_detector_mm - source_center_mm below that half
 * depth (the detector inside the slab); nu or nv below 1, nu * nv above 2^31 - 1 (num * nu * nv for the planes); view_pa, parallel or clip other
 * than 0 or 1; water == air, either not finite; a density_max that is not a number >= 0; num outside 1 ... 255.
 * Host pointers in and out; synchronous; the call owns its device scratch and frees it on every path.  (ABI 9, optional symbols) */
#define TS2D_XR_NONFINITE 1
int ts2d_project_xr(int device, const void* volume, size_t n_elems, int dtype, int nz, int ny, int nx, long long sz, long long sy, long long sx,
                    long long base, double spacing_x, double spacing_y, double spacing_z, double source_detector_mm, double source_center_mm,
                    int view_pa, int parallel, double du, double dv, int nu, int nv, double air, double water, int clip, double density_max,
                    double* out_sum_f64, float* out_xr_f32, int32_t* status);
int ts2d_project_labels_xr(int device, const void* volume, size_t n_elems, int dtype, int nz, int ny, int nx, long long sz, long long sy,
                           long long sx, long long base, double spacing_x, double spacing_y, double spacing_z, double source_detector_mm,
                           double source_center_mm, int view_pa, int parallel, double du, double dv, int nu, int nv, int num, uint8_t* planes_u8,
                           int32_t* status);

/* nnU-Net's input resample for the 2-D configurations on the device: every plane of src [n_planes][in_h][in_w] float32 resampled to
 * dst [n_planes][out_h][out_w] float32 as skimage.transform.resize(plane, (out_h, out_w), order=3, mode='edge', anti_aliasing=False,
 * clip=True) does it (reference flow DefaultPreprocessor.run_case, ts2d/core/inference/prediction_worker.py:194-199, for a case whose
 * spacing is not the plan's).  Host pointers in and out, synchronous, scratch of the call's own, freed on every path.
 * Arithmetic contract = preprocess.resize_cubic_f64, bit for bit, which is bit for bit scipy's zoom(order=3, mode='nearest',
 * grid_mode=True) and the clip that follows it: the plane padded by 12 edge samples, widened to float64, cubic B-spline prefilter along
 * axis 0 and then along axis 1 exactly as scipy's line filter runs it (pole = the float64 nearest to sqrt(3) - 2, the boundary sum with
 * its running products of the pole and its accumulator read back in the last term, sequential recursions), 16 taps per output pixel in
 * row-major order, each (c * wy) * wx, summed left to right from 0, every product and sum rounded to float64 (no FMA), ONE rounding
 * to float32, then x < lo ? lo : x and x > hi ? hi : x.  Taps and line constants are computed on the host in float64.
 *   lo_hi      [n_planes][2]: the float32 minimum and maximum of each source plane (the caller has them from numpy).  They must be
 *              finite and ordered: a plane with a non-finite sample is outside the contract (its minimum or maximum says so).
 * TS2D_ERR_INVALID, by name, before any device work: null pointers, n_planes < 1, an extent below 2 or above 8192, more than 2^28
 * padded or output samples in one call, a zoom whose taps would leave the padded plane, non-finite or inverted lo_hi.
 * (A new symbol of ABI 9: nothing that existed changed.) */
int ts2d_resample_cubic(int device, const float* src, int n_planes, int in_h, int in_w, int out_h, int out_w, const float* lo_hi,
                        float* dst);

/* nnU-Net's preprocessing of an input that is 2-D when it arrives - an X-ray image, a pre-projected multi-channel image - on planes that
 * stay on the device: crop_to_nonzero, the normalisation of each channel, the resample to the plan spacing (reference flow
 * DefaultPreprocessor.run_case, ts2d/core/inference/prediction_worker.py:194-199).  The planes are uploaded once and downloaded once.
 * Every entry validates its arguments before any device work and names itself in ts2d_last_error, frees its scratch on every path and
 * is synchronous.  (New symbols of ABI 9: nothing that existed changed.) */
typedef struct ts2d_planes ts2d_planes;

/* Upload src [n_planes][h][w] float32 (the channels of one case, prediction_worker.py:194-199: the array run_case reads) to HIP device
 * `device`.  TS2D_ERR_INVALID: null pointers, n_planes outside 1 ... 65535, an extent outside 1 ... 8192, more than 2^28 samples. */
int ts2d_planes_create(int device, const float* src, int n_planes, int h, int w, ts2d_planes** out);

/* crop_to_nonzero and the per-plane z-score of run_case (prediction_worker.py:194-199), in place on the handle:
 *   box    {first row, one past the last row, first column, one past the last column} of the pixels that are non-zero in ANY plane
 *          (`!= 0` as numpy has it: a NaN is not zero; planes of zeros keep their whole extent); the planes are compacted to it, so the
 *          handle's extent becomes (box[1] - box[0]) x (box[3] - box[2]).
 *   stats  [n_planes][2]: float32 mean and standard deviation of each cropped plane.
 * Arithmetic contract = preprocess.zscore_f32_statement, bit for bit, which is bit for bit numpy's img.mean(), img.std(), img -= mean,
 * img /= max(std, 1e-8) on the C-contiguous float32 plane: the float32 sum in chunks of 8192 elements added in index order from +0, each
 * chunk summed pairwise (runs of at most 128 elements in eight strided accumulators combined ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)), then
 * the last len % 8 elements; a longer run split at n/2 - (n/2) % 8), sum / n in float64 rounded once to float32, the second sum over
 * fl32(fl32(x - mean)^2), the float32 square root, and per element fl32(fl32(x - mean) / max(std, 1e-8)) with a correctly rounded
 * division.  No fused multiply-add, no atomics on floats: two calls give the same bits.  The float32 minimum and maximum of each
 * normalised plane stay on the handle: they are the clip bounds of ts2d_planes_resample_cubic.
 *   nonfinite  set to 1 when a mean, a variance or a normalised sample is not finite (a non-finite sample, or float32 sums that
 *          overflow): the planes are then cropped but NOT a normalisation the caller may use; it drops the handle and runs numpy. */
int ts2d_planes_crop_zscore(ts2d_planes* p, int32_t box[4], float* stats, int* nonfinite);

/* crop_to_nonzero and ANY of nnU-Net's normalisation schemes per plane (run_case, prediction_worker.py:194-199; nnunetv2's
 * default_normalization_schemes), in place on the handle - what ts2d_planes_crop_zscore does for the plain z-score, for the cases it does
 * not take: an ordinary CT model, a plan with use_mask_for_norm, a natural-image model, a channel that is not normalised.
 *   schemes   [n_planes]: TS2D_NORM_* of each plane.
 *   params    [n_planes][4] float32, read for TS2D_NORM_CT only: {mean, divisor = float32(max(std, 1e-8)), lower bound, upper bound}, each as
 *             numpy converts the plan's number for a float32 array.  They must be finite.
 *   use_mask  [n_planes]: non-zero = a TS2D_NORM_ZSCORE plane takes its statistics over, and is normalised only inside, the non-zero mask
 *             of the case: the pixels of the box that are non-zero in ANY plane (nnU-Net's `seg >= 0` for a single slice; the hole
 *             filling of create_nonzero_mask changes nothing there).  Ignored for the other schemes, as nnU-Net ignores it.
 *   box       as ts2d_planes_crop_zscore returns it; the planes are compacted to it.
 *   stats     [n_planes][2]: (mean, std) of a z-score plane - of its masked samples with use_mask - and the (subtrahend, divisor) actually
 *             used otherwise: CT (mean, divisor), Rescale (minimum, divisor), RGB (0, 255), none (0, 1).
 * Arithmetic contract = the statements of preprocess.py, bit for bit, each bit for bit numpy's (preprocess.normalize_channel):
 *   TS2D_NORM_ZSCORE     zscore_f32_statement; with use_mask masked_zscore_f32_statement: the sums of ts2d_planes_crop_zscore over
 *                        plane[mask], a compact copy in row-major order (n_m samples: chunks of 8192, the pairwise tree of the last
 *                        n_m % 8192), fl32(fl32(x - mean) / max(std, 1e-8)) inside the mask, the sample itself outside.
 *   TS2D_NORM_CT         ct_f32_statement: x < lo ? lo : x, then x > hi ? hi : x (a sample equal to a bound keeps its sign of zero, a NaN
 *                        stays NaN), then fl32(fl32(x - mean) / divisor).
 *   TS2D_NORM_RESCALE01  rescale01_f32_statement: fl32(fl32(x - min) / d) with d = fl32(max - min), or float32(1e-8) if that is larger.
 *   TS2D_NORM_RGB01      rgb01_f32_statement: fl32(x / 255).
 *   TS2D_NORM_NONE       the sample itself.
 * No fused multiply-add, correctly rounded divisions, no atomics on floats, a compaction by integer counts: two calls give the same bits.
 * The float32 minimum and maximum of each resulting plane stay on the handle: the clip bounds of ts2d_planes_resample_cubic.
 *   status    0, or TS2D_PLANES_* bits: the planes are then cropped but NOT a result the caller may use; it drops the handle and runs numpy,
 *             which computes (or raises) what numpy computes of such a case.
 * TS2D_ERR_INVALID, by name, before any device work: null pointers, a scheme outside TS2D_NORM_*, a non-finite CT parameter. */
#define TS2D_NORM_ZSCORE 0      /* ZScoreNormalization */
#define TS2D_NORM_CT 1          /* CTNormalization */
#define TS2D_NORM_RESCALE01 2   /* RescaleTo01Normalization */
#define TS2D_NORM_RGB01 3       /* RGBTo01Normalization */
#define TS2D_NORM_NONE 4        /* NoNormalization */
#define TS2D_PLANES_NONFINITE 1     /* a statistic, a Rescale bound or a resulting sample is not finite */
#define TS2D_PLANES_RGB_RANGE 2     /* a TS2D_NORM_RGB01 plane holds a sample outside [0, 255]: upstream raises */
#define TS2D_PLANES_EMPTY_MASK 4    /* use_mask on an image of zeros: there is nothing to take a mean of */
#define TS2D_PLANES_ZERO_SIGN 8     /* a TS2D_NORM_RESCALE01 plane whose minimum is -0.0: if it holds +0.0 too, numpy's min() may return
                                     * either, and the sign of every resulting zero hangs on it */
#define TS2D_PLANES_FILL_ROUNDS 16  /* ts2d_planes_crop_normalize_stack_masked only: the 3-D hole filling of the mask was still adding voxels after
                                     * its 64 rounds (a corridor that winds through the volume): the fill is left to the host */
int ts2d_planes_crop_normalize(ts2d_planes* p, const int32_t* schemes, const float* params, const uint8_t* use_mask, int32_t box[4],
                               float* stats, int* status);

/* A STACK on the handle: a 3-D volume that a 2-D plan takes slice by slice (run_case, prediction_worker.py:194-199, fed a volume - what
 * `nnUNetv2_predict -c 2d` does with a CT).  Upload src [channels][slices][h][w] float32; the handle then holds channels x slices planes, and
 * ts2d_planes_resample_cubic, ts2d_planes_extent, ts2d_planes_download and ts2d_planes_destroy treat every slice as a plane.  The two crop
 * entries above refuse such a handle (TS2D_ERR_INVALID); ts2d_planes_crop_normalize_stack and ts2d_planes_crop_normalize_stack_masked are its own.
 * TS2D_ERR_INVALID, by name, before any device work: null pointers, channels or slices below 1, more than 65535 planes, an extent outside
 * 1 ... 8192, more than 2^28 samples.  (A new symbol of ABI 9: nothing that existed changed.) */
int ts2d_planes_create_stack(int device, const float* src, int channels, int slices, int h, int w, ts2d_planes** out);

/* crop_to_nonzero and the normalisation of a stack (run_case on [C, Z, H, W] with Z > 1), in place on the handle:
 *   box       {first slice, one past the last slice, first row, one past the last row, first column, one past the last column} of the voxels
 *             that are non-zero in ANY channel (`!= 0` as numpy has it: a NaN is not zero, -0.0 is; a volume of zeros keeps its whole
 *             extent) = preprocess.crop_box3_statement = crop_to_nonzero's box: the holes nnU-Net fills in the mask of a volume lie inside
 *             the box of the unfilled one.  The volume is compacted to it, dense [channels][Z'][h'][w']: the handle then holds channels x Z'
 *             planes of h' x w'.
 *   schemes, params   per CHANNEL, as in ts2d_planes_crop_normalize.
 *   use_mask  [channels]: must be zero for every TS2D_NORM_ZSCORE channel - the mask of a volume is hole-filled in 3-D, which
 *             ts2d_planes_crop_normalize_stack_masked does; ignored for the other schemes, as nnU-Net ignores it.
 *   stats     [channels][2], as in ts2d_planes_crop_normalize.
 * Arithmetic contract = the statements of ts2d_planes_crop_normalize applied to each channel's WHOLE cropped volume, flattened in C order, which
 * is what numpy reduces (normalize_channel copies the cropped view into a dense array): the z-score sums run over N = Z' h' w' samples, their
 * chunks of 8192 crossing the slice boundaries, mean and variance fl32(f64(sum) / N) (numpy's, beyond 2^24 samples too); Rescale takes the
 * minimum and maximum of the whole channel.  Each sample is then normalised by its CHANNEL's parameters.  The clip bounds kept for
 * ts2d_planes_resample_cubic are the float32 minimum and maximum of each resulting SLICE: nnU-Net's resize clips every 2-D slice to its own.
 *   status    0, or TS2D_PLANES_NONFINITE, TS2D_PLANES_RGB_RANGE, TS2D_PLANES_ZERO_SIGN with their meaning above: the volume is then cropped
 *             but NOT a result the caller may use; it drops the handle and runs numpy.
 * TS2D_ERR_INVALID, by name, before any device work and with nothing written: null pointers, a scheme outside TS2D_NORM_*, a masked z-score
 * channel, a non-finite CT parameter.
 * Device scratch of the call's own, freed on every path: 16 bytes per slice, 32 per channel, and per channel 4 bytes per 8192 samples of the
 * uncropped volume + 640 (the chunk and leaf sums); the compaction holds the cropped copy beside the volume until it has been made.
 * (A new symbol of ABI 9: nothing that existed changed.) */
int ts2d_planes_crop_normalize_stack(ts2d_planes* p, const int32_t* schemes, const float* params, const uint8_t* use_mask, int32_t box[6],
                                     float* stats, int* status);

/* ts2d_planes_crop_normalize_stack that TAKES a masked z-score channel (use_mask_for_norm of an MR plan): the same arguments, box, limits and
 * messages under its own name, and for the channels that are not masked the same bytes.
 *   use_mask  [channels]: non-zero = a TS2D_NORM_ZSCORE channel takes its statistics over, and is normalised only inside, the non-zero mask of
 *             the cropped volume with its holes filled in 3-D: "non-zero in ANY channel" (`!= 0`: a NaN counts, -0.0 does not) plus every zero
 *             voxel that is not 6-connected through zero voxels to a face of the box = scipy.ndimage.binary_fill_holes of the mask of the whole
 *             array (default cross structure), cropped - what nnU-Net's create_nonzero_mask computes of a volume; every voxel outside the box is
 *             zero and reaches the array's border in a straight line, so the faces of the box stand in for that border.  Ignored for the other
 *             schemes.  The fill runs only when a channel is masked.
 *   stats     (mean, std) of a masked channel are those of its masked samples.
 * Arithmetic contract of a masked channel = preprocess.masked_zscore_stack_statement: masked_zscore_f32_statement over the flattened channel - the
 * masked samples in index order are ONE run of n_m elements, so numpy's chunks of 8192 cross the slices as `img[mask]` does; inside the mask
 * fl32(fl32(x - mean) / max(std, 1e-8)), outside it the sample itself.  The mask itself = preprocess.fill_holes_sweeps_statement: rounds of six
 * directional sweeps (z up, z down, y up, y down, x up, x down) from the background voxels on the faces until a round adds nothing.
 *   status    the bits of ts2d_planes_crop_normalize_stack, and
 *             TS2D_PLANES_EMPTY_MASK   a masked channel in a volume of zeros;
 *             TS2D_PLANES_FILL_ROUNDS  64 rounds each still added a voxel: nothing is normalised, no retry; the caller runs numpy.
 * Device scratch beside that of ts2d_planes_crop_normalize_stack, only with a masked channel and freed on every path: two bit planes of the
 * cropped volume (a quarter of a byte per voxel), one byte per voxel for the mask, 4 bytes per 2048 voxels twice, and the masked samples of
 * every channel (4 bytes each).  (A new symbol of ABI 9: nothing that existed changed.) */
int ts2d_planes_crop_normalize_stack_masked(ts2d_planes* p, const int32_t* schemes, const float* params, const uint8_t* use_mask, int32_t box[6],
                                            float* stats, int* status);

/* The order-3 resample of run_case (prediction_worker.py:194-199, a case whose spacing is not the plan's) of every plane of the handle to
 * out_h x out_w, clipped to the bounds ts2d_planes_crop_zscore left: the arithmetic, the limits and the messages of ts2d_resample_cubic.
 * The handle's extent becomes out_h x out_w and its clip bounds are used up (TS2D_ERR_STATE without them). */
int ts2d_planes_resample_cubic(ts2d_planes* p, int out_h, int out_w);

/* The current extent of the planes (prediction_worker.py:194-199: the shape of the array run_case returns). */
int ts2d_planes_extent(const ts2d_planes* p, int* h, int* w);

/* Copy the planes [n_planes][h][w] (current extent) back to the host (prediction_worker.py:194-199: the array run_case returns). */
int ts2d_planes_download(const ts2d_planes* p, float* dst);

/* Free the handle and its device memory (NULL is fine).  Reference: the preprocessed array going out of scope (prediction_worker.py:194-199). */
int ts2d_planes_destroy(ts2d_planes* p);

/* nnU-Net's postprocessing of a decided label map, the plan nnUNetv2_find_best_configuration stores beside a model: the steps of
 * remove_all_but_largest_component_from_segmentation, one after the other on the device (kernels_post_cc.h).  The reference has no counterpart
 * (its models are multilabel and carry no such plan); the contract is postprocess.keep_largest_components_statement, byte for byte.
 *   seg       host uint8 [Z][H][W], changed IN PLACE; a 2-D case is Z = 1.  One upload, every step on the device, one download.
 *   steps     [n_steps], applied in order, each to the result of the one before.  A step: `member` - 1 at every label value it names, label or
 *             region alike (the union) - and `background`.  mask = member[seg]; its components under FULL connectivity (26 neighbours, 8 at
 *             Z = 1) are sized; every mask voxel of a component smaller than the largest becomes `background`; components that tie for the
 *             largest all stay; an empty mask changes nothing.
 *   stats     NULL, or int64 [n_steps][4]: mask voxels, components, largest size, voxels removed.
 *   status    0, or TS2D_CC_GIVE_UP: a bounded loop of the labelling reached its hard cap (32768 steps of one find chain, 1024 lost races of one
 *             union - neither has been seen).  The call returns TS2D_OK with seg and stats as the caller passed them; no retry, the caller takes the
 *             host route.
 * The result does not depend on the order in which the lanes arrive: the partition, the integer sizes and their maximum are unique and ties are kept.
 * TS2D_ERR_INVALID, by name, before any device work: null seg or status, null steps with n_steps > 0, a non-positive extent, more than 2^31 - 1
 * voxels (the indices are int32), n_steps < 0.  n_steps = 0 does nothing.  On any error the host buffer is untouched.
 * Device scratch of the call's own, freed on every path: 9 1/8 bytes per voxel (the map, its bit words, parent and count), 257 bytes and four
 * counters per step.  (A new symbol of ABI 9: nothing that existed changed.) */
typedef struct { uint8_t member[256]; uint8_t background; } ts2d_cc_step;
#define TS2D_CC_GIVE_UP 1   /* a bounded loop reached its cap: seg is unchanged, the caller takes the host route */
int ts2d_keep_largest_components(int device, uint8_t* seg /* host [Z][H][W], in place */, int Z, int H, int W,
                                 const ts2d_cc_step* steps, int n_steps, int64_t* stats /* [n_steps][4] or NULL */, int* status);

/* PNG visuals of a result on the device: the reference's create_visual (ts2d/core/util/image.py:383-453), which Result.save calls for every file
 * it writes (ts2d/tool.py:272-311).  The statement is totalsegmentator2d_amd/visual.py (numpy float64); both entries reproduce it byte for byte.
 * Host pointers in and out, synchronous, scratch of the call's own, freed on every path.  Geometry of both: a plane of H x W samples at spacing
 * spacing_h x spacing_w is resampled to the smaller spacing m; per axis of N samples at spacing s the output has M = int(0.5 + N*s/m) samples,
 * output index j reads the continuous source index x_j = (N/2) + (j - M/2) * (m/s) (float64, in that order) and is inside iff
 * -0.5 <= x_j < N - 0.5; outside pixels are 0.  out_h x out_w must be those extents (the caller sizes its buffer by them).  A plane that needs no
 * resample is handed over with spacing 1 x 1.
 *
 * ts2d_visual_labels: planes [K][H][W] uint8; K = 1 is a label map, K > 1 is flattened to 1 + the index of the LAST non-zero plane (0: none).
 * Nearest sample floor(x + 0.5); rgb [out_h][out_w][3] = palette[v % n_palette] for v > 0, black for 0 and outside.  palette [n_palette][3].
 *
 * ts2d_visual_grey: one plane of `dtype` (the codes of ts2d_project_coronal: 0 int16, 1 uint8, 2 float32, 3 uint16, 4 int32).  cubic = 0: the
 * nearest sample; cubic = 1 (not for uint8; extents of at least 2): the order-3 B-spline with mirror boundaries in float64 - prefilter along both
 * axes, 16 taps - cast back to the pixel type (float32: one rounding; an integer type: clamped, truncated toward zero).  The window maps lo ... hi
 * to 0 ... 255 (below lo 0, above hi 255, hi == lo: an all-zero plane); auto_lo / auto_hi != 0 take the minimum / maximum of the RESAMPLED plane
 * in place of lo / hi.  grey [out_h][out_w]; window_used[2] receives lo and hi as used.
 *   status    0, or TS2D_VISUAL_NONFINITE: a float32 sample is NaN or infinite; grey and window_used are not written, the caller takes the host
 *             route.  The call returns TS2D_OK.
 * TS2D_ERR_INVALID, by name, before any device work: a null pointer, K outside 1 ... 255, n_palette outside 1 ... 256, an unknown dtype, cubic
 * outside {0, 1} or with uint8 or with an extent below 2, a non-finite window bound that is not automatic, an extent outside 1 ... 8192, a spacing
 * that is not finite and positive, output extents above 32768 per axis or 2^28 pixels, out_h x out_w that are not the resample's.
 * (New symbols of ABI 9: nothing that existed changed.) */
#define TS2D_VISUAL_NONFINITE 1
int ts2d_visual_labels(int device, const uint8_t* planes, int K, int H, int W, double spacing_h, double spacing_w, const uint8_t* palette,
                       int n_palette, int out_h, int out_w, uint8_t* rgb);
int ts2d_visual_grey(int device, const void* plane, int dtype, int H, int W, double spacing_h, double spacing_w, int cubic, double lo, double hi,
                     int auto_lo, int auto_hi, int out_h, int out_w, uint8_t* grey, double* window_used, int* status);

/* Per-label statistics of a segmentation on the device: is a structure there, how large is it, where is it, how bright is the image under it
 * (the reference's get_labels_voxels / get_voxel_mm, ts2d/core/util/meta.py:64-80, and beyond them box, centroid sums and intensity moments).
 * The statement is totalsegmentator2d_amd/statistics.py (label_statistics_statement, numpy); the entry reproduces it bit for bit, the float64
 * sums included.  Host pointers in and out, synchronous: ONE upload, every label on the device, ONE download; scratch of the call's own, freed
 * on every path.  A volume is Z x H x W samples (a 2-D image: Z = 1), addressed as R = Z * H rows of W samples.
 *   seg, kind  TS2D_STATS_PLANES: uint8 [K][Z][H][W], label k is plane k > 0.  TS2D_STATS_LABELMAP: ONE uint8 [Z][H][W] and values[K] (each
 *              1 ... 255), label k is seg == values[k].  values may be NULL for planes.
 *   intensities  float32 [C][Z][H][W]; NULL with C = 0: counts, boxes and index sums only (out_f64 may then be NULL too).
 *   max_scratch_bytes  bound of the row partials (20 + 16 C bytes per label and row); the labels are processed in chunks that stay below it;
 *              0: 256 MiB.  The result does not depend on the chunking.
 *   out_int    int64 [K][TS2D_STATS_INTS]: count; the sum of the z, y and x indices of the label's samples; min z, max z, min y, max y,
 *              min x, max x (inclusive).  An empty label: count 0, sums 0, minima Z, H, W, maxima -1.
 *   out_f64    float64 [K][C][TS2D_STATS_F64S]: sum, ssq, mean, std, min, max.  sum: the float64 sum of the samples under the label; mean =
 *              sum / count; ssq: the sum of (x - mean)^2, difference, product and sum each rounded on its own; std = sqrt(ssq / count); IEEE
 *              divide and square root; min and max: the float32 extremes on the order-preserving keys of csrc/ray_select.h (-0.0 < +0.0),
 *              widened exactly.  An empty label: all six +0.0.
 *              Both sums are added in ONE fixed order (csrc/stats_tree.h): per row, lane l of 64 adds the terms at x = l, l + 64, ... in
 *              increasing x from +0.0 (a sample outside the label is the term +0.0) and the 64 lane values are halved, v[l] + v[l + 32], then
 *              + 16 ... + 1; per label the row partials meet the same way over the rows l, l + 64, ...  The order is a function of (Z * H, W).
 *   status     0, or TS2D_STATS_NONFINITE: an intensity under a label is NaN or infinite; out_int and out_f64 are not written, the caller takes
 *              the host route.  The call returns TS2D_OK.
 * TS2D_ERR_INVALID, by name, before any device work: a null pointer, an unknown kind, K outside 1 ... 255, an extent below 1 or more than
 * 2^31 - 1 voxels, C outside 0 ... TS2D_STATS_MAX_CHANNELS, C > 0 without intensities or out_f64, a label map without values or with a value 0,
 * row partials of ONE label above max_scratch_bytes.  On any error the outputs are untouched.
 * (A new symbol of ABI 9: nothing that existed changed.) */
#define TS2D_STATS_PLANES 0
#define TS2D_STATS_LABELMAP 1
#define TS2D_STATS_NONFINITE 1
#define TS2D_STATS_INTS 10
#define TS2D_STATS_F64S 6
#define TS2D_STATS_MAX_CHANNELS 64
int ts2d_label_statistics(int device, const uint8_t* seg, int kind, const uint8_t* values, int K, int Z, int H, int W, const float* intensities,
                          int C, size_t max_scratch_bytes, int64_t* out_int, double* out_f64, int* status);

/* Percentiles of the intensities under a label on the device: per (label, channel, percentile) the two float32 samples numpy's linear
 * percentile interpolates between, and the weight.  The statement is totalsegmentator2d_amd/statistics.py (label_percentiles_statement, numpy);
 * the entry reproduces counts, rank values and weights bit for bit, and the caller interpolates on the host (statistics.percentile_of_values).
 * Host pointers in and out, synchronous: ONE upload, every label on the device, ONE download; scratch of the call's own, freed on every path.
 *   seg, kind, values, K, Z, H, W   as ts2d_label_statistics has them, with its limits.
 *   intensities  float32 [C][Z][H][W], C in 1 ... TS2D_STATS_MAX_CHANNELS.
 *   percentiles  float64 [P], P in 1 ... TS2D_STATS_MAX_PERCENTILES, each finite and in 0 ... 100.
 *   max_scratch_bytes  bound of the device state of the labels that work at once: per label and channel 2 P selections of a rank (int64), a
 *              prefix (uint64) and 256 bins (uint32), and per label the row partials of the counting pass (20 bytes per row); the labels are
 *              processed in chunks that stay below it; 0: 256 MiB.  The result does not depend on the chunking.
 *   out_count  int64 [K]: the label's samples, n.
 *   out_rank_f32  float32 [K][C][P][2]: the channel's samples under the label at the sorted positions i and j of percentile q among n:
 *              h = (n - 1) * (q / 100), i = min(floor(h), n - 1), j = min(i + 1, n - 1), each operation an IEEE float64 one.  The order is
 *              that of the order-preserving keys of csrc/ray_select.h: -0.0 right below +0.0, equal values repeated.
 *   out_weight_f64  float64 [K][P]: t = h - i.  It does not depend on the channel.
 *              An empty label: count 0, rank values +0.0, weights +0.0.
 *   status     0, or TS2D_STATS_NONFINITE: an intensity under a label is NaN or infinite; the outputs are not written, the caller takes the
 *              host route.  The call returns TS2D_OK.  A non-finite sample under no label is of no consequence.
 * The selection runs straight over (segmentation, intensity) pairs inside the label's bounding box - four rounds of one 8-bit digit of the key
 * each, no key buffer; the boxes are read on the device, none is downloaded (csrc/kernels_stats_select.h).
 * TS2D_ERR_INVALID, by name, before any device work: a null pointer, an unknown kind, K outside 1 ... 255, an extent below 1 or more than
 * 2^31 - 1 voxels, C outside 1 ... TS2D_STATS_MAX_CHANNELS, P outside 1 ... TS2D_STATS_MAX_PERCENTILES, a percentile that is not finite or
 * outside 0 ... 100, a label map without values or with a value 0, the state of ONE label above max_scratch_bytes.  On any error the outputs
 * are untouched.
 * (A new symbol of ABI 9: nothing that existed changed.) */
#define TS2D_STATS_MAX_PERCENTILES 8
int ts2d_label_percentiles(int device, const uint8_t* seg, int kind, const uint8_t* values, int K, int Z, int H, int W, const float* intensities,
                           int C, const double* percentiles, int P, size_t max_scratch_bytes, int64_t* out_count, float* out_rank_f32,
                           double* out_weight_f64, int* status);

/* The connected components of EVERY label of a segmentation at once on the device: per label how many pieces it has and how large they are, and a
 * clean-up rule - keep the largest piece, drop every piece below a size - for all labels in the same six or seven launches, whatever K is
 * (csrc/kernels_components.h; ts2d_keep_largest_components above takes one union of labels per step and six launches per step).  The statement is
 * totalsegmentator2d_amd/components.py (label_components_statement: scipy.ndimage.label per label); the entry reproduces it byte for byte.
 * Host pointers in and out, synchronous: ONE upload, every label on the device, ONE download; scratch of the call's own, freed on every path.
 *   seg, kind, values, K, Z, H, W   as ts2d_label_statistics has them, with its limits; a 2-D case is Z = 1.  The values of a label map are distinct.
 *   connectivity  TS2D_COMP_FULL: 26 neighbours (8 at Z = 1), what ts2d_keep_largest_components uses; TS2D_COMP_FACES: 6 (4 at Z = 1), scipy's default.
 *              The components are those of each label's mask ON ITS OWN: two labels that touch in a label map never join, nor do plane k and
 *              plane k + 1.
 *   keep_largest, min_voxels  the rule: a component of size s of label k is REMOVED iff (keep_largest != 0 and s < the largest size of label k) or
 *              s < min_voxels[k].  Components that tie for the largest all stay; s == min_voxels[k] stays; min_voxels NULL: zeros.  Removed voxels
 *              become 0: the background of a label map, that plane's voxel of planes.
 *   max_scratch_bytes  bound of the labelling state that works at once: 9 1/8 bytes per voxel (class 1, parent 4, count 4, one bit of run structure) -
 *              ONCE for a label map, whatever K is, and per label for planes, whose labels are processed in chunks that stay below the bound;
 *              0: 1 GiB.  The result does not depend on the chunking.  (The segmentation itself and the list lie beside it.)
 *   out_seg    NULL, or the cleaned segmentation, of the shape of seg.
 *   out_counters  int64 [K][TS2D_COMP_COUNTERS]: voxels, components, largest size, voxels removed, components removed.  An absent label: zeros.
 *   out_components, capacity  NULL with capacity 0, or int64 [capacity][3]: per component of the INPUT (label index k, first, size), first the smallest
 *              linear index of the component inside [Z][H][W]; sorted by (k, size descending, first), so the order in which the lanes arrive does
 *              not show.  out_n_components receives their number N, whatever the capacity is; the first N rows are written.
 *   status     0, or a union of
 *              TS2D_COMP_GIVE_UP    a bounded loop of the labelling reached its hard cap (those of ts2d_keep_largest_components; neither has been
 *                                   seen).  NO output is written; no retry, the caller takes the host route.
 *              TS2D_COMP_LIST_FULL  N > capacity.  out_seg, out_counters and out_n_components are valid, out_components is not written; a caller
 *                                   that wants the list calls again with a capacity of N.  (With capacity 0 that is every call that finds a
 *                                   component: a caller that wants no list ignores the bit.)
 *              The call returns TS2D_OK.
 * TS2D_ERR_INVALID, by name, before any device work: a null seg, out_counters, out_n_components or status, an unknown kind or connectivity, K outside
 * 1 ... 255, an extent below 1 or more than 2^31 - 1 voxels, a label map without values, with a value 0 or with a repeated value, a negative min_voxels
 * or capacity, capacity > 0 without out_components, the state of ONE label above max_scratch_bytes.  On any error the outputs are untouched.
 * (A new symbol of ABI 9: nothing that existed changed.) */
#define TS2D_COMP_FULL 0
#define TS2D_COMP_FACES 1
#define TS2D_COMP_GIVE_UP 1
#define TS2D_COMP_LIST_FULL 2
#define TS2D_COMP_COUNTERS 5
int ts2d_label_components(int device, const uint8_t* seg, int kind /* TS2D_STATS_PLANES | TS2D_STATS_LABELMAP */, const uint8_t* values, int K,
                          int Z, int H, int W, int connectivity, int keep_largest, const int64_t* min_voxels /* [K] or NULL */,
                          size_t max_scratch_bytes, uint8_t* out_seg /* cleaned, same shape; NULL: not wanted */,
                          int64_t* out_counters /* [K][5] */, int64_t* out_components /* [capacity][3] or NULL */, int64_t capacity,
                          int64_t* out_n_components, int* status);

/* Scoring a segmentation against a reference on the device.  The statements are totalsegmentator2d_amd/evaluate.py (project_labels,
 * overlap_statement, surface_statement; numpy); the three entries reproduce them byte for byte and bit for bit.  Host pointers in and out,
 * synchronous; each input is uploaded once, the result downloaded once; scratch of the call's own, freed on every path.
 *
 * ts2d_project_labels_coronal: the reference's project(..., 'multiclass:<num>') along the coronal axis (ts2d/core/util/image.py:164-194) of a
 * scalar INTEGER label volume, through the strided view of ts2d_project_coronal_modes (volume, n_elems, dtype, extents, element strides and base
 * as there; dtype 2, float, is refused).  planes_u8 [num][nz][nx]: plane k is 1 where any sample of the ray equals k + 1, else 0.  One pass over
 * the volume whatever num (1 ... 255) is.
 *   status     0, or TS2D_LABELS_RANGE: a sample lies outside 0 ... num; planes_u8 is not written, and the caller raises (there is no other route
 *              that would give a result).  The call returns TS2D_OK.
 *
 * ts2d_label_overlap: per label the samples on side a, on side b and on both.  a, kind_a and b, kind_b: each as seg, kind of
 * ts2d_label_statistics (TS2D_STATS_PLANES: uint8 [K][Z][H][W], label k is plane k > 0; TS2D_STATS_LABELMAP: ONE uint8 [Z][H][W], label k is
 * == values[k]); the two kinds may be mixed; values may be NULL where both are planes.  out_i64 [K][3] = n_a, n_b, n_both.
 *
 * ts2d_surface_distances: the boundary distances of 2-D planes [H][W] (a and b as above with Z = 1; H, W at most TS2D_EVAL_MAX_EXTENT).
 * A border pixel of a mask is a foreground pixel with at least one of its four neighbours background, outside the image being background.
 * For a border pixel p of one side, d2(p) = min over the border pixels q of the other side of
 * ((|py - qy| * spacing_h) * (|py - qy| * spacing_h) + (|px - qx| * spacing_w) * (|px - qx| * spacing_w)) in float64, every product and the sum
 * rounded on their own, +inf where the other side has no border - computed by the exact two-pass decomposition of csrc/surface_dist.h.
 *   tol_sq     [T] float64, T at most TS2D_EVAL_MAX_TOLERANCES: the SQUARES of the tolerances (the caller squares once)
 *   max_scratch_bytes  bound of the scratch (6 bytes per label and pixel); the labels are processed in chunks that stay below it; 0: 256 MiB.
 *              The result does not depend on the chunking.
 *   out_i64    [K][2][1 + T], direction 0: a against b, direction 1: b against a: the border pixels of the direction's own side, then per
 *              tolerance those of them with d2 <= tol_sq[t]
 *   out_f64    [K][2]: the largest d2 of the direction; -inf for an empty border, +inf where only the other side's is empty
 * TS2D_ERR_INVALID, by name, before any device work: a null pointer, an unknown kind or dtype, K or num outside 1 ... 255, an extent below 1 or
 * above its limit, a view that leaves the buffer, a label map without values or with a value 0, T outside its range, a negative tol_sq, a spacing
 * that is not finite and positive, scratch of ONE label above max_scratch_bytes.  On any error the outputs are untouched.
 * (New symbols of ABI 9: nothing that existed changed.) */
#define TS2D_LABELS_RANGE 1
#define TS2D_EVAL_MAX_TOLERANCES 8
#define TS2D_EVAL_MAX_EXTENT 32767
int ts2d_project_labels_coronal(int device, const void* volume, size_t n_elems, int dtype, int nz, int ny, int nx, long long sz, long long sy,
                                long long sx, long long base, int num, uint8_t* planes_u8, int32_t* status);
int ts2d_label_overlap(int device, const uint8_t* a, int kind_a, const uint8_t* b, int kind_b, const uint8_t* values, int K, int Z, int H, int W,
                       int64_t* out_i64);
int ts2d_surface_distances(int device, const uint8_t* a, int kind_a, const uint8_t* b, int kind_b, const uint8_t* values, int K, int H, int W,
                           double spacing_h, double spacing_w, const double* tol_sq, int T, size_t max_scratch_bytes, int64_t* out_i64,
                           double* out_f64);

/* ts2d_surface_distance_profile: ts2d_surface_distances and, from the same pass over the border pixels, per (label, direction) the SUM of the
 * boundary distances and their exact ORDER STATISTICS at requested percentiles - what the average surface distances and the percentile Hausdorff
 * distance (HD95) are made of.  The statement is evaluate.distance_profile_statement; the entry reproduces it bit for bit.  Every argument of
 * ts2d_surface_distances means what it means there, out_i64 and out_f64 are filled exactly as there, and one call serves a whole evaluation.
 *   percentiles  [P] float64, P at most TS2D_EVAL_MAX_PERCENTILES (0: none), each in 0 ... 100
 *   want_sum     not 0: out_sum_f64 is filled
 *   max_scratch_bytes  as above; per label and pixel 6 bytes, and with percentiles 16 more (the float64 bits of d2 of both directions, kept
 *                dense: a pixel's key lies at the pixel's place) besides 4 KiB of bins per label and percentile; with the sum 16 bytes per
 *                label and row.  The result does not depend on the chunking.
 *   out_sum_f64  [K][2] (want_sum): the sum of sqrt(d2) over the border pixels of the direction's own side, the correctly rounded root, added in
 *                the ONE fixed order of csrc/stats_tree.h over (H, W) with the term +0.0 for every other pixel (see ts2d_label_statistics).
 *                +0.0 for an empty border, +inf where only the other side's is empty.
 *   out_rank_f64 [K][2][P][2] (P > 0): with n border pixels, h = (n - 1) * (percentiles[p] / 100), i = min(floor(h), n - 1) and
 *                j = min(i + 1, n - 1) in IEEE float64 arithmetic, the d2 at the sorted positions i and j (from 0; ties are repeated values) -
 *                selected on the integer bits of d2, which order as the values do.  Both -inf for an empty border.
 *   out_weight_f64  [K][2][P] (P > 0): h - i, the weight of position j in the linear interpolation between the two ROOTS, which the caller
 *                forms (evaluate.percentile_of_ranks).  +0.0 for an empty border.
 * TS2D_ERR_INVALID, by name, before any device work: what ts2d_surface_distances refuses, P outside 0 ... TS2D_EVAL_MAX_PERCENTILES or without
 * percentiles, a percentile that is not a number or lies outside 0 ... 100, a null output that is asked for (out_sum_f64 with want_sum,
 * out_rank_f64 or out_weight_f64 with P > 0).  On any error the outputs are untouched.
 * (A new symbol of ABI 9: nothing that existed changed.) */
#define TS2D_EVAL_MAX_PERCENTILES 8
int ts2d_surface_distance_profile(int device, const uint8_t* a, int kind_a, const uint8_t* b, int kind_b, const uint8_t* values, int K, int H,
                                  int W, double spacing_h, double spacing_w, const double* tol_sq, int T, const double* percentiles, int P,
                                  int want_sum, size_t max_scratch_bytes, int64_t* out_i64, double* out_f64, double* out_sum_f64,
                                  double* out_rank_f64, double* out_weight_f64);

/* ts2d_volume_surface_distances: the boundary distances of VOLUMES [Z][H][W] and, on request, their profile - ts2d_surface_distance_profile
 * with one more axis.  The statements are evaluate.volume_surface_statement and evaluate.volume_distance_profile_statement; the entry reproduces
 * them bit for bit.  a, kind_a, b, kind_b, values, K as in ts2d_label_overlap; each extent 1 ... TS2D_EVAL_MAX_EXTENT and Z * H * W at most
 * 2^31 - 1.  A border voxel of a mask is a foreground voxel with at least one of its SIX face neighbours background, outside the volume being
 * background (so with Z = 1 every foreground voxel is one: that is not the 2-D border of ts2d_surface_distances).  For a border voxel p of one
 * side, d2(p) = min over the border voxels q of the other side of ((f(|pz - qz|, spacing_z) + f(|py - qy|, spacing_h)) + f(|px - qx|, spacing_w))
 * with f(n, s) = (n * s) * (n * s), in float64, that association, every operation rounded on its own, +inf where the other side has no border -
 * computed by the exact three-pass decomposition of csrc/surface_dist.h inside each label's joint bounding box (csrc/kernels_evaluate_volume.h).
 * P = 0 and want_sum = 0 is the plain form: out_sum_f64, out_rank_f64 and out_weight_f64 may then be NULL.  tol_sq, T, percentiles, P, want_sum
 * and the five outputs mean what they mean in ts2d_surface_distance_profile, with the same layouts; the sum meets in the tree of
 * csrc/stats_tree.h over (Z * H, W).
 *   max_scratch_bytes  bound of the scratch that labels working at once take together; 0: 4 GiB.  Per label and voxel OF ITS BOX (the inclusive
 *              box of the label over both sides) 22 bytes - 2 of border, 4 of line distances, 16 of the float64 second pass -, with percentiles 16
 *              more, and with the sum 16 per box row (z, y); a label that is empty on both sides takes none.  The labels are packed into chunks
 *              that stay below the bound, in their order.  The result does not depend on the chunking.
 * TS2D_ERR_INVALID, by name: what ts2d_surface_distance_profile refuses (before any device work) and, once the boxes are known, scratch of ONE
 * label above max_scratch_bytes, or a label whose box has more than 2^26 - 1 = 67 108 863 rows (z, y) - one wave works per box row, and the
 * runtime cuts a launch of 2^32 lanes or more short instead of refusing it; W < 32 at such a box.  On any error the outputs are untouched.
 * (A new symbol of ABI 9: nothing that existed changed.) */
int ts2d_volume_surface_distances(int device, const uint8_t* a, int kind_a, const uint8_t* b, int kind_b, const uint8_t* values, int K, int Z,
                                  int H, int W, double spacing_z, double spacing_h, double spacing_w, const double* tol_sq, int T,
                                  const double* percentiles, int P, int want_sum, size_t max_scratch_bytes, int64_t* out_i64, double* out_f64,
                                  double* out_sum_f64, double* out_rank_f64, double* out_weight_f64);

/* ts2d_label_confusion: the confusion (co-occurrence) matrix of two segmentations - for every pair of labels (i of a, j of b) the samples that
 * are in both - in ONE integer matrix product on the device (csrc/kernels_confusion.h: v_mfma_i32_32x32x32_i8 over 0 / 1 bytes, exact in int32).
 * The statement is evaluate.confusion_statement; the entry reproduces it integer for integer.  a, kind_a, b, kind_b, values, K, Z, H, W as in
 * ts2d_label_overlap, with its contract: host pointers, synchronous, each input uploaded once (a == b, the same pointer with the same kind, is
 * allowed and uploaded once), one download, scratch of the call's own (one byte per sample and side), freed on every path.
 *   out_i64    [K + 2][K + 2], row = side a, column = side b.  Either side has K + 2 indicator rows over the N = Z * H * W samples: row 0 "none
 *              of the K labels" (planes: every plane is 0 there; label map: the byte is not among values), row 1 + k the mask of label k, row
 *              K + 1 every sample.  out[i][j] counts the samples in row i of a and in row j of b, so out[1 + k][1 + k], out[1 + k][K + 1] and
 *              out[K + 1][1 + k] are n_both, n_a and n_b of ts2d_label_overlap, and out[K + 1][K + 1] = N.  With a planes side a sample may be in
 *              several rows.
 * Limits: K 1 ... 255; every extent at least 1; N at most 2^31 - 1 samples (an int32 accumulator of the product counts samples, so none can
 * overflow); a planes side is K * N bytes, up to 2^39, and every byte offset is 64-bit.
 * TS2D_ERR_INVALID, by name, before any device work: a null pointer, an unknown kind, K outside 1 ... 255, an extent below 1, more than
 * 2^31 - 1 samples, a label map without values or with a value 0.  On any error the output is untouched.
 * (A new symbol of ABI 9: nothing that existed changed.) */
int ts2d_label_confusion(int device, const uint8_t* a, int kind_a, const uint8_t* b, int kind_b, const uint8_t* values, int K, int Z, int H, int W,
                         int64_t* out_i64 /* [K + 2][K + 2], row = side a */);

/* ts2d_label_morphology: grow (dilate), shrink (erode), open or close every label of a 2-D segmentation by a radius in the unit of the spacing, with
 * an exact Euclidean disc: offset (dy, dx) belongs iff (|dy| * sy)^2 + (|dx| * sx)^2 <= radius * radius in float64, every operation rounded on its
 * own (csrc/morph.h; a pixel exactly on the circle belongs).  Erosion is the dual INSIDE the image, E(M) = ~D(~M): outside the image is neither
 * background nor foreground, so a mask that touches an edge is not eaten from that edge.  open = D(E(M)), close = E(D(M)).  The statement is
 * morphology.label_morphology_statement; the entry reproduces it byte for byte, counters included.  The float64 comparison is decided on the host,
 * in a table of at most H integers; the kernels (csrc/kernels_morph.h) hold no floating-point number, and every loop is bounded by an extent: there
 * is no give-up status.
 *   seg, kind, values, K   as in ts2d_label_statistics with Z = 1: TS2D_STATS_PLANES, uint8 [K][H][W], label k is plane k > 0;
 *                 TS2D_STATS_LABELMAP, ONE uint8 [H][W] and values[K], each 1 ... 255 and distinct, label k is seg == values[k].
 *   sy, sx        the spacing of a row step and of a column step; radius in the same unit, 0 allowed (the output equals the input)
 *   select        NULL (every label) or K bytes: label k is worked iff select[k] != 0.  An unselected label is returned untouched.
 *   out_seg       the layout of seg.  Planes: every label on its own; a pixel that stays set keeps its byte, a cleared one becomes 0, a new one 1.
 *                 Label map: each selected label's result is computed on its own mask (everything else counts as outside it).  erode and open
 *                 clear the pixels of label k that its result does not hold.  dilate and close paint samples equal to 0 only, in the order of
 *                 values (the first label wins); a non-zero sample, named or not, is never overwritten.
 *   out_counters  int64 [K][TS2D_MORPH_COUNTERS]: pixels before, pixels after, added, removed (of a label map: counted after painting).
 *   max_scratch_bytes   bounds the device scratch of the labels that work at once (0: 256 MiB): per label and pixel 2 bytes, + 1 for open and
 *                 close, + 1 for a label map.  The two copies of the segmentation are not counted.
 * Host pointers in and out; synchronous; the call owns its device scratch and frees it on every path.
 * TS2D_ERR_INVALID, by name, before any device work and with the outputs untouched: a null seg, out_seg or out_counters, an unknown kind or op, K
 * outside 1 ... 255, an extent below 1 or above TS2D_EVAL_MAX_EXTENT, more than 2^31 - 1 pixels, a radius that is negative or not finite, a
 * spacing that is not positive and finite, a label map without values, with a value 0 or a repeated one, a bound below the scratch of one label.
 * (A new symbol of ABI 9: nothing that existed changed.) */
#define TS2D_MORPH_DILATE 0
#define TS2D_MORPH_ERODE 1
#define TS2D_MORPH_OPEN 2
#define TS2D_MORPH_CLOSE 3
#define TS2D_MORPH_COUNTERS 4
int ts2d_label_morphology(int device, const uint8_t* seg, int kind /* TS2D_STATS_PLANES | TS2D_STATS_LABELMAP */, const uint8_t* values, int K,
                          int H, int W, double sy, double sx, int op /* TS2D_MORPH_* */, double radius, const uint8_t* select /* K or NULL */,
                          uint64_t max_scratch_bytes, uint8_t* out_seg, int64_t* out_counters /* [K][TS2D_MORPH_COUNTERS] */);

/* Synthetic slice stream on the device (BASELINE config 4: "synthetic 10k-slice stream", generated per rank from (seed, slice
 * index) so that no host transfer skews the timing).  Writes n_elements fp32 values, approximately N(0,1), to device memory:
 * element i of the call = element (first_element + i) of the stream identified by `key`; a value depends on (key, element index)
 * only, so every rank can produce any block of the stream, and it is bit-identical to the host generator
 * totalsegmentator2d_amd/prng.py (key = prng.key(seed, stream)).  Asynchronous on `stream` (hipStream_t as void*, NULL = default).
 * The reference has no counterpart (it reads files); the bench and the multi-GPU tests are the callers. */
int ts2d_synth_slices(int device, unsigned long long key, unsigned long long first_element, unsigned long long n_elements,
                      float* out_device, void* stream);

/* Pre-allocate the activation workspace for (B, H, W) (reference warm-up contract: a zero patch is pushed through
 * the predictor once at start-up, prediction_worker.py:74-96,136-138). */
int ts2d_engine_reserve(ts2d_engine* e, int B, int H, int W);

/* Caller-provided activation workspace (ABI 6).  ts2d_engine_workspace_bytes: the bytes ts2d_engine_reserve(B, H, W) would
 * allocate under the engine's current precision mode / options.  ts2d_engine_set_workspace: use [dev_ptr, dev_ptr + n_bytes) (256-byte
 * aligned device memory owned by the caller, alive until it is replaced or the engine destroyed) instead of an allocation of the
 * engine's own; dev_ptr = NULL returns to that.  A forward that needs more than n_bytes fails with TS2D_ERR_NOMEM.  Purpose: the five
 * sub-models of ts2d-v2 run one after the other on one stream (the reference drives them sequentially, ts2d/tool.py:110-112), so ONE
 * workspace of the largest size serves all five engines.  Engines that share a workspace must be driven on the same stream (or be
 * ordered by the caller): the engine's own cross-stream ordering covers the runs of ONE handle only. */
int ts2d_engine_workspace_bytes(ts2d_engine* e, int B, int H, int W, size_t* n_bytes);
int ts2d_engine_set_workspace(ts2d_engine* e, void* dev_ptr, size_t n_bytes);

/* Per-op device timing (HIP events on the launch stream).  enable != 0 brackets every kernel of subsequent forwards
 * with events; ts2d_engine_op_times returns for the LAST forward the elapsed ms per op (n_ops entries, program
 * order; see ts2d_engine_op_name) - synchronises the stream. */
int ts2d_engine_set_profiling(ts2d_engine* e, int enable);
int ts2d_engine_num_ops(ts2d_engine* e);
const char* ts2d_engine_op_name(ts2d_engine* e, int op);
/* The kernel that served entry `op` of the last profiled forward ("conv3x3_f16x3_q", "conv3x3_upc<64>", "finalize_stats", ...):
 * the dispatch depends on precision mode, channel counts and tile geometry, bench.py groups its roofline blocks by this. */
const char* ts2d_engine_op_kernel(ts2d_engine* e, int op);
/* Test accessor (ABI 9): the split-K factor entry `op` of the last profiled forward ran with - S > 1: the conv wrote S fp32 partial
 * sums that the entry "<name>.stats" behind it reduced; 1: it did not split (every ".stats" entry, every kernel without a split-K
 * form).  0: no such entry - an op that was composed into its consumer launches nothing and has none.  The factor depends on the
 * batch size and the CU count (option "sbk"), so a test that means to address the split-K arithmetic asserts it here first. */
int ts2d_engine_op_ksplit(ts2d_engine* e, int op);
int ts2d_engine_op_times(ts2d_engine* e, float* ms, int n_ops);

/* Test/debug accessor (not on the product path): copies activation tensor `name` ("enc0.c1", "dec3.up", ... - the
 * op names of ts2d_engine_op_name) of the LAST forward to host as NCHW fp32 [B,C,h,w], with the InstanceNorm +
 * LeakyReLU that its consumer applies on load already applied (i.e. what torch holds after the block).
 * `capacity` = floats available in out; *dims receives {B, C, h, w}.  Synchronises the engine. */
int ts2d_engine_debug_tensor(ts2d_engine* e, const char* name, float* out, size_t capacity, int32_t dims[4]);

/* Bytes of device memory currently held (weights + workspace). */
size_t ts2d_engine_device_bytes(ts2d_engine* e);

int ts2d_engine_destroy(ts2d_engine* e);

/* Thread-local message of the last failing call on this thread ("" if none). */
const char* ts2d_last_error(void);

/* ABI version of this header (bumped on any signature change). */
int ts2d_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* TS2D_ENGINE_H */
