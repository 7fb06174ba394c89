// What the host planning (tiled_plan.cpp, prep_plan.cpp: plain C++, no offload pass) and the kernels that read it agree on: the PODs that are
// copied to the device as bytes or passed by value, and the constants both sides use.  No device code here (the pattern of tile_dims.h);
// kernels_sw.h, kernels_resample.h, kernels_resample_in.h, kernels_prep.h and kernels.h include it instead of declaring these themselves.
#pragma once

namespace ts2d {

// sigmoid(x) > 0.5  <=>  x > 1.5 * 2^-24 on the ATen CPU kernels the oracle was pinned with (kernels.h, the head; tests/test_oracle.py)
constexpr float kSigmoidHalfThreshold = 0x1.8p-24f;

// ---- sliding window (kernels_sw.h): one segment per image that has rows in a chunk
constexpr int kSwChunkRows = 64;        // network rows (tile x mirror variant) of one chunk = the batch of one forward
constexpr int kMaxFolds = 32;           // engines of one ensemble call

struct SwSeg {
    long long img_off;      // floats from the image area to this image's [C, Hp, Wp] (a multiple of 4)
    long long out_off;      // elements from the output areas to this image's [K, Hp, Wp] (a multiple of 8)
    int Hp, Wp;
    int tile0, n_tiles;     // its tile origins are tile_y / tile_x[tile0 ... tile0 + n_tiles)
    int row0, n_rows;       // rows (tile * V + variant) of the image gathered in this chunk: [row0, row0 + n_rows)
    int batch_row;          // ... they are rows [batch_row, batch_row + n_rows) of the chunk's batch
    int log_row;            // row of the logit buffer that holds the image's row 0 (aggregate)
    int image;              // index of the image in the call (its inf flag)
    int pad_;
    unsigned gblock0;       // first block of the segment in the gather launch
    unsigned ablock0;       // ... in the aggregate launch
};
static_assert(sizeof(SwSeg) == 64, "SwSeg is copied to the device as bytes");

// ---- the export's order-1 resample (kernels_resample.h: K planes out; kernels_labelmap.h: the argmax over the K planes, ONE plane out)
struct RsSeg {
    long long src_off;      // elements from the half outputs to this image's aggregated [K, Hp, Wp] (SwSeg::out_off)
    long long dst_off;      // elements from the resampled outputs to this image's [K, out_h, out_w] (a multiple of 4); label map: [out_h, out_w]
    int Hp, Wp;
    int out_h, out_w;
    int tap0;               // its taps: rows at taps[tap0 ... tap0 + out_h), columns at taps[tap0 + out_h ... tap0 + out_h + out_w)
                            // label map only: -1 = output extent == source rectangle, no taps - src_off then points at the rectangle's first sample
    unsigned block0;        // first block of the image in the launch
};
static_assert(sizeof(RsSeg) == 40, "RsSeg is copied to the device as bytes");

struct RsTap {
    double w0, w1;          // weights of the two source samples
    int i0, i1;             // their row / column in the padded [Hp, Wp] plane (source rectangle origin included)
};
static_assert(sizeof(RsTap) == 24, "RsTap is copied to the device as bytes");

// ---- the export's probabilities (kernels_prob.h): what a segment of sw_probabilities needs beside its RsSeg (same index).  The lanes of a
// probabilities segment walk the FULL pre-crop extent, not the output extent: RsSeg::block0 counts blocks of full_h x ceil(full_w / 4) lanes
enum ProbMode : int { kProbMultilabel = 0, kProbLabelmap = 1, kProbRegions = 2 };      // the TS2D_PROB_* of the C header
struct ProbSeg {
    long long prob_off;     // elements from the float outputs to this image's [K, full_h, full_w] (a multiple of 4)
    long long dec_off;      // elements from the uint8 outputs to this image's decided map (a multiple of 4): [K, full_h, full_w] multilabel, else [full_h, full_w]
    int full_h, full_w;     // the extent before cropping: what the kernel writes
    int box_y, box_x;       // where the resampled [out_h, out_w] rectangle sits in it; everything else is the fill
};
static_assert(sizeof(ProbSeg) == 32, "ProbSeg is copied to the device as bytes");

// ... and of sw_probabilities<ProbStackSeg>: the image is slice s of a RUN of n_slices images whose outputs lie head-major, [K][n_slices][full_h][full_w],
// so that a head of the whole run is one contiguous piece; head k of the slice is at prob_off + k * prob_stride.  Every field is a multiple of 4
// where full_w is (the vector stores' condition)
struct ProbStackSeg {
    long long prob_off;     // elements from the float outputs to head 0 of this slice: the run's first element + s * full_h * full_w
    long long dec_off;      // ... from the uint8 outputs to this slice of the decided map ([K][n_slices] planes multilabel, else [n_slices] planes)
    long long prob_stride;  // elements between the heads of a slice: n_slices * full_h * full_w
    long long dec_stride;   // ... of the decided map (multilabel; else unused: its one plane is head 0)
    int full_h, full_w;
    int box_y, box_x;
};
static_assert(sizeof(ProbStackSeg) == 48, "ProbStackSeg is copied to the device as bytes");

// ---- the order-3 input resample (kernels_resample_in.h)
constexpr int kRsInPad = 12;            // scipy's _prepad_for_spline_filter for mode='nearest'
constexpr int kRsInMaxExtent = 8192;    // preprocess.CUBIC_MAX_EXTENT

struct RsInAxis {           // line-independent constants of the prefilter along one axis (n = padded extent of that axis)
    double z, gain, zn;     // pole, gain, z^n (libm pow on the host, as scipy calls it)
    double k0, k1;          // z / (1 - z^n * z^n),  z / (z - 1)
};
static_assert(sizeof(RsInAxis) == 40, "RsInAxis is passed by value");

struct RsInTap {
    double w[4];            // weights of four consecutive coefficients
    int start, pad_;        // index of the first one in the padded line
};
static_assert(sizeof(RsInTap) == 40, "RsInTap is copied to the device as bytes");

// ---- crop box and z-score of native 2-D inputs (kernels_prep.h)
constexpr int kPrepChunk = 8192;        // numpy's buffer size in elements: the run its add.reduce hands to the pairwise sum
constexpr int kPrepLeaf = 128;          // numpy's PW_BLOCKSIZE: the longest run summed in eight accumulators
constexpr int kPrepMaxTailLeaves = 160; // a partial chunk (< 8192 elements) has fewer leaves than this (each is longer than 56)

struct PrepLeaf { int off, len; };      // a leaf of the partial chunk's tree, `off` counted from the chunk's first element
static_assert(sizeof(PrepLeaf) == 8, "PrepLeaf is copied to the device as bytes");

struct PrepNorm { float mean, div; };   // per plane: what prep_chunk_sums<1> subtracts and prep_normalise subtracts and divides by
static_assert(sizeof(PrepNorm) == 8, "PrepNorm is copied to the device as bytes");

// ---- every normalisation scheme on those planes (kernels_prep_schemes.h); the ids and status bits are the TS2D_NORM_* / TS2D_PLANES_* of the C header
enum PrepSchemeId : int { kPrepZScore = 0, kPrepCT = 1, kPrepRescale01 = 2, kPrepRGB01 = 3, kPrepNone = 4 };
enum PrepStatus : int { kPrepStatusNonfinite = 1, kPrepStatusRgbRange = 2, kPrepStatusEmptyMask = 4, kPrepStatusZeroSign = 8, kPrepStatusFillRounds = 16 };
constexpr int kPrepMaskBlock = 2048;    // pixels per workgroup of the mask kernels: 8 rows of 256 lanes

// per plane: x <- fl32(fl32(clip(x) - sub) / div); the clip to [lo, hi] for kPrepCT only, nothing at all for kPrepNone, and with `masked`
// (kPrepZScore only) only where the case's non-zero mask is set
struct PrepScheme { int id, masked; float sub, div, lo, hi; };
static_assert(sizeof(PrepScheme) == 24, "PrepScheme is copied to the device as bytes");

}  // namespace ts2d
