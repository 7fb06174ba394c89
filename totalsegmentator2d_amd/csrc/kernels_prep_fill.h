// The non-zero mask of a STACK with its holes filled in 3-D: what nnU-Net's create_nonzero_mask makes of a volume (reference flow
// DefaultPreprocessor.run_case, ts2d/core/inference/prediction_worker.py:194-199; the mask is scipy's binary_fill_holes with its default cross
// structure over "non-zero in ANY channel") and what ZScoreNormalization with use_mask_for_norm takes its mean and std over.  It runs on the dense
// cropped buffer [C][bz][bh][bw] that prep_compact_box3 of kernels_prep_stack.h leaves.  Five kernels behind ts2d_planes_crop_normalize_stack_masked
// (prep.hip):
//     prep_fill_planes          two bit planes, 64 voxels of a row per 64-bit word along x: bg = "zero in every channel", out = the SEEDS, the bg voxels
//                               on one of the six faces of the box
//     prep_fill_sweep_words     one directional sweep along z or y, word-wise: out[i] |= bg[i] & out[i -+ 1]
//     prep_fill_sweep_rows<D>   one directional sweep along x: an occluded fill inside each word, the carry handed from word to word of the row
//     prep_fill_mask_counts     the mask ~out as the bytes prep_mask_scatter and prep_apply_schemes_stack read, and how many voxels of it each block
//                               of 2048 holds: prep_mask_counts of kernels_prep_schemes.h for a GIVEN mask instead of one derived from the samples
//
// Why the box is enough.  Upstream fills the holes of the mask of the WHOLE array and crops afterwards; here the crop comes first and the six faces of
// the box are the border.  Every voxel outside the box is zero in every channel, and from any of them a straight line along an axis reaches the array's
// border without meeting the mask: the whole outside of the box is background connected to the border.  A background voxel inside the box is therefore
// connected to the array's border iff it is 6-connected through background to a face of the box - through the face into the outside one way, and a
// path to the array's border must cross a face the other way.  So the fill inside the box, seeded at its faces, gives upstream's mask restricted to
// the box (tests/test_stack_masked_cpu.py: hundreds of random volumes against scipy, no mismatch).
//
// Why the order does not show.  The result is unique: a background voxel stays OUTSIDE the mask iff it is 6-connected through background to a face.
// `out` only ever grows, stays inside bg, and a round that adds nothing has reached that fixed point; any order of propagation gives scipy's bytes.
// A ROUND is six sweeps in fixed order - z up, z down, y up, y down, x up, x down - each its own launch that sees the one before; every sweep ORs
// "some bit was added" into one device int with an ordinary integer atomic, and the host reads it after the round.  A round that adds nothing ends
// the loop; after kPrepFillMaxRounds rounds that each still added something the entry gives up (TS2D_PLANES_FILL_ROUNDS) and the caller takes numpy:
// no open-ended loop on the device and no retry.  Head-like masks take 2 ... 7 rounds; a one-voxel serpentine corridor of height H takes
// (H - 1) / 2 + 1 (preprocess.fill_holes_sweeps_statement restates these sweeps and counts the same rounds).
//
// Ownership: in a sweep along z a lane owns one word COLUMN (y, word) and walks it through the slices, along y the column (z, word) through the rows
// - adjacent lanes take adjacent words of a row, so the loads coalesce; along x a lane owns one ROW.  No two lanes of a launch touch the same word.
// The padding bits of a row's last word are neither background nor seed: they would otherwise carry "outside" across the row end.
// Integers only, plain stores; nothing here uses MFMA or LDS beyond the 4-byte block count of prep_fill_mask_counts.
#pragma once
#include "kernels_prep_schemes.h"

namespace ts2d {

constexpr int kPrepFillMaxRounds = 64;  // rounds of six sweeps the entry runs before it leaves the volume to numpy
constexpr int kPrepFillBatch = 8;       // words of a line prep_fill_sweep_words has in flight: the loads do not hang on the chain, only the ORs do

typedef unsigned long long prep_word;

// bg, out [bz][bh][ww] with ww = ceil(bw / 64): bit k of word w of a row is its voxel 64 w + k.  x [channels][bz][bh][bw].  `v != 0` as numpy has it:
// a NaN is not zero, -0.0 is.  One WAVE per word (the ballot of its 64 lanes is the word); grid = ceil(bz bh ww / 4), 256 lanes.
__global__ __launch_bounds__(256) void prep_fill_planes(const float* __restrict__ x, int channels, int bz, int bh, int bw, prep_word* __restrict__ bg,
                                                        prep_word* __restrict__ out) {
    const int ww = (bw + 63) >> 6, lane = threadIdx.x & 63;
    const long long words = (long long)bz * bh * ww, word = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (word >= words) return;                                   // (the whole wave leaves together)
    const long long row = word / ww;
    const int col = (int)(word % ww) * 64 + lane, y = (int)(row % bh), z = (int)(row / bh);
    const size_t n = (size_t)bz * bh * bw;
    bool zero = col < bw;
    if (zero)
        for (int c = 0; c < channels; ++c) zero &= !(x[(size_t)c * n + (size_t)row * bw + col] != 0.f);
    const bool face = z == 0 || z == bz - 1 || y == 0 || y == bh - 1 || col == 0 || col == bw - 1;
    const prep_word b = __ballot(zero), s = __ballot(zero && face);
    if (lane == 0) { bg[word] = b; out[word] = s; }
}

// One sweep along z or y.  Line l of `lines` starts at word (l / inner) * outer + l % inner and has `len` words `stride` apart; dir = +1 walks it from
// its first word, -1 from its last.  Along z: lines = inner = bh ww, outer = 0, stride = bh ww, len = bz; along y: lines = bz ww, inner = ww,
// outer = bh ww, stride = ww, len = bh.  *added |= 1 where a bit was set.  grid = ceil(lines / 64), 64 lanes.
__global__ __launch_bounds__(64) void prep_fill_sweep_words(const prep_word* __restrict__ bg, prep_word* __restrict__ out, long long lines, long long inner,
                                                            long long outer, long long stride, int len, int dir, int* __restrict__ added) {
    const long long l = (long long)blockIdx.x * 64 + threadIdx.x;
    bool any = false;
    if (l < lines) {
        const long long base = (l / inner) * outer + l % inner + (dir > 0 ? 0 : (long long)(len - 1) * stride), step = dir * stride;
        prep_word prev = out[base];
        for (int k = 1; k < len; k += kPrepFillBatch) {
            prep_word o[kPrepFillBatch], b[kPrepFillBatch];
#pragma unroll
            for (int j = 0; j < kPrepFillBatch; ++j)
                if (k + j < len) { o[j] = out[base + (k + j) * step]; b[j] = bg[base + (k + j) * step]; }
#pragma unroll
            for (int j = 0; j < kPrepFillBatch; ++j)
                if (k + j < len) {
                    const prep_word g = o[j] | (b[j] & prev);
                    if (g != o[j]) { out[base + (k + j) * step] = g; any = true; }
                    prev = g;
                }
        }
    }
    if (__any(any) && threadIdx.x == 0) atomicOr(added, 1);
}

// the bits of p (a run of background) that g reaches towards the higher / the lower bits: a Kogge-Stone occluded fill, six doubling steps
__device__ __forceinline__ prep_word prep_fill_up(prep_word g, prep_word p) {
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) { g |= p & (g << s); p &= p << s; }
    return g;
}
__device__ __forceinline__ prep_word prep_fill_down(prep_word g, prep_word p) {
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) { g |= p & (g >> s); p &= p >> s; }
    return g;
}

// One sweep along x: a lane owns one of the `rows` = bz bh rows of ww words and hands the carry - the last voxel it reached - from word to word.
// UP walks towards the higher x.  *added |= 1 where a bit was set.  grid = ceil(rows / 64), 64 lanes.
template <bool UP>
__global__ __launch_bounds__(64) void prep_fill_sweep_rows(const prep_word* __restrict__ bg, prep_word* __restrict__ out, long long rows, int ww,
                                                           int* __restrict__ added) {
    const long long r = (long long)blockIdx.x * 64 + threadIdx.x;
    bool any = false;
    if (r < rows) {
        const prep_word* b = bg + (size_t)r * ww;
        prep_word* o = out + (size_t)r * ww;
        prep_word carry = 0;
        for (int k = 0; k < ww; ++k) {
            const int w = UP ? k : ww - 1 - k;
            const prep_word cur = o[w], p = b[w];
            const prep_word g = UP ? prep_fill_up(cur | (p & carry), p) : prep_fill_down(cur | (p & (carry << 63)), p);
            if (g != cur) { o[w] = g; any = true; }
            carry = UP ? g >> 63 : g & 1;
        }
    }
    if (__any(any) && threadIdx.x == 0) atomicOr(added, 1);
}

// mask [n] <- 1 where the voxel is NOT in `out` (n = bz bh bw voxels in index order, out [bz bh][ceil(bw / 64)]), counts [blocks] <- masked voxels of
// each block: the contract of prep_mask_counts.  grid = ceil(n / 2048), 256 lanes.
__global__ __launch_bounds__(256) void prep_fill_mask_counts(const prep_word* __restrict__ out, int bw, long long n, uint8_t* __restrict__ mask,
                                                             int* __restrict__ counts) {
    __shared__ int total;
    if (threadIdx.x == 0) total = 0;
    __syncthreads();
    const int ww = (bw + 63) >> 6;
    const long long i0 = (long long)blockIdx.x * kPrepMaskBlock + threadIdx.x;
    int mine = 0;
#pragma unroll
    for (int k = 0; k < kPrepMaskRows; ++k) {
        const long long i = i0 + k * 256;
        bool in = false;
        if (i < n) {
            const long long row = i / bw;
            const int col = (int)(i - row * bw);
            in = !(out[(size_t)row * ww + (col >> 6)] >> (col & 63) & 1);
            mask[i] = in ? 1 : 0;
        }
        mine += __popcll(__ballot(in));                          // (every lane of the wave holds the wave's count)
    }
    if ((threadIdx.x & 63) == 0) atomicAdd(&total, mine);        // integers: the order of the four waves does not show
    __syncthreads();
    if (threadIdx.x == 0) counts[blockIdx.x] = total;
}

}  // namespace ts2d
