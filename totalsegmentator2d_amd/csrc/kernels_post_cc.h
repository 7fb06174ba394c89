// nnU-Net's postprocessing on a decided label map [UPSTREAM-RECALL: remove_all_but_largest_component_from_segmentation, the function that
// nnUNetv2_find_best_configuration stores beside a model]: of the voxels whose label a step names, every 26-connected component that is not of
// maximal size becomes the step's background label.  postprocess.keep_largest_components_statement is the definition (scipy.ndimage.label with the
// full 3 x 3 x 3 structure, np.bincount, "keep every component of the largest size"); these kernels give its bytes.  They work on a device-resident
// uint8 [Z][H][W], a 2-D case being Z = 1, and are launched one after the other, per step, by ts2d_keep_largest_components (post.hip):
//     cc_mask_init   mask = member[seg]; its bit words, 64 voxels of a row per word (one ballot per word, as prep_fill_planes builds them); the initial
//                    parent of a mask voxel = the first voxel of its run inside the word, so a run along x costs no atomic; count <- 0; the mask voxels
//     cc_link        every mask voxel joins the components of its 13 earlier neighbours (cc_label.h: cc_link_voxel, cc_union)
//     cc_flatten     parent[i] <- the root above i; the roots are counted: the components
//     cc_count       count[root] += the voxels of every run of a word, one integer atomicAdd per run (the lanes of a run share their root)
//     cc_max         the largest count: an integer atomicMax per wave over its roots
//     cc_apply       seg[i] <- background where i is in the mask and count[parent[i]] is below the maximum; the voxels removed
// Every kernel runs one WAVE per 64-bit word, lane k on voxel 64 w + k of the row (lanes past W idle): grid = ceil(Z H ceil(W / 64) / 4), 256 lanes;
// from 2^26 - 3 words on (W < 32 at the largest volumes) that grid passes 2^32 threads and folds along z (entry_util.h: fold_grid).
// All indices are int32: the entry refuses more than 2^31 - 1 voxels.  parent holds -1 or an index below Z H W, count is indexed by a parent that is
// >= 0 only, the tables have 256 entries and are indexed by a byte: no access can leave its array whatever the arrival order.
//
// Termination (the machines are shared; each loop is bounded twice).  The only loops are cc_find and cc_union of cc_label.h.  Parents only decrease and
// parent[x] <= x, so a find chain is strictly decreasing and a union round that does not finish strictly lowers its pair: both end by monotonicity.
// Both also count their iterations against a hard cap (kCcFindCap, kCcUnionCap); a lane that reaches it ORs TS2D_CC_GIVE_UP into the status word and
// returns.  Every later launch of the call stays bounded the same way, cc_apply writes nothing once the bit is set, and the entry leaves the caller's
// buffer alone and reports the bit: the caller takes the host route, there is no retry here.
// No lane waits for another: no flag, no spin, no cooperative or persistent launch; what one phase needs of the one before it gets from the launch
// boundary.  Integer atomics (min, add, max, or), relaxed loads and plain vector stores only; no inline assembly, no LDS, no floating point.
//
// Why the arrival order does not show.  The edges cc_link joins are a fixed set - those of the 26-neighbourhood inside the mask - and a union-find
// that has joined all of them holds the one partition they generate, whichever lane won which race; only WHICH voxel a component has as its root could
// differ, and in fact does not: the root is the minimum index.  The sizes are integer sums, the maximum an integer maximum, and "below the maximum"
// keeps every component that ties for it, so no choice is left to the order: seg and the four counters are functions of the input alone.
#pragma once
#include <hip/hip_runtime.h>

#include "cc_label.h"           // cc_find, cc_union, cc_link_voxel (its device atomics need the runtime header first)

namespace ts2d {

constexpr int kCcStatusGiveUp = 1;       // TS2D_CC_GIVE_UP
constexpr int kCcCounters = 4;           // per step: mask voxels, components, largest size, voxels removed

// where the lane stands: word `word` of `words`, its row, and voxel x of that row (x may lie past W - 1 in a row's last word)
struct CcLane {
    long long word, row;
    int lane, x;
};
__device__ __forceinline__ bool cc_lane(long long words, int ww, CcLane* l) {
    l->lane = threadIdx.x & 63;
    l->word = ((long long)blockIdx.z * gridDim.x + blockIdx.x) * 4 + (threadIdx.x >> 6);      // (a folded grid: entry_util.h, fold_grid)
    if (l->word >= words) return false;                          // (the whole wave leaves together)
    l->row = l->word / ww;
    l->x = (int)(l->word - l->row * ww) * 64 + l->lane;
    return true;
}

// member [256]: 1 for the labels the step names.  ctr [kCcCounters] of the step, zero on entry.
__global__ __launch_bounds__(256) void cc_mask_init(const uint8_t* __restrict__ seg, const uint8_t* __restrict__ member, int W, long long words,
                                                    cc_word* __restrict__ bits, int* __restrict__ parent, int* __restrict__ count, int* __restrict__ ctr) {
    const int ww = (W + 63) >> 6;
    CcLane l;
    if (!cc_lane(words, ww, &l)) return;
    const bool inside = l.x < W;
    const int i = inside ? (int)(l.row * W + l.x) : 0;
    const bool in = inside && member[seg[i]];
    const cc_word m = __ballot(in);
    if (inside) {
        parent[i] = in ? i - l.lane + cc_run_start(m, l.lane) : -1;
        count[i] = 0;
    }
    if (l.lane == 0) {
        bits[l.word] = m;
        if (m) atomicAdd(ctr, __popcll(m));
    }
}

__global__ __launch_bounds__(256) void cc_link(const cc_word* __restrict__ bits, int* parent, int H, int W, long long words, int* __restrict__ status) {
    const int ww = (W + 63) >> 6;
    CcLane l;
    if (!cc_lane(words, ww, &l)) return;
    if (!(bits[l.word] >> l.lane & 1)) return;
    int gave_up = 0;
    cc_link_voxel(parent, bits, H, W, ww, (int)(l.row / H), (int)(l.row % H), l.x, kCcFindCap, kCcUnionCap, &gave_up);
    if (gave_up) atomicOr(status, kCcStatusGiveUp);
}

// (Only lane i writes parent[i] here, with a value found by walking down from it: the chains other lanes walk meanwhile stay decreasing.)
__global__ __launch_bounds__(256) void cc_flatten(int* parent, int W, long long words, int* __restrict__ ctr, int* __restrict__ status) {
    const int ww = (W + 63) >> 6;
    CcLane l;
    if (!cc_lane(words, ww, &l)) return;
    bool root = false;
    if (l.x < W) {
        const int i = (int)(l.row * W + l.x);
        if (cc_load(parent + i) >= 0) {
            int gave_up = 0;
            const int r = cc_find(parent, i, kCcFindCap, &gave_up);
            if (gave_up) atomicOr(status, kCcStatusGiveUp);
            else {
                __hip_atomic_store(parent + i, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                root = r == i;
            }
        }
    }
    const int n = __popcll(__ballot(root));
    if (l.lane == 0 && n) atomicAdd(ctr + 1, n);
}

__global__ __launch_bounds__(256) void cc_count(const int* __restrict__ parent, int W, long long words, int* __restrict__ count) {
    const int ww = (W + 63) >> 6;
    CcLane l;
    if (!cc_lane(words, ww, &l)) return;
    const int p = l.x < W ? parent[(int)(l.row * W + l.x)] : -1;
    const cc_word m = __ballot(p >= 0);
    if (p >= 0 && (l.lane == 0 || !(m >> (l.lane - 1) & 1))) atomicAdd(count + p, cc_run_length(m, l.lane));
}

__global__ __launch_bounds__(256) void cc_max(const int* __restrict__ parent, const int* __restrict__ count, int W, long long words, int* __restrict__ ctr) {
    const int ww = (W + 63) >> 6;
    CcLane l;
    if (!cc_lane(words, ww, &l)) return;
    int v = 0;
    if (l.x < W) {
        const int i = (int)(l.row * W + l.x);
        if (parent[i] == i) v = count[i];
    }
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) v = max(v, __shfl_xor(v, s));
    if (l.lane == 0 && v > 0) atomicMax(ctr + 2, v);
}

__global__ __launch_bounds__(256) void cc_apply(uint8_t* __restrict__ seg, const int* __restrict__ parent, const int* __restrict__ count, int W,
                                                long long words, uint8_t background, int* __restrict__ ctr, const int* __restrict__ status) {
    const int ww = (W + 63) >> 6;
    CcLane l;
    if (!cc_lane(words, ww, &l)) return;
    bool kill = false;
    if (l.x < W && !*status) {
        const int i = (int)(l.row * W + l.x), p = parent[i];
        if (p >= 0 && count[p] < ctr[2]) {
            seg[i] = background;
            kill = true;
        }
    }
    const int n = __popcll(__ballot(kill));
    if (l.lane == 0 && n) atomicAdd(ctr + 3, n);
}

}  // namespace ts2d
