// The connected components of EVERY label of a segmentation at once, behind ts2d_label_components (post.hip): per label the voxels, the components,
// the largest size, and a clean-up rule - keep the largest, drop what is below a size - applied to every label in the same launches.
// components.label_components_statement is the definition (scipy.ndimage.label per label, np.bincount); these kernels give its bytes.
//
// Sets.  The labelling runs on SETS of Z H W voxels: a label map is ONE set whose class array holds the label index + 1 (through a 256-entry table built
// from the caller's values) or 0; planes are one set per label with classes in {0, 1}.  cls, parent and count are indexed LOCALLY inside a set (int32:
// the entry refuses more than 2^31 - 1 voxels, whatever K is) and a kernel reaches its set through blockIdx.y alone: no index can name a voxel of
// another set, so plane k and plane k + 1 never join.  Inside a set two voxels join iff their classes are equal and not 0 (cc_label.h:
// cc_link_voxel_classes), so two labels that touch in a label map never join either.  Per voxel of a set: cls 1 byte, parent 4, count 4, and one bit of
// the word `eq` ("has a class and the voxel before it in the word has the same one"), which spells the runs of equal class for every later launch.
//     lc_init      classes, eq words, parents (the first voxel of the voxel's run inside its word: a run along x costs no atomic), count <- 0, and the
//                  voxels per label: one integer add per run of equal class (label map) or per word (planes)
//     lc_link      every voxel with a class joins the earlier neighbours of its class: 13 under full connectivity, 3 under faces
//     lc_flatten   parent[i] <- the root above i; the roots are counted per label: the components
//     lc_count     count[root] += the voxels of every run, one integer atomicAdd per run (the lanes of a run share their root)
//     lc_max       per label the largest count: an integer atomicMax by the root lanes
//     lc_apply     a component of size s of label k goes iff (keep_largest and s < largest_k) or s < min_voxels[k]: its voxels become 0 in the
//                  segmentation; voxels removed (one add per run) and components removed (by the root lanes) are counted per label
//     lc_list      every root appends (label, root, count) through ONE integer cursor, and writes only while its slot is below the capacity
// Every kernel runs one WAVE per 64-voxel word with CcLane's addressing (kernels_post_cc.h): grid = (ceil(Z H ceil(W / 64) / 4), sets), 256 lanes,
// folded along z where it passes 2^32 threads.
//
// Termination and order: the arguments of kernels_post_cc.h hold unchanged.  The only loops are cc_find and cc_union, bounded by monotonicity AND a hard
// cap; a lane at a cap ORs kLcStatusGiveUp into the status, lc_apply and lc_list write nothing once it is set, and the entry leaves the caller's
// buffers alone.  No lane waits for another.  Integer atomics (min, add, max, or), relaxed loads and plain vector stores only; no inline assembly, no
// LDS, no floating point.  The edges are a fixed set, the partition they generate is unique, a root is the MINIMUM index of its component, sizes and
// maxima are integers and ties are kept: every output is a function of the input but the ORDER of the list, which the entry sorts on the host.
#pragma once
#include <hip/hip_runtime.h>

#include "kernels_post_cc.h"    // CcLane, cc_lane; cc_label.h behind it

namespace ts2d {

constexpr int kLcStatusGiveUp = 1;       // TS2D_COMP_GIVE_UP
constexpr int kLcStatusListFull = 2;     // TS2D_COMP_LIST_FULL (set by the entry, on the host)
constexpr int kLcCounters = 5;           // per label: voxels, components, largest size, voxels removed, components removed
constexpr int kLcPlanes = 0, kLcLabelMap = 1;      // TS2D_STATS_PLANES, TS2D_STATS_LABELMAP
constexpr int kLcFull = 0, kLcFaces = 1;           // TS2D_COMP_FULL, TS2D_COMP_FACES

// The state of the sets that work at once, each array [sets][n] (eq: [sets][words]); k0: the label of set 0 (planes).
struct LcState {
    uint8_t* cls;
    cc_word* eq;
    int* parent;
    int* count;
    long long n, words;
    int W, kind, k0;
};

// where the lane stands: its set's arrays, the voxel's local index i (valid iff inside) and the label of class c there
struct LcLane {
    CcLane l;
    uint8_t* cls;
    cc_word* eq;
    int* parent;
    int* count;
    int i;
    bool inside;
};
__device__ __forceinline__ bool lc_lane(const LcState& s, LcLane* a) {
    if (!cc_lane(s.words, (s.W + 63) >> 6, &a->l)) return false;
    const size_t set = blockIdx.y;
    a->cls = s.cls + set * (size_t)s.n;
    a->eq = s.eq + set * (size_t)s.words;
    a->parent = s.parent + set * (size_t)s.n;
    a->count = s.count + set * (size_t)s.n;
    a->inside = a->l.x < s.W;
    a->i = a->inside ? (int)(a->l.row * s.W + a->l.x) : 0;
    return true;
}
__device__ __forceinline__ int lc_label(const LcState& s, uint8_t c) { return s.kind == kLcLabelMap ? (int)c - 1 : s.k0 + (int)blockIdx.y; }

// seg: the caller's segmentation on the device, [n] (label map) or [K][n] (planes).  table [256]: the class of a label-map value.  ctr [K][kLcCounters].
__global__ __launch_bounds__(256) void lc_init(const uint8_t* __restrict__ seg, const uint8_t* __restrict__ table, LcState s, int* __restrict__ ctr) {
    LcLane a;
    if (!lc_lane(s, &a)) return;
    int c = 0;
    if (a.inside) c = s.kind == kLcLabelMap ? table[seg[a.i]] : seg[(size_t)(s.k0 + (int)blockIdx.y) * (size_t)s.n + a.i] > 0;
    const int before = __shfl_up(c, 1);
    const int lane = a.l.lane;
    const cc_word eq = __ballot(c != 0 && lane > 0 && before == c);
    if (a.inside) {
        a.cls[a.i] = (uint8_t)c;
        a.parent[a.i] = c ? a.i - lane + cc_class_run_start(eq, lane) : -1;
        a.count[a.i] = 0;
    }
    if (lane == 0) a.eq[a.l.word] = eq;
    if (s.kind == kLcLabelMap) {
        if (c && !(eq >> lane & 1)) atomicAdd(ctr + lc_label(s, (uint8_t)c) * kLcCounters, cc_class_run_length(eq, lane));
    } else {
        const int n = __popcll(__ballot(c != 0));
        if (lane == 0 && n) atomicAdd(ctr + lc_label(s, 1) * kLcCounters, n);
    }
}

__global__ __launch_bounds__(256) void lc_link(LcState s, int H, int faces, int* __restrict__ status) {
    LcLane a;
    if (!lc_lane(s, &a)) return;
    if (!a.inside || !a.cls[a.i]) return;
    int gave_up = 0;
    cc_link_voxel_classes(a.parent, a.cls, H, s.W, (int)(a.l.row / H), (int)(a.l.row % H), a.l.x, faces, kCcFindCap, kCcUnionCap, &gave_up);
    if (gave_up) atomicOr(status, kLcStatusGiveUp);
}

// (Only lane i writes parent[i] here, with a value found by walking down from it: the chains other lanes walk meanwhile stay decreasing.)
__global__ __launch_bounds__(256) void lc_flatten(LcState s, int* __restrict__ ctr, int* __restrict__ status) {
    LcLane a;
    if (!lc_lane(s, &a)) return;
    bool root = false;
    if (a.inside && cc_load(a.parent + a.i) >= 0) {
        int gave_up = 0;
        const int r = cc_find(a.parent, a.i, kCcFindCap, &gave_up);
        if (gave_up) atomicOr(status, kLcStatusGiveUp);
        else {
            __hip_atomic_store(a.parent + a.i, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            root = r == a.i;
        }
    }
    if (s.kind == kLcLabelMap) {
        if (root) atomicAdd(ctr + lc_label(s, a.cls[a.i]) * kLcCounters + 1, 1);
    } else {
        const int n = __popcll(__ballot(root));
        if (a.l.lane == 0 && n) atomicAdd(ctr + lc_label(s, 1) * kLcCounters + 1, n);
    }
}

__global__ __launch_bounds__(256) void lc_count(LcState s) {
    LcLane a;
    if (!lc_lane(s, &a)) return;
    const int p = a.inside ? a.parent[a.i] : -1;
    const cc_word eq = a.eq[a.l.word];
    if (p >= 0 && !(eq >> a.l.lane & 1)) atomicAdd(a.count + p, cc_class_run_length(eq, a.l.lane));
}

__global__ __launch_bounds__(256) void lc_max(LcState s, int* __restrict__ ctr) {
    LcLane a;
    if (!lc_lane(s, &a)) return;
    if (a.inside && a.parent[a.i] == a.i) atomicMax(ctr + lc_label(s, a.cls[a.i]) * kLcCounters + 2, a.count[a.i]);
}

// seg is changed in place.  min_voxels [K] (never NULL: zeros where the caller gave none).
__global__ __launch_bounds__(256) void lc_apply(uint8_t* __restrict__ seg, LcState s, int keep_largest, const long long* __restrict__ min_voxels,
                                                int* __restrict__ ctr, const int* __restrict__ status) {
    LcLane a;
    if (!lc_lane(s, &a)) return;
    if (!a.inside || *status) return;
    const int p = a.parent[a.i];
    if (p < 0) return;
    const int k = lc_label(s, a.cls[a.i]), size = a.count[p];
    if (!((keep_largest && size < ctr[k * kLcCounters + 2]) || (long long)size < min_voxels[k])) return;
    seg[(s.kind == kLcLabelMap ? (size_t)0 : (size_t)k * (size_t)s.n) + a.i] = 0;
    const cc_word eq = a.eq[a.l.word];
    if (!(eq >> a.l.lane & 1)) atomicAdd(ctr + k * kLcCounters + 3, cc_class_run_length(eq, a.l.lane));
    if (p == a.i) atomicAdd(ctr + k * kLcCounters + 4, 1);
}

// list [capacity][3] int32: (label, root, count).  *cursor counts every root, those past the capacity included.
__global__ __launch_bounds__(256) void lc_list(LcState s, int* __restrict__ list, unsigned long long capacity, unsigned long long* __restrict__ cursor,
                                               const int* __restrict__ status) {
    LcLane a;
    if (!lc_lane(s, &a)) return;
    if (!a.inside || *status || a.parent[a.i] != a.i) return;
    const unsigned long long slot = atomicAdd(cursor, 1ull);
    if (slot >= capacity) return;
    int* const e = list + slot * 3;
    e[0] = lc_label(s, a.cls[a.i]);
    e[1] = a.i;
    e[2] = a.count[a.i];
}

}  // namespace ts2d
