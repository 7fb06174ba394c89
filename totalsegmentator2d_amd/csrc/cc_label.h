// The label-equivalence routines of the connected-component kernels (kernels_post_cc.h): find, union, the run of a voxel inside its 64-bit
// word, and the links of one voxel to its 13 "earlier" neighbours under full connectivity.  Their own header, host and device:
// tests/test_postprocess_cpu.py compiles it as plain C++ - the atomics become plain single-threaded operations - and holds the partition
// it builds against scipy's on hundreds of volumes.
//
// The forest.  parent[i] is -1 outside the mask and an index of the SAME component, never above i, inside it; a root has parent[i] == i.
// Every write is an integer minimum (cc_min) or a store of a value found by walking down, so parents only decrease and parent[x] <= x
// holds throughout.  Hence
//     cc_find   walks a strictly decreasing chain: it ends at a root after at most x steps;
//     cc_union  lowers parent[a] of the larger root a to the smaller root b.  If another lane got there first (the minimum returns an
//               old value other than a), that old value is below a, and the loop goes on from it: the pair (a, b) drops strictly in
//               every round that does not finish.  The minimum may have replaced old by b at a voxel that was no root any more - a is
//               then cut from old - and the next round, union(old, b), is what joins them again: no link is ever lost for good.
// Both loops also carry a HARD CAP beside the monotonicity argument; a lane that reaches it sets *gave_up and returns, nothing waits.
// A read may be stale.  It still names a voxel that was an ancestor, i.e. of the same final component, and the chain below it is as
// decreasing as any: staleness costs steps, never the result.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define TS2D_CC_HD __host__ __device__ __forceinline__
#else
#define TS2D_CC_HD inline
#endif

namespace ts2d {

typedef unsigned long long cc_word;      // 64 voxels of a row along x: bit k of word w is voxel 64 w + k (prep_word of kernels_prep_fill.h)

constexpr int kCcFindCap = 1 << 15;      // steps of one cc_find.  A chain is as deep as roots were hung under roots before anything flattened
                                         // it: on the host build 3 steps on a 4 x 32 x 32 one-voxel serpentine linked in index order, 73 in reverse
constexpr int kCcUnionCap = 1 << 10;     // rounds of one cc_union: each round but the last lost a race for the same root

TS2D_CC_HD int cc_load(const int* p) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#else
    return *p;
#endif
}

// *p = min(*p, v); the value it displaced
TS2D_CC_HD int cc_min(int* p, int v) {
#if defined(__HIP_DEVICE_COMPILE__)
    return atomicMin(p, v);
#else
    const int old = *p;
    if (v < old) *p = v;
    return old;
#endif
}

// the root above mask voxel x.  (A parent outside [0, x] cannot arise; it is treated like the cap so that no index ever leaves the array.)
TS2D_CC_HD int cc_find(const int* parent, int x, int cap, int* gave_up) {
    for (int k = 0; k < cap; ++k) {
        const int p = cc_load(parent + x);
        if (p == x) return x;
        if (p < 0 || p > x) break;
        x = p;
    }
    *gave_up = 1;
    return x;
}

// join the components of mask voxels a and b
TS2D_CC_HD void cc_union(int* parent, int a, int b, int find_cap, int union_cap, int* gave_up) {
    for (int k = 0; k < union_cap; ++k) {
        a = cc_find(parent, a, find_cap, gave_up);
        b = cc_find(parent, b, find_cap, gave_up);
        if (*gave_up || a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = cc_min(parent + a, b);
        if (old == a) return;            // a was still a root: it hangs under b now
        a = old;                         // (old < a) someone else lowered it first; join what it pointed to with b
    }
    *gave_up = 1;
}

// is voxel x of the row whose words start at `row` in the mask?  Outside 0 ... W - 1: no.
TS2D_CC_HD bool cc_bit(const cc_word* row, int W, int x) { return x >= 0 && x < W && (row[x >> 6] >> (x & 63) & 1); }

// bit `lane` of m is set: the lowest bit of the run of ones it lies in, and how many ones follow from `lane` on (itself included)
TS2D_CC_HD int cc_run_start(cc_word m, int lane) {
    const cc_word below = ~m & ((1ull << lane) - 1);
    return below ? 64 - __builtin_clzll(below) : 0;
}
TS2D_CC_HD int cc_run_length(cc_word m, int lane) {
    const cc_word t = ~(m >> lane);
    return t ? __builtin_ctzll(t) : 64;
}

// The links of mask voxel (z, y, x) of a [Z][H][W] volume to the 13 neighbours that lie before it in index order.  bits [Z H][ww], ww = ceil(W / 64).
// The initial parent of a voxel is the start of its run INSIDE its word (cc_run_start), so along x only a run that crosses a word end needs a link.
// Towards each of the four earlier rows - (dz, dy) = (0, -1), (-1, -1), (-1, 0), (-1, +1) - a voxel links straight down where the row has a voxel,
// else diagonally; a link that the voxel to its left or right makes for the same pair of runs is left to that voxel:
//     straight, and the left neighbour is in the mask with a voxel below it too   the two runs overlap further left: the first voxel of the overlap links
//     diagonal to the left, and the left neighbour is in the mask                 that neighbour has the voxel straight below it
//     diagonal to the right, and the right neighbour is in the mask               likewise
TS2D_CC_HD void cc_link_voxel(int* parent, const cc_word* bits, int H, int W, int ww, int z, int y, int x, int find_cap, int union_cap, int* gave_up) {
    const long long row = (long long)z * H + y;
    const cc_word* me = bits + row * ww;
    const int i = (int)(row * W + x);
    const bool left = cc_bit(me, W, x - 1), right = cc_bit(me, W, x + 1);
    if (left && (x & 63) == 0) cc_union(parent, i, i - 1, find_cap, union_cap, gave_up);
    for (int k = 0; k < 4; ++k) {
        const int zz = z - (k > 0), yy = y + (k == 0 ? -1 : k - 2);
        if (zz < 0 || yy < 0 || yy >= H) continue;
        const long long nrow = (long long)zz * H + yy;
        const cc_word* nb = bits + nrow * ww;
        const int j = (int)(nrow * W + x);
        const bool c = cc_bit(nb, W, x), l = cc_bit(nb, W, x - 1), r = cc_bit(nb, W, x + 1);
        if (c) {
            if (!(left && l)) cc_union(parent, i, j, find_cap, union_cap, gave_up);
        } else {
            if (l && !left) cc_union(parent, i, j - 1, find_cap, union_cap, gave_up);
            if (r && !right) cc_union(parent, i, j + 1, find_cap, union_cap, gave_up);
        }
    }
}

// ---- every label at once (kernels_components.h): the same forest, linked by CLASS EQUALITY in place of mask membership.
// cls [Z H W] holds 0 outside every label and the voxel's class (1 ... 255) inside; two voxels may join iff their classes are equal and not 0.
// "Has my class" is an equivalence on a row, so a row falls into maximal runs of equal class exactly as a mask falls into runs of ones, and every
// rule of cc_link_voxel holds with "is in the mask" read as "has my class".

// does voxel x of the row `row` have the non-zero class c?  Outside 0 ... W - 1: no.
TS2D_CC_HD bool cc_same(const uint8_t* row, int W, int x, uint8_t c) { return x >= 0 && x < W && row[x] == c; }

// eq: bit l is set iff voxel l of the word has a non-zero class AND voxel l - 1 of the SAME word has the same one (bit 0 is never set).  The voxel at
// `lane` has a class: the first voxel of its run of equal class inside the word, and how many voxels the run has from `lane` on (itself included).
TS2D_CC_HD int cc_class_run_start(cc_word eq, int lane) { return (eq >> lane & 1) ? cc_run_start(eq, lane) - 1 : lane; }
TS2D_CC_HD int cc_class_run_length(cc_word eq, int lane) { return lane < 63 ? 1 + cc_run_length(eq, lane + 1) : 1; }

// The links of voxel (z, y, x), of class cls[.] != 0, to the earlier neighbours of its own class.  The initial parent of a voxel is the start of its run
// of equal class inside its 64-voxel word (cc_class_run_start), so along x only a run that crosses a word end needs a link.
//     faces == 0  the 13 earlier neighbours of full connectivity, with the three de-duplication rules of cc_link_voxel
//     faces != 0  x - 1 (at a word start), (y - 1, x) and (z - 1, y, x) only; of the rules only "straight, and the left neighbour has my class with one
//                 of my class below it too" applies - the two runs overlap further left and the first voxel of the overlap links
TS2D_CC_HD void cc_link_voxel_classes(int* parent, const uint8_t* cls, int H, int W, int z, int y, int x, int faces, int find_cap, int union_cap,
                                      int* gave_up) {
    const long long row = (long long)z * H + y;
    const uint8_t* me = cls + row * W;
    const uint8_t c = me[x];
    const int i = (int)(row * W + x);
    const bool left = cc_same(me, W, x - 1, c), right = cc_same(me, W, x + 1, c);
    if (left && (x & 63) == 0) cc_union(parent, i, i - 1, find_cap, union_cap, gave_up);
    for (int k = 0; k < 4; ++k) {
        if (faces && (k & 1)) continue;          // (dz, dy) = (-1, -1) and (-1, +1) are no face neighbours
        const int zz = z - (k > 0), yy = y + (k == 0 ? -1 : k - 2);
        if (zz < 0 || yy < 0 || yy >= H) continue;
        const long long nrow = (long long)zz * H + yy;
        const uint8_t* nb = cls + nrow * W;
        const int j = (int)(nrow * W + x);
        if (cc_same(nb, W, x, c)) {
            if (!(left && cc_same(nb, W, x - 1, c))) cc_union(parent, i, j, find_cap, union_cap, gave_up);
        } else if (!faces) {
            if (!left && cc_same(nb, W, x - 1, c)) cc_union(parent, i, j - 1, find_cap, union_cap, gave_up);
            if (!right && cc_same(nb, W, x + 1, c)) cc_union(parent, i, j + 1, find_cap, union_cap, gave_up);
        }
    }
}

}  // namespace ts2d
