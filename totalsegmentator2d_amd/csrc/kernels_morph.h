// Grow, shrink, open and close every label of a segmentation by a radius in mm, behind ts2d_label_morphology (morph.hip).  The arithmetic, the
// table that carries every floating-point decision and the proof of the scan form: morph.h; the definition: morphology.label_morphology_statement.
// The kernels hold no floating-point number.
//
// The labels of a call that were selected are worked in chunks (MoChunk: the chunk's labels by their index k, in increasing k); slot j of a chunk
// has per pixel 2 bytes of g, 1 byte of the intermediate plane (open and close) and 1 byte of result plane (label maps).
//     mo_before    per label the pixels of the INPUT (every label, selected or not)
//     mo_columns   a lane per column, adjacent lanes on adjacent columns: two scans over the rows write g, capped at the table's length
//     mo_rows      the hot path: ONE WAVE per row and label walks the row in 64-pixel chunks, left to right for the prefix maximum of x' + cover[g]
//                  and right to left for the suffix minimum of x' - cover[g], each by six cross-lane steps and a carried value.  The first walk
//                  leaves "covered from the left" in the destination byte, which the SAME lane reads back in the second walk.  The last step of
//                  planes writes the output bytes and counts added and removed pixels: one integer atomicAdd per row and counter.
//     mo_compose   label maps: one lane owns a pixel and walks the chunk's labels in the order of `values`; chunks are launched in that order too,
//                  so the first label wins whatever the arrival order.  A growing operation paints samples equal to 0 only; a shrinking one clears
//                  the pixels of a label that its result does not hold.
// cover is read through the cache (at most 64 KiB, the same few entries for neighbouring pixels), not staged in LDS.
// Every loop is bounded by an extent, the chunk's labels or the 64 lanes; no lane waits for another; integer atomic adds and plain vector stores only.
#pragma once
#include <hip/hip_runtime.h>

#include "morph.h"

namespace ts2d {

constexpr int kMoCtr = 3;                // per label on the device: before, added, removed (after = before + added - removed: the entry)
enum { kMoSrcPlanes = 0, kMoSrcLabelMap = 1, kMoSrcSlots = 2 };      // what mo_columns reads: the caller's planes [K][n], label map [n], or slots [L][n]

struct MoChunk {
    const int* sel;            // the labels of the chunk, `count` of them
    const uint8_t* values;     // [K]: the value of a label in a label map
    int count;
    long long n;               // H * W
    int H, W;
};

__device__ __forceinline__ int mo_wave_prefix_max(int v, int lane) {
    for (int d = 1; d < 64; d <<= 1) {
        const int o = __shfl_up(v, d);
        if (lane >= d) v = o > v ? o : v;
    }
    return v;
}
__device__ __forceinline__ int mo_wave_suffix_min(int v, int lane) {
    for (int d = 1; d < 64; d <<= 1) {
        const int o = __shfl_down(v, d);
        if (lane + d < 64) v = o < v ? o : v;
    }
    return v;
}

// ctr[label * kMoCtr + slot] += the lanes of the wave that name `label` (-1: none).  Every lane of the wave calls it; at most 64 rounds, each of
// which takes all lanes of one label off the list.
__device__ __forceinline__ void mo_count_by_label(int label, int* __restrict__ ctr, int slot, int lane) {
    unsigned long long todo = __ballot(label >= 0);
    for (int round = 0; round < 64 && todo; ++round) {
        const int first = __ffsll((long long)todo) - 1;
        const int l = __shfl(label, first);
        const unsigned long long same = __ballot(label == l);
        if (lane == first) atomicAdd(ctr + l * kMoCtr + slot, __popcll(same));
        todo &= ~same;
    }
}

// table [256]: label index + 1 of a label-map value, 0 for a value that names no label.  grid (ceil(n / 256), planes: K, label map: 1)
__global__ __launch_bounds__(256) void mo_before(const uint8_t* __restrict__ seg, int kind, const uint8_t* __restrict__ table, long long n,
                                                 int* __restrict__ ctr) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const int lane = threadIdx.x & 63;
    if (kind == kStLabelMap) {
        mo_count_by_label(i < n ? (int)table[seg[i]] - 1 : -1, ctr, 0, lane);
    } else {
        const int k = blockIdx.y;
        const int c = __popcll(__ballot(i < n && seg[(size_t)k * (size_t)n + i] > 0));
        if (lane == 0 && c) atomicAdd(ctr + k * kMoCtr, c);
    }
}

// grid (ceil(W / 64), the chunk's labels), 64 lanes.  g [count][n]
__global__ __launch_bounds__(64) void mo_columns(MoChunk ch, const uint8_t* __restrict__ src, int src_mode, int complement, int T,
                                                 uint16_t* __restrict__ g) {
    const int x = blockIdx.x * 64 + threadIdx.x;
    if (x >= ch.W) return;
    const int j = blockIdx.y, k = ch.sel[j];
    const size_t plane = src_mode == kMoSrcPlanes ? (size_t)k * (size_t)ch.n : src_mode == kMoSrcSlots ? (size_t)j * (size_t)ch.n : 0;
    const int kind = src_mode == kMoSrcLabelMap ? (int)kStLabelMap : (int)kStPlanes;
    const uint8_t value = src_mode == kMoSrcLabelMap ? ch.values[k] : (uint8_t)0;
    const uint8_t* const s = src + plane + x;
    uint16_t* const gc = g + (size_t)j * (size_t)ch.n + x;
    int last = -1;
    for (int y = 0; y < ch.H; ++y) {
        if (mo_member(s[(size_t)y * ch.W], kind, value, complement != 0)) last = y;
        gc[(size_t)y * ch.W] = mo_g(last < 0 ? -1 : y - last, T);
    }
    last = -1;
    for (int y = ch.H - 1; y >= 0; --y) {
        if (mo_member(s[(size_t)y * ch.W], kind, value, complement != 0)) last = y;
        const uint16_t d = mo_g(last < 0 ? -1 : last - y, T);
        const uint16_t before = gc[(size_t)y * ch.W];
        gc[(size_t)y * ch.W] = d < before ? d : before;
    }
}

// grid (ceil(H / 4), the chunk's labels), 256 lanes: wave w of a block walks row 4 * blockIdx.x + w.  dst [.][n] is indexed by the label where
// dst_by_label, else by the slot.  FINAL_PLANES: dst is the output planes, seg the caller's planes, and added / removed are counted into ctr; else
// dst receives 1 / 0.
template <bool FINAL_PLANES>
__global__ __launch_bounds__(256) void mo_rows(MoChunk ch, const uint16_t* __restrict__ g, const uint16_t* __restrict__ cover, int T, int erodes,
                                               uint8_t* __restrict__ dst, int dst_by_label, const uint8_t* __restrict__ seg, int* __restrict__ ctr) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= ch.H) return;                                        // the whole wave leaves
    const int j = blockIdx.y, k = ch.sel[j], W = ch.W;
    const size_t at = (size_t)row * W;
    const uint16_t* const gr = g + (size_t)j * (size_t)ch.n + at;
    uint8_t* const d = dst + (size_t)(dst_by_label ? k : j) * (size_t)ch.n + at;
    const int chunks = (W + 63) >> 6;
    int carry = kMoNoReach;
    for (int c = 0; c < chunks; ++c) {
        const int x = c * 64 + lane;
        int v = x < W ? mo_reach_right(cover, T, gr[x], x) : kMoNoReach;
        v = mo_wave_prefix_max(v, lane);
        v = v > carry ? v : carry;
        carry = __shfl(v, 63);
        if (x < W) d[x] = v >= x ? 1 : 0;
    }
    carry = kMoFar;
    int added = 0, removed = 0;
    for (int c = chunks - 1; c >= 0; --c) {
        const int x = c * 64 + lane;
        int v = x < W ? mo_reach_left(cover, T, gr[x], x) : kMoFar;
        v = mo_wave_suffix_min(v, lane);
        v = v < carry ? v : carry;
        carry = __shfl(v, 0);
        const bool in = x < W;
        const bool after = in && ((d[in ? x : 0] != 0 || v <= x) != (erodes != 0));
        if (FINAL_PLANES) {
            const uint8_t sb = in ? seg[(size_t)k * (size_t)ch.n + at + x] : (uint8_t)0;
            if (in) d[x] = mo_plane_byte(sb, after);
            added += __popcll(__ballot(after && !sb));
            removed += __popcll(__ballot(in && sb && !after));
        } else if (in) {
            d[x] = after ? 1 : 0;
        }
    }
    if (FINAL_PLANES && lane == 0) {
        if (added) atomicAdd(ctr + k * kMoCtr + 1, added);
        if (removed) atomicAdd(ctr + k * kMoCtr + 2, removed);
    }
}

// seg: the caller's label map [n]; out: the map being built [n] (a copy of seg before the first chunk); res [count][n].  grid ceil(n / 256)
__global__ __launch_bounds__(256) void mo_compose(MoChunk ch, const uint8_t* __restrict__ seg, const uint8_t* __restrict__ res, int grows,
                                                  uint8_t* __restrict__ out, int* __restrict__ ctr) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    int label = -1;
    if (i < ch.n) {
        if (grows) {
            if (out[i] == 0)
                for (int j = 0; j < ch.count; ++j)
                    if (res[(size_t)j * (size_t)ch.n + i]) {
                        label = ch.sel[j];
                        out[i] = ch.values[label];
                        break;
                    }
        } else {
            const uint8_t v = seg[i];
            for (int j = 0; v && j < ch.count; ++j)
                if (ch.values[ch.sel[j]] == v) {
                    if (!res[(size_t)j * (size_t)ch.n + i]) {
                        label = ch.sel[j];
                        out[i] = 0;
                    }
                    break;
                }
        }
    }
    mo_count_by_label(label, ctr, grows ? 1 : 2, threadIdx.x & 63);
}

}  // namespace ts2d
