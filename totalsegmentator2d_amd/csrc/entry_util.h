// What the entries that need no engine (prep.hip, post.hip, visual.hip, stats.hip, evaluate.hip, morph.hip, ts2d_probabilities_from_logits) share of
// their call scaffolding: the layout of a call's one DevMem, the strided-view check, the sample types, the label side of a call and the size of
// a chunk of labels.  Host only and free of HIP: plain C++ includes it, and tests/test_entry_util_cpu.py compiles it behind a main of its own.
#pragma once
#include "../../include/ts2d_engine.h"

#include <cstddef>
#include <cstdint>
#include <cstdio>

#pragma GCC visibility push(hidden)
namespace ts2d {

int fail(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));      // program.cpp (as engine_internal.h declares it)

// The regions of one device allocation, in the order they are added: add() gives a region's offset, a multiple of 256, and total() the bytes to
// allocate.  An offset is never restated: a region's end is the next one's start, so two regions cannot overlap; a zero-byte region takes no room.
class ArenaLayout {
public:
    size_t add(size_t bytes) { const size_t at = total_; total_ = (at + bytes + 255) / 256 * 256; return at; }
    size_t total() const { return total_; }
private:
    size_t total_ = 0;
};

// Every element a view of `extents` elements at element `strides` from element `base` can touch lies inside a buffer of n_elems: its lowest
// and highest index are 0 <= lo and hi < n_elems.  named = false: the wording ts2d_project_coronal had before the view's parts were named.
inline int check_strided_view(const char* entry, size_t n_elems, long long base, const int (&extents)[3], const long long (&strides)[3],
                              bool named = true) {
    long long lo = base, hi = base;
    for (int k = 0; k < 3; ++k) {
        const long long ext = (long long)(extents[k] - 1) * strides[k];
        if (ext < 0) lo += ext; else hi += ext;
    }
    if (lo >= 0 && hi < (long long)n_elems) return TS2D_OK;
    char of[48] = "";
    if (named) snprintf(of, sizeof(of), " of n_elems %zu", n_elems);
    return fail(TS2D_ERR_INVALID, "%s: the strided view%s leaves the buffer%s", entry, named ? " (base, sz, sy, sx)" : "", of);
}

// The sample types of a volume or plane, by the dtype code of the C header: 0 int16, 1 uint8, 2 float32, 3 uint16, 4 int32.
inline size_t sample_size(int dtype) { static const int esize[5] = {2, 1, 4, 2, 4}; return (size_t)esize[dtype]; }
template <int DT, class T> struct SampleType { static constexpr int dtype = DT; using type = T; };
template <class F>
auto by_sample_type(int dtype, F&& f) {      // f(SampleType<dtype, its C type>{}) for a dtype in 0 ... 4
    switch (dtype) {
        case 0: return f(SampleType<0, int16_t>{});
        case 1: return f(SampleType<1, uint8_t>{});
        case 2: return f(SampleType<2, float>{});
        case 3: return f(SampleType<3, uint16_t>{});
        default: return f(SampleType<4, int32_t>{});
    }
}

// The label side of a call (the kinds by their numbers in the C header; for the kernels, and who belongs to a label: stats_tree.h).
inline bool label_kind(int kind) { return kind == TS2D_STATS_PLANES || kind == TS2D_STATS_LABELMAP; }
inline int check_label_count(const char* entry, int K) {
    return K < 1 || K > 255 ? fail(TS2D_ERR_INVALID, "%s: K = %d labels outside 1 ... 255", entry, K) : TS2D_OK;
}
// ... of a label map: the values of its K labels, none of them the background
inline int check_label_values(const char* entry, const uint8_t* values, int K) {
    if (!values) return fail(TS2D_ERR_INVALID, "%s: a label map needs the values of its K labels", entry);
    for (int k = 0; k < K; ++k)
        if (values[k] == 0) return fail(TS2D_ERR_INVALID, "%s: values[%d] = 0 is the background, not a label", entry, k);
    return TS2D_OK;
}

// Z x H x W samples, each extent at least 1, are indexed by an int32, and so are the Z * H rows.
inline bool volume_fits_int32(int Z, int H, int W) {
    return Z >= 1 && H >= 1 && W >= 1 && (long long)Z * H <= 0x7FFFFFFFll && (long long)Z * H * W <= 0x7FFFFFFFll;
}

// One axis of a dispatch counts its work-items in 32 bits, and the runtime does not refuse a launch beyond them: the count wraps and only a part of
// the grid runs.  `blocks` workgroups of `threads` lanes along x are therefore FOLDED: x workgroups along x (x * threads < 2^32), `fold` times along
// an axis the kernel does not use otherwise; the workgroup's number is fold index * gridDim.x + blockIdx.x, and a kernel leaves where that number
// reaches `blocks` (x * fold >= blocks).  fold == 1 and x == blocks wherever blocks * threads < 2^32: the launch of before.
struct FoldedGrid {
    unsigned x, fold;
};
inline FoldedGrid fold_grid(long long blocks, int threads) {
    const long long cap = 0xFFFFFFFFll / threads;
    if (blocks <= cap) return {(unsigned)blocks, 1u};
    const long long fold = (blocks + cap - 1) / cap;
    return {(unsigned)((blocks + fold - 1) / fold), (unsigned)fold};
}

// The labels of one chunk: as many as have their scratch of per_label bytes under max_scratch_bytes (0: 256 MiB; *budget: what was used), at
// most K.  0: ONE label does not fit - the entry refuses in its own words.
inline size_t labels_per_chunk(size_t max_scratch_bytes, size_t per_label, int K, size_t* budget) {
    *budget = max_scratch_bytes ? max_scratch_bytes : ((size_t)256 << 20);
    const size_t L = *budget / per_label;
    return L > (size_t)K ? (size_t)K : L;
}

}  // namespace ts2d
#pragma GCC visibility pop
