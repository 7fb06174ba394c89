// The confusion matrix of two segmentations (ts2d_label_confusion; the statement: evaluate.confusion_statement): what a ROW of a side is, as
// the bytes the integer matrix product takes.  Host and device: kernels_confusion.h builds its MFMA operands from these functions, and
// tests/confusion_driver.cpp forms the whole matrix from them on the host, under the sanitizers.
//
// A side has K + 2 rows over the N samples: row 0 "none of the K labels", row 1 + k the mask of label k, row K + 1 every sample.  The product
// wants every row as 0 / 1 bytes, four samples to a 32-bit word.  A row's bytes come from a SOURCE - the side's none plane (made by cf_none from
// cf_none_of_planes / cf_in_set), plane k, the label map, or nothing - and a FORM, four words that turn a raw word of the source into the operand
// word without a branch:
//
//     operand = (((bytes of (raw ^ xorv) that are not 0, as 0 / 1) ^ flip) & andm) | orc
//
//     none row, plane row     xorv 0         flip 0           andm ~0   orc 0            byte != 0 -> 1 (a plane byte of 128 ... 255 is a
//                                                                                         negative i8: no plane byte goes to the product raw)
//     label-map row of value  xorv value x 4 flip 0x01010101  andm ~0   orc 0            byte == value -> 1
//     all row                 -              -                andm 0    orc 0x01010101   no load
//     a row beyond K + 1      -              -                andm 0    orc 0            no load: a zero operand
//
// Samples beyond N inside the last step are cleared by cf_valid_word on BOTH operands (the all row has no source that would end).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define CF_HD __host__ __device__ __forceinline__
#else
#define CF_HD inline
#endif

namespace ts2d {

constexpr int kCfPlanes = 0, kCfLabelMap = 1;          // TS2D_STATS_PLANES, TS2D_STATS_LABELMAP
constexpr int kCfTile = 32;                            // rows of a tile of either side: the M and N of the 32x32x32 product
constexpr int kCfStep = 32;                            // samples of one product step: its K
constexpr int kCfLoad = 16;                            // bytes of one operand: a lane's 16 consecutive samples

enum CfSource { kCfSrcNothing = 0, kCfSrcNone = 1, kCfSrcPlane = 2, kCfSrcMap = 3 };

struct CfRow {
    uint32_t xorv, flip, andm, orc;
    int source;                                        // CfSource
    int plane;                                         // kCfSrcPlane: which
};

// 0 / 1 in every byte of y that is not 0
CF_HD uint32_t cf_nonzero_bytes(uint32_t y) { return ((((y & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | y) & 0x80808080u) >> 7; }

// row i (0 ... ) of a side of kind `kind` with K labels; values: the K values of a label map (not read for planes)
CF_HD CfRow cf_row(int i, int K, int kind, const uint8_t* values) {
    CfRow r = {0u, 0u, 0u, 0u, kCfSrcNothing, 0};
    if (i == 0) {
        r.andm = 0xFFFFFFFFu; r.source = kCfSrcNone;
    } else if (i <= K) {
        r.andm = 0xFFFFFFFFu;
        if (kind == kCfLabelMap) {
            r.xorv = (uint32_t)values[i - 1] * 0x01010101u; r.flip = 0x01010101u; r.source = kCfSrcMap;
        } else {
            r.source = kCfSrcPlane; r.plane = i - 1;
        }
    } else if (i == K + 1) {
        r.orc = 0x01010101u;
    }
    return r;
}

// the operand word of four samples from the raw word of the row's source (raw: anything where the row has no source)
CF_HD uint32_t cf_operand_word(uint32_t raw, const CfRow& r) { return ((cf_nonzero_bytes(raw ^ r.xorv) ^ r.flip) & r.andm) | r.orc; }

// 0xFF in byte t where sample s + t exists (s + t < n), for the word of samples s ... s + 3
CF_HD uint32_t cf_valid_word(long long s, long long n) {
    const long long left = n - s;
    return left >= 4 ? 0xFFFFFFFFu : left <= 0 ? 0u : (0xFFFFFFFFu >> (8 * (4 - (int)left)));
}

// THE CLASS OF A BYTE of a label map: the 256-bit set of the K values, and whether a byte is in it ("none" is: it is not)
CF_HD void cf_set_build(const uint8_t* values, int K, uint32_t set[8]) {
    for (int w = 0; w < 8; ++w) set[w] = 0u;
    for (int k = 0; k < K; ++k) set[values[k] >> 5] |= 1u << (values[k] & 31);
}
CF_HD uint32_t cf_in_set(const uint32_t* set, uint8_t byte) { return (set[byte >> 5] >> (byte & 31)) & 1u; }

// ... of planes: the OR of the K plane words of four samples -> the none word
CF_HD uint32_t cf_none_of_planes(uint32_t any) { return cf_nonzero_bytes(any) ^ 0x01010101u; }

}  // namespace ts2d
