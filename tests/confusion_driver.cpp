// TEST INFRASTRUCTURE (never linked into the product): the operand forms and the class-of-byte rule of csrc/confusion.h as plain C++ behind a
// main of its own.  Built by tests/test_confusion_cpu.py under the address and undefined-behaviour sanitizers; touches no device and is never
// loaded into Python.
//
//     confusion_driver IN OUT     IN: cases of (int32 N, K, kind_a, kind_b; uint8 values[K]; uint8 a[K N or N]; uint8 b[K N or N]).  The walk of
//                                 csrc/kernels_confusion.h in one thread: the none plane of either side 16 samples at a time (cf_none), then per
//                                 step of 32 samples and per half of 16 the operand words of every row of a and of b (cf_row, cf_operand_word;
//                                 the samples past N byte by byte and cleared by cf_valid_word) and their byte-wise products, added per row pair.
//                                 Every buffer has exactly its size, so a read past a row's end is the sanitizer's finding.
//                                 OUT, per case: int64 M[K + 2][K + 2], row = side a.
#include "../totalsegmentator2d_amd/csrc/confusion.h"

#include <cstdio>
#include <cstring>
#include <vector>

using namespace ts2d;

// 16 samples from `off` on as four words: a copy of 16 bytes where they all exist, else the existing ones byte by byte and 0
static void load_words(const uint8_t* p, long long off, long long n, uint32_t w[4]) {
    w[0] = w[1] = w[2] = w[3] = 0u;
    if (!p || off >= n) return;
    if (n - off >= kCfLoad) { std::memcpy(w, p + off, kCfLoad); return; }
    for (int t = 0; t < (int)(n - off); ++t) w[t >> 2] |= (uint32_t)p[off + t] << (8 * (t & 3));
}

static std::vector<uint8_t> none_plane(const uint8_t* seg, int kind, int K, long long n, const uint32_t* set) {
    std::vector<uint8_t> none((size_t)n);
    for (long long s = 0; s < n; s += kCfLoad) {
        uint32_t w[4];
        if (kind == kCfLabelMap) {
            uint32_t x[4];
            load_words(seg, s, n, x);
            for (int j = 0; j < 4; ++j) {
                w[j] = 0u;
                for (int t = 0; t < 4; ++t) w[j] |= (cf_in_set(set, (uint8_t)(x[j] >> (8 * t))) ^ 1u) << (8 * t);
            }
        } else {
            uint32_t any[4] = {0u, 0u, 0u, 0u};
            for (int k = 0; k < K; ++k) {
                uint32_t x[4];
                load_words(seg + (long long)k * n, s, n, x);
                for (int j = 0; j < 4; ++j) any[j] |= x[j];
            }
            for (int j = 0; j < 4; ++j) w[j] = cf_none_of_planes(any[j]);
        }
        for (int t = 0; t < kCfLoad && s + t < n; ++t) none[(size_t)(s + t)] = (uint8_t)(w[t >> 2] >> (8 * (t & 3)));
    }
    return none;
}

static const uint8_t* source(const CfRow& r, const uint8_t* seg, const uint8_t* none, long long n) {
    return r.source == kCfSrcNone ? none : r.source == kCfSrcPlane ? seg + (long long)r.plane * n : r.source == kCfSrcMap ? seg : nullptr;
}

int main(int argc, char** argv) {
    if (argc != 3) return 1;
    FILE* in = std::fopen(argv[1], "rb");
    FILE* out = std::fopen(argv[2], "wb");
    if (!in || !out) return 2;
    int head[4];
    while (std::fread(head, sizeof(int), 4, in) == 4) {
        const long long n = head[0];
        const int K = head[1], kind_a = head[2], kind_b = head[3];
        std::vector<uint8_t> values((size_t)K), a((size_t)(kind_a == kCfPlanes ? K * n : n)), b((size_t)(kind_b == kCfPlanes ? K * n : n));
        if (std::fread(values.data(), 1, values.size(), in) != values.size() || std::fread(a.data(), 1, a.size(), in) != a.size() ||
            std::fread(b.data(), 1, b.size(), in) != b.size())
            return 3;
        uint32_t set[8];
        cf_set_build(values.data(), K, set);
        const std::vector<uint8_t> none_a = none_plane(a.data(), kind_a, K, n, set), none_b = none_plane(b.data(), kind_b, K, n, set);
        const int rows = K + 2, padded = (rows + kCfTile - 1) / kCfTile * kCfTile;         // the rows of the last tile beyond K + 1: zero operands
        std::vector<long long> m((size_t)rows * rows, 0);
        std::vector<uint32_t> wa((size_t)padded * 4), wb((size_t)padded * 4);
        for (long long s = 0; s < n; s += kCfStep)
            for (int h = 0; h < 2; ++h) {
                const long long off = s + kCfLoad * h;
                for (int i = 0; i < padded; ++i) {
                    const CfRow ra = cf_row(i, K, kind_a, values.data()), rb = cf_row(i, K, kind_b, values.data());
                    uint32_t xa[4], xb[4];
                    load_words(source(ra, a.data(), none_a.data(), n), off, n, xa);
                    load_words(source(rb, b.data(), none_b.data(), n), off, n, xb);
                    for (int j = 0; j < 4; ++j) {
                        wa[(size_t)i * 4 + j] = cf_operand_word(xa[j], ra) & cf_valid_word(off + 4 * j, n);
                        wb[(size_t)i * 4 + j] = cf_operand_word(xb[j], rb) & cf_valid_word(off + 4 * j, n);
                    }
                }
                for (int i = 0; i < padded; ++i)
                    for (int j = 0; j < padded; ++j) {
                        long long sum = 0;
                        for (int t = 0; t < kCfLoad; ++t)
                            sum += (long long)(int8_t)(wa[(size_t)i * 4 + (t >> 2)] >> (8 * (t & 3))) * (int8_t)(wb[(size_t)j * 4 + (t >> 2)] >> (8 * (t & 3)));
                        if (i < rows && j < rows) m[(size_t)i * rows + j] += sum;
                        else if (sum != 0) return 5;                                       // a row beyond K + 1 is a zero operand
                    }
            }
        if (std::fwrite(m.data(), sizeof(long long), m.size(), out) != m.size()) return 4;
    }
    std::fclose(in);
    std::fclose(out);
    return 0;
}
