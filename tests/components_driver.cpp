// TEST INFRASTRUCTURE (never linked into the product): the class-equality linking of csrc/cc_label.h (cc_link_voxel_classes, cc_class_run_start,
// cc_class_run_length) as plain C++ behind a main of its own - the atomics become plain single-threaded operations.  Built by
// tests/test_components_cpu.py under the address and undefined-behaviour sanitizers; touches no device and is never loaded into Python.
//
//     components_driver IN OUT     IN: cases of (int32 Z, H, W, faces, reverse; uint8 cls[Z H W]).  The phases of csrc/kernels_components.h on one set, in
//                                  one thread: eq words and initial parents per 64-voxel word, the links of every voxel with a class (in index
//                                  order, or in reverse), the flattening, the counts per run.  OUT, per case: int32 gave_up, parent[Z H W], count[Z H W].
#include "../totalsegmentator2d_amd/csrc/cc_label.h"

#include <cstdio>
#include <vector>

using namespace ts2d;

int main(int argc, char** argv) {
    if (argc != 3) return 1;
    FILE* in = std::fopen(argv[1], "rb");
    FILE* out = std::fopen(argv[2], "wb");
    if (!in || !out) return 2;
    int head[5];
    while (std::fread(head, sizeof(int), 5, in) == 5) {
        const int Z = head[0], H = head[1], W = head[2], faces = head[3], reverse = head[4];
        const size_t n = (size_t)Z * H * W;
        const int ww = (W + 63) >> 6;
        std::vector<uint8_t> cls(n);
        if (std::fread(cls.data(), 1, n, in) != n) return 3;
        std::vector<int> parent(n), count(n, 0);
        std::vector<cc_word> eq((size_t)Z * H * ww, 0);
        for (long long row = 0; row < (long long)Z * H; ++row)
            for (int w = 0; w < ww; ++w) {
                cc_word m = 0;
                for (int l = 1; l < 64 && w * 64 + l < W; ++l) {
                    const uint8_t c = cls[(size_t)row * W + w * 64 + l];
                    if (c && cls[(size_t)row * W + w * 64 + l - 1] == c) m |= 1ull << l;
                }
                eq[(size_t)row * ww + w] = m;
                for (int l = 0; l < 64 && w * 64 + l < W; ++l) {
                    const size_t i = (size_t)row * W + w * 64 + l;
                    parent[i] = cls[i] ? (int)i - l + cc_class_run_start(m, l) : -1;
                }
            }
        int gave_up = 0;
        for (size_t s = 0; s < n; ++s) {
            const size_t i = reverse ? n - 1 - s : s;
            if (!cls[i]) continue;
            const int x = (int)(i % W), y = (int)(i / W % H), z = (int)(i / W / H);
            cc_link_voxel_classes(parent.data(), cls.data(), H, W, z, y, x, faces, kCcFindCap, kCcUnionCap, &gave_up);
        }
        for (size_t i = 0; i < n; ++i)
            if (parent[i] >= 0) parent[i] = cc_find(parent.data(), (int)i, kCcFindCap, &gave_up);
        for (size_t i = 0; i < n; ++i) {
            const int l = (int)(i % W) & 63;
            const cc_word m = eq[i / W * ww + (i % W >> 6)];
            if (parent[i] >= 0 && !(m >> l & 1)) count[parent[i]] += cc_class_run_length(m, l);
        }
        if (std::fwrite(&gave_up, sizeof(int), 1, out) != 1 || std::fwrite(parent.data(), sizeof(int), n, out) != n ||
            std::fwrite(count.data(), sizeof(int), n, out) != n)
            return 4;
    }
    std::fclose(in);
    std::fclose(out);
    return 0;
}
