// TEST INFRASTRUCTURE (never linked into the product): the host side of csrc/morph.h - the cover table (mo_cover_table) and the ONE host walk of a
// label (mo_label: the column scans and the row walk in 64-pixel chunks with their carries) - as plain C++ behind a main of its own.  Built by
// tests/test_morphology_cpu.py under the address and undefined-behaviour sanitizers; touches no device and is never loaded into Python.
//
//     morph_driver IN OUT     IN: cases of (int32 H, W, kind, value, op; float64 radius, sy, sx; uint8 seg[H W]).
//                             OUT, per case: int32 T, int32 cover[T], uint8 res[H W] (1 where the operation leaves the label's pixel set).
// Every buffer has exactly the size the header asks for, so a step past an end is the sanitizer's to report.
#include "../totalsegmentator2d_amd/csrc/morph.h"

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
        const int H = head[0], W = head[1], kind = head[2], value = head[3], op = head[4];
        double real[3];
        if (std::fread(real, sizeof(double), 3, in) != 3) return 3;
        const size_t n = (size_t)H * W;
        std::vector<uint8_t> seg(n);
        if (std::fread(seg.data(), 1, n, in) != n) return 3;
        std::vector<uint16_t> cover((size_t)H);
        const int T = mo_cover_table(real[0], real[1], real[2], H, W, cover.data());
        cover.resize((size_t)T);                                   // the walk may read the T entries and no more
        std::vector<uint16_t> g(n);
        std::vector<uint8_t> mid(mo_steps(op) == 2 ? n : 0), res(n);
        mo_label(seg.data(), kind, (uint8_t)value, H, W, op, cover.data(), T, g.data(), mid.data(), res.data());
        std::vector<int> table(cover.begin(), cover.end());
        if (std::fwrite(&T, sizeof(int), 1, out) != 1 || std::fwrite(table.data(), sizeof(int), (size_t)T, out) != (size_t)T ||
            std::fwrite(res.data(), 1, n, out) != n)
            return 4;
    }
    std::fclose(in);
    std::fclose(out);
    return 0;
}
