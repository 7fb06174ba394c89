// The host plan of ts2d_label_morphology (morph.hip, kernels_morph.h): the cover table, which carries every floating-point decision of a call
// (morph.h), and how many labels work at once under a bound.  Plain C++ with no HIP in it.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#pragma GCC visibility push(hidden)      // (the library exports the C-ABI only)
namespace ts2d {

struct MoPlan {
    std::vector<uint16_t> cover;      // cover[0 ... T - 1], 1 <= T <= H
    size_t per_label = 0;             // the scratch of one label: per pixel 2 bytes of g, 1 of the intermediate plane (open, close), 1 of result plane (label map)
    size_t labels = 0;                // the labels of one chunk
    size_t budget = 0;                // the bound that was used
};

// Returns 0, or -1 where ONE label does not fit the bound (max_scratch_bytes; 0: 256 MiB) - the table is built either way.  The extents
// (1 ... 32767), the op, the kind, K >= 1 and finite radius >= 0 and spacings > 0 are the caller's to check.
int mo_plan(int kind, int op, int H, int W, double sy, double sx, double radius, int K, size_t max_scratch_bytes, MoPlan* plan);

}  // namespace ts2d
#pragma GCC visibility pop
