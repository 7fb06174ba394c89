// The host plan of ts2d_volume_surface_distances (evaluate.hip, kernels_evaluate_volume.h): from the K x 6 integers of the labels' joint
// bounding boxes, the scratch of every label and the chunks of labels that work at once under a bound.  Plain C++ with no HIP in it, so
// evaluate_plan.cpp also compiles into a stand-alone host program (tests/test_evaluate_volume_cpu.py).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#pragma GCC visibility push(hidden)      // (the library exports the C-ABI only)
namespace ts2d {

// One label of a call, as the kernels read it: the first voxel and the extents of its box (bz = by = bx = 0: empty on both sides, no box),
// and where its scratch starts in the arrays of its chunk - vox: in box voxels, row: in box rows (z, y), both summed over the chunk's labels
// before it.
struct SdvLabel {
    int z0, y0, x0, bz, by, bx;
    long long vox, row;
};
static_assert(sizeof(SdvLabel) == 40, "SdvLabel is copied to the device as bytes");

// Labels [k0, k1) work at once: vox and rows are the sums of their box voxels and box rows (what the chunk's arrays hold per side).
struct SdvChunk {
    int k0, k1;
    long long vox, rows;
};

// The scratch of one label: per box voxel 2 (border) + 4 (g) + 16 (h) bytes and with percentiles 16 more (keys), with the sum 16 per box row.
size_t sdv_label_bytes(long long vox, long long rows, int P, int want_sum);

// box: [K][6] = smallest z, y, x, largest z, y, x (inclusive; largest z < 0: the label is empty on both sides).  Fills labels [K] and the
// chunks: labels in their order, a chunk closed where the next label would pass `budget` bytes; an empty label joins the chunk at hand and
// costs nothing.  Returns -1, or the first label whose own scratch is above the budget (*need: its bytes) - then nothing is planned.
int sdv_plan(const int32_t* box, int K, int P, int want_sum, size_t budget, std::vector<SdvLabel>* labels, std::vector<SdvChunk>* chunks,
             size_t* need);

}  // namespace ts2d
#pragma GCC visibility pop
