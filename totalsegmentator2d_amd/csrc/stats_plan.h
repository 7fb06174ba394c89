// The host plans of ts2d_label_statistics and ts2d_label_percentiles (stats.hip, kernels_stats.h, kernels_stats_select.h): the device state of
// one label and the chunks of labels that work at once under a bound.  Plain C++ with no HIP in it, so stats_plan.cpp also compiles into a stand-alone host program
// (tests/test_statistics_percentiles_cpu.py sweeps it).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#pragma GCC visibility push(hidden)      // (the library exports the C-ABI only)
namespace ts2d {

// Labels [k0, k1) work at once.
struct LsChunk {
    int k0, k1;
};

// The state of one label: per channel R = 2 P selections of a rank (int64), a prefix (uint64) and 256 bins (uint32), and the row partials of
// the counting pass (count, min x, max x as int32, the x sum as int64: 20 bytes per row).
size_t ls_label_bytes(int C, int P, long long rows);

// Chunks of equally many labels in their order (the last one takes the rest), as many per chunk as keep the chunk's state at or below the
// bound (max_scratch_bytes; 0: 256 MiB; *budget: what was used) and its row partials within an int32 index.  Returns 0, or -1 where ONE label
// does not fit (*need: its bytes) - then nothing is planned.  K, C, P >= 1 and 1 <= rows <= 2^31 - 1 are the caller's to check.
int ls_plan(int K, int C, int P, long long rows, size_t max_scratch_bytes, std::vector<LsChunk>* chunks, size_t* need, size_t* budget);

// ts2d_label_statistics: the row partials of one label - count, min x, max x (int32) and the x sum (int64) per row, and per channel and row one
// float64 and two keys: rows * (20 + 16 C) bytes.
size_t st_label_bytes(int C, long long rows);

// The labels of one chunk of ts2d_label_statistics (*labels; every chunk but the last has as many): as many as keep the row partials at or below
// the bound (max_scratch_bytes; 0: 256 MiB; *budget: what was used), at most K, and at most as many as keep a channel partial's slot,
// (label * C + channel) * rows + row, within an int32.  Returns 0; -1 where ONE label does not fit the bound (*need: its bytes); -2 where one
// label's rows * max(C, 1) slots alone pass an int32.  K >= 1, C >= 0 and 1 <= rows <= 2^31 - 1 are the caller's to check.
int st_plan(int K, int C, long long rows, size_t max_scratch_bytes, size_t* labels, size_t* need, size_t* budget);

}  // namespace ts2d
#pragma GCC visibility pop
