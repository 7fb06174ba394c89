// The host plans of ts2d_label_statistics and ts2d_label_percentiles: stats_plan.h.
#include "stats_plan.h"

#include "entry_util.h"

namespace ts2d {

size_t ls_label_bytes(int C, int P, long long rows) {
    const size_t R = 2 * (size_t)P;
    return (size_t)C * R * (sizeof(int64_t) + sizeof(uint64_t) + 256 * sizeof(uint32_t)) + (size_t)rows * 20;
}

int ls_plan(int K, int C, int P, long long rows, size_t max_scratch_bytes, std::vector<LsChunk>* chunks, size_t* need, size_t* budget) {
    chunks->clear();
    *budget = max_scratch_bytes ? max_scratch_bytes : ((size_t)256 << 20);
    *need = ls_label_bytes(C, P, rows);
    size_t L = *budget / *need;
    if (L < 1) return -1;
    const size_t slot_cap = (size_t)(0x7FFFFFFFll / rows);          // a row partial's slot, label * rows + row, is an int32 (>= 1: rows <= 2^31 - 1)
    if (L > slot_cap) L = slot_cap;
    if (L > (size_t)K) L = (size_t)K;
    for (int k0 = 0; k0 < K; k0 += (int)L) chunks->push_back(LsChunk{k0, k0 + (int)L < K ? k0 + (int)L : K});
    return 0;
}

size_t st_label_bytes(int C, long long rows) { return (size_t)rows * (20 + 16 * (size_t)C); }

int st_plan(int K, int C, long long rows, size_t max_scratch_bytes, size_t* labels, size_t* need, size_t* budget) {
    *labels = 0;
    *need = st_label_bytes(C, rows);
    size_t L = labels_per_chunk(max_scratch_bytes, *need, K, budget);
    if (L < 1) return -1;
    const size_t slot_cap = (size_t)0x7FFFFFFF / ((size_t)rows * (size_t)(C > 0 ? C : 1));       // int32 slots: L * C * rows stays below 2^31
    if (slot_cap < 1) return -2;
    if (L > slot_cap) L = slot_cap;
    *labels = L;
    return 0;
}

}  // namespace ts2d
