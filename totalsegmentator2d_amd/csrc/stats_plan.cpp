// The host plan of ts2d_label_percentiles: stats_plan.h.
#include "stats_plan.h"

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

}  // namespace ts2d
