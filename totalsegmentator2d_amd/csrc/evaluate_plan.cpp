// The host plan of ts2d_volume_surface_distances: evaluate_plan.h.
#include "evaluate_plan.h"

namespace ts2d {

size_t sdv_label_bytes(long long vox, long long rows, int P, int want_sum) {
    return (size_t)vox * (2 * (1 + sizeof(uint16_t) + sizeof(double)) + (P ? 2 * sizeof(uint64_t) : 0)) + (want_sum ? (size_t)rows * 2 * sizeof(double) : 0);
}

int sdv_plan(const int32_t* box, int K, int P, int want_sum, size_t budget, std::vector<SdvLabel>* labels, std::vector<SdvChunk>* chunks,
             size_t* need) {
    labels->assign((size_t)K, SdvLabel{0, 0, 0, 0, 0, 0, 0, 0});
    chunks->clear();
    for (int k = 0; k < K; ++k) {
        const int32_t* b = box + (size_t)k * 6;
        if (b[3] < 0) continue;
        SdvLabel& l = (*labels)[(size_t)k];
        l.z0 = b[0]; l.y0 = b[1]; l.x0 = b[2];
        l.bz = b[3] - b[0] + 1; l.by = b[4] - b[1] + 1; l.bx = b[5] - b[2] + 1;
        *need = sdv_label_bytes((long long)l.bz * l.by * l.bx, (long long)l.bz * l.by, P, want_sum);
        if (*need > budget) {
            labels->clear();
            return k;
        }
    }
    SdvChunk c = {0, 0, 0, 0};
    size_t used = 0;
    for (int k = 0; k < K; ++k) {
        SdvLabel& l = (*labels)[(size_t)k];
        const long long rows = (long long)l.bz * l.by, vox = rows * l.bx;
        const size_t bytes = sdv_label_bytes(vox, rows, P, want_sum);
        if (used + bytes > budget) {                               // (bytes > 0: an empty label never closes a chunk)
            chunks->push_back(c);
            c = SdvChunk{k, k, 0, 0};
            used = 0;
        }
        l.vox = c.vox; l.row = c.rows;
        c.vox += vox; c.rows += rows; c.k1 = k + 1;
        used += bytes;
    }
    chunks->push_back(c);
    return -1;
}

}  // namespace ts2d
