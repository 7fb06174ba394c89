// The host plan of ts2d_label_morphology: morph_plan.h.
#include "morph_plan.h"

#include "entry_util.h"
#include "morph.h"

namespace ts2d {

int mo_plan(int kind, int op, int H, int W, double sy, double sx, double radius, int K, size_t max_scratch_bytes, MoPlan* plan) {
    plan->cover.assign((size_t)H, 0);
    plan->cover.resize((size_t)mo_cover_table(radius, sy, sx, H, W, plan->cover.data()));
    const size_t n = (size_t)H * (size_t)W;
    plan->per_label = n * (sizeof(uint16_t) + (mo_steps(op) == 2 ? 1 : 0) + (kind == kStLabelMap ? 1 : 0));
    plan->labels = labels_per_chunk(max_scratch_bytes, plan->per_label, K, &plan->budget);
    return plan->labels < 1 ? -1 : 0;
}

}  // namespace ts2d
