// The output side behind the export of libts2d_engine.so, which needs no engine: nnU-Net's largest-component postprocessing of a decided label map
// (kernels_post_cc.h).  One upload, every step on the device, one download; every device buffer of the call is a DevMem, so HIP_TRY may return
// wherever it fails.
#include "engine_internal.h"
#include "entry_util.h"
#include "kernels_post_cc.h"

#include <vector>

using namespace ts2d;

static_assert(kCcStatusGiveUp == TS2D_CC_GIVE_UP, "the status bit speaks the C header's number");
static_assert(sizeof(ts2d_cc_step) == 257, "a step is its 256-byte table and the background byte");

int ts2d_keep_largest_components(int device, uint8_t* seg, int Z, int H, int W, const ts2d_cc_step* steps, int n_steps, int64_t* stats, int* status) {
    const char* const entry = "ts2d_keep_largest_components";
    if (!seg || !status || (!steps && n_steps > 0)) return fail(TS2D_ERR_INVALID, "%s: null argument", entry);
    *status = 0;
    if (Z < 1 || H < 1 || W < 1) return fail(TS2D_ERR_INVALID, "%s: extents %d x %d x %d must be positive", entry, Z, H, W);
    if (!volume_fits_int32(Z, H, W))
        return fail(TS2D_ERR_INVALID, "%s: %d x %d x %d are more voxels than one call takes (2^31 - 1: the indices are int32)", entry, Z, H, W);
    if (n_steps < 0) return fail(TS2D_ERR_INVALID, "%s: %d steps", entry, n_steps);
    if (n_steps == 0) return TS2D_OK;
    HIP_TRY(hipSetDevice(device));
    const size_t n = (size_t)Z * H * W;
    const int ww = (W + 63) >> 6;
    const long long words = (long long)Z * H * ww;
    // [status, counters of every step | the steps | seg | bit words | parent | count]
    const size_t ctr_ints = 1 + (size_t)n_steps * kCcCounters;
    ArenaLayout lay;
    const size_t o_ctr = lay.add(ctr_ints * sizeof(int)), o_steps = lay.add((size_t)n_steps * sizeof(ts2d_cc_step)), o_seg = lay.add(n);
    const size_t o_bits = lay.add((size_t)words * sizeof(cc_word)), o_parent = lay.add(n * sizeof(int)), o_count = lay.add(n * sizeof(int));
    DevMem d;
    HIP_TRY(d.alloc(lay.total()));
    int* const d_status = d.as<int>(o_ctr);
    uint8_t* const d_seg = d.as<uint8_t>(o_seg);
    cc_word* const d_bits = d.as<cc_word>(o_bits);
    int* const d_parent = d.as<int>(o_parent);
    int* const d_count = d.as<int>(o_count);
    HIP_TRY(hipMemset(d_status, 0, ctr_ints * sizeof(int)));
    HIP_TRY(hipMemcpy(d.as<char>(o_steps), steps, (size_t)n_steps * sizeof(ts2d_cc_step), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_seg, seg, n, hipMemcpyHostToDevice));
    const dim3 grid((unsigned)((words + 3) / 4)), block(256);
    for (int s = 0; s < n_steps; ++s) {          // each launch sees the one before it: the default stream orders them
        const uint8_t* member = d.as<const uint8_t>(o_steps + (size_t)s * sizeof(ts2d_cc_step));
        int* ctr = d_status + 1 + (size_t)s * kCcCounters;
        hipLaunchKernelGGL(cc_mask_init, grid, block, 0, 0, d_seg, member, W, words, d_bits, d_parent, d_count, ctr);
        hipLaunchKernelGGL(cc_link, grid, block, 0, 0, d_bits, d_parent, H, W, words, d_status);
        hipLaunchKernelGGL(cc_flatten, grid, block, 0, 0, d_parent, W, words, ctr, d_status);
        hipLaunchKernelGGL(cc_count, grid, block, 0, 0, d_parent, W, words, d_count);
        hipLaunchKernelGGL(cc_max, grid, block, 0, 0, d_parent, d_count, W, words, ctr);
        hipLaunchKernelGGL(cc_apply, grid, block, 0, 0, d_seg, d_parent, d_count, W, words, steps[s].background, ctr, d_status);
        HIP_TRY(hipGetLastError());
    }
    std::vector<int> ctr(ctr_ints);
    HIP_TRY(hipMemcpy(ctr.data(), d_status, ctr_ints * sizeof(int), hipMemcpyDeviceToHost));
    if (ctr[0]) { *status = ctr[0]; return TS2D_OK; }            // a bounded loop reached its cap: the caller's buffer and stats stay as they are
    HIP_TRY(hipMemcpy(seg, d_seg, n, hipMemcpyDeviceToHost));
    if (stats)
        for (size_t k = 0; k < (size_t)n_steps * kCcCounters; ++k) stats[k] = ctr[1 + k];
    return TS2D_OK;
}
