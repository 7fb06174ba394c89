// conv3x3s2_v2p: the split-mode instance <128, float, 3, no resident weights, fixed 8 x 32 tile> of conv3x3s2_v2 (kernels_s2v2.h) as a
// PIPELINE in the manner of conv3x3_f16x3_qp (enc2.c0, enc3.c0, enc4.c0 of the canonical net).
//
// In-kernel stamps of conv3x3s2_v2 (profiles/r06_phase_stamps.txt, enc3.c0): of ~939 k cycles per workgroup 295 k are the InstanceNorm +
// LeakyReLU + hi / lo split of the patch - all eight waves at once, between two barriers, every matrix pipe idle.  A second patch buffer did
// not fit beside the chunk's weight block (71936 + 73728 of 163840 bytes).  Here
//   * the B operand comes straight from L2 (the packed image a.wph, unchanged) through a register ring two taps deep, as in conv3x3_upq
//     phase 1: per tap a wave loads its four fragments (2 nt x hi, lo) of 16 bytes per lane; no weight image in LDS;
//   * LDS = two patch buffers (same planes, same even | odd column order, same plane stride) + a statistics exchange of its own;
//   * one stream of (tile, chunk) items per workgroup: the MFMAs of item i, the conversion of item i+1 into the other buffer - unit t at
//     tap t - and the raw load of that unit for item i+2 right behind its conversion; one LDS-only barrier per item; a tile's epilogue
//     overlaps the staging of the next tile's first chunk;
//   * nine taps are an odd number and the ring has two slots, so tap 0 changes slot from item to item: the item body exists twice (even
//     and odd items), which also makes the patch buffer a compile-time constant.
// Arithmetic as conv3x3s2_v2: same tap order, 16-channel chunks, fresh accumulator per chunk merged into the tile's, same epilogue and
// shifted partials - outputs and partials are bit-identical to it (tests/test_gpu_s2_pipeline.py).
//
// Memory counters.  vmcnt retires in order, so a wait for the ring's tap t+1 is also a wait for every patch load issued before it.  Per tap
// the order of issue is: the four weight loads of tap t+2 (behind the tap's last MFMA: they overwrite its slot), then the one patch unit;
// hipcc counts the waits (vmcnt(N), N = what was issued behind the load), there is no vmcnt(0) in the tap stream and no DMA that would
// force one.  The scale / shift of item i+2 are requested at tap 8 AHEAD of that tap's weight and patch loads: their first use is tap 0.
// The conversion is branch-free (padding by select, a unit that has no slot loads out of range and stores into its row's unused 66th
// slot; only unit 8 - slots past the plane - is predicated): the dispatch gives this instance normalised sources only.
// Registers: 256 VGPRs, no scratch (tests/test_s2_pipeline_isa.py) - the unit coordinates are packed (five registers for nine units + their
// padding flags) and a tap reads the next tap's A fragments only behind the product group that frees their registers.
// Measured (profiles/r21_s2_pipeline.txt, B = 64): enc2-4.c0 0.56-0.59 -> 0.49-0.50 ms per launch (-13 ... -16 %), bench.py +0.8 ... +1.1 %.
#pragma once
#include "kernels_s2v2.h"
#include "tile_dims.h"

namespace ts2d {

constexpr int kS2pPatch = 4 * kS2Plane;                       // hi, lo x h planes of one patch
constexpr int kS2pRed = 2 * kS2pPatch, kS2pLds = kS2pRed + 8192;      // + the statistics exchange [wm 4][column 128] x (S, Q, K, n)
static_assert(kS2pLds <= kS2LdsMax && kS2Plane == kS2PlaneBytes, "LDS of conv3x3s2_v2p");
template <int V> struct S2pParity { static constexpr int value = V; };

__global__ __launch_bounds__(kS2Threads, 2) void conv3x3s2_v2p(const ConvArgs a) {
    constexpr int BN = 128, NTW = 2, MAXU = 9, USTEP = 128;
    constexpr int WTAP = 2 * 2 * BN * 16, WB = 9 * WTAP;      // weight bytes per tap / per chunk of the global image
    extern __shared__ __attribute__((aligned(16))) unsigned char smem8[];
    typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

    // ---- this workgroup's tiles (as conv3x3s2_v2)
    const int xcd = blockIdx.x & 7, q80 = blockIdx.x >> 3;
    const int qm0 = q80 / a.n_ctiles;
    const int ctile = q80 - qm0 * a.n_ctiles, n0col = ctile * BN;
    const int mtile0 = qm0 * 8 + xcd, mstep = ((int)(gridDim.x >> 3) / a.n_ctiles) * 8;
    if (mtile0 >= a.n_mtiles) return;
    const int ntl = (a.n_mtiles - 1 - mtile0) / mstep + 1;
    const int nchunks = a.C0 / 16;
    const int tpi = a.tiles_x * a.tiles_y;

    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6), wm = w & 3, wn = w >> 2;
    const int r = lane & 31, h = lane >> 5;

    // ---- staging plan (tile-independent; conv3x3s2_v2, fp32 storage): unit it of thread tid = slot (tid >> 2) + 128 it, quarter sub = tid & 3
    const int sub = tid & 3, slot0 = tid >> 2;
    // (py, px) of the nine units packed 12 bits each, two per register (py = 31: no unit - the 66th slot of a row, slots past the patch; its
    // load goes out of range and returns zeros): the byte offset and the padding test are recomputed per use instead of living in 10 registers
    // Bits 24-27 of a register: per unit "patch row 0" | "patch column 0" << 1 - the padding candidates.
    unsigned upk[(MAXU + 1) / 2] = {0, 0, 0, 0, 0};
    const int lw0 = (sub >> 1) * kS2Plane + slot0 * 16 + (sub & 1) * 8;
    const bool unit8 = slot0 + USTEP * 8 < kS2Slots;       // unit 8 has a slot inside the plane
#pragma unroll
    for (int it = 0; it < MAXU; ++it) {
        const int q = slot0 + USTEP * it;
        const int py = q / kS2PW, rem = q - py * kS2PW;
        const int half = rem >= 33 ? 1 : 0, px = 2 * (rem - 33 * half) + half;
        const bool exists = q < kS2Slots && px <= 64;
        upk[it >> 1] |= (exists ? (unsigned)((py << 7) | px) : (31u << 7)) << (12 * (it & 1));
        if (exists) upk[it >> 1] |= ((py == 0 ? 1u : 0u) | (px == 0 ? 2u : 0u)) << (24 + 2 * (it & 1));
    }
    // (opaque per use: hoisted out of the item loop, the nine offsets would live in registers again)
    auto unit_word = [&](int it) { unsigned u = upk[it >> 1]; asm volatile("" : "+v"(u)); return u; };

    struct Item { int k, c; };
    auto advance = [&](Item& t) {                          // next item of the stream; the last item repeats (loaded / staged, never used)
        int c = t.c + 1, k = t.k;
        if (c == nchunks) { c = 0; ++k; }
        if (k < ntl) { t.k = k; t.c = c; }
    };
    auto tile_origin = [&](int k, int& nimg, int& tyi, int& txi, int& tin) {
        const int mtile = mtile0 + k * mstep;
        nimg = udiv_magic(mtile, a.mg_tpi); tin = mtile - nimg * tpi;
        tyi = udiv_magic(tin, a.mg_tx); txi = tin - tyi * a.tiles_x;
    };
    const size_t img_px = (size_t)a.Hin * a.Win;
    const int rowb = a.C0 * 4;                             // bytes of a pixel record
    u32x4 pv[MAXU];                                        // raw patch units in flight
    f32x4 nsa, nta;                                        // scale / shift of this thread's four channels
    struct Req { __amdgpu_buffer_rsrc_t rs; unsigned org; int soff, noff; unsigned padm; };
    auto request = [&](const Item& t) {
        int nimg, tyi, txi, tin;
        tile_origin(t.k, nimg, tyi, txi, tin);
        Req q;
        q.rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(reinterpret_cast<const float*>(a.src0)) + (size_t)nimg * img_px * a.C0, 0,
                                                 (int)(img_px * a.C0 * 4), 0x00020000);
        // patch origin (2 ty0 - 1, 2 tx0 - 1) may lie one row / column outside the image: unsigned wrap-around is fine, the affected
        // units are padding (zeroed at conversion)
        q.org = (unsigned)((((16 * tyi - 1) * a.Win + 64 * txi - 1) * a.C0) * 4);
        q.soff = t.c * 64;
        q.noff = nimg * a.C0 + t.c * 16;
        q.padm = ((tyi == 0 ? 1u : 0u) | (txi == 0 ? 2u : 0u)) * 0x05000000u;      // which flag bits mean "outside the image" on this tile (both units of a register)
        return q;
    };
    auto load_unit = [&](const Req& q, unsigned uw, int it) {
        const unsigned yx = (uw >> (12 * (it & 1))) & 0xFFFu;
        const unsigned py = yx >> 7, px = yx & 127u;
        // (two 24-bit multiply-adds - a pixel index and a record size - written out: hipcc makes a 64-bit multiply-add and a branch around it of the C form)
        unsigned pix, off;
        asm("v_mad_u32_u24 %0, %1, %2, %3" : "=v"(pix) : "v"(py), "s"(a.Win), "v"(px));
        asm("v_mad_u32_u24 %0, %1, %2, %3" : "=v"(off) : "v"(pix), "s"(rowb), "v"(q.org + 16u * sub));
        const unsigned vo = py == 31u ? 0x80000000u : off;
        pv[it] = __builtin_amdgcn_raw_buffer_load_b128(q.rs, vo, q.soff, 0);
    };
    // (scale / shift: a scalar base and one 32-bit offset register instead of two 64-bit lane addresses)
    auto load_norm = [&](const Req& q) {
        nsa = *reinterpret_cast<const f32x4*>(reinterpret_cast<const unsigned char*>(a.sc0 + q.noff) + (unsigned)(16 * sub));
        nta = *reinterpret_cast<const f32x4*>(reinterpret_cast<const unsigned char*>(a.sh0 + q.noff) + (unsigned)(16 * sub));
    };
    const f32x4 slope4 = f32x4{a.slope, a.slope, a.slope, a.slope};
    auto convert = [&](unsigned uw, int it, unsigned char* pb, unsigned padm) {      // InstanceNorm + LeakyReLU, fp16 hi / lo; padding units store zeros
        unsigned char* d = pb + lw0 + it * USTEP * 16;
        const bool real = (uw & padm & (3u << (24 + 2 * (it & 1)))) == 0u;
        f32x4 va = __builtin_bit_cast(f32x4, pv[it]);
        va = va * nsa + nta;
        const f32x4 na = va * slope4;
#pragma unroll
        for (int e = 0; e < 4; ++e) va[e] = fmaxf(va[e], na[e]);      // LeakyReLU (0 < slope < 1)
        uint2 hi, lo;
        split_hi_lo_4(va, hi, lo);
        hi.x = real ? hi.x : 0u; hi.y = real ? hi.y : 0u; lo.x = real ? lo.x : 0u; lo.y = real ? lo.y : 0u;
        if (it < MAXU - 1 || unit8) {
            *reinterpret_cast<uint2*>(d) = hi;
            *reinterpret_cast<uint2*>(d + 2 * kS2Plane) = lo;
        }
    };

    // ---- weight ring: fragment (tap, part, nt) of lane (r, h) in the image [chunk][column tile][tap][hi, lo][h][column] x 16 B
    const __amdgpu_buffer_rsrc_t rsw = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(reinterpret_cast<const float*>(a.wph)), 0,
                                                                         nchunks * a.n_ctiles * WB, 0x00020000);
    const int wvo = h * BN * 16 + (wn * (BN / 2) + r) * 16;
    half8 rb[2][NTW][2];                                   // [slot][nt][hi, lo]
#define TS2D_LOAD_W(SLOT, CH, TAP) { \
        const int so_ = ((CH) * a.n_ctiles + ctile) * WB + (TAP) * WTAP; \
        _Pragma("unroll") for (int p = 0; p < 2; ++p) _Pragma("unroll") for (int nt = 0; nt < NTW; ++nt) \
            rb[SLOT][nt][p] = __builtin_bit_cast(half8, __builtin_amdgcn_raw_buffer_load_b128(rsw, wvo + nt * 512, so_ + p * 2 * BN * 16, 0)); }

    TS2D_PROF_DECL(a.prof);
    // ---- fill the pipeline: item 0 staged synchronously (once per workgroup), item 1 requested
    Item cur{0, 0}, nx1{0, 0}, nx2{0, 0};
    unsigned padm_nx1;                                     // borders of the tile of nx1 (from its request, one item earlier)
    {
        const Req q0 = request(cur);
#pragma unroll
        for (int it = 0; it < MAXU; ++it) load_unit(q0, unit_word(it), it);
        load_norm(q0);
#pragma unroll
        for (int it = 0; it < MAXU; ++it) convert(unit_word(it), it, smem8, q0.padm);
        advance(nx1);
        nx2 = nx1;
        const Req q1 = request(nx1);
        // the order of issue that an item leaves behind (taps 7 and 8), so that the first item's counted waits are the loop's: ring tap 0,
        // scale / shift, ring tap 1, the units
        __builtin_amdgcn_sched_barrier(0);
        TS2D_LOAD_W(0, 0, 0)
        __builtin_amdgcn_sched_barrier(0);
        load_norm(q1);
        __builtin_amdgcn_sched_barrier(0);
        TS2D_LOAD_W(1, 0, 1)
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int it = 0; it < MAXU; ++it) load_unit(q1, unit_word(it), it);
        padm_nx1 = q1.padm;
        advance(nx2);
    }
    TS2D_STAMP_AT(a.prof, 6)
    lds_barrier();
    TS2D_STAMP_AT(a.prof, 0)

    // ---- lane constants of the MFMA phase: output pixel (2 wm + mt, r) reads patch row 2 (2 wm + mt) + dy, slot (dx & 1) 33 + r + (dx >> 1)
    const int abase = h * kS2Plane + ((4 * wm) * kS2PW + r) * 16;      // + mt * 2 * 66 * 16 + part * 2 * Plane + tap offset

    f32x16 acc_t[2][NTW];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int nt = 0; nt < NTW; ++nt)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc_t[mt][nt][i] = 0.f;

    if (!(a.dbg & 512)) { if (w >= 4) __builtin_amdgcn_s_setprio(1); }      // static issue priority for waves 4-7 (kernels_f16x3_qp.h)
    const int nitems = ntl * nchunks;
    int pend = -1;                                         // statistics of a finished tile waiting for the item barrier: its entry in a.part
    // one (tile, chunk) item; P = its parity in the stream = patch buffer = ring slot of tap 0
    auto item = [&](auto parity) __attribute__((always_inline)) {
        constexpr int P = decltype(parity)::value;
        const unsigned char* pa = smem8 + P * kS2pPatch + abase;
        unsigned char* pb_next = smem8 + (P ^ 1) * kS2pPatch;
        const unsigned padm = padm_nx1;
        const Req rq = request(nx2);                       // the item after next: each unit re-requested right behind its conversion
        padm_nx1 = rq.padm;
        f32x16 acc_c[2][NTW];                              // fresh accumulator per chunk (accuracy)
        half8 fa[2][2][2];                                 // [buffer][mt][hi, lo]
#define TS2D_LOAD_A(BUF, TAP, PART) { \
        constexpr int toff_ = (((TAP) / 3) * kS2PW + (((TAP) % 3) & 1) * 33 + (((TAP) % 3) >> 1)) * 16; \
        _Pragma("unroll") for (int mt = 0; mt < 2; ++mt) \
            fa[BUF][mt][PART] = *reinterpret_cast<const half8*>(pa + mt * 2 * kS2PW * 16 + (PART) * 2 * kS2Plane + toff_); }
        // tap T: A fragments of tap T+1 from LDS, MFMAs (ring slot (T + P) & 1), conversion of unit T of item i+1 between them; behind the last
        // MFMA the weights of tap T+2 (taps 7, 8: taps 0, 1 of item i+1) into the slot just used, then unit T of item i+2
#define TS2D_TAP(T) { constexpr int cur_ = (T) & 1, sl_ = ((T) + P) & 1; \
        _Pragma("unroll") for (int mt = 0; mt < 2; ++mt) _Pragma("unroll") for (int nt = 0; nt < NTW; ++nt) \
            acc_c[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fa[cur_][mt][1], rb[sl_][nt][0], (T) == 0 ? kZero16 : acc_c[mt][nt], 0, 0, 0); \
        __builtin_amdgcn_sched_barrier(0); \
        if constexpr ((T) + 1 < 9) TS2D_LOAD_A(cur_ ^ 1, (T) + 1, 1) \
        _Pragma("unroll") for (int mt = 0; mt < 2; ++mt) _Pragma("unroll") for (int nt = 0; nt < NTW; ++nt) \
            acc_c[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fa[cur_][mt][0], rb[sl_][nt][1], acc_c[mt][nt], 0, 0, 0); \
        const unsigned uw_ = unit_word(T); \
        convert(uw_, (T), pb_next, padm); \
        if constexpr ((T) == 8) load_norm(rq); \
        _Pragma("unroll") for (int mt = 0; mt < 2; ++mt) _Pragma("unroll") for (int nt = 0; nt < NTW; ++nt) \
            acc_c[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fa[cur_][mt][0], rb[sl_][nt][0], acc_c[mt][nt], 0, 0, 0); \
        __builtin_amdgcn_sched_barrier(0); \
        if constexpr ((T) + 1 < 9) TS2D_LOAD_A(cur_ ^ 1, (T) + 1, 0) \
        if constexpr ((T) + 2 < 9) TS2D_LOAD_W(sl_, cur.c, (T) + 2) else TS2D_LOAD_W(sl_, nx1.c, (T) + 2 - 9) \
        load_unit(rq, uw_, (T)); \
        __builtin_amdgcn_sched_barrier(0); }
        TS2D_LOAD_A(0, 0, 0) TS2D_LOAD_A(0, 0, 1)
        TS2D_TAP(0) TS2D_TAP(1) TS2D_TAP(2) TS2D_TAP(3) TS2D_TAP(4) TS2D_TAP(5) TS2D_TAP(6) TS2D_TAP(7) TS2D_TAP(8)
#undef TS2D_TAP
#undef TS2D_LOAD_A
        TS2D_STAMP_AT(a.prof, 5)
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
            for (int nt = 0; nt < NTW; ++nt) acc_t[mt][nt] += acc_c[mt][nt];
        TS2D_STAMP_AT(a.prof, 3)

        if (cur.c == nchunks - 1) {                        // (uniform) the tile is complete; the next items' staging is in flight
            // ---- epilogue: C/D map of the 32x32 MFMA: column = lane & 31 (output channel), row = (i & 3) + 8 (i >> 2) + 4 h (pixel ox)
            int nimg0, tyi, txi, tin;
            tile_origin(cur.k, nimg0, tyi, txi, tin);
            const int ty0 = tyi * 8, tx0 = txi * 32;
            int le = tid;                                  // (opaque: the epilogue's lane constants are not hoisted into registers of the tap stream)
            asm volatile("" : "+v"(le));
            const int r = le & 31, h = (le >> 5) & 1;
            const float oscale = *a.oscale;
            const size_t img_el = (size_t)a.Ht * a.Wt * a.Cout;
            const auto rsd = __builtin_amdgcn_make_buffer_rsrc(reinterpret_cast<float*>(a.dst) + (size_t)nimg0 * img_el, 0, (int)(img_el * 4), 0x00020000);
            float st_s[NTW], st_q[NTW], st_k[NTW];
            float bvs[NTW];       // every bias value before the first store: a load issued between stores waits (in-order vmcnt) for the stores ahead of it
#pragma unroll
            for (int nt = 0; nt < NTW; ++nt) bvs[nt] = a.bias[n0col + wn * (BN / 2) + nt * 32 + r];
#pragma unroll
            for (int nt = 0; nt < NTW; ++nt) {
                const int co = n0col + wn * (BN / 2) + nt * 32 + r;
                const float bv = bvs[nt];
                const float kv = stat_pivot(round_act<float>(__builtin_fmaf(acc_t[0][nt][0], oscale, bv)));      // shifted statistics (kernels.h)
                float s = 0.f, q = 0.f;
#pragma unroll
                for (int mt = 0; mt < 2; ++mt) {
                    const int oy = ty0 + 2 * wm + mt, ox = tx0 + 4 * h;
                    const unsigned voff = (unsigned)(((oy * a.Wt + ox) * a.Cout + co) * 4);
#pragma unroll
                    for (int i2 = 0; i2 < 16; ++i2) {
                        const unsigned soff = (unsigned)((((i2 & 3) + 8 * (i2 >> 2)) * a.Cout) * 4);      // scalar
                        float v = __builtin_fmaf(acc_t[mt][nt][i2], oscale, bv);
                        buffer_store_act<float>(v, rsd, voff, soff);
                        const float d = round_act<float>(v) - kv;                        // statistics of what is stored
                        s += d; q = __builtin_fmaf(d, d, q);
                        acc_t[mt][nt][i2] = 0.f;
                    }
                }
                st_s[nt] = s; st_q[nt] = q; st_k[nt] = kv;
            }
            float* red = reinterpret_cast<float*>(smem8 + kS2pRed);      // [wm 4][column BN] x (S, Q, K, n)
#pragma unroll
            for (int nt = 0; nt < NTW; ++nt) {
                float s = st_s[nt], q = st_q[nt];
                s += __shfl_xor(s, 32); q += __shfl_xor(q, 32);
                if (h == 0) stat_wave_put(red, wm * BN + wn * (BN / 2) + nt * 32 + r, s, q, st_k[nt], 64.f);
            }
            // the cross-wave merge waits for the item's own barrier (conv3x3_f16x3_qp); with two chunks or more per tile (dispatch) `red` is
            // not written again before the merge of this tile has read it
            pend = (nimg0 * tpi + tin) * a.Cout + n0col;
            TS2D_STAMP_AT(a.prof, 4)
        }
        advance(cur); advance(nx1); advance(nx2);
        lds_barrier();                                     // LDS only: the patch requests and the ring stay in flight across it
        TS2D_STAMP_AT(a.prof, 1)
        if (pend >= 0) {                                   // (uniform)
            if (tid < BN) stat_tile_store(reinterpret_cast<const float*>(smem8 + kS2pRed), 4, BN, tid, a.part + ((size_t)pend + tid) * 4);
            pend = -1;
        }
    };
    // Pairs of items with ONE exit at the bottom, the odd stream's last item peeled: hipcc counts the ring's waits over every path of the
    // control-flow graph, and a loop that can be left behind an even item has - after structurisation - a path from an even item to an
    // even item that never runs but shortens every counted wait of tap 0.
    int i = 0;
    for (; i + 1 < nitems; i += 2) {
        item(S2pParity<0>{});
        item(S2pParity<1>{});
    }
    if (i < nitems) item(S2pParity<0>{});
#undef TS2D_LOAD_W
    TS2D_PROF_FLUSH(a.prof)
}

}  // namespace ts2d
