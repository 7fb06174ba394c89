// CDNA4 (gfx950) kernels of the 2-D U-Net hot path.  DESIGN.md section 4 describes each kernel, its data layout
// and the roofline that bounds it.  All activations are NHWC fp32 in HBM; a conv writes its RAW output
// (conv + bias, before InstanceNorm) exactly once and the InstanceNorm + LeakyReLU of that tensor is applied by
// the CONSUMER while it stages its input tile into LDS, from per-(n,c) scale/shift vectors.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "tile_dims.h"
#include "device_tables.h"      // kSigmoidHalfThreshold

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

namespace ts2d {

// Workgroup barrier for an exchange through LDS: waits for this wave's LDS operations only.  __syncthreads() also fences global
// memory - after an epilogue's output stores that is s_waitcnt vmcnt(0), the whole HBM write latency of the tile, spent with the
// matrix pipe idle (in-kernel stamps, gpurun r2 upc_ph: 30-36 % of a level-0 / level-1 workgroup's life).  One asm statement,
// so that no memory operation moves across it.  (Never between an LDS-DMA and the reads of what it wrote.)
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// C operand of the first MFMA into a fresh accumulator: the inline constant 0 (zeroing 64 registers per chunk costs 64 VALU issues)
constexpr f32x16 kZero16 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};

// In-kernel phase stamps (diagnostic runs, TS2D_DBG=256): wave 0 of every workgroup adds the shader-clock cycles between
// consecutive stamps to slot I of its op's counters (64 sets of 8, picked by block index); slot 7 counts workgroups.  PROF is the pointer (nullptr in production:
// one scalar compare per stamp).  This is how the serialised epilogue of conv3x3_upc was found (gpurun r2 upc_ph3).
#define TS2D_PROF_DECL(PROF) long long tacc_[7] = {0, 0, 0, 0, 0, 0, 0}, tlast_ = (PROF) ? (long long)__builtin_readcyclecounter() : 0
#define TS2D_STAMP_AT(PROF, I) if (PROF) { const long long t_ = (long long)__builtin_readcyclecounter(); tacc_[I] += t_ - tlast_; tlast_ = t_; }
#define TS2D_PROF_FLUSH(PROF) if ((PROF) && threadIdx.x == 0) {       /* 64 slot sets per op: no hot address */ \
        unsigned long long* p_ = (PROF) + (blockIdx.x & 63) * 8; \
        _Pragma("unroll") for (int i_ = 0; i_ < 7; ++i_) atomicAdd(p_ + i_, (unsigned long long)tacc_[i_]); \
        atomicAdd(p_ + 7, 1ull); }


// ------------------------------------------------------------------------------------------------------------
// InstanceNorm partial statistics as SHIFTED sums (round 3; SURVEY section 7 "InstanceNorm numerics").
// A tile's partial for one channel is the float4 (S, Q, K, n):  S = sum(v - K), Q = sum((v - K)^2) over the n values v of the
// tile AS STORED (after the bias, after rounding to the storage type), K = a pivot taken from the tile itself (the value of one of
// its pixels).  Plain sum(v), sum(v^2) in fp32 lose (mean / sigma)^2 of their digits when var = E[v^2] - E[v]^2 is formed - a conv bias of
// 100 sigma, or a network input with an offset, costs 1e-3 on the normalised activations; torch computes the mean first and then
// sum((x - mean)^2).  With the pivot the fp32 sums run over deviations of the size of sigma whatever the mean is, and everything that
// involves K itself happens in double in finalize_stats_t.  Cost: one v_sub_f32 per output element in the epilogue, 16 instead of 8
// bytes per (tile, channel).  Deterministic: fixed summation order, no atomics, the pivot depends on the slice's own data only.
// Wave-level protocol (32x32 MFMA layouts: channel = lane & 31, both lane halves hold pixels of that channel):
//   kv = stat_pivot(first stored value of lane half 0);  per element: d = v - kv; s += d; q = fma(d, d, q);
//   stat_wave_put(red, w * BN + column, s, q, kv, n)  [h == 0 lanes, after adding the other half];  barrier;
//   stat_tile_store(red, waves, BN, column, part entry)  [BN threads]: waves rebased onto wave 0's pivot, all terms of size sigma.
__device__ __forceinline__ float stat_pivot(float v_first) { return __shfl(v_first, (int)(threadIdx.x & 31)); }   // lane r of half 0 -> both halves
__device__ __forceinline__ void stat_wave_put(float* red, int slot, float s, float q, float kv, float n) {
    *reinterpret_cast<f32x4*>(red + 4 * slot) = f32x4{s, q, kv, n};
}
__device__ __forceinline__ void stat_tile_store(const float* red, int nwaves, int bn, int col, float* part_entry) {
    f32x4 a = *reinterpret_cast<const f32x4*>(red + 4 * col);
    for (int ww = 1; ww < nwaves; ++ww) {
        const f32x4 b = *reinterpret_cast<const f32x4*>(red + 4 * (ww * bn + col));
        const float d = b[2] - a[2];                                   // pivot of wave ww relative to wave 0's: a difference of two samples
        a[1] += b[1] + d * (2.f * b[0] + b[3] * d);                      // sum((v - K0)^2) = sum((v - Kw)^2) + 2 d sum(v - Kw) + n d^2
        a[0] += b[0] + b[3] * d;
        a[3] += b[3];
    }
    *reinterpret_cast<f32x4*>(part_entry) = a;
}

// The library is built WITHOUT packed fp32 VALU instructions (csrc/Makefile: DEVFLAGS); a kernel that is faster with them opts back in.  (A kernel's
// lambdas and the shared helpers keep the library default: a callee with fewer target features inlines into a caller with more.)
#if defined(__HIP_DEVICE_COMPILE__)
#define TS2D_PACKED_F32 __attribute__((target("packed-fp32-ops")))
#else
#define TS2D_PACKED_F32      // (the host pass of hipcc parses the kernels too and does not know the feature)
#endif

// (kBlock, kBM - threads and output pixels per workgroup tile: tile_dims.h)

// n / d for 0 <= n < 2^22 by the float reciprocal inv_d = 1.0f / d (correctly rounded, computed on the host): exact, because
// (n + 0.5) / d is at least 0.5 / d away from an integer and the two roundings move it by less than (n + 0.5) 2^-23 / d.
__device__ __forceinline__ int fdiv(int n, float inv_d) { return (int)(((float)n + 0.5f) * inv_d); }
// n / d for wave-uniform n with n * d < 2^32 by the multiplier mg = ceil(2^32 / d) (host; 0 stands for d == 1): ONE scalar
// multiply-high.  Exact: mg d = 2^32 + e with 0 <= e < d, so n mg / 2^32 = n / d + n e / (d 2^32) and n e < 2^32 keeps the floor.
__device__ __forceinline__ int udiv_magic(int n, unsigned mg) { return mg ? (int)__umulhi((unsigned)n, mg) : n; }

// ------------------------------------------------------------------------------------------------------------
// Implicit-GEMM convolution on the fp32 MFMA (v_mfma_f32_32x32x2_f32: exact fp32 FMA chain).
//   GEMM view: M = output pixels, N = output channels, K = TAPS * Cin.
//   TAPS = 9 : Conv2d 3x3 pad 1 stride (SY, SX)     (virtual concat via src0/src1)
//   TAPS = 1 : ConvTranspose2d kernel = stride = (KA, KB) as a GEMM with N = KA*KB*Cout (tap (a,b) = n / Cout)   
// Workgroup tile: 256 pixels = NIMG images x TH x TW (powers of two) x BN channels; wave w owns pixels
// [64w, 64w+64) = 2 MFMA row tiles, all BN columns.  Per Cin chunk of CK channels the (haloed) input patch is
// staged ONCE into LDS (normalised + activated on the way) and reused by all taps.
// ------------------------------------------------------------------------------------------------------------
struct ConvArgs {
    const float* src0; const float* sc0; const float* sh0; int C0;   // sc0 == nullptr: identity (no norm/act)
    const float* src1; const float* sc1; const float* sh1; int C1;   // second half of the virtual concat (or C1=0)
    const float* wp;      // packed weights [chunk][tap][CK/8][N][8]
    const float* bias;    // [Cout_real]
    float* dst;           // raw output NHWC
    float* part;          // partial statistics [n][tile][Cout][2] or nullptr
    int B, Hin, Win;      // input tensor dims
    int Ht, Wt;           // tile-space dims (= output dims for conv, = input dims for convT)
    int N;                // GEMM N (= Cout for conv, 4*Cout for convT)
    int Cout;             // real output channels (dst channel stride)
    int TH, TW, NIMG;     // pixel tile = NIMG images x TH x TW pixels (NIMG * TH * TW <= 256; any extents - round 5: a level of 80 x 48 or
                          // 28 x 36 pixels gets tiles that divide it, e.g. 5 x 48 or 7 x 36, instead of idle rows in power-of-two tiles)
    float inv_tw, inv_thw;       // 1 / TW, 1 / (TH * TW) for tile_row()
    int lgTH, lgTW;       // log2 of TH / TW when BOTH are powers of two, else -1 (the fast epilogues address a tile row with shifts)
    int tiles_x, tiles_y; // tiles per image
    int n_mtiles, n_ctiles;
    unsigned mg_tx, mg_tpi;      // ceil(2^32 / tiles_x), ceil(2^32 / (tiles_x * tiles_y)) (0 for a divisor of 1): the persistent kernels decode a tile
                                 // number per item with udiv_magic() - scalar multiplies, any tile count (the power-of-two gate of rounds 1-4 is gone)
    int PH, PW;           // staged patch dims per image
    int KA, KB;           // transposed conv (conv_mfma_f32, TAPS == 1): kernel = stride (along H, along W); N = KA * KB * Cout
    float slope;
    const void* wph;      // split-fp16 packed weights [chunk][tap][N][16 hi | 16 lo] (f16x3 kernel only)
    int ksplit;           // split-K: blockIdx.y = K slice; slice s writes un-biased partials to dst + s * kslice_stride
    long long kslice_stride;
    unsigned long long* prof;   // diagnostic (TS2D_DBG=256): in-kernel phase cycle counters of this op, 8 entries, or nullptr
    int dbg;              // timing ablations of diagnostic runs (TS2D_DBG; 0 in production): bit 0 = skip the MFMA phase, bit 1 = skip the
                          // patch conversion, bit 2 = skip the weight staging
    const float* oscale;  // device scalar: 1 / (power-of-two weight pre-scale); lives in the weight arena so that it
                          // travels with the multi-GPU weight broadcast (f16x3 kernel only)
};

// row m of a pixel tile -> (image inside the tile, y, x inside the image's TH x TW part); rows past NIMG * TH * TW give il >= NIMG
__device__ __forceinline__ void tile_row(const ConvArgs& a, int m, int& il, int& ty, int& tx) {
    il = fdiv(m, a.inv_thw);
    const int rem = m - il * (a.TH * a.TW);
    ty = fdiv(rem, a.inv_tw); tx = rem - ty * a.TW;
}

template <int SY, int SX, int CK>
struct ConvCfg {
    static constexpr int MAXP = (SY == 1 && SX == 1) ? 576 : 1296;          // max patch pixels (16 images of 4x4)
    static constexpr int MAXIT = (MAXP * (CK / 4) + kBlock - 1) / kBlock;   // staging iterations per thread
};

// Activation STORAGE type ST: float (the fp32-parity modes) or _Float16 ("mixed fp16": fp16 storage).
template <typename ST> __device__ __forceinline__ float round_act(float v) { return (float)(ST)v; }
template <typename ST> __device__ __forceinline__ void store_act(void* base, size_t off, float v) { reinterpret_cast<ST*>(base)[off] = (ST)v; }
template <typename ST> __device__ __forceinline__ f32x4 load_act4(const void* base, size_t off);
template <> __device__ __forceinline__ f32x4 load_act4<float>(const void* base, size_t off) {
    return *reinterpret_cast<const f32x4*>(reinterpret_cast<const float*>(base) + off);
}
template <> __device__ __forceinline__ f32x4 load_act4<_Float16>(const void* base, size_t off) {
    typedef _Float16 half4_t __attribute__((ext_vector_type(4)));
    const half4_t hv = *reinterpret_cast<const half4_t*>(reinterpret_cast<const _Float16*>(base) + off);
    return f32x4{(float)hv[0], (float)hv[1], (float)hv[2], (float)hv[3]};
}

// SY, SX: stride along H / W (1 or 2 each: nnU-Net pools every axis separately, so a plan may end in (2, 1) / (1, 2) stages; those -
// in every precision mode - and the whole exact mode run here).  ST = _Float16: the arithmetic CONTRACT of the 16-bit mode on the fp32
// matrix core (operands rounded to fp16 - weights once, activations after the normalisation, LeakyReLU in fp16 - fp32 accumulation,
// output stored as fp16, statistics of the stored values).  TAPS == 1: ConvTranspose2d with kernel = stride = (a.KA, a.KB).
template <int TAPS, int SY, int SX, int CK, int BN, int EPI, typename ST = float>
__global__ __launch_bounds__(kBlock, 2) void conv_mfma_f32(const ConvArgs a) {
    constexpr int KK = CK / 8, NT = BN / 32, PSTR = CK + 4, QPP = CK / 4;
    constexpr int PAD = (TAPS == 9) ? 1 : 0;
    constexpr int MAXIT = ConvCfg<SY, SX, CK>::MAXIT;
    constexpr bool F16 = sizeof(ST) == 2;
    extern __shared__ __attribute__((aligned(16))) float smem[];

    // ---- XCD-aware block -> tile map: blocks b and b+8 share an XCD (and its L2); consecutive blocks of one
    //      XCD walk the channel tiles of the SAME pixel tile so the input patch is re-read from that L2.
    const int bid = blockIdx.x;
    const int xcd = bid & 7, q8 = bid >> 3;
    const int mtile = (q8 / a.n_ctiles) * 8 + xcd;
    const int ctile = q8 % a.n_ctiles;
    if (mtile >= a.n_mtiles) return;                       // uniform: whole workgroup leaves before any barrier
    const int n0col = ctile * BN;

    const int NIMG = a.NIMG;
    const int tpi = a.tiles_x * a.tiles_y;
    const int grp = mtile / tpi, tin = mtile - grp * tpi;
    const int tyi = tin / a.tiles_x, txi = tin - tyi * a.tiles_x;
    const int nimg0 = grp * NIMG;
    const int ty0 = tyi * a.TH, tx0 = txi * a.TW;

    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int r = lane & 31, h = lane >> 5;

    const int PHW = a.PH * a.PW;
    const int P = PHW * NIMG;
    float* sA = smem;
    float* sB = smem + ((P * PSTR + 3) & ~3);

    // ---- per-thread staging plan (same for every chunk): source pixel index or -1, and the local image.
    int goff[MAXIT];
    unsigned long long imgbits = 0;
    const int total4 = P * QPP;
#pragma unroll
    for (int it = 0; it < MAXIT; ++it) {
        const int idx = tid + it * kBlock;
        int g = -1;
        if (idx < total4) {
            const int pp = idx / QPP;
            const int il = pp / PHW, rem = pp - il * PHW;
            const int py = rem / a.PW, px = rem - py * a.PW;
            const int n = nimg0 + il, iy = ty0 * SY - PAD + py, ix = tx0 * SX - PAD + px;
            if (n < a.B && iy >= 0 && iy < a.Hin && ix >= 0 && ix < a.Win) g = (n * a.Hin + iy) * a.Win + ix;
            imgbits |= (unsigned long long)il << (4 * it);
        }
        goff[it] = g;
    }
    const int qch = (tid % QPP) * 4;   // this thread's channel quad inside a chunk (kBlock % QPP == 0)

    // ---- this lane's A-fragment base addresses (one per MFMA row tile)
    int abase[2];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) {
        const int m = 64 * w + 32 * mt + r;
        int il, ty, tx;
        tile_row(a, m, il, ty, tx);
        // rows past the tile's NIMG*TH*TW pixels (tiny images: NIMG is capped at 16) read a valid dummy address
        abase[mt] = (il < NIMG ? (il * PHW + ty * SY * a.PW + tx * SX) * PSTR : 0) + 4 * h;
    }
    const int bbase = r * 8 + 4 * h;

    f32x16 acc_t[2][NT];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc_t[mt][nt][i] = 0.f;

    const int nchunks = (a.C0 + a.C1) / CK;
    for (int ch = 0; ch < nchunks; ++ch) {
        int cb = ch * CK;
        const float* src; const float* sc; const float* sh; int C;
        if (cb < a.C0) { src = a.src0; sc = a.sc0; sh = a.sh0; C = a.C0; }
        else { cb -= a.C0; src = a.src1; sc = a.sc1; sh = a.sh1; C = a.C1; }
        const int coff = cb + qch;

        __syncthreads();   // previous chunk's LDS reads are done
        // ---- stage the input patch: global -> regs -> (x*scale+shift, LeakyReLU) -> LDS; zeros outside the image
        {
            f32x4 v[MAXIT];
#pragma unroll
            for (int it = 0; it < MAXIT; ++it) {
                v[it] = f32x4{0.f, 0.f, 0.f, 0.f};
                if (goff[it] >= 0) v[it] = load_act4<ST>(src, (size_t)goff[it] * C + coff);
            }
            if (sc != nullptr) {
                f32x4 s1 = f32x4{1.f, 1.f, 1.f, 1.f}, s2 = f32x4{0.f, 0.f, 0.f, 0.f};
                if (NIMG == 1 && nimg0 < a.B) {
                    s1 = *reinterpret_cast<const f32x4*>(sc + (size_t)nimg0 * C + coff);
                    s2 = *reinterpret_cast<const f32x4*>(sh + (size_t)nimg0 * C + coff);
                }
#pragma unroll
                for (int it = 0; it < MAXIT; ++it) {
                    if (goff[it] >= 0) {
                        if (NIMG != 1) {
                            const int n = nimg0 + (int)((imgbits >> (4 * it)) & 15);
                            s1 = *reinterpret_cast<const f32x4*>(sc + (size_t)n * C + coff);
                            s2 = *reinterpret_cast<const f32x4*>(sh + (size_t)n * C + coff);
                        }
                        f32x4 t = v[it] * s1 + s2;
                        if constexpr (F16) {      // the operand the 16-bit mode multiplies: fp16(normalised), LeakyReLU in fp16
                            const float sl = (float)(_Float16)a.slope;
#pragma unroll
                            for (int e = 0; e < 4; ++e) { const float y = (float)(_Float16)t[e]; t[e] = fmaxf(y, (float)(_Float16)(y * sl)); }
                        } else {
#pragma unroll
                            for (int e = 0; e < 4; ++e) t[e] = t[e] > 0.f ? t[e] : t[e] * a.slope;
                        }
                        v[it] = t;
                    }
                }
            }
#pragma unroll
            for (int it = 0; it < MAXIT; ++it) {
                const int idx = tid + it * kBlock;
                if (idx < total4) *reinterpret_cast<f32x4*>(sA + (idx / QPP) * PSTR + qch) = v[it];
            }
        }
        // ---- stage this chunk's weights for columns [n0col, n0col+BN): LDS image [tap][kk][BN][8]
        {
            constexpr int W4 = TAPS * KK * BN * 2;
            const float* wsrc = a.wp + (size_t)ch * TAPS * KK * a.N * 8 + (size_t)n0col * 8;
#pragma unroll
            for (int it = 0; it < (W4 + kBlock - 1) / kBlock; ++it) {
                const int idx = tid + it * kBlock;
                if (idx < W4) {
                    const int tk = idx / (BN * 2), rr = idx - tk * (BN * 2);
                    f32x4 wv = *reinterpret_cast<const f32x4*>(wsrc + (size_t)tk * a.N * 8 + rr * 4);
                    if constexpr (F16) {
#pragma unroll
                        for (int e = 0; e < 4; ++e) wv[e] = (float)(_Float16)wv[e];
                    }
                    *reinterpret_cast<f32x4*>(sB + idx * 4) = wv;
                }
            }
        }
        __syncthreads();

        // ---- MFMA: fresh accumulator per chunk (bounded fp32 chain length, see DESIGN.md "accumulation order")
        f32x16 acc_c[2][NT];
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt)
#pragma unroll
                for (int i = 0; i < 16; ++i) acc_c[mt][nt][i] = 0.f;
#pragma unroll
        for (int tap = 0; tap < TAPS; ++tap) {
            const int toff = (TAPS == 9) ? ((tap / 3) * a.PW + (tap % 3)) * PSTR : 0;
#pragma unroll
            for (int kk = 0; kk < KK; ++kk) {
                f32x4 av[2], bv[NT];
#pragma unroll
                for (int mt = 0; mt < 2; ++mt) av[mt] = *reinterpret_cast<const f32x4*>(sA + abase[mt] + toff + kk * 8);
#pragma unroll
                for (int nt = 0; nt < NT; ++nt)
                    bv[nt] = *reinterpret_cast<const f32x4*>(sB + ((tap * KK + kk) * BN + nt * 32) * 8 + bbase);
#pragma unroll
                for (int e = 0; e < 4; ++e)
#pragma unroll
                    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                        for (int nt = 0; nt < NT; ++nt)
                            acc_c[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[mt][e], bv[nt][e], acc_c[mt][nt], 0, 0, 0);
            }
        }
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) acc_t[mt][nt] += acc_c[mt][nt];
    }

    // ---- epilogue.  C/D map of the 32x32 MFMA: column = lane & 31, row = (i & 3) + 8 * (i >> 2) + 4 * (lane >> 5).
    float st_s[NT], st_q[NT], st_k[NT], st_n[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) { st_s[nt] = 0.f; st_q[nt] = 0.f; st_n[nt] = 0.f; }
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        const int col = n0col + nt * 32 + r;
        int co = col, oa = 0, ob = 0;
        if (EPI == 1) { const int ab = (n0col + nt * 32) / a.Cout; co = col - ab * a.Cout; oa = ab / a.KB; ob = ab - oa * a.KB; }
        const float bv = a.bias[co];
        const float kv = stat_pivot(round_act<ST>(acc_t[0][nt][0] + bv));      // (a pixel outside the image is still a finite value: fine as a pivot)
        st_k[nt] = kv;
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) {
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int row = (i & 3) + 8 * (i >> 2) + 4 * h;
                const int m = 64 * w + 32 * mt + row;
                int il, ty, tx;
                tile_row(a, m, il, ty, tx);
                const int n = nimg0 + il, oy = ty0 + ty, ox = tx0 + tx;
                if (il < NIMG && n < a.B && oy < a.Ht && ox < a.Wt) {
                    const float v = acc_t[mt][nt][i] + bv;
                    if (EPI == 0) {
                        store_act<ST>(a.dst, ((size_t)(n * a.Ht + oy) * a.Wt + ox) * a.Cout + co, v);
                        const float d = round_act<ST>(v) - kv;                 // statistics of what is stored
                        st_s[nt] += d; st_q[nt] = __builtin_fmaf(d, d, st_q[nt]); st_n[nt] += 1.f;
                    } else {
                        store_act<ST>(a.dst, ((size_t)(n * a.KA * a.Ht + a.KA * oy + oa) * (a.KB * a.Wt) + a.KB * ox + ob) * a.Cout + co, v);
                    }
                }
            }
        }
    }
    if (EPI == 0 && a.part != nullptr) {   // fused InstanceNorm partial statistics (host guarantees NIMG == 1)
        lds_barrier();
        float* red = smem;                 // [4 waves][BN][4]
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            float s = st_s[nt], q = st_q[nt], n = st_n[nt];
            s += __shfl_xor(s, 32); q += __shfl_xor(q, 32); n += __shfl_xor(n, 32);
            if (h == 0) stat_wave_put(red, w * BN + nt * 32 + r, s, q, st_k[nt], n);
        }
        lds_barrier();
        if (tid < BN) stat_tile_store(red, 4, BN, tid, a.part + ((size_t)(nimg0 * tpi + tin) * a.Cout + n0col + tid) * 4);
    }
}

// ------------------------------------------------------------------------------------------------------------
// InstanceNorm statistics -> per-(n,c) scale/shift.  scale = gamma * rstd, shift = beta - mean * scale,
// biased variance, eps inside the sqrt, combined in double.
// ------------------------------------------------------------------------------------------------------------
// (a) from the conv epilogue's per-tile shifted partials (S, Q, K, n) - see "InstanceNorm partial statistics" above.  Grid (B, C/32), 32 TL threads = TL tile lanes x 32
// channels (TL = 32 for the levels with hundreds of tiles per image: a 64-block grid is latency-bound, so each block brings 1024
// threads; TL = 8 otherwise); fixed summation order -> bit-reproducible, and independent of the batch a slice travels in.
template <int TL, int CG = 32>      // CG channels per block (8: four times the blocks for the 32- and 64-channel levels, whose grids would leave most CUs idle)
__global__ __launch_bounds__(CG * TL) void finalize_stats_t(const float* __restrict__ part, int ntiles, int C, int B, int HW,
                                                           const float* __restrict__ gamma, const float* __restrict__ beta,
                                                           float eps, float* __restrict__ scale, float* __restrict__ shift) {
    const int n = blockIdx.x, cl = threadIdx.x % CG, c = blockIdx.y * CG + cl, tl = threadIdx.x / CG;
    __shared__ double rs[TL][CG], rq[TL][CG];
    const f32x4* p = reinterpret_cast<const f32x4*>(part) + (size_t)n * ntiles * C + c;
    double s = 0.0, q = 0.0;
    // (S, Q, K, n) -> sum(v), sum(v^2): everything that involves the pivot, in double.  Eight partials are REQUESTED before the first
    // is added (same order of additions): the plain loop was one memory round trip per partial - 17-31 us per level-0 launch
    for (int t0 = tl; t0 < ntiles; t0 += 8 * TL) {
        f32x4 v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int t = t0 + j * TL;
            v[j] = p[(size_t)(t < ntiles ? t : tl) * C];
        }
#pragma unroll
        for (int j = 0; j < 8; ++j)
            if (t0 + j * TL < ntiles) {
                const double k = (double)v[j][2], nn = (double)v[j][3];
                s += (double)v[j][0] + nn * k; q += (double)v[j][1] + k * (2.0 * (double)v[j][0] + nn * k);
            }
    }
    rs[tl][cl] = s; rq[tl][cl] = q;
    __syncthreads();
    if (tl == 0) {
        for (int k = 1; k < TL; ++k) { s += rs[k][cl]; q += rq[k][cl]; }
        const double mean = s / HW;
        double var = q / HW - mean * mean;
        var = var > 0.0 ? var : 0.0;
        const double rstd = 1.0 / sqrt(var + (double)eps);
        const double g = gamma[c];
        scale[(size_t)n * C + c] = (float)(g * rstd);
        shift[(size_t)n * C + c] = (float)((double)beta[c] - mean * g * rstd);
    }
}

// (b) directly from the raw NHWC tensor (small layers whose tile spans several images): block per (n, 32 channels).
template <typename ST>
__global__ __launch_bounds__(256) void stats_direct(const ST* __restrict__ x, int C, int HW,
                                                   const float* __restrict__ gamma, const float* __restrict__ beta,
                                                   float eps, float* __restrict__ scale, float* __restrict__ shift) {
    const int n = blockIdx.x, c = blockIdx.y * 32 + (threadIdx.x & 31), pl = threadIdx.x >> 5;
    __shared__ double rs[8][32], rq[8][32];
    double s = 0.0, q = 0.0;
    for (int p = pl; p < HW; p += 8) {
        const double v = (double)(float)x[((size_t)n * HW + p) * C + c];
        s += v; q += v * v;
    }
    rs[pl][threadIdx.x & 31] = s; rq[pl][threadIdx.x & 31] = q;
    __syncthreads();
    if (pl == 0) {
        for (int k = 1; k < 8; ++k) { s += rs[k][threadIdx.x & 31]; q += rq[k][threadIdx.x & 31]; }
        const double mean = s / HW;
        double var = q / HW - mean * mean;
        var = var > 0.0 ? var : 0.0;
        const double rstd = 1.0 / sqrt(var + (double)eps);
        const double g = gamma[c];
        scale[(size_t)n * C + c] = (float)(g * rstd);
        shift[(size_t)n * C + c] = (float)((double)beta[c] - mean * g * rstd);
    }
}

// (c) split-K epilogue for the tiny bottleneck layers: fixed-order sum of the S partial outputs + bias -> raw output,
// and the InstanceNorm scale/shift of that output in the same pass.  Grid (B, C/32), 256 threads = 8 pixel lanes x 32 ch.
template <typename ST, int PL = 8>
__global__ __launch_bounds__(32 * PL) void splitk_reduce_stats(const float* __restrict__ partial, int S, long long slice_stride,
                                                          const float* __restrict__ bias, int C, int HW,
                                                          const float* __restrict__ gamma, const float* __restrict__ beta,
                                                          float eps, ST* __restrict__ dst, float* __restrict__ scale,
                                                          float* __restrict__ shift) {
    const int n = blockIdx.x, cl = threadIdx.x & 31, c = blockIdx.y * 32 + cl, pl = threadIdx.x >> 5;
    __shared__ double rs[PL][32], rq[PL][32];
    const float b = bias[c];
    double s = 0.0, q = 0.0;
    // (PL = 32, round 6: images of 256 ... 1024 pixels under the small-batch split-K - four pixels' partials in flight per thread)
#pragma unroll PL == 32 ? 4 : 1
    for (int p = pl; p < HW; p += PL) {
        const size_t o = ((size_t)n * HW + p) * C + c;
        float v = 0.f;
        for (int k0 = 0; k0 < S; k0 += 8) {             // the partials of 8 splits requested together, added in the fixed order k = 0, 1, ...
            float pk[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) pk[j] = partial[(size_t)(k0 + j < S ? k0 + j : k0) * slice_stride + o];
#pragma unroll
            for (int j = 0; j < 8; ++j) if (k0 + j < S) v += pk[j];
        }
        v += b;
        dst[o] = (ST)v;
        v = (float)(ST)v;
        s += (double)v; q += (double)v * (double)v;
    }
    rs[pl][cl] = s; rq[pl][cl] = q;
    __syncthreads();
    if (pl == 0) {
        for (int k = 1; k < PL; ++k) { s += rs[k][cl]; q += rq[k][cl]; }
        const double mean = s / HW;
        double var = q / HW - mean * mean;
        var = var > 0.0 ? var : 0.0;
        const double rstd = 1.0 / sqrt(var + (double)eps);
        const double g = gamma[c];
        scale[(size_t)n * C + c] = (float)(g * rstd);
        shift[(size_t)n * C + c] = (float)((double)beta[c] - mean * g * rstd);
    }
}

// (d) split-K epilogue for images of >= 256 pixels (round 6: the small-batch split-K of the 16 x 16 ... 128 x 128 levels).  Grid (HW / 256, C / 32, B),
// 256 threads = 8 pixel lanes x 32 channels: fixed-order sum of the S partial outputs + bias -> raw output, and ONE shifted partial (S, Q, K, n = 256) per
// block and channel in the layout of the conv epilogues' tile partials ([n][block][C]); finalize_stats_t turns them into scale / shift.  The pivot is the
// value of the block's first pixel; the value of a pixel and the partial depend on the slice's own data and the split factor only.
template <typename ST>
__global__ __launch_bounds__(256) void splitk_reduce_part(const float* __restrict__ partial, int S, long long slice_stride,
                                                         const float* __restrict__ bias, int C, int HW, ST* __restrict__ dst, float* __restrict__ part) {
    const int blk = blockIdx.x, n = blockIdx.z, cl = threadIdx.x & 31, c = blockIdx.y * 32 + cl, pl = threadIdx.x >> 5;
    __shared__ float rs[8][32], rq[8][32];
    const float b = bias[c];
    auto value = [&](int p) -> float {
        const size_t o = ((size_t)n * HW + p) * C + c;
        float v = 0.f;
        for (int k0 = 0; k0 < S; k0 += 8) {             // the partials of 8 splits requested together, added in the fixed order k = 0, 1, ...
            float pk[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) pk[j] = partial[(size_t)(k0 + j < S ? k0 + j : k0) * slice_stride + o];
#pragma unroll
            for (int j = 0; j < 8; ++j) if (k0 + j < S) v += pk[j];
        }
        return v + b;
    };
    const int p0 = blk * 256;
    const float kv = (float)(ST)value(p0);               // (every pixel lane recomputes the pivot: L1 hits, no barrier)
    float s = 0.f, q = 0.f;
#pragma unroll 4
    for (int i = 0; i < 32; ++i) {
        const int p = p0 + pl + 8 * i;
        const float v = value(p);
        dst[((size_t)n * HW + p) * C + c] = (ST)v;
        const float d = (float)(ST)v - kv;
        s += d; q = __builtin_fmaf(d, d, q);
    }
    rs[pl][cl] = s; rq[pl][cl] = q;
    __syncthreads();
    if (pl == 0) {
        for (int k = 1; k < 8; ++k) { s += rs[k][cl]; q += rq[k][cl]; }
        *reinterpret_cast<f32x4*>(part + (((size_t)n * (HW / 256) + blk) * C + c) * 4) = f32x4{s, q, kv, 256.f};
    }
}

// ------------------------------------------------------------------------------------------------------------
// Boundary layout change: NCHW fp32 [B,C,H,W] -> NHWC with channels zero-padded to CP (multiple of 8).
// ------------------------------------------------------------------------------------------------------------
__global__ void nchw_to_nhwc_pad(const float* __restrict__ x, int C, int HW, long long total, int CP,
                                 float* __restrict__ y) {
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;   // pixel over B*H*W
    if (p >= total) return;
    const long long n = p / HW, o = p - n * HW;
    for (int c0 = 0; c0 < CP; c0 += 4) {
        f32x4 v;
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = (c0 + e < C) ? x[(n * C + c0 + e) * HW + o] : 0.f;
        *reinterpret_cast<f32x4*>(y + p * CP + c0) = v;
    }
}

// ------------------------------------------------------------------------------------------------------------
// Head (SURVEY K7 + A7): InstanceNorm/LeakyReLU of the last decoder conv applied on load, 1x1 conv C -> K + bias,
// fp32 logits written NCHW (the boundary layout [B,K,H,W]) and, optionally, the bit-packed multilabel mask
// sigmoid(logit) > 0.5.  HBM-bound: reads C*4 B and writes K*4 B (+K/8 B) per pixel, all coalesced.
// The predicate: on the ATen CPU kernels the oracle was pinned with, sigmoid(x) > 0.5  <=>  x > 1.5 * 2^-24
// (exhaustive fp32 scan, tests/test_oracle.py); NaN compares false on both sides.
// ------------------------------------------------------------------------------------------------------------
struct HeadArgs {
    const float* src; const float* sc; const float* sh;   // raw NHWC [B,H,W,C] + its scale/shift [B,C]
    const float* w; const float* bias;                     // [K][C], [K]
    const float* wph; const float* oscale;                 // head_mfma32: split-fp16 weight image [ks 2][32][16 hi | 16 lo], 1 / scale
    float* logits; uint32_t* mask;                         // NCHW [B,K,H,W]; [B,K,H,W/32] (either may be nullptr)
    int C, K, HW; long long total;                         // total = B*H*W pixels
    float slope;
    int* nonfinite;                                        // device flag, set when a logit is inf / NaN (ts2d_engine_check)
};

// true for +-inf and NaN
__device__ __forceinline__ bool not_finite(float v) { return !(__builtin_fabsf(v) < __builtin_inff()); }

// Diagnosis pass of ts2d_engine_check: does a tensor hold a non-finite value?  (run only after the head reported one)
template <typename ST>
__global__ void scan_nonfinite(const ST* __restrict__ p, size_t n, int* __restrict__ flag) {
    bool bad = false;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) bad |= not_finite((float)p[i]);
    if (bad) atomicOr(flag, 1);
}

template <int C, typename ST = float>
__global__ __launch_bounds__(256) void head_1x1(const HeadArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* sx = smem;                       // [256][C+1]
    float* sw = smem + 256 * (C + 1);       // [K][C] then bias [K]
    const int tid = threadIdx.x;
    const long long p0 = (long long)blockIdx.x * 256;
    for (int i = tid; i < a.K * C; i += 256) sw[i] = a.w[i];
    for (int i = tid; i < a.K; i += 256) sw[a.K * C + i] = a.bias[i];
    // stage 256 pixels x C channels, coalesced float4, normalise + activate
    constexpr int Q = C / 4;
    for (int idx = tid; idx < 256 * Q; idx += 256) {
        const int pl = idx / Q, c4 = (idx - pl * Q) * 4;
        const long long p = p0 + pl;
        f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
        if (p < a.total) {
            const long long n = p / a.HW;
            if (sizeof(ST) == 4) v = *reinterpret_cast<const f32x4*>(a.src + p * C + c4);
            else {
                typedef _Float16 half4_t __attribute__((ext_vector_type(4)));
                const half4_t hv = *reinterpret_cast<const half4_t*>(reinterpret_cast<const _Float16*>(a.src) + p * C + c4);
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = (float)hv[e];
            }
            const f32x4 s1 = *reinterpret_cast<const f32x4*>(a.sc + n * C + c4);
            const f32x4 s2 = *reinterpret_cast<const f32x4*>(a.sh + n * C + c4);
            v = v * s1 + s2;
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = v[e] > 0.f ? v[e] : v[e] * a.slope;
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) sx[pl * (C + 1) + c4 + e] = v[e];
    }
    __syncthreads();
    const long long p = p0 + tid;
    const bool valid = p < a.total;
    float xr[C];
#pragma unroll
    for (int c = 0; c < C; ++c) xr[c] = sx[tid * (C + 1) + c];
    const long long n = valid ? p / a.HW : 0, o = valid ? p - n * a.HW : 0;
    bool bad = false;
    for (int k = 0; k < a.K; ++k) {
        float acc = 0.f;
#pragma unroll
        for (int c = 0; c < C; ++c) acc = fmaf(xr[c], sw[k * C + c], acc);
        acc += sw[a.K * C + k];
        if (valid && not_finite(acc)) bad = true;
        if (a.logits != nullptr && valid) a.logits[(n * a.K + k) * a.HW + o] = acc;
        if (a.mask != nullptr) {
            const unsigned long long bits = __ballot(valid && acc > kSigmoidHalfThreshold);
            // a wave covers 64 consecutive pixels of one image row segment (HW % 64 == 0, W % 32 == 0)
            if ((tid & 63) == 0 && valid)
                *reinterpret_cast<unsigned long long*>(a.mask + ((n * a.K + k) * a.HW + o) / 32) = bits;
        }
    }
    if (bad && a.nonfinite != nullptr) atomicOr(a.nonfinite, 1);
}

}  // namespace ts2d
