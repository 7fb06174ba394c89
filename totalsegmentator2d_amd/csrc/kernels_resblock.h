// Residual blocks of nnU-Net's ResidualEncoderUNet (BasicBlockD): out = lrelu(norm2(conv2(lrelu(norm1(conv1(x))))) + skip(x)).
// conv1 and conv2 are the engine's ordinary 3x3 blocks (raw output + per-(image, channel) scale / shift); this header holds what is new:
//   pool_proj1x1  the skip path where the widths differ: AvgPool2d(kernel = stride) -> Conv2d 1x1 without bias (-> norm: launch_stats)
//   res_join      t = norm2(conv2) + residual, stored BEFORE the block's LeakyReLU with scale 1 / shift 0, so that every consumer's
//                 load-time lrelu(scale * t + shift) is the block's output, exactly
// Both are per-pixel: a pixel's result depends on its own image only, whatever else is in the batch.
// Storage: fp32 (res_join<float>, pool_proj1x1) or fp16 (res_join<_Float16>, pool_proj1x1_h - the 16-bit mode, behind the option "resf16").
// The 16-bit contract of a residual block (include/ts2d_engine.h, TS2D_PRECISION_F16): every operand value is the half the other 16-bit
// consumers load, a = act16(h(scale * stored + shift)); the normalised conv2 and the residual are fp32, their sum is rounded to half ONCE,
// on the store; a projection multiplies h(pool(a)) with h(w), accumulates in fp32 and stores half, statistics over the stored values.
#pragma once
#include "kernels.h"
#include "kernels_h32.h"      // norm_lrelu_8: the 16-bit consumers' load of eight values

#include <type_traits>

namespace ts2d {

__device__ __forceinline__ f32x4 norm_act4(f32x4 v, f32x4 sc, f32x4 sh, float slope) {
    f32x4 o;
#pragma unroll
    for (int j = 0; j < 4; ++j) { const float t = fmaf(sc[j], v[j], sh[j]); o[j] = t > 0.f ? t : t * slope; }
    return o;
}

// The activated source, average-pooled over the (sy, sx) window whose first pixel is at `p`: summed in row-major order, times 1 / n
// (n = 1, 2 or 4: the product is the quotient, exactly).  `row`: elements from one source row to the next.
__device__ __forceinline__ f32x4 pooled_act4(const float* __restrict__ p, size_t row, int C, int sy, int sx, f32x4 sc, f32x4 sh, float slope, float inv_n) {
    f32x4 s = norm_act4(*reinterpret_cast<const f32x4*>(p), sc, sh, slope);
    for (int dy = 0; dy < sy; ++dy)
        for (int dx = 0; dx < sx; ++dx) {
            if (dy == 0 && dx == 0) continue;
            const f32x4 v = norm_act4(*reinterpret_cast<const f32x4*>(p + dy * row + (size_t)dx * C), sc, sh, slope);
#pragma unroll
            for (int j = 0; j < 4; ++j) s[j] += v[j];
        }
#pragma unroll
    for (int j = 0; j < 4; ++j) s[j] *= inv_n;
    return s;
}

// Eight stored halves of the 16-bit mode as the operand values their consumers multiply, a = act16(h(scale * stored + shift)), pooled as
// above: fp32 sum in row-major order, times 1 / n.  `p`: first pixel of the window, `row` / `C` in elements.
__device__ __forceinline__ void pooled_act8_h(const _Float16* __restrict__ p, size_t row, int C, int sy, int sx, f32x4 sa, f32x4 sb, f32x4 ta, f32x4 tb,
                                              unsigned slope2, float inv_n, float s[8]) {
    for (int dy = 0; dy < sy; ++dy)
        for (int dx = 0; dx < sx; ++dx) {
            const uint4 y = norm_lrelu_8(*reinterpret_cast<const uint4*>(p + dy * row + (size_t)dx * C), sa, sb, ta, tb, slope2);
            const half8 v = __builtin_bit_cast(half8, y);
#pragma unroll
            for (int j = 0; j < 8; ++j) s[j] = (dy == 0 && dx == 0) ? (float)v[j] : s[j] + (float)v[j];
        }
#pragma unroll
    for (int j = 0; j < 8; ++j) s[j] *= inv_n;
}
__device__ __forceinline__ unsigned slope_pk(float slope) {       // h(slope) in both halves of a register
    return (unsigned)__builtin_bit_cast(unsigned short, (_Float16)slope) * 0x10001u;
}

// ------------------------------------------------------------------------------------------------------------
// res_join<ST>: element-wise over NHWC; a lane owns 16 bytes of one pixel - 4 consecutive channels of fp32 storage (a block: 32 pixels x
// 32 channels; grid: pixel groups x C / 32), 8 of fp16 storage (a block: 256 / (C / 8) whole pixels; grid: pixel groups; C <= 2048).  No LDS,
// no atomics; three tensor passes (conv2, the residual, the output).  fp16 storage: both addends in fp32, ONE rounding of the sum, on the store.
// ------------------------------------------------------------------------------------------------------------
struct JoinArgs {
    const float* raw2; const float* sc2; const float* sh2;      // conv2: raw output [B][HW][C], scale / shift [B][C]
    const float* r; const float* scr; const float* shr;         // the residual's source and its scale / shift
    float* dst; float* dsc; float* dsh;                         // the block's pre-activation output; its scale (1) / shift (0) [B][C]
    int linear;            // 1: r is a projection (normalised, not activated, already at the output's extent); 0: the block's activated input,
    int sy, sx;            //    average-pooled over this window ((1, 1): the identity skip)
    int HW, Wt, Win;       // output pixels per image, output width, width of the residual's source
    int C, npix;           // channels (a multiple of 32), B * HW
    float slope, inv_n;    // inv_n = 1 / (sy * sx)
};

template <typename ST>
__global__ __launch_bounds__(256) void res_join(const JoinArgs a) {
  if constexpr (std::is_same<ST, float>::value) {
    const unsigned upix = blockIdx.x * 32u + (threadIdx.x >> 3);
    if (upix >= (unsigned)a.npix) return;
    const int pix = (int)upix, c = blockIdx.y * 32 + (threadIdx.x & 7) * 4;
    const int b = pix / a.HW, p = pix - b * a.HW;
    const size_t o = (size_t)pix * a.C + c, oc = (size_t)b * a.C + c;
    const f32x4 v2 = *reinterpret_cast<const f32x4*>(a.raw2 + o);
    const f32x4 s2 = *reinterpret_cast<const f32x4*>(a.sc2 + oc), h2 = *reinterpret_cast<const f32x4*>(a.sh2 + oc);
    const f32x4 sr = *reinterpret_cast<const f32x4*>(a.scr + oc), hr = *reinterpret_cast<const f32x4*>(a.shr + oc);
    f32x4 r;
    if (a.linear) {
        const f32x4 vp = *reinterpret_cast<const f32x4*>(a.r + o);
#pragma unroll
        for (int j = 0; j < 4; ++j) r[j] = fmaf(sr[j], vp[j], hr[j]);
    } else {
        const int y = p / a.Wt, x = p - y * a.Wt;
        const size_t row = (size_t)a.Win * a.C;
        const float* src = a.r + ((size_t)b * a.HW * (a.sy * a.sx) + (size_t)(y * a.sy) * a.Win + (size_t)x * a.sx) * a.C + c;
        r = pooled_act4(src, row, a.C, a.sy, a.sx, sr, hr, a.slope, a.inv_n);
    }
    f32x4 t;
#pragma unroll
    for (int j = 0; j < 4; ++j) t[j] = fmaf(s2[j], v2[j], h2[j]) + r[j];
    *reinterpret_cast<f32x4*>(a.dst + o) = t;
    if (p == 0) {
        *reinterpret_cast<f32x4*>(a.dsc + oc) = f32x4{1.f, 1.f, 1.f, 1.f};
        *reinterpret_cast<f32x4*>(a.dsh + oc) = f32x4{0.f, 0.f, 0.f, 0.f};
    }
  } else {
    // C / 8 lanes per pixel, 256 / (C / 8) whole pixels per block: a block's loads and stores are one contiguous run of whole pixels (a block of
    // 32 channels would touch half of every 128-byte line of a 64-channel tensor, the other half left to a block on another XCD)
    const unsigned lpp = (unsigned)a.C >> 3, ppb = 256u / lpp, pl = threadIdx.x / lpp;
    const unsigned upix = blockIdx.x * ppb + pl;
    if (pl >= ppb || upix >= (unsigned)a.npix) return;
    const int pix = (int)upix, c = (int)(threadIdx.x - pl * lpp) * 8;
    const int b = pix / a.HW, p = pix - b * a.HW;
    const size_t o = (size_t)pix * a.C + c, oc = (size_t)b * a.C + c;
    const half8 v2 = *reinterpret_cast<const half8*>(reinterpret_cast<const _Float16*>(a.raw2) + o);
    const f32x4 s2a = *reinterpret_cast<const f32x4*>(a.sc2 + oc), s2b = *reinterpret_cast<const f32x4*>(a.sc2 + oc + 4);
    const f32x4 h2a = *reinterpret_cast<const f32x4*>(a.sh2 + oc), h2b = *reinterpret_cast<const f32x4*>(a.sh2 + oc + 4);
    const f32x4 sra = *reinterpret_cast<const f32x4*>(a.scr + oc), srb = *reinterpret_cast<const f32x4*>(a.scr + oc + 4);
    const f32x4 hra = *reinterpret_cast<const f32x4*>(a.shr + oc), hrb = *reinterpret_cast<const f32x4*>(a.shr + oc + 4);
    const _Float16* rh = reinterpret_cast<const _Float16*>(a.r);
    float r[8];
    if (a.linear) {
        const half8 vp = *reinterpret_cast<const half8*>(rh + o);
#pragma unroll
        for (int j = 0; j < 4; ++j) { r[j] = fmaf(sra[j], (float)vp[j], hra[j]); r[4 + j] = fmaf(srb[j], (float)vp[4 + j], hrb[j]); }
    } else {
        const int y = p / a.Wt, x = p - y * a.Wt;
        const size_t row = (size_t)a.Win * a.C;
        const _Float16* src = rh + ((size_t)b * a.HW * (a.sy * a.sx) + (size_t)(y * a.sy) * a.Win + (size_t)x * a.sx) * a.C + c;
        pooled_act8_h(src, row, a.C, a.sy, a.sx, sra, srb, hra, hrb, slope_pk(a.slope), a.inv_n, r);
    }
    half8 t;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        t[j] = (_Float16)(fmaf(s2a[j], (float)v2[j], h2a[j]) + r[j]);
        t[4 + j] = (_Float16)(fmaf(s2b[j], (float)v2[4 + j], h2b[j]) + r[4 + j]);
    }
    *reinterpret_cast<half8*>(reinterpret_cast<_Float16*>(a.dst) + o) = t;
    if (p == 0) {
        *reinterpret_cast<f32x4*>(a.dsc + oc) = f32x4{1.f, 1.f, 1.f, 1.f}; *reinterpret_cast<f32x4*>(a.dsc + oc + 4) = f32x4{1.f, 1.f, 1.f, 1.f};
        *reinterpret_cast<f32x4*>(a.dsh + oc) = f32x4{0.f, 0.f, 0.f, 0.f}; *reinterpret_cast<f32x4*>(a.dsh + oc + 4) = f32x4{0.f, 0.f, 0.f, 0.f};
    }
  }
}

// ------------------------------------------------------------------------------------------------------------
// pool_proj1x1: GEMM with M = the batch's output pixels (numbered through the whole batch: a 1x1 conv knows no neighbours, so a tile of 128
// rows may span images of any extent - a 2 x 4 bottleneck fills it with 16 images), K = Cin, N = Cout, on v_mfma_f32_32x32x2_f32 (an exact
// fp32 FMA chain, as the K_EXACT kernels).  Workgroup: 128 rows x BN columns, wave w rows [32 w, 32 w + 32).  Per chunk of 32 input channels
// the A rows are normalised, activated and average-pooled on the way into LDS (row pitch 33 floats: the fragment reads of 32 rows hit 32
// banks) and the weight rows [32][BN] are staged beside them.  No bias.  Statistics: where an image is a whole number of tiles (HW % 128 == 0,
// `part` set) the epilogue leaves the shifted partial (S, Q, K, n) of every (tile, channel) for finalize_stats_t - the protocol of kernels.h,
// a tile's partials depend on its own image only; else stats_direct reads the output.
// LDS: 128 * 33 * 4 + 32 * BN * 4 = 25 088 bytes at BN = 64.
// ------------------------------------------------------------------------------------------------------------
struct ProjArgs {
    const float* src; const float* sc; const float* sh;      // the block's input [B][Hin][Win][Cin] and its scale / shift [B][Cin]
    const float* w;        // [Cin][Cout]
    const void* wh;        // (pool_proj1x1_h) the weights rounded to half, [Cin / 32][Cout][32 halves]
    float* dst;            // raw output [M][Cout]
    float* part;           // [M / 128][Cout][4] partial statistics, or nullptr (HW % 128 != 0: tiles span images)
    int Cin, Cout;         // multiples of 32
    int sy, sx;            // pooling window = the block's stride
    int HW, Wt, Win;       // output pixels per image, output width, source width
    int M;                 // B * HW
    float slope, inv_n;
};

constexpr int kProjBM = 128, kProjPitch = 33;

template <int BN>
__global__ __launch_bounds__(256) void pool_proj1x1(const ProjArgs a) {
    __shared__ __attribute__((aligned(16))) float As[kProjBM * kProjPitch];
    __shared__ __attribute__((aligned(16))) float Ws[32 * BN];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const unsigned m0 = blockIdx.x * (unsigned)kProjBM;
    const int n0 = blockIdx.y * BN;
    // the 4 rows this thread stages (row = tid / 8 + 32 i, channels 4 (tid % 8) ... + 3 of the chunk)
    const int c4 = (tid & 7) * 4;
    size_t base[4]; int boff[4]; bool valid[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const unsigned m = m0 + (tid >> 3) + 32 * i;
        valid[i] = m < (unsigned)a.M;
        const int mm = valid[i] ? (int)m : 0;
        const int b = mm / a.HW, p = mm - b * a.HW, y = p / a.Wt, x = p - y * a.Wt;
        base[i] = ((size_t)b * a.HW * (a.sy * a.sx) + (size_t)(y * a.sy) * a.Win + (size_t)x * a.sx) * a.Cin + c4;
        boff[i] = b * a.Cin + c4;
    }
    const size_t row = (size_t)a.Win * a.Cin;
    f32x16 acc[BN / 32];
#pragma unroll
    for (int nt = 0; nt < BN / 32; ++nt) acc[nt] = kZero16;
    for (int k0 = 0; k0 < a.Cin; k0 += 32) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (valid[i]) {
                const f32x4 sc = *reinterpret_cast<const f32x4*>(a.sc + boff[i] + k0), sh = *reinterpret_cast<const f32x4*>(a.sh + boff[i] + k0);
                v = pooled_act4(a.src + base[i] + k0, row, a.Cin, a.sy, a.sx, sc, sh, a.slope, a.inv_n);
            }
            float* d = As + ((tid >> 3) + 32 * i) * kProjPitch + c4;
            d[0] = v[0]; d[1] = v[1]; d[2] = v[2]; d[3] = v[3];
        }
#pragma unroll
        for (int i = 0; i < BN / 32; ++i) {          // 32 * BN / 4 units of 4 columns, 256 per pass
            const int u = tid + 256 * i, k = u / (BN / 4), n4 = (u - k * (BN / 4)) * 4;
            *reinterpret_cast<f32x4*>(Ws + k * BN + n4) = *reinterpret_cast<const f32x4*>(a.w + (size_t)(k0 + k) * a.Cout + n0 + n4);
        }
        __syncthreads();
        const float* ar = As + (32 * wave + (lane & 31)) * kProjPitch + (lane >> 5);
        const float* br = Ws + (lane >> 5) * BN + (lane & 31);
#pragma unroll
        for (int kk = 0; kk < 16; ++kk) {
            const float av = ar[2 * kk];
#pragma unroll
            for (int nt = 0; nt < BN / 32; ++nt) acc[nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, br[2 * kk * BN + nt * 32], acc[nt], 0, 0, 0);
        }
        __syncthreads();
    }
    // C / D layout of the 32x32 MFMA: column = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const unsigned m = m0 + 32 * wave + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        if (m >= (unsigned)a.M) continue;
#pragma unroll
        for (int nt = 0; nt < BN / 32; ++nt) a.dst[(size_t)m * a.Cout + n0 + nt * 32 + (lane & 31)] = acc[nt][r];
    }
    if (a.part != nullptr) {      // (every row of the tile is a pixel of ONE image; As is free: the chunk loop ended with a barrier)
        float* red = As;          // [4 waves][BN][4]
#pragma unroll
        for (int nt = 0; nt < BN / 32; ++nt) {
            const float kv = stat_pivot(acc[nt][0]);
            float s = 0.f, q = 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) { const float d = acc[nt][r] - kv; s += d; q = __builtin_fmaf(d, d, q); }
            s += __shfl_xor(s, 32); q += __shfl_xor(q, 32);
            if (lane < 32) stat_wave_put(red, wave * BN + nt * 32 + lane, s, q, kv, 32.f);
        }
        lds_barrier();
        if (tid < BN) stat_tile_store(red, 4, BN, tid, a.part + ((size_t)blockIdx.x * a.Cout + n0 + tid) * 4);
    }
}

// ------------------------------------------------------------------------------------------------------------
// pool_proj1x1_h: the same GEMM for fp16 storage (the 16-bit mode), on v_mfma_f32_32x32x16_f16 - one product per MAC, fp32 accumulation.
// Same workgroup tile (128 rows x BN columns, wave w rows [32 w, 32 w + 32)) and the same `part` protocol.  Per chunk of 32 input channels a
// thread stages two (row, channel octet) units: eight stored halves per window pixel -> operand values (norm_lrelu_8) -> fp32 window sum
// times 1 / n -> rounded to half, 16 bytes into the row's LDS record; the chunk's weights (rounded to half once, on the host: pack_weights)
// go beside them as one record per column.  Records are [ch 0..15 | ch 16..31 | pad] of 80 bytes (kRec), as in conv3x3_h32: lane (r, h)
// reads 16 bytes at record r + 16 h (k-step 0) and + 32 (k-step 1) - 20-dword pitch, conflict-free for ds_read_b128.  Output stored as half;
// the partial statistics are taken over the stored (rounded) values.
// LDS: 128 * 80 + BN * 80 = 15 360 bytes at BN = 64 (the statistics exchange, 4 * BN * 16 bytes, reuses the A records).
// ------------------------------------------------------------------------------------------------------------
template <int BN>
__global__ __launch_bounds__(256) void pool_proj1x1_h(const ProjArgs a) {
    constexpr int NT = BN / 32;
    __shared__ __attribute__((aligned(16))) unsigned char As[kProjBM * kRec];
    __shared__ __attribute__((aligned(16))) unsigned char Bs[BN * kRec];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
    const unsigned m0 = blockIdx.x * (unsigned)kProjBM;
    const int n0 = blockIdx.y * BN;
    // the 2 units this thread stages (row = tid / 4 + 64 i, channels 8 (tid % 4) ... + 7 of the chunk)
    const int oct = (tid & 3) * 8;
    size_t base[2]; int boff[2]; bool valid[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const unsigned m = m0 + (tid >> 2) + 64 * i;
        valid[i] = m < (unsigned)a.M;
        const int mm = valid[i] ? (int)m : 0;
        const int b = mm / a.HW, p = mm - b * a.HW, y = p / a.Wt, x = p - y * a.Wt;
        base[i] = ((size_t)b * a.HW * (a.sy * a.sx) + (size_t)(y * a.sy) * a.Win + (size_t)x * a.sx) * a.Cin + oct;
        boff[i] = b * a.Cin + oct;
    }
    const size_t row = (size_t)a.Win * a.Cin;
    const _Float16* src = reinterpret_cast<const _Float16*>(a.src);
    const unsigned slope2 = slope_pk(a.slope);
    f32x16 acc[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) acc[nt] = kZero16;
    for (int k0 = 0; k0 < a.Cin; k0 += 32) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            uint4 o = uint4{0u, 0u, 0u, 0u};
            if (valid[i]) {
                const float* ps = a.sc + boff[i] + k0; const float* pt = a.sh + boff[i] + k0;
                float s[8];
                pooled_act8_h(src + base[i] + k0, row, a.Cin, a.sy, a.sx, *reinterpret_cast<const f32x4*>(ps), *reinterpret_cast<const f32x4*>(ps + 4),
                              *reinterpret_cast<const f32x4*>(pt), *reinterpret_cast<const f32x4*>(pt + 4), slope2, a.inv_n, s);
                half8 ov;
#pragma unroll
                for (int j = 0; j < 8; ++j) ov[j] = (_Float16)s[j];
                o = __builtin_bit_cast(uint4, ov);
            }
            *reinterpret_cast<uint4*>(As + ((tid >> 2) + 64 * i) * kRec + (tid & 3) * 16) = o;
        }
        const uint4* wsrc = reinterpret_cast<const uint4*>(a.wh) + ((size_t)(k0 >> 5) * a.Cout + n0) * 4;      // [column][4 units of 8 halves]
        if (BN * 4 >= 256 || tid < BN * 4) *reinterpret_cast<uint4*>(Bs + (tid >> 2) * kRec + (tid & 3) * 16) = wsrc[tid];
        __syncthreads();
        const half8 fa0 = *reinterpret_cast<const half8*>(As + (32 * wave + r) * kRec + 16 * h);
        const half8 fa1 = *reinterpret_cast<const half8*>(As + (32 * wave + r) * kRec + 16 * h + 32);
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            const half8 fb0 = *reinterpret_cast<const half8*>(Bs + (nt * 32 + r) * kRec + 16 * h);
            const half8 fb1 = *reinterpret_cast<const half8*>(Bs + (nt * 32 + r) * kRec + 16 * h + 32);
            acc[nt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fa0, fb0, acc[nt], 0, 0, 0);
            acc[nt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fa1, fb1, acc[nt], 0, 0, 0);
        }
        __syncthreads();
    }
    // the values as stored; C / D layout of the 32x32 MFMA: column = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
    _Float16* dst = reinterpret_cast<_Float16*>(a.dst);
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int rg = 0; rg < 16; ++rg) acc[nt][rg] = round_act<_Float16>(acc[nt][rg]);
#pragma unroll
    for (int rg = 0; rg < 16; ++rg) {
        const unsigned m = m0 + 32 * wave + (rg & 3) + 8 * (rg >> 2) + 4 * h;
        if (m >= (unsigned)a.M) continue;
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) dst[(size_t)m * a.Cout + n0 + nt * 32 + r] = (_Float16)acc[nt][rg];
    }
    if (a.part != nullptr) {      // (every row of the tile is a pixel of ONE image; As is free: the chunk loop ended with a barrier)
        float* red = reinterpret_cast<float*>(As);          // [4 waves][BN][4]
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            const float kv = stat_pivot(acc[nt][0]);
            float s = 0.f, q = 0.f;
#pragma unroll
            for (int rg = 0; rg < 16; ++rg) { const float d = acc[nt][rg] - kv; s += d; q = __builtin_fmaf(d, d, q); }
            s += __shfl_xor(s, 32); q += __shfl_xor(q, 32);
            if (lane < 32) stat_wave_put(red, wave * BN + nt * 32 + lane, s, q, kv, 32.f);
        }
        lds_barrier();
        if (tid < BN) stat_tile_store(red, 4, BN, tid, a.part + ((size_t)blockIdx.x * a.Cout + n0 + tid) * 4);
    }
}

}  // namespace ts2d
