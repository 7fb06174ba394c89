// Residual blocks of nnU-Net's ResidualEncoderUNet (BasicBlockD): out = lrelu(norm2(conv2(lrelu(norm1(conv1(x))))) + skip(x)).
// conv1 and conv2 are the engine's ordinary 3x3 blocks (raw output + per-(image, channel) scale / shift); this header holds what is new:
//   pool_proj1x1  the skip path where the widths differ: AvgPool2d(kernel = stride) -> Conv2d 1x1 without bias (-> norm: launch_stats)
//   res_join      t = norm2(conv2) + residual, stored BEFORE the block's LeakyReLU with scale 1 / shift 0, so that every consumer's
//                 load-time lrelu(scale * t + shift) is the block's output, exactly
// Both are per-pixel: a pixel's result depends on its own image only, whatever else is in the batch.  fp32 storage only (the 16-bit
// mode refuses a residual engine).
#pragma once
#include "kernels.h"

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

// ------------------------------------------------------------------------------------------------------------
// res_join: element-wise over NHWC fp32; a lane owns 4 consecutive channels of one pixel (16-byte loads and stores), a block 32 pixels x
// 32 channels (grid: pixel groups x C / 32).  No LDS, no atomics; three tensor passes (conv2, the residual, the output).
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

__global__ __launch_bounds__(256) void res_join(const JoinArgs a) {
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

}  // namespace ts2d
