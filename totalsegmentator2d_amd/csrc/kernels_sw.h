// Device side of nnU-Net's sliding-window inference: tile gather with mirroring, and the
// Gaussian-weighted aggregation into upstream's float16 buffers (predicted_logits / n_predictions / gaussian are torch.half;
// a half operation = fp32 operation + round-to-nearest-even to half, which is what ATen's CPU half kernels and numpy do).
// Two orders (ts2d_engine_set_tile_dtype; pinned by plain-ATen statements in tests/test_oracle.py):
//   tile_half == 0 (default, the reference's CPU path): the mirror-averaged tile stays fp32, `p *= g` is fp32 x float(g) in
//     fp32, `logits[sl] += p` is a float add with ONE cast to half;
//   tile_half != 0 (the CUDA autocast path): the tile is cast to half first, the product and the sum each round to half.
// Tiles are accumulated in upstream order per output pixel, so the result is bit-identical to the host implementation in
// predictor.py (tests/test_gpu_predictor.py).
//
// One kernel pair serves ts2d_engine_predict_tiled (one image) and ts2d_engine_predict_tiled_batch: ONE gather and ONE aggregate launch
// per chunk of network rows, whatever the number of images in it.  A chunk is described by a device table of segments (one per image
// that has rows in the chunk); a block belongs to exactly one segment, found by a search over the `first block` prefix with the block
// index - wave-uniform, so no lane diverges on it.  Both kernels are pure HBM traffic: each lane owns 4 consecutive X, reads 16 bytes
// where the tile origin and the row pitch allow (a W-mirrored variant reads the 16 bytes at the mirrored position and reverses them)
// and stores 16 / 8 / 4 bytes.
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <stdint.h>
#include "device_tables.h"      // SwSeg

namespace ts2d {

// the segment that owns block `blk`: the last one whose first block is <= blk (n <= 64: at most 6 steps, all in scalar registers)
template <bool AGG>
__device__ __forceinline__ int sw_find_seg(const SwSeg* __restrict__ segs, int n, unsigned blk) {
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        const unsigned first = AGG ? segs[mid].ablock0 : segs[mid].gblock0;
        if (first <= blk) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// batch row (t * V + v) = tile t, mirror variant v; variant flips: bit0 = flip H (tensor dim 2), bit1 = flip W (dim 3), packed 8 bits per variant
__device__ __forceinline__ int sw_vflip(int packed, int v) { return (packed >> (8 * v)) & 3; }

__global__ __launch_bounds__(256) void sw_gather(const float* __restrict__ images, const SwSeg* __restrict__ segs, int n_segs,
                                                 int C, int ph, int pw, int V, int vflips, const int* __restrict__ tile_y,
                                                 const int* __restrict__ tile_x, float* __restrict__ batch) {
    const SwSeg sg = segs[sw_find_seg<false>(segs, n_segs, blockIdx.x)];
    const int pwq = (pw + 3) >> 2;
    const long long q = (long long)(blockIdx.x - sg.gblock0) * 256 + threadIdx.x;
    if (q >= (long long)sg.n_rows * C * ph * pwq) return;
    const int x0 = (int)(q % pwq) * 4; long long r = q / pwq;
    const int y = (int)(r % ph); r /= ph;
    const int c = (int)(r % C); const int lrow = (int)(r / C);
    const int row = sg.row0 + lrow, t = row / V, f = sw_vflip(vflips, row % V);
    const int ty = tile_y[sg.tile0 + t], tx = tile_x[sg.tile0 + t];
    const int sy = (f & 1) ? ph - 1 - y : y;
    const float* src = images + sg.img_off + ((size_t)c * sg.Hp + ty + sy) * sg.Wp + tx;
    float* dst = batch + (((size_t)(sg.batch_row + lrow) * C + c) * ph + y) * pw + x0;
    if (((pw | sg.Wp | tx) & 3) == 0) {
        float4 v;
        if (f & 2) { const float4 m = *reinterpret_cast<const float4*>(src + pw - 4 - x0); v = make_float4(m.w, m.z, m.y, m.x); }
        else v = *reinterpret_cast<const float4*>(src + x0);
        *reinterpret_cast<float4*>(dst) = v;
    } else {
        for (int j = 0; j < 4; ++j) {
            const int x = x0 + j;
            if (x < pw) dst[j] = src[(f & 2) ? pw - 1 - x : x];
        }
    }
}

__device__ __forceinline__ __half h_mul(__half a, __half b) { return __float2half_rn(__half2float(a) * __half2float(b)); }
__device__ __forceinline__ __half h_add(__half a, __half b) { return __float2half_rn(__half2float(a) + __half2float(b)); }
__device__ __forceinline__ __half h_div(__half a, __half b) { return __float2half_rn(__half2float(a) / __half2float(b)); }

// one tile's contribution to one pixel (y: the sum over the mirror variants), shared by the 16-byte and the per-pixel path of sw_aggregate
__device__ __forceinline__ void sw_blend(__half& acc, __half& n, float y, int V, bool has_gauss, __half g, int tile_half) {
    if (V > 1) y /= (float)V;
    if (tile_half) {
        __half p = __float2half_rn(y);
        if (has_gauss) p = h_mul(p, g);
        acc = h_add(acc, p);
    } else {      // (explicit _rn intrinsics: the product must round to fp32 before the add - no FMA contraction)
        const float pf = has_gauss ? __fmul_rn(y, __half2float(g)) : y;
        acc = __float2half_rn(__fadd_rn(__half2float(acc), pf));
    }
    n = h_add(n, g);
}

// one lane per 4 consecutive X of one (k, Y) row of one image's padded extent
__global__ __launch_bounds__(256) void sw_aggregate(const float* __restrict__ logits, const SwSeg* __restrict__ segs, int n_segs,
                                                    int K, int ph, int pw, int V, int vflips, const int* __restrict__ tile_y,
                                                    const int* __restrict__ tile_x, const __half* __restrict__ gauss,
                                                    __half* __restrict__ out16, uint8_t* __restrict__ seg, float thr,
                                                    int* __restrict__ inf_flags, int tile_half) {
    const SwSeg sg = segs[sw_find_seg<true>(segs, n_segs, blockIdx.x)];
    const int Hp = sg.Hp, Wp = sg.Wp, Wq = (Wp + 3) >> 2;
    const long long total = (long long)K * Hp * Wq;
    // the rows of the image this WAVE covers (one k only, else every row): a tile outside them is skipped with one scalar test
    const long long qw = (long long)(blockIdx.x - sg.ablock0) * 256 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x & ~63u));
    if (qw >= total) return;
    const long long rw0 = qw / Wq, rw1 = (qw + 63 < total ? qw + 63 : total - 1) / Wq;
    const bool one_k = rw0 / Hp == rw1 / Hp;
    const int Ylo = one_k ? (int)(rw0 % Hp) : 0, Yhi = one_k ? (int)(rw1 % Hp) : Hp - 1;
    const long long q = qw + (threadIdx.x & 63);
    if (q >= total) return;
    const int X0 = (int)(q % Wq) * 4; const long long r = q / Wq;
    const int Y = (int)(r % Hp), k = (int)(r / Hp);
    const size_t plane = (size_t)ph * pw;
    const __half one = __float2half_rn(1.f);
    __half acc[4], n[4];
    for (int j = 0; j < 4; ++j) { acc[j] = __float2half_rn(0.f); n[j] = __float2half_rn(0.f); }
    for (int t = 0; t < sg.n_tiles; ++t) {                // tiles in ascending (upstream) order
        const int ty = tile_y[sg.tile0 + t], tx = tile_x[sg.tile0 + t];
        if (Yhi < ty || Ylo >= ty + ph) continue;         // (wave-uniform)
        const int yy = Y - ty, xx0 = X0 - tx;
        if (yy < 0 || yy >= ph || xx0 + 3 < 0 || xx0 >= pw) continue;
        const float* base = logits + ((size_t)(sg.log_row + t * V) * K + k) * plane;
        if (((tx | pw) & 3) == 0) {                       // (wave-uniform) xx0 is a multiple of 4: the four pixels are inside the tile
            const float4 a = *reinterpret_cast<const float4*>(base + (size_t)yy * pw + xx0);
            float y[4] = {a.x, a.y, a.z, a.w};
            for (int v = 1; v < V; ++v) {                 // variants in upstream order; each read at the un-flipped position
                const int f = sw_vflip(vflips, v);
                const float* p = base + (size_t)v * K * plane + (size_t)((f & 1) ? ph - 1 - yy : yy) * pw;
                if (f & 2) { const float4 m = *reinterpret_cast<const float4*>(p + pw - 4 - xx0); y[0] += m.w; y[1] += m.z; y[2] += m.y; y[3] += m.x; }
                else { const float4 m = *reinterpret_cast<const float4*>(p + xx0); y[0] += m.x; y[1] += m.y; y[2] += m.z; y[3] += m.w; }
            }
            __half g[4] = {one, one, one, one};
            if (gauss) {
                const uint2 gb = *reinterpret_cast<const uint2*>(gauss + (size_t)yy * pw + xx0);
                g[0] = __ushort_as_half((unsigned short)(gb.x & 0xFFFFu)); g[1] = __ushort_as_half((unsigned short)(gb.x >> 16));
                g[2] = __ushort_as_half((unsigned short)(gb.y & 0xFFFFu)); g[3] = __ushort_as_half((unsigned short)(gb.y >> 16));
            }
            for (int j = 0; j < 4; ++j) sw_blend(acc[j], n[j], y[j], V, gauss != nullptr, g[j], tile_half);
        } else {
            for (int j = 0; j < 4; ++j) {
                const int xx = xx0 + j;
                if (xx < 0 || xx >= pw) continue;
                float y = base[(size_t)yy * pw + xx];
                for (int v = 1; v < V; ++v) {
                    const int f = sw_vflip(vflips, v);
                    const int sy = (f & 1) ? ph - 1 - yy : yy, sx = (f & 2) ? pw - 1 - xx : xx;
                    y += base[(size_t)v * K * plane + (size_t)sy * pw + sx];
                }
                const __half g = gauss ? gauss[(size_t)yy * pw + xx] : one;
                sw_blend(acc[j], n[j], y, V, gauss != nullptr, g, tile_half);
            }
        }
    }
    __half res[4];
    bool inf = false;
    const int nx = Wp - X0 < 4 ? Wp - X0 : 4;             // (the last quad of a row whose pitch is no multiple of 4)
    for (int j = 0; j < 4; ++j) {
        res[j] = h_div(acc[j], n[j]);
        inf |= j < nx && (__half_as_ushort(res[j]) & 0x7FFFu) == 0x7C00u;
    }
    if (inf) inf_flags[sg.image] = 1;                     // upstream's "Encountered inf in predicted array" check, per image
    const size_t o = (size_t)sg.out_off + ((size_t)k * Hp + Y) * Wp + X0;
    if ((Wp & 3) == 0) {
        if (out16) {
            uint2 w;
            w.x = (unsigned)__half_as_ushort(res[0]) | ((unsigned)__half_as_ushort(res[1]) << 16);
            w.y = (unsigned)__half_as_ushort(res[2]) | ((unsigned)__half_as_ushort(res[3]) << 16);
            *reinterpret_cast<uint2*>(out16 + o) = w;
        }
        if (seg) {
            unsigned w = 0;
            for (int j = 0; j < 4; ++j) w |= (__half2float(res[j]) > thr ? 1u : 0u) << (8 * j);
            *reinterpret_cast<unsigned*>(seg + o) = w;
        }
    } else {
        for (int j = 0; j < 4; ++j) {                     // (constant trip count: res[] stays in registers)
            if (j >= nx) continue;
            if (out16) out16[o + j] = res[j];
            if (seg) seg[o + j] = __half2float(res[j]) > thr ? 1 : 0;
        }
    }
}

}  // namespace ts2d
