// PyTorch-layout weight blob -> the packed device layouts of every kernel family (fp16 hi / lo split images, the fp64 composition of a
// transposed conv with the following 3x3 conv), on host threads.
#include "engine_internal.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <thread>

namespace ts2d {

float f16_to_f32(uint16_t hb) {
    const uint32_t sign = (uint32_t)(hb & 0x8000u) << 16, ex = (hb >> 10) & 0x1F, m = hb & 0x3FFu;
    uint32_t x;
    if (ex == 0) {
        if (m == 0) x = sign;
        else { float v = (float)m * 5.9604644775390625e-08f; memcpy(&x, &v, 4); x |= sign; }
    } else if (ex == 31) x = sign | 0x7F800000u | (m << 13);
    else x = sign | ((ex + 112) << 23) | (m << 13);
    float f; memcpy(&f, &x, 4); return f;
}

namespace {

// fp32 -> fp16 bits, round to nearest even (host side of the weight split; the device uses v_cvt_f16_f32, also RNE)
uint16_t f32_to_f16(float f) {
    uint32_t x; memcpy(&x, &f, 4);
    const uint32_t sign = (x >> 16) & 0x8000u;
    x &= 0x7FFFFFFFu;
    if (x >= 0x7F800000u) return (uint16_t)(sign | (x > 0x7F800000u ? 0x7E00u : 0x7C00u));
    if (x >= 0x477FF000u) return (uint16_t)(sign | 0x7C00u);                       // rounds to >= 65520 -> inf
    if (x < 0x38800000u) {                                                          // subnormal half (or zero)
        if (x < 0x33000000u) return (uint16_t)sign;
        const int shift = 126 - (int)(x >> 23);                                     // 14..24
        uint32_t m = (x & 0x7FFFFFu) | 0x800000u;
        const uint32_t half = m >> shift, rem = m & ((1u << shift) - 1), mid = 1u << (shift - 1);
        return (uint16_t)(sign | (half + ((rem > mid || (rem == mid && (half & 1))) ? 1 : 0)));
    }
    const uint32_t rem = x & 0x1FFFu;
    uint32_t hbits = (x - 0x38000000u) >> 13;
    if (rem > 0x1000u || (rem == 0x1000u && (hbits & 1))) ++hbits;
    return (uint16_t)(sign | hbits);
}
// Host threads for the weight packing (the fp64 composition of the transposed convs is 4.8 GFLOP per 512-channel level: 3.5 s
// single-threaded for the canonical net - VERDICT r2 item 14).  Static partition of [0, n): every index is written by one thread.
template <typename F>
void parallel_for(int n, F&& f) {
    int nt = (int)std::thread::hardware_concurrency();
    nt = std::max(1, std::min(std::min(nt, 16), n));
    if (nt == 1) { for (int i = 0; i < n; ++i) f(i); return; }
    // Thread creation can fail (process / thread limits of a pool box): nothing may escape through the C-ABI, and a started thread
    // must be joined.  Thread t takes the indices t, t + nt, ...; the lanes whose thread could not start run here, serially.
    std::vector<std::thread> th;
    int started = 0;
    try {
        th.reserve(nt);
        for (int t = 0; t < nt; ++t) { th.emplace_back([&f, t, nt, n]() { for (int i = t; i < n; i += nt) f(i); }); ++started; }
    } catch (...) { /* fall through with `started` threads */ }
    for (int t = started; t < nt; ++t) for (int i = t; i < n; i += nt) f(i);
    for (auto& x : th) if (x.joinable()) x.join();
}

}  // namespace

// PyTorch-layout blob -> packed device layouts (host staging buffer `out`, weight_floats long).
void pack_weights(const ts2d_engine* e, const float* blob, float* out) {
    memset(out, 0, e->weight_floats * sizeof(float));
    for (const Op& op : e->ops) {
        if (op.first_direct) memcpy(out + op.dev_wraw, blob + op.blob_w, (size_t)op.cout * op.cin * 9 * sizeof(float));
        if (op.type == OP_HEAD && op.split_ok) {
            const int ct = op.cin, co_n = op.cout;          // W[k][c]
            const float* w = blob + op.blob_w;
            float mx = 0.f;
            for (size_t i = 0; i < (size_t)ct * co_n; ++i) mx = std::max(mx, std::fabs(w[i]));
            const float wscale = (mx > 0.f && std::isfinite(mx)) ? std::exp2(std::floor(std::log2(16383.0f / mx))) : 1.f;
            out[op.dev_ws] = 1.0f / wscale;
            uint16_t* d = reinterpret_cast<uint16_t*>(out + op.dev_wh);         // zero-initialised: columns >= K stay 0
            for (int k = 0; k < co_n; ++k)
                for (int c = 0; c < ct; ++c) {
                    const float v = w[(size_t)k * ct + c] * wscale;
                    const uint16_t hi = f32_to_f16(v), lo = f32_to_f16(v - f16_to_f32(hi));
                    uint16_t* rec = d + ((size_t)(c / 16) * 32 + k) * 32;
                    rec[c % 16] = hi; rec[16 + c % 16] = lo;
                }
        }
        if (op.type == OP_CONVT && op.split_ok) {
            const int ct = op.cin, co_n = op.cout, N = 4 * co_n;
            const float* w = blob + op.blob_w;
            float mx = 0.f;
            for (size_t i = 0; i < (size_t)ct * co_n * 4; ++i) mx = std::max(mx, std::fabs(w[i]));
            const float wscale = (mx > 0.f && std::isfinite(mx)) ? std::exp2(std::floor(std::log2(16383.0f / mx))) : 1.f;
            out[op.dev_ws] = 1.0f / wscale;
            uint16_t* d = reinterpret_cast<uint16_t*>(out + op.dev_wh);
            for (int ci = 0; ci < ct; ++ci) {
                const int chunk = ci / 32, kk = (ci % 32) / 16, cc = ci % 16;
                for (int co = 0; co < co_n; ++co)
                    for (int ab = 0; ab < 4; ++ab) {
                        const float v = w[((size_t)ci * co_n + co) * 4 + ab] * wscale;
                        const uint16_t hi = f32_to_f16(v);
                        const uint16_t lo = f32_to_f16(v - f16_to_f32(hi));
                        const int n = ab * co_n + co;          // [chunk32][column tile of 64][k-step][column][32 halves]
                        uint16_t* rec = d + ((((size_t)chunk * (N / 64) + n / 64) * 2 + kk) * 64 + n % 64) * 32;
                        rec[cc] = hi; rec[16 + cc] = lo;
                    }
            }
        }
        if (op.type == OP_CONV && op.split_ok) {
            // split-fp16 image: w * S = hi + lo with S = 2^k chosen so that max|w| * S is in [8192, 16384): hi and lo of
            // typical weights stay in fp16's normal range, products stay far from fp32 overflow.
            const int ct = op.cin + op.cin_skip, co_n = op.cout;
            const float* w = blob + op.blob_w;
            float mx = 0.f;
            for (size_t i = 0; i < (size_t)co_n * ct * 9; ++i) mx = std::max(mx, std::fabs(w[i]));
            const float wscale = (mx > 0.f && std::isfinite(mx)) ? std::exp2(std::floor(std::log2(16383.0f / mx))) : 1.f;
            out[op.dev_ws] = 1.0f / wscale;
            uint16_t* d = reinterpret_cast<uint16_t*>(out + op.dev_wh);
            parallel_for(co_n, [&](int co) {                         // (every packed element belongs to one output channel)
                for (int ci = 0; ci < ct; ++ci) {
                    for (int tap = 0; tap < 9; ++tap) {
                        const float v = w[((size_t)co * ct + ci) * 9 + tap] * wscale;
                        const uint16_t hi = f32_to_f16(v);
                        const uint16_t lo = f32_to_f16(v - f16_to_f32(hi));
                        if (op.stride == 1) {   // [chunk16][column tile][tap][column in tile][16 hi | 16 lo]: one contiguous block per (chunk, tile)
                            const int chunk = ci / 16, cc = ci % 16, bn = co_n % 64 == 0 ? 64 : 32;
                            uint16_t* rec = d + ((((size_t)chunk * (co_n / bn) + co / bn) * 9 + tap) * bn + co % bn) * 32;
                            rec[cc] = hi; rec[16 + cc] = lo;
                            if (bn == 64) {   // plane order of conv3x3_f16x3_qp: [chunk][column tile][tap][hi,lo][h][column][8 halves]
                                uint16_t* wp = reinterpret_cast<uint16_t*>(out + op.dev_wp);
                                const size_t base = (((size_t)chunk * (co_n / bn) + co / bn) * 9 + tap) * 4;
                                wp[((base + 0 + cc / 8) * bn + co % bn) * 8 + cc % 8] = hi;
                                wp[((base + 2 + cc / 8) * bn + co % bn) * 8 + cc % 8] = lo;
                            }
                            if (op.res_ok) {
                                uint16_t* rw = reinterpret_cast<uint16_t*>(out + op.dev_wres);
                                rw[((((size_t)tap * 2 + 0) * 4 + ci / 8) * 32 + co) * 8 + ci % 8] = hi;
                                rw[((((size_t)tap * 2 + 1) * 4 + ci / 8) * 32 + co) * 8 + ci % 8] = lo;
                            }
                            if (op.h32_ok)          // same blocks with 32 real channels per record (the hi parts only)
                                reinterpret_cast<uint16_t*>(out + op.dev_wh32)[((((size_t)(ci / 32) * (co_n / bn) + co / bn) * 9 + tap) * bn + co % bn) * 32 + ci % 32] = hi;
                        } else {       // K packed as 8 channels x 2 taps: k = 8 * (tap & 1) + (ci % 8) of k-step tap / 2
                            if (op.s2v2_ok) {      // [chunk16][column tile][tap][hi,lo][h = (ci % 16) / 8][column][ci % 8]
                                const int bn2 = op.bn2;
                                uint16_t* w2 = reinterpret_cast<uint16_t*>(out + op.dev_w2);
                                const size_t blk = ((size_t)(ci / 16) * (co_n / bn2) + co / bn2) * (9 * 2 * 2 * bn2 * 8);
                                w2[blk + ((((size_t)tap * 2 + 0) * 2 + (ci % 16) / 8) * bn2 + co % bn2) * 8 + ci % 8] = hi;
                                w2[blk + ((((size_t)tap * 2 + 1) * 2 + (ci % 16) / 8) * bn2 + co % bn2) * 8 + ci % 8] = lo;
                            }
                            const int chunk = ci / 8, cc = (tap & 1) * 8 + ci % 8, bn = co_n % 64 == 0 ? 64 : 32;
                            uint16_t* rec = d + ((((size_t)chunk * (co_n / bn) + co / bn) * 5 + tap / 2) * bn + co % bn) * 32;
                            rec[cc] = hi; rec[16 + cc] = lo;
                        }
                    }
                }
            });
        }
    }
    for (const Op& op : e->ops) {
        if (!op.upc_ok) continue;
        // ConvTranspose2d (2x2, stride 2) composed with the "up" half of the following 3x3 conv (kernels_upc.h), in fp64:
        //   Weff[A][B][dI][dJ][co][cb] = sum_{(ky,kx) -> (dI,dJ)} sum_cu W3[co][cu][ky][kx] WT[cb][cu][a][b]
        // with, for output parity A and tap ky: up row 2I + A + ky - 1 = 2 (I + A - 1 + dI) + a.
        const Op& up = e->ops[op.up_idx];
        const int cb_n = up.cin, cu_n = op.cin, cs_n = op.cin_skip, ct = cu_n + cs_n, co_n = op.cout;
        const float* w3 = blob + op.blob_w;          // [co][ct][3][3], channels 0 .. cu_n-1 = the upsampled half (torch.cat((up, skip), 1))
        const float* wt = blob + up.blob_w;          // [cb][cu][2][2]
        const float* bt = blob + up.blob_b;
        std::vector<double> R((size_t)4 * cu_n * cb_n);              // R[ab][cu][cb]
        for (int cb = 0; cb < cb_n; ++cb)
            for (int cu = 0; cu < cu_n; ++cu)
                for (int ab = 0; ab < 4; ++ab) R[((size_t)ab * cu_n + cu) * cb_n + cb] = wt[((size_t)cb * cu_n + cu) * 4 + ab];
        std::vector<double> Weff((size_t)16 * co_n * cb_n, 0.0);     // [tapidx = (A*2+B)*4 + dI*2+dJ][co][cb]
        parallel_for(co_n, [&](int co) {                             // (rows of Weff are disjoint per output channel; same summation order as serial)
            for (int A = 0; A < 2; ++A)
                for (int Bp = 0; Bp < 2; ++Bp)
                    for (int ky = 0; ky < 3; ++ky)
                        for (int kx = 0; kx < 3; ++kx) {
                            const int fy = (A + ky + 1) / 2 - 1, fx = (Bp + kx + 1) / 2 - 1;          // floor((A + ky - 1) / 2)
                            const int dI = fy - A + 1, dJ = fx - Bp + 1, ta = (A + ky + 1) & 1, tb = (Bp + kx + 1) & 1;
                            double* arow = Weff.data() + ((size_t)((A * 2 + Bp) * 4 + dI * 2 + dJ) * co_n + co) * cb_n;
                            const double* Rm = R.data() + (size_t)(ta * 2 + tb) * cu_n * cb_n;
                            for (int cu = 0; cu < cu_n; ++cu) {
                                const double l = w3[((size_t)co * ct + cu) * 9 + ky * 3 + kx];
                                const double* rrow = Rm + (size_t)cu * cb_n;
                                for (int cb = 0; cb < cb_n; ++cb) arow[cb] += l * rrow[cb];
                            }
                        }
        });
        double mx = 0.0;
        for (double v : Weff) mx = std::max(mx, std::fabs(v));
        for (int co = 0; co < co_n; ++co)
            for (int cs = 0; cs < cs_n; ++cs)
                for (int tap = 0; tap < 9; ++tap) mx = std::max(mx, (double)std::fabs(w3[((size_t)co * ct + cu_n + cs) * 9 + tap]));
        const float wscale = (mx > 0.0 && std::isfinite(mx)) ? std::exp2(std::floor(std::log2(16383.0 / mx))) : 1.f;
        out[op.dev_wcs] = 1.0f / wscale;
        const int bn = co_n % 64 == 0 ? 64 : 32, nct = co_n / bn;
        uint16_t* dc = reinterpret_cast<uint16_t*>(out + op.dev_wc);
        uint16_t* dk = reinterpret_cast<uint16_t*>(out + op.dev_wk);
        parallel_for(co_n, [&](int co) {
            for (int t = 0; t < 16; ++t)
                for (int cb = 0; cb < cb_n; ++cb) {
                    const float v = (float)(Weff[((size_t)t * co_n + co) * cb_n + cb] * (double)wscale);
                    const uint16_t hi = f32_to_f16(v), lo = f32_to_f16(v - f16_to_f32(hi));
                    const size_t base = (((size_t)(cb / 16) * nct + co / bn) * 16 + t) * 4;
                    const int hh = (cb % 16) / 8;
                    dc[((base + 0 + hh) * bn + co % bn) * 8 + cb % 8] = hi;
                    dc[((base + 2 + hh) * bn + co % bn) * 8 + cb % 8] = lo;
                    if (op.up0_ok) {       // fragment order of conv3x3_up0: lane = k-group (cb % 32) / 8, row co % 16
                        uint16_t* d0 = reinterpret_cast<uint16_t*>(out + op.dev_w0c);
                        const size_t f = ((size_t)(t >> 2) * 8 + (cb / 32) * 4 + (t & 3)) * 4;      // (parity, k-step) x [hi,lo][cb 2]
                        // MFMA block (co % 8) / 4, row 4 (co / 8) + co % 4: the lane that holds rows 4 g .. 4 g + 3 of both blocks owns channels 8 g .. 8 g + 7
                        const int blk = (co % 8) / 4, row = 4 * (co / 8) + co % 4;
                        const int ln = ((cb % 32) / 8) * 16 + row;
                        d0[((f + 0 + blk) * 64 + ln) * 8 + cb % 8] = hi;
                        d0[((f + 2 + blk) * 64 + ln) * 8 + cb % 8] = lo;
                    }
                }
            for (int cs = 0; cs < cs_n; ++cs)
                for (int tap = 0; tap < 9; ++tap) {
                    const float v = w3[((size_t)co * ct + cu_n + cs) * 9 + tap] * wscale;
                    const uint16_t hi = f32_to_f16(v), lo = f32_to_f16(v - f16_to_f32(hi));
                    const size_t base = (((size_t)(cs / 16) * nct + co / bn) * 9 + tap) * 4;
                    const int hh = (cs % 16) / 8;
                    dk[((base + 0 + hh) * bn + co % bn) * 8 + cs % 8] = hi;
                    dk[((base + 2 + hh) * bn + co % bn) * 8 + cs % 8] = lo;
                    if (op.up0_ok) {
                        uint16_t* k0 = reinterpret_cast<uint16_t*>(out + op.dev_w0k);
                        const int prow = ((co % 8) / 4) * 16 + 4 * (co / 8) + co % 4;      // (the same row permutation)
                        k0[((((size_t)tap * 2 + 0) * 4 + cs / 8) * 32 + prow) * 8 + cs % 8] = hi;
                        k0[((((size_t)tap * 2 + 1) * 4 + cs / 8) * 32 + prow) * 8 + cs % 8] = lo;
                    }
                }
        });
        // bias variants: the transposed conv's bias reaches an output pixel through the taps that lie inside the image
        float* bv = out + op.dev_bvar;
        for (int co = 0; co < co_n; ++co) {
            double bc[3][3];
            for (int ky = 0; ky < 3; ++ky)
                for (int kx = 0; kx < 3; ++kx) {
                    double acc = 0.0;
                    for (int cu = 0; cu < cu_n; ++cu) acc += (double)w3[((size_t)co * ct + cu) * 9 + ky * 3 + kx] * (double)bt[cu];
                    bc[ky][kx] = acc;
                }
            for (int ry = 0; ry < 3; ++ry)
                for (int rx = 0; rx < 3; ++rx) {
                    double acc = (double)blob[op.blob_b + co];
                    for (int ky = (ry == 0 ? 1 : 0); ky < (ry == 2 ? 2 : 3); ++ky)
                        for (int kx = (rx == 0 ? 1 : 0); kx < (rx == 2 ? 2 : 3); ++kx) acc += bc[ky][kx];
                    bv[(size_t)(ry * 3 + rx) * co_n + co] = (float)acc;
                }
        }
    }
    for (const Op& op : e->ops) {
        const int ct = op.cin + op.cin_skip, co_n = op.cout;
        if (op.type == OP_JOIN) continue;
        if (op.type == OP_PROJ) {           // W[co][ci] -> [ci][co]; no bias
            const float* w = blob + op.blob_w;
            float* d = out + op.dev_w;
            for (int co = 0; co < co_n; ++co)
                for (int ci = 0; ci < ct; ++ci) d[(size_t)ci * co_n + co] = w[(size_t)co * ct + ci];
            if (ct % 32 == 0) {             // the 16-bit mode's copy: h(w), [chunk32][co][32 halves]
                uint16_t* dh = reinterpret_cast<uint16_t*>(out + op.dev_wh);
                for (int co = 0; co < co_n; ++co)
                    for (int ci = 0; ci < ct; ++ci) dh[((size_t)(ci / 32) * co_n + co) * 32 + ci % 32] = f32_to_f16(w[(size_t)co * ct + ci]);
            }
            memcpy(out + op.dev_g, blob + op.blob_g, co_n * sizeof(float));
            memcpy(out + op.dev_be, blob + op.blob_be, co_n * sizeof(float));
            continue;
        }
        if (op.type == OP_CONV) {           // W[co][ci][ky][kx] -> [chunk][tap][kk][co][8]
            const int ck = op.ck, kkn = ck / 8;
            const float* w = blob + op.blob_w;
            float* d = out + op.dev_w;
            parallel_for(co_n, [&](int co) {
                for (int ci = 0; ci < ct; ++ci) {
                    const int chunk = ci / ck, cc = ci % ck, kk = cc / 8, el = cc % 8;
                    for (int tap = 0; tap < 9; ++tap)
                        d[((((size_t)chunk * 9 + tap) * kkn + kk) * co_n + co) * 8 + el] = w[((size_t)co * ct + ci) * 9 + tap];
                }
            });
            memcpy(out + op.dev_g, blob + op.blob_g, co_n * sizeof(float));
            memcpy(out + op.dev_be, blob + op.blob_be, co_n * sizeof(float));
        } else if (op.type == OP_CONVT) {   // W[ci][co][a][b] -> [chunk][kk][(a*KB+b)*Cout + co][8]   (kernel = stride = (KA, KB))
            const int ck = op.ck, kkn = ck / 8, nab = op.sy * op.sx, N = nab * co_n;
            const float* w = blob + op.blob_w;
            float* d = out + op.dev_w;
            for (int ci = 0; ci < ct; ++ci) {
                const int chunk = ci / ck, cc = ci % ck, kk = cc / 8, el = cc % 8;
                for (int co = 0; co < co_n; ++co)
                    for (int ab = 0; ab < nab; ++ab)
                        d[(((size_t)chunk * kkn + kk) * N + ab * co_n + co) * 8 + el] = w[((size_t)ci * co_n + co) * nab + ab];
            }
        } else {                            // head W[k][c] as is
            memcpy(out + op.dev_w, blob + op.blob_w, (size_t)ct * co_n * sizeof(float));
        }
        memcpy(out + op.dev_b, blob + op.blob_b, co_n * sizeof(float));
    }
}

}  // namespace ts2d
