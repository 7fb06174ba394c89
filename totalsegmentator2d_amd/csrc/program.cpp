// The network descriptor as a program: tensors, ops in PlainConvUNet (or ResidualEncoderUNet) forward order, offsets into the caller's blob and into the device
// weight arena (which packed weight images an op gets is decided here, by its channel counts).  Also the library's last-error slot.
#include "engine_internal.h"

#include <cstdarg>
#include <cstdio>
#include <cstring>

namespace ts2d {

namespace { thread_local std::string g_err; }

int fail(int code, const char* fmt, ...) {
    char buf[1024];
    va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof(buf), fmt, ap); va_end(ap);
    g_err = buf;
    return code;
}
const char* last_error() { return g_err.c_str(); }

int tensor_index(ts2d_engine* e, const std::string& name) {
    for (size_t i = 0; i < e->tensors.size(); ++i) if (e->tensors[i].name == name) return (int)i;
    return -1;
}

namespace {

int add_tensor(ts2d_engine* e, const std::string& name, int C, int level, bool normed) {
    Tensor t; t.name = name; t.C = C; t.level = level; t.normed = normed; t.ly = e->lvl_y[level]; t.lx = e->lvl_x[level];
    t.Cu = (name == "input") ? C : e->user_arch.features[level];
    e->tensors.push_back(t);
    return (int)e->tensors.size() - 1;
}

// The parameter tensors of a descriptor in state-dict order, as (rows, columns of the first / second source, inner) blocks; vectors have inner 0.
struct ParamSeg { int rows, ca, cb, inner; };
// `ua`: the CALLER's descriptor - whether a residual block has a projection is a property of the caller's widths (40 and 48 channels both run
// at 64, and the block still has its 1x1 conv); `n_blocks`: blocks per stage of a residual encoder, or null.
std::vector<ParamSeg> param_segs(const ts2d_arch_desc& a, const ts2d_arch_desc& ua, const int* n_blocks) {
    std::vector<ParamSeg> v;
    auto stride_of = [&](int s, int ax) { const int y = a.strides[s][0], x = a.strides[s][1]; return (y == 0 && x == 0) ? (s ? 2 : 1) : (ax ? x : y); };
    auto block3x3 = [&](int f, int cin) { v.push_back({f, cin, 0, 9}); v.push_back({f, 0, 0, 0}); v.push_back({f, 0, 0, 0}); v.push_back({f, 0, 0, 0}); };
    int cin = a.input_channels;
    if (n_blocks) {       // stem; per stage and block conv1, conv2, then the projection (w, gamma, beta) where the widths differ
        block3x3(a.features[0], cin);
        cin = a.features[0];
        for (int s = 0; s < a.n_stages; ++s)
            for (int b = 0; b < n_blocks[s]; ++b) {
                const int f = a.features[s];
                const bool proj = b == 0 && s > 0 && ua.features[s - 1] != ua.features[s];
                block3x3(f, cin); block3x3(f, f);
                if (proj) { v.push_back({f, cin, 0, 1}); v.push_back({f, 0, 0, 0}); v.push_back({f, 0, 0, 0}); }
                cin = f;
            }
    } else
    for (int s = 0; s < a.n_stages; ++s)
        for (int i = 0; i < a.n_conv_enc[s]; ++i) {
            const int f = a.features[s];
            block3x3(f, cin);
            cin = f;
        }
    for (int j = 0; j < a.n_stages - 1; ++j) {
        const int lvl = a.n_stages - 2 - j, f = a.features[lvl];
        v.push_back({cin, f, 0, stride_of(lvl + 1, 0) * stride_of(lvl + 1, 1)}); v.push_back({f, 0, 0, 0});      // ConvTranspose2d weight [Cin][Cout][sy][sx], bias
        for (int i = 0; i < a.n_conv_dec[j]; ++i) {
            v.push_back({f, f, i == 0 ? f : 0, 9}); v.push_back({f, 0, 0, 0}); v.push_back({f, 0, 0, 0}); v.push_back({f, 0, 0, 0});
        }
        cin = f;
    }
    v.push_back({a.num_classes, cin, 0, 1}); v.push_back({a.num_classes, 0, 0, 0});
    return v;
}

size_t segs_floats(const std::vector<ParamSeg>& v) {
    size_t n = 0;
    for (const ParamSeg& g : v) n += g.inner ? (size_t)g.rows * (g.ca + g.cb) * g.inner : (size_t)g.rows;
    return n;
}

}  // namespace

// Feature counts the MFMA tilings do not divide ("a descriptor-driven engine needs a correct generic path for what it
// cannot make fast"): every stage's width is rounded up to a multiple of 32 (stage 0: to 32 or 64, what the head kernel reads) and the network
// runs at that width with ZERO weights, bias, gamma and beta in the added channels.  Exact, not approximate: an added channel's conv output is
// 0 in every pixel, its InstanceNorm scale gamma * rsqrt(0 + eps) = 0 and shift 0, so it enters the next layer as LeakyReLU(0) = 0 under zero
// weights; the caller's channels see the same sums with zeros added.  The caller's blob keeps the caller's layout (expand_blob below).
ts2d_arch_desc pad_arch(const ts2d_arch_desc& a, bool& padded) {
    ts2d_arch_desc p = a;
    padded = false;
    for (int s = 0; s < a.n_stages && s < TS2D_MAX_STAGES; ++s) {
        if (a.features[s] < 1) continue;                       // (build_program reports it)
        p.features[s] = (a.features[s] + 31) / 32 * 32;
        padded |= p.features[s] != a.features[s];
    }
    return p;
}

// caller-layout blob -> the blob of the padded architecture (zeros in every added row / column; the second source of a decoder block's
// first conv - the skip half of cat((up, skip), 1) - starts at the PADDED width of the first)
void expand_blob(const ts2d_arch_desc& ua, const ts2d_arch_desc& pa, const int* n_blocks, const float* ub, std::vector<float>& pb) {
    const std::vector<ParamSeg> us = param_segs(ua, ua, n_blocks), ps = param_segs(pa, ua, n_blocks);
    pb.assign(segs_floats(ps), 0.f);
    size_t uo = 0, po = 0;
    for (size_t k = 0; k < us.size(); ++k) {
        const ParamSeg &u = us[k], &q = ps[k];
        if (!u.inner) {
            memcpy(pb.data() + po, ub + uo, (size_t)u.rows * sizeof(float));
            uo += u.rows; po += q.rows;
            continue;
        }
        const int ucols = u.ca + u.cb, qcols = q.ca + q.cb;
        for (int r = 0; r < u.rows; ++r)
            for (int c = 0; c < ucols; ++c) {
                const int cq = c < u.ca ? c : q.ca + (c - u.ca);
                memcpy(pb.data() + po + ((size_t)r * qcols + cq) * q.inner, ub + uo + ((size_t)r * ucols + c) * u.inner, (size_t)u.inner * sizeof(float));
            }
        uo += (size_t)u.rows * ucols * u.inner; po += (size_t)q.rows * qcols * q.inner;
    }
}

// Mirror of UNetArch.program() (totalsegmentator2d_amd/arch.py): PlainConvUNet forward order, or - `e->residual` - ResidualEncoderUNet's:
// stem, then per stage and block conv1 (3x3, the block's stride), conv2 (3x3, normalised, NOT activated), the projection of the skip path where
// the widths differ (average pool over the stride + 1x1 conv without bias + norm, not activated) and the join.  The join stores
// t = norm2(conv2) + residual BEFORE the block's LeakyReLU with scale 1 / shift 0: every consumer applies lrelu(1 * t + 0) = lrelu(t) as it
// loads (exact in fp32), so no convolution kernel knows about residual blocks.
int build_program(ts2d_engine* e) {
    const ts2d_arch_desc& a = e->arch;
    if (a.n_stages < 2 || a.n_stages > TS2D_MAX_STAGES) return fail(TS2D_ERR_INVALID, "n_stages %d out of range [2,%d]", a.n_stages, TS2D_MAX_STAGES);
    if (a.input_channels < 1 || a.num_classes < 1) return fail(TS2D_ERR_INVALID, "input_channels / num_classes must be positive");
    if (a.num_classes > 256) return fail(TS2D_ERR_INVALID, "num_classes %d > 256 is not supported", a.num_classes);
    for (int s = 0; s < a.n_stages; ++s) {
        if (e->user_arch.features[s] < 1) return fail(TS2D_ERR_INVALID, "features[%d] = %d must be positive", s, e->user_arch.features[s]);
        if (!e->residual && a.n_conv_enc[s] < 1) return fail(TS2D_ERR_INVALID, "n_conv_enc[%d] must be >= 1", s);
        if (e->residual && e->n_blocks[s] < 1) return fail(TS2D_ERR_INVALID, "n_blocks[%d] must be >= 1", s);
        if (s < a.n_stages - 1 && a.n_conv_dec[s] < 1) return fail(TS2D_ERR_INVALID, "n_conv_dec[%d] must be >= 1", s);
    }
    if (a.features[0] != 32 && a.features[0] != 64) return fail(TS2D_ERR_INVALID, "features[0] = %d: the head kernel supports at most 64 channels", e->user_arch.features[0]);
    // per-axis strides (ABI 7).  An all-zero entry = (2, 2): descriptors written for ABI <= 6 carry no strides.
    int st[TS2D_MAX_STAGES][2];
    for (int s = 0; s < a.n_stages; ++s) {
        st[s][0] = a.strides[s][0]; st[s][1] = a.strides[s][1];
        if (st[s][0] == 0 && st[s][1] == 0) { st[s][0] = st[s][1] = (s == 0) ? 1 : 2; }
        if (st[s][0] < 1 || st[s][0] > 2 || st[s][1] < 1 || st[s][1] > 2)
            return fail(TS2D_ERR_INVALID, "strides[%d] = (%d, %d): 1 or 2 per axis", s, st[s][0], st[s][1]);
        if (s == 0 && (st[0][0] != 1 || st[0][1] != 1)) return fail(TS2D_ERR_INVALID, "strides[0] must be (1, 1)");
        e->lvl_y[s] = (s ? e->lvl_y[s - 1] : 0) + (st[s][0] == 2); e->lvl_x[s] = (s ? e->lvl_x[s - 1] : 0) + (st[s][1] == 2);
    }
    auto stride_code = [](int sy, int sx) { return sy == 1 && sx == 1 ? 1 : (sy == 2 && sx == 2 ? 2 : 3); };
    e->cin_pad = (a.input_channels + 7) / 8 * 8;
    size_t bo = 0;
    int cur = add_tensor(e, "input", e->cin_pad, 0, false), cin = a.input_channels;
    std::vector<int> skips(a.n_stages);
    char nm[64];
    if (e->residual) {
        auto conv3x3 = [&](const char* name, int src, int ci, int f, int s, int sy, int sx, bool linear) {
            Op op{}; op.type = OP_CONV; op.name = name; op.src = src; op.skip = -1;
            op.cin = ci; op.cin_skip = 0; op.cout = f; op.level = s; op.ly = e->lvl_y[s]; op.lx = e->lvl_x[s];
            op.sy = sy; op.sx = sx; op.stride = stride_code(sy, sx);
            op.dst = add_tensor(e, name, f, s, true);
            e->tensors[op.dst].linear = linear;
            op.blob_w = bo; bo += (size_t)f * ci * 9; op.blob_b = bo; bo += f; op.blob_g = bo; bo += f; op.blob_be = bo; bo += f;
            e->ops.push_back(op);
            return op.dst;
        };
        cur = conv3x3("stem", cur, cin, a.features[0], 0, 1, 1, false);
        cin = a.features[0];
        for (int s = 0; s < a.n_stages; ++s) {
            const int f = a.features[s];
            for (int b = 0; b < e->n_blocks[s]; ++b) {
                const bool first = b == 0 && s > 0;
                const int sy = first ? st[s][0] : 1, sx = first ? st[s][1] : 1;
                const bool proj = first && e->user_arch.features[s - 1] != e->user_arch.features[s];
                snprintf(nm, sizeof(nm), "enc%d.b%d.c1", s, b);
                const int c1 = conv3x3(nm, cur, cin, f, s, sy, sx, false);
                snprintf(nm, sizeof(nm), "enc%d.b%d.c2", s, b);
                const int c2 = conv3x3(nm, c1, f, f, s, 1, 1, true);
                int res = cur;
                if (proj) {
                    snprintf(nm, sizeof(nm), "enc%d.b%d.proj", s, b);
                    Op op{}; op.type = OP_PROJ; op.name = nm; op.src = cur; op.skip = -1;
                    op.cin = cin; op.cin_skip = 0; op.cout = f; op.level = s; op.ly = e->lvl_y[s]; op.lx = e->lvl_x[s];
                    op.sy = sy; op.sx = sx; op.stride = stride_code(sy, sx);
                    op.dst = add_tensor(e, nm, f, s, true);
                    e->tensors[op.dst].linear = true;
                    op.blob_w = bo; bo += (size_t)f * cin; op.blob_g = bo; bo += f; op.blob_be = bo; bo += f;      // (no bias)
                    e->ops.push_back(op);
                    res = op.dst;
                }
                snprintf(nm, sizeof(nm), "enc%d.b%d", s, b);
                Op jn{}; jn.type = OP_JOIN; jn.name = nm; jn.src = c2; jn.skip = -1; jn.res = res;
                jn.cin = f; jn.cin_skip = 0; jn.cout = f; jn.level = s; jn.ly = e->lvl_y[s]; jn.lx = e->lvl_x[s];
                jn.sy = proj ? 1 : sy; jn.sx = proj ? 1 : sx;      // the window the join itself pools over (a projection has pooled already)
                jn.stride = stride_code(jn.sy, jn.sx);
                jn.dst = add_tensor(e, nm, f, s, true);           // "normed": the kernel writes scale 1 / shift 0
                e->ops.push_back(jn);
                cur = jn.dst; cin = f;
            }
            skips[s] = cur;
        }
    } else
    for (int s = 0; s < a.n_stages; ++s) {
        const int f = a.features[s];
        for (int i = 0; i < a.n_conv_enc[s]; ++i) {
            snprintf(nm, sizeof(nm), "enc%d.c%d", s, i);
            Op op{}; op.type = OP_CONV; op.name = nm; op.src = cur; op.skip = -1;
            op.cin = cin; op.cin_skip = 0; op.cout = f; op.level = s; op.ly = e->lvl_y[s]; op.lx = e->lvl_x[s];
            if (i == 0 && s > 0) { op.sy = st[s][0]; op.sx = st[s][1]; }
            op.stride = stride_code(op.sy, op.sx);
            op.dst = add_tensor(e, nm, f, s, true);
            op.blob_w = bo; bo += (size_t)f * cin * 9; op.blob_b = bo; bo += f; op.blob_g = bo; bo += f; op.blob_be = bo; bo += f;
            e->ops.push_back(op);
            cur = op.dst; cin = f;
        }
        skips[s] = cur;
    }
    for (int j = 0; j < a.n_stages - 1; ++j) {
        const int lvl = a.n_stages - 2 - j, f = a.features[lvl];
        snprintf(nm, sizeof(nm), "dec%d.up", lvl);
        Op up{}; up.type = OP_CONVT; up.name = nm; up.src = cur; up.skip = -1; up.cin = cin; up.cin_skip = 0; up.cout = f;
        up.sy = st[lvl + 1][0]; up.sx = st[lvl + 1][1];       // kernel = stride = the stride of the encoder stage below (upstream UNetDecoder)
        up.stride = stride_code(up.sy, up.sx); up.level = lvl; up.ly = e->lvl_y[lvl]; up.lx = e->lvl_x[lvl];
        up.dst = add_tensor(e, nm, f, lvl, false);
        up.blob_w = bo; bo += (size_t)cin * f * up.sy * up.sx; up.blob_b = bo; bo += f;
        e->ops.push_back(up);
        cur = up.dst;
        for (int i = 0; i < a.n_conv_dec[j]; ++i) {
            snprintf(nm, sizeof(nm), "dec%d.c%d", lvl, i);
            Op op{}; op.type = OP_CONV; op.name = nm; op.src = cur; op.skip = (i == 0) ? skips[lvl] : -1;
            op.cin = f; op.cin_skip = (i == 0) ? f : 0; op.cout = f; op.stride = 1; op.level = lvl; op.ly = e->lvl_y[lvl]; op.lx = e->lvl_x[lvl];
            op.dst = add_tensor(e, nm, f, lvl, true);
            const int ct = op.cin + op.cin_skip;
            op.blob_w = bo; bo += (size_t)f * ct * 9; op.blob_b = bo; bo += f; op.blob_g = bo; bo += f; op.blob_be = bo; bo += f;
            e->ops.push_back(op);
            cur = op.dst;
        }
        cin = f;
    }
    {
        Op hd{}; hd.type = OP_HEAD; hd.name = "head"; hd.src = cur; hd.skip = -1; hd.cin = cin; hd.cin_skip = 0;
        hd.cout = a.num_classes; hd.stride = 1; hd.level = 0; hd.dst = -1;
        hd.blob_w = bo; bo += (size_t)a.num_classes * cin; hd.blob_b = bo; bo += a.num_classes;
        e->ops.push_back(hd);
    }
    e->blob_floats = bo;
    e->user_blob_floats = e->padded ? segs_floats(param_segs(e->user_arch, e->user_arch, e->residual ? e->n_blocks : nullptr)) : bo;
    // device weight arena layout
    size_t wo = 0;
    for (Op& op : e->ops) {
        const int ct = op.cin + op.cin_skip;
        if (op.type == OP_JOIN) continue;                                // (no parameters)
        if (op.type == OP_PROJ) {                                        // W[co][ci] -> [ci][co] (pool_proj1x1 stages rows of it), gamma, beta; no bias
            op.ck = 0; op.dev_w_floats = (size_t)ct * op.cout;
            op.dev_w = wo; wo = align_up(wo + op.dev_w_floats, 64);
            op.dev_g = wo; wo = align_up(wo + op.cout, 64); op.dev_be = wo; wo = align_up(wo + op.cout, 64);
            op.dev_wh = wo; wo = align_up(wo + op.dev_w_floats / 2, 64);     // rounded to half, [chunk32][Cout][32 halves] (pool_proj1x1_h; Cin % 32 == 0: pad_arch)
            continue;
        }
        if (op.type == OP_CONV) {
            const int ctp = (op.src == 0) ? e->cin_pad : ct;             // first conv reads the zero-padded input
            op.ck = (op.stride != 1 || ctp % 16) ? 8 : 16;
            op.dev_w_floats = (size_t)ctp * 9 * op.cout;
        } else if (op.type == OP_CONVT) {
            op.ck = 16;
            op.dev_w_floats = (size_t)ct * op.sy * op.sx * op.cout;
        } else {
            op.ck = 0;
            op.dev_w_floats = (size_t)ct * op.cout;
        }
        op.dev_w = wo; wo = align_up(wo + op.dev_w_floats, 64);
        op.dev_b = wo; wo = align_up(wo + op.cout, 64);
        if (op.type == OP_CONV) { op.dev_g = wo; wo = align_up(wo + op.cout, 64); op.dev_be = wo; wo = align_up(wo + op.cout, 64); }
        if (op.type == OP_CONV && op.src != 0 && ((op.stride == 1 && ct % 16 == 0) || (op.stride == 2 && ct % 8 == 0))) {
            op.split_ok = true;        // stride 1: [chunk16][tap 9][Cout][32 halves]; stride 2: [chunk8][column tile][k-step 5][column][32 halves]
            const size_t recs = op.stride == 1 ? (size_t)(ct / 16) * 9 : (size_t)(ct / 8) * 5;
            op.dev_wh = wo; wo = align_up(wo + recs * op.cout * 16, 64);
            op.dev_ws = wo; wo = align_up(wo + 1, 64);                  // 1 / scale, read by the kernel
            if (op.stride == 1 && op.cout % 64 == 0) { op.dev_wp = wo; wo = align_up(wo + recs * op.cout * 16, 64); }      // plane order (conv3x3_f16x3_qp)
            if (op.stride == 2 && ct % 16 == 0 && op.cout % 64 == 0) {
                op.s2v2_ok = true; op.bn2 = op.cout % 128 == 0 ? 128 : 64;
                op.dev_w2 = wo; wo = align_up(wo + (size_t)ct * 9 * op.cout, 64);
            }
            if (op.stride == 1 && ct == 32 && op.cout == 32) {      // resident image of the 32 -> 32 block: [tap][hi,lo][g][cout][8 halves]
                op.res_ok = true;
                op.dev_wres = wo; wo = align_up(wo + 9 * 2 * 4 * 32 * 8 / 2, 64);
            }
            const size_t oi = (size_t)(&op - e->ops.data());
            if (op.stride == 1 && op.skip >= 0 && oi > 0 && e->ops[oi - 1].type == OP_CONVT && e->ops[oi - 1].dst == op.src &&
                e->ops[oi - 1].stride == 2 && e->ops[oi - 1].cin % 32 == 0 && op.cin % 16 == 0 && op.cin_skip % 16 == 0 && op.cout % 32 == 0 &&
                (double)op.cout * e->ops[oi - 1].cin * op.cin * 36.0 <= 6.0e9) {        // (host composition cost bound: 512 x 512 x 512 channels = 4.8 GFLOP, about a second)
                const int cb = e->ops[oi - 1].cin;
                op.upc_ok = true; op.up_idx = (int)oi - 1;
                op.dev_wc = wo; wo = align_up(wo + (size_t)cb * op.cout * 16, 64);
                op.dev_wk = wo; wo = align_up(wo + (size_t)op.cin_skip * op.cout * 9, 64);
                op.dev_wcs = wo; wo = align_up(wo + 1, 64);
                op.dev_bvar = wo; wo = align_up(wo + (size_t)9 * op.cout, 64);
                if (cb == 64 && op.cin == 32 && op.cin_skip == 32 && op.cout == 32) {
                    op.up0_ok = true;
                    op.dev_w0c = wo; wo = align_up(wo + 4 * 8 * 2 * 2 * 64 * 8 / 2, 64);
                    op.dev_w0k = wo; wo = align_up(wo + 9 * 2 * 4 * 32 * 8 / 2, 64);
                }
            }
            if (op.stride == 1 && op.cin % 32 == 0 && op.cin_skip % 32 == 0) {      // [chunk32][column tile][tap][column][32 halves]
                op.h32_ok = true;
                op.dev_wh32 = wo; wo = align_up(wo + (size_t)(ct / 32) * 9 * op.cout * 16, 64);
            }
        }
        if (op.type == OP_CONV && op.src == 0 && ct <= 4) {              // first block: PyTorch-layout fp32 copy for conv3x3_first
            op.dev_wraw = wo; wo = align_up(wo + (size_t)op.cout * ct * 9, 64);
            op.first_direct = true;
        }
        if (op.type == OP_HEAD && ct == 32 && op.cout <= 32) {          // head_mfma32: [k-step 2][column 32][16 hi | 16 lo] halves
            op.split_ok = true;
            op.dev_wh = wo; wo = align_up(wo + 2 * 32 * 16, 64);
            op.dev_ws = wo; wo = align_up(wo + 1, 64);
        }
        if (op.type == OP_CONVT && op.stride == 2 && ct % 32 == 0) {    // [chunk32][column tile of 64][k-step 2][column][32 halves]
            op.split_ok = true;
            op.dev_wh = wo; wo = align_up(wo + (size_t)(ct / 32) * 2 * 4 * op.cout * 16, 64);
            op.dev_ws = wo; wo = align_up(wo + 1, 64);
        }
    }
    e->weight_floats = wo;
    return TS2D_OK;
}

// The largest plane ONE image of an H x W forward occupies: the widest activation tensor, or the NCHW input, counted as floats in EVERY mode.  The
// kernels of the dedicated families address an image through a buffer resource whose record count is (int)plane_bytes and whose lane and scalar
// offsets are 32-bit byte offsets ("32-bit quantities of the forward path"); dispatch.cpp hands them an op only while fits32() holds for
// the op's planes at four bytes per element - the 16-bit mode included, whose buffers the workspace plan sizes for floats too - and beyond that
// falls back to the generic kernels, which no test has ever run at such a size.  reserve_checked therefore refuses where the first plane reaches
// 2^31 bytes: inside the limit fits32() holds for every op, and every accepted extent runs the kernels the suite judges.
// Extents whose pixel count alone reaches 2^31 are answered with that count (no product here leaves 64 bits).
long long image_plane_bytes(const ts2d_engine* e, int H, int W, int* widest) {
    if (widest) *widest = -1;
    if (H < 1 || W < 1 || (long long)H * W >= (1LL << 31)) return (long long)H * W;
    const long long elt = 4;
    long long worst = (long long)H * W * e->arch.input_channels * 4;
    for (size_t t = 0; t < e->tensors.size(); ++t) {
        const Tensor& x = e->tensors[t];
        const long long b = (long long)(H >> x.ly) * (W >> x.lx) * x.C * elt;
        if (b > worst) { worst = b; if (widest) *widest = (int)t; }
    }
    return worst;
}
// Pixels B * H * W one call may hold (exclusive).  2^31: the pixel index of the generic staging loops is an int.  A residual encoder: res_join (fp32
// storage) launches 256 threads per 32 pixels of a level - 8 per pixel - and a launch holds fewer than 2^32 threads, so its level-0 join ends where ceil(pixels / 32) * 256 would reach 2^32: at most 2^29 - 32 pixels.
long long call_pixel_limit(const ts2d_engine* e) { return e->residual ? (1LL << 29) - 31 : (1LL << 31); }
bool image_extent_ok(const ts2d_engine* e, int H, int W) { return H >= 1 && W >= 1 && (long long)H * W < (1LL << 31) && image_plane_bytes(e, H, W, nullptr) <= kImagePlaneMax; }

}  // namespace ts2d
