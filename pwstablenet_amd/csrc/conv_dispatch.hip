// The conv dispatch ladder: which kernel family runs a forward conv / a data gradient.  pws_conv2d_fwd and pws_conv2d_bwd_data check
// their arguments, set up the ConvKParams block, and then ask the families in a fixed order; the first one that takes the launch wins.
// A family decides from the shapes, the strides, the pointers' alignment and the CU count alone (its plan step makes no HIP call), so
// the same ladder answers "what would run" without a device: pws_conv2d_fwd_plan / pws_conv2d_bwd_data_plan, and the generator's
// pws_netg_forward_plan (netg_forward.cpp) walk it with ConvCtx.launch = false.  tools/conv_plan_table.py prints the outcome per layer;
// tests/golden/conv_dispatch.json pins it.
#include "conv_common.h"

namespace pws {

// Parity ledger (tools/parity_budget.py): PWS_OPT_EXPERIMENT 3000 + mask takes ONE kernel family of the fp32 forward at a time back to the plain
// direct fp32 kernel (conv_mfma_kernel), so that the whole-network error can be attributed family by family.  Bits: 1 = first layer (no
// F(2x2,5x5), no planar-LDS kernel), 2 = the 3x3 stride-1 Winograd kernels, 4 = the transposed layers' F(2x2,2x2), 8 = conv_ringf_kernel,
// 16 = conv_skinny_kernel.  Measurement only: nothing in the product sets it.
static inline bool ledger_direct(int bit) { return (exp_mask(EXP_PARITY_LEDGER, 32) & bit) != 0; }

int conv2d_fwd_impl(const pws_conv_args *a, const ConvCtx &cx) {
    PWS_REQUIRE(a != nullptr, "pws_conv2d_fwd: args is NULL");
    PWS_REQUIRE(a->n >= 0 && a->h > 0 && a->w > 0, "pws_conv2d_fwd: bad n/h/w %d/%d/%d", a->n, a->h, a->w);
    PWS_REQUIRE(a->nsrc >= 1 && a->nsrc <= 4, "pws_conv2d_fwd: nsrc %d not in 1..4", a->nsrc);
    PWS_REQUIRE(a->cout > 0 && a->cout % 4 == 0, "pws_conv2d_fwd: cout %d must be a positive multiple of 4", a->cout);
    PWS_REQUIRE(a->out && a->w_packed, "pws_conv2d_fwd: NULL out / w_packed");
    PWS_REQUIRE(a->out_ld >= a->cout, "pws_conv2d_fwd: out_ld %d < cout %d", a->out_ld, a->cout);
    PWS_REQUIRE(a->act >= PWS_ACT_NONE && a->act <= PWS_ACT_RELU, "pws_conv2d_fwd: bad act %d", a->act);
    PWS_REQUIRE(a->ws == nullptr || (reinterpret_cast<size_t>(a->ws) & 15) == 0, "pws_conv2d_fwd: ws must be 16-B aligned");
    if (a->n == 0) return PWS_OK;

    ConvKParams kp{};
    int cin = 0;
    kp.nsrc = a->nsrc;
    const bool nchw = a->src_nchw != 0;
    if (nchw) {
        PWS_REQUIRE(a->kind == PWS_CONV_K5S1 && a->nsrc == 1, "pws_conv2d_fwd: NCHW source only for the k5 first layer");
        PWS_REQUIRE(a->src[0].ptr && a->src[0].channels > 0, "pws_conv2d_fwd: bad NCHW source");
        PWS_REQUIRE(a->src[0].ld >= 0, "pws_conv2d_fwd: NCHW source: ld is the sample stride in floats (0 = dense)");
        kp.src_ptr[0] = a->src[0].ptr, kp.src_c[0] = a->src[0].channels, kp.src_ld[0] = a->src[0].ld;
        cin = a->src[0].channels;
    } else {
        for (int s = 0; s < a->nsrc; ++s) {
            const pws_src &sr = a->src[s];
            PWS_REQUIRE(sr.ptr && sr.channels > 0 && sr.channels % 16 == 0 && sr.ld >= sr.channels && sr.ld % 4 == 0 &&
                            (reinterpret_cast<size_t>(sr.ptr) & 15) == 0,
                        "pws_conv2d_fwd: source %d (channels %d, ld %d) must be 16-B aligned, channels %% 16 == 0, ld %% 4 == 0",
                        s, sr.channels, sr.ld);
            kp.src_ptr[s] = sr.ptr, kp.src_c[s] = sr.channels, kp.src_ld[s] = sr.ld;
            cin += sr.channels;
        }
    }
    kp.cin_pad = (cin + 15) / 16 * 16;
    kp.N = a->n, kp.H = a->h, kp.W = a->w;
    kp.cout = a->cout, kp.w = a->w_packed, kp.bias = a->bias, kp.out_ld = a->out_ld, kp.act = a->act;
    kp.nclasses = 1;
    PWS_REQUIRE((size_t)a->n * a->h * a->w < (1u << 31), "pws_conv2d_fwd: n*h*w too large for 32-bit pixel indices");
    float *ws = static_cast<float *>(a->ws);
    const size_t ws_floats = a->ws_bytes / sizeof(float);
    const bool bf16 = a->math == PWS_MATH_BF16 && a->w_bf16 && !nchw;
    if (a->store == PWS_STORE_BF16) {
        PWS_REQUIRE(bf16, "pws_conv2d_fwd: bf16 storage needs math == PWS_MATH_BF16, w_bf16 and NHWC sources");
        PWS_REQUIRE(a->out_ld % 2 == 0 && a->cout % 2 == 0 && (reinterpret_cast<size_t>(a->out) & 3) == 0,
                    "pws_conv2d_fwd: bf16 storage needs an even cout / out_ld and a 4-byte aligned out");
        for (int s = 0; s < a->nsrc; ++s)
            PWS_REQUIRE(a->src[s].channels % 32 == 0 && a->src[s].ld % 8 == 0,
                        "pws_conv2d_fwd: bf16 storage needs channels %% 32 == 0 and ld %% 8 == 0 (source %d: %d, %d)", s,
                        a->src[s].channels, a->src[s].ld);
        kp.io_bf16 = 1;
        kp.epi16 = a->cout % 8 == 0 && a->out_ld % 8 == 0 && (reinterpret_cast<size_t>(a->out) & 15) == 0;
    }
    kp.w_bf = a->w_bf16, kp.kpad_bf = (kp.cin_pad + 31) / 32 * 32, kp.npad_bf = (a->cout + 63) / 64 * 64;
    if (a->out_sign) {
        PWS_REQUIRE(a->store == PWS_STORE_BF16 && a->cout % 8 == 0 && a->out_sign_ld >= a->cout / 8,
                    "pws_conv2d_fwd: out_sign needs bf16 storage, cout %% 8 == 0 and out_sign_ld >= cout / 8");
        kp.out_sign = a->out_sign, kp.out_sign_ld = a->out_sign_ld;
    }

    // the sides of the ladder: what each rung needs beside the family's own coverage test
    const bool fp32_nhwc = !bf16 && !nchw, k5 = a->kind == PWS_CONV_K5S1;
    const bool ringf_on = fp32_nhwc && !k5 && !ledger_direct(8), skinny_on = fp32_nhwc && !k5 && !ledger_direct(16);
    int k2;   // taps per output pixel
    bool wring_on = false, wino_on = false;
    switch (a->kind) {
    case PWS_CONV_K3S1:
    case PWS_CONVT_K3S1: {
        kp.OH = kp.LH = a->h, kp.OW = kp.LW = a->w, k2 = 9;
        // second-generation Winograd (persistent LDS ring) where whole 16 x 32 units fill the chip
        wring_on = a->w_wring && fp32_nhwc && !ledger_direct(2);
        // Winograd F(2x2,3x3) when there is enough of the map to fill the chip (measured cross-over, tools/conv_bench.py:
        // 256->256 @32x32 x8: 104 -> 79 us; 512->512 @16x16 x8: 106 -> 138 us); the deep maps stay direct + split-K
        // (measured: with <= 64 input channels the per-workgroup prologue/epilogue outweighs the saving unless the map is huge)
        const long wblocks = cdiv(a->w, 16) * cdiv(a->h, 16) * a->n * cdiv(a->cout, 64);
        wino_on = a->w_wino && !nchw && a->h >= 16 && a->w >= 16 && wblocks >= 128 && (cin >= 128 || wblocks >= 2048) && !ledger_direct(2);
        break;
    }
    case PWS_CONV_K3S2: kp.OH = kp.LH = (a->h + 2 - 3) / 2 + 1, kp.OW = kp.LW = (a->w + 2 - 3) / 2 + 1, k2 = 9; break;
    case PWS_CONV_K5S1:
        kp.OH = kp.LH = a->h, kp.OW = kp.LW = a->w, k2 = 25;
        ws = nullptr;   // (no K split for the first layer: no family looks at ws_floats then)
        break;
    case PWS_CONVT_K4S2: {
        kp.LH = a->h, kp.LW = a->w, kp.OH = 2 * a->h, kp.OW = 2 * a->w, kp.nclasses = 4, k2 = 4;  // every output pixel sees 2x2 taps
        // Winograd F(2x2,2x2) per parity class on the LDS ring (whole 16 x 32 input units)
        wring_on = a->w_wring && fp32_nhwc && !ledger_direct(4);
        // Winograd F(3x3,2x2) per parity class (4 classes x 12x24-pixel workgroups) when the caller packed the weights for it.
        // Measured (tools/conv_bench.py, N=8): 256->64 @128x128 646 vs 661 us direct, but 512->64 @64x64 473 vs 333 us -- the
        // 3-pixel tiles waste 21-41 % of a 64/32-pixel map and the 9-output epilogue is 2.25x the F(2x2,3x3) one -- so the
        // generator's executor does not pack these weights; the path stays available for large maps.
        const long wb = cdiv(a->w, 24) * cdiv(a->h, 12) * a->n * cdiv(a->cout, 64) * 4;
        wino_on = a->w_wino && a->h >= 24 && a->w >= 24 && wb >= 256 && !ledger_direct(4);
        break;
    }
    default:
        set_error("pws_conv2d_fwd: kind %d is not a runnable conv kind", a->kind);
        return PWS_EINVAL;
    }
    // algorithmic work of this launch (real channels, each tensor touched once)
    const double out_pix = (double)a->n * kp.OH * kp.OW, es = a->store == PWS_STORE_BF16 ? 2.0 : 4.0, ws_ = bf16 ? 2.0 : 4.0;   // activation / weight element size
    ProfInfo pi{2.0 * out_pix * a->cout * (double)cin * k2, es * ((double)a->n * a->h * a->w * cin + out_pix * a->cout) + ws_ * (double)k2 * cin * a->cout};
    if (a->kind == PWS_CONVT_K4S2) pi.bytes += ws_ * 12.0 * cin * a->cout;   // all 16 taps of the weight are read
    int rc = PWS_OK;
    // ---- the ladder: first acceptance wins
    if (bf16 && conv_bf16_fwd(a->kind, kp, kp.cin_pad, a->out, ws, ws_floats, pi, cx, &rc)) return rc;   // conv_ring / conv_skinny16 / conv_bf16(_k5) kernels
    if (wring_on && conv_wring(a, pi, cx, &rc)) return rc;
    if (wino_on && conv_wino(a, pi, cx, &rc)) return rc;
    kp.out = a->out;
    if (ringf_on && conv_ringf(a->kind, kp, pi, cx, &rc)) return rc;                           // the persistent LDS-ring kernel (exact fp32)
    if (skinny_on && conv_skinny(a->kind, kp, a->out, ws, ws_floats, pi, cx, &rc)) return rc;        // the deep levels: one-shot weight fetch
    if (k5 && nchw && !ledger_direct(1)) {   // the first layer's persistent kernels (the generator's 256 x 256 windows)
        if (a->w_wring && conv_first_wino(kp, static_cast<const float *>(a->w_wring), pi, cx, &rc)) return rc;                          // Winograd F(2x2,5x5): whole 8 x 16 units that fill the chip
        if (conv_first(kp, pi, cx, &rc)) return rc;                                                   // planar LDS
    }
    conv_mfma(a->kind, false, nchw, kp, kp.cin_pad, a->out, ws, ws_floats, pi, cx, &rc);
    return rc;
}

// Data gradient of one forward layer: dx (scattered over the forward layer's sources) from dy.
// Every case is again a convolution of dy, run by the same kernel with re-packed weights (pack.hip, dgrad layouts).
int conv2d_bwd_data_impl(const pws_conv_bwd_data_args *a, const ConvCtx &cx) {
    PWS_REQUIRE(a != nullptr, "pws_conv2d_bwd_data: args is NULL");
    PWS_REQUIRE(a->n >= 0 && a->h > 0 && a->w > 0 && a->cout > 0 && a->cout % 16 == 0, "pws_conv2d_bwd_data: bad shape");
    PWS_REQUIRE(a->gout && a->w_dgrad && a->gout_ld >= a->cout && a->gout_ld % 4 == 0, "pws_conv2d_bwd_data: bad gout / weights");
    PWS_REQUIRE(a->ndst >= 1 && a->ndst <= 4, "pws_conv2d_bwd_data: ndst %d not in 1..4", a->ndst);
    if (a->n == 0) return PWS_OK;
    ConvKParams kp{};
    int oh = a->h, ow = a->w;  // forward OUTPUT extent = extent of gout
    if (a->kind == PWS_CONV_K3S2) oh = (a->h - 1) / 2 + 1, ow = (a->w - 1) / 2 + 1;
    if (a->kind == PWS_CONVT_K4S2) oh = 2 * a->h, ow = 2 * a->w;
    kp.nsrc = 1, kp.src_ptr[0] = a->gout, kp.src_c[0] = a->cout, kp.src_ld[0] = a->gout_ld;
    kp.N = a->n, kp.H = oh, kp.W = ow;
    kp.OH = a->h, kp.OW = a->w;  // dx has the forward INPUT extent
    kp.cin_pad = a->cout;
    int cin_f = 0;
    kp.ndst = a->ndst;
    for (int s = 0; s < a->ndst; ++s) {
        const pws_dst &d = a->dst[s];
        PWS_REQUIRE(d.ptr && d.channels > 0 && d.ld >= d.channels, "pws_conv2d_bwd_data: bad destination %d", s);
        kp.dst_ptr[s] = d.ptr, kp.dst_c0[s] = cin_f, kp.dst_c1[s] = cin_f + d.channels, kp.dst_ld[s] = d.ld;
        kp.dst_acc[s] = d.accumulate ? 1 : 0;
        if (d.act_y && d.act != PWS_ACT_NONE) {
            PWS_REQUIRE(a->store == PWS_STORE_BF16 && (d.act == PWS_ACT_LRELU || d.act == PWS_ACT_RELU),
                        "pws_conv2d_bwd_data: the fused act' (dst[%d].act_y) needs bf16 storage and PWS_ACT_LRELU / PWS_ACT_RELU", s);
            PWS_REQUIRE(d.act_y_ld >= d.channels && d.act_y_ld % 2 == 0 && (reinterpret_cast<size_t>(d.act_y) & 3) == 0,
                        "pws_conv2d_bwd_data: bad act_y / act_y_ld of destination %d", s);
            kp.dst_y[s] = d.act_y, kp.dst_y_ld[s] = d.act_y_ld, kp.dst_act[s] = d.act;
            if (d.act_sign) {
                PWS_REQUIRE(d.channels % 8 == 0 && d.act_sign_ld >= d.channels / 8, "pws_conv2d_bwd_data: bad act_sign / act_sign_ld of destination %d", s);
                kp.dst_sign[s] = d.act_sign, kp.dst_sign_ld[s] = d.act_sign_ld;
            }
        }
        cin_f += d.channels;
    }
    PWS_REQUIRE(cin_f % 4 == 0, "pws_conv2d_bwd_data: total destination channels %d must be a multiple of 4", cin_f);
    kp.cout = cin_f, kp.w = a->w_dgrad, kp.bias = nullptr, kp.act = PWS_ACT_NONE, kp.out_ld = cin_f, kp.nclasses = 1;
    PWS_REQUIRE((size_t)a->n * oh * ow < (1u << 31) && (size_t)a->n * a->h * a->w < (1u << 31), "pws_conv2d_bwd_data: too large");
    float *ws = static_cast<float *>(a->ws);
    const size_t ws_floats = a->ws_bytes / sizeof(float);
    ProfInfo pi;
    const double k2 = a->kind == PWS_CONVT_K4S2 ? 4.0 : 9.0;  // taps per forward OUTPUT pixel
    pi.flops = 2.0 * a->n * oh * ow * (double)a->cout * cin_f * k2;
    // algorithmic bytes: dy read once, every destination written once -- plus what the fused epilogue reads: the old gradient of
    // an accumulating destination and the forward tensor whose act' multiplies the sum (bf16 storage: 2 bytes per element)
    {
        const double es = a->store == PWS_STORE_BF16 ? 2.0 : 4.0, in_pix = (double)a->n * a->h * a->w;
        pi.bytes = es * ((double)a->n * oh * ow * a->cout + in_pix * cin_f);
        for (int s = 0; s < a->ndst; ++s)
            pi.bytes += es * in_pix * a->dst[s].channels * (a->dst[s].accumulate ? 1.0 : 0.0) +
                        (kp.dst_act[s] == PWS_ACT_NONE ? 0.0 : (kp.dst_sign[s] ? in_pix * a->dst[s].channels / 8.0 : es * in_pix * a->dst[s].channels));
    }
    if (a->kind == PWS_CONV_K3S2)
        kp.LH = oh, kp.LW = ow, kp.nclasses = 4;
    else
        kp.LH = a->h, kp.LW = a->w;
    if (a->store == PWS_STORE_BF16) {
        PWS_REQUIRE(a->math == PWS_MATH_BF16 && a->w_dgrad_bf16 && a->cout % 32 == 0 && a->gout_ld % 8 == 0,
                    "pws_conv2d_bwd_data: bf16 storage needs bf16 math, w_dgrad_bf16, cout %% 32 == 0 and gout_ld %% 8 == 0");
        for (int s = 0; s < a->ndst; ++s)
            PWS_REQUIRE(a->dst[s].channels % 2 == 0 && a->dst[s].ld % 2 == 0 && (reinterpret_cast<size_t>(a->dst[s].ptr) & 3) == 0,
                        "pws_conv2d_bwd_data: bf16 storage needs even channels / ld and 4-byte aligned destinations");
        kp.io_bf16 = 1;
        kp.epi16 = 1;
        for (int s = 0; s < a->ndst; ++s)
            if (a->dst[s].channels % 8 || a->dst[s].ld % 8 || (reinterpret_cast<size_t>(a->dst[s].ptr) & 15) ||
                (kp.dst_act[s] != PWS_ACT_NONE && (kp.dst_y_ld[s] % 8 || (reinterpret_cast<size_t>(kp.dst_y[s]) & 15))))
                kp.epi16 = 0;
    }
    int rc = PWS_OK;
    // ---- the ladder: the bf16 kernels (conv_ring / conv_skinny16 / conv_bf16) where the call has their weights, else the direct fp32 kernel
    if (a->math == PWS_MATH_BF16 && a->w_dgrad_bf16) {
        kp.w_bf = a->w_dgrad_bf16, kp.kpad_bf = (a->cout + 31) / 32 * 32, kp.npad_bf = (cin_f + 63) / 64 * 64;
        if (conv_bf16_dgrad(a->kind, kp, a->cout, ws, ws_floats, pi, cx, &rc)) return rc;
    }
    if (a->kind != PWS_CONV_K3S1 && a->kind != PWS_CONVT_K3S1 && a->kind != PWS_CONV_K3S2 && a->kind != PWS_CONVT_K4S2) {
        set_error("pws_conv2d_bwd_data: kind %d has no data gradient here", a->kind);
        return PWS_EINVAL;
    }
    conv_mfma(a->kind, true, false, kp, a->cout, nullptr, ws, ws_floats, pi, cx, &rc);
    return rc;
}

}  // namespace pws

static pws::ConvCtx run_ctx(pws_stream_t stream) { return pws::ConvCtx{pws::as_stream(stream), pws::device_cus(), true, nullptr}; }
static pws::ConvCtx plan_ctx(int compute_units, pws_conv_choice *out) {
    *out = pws_conv_choice{};
    out->kernel_id = -1;
    return pws::ConvCtx{nullptr, compute_units, false, out};
}

extern "C" int pws_conv2d_fwd(const pws_conv_args *args, pws_stream_t stream) { return pws::conv2d_fwd_impl(args, run_ctx(stream)); }

extern "C" int pws_conv2d_bwd_data(const pws_conv_bwd_data_args *args, pws_stream_t stream) {
    return pws::conv2d_bwd_data_impl(args, run_ctx(stream));
}

extern "C" int pws_conv2d_fwd_plan(const pws_conv_args *args, int compute_units, pws_conv_choice *out) {
    PWS_REQUIRE(out && compute_units > 0, "pws_conv2d_fwd_plan: NULL out / compute_units %d", compute_units);
    return pws::conv2d_fwd_impl(args, plan_ctx(compute_units, out));
}

extern "C" int pws_conv2d_bwd_data_plan(const pws_conv_bwd_data_args *args, int compute_units, pws_conv_choice *out) {
    PWS_REQUIRE(out && compute_units > 0, "pws_conv2d_bwd_data_plan: NULL out / compute_units %d", compute_units);
    return pws::conv2d_bwd_data_impl(args, plan_ctx(compute_units, out));
}
