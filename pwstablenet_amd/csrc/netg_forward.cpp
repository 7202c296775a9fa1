// The generator's forward: the lockstep schedule (stages 2 and 3 as one launch per layer), the per-stage schedule, and the forward
// entry points.  The backward replays forward_graph without launching to recover the tape and every address (netg_backward.cpp).
#include "netg_exec.h"

namespace pws {

// The forward with stages 2 and 3 in lockstep (Exec::Groups): every level's tensors of the three stages are the sample groups of ONE
// buffer, the layers stages 2 and 3 share run as one launch of batch 2n wherever both stages' inputs are such views.
//   encoder level k (k = 2 .. 8, maps 128 .. 1):  Ek = [x1k | x2k | x3k]   (x32 == x22: the reference computes it twice, :178,:200)
//       x2k, x3k = mpconv_{k-1}(cat(x_left, conv_same_{k-1}(x_up))),  x_up = (x1,k-1 | x2,k-1) = groups (0, 1) of E_{k-1},
//                                                                  x_left = (x2,k-1 | x3,k-1) = groups (1, 2)
//       conv_same merges from k = 3, mpconv from k = 4 (at k = 3 x_left would be (x22 | x32) = the same tensor twice)
//   decoder level l (l = 7 .. 1):  d_s(l) = cat(V_l[s], x_sl),  V_l = [u1l | v2l | v3l];  d_s(8) = x_s8
//       v_sl = mpconv_l(cat(conv_same_l(x_up), x_left)),  x_up = (d1 | d2)(l+1), x_left = (d2 | d3)(l+1): merged for l = 7 .. 2
//       (level 1 exists for stage 3 only at inference; in training its inputs d_s(2) hold x22 twice: separate launches)
// Queues: 0 = stage-1 encoder, stage-1 decoder, then the large merged decoder levels and the heads; 1 = the stage-2/3 encoder beside the
// stage-1 decoder, then the deep merged decoder levels.
static void forward_lockstep(Exec &E, const Tn &in, const FwdArgs &a, float *th1, float *th2, float *th3) {
    const float *x = a.x;
    const int n = a.n, input_nc = a.input_nc, g = a.g, is_training = a.is_training, ac = a.ac;
    float *grids = a.grids, *resid = a.resid;
    const int S = 256;
    const size_t gsz = (size_t)n * S * S * 2;
    const int enc_c[9] = {0, g, g, 2 * g, 4 * g, 4 * g, 4 * g, 4 * g, 4 * g};        // channels of x_sk, k = 1 .. 8
    const int dec_c[8] = {0, g, g, 2 * g, 4 * g, 4 * g, 4 * g, 4 * g};               // channels of v_sl, l = 1 .. 7
    auto side = [&](int k) { return S >> (k - 1); };                                // map edge at level k
    // ---- buffers
    Exec::Groups Ek[9], Ck[9], Vl[8], Gl[8];
    for (int k = 2; k <= 8; ++k) Ek[k] = E.alloc_groups(k == 2 ? 2 : 3, side(k), side(k), enc_c[k], PWS_ACT_LRELU);   // (x32 == x22: E2 has no third group)
    for (int k = 3; k <= 8; ++k) Ck[k] = E.alloc_groups(2, side(k - 1), side(k - 1), enc_c[k - 1], PWS_ACT_LRELU);   // conv_same_{k-1}: level k-1 in, same size out
    for (int l = 7; l >= 2; --l) {
        Vl[l] = E.alloc_groups(3, side(l), side(l), dec_c[l], PWS_ACT_RELU);
        // conv_same of up_bottom level l: input x_up at level l + 1 (channels of d(l+1): v + skip, or the bottom x_s8), same size out
        const int cin = l == 7 ? enc_c[8] : dec_c[l + 1] + enc_c[l + 1];
        Gl[l] = E.alloc_groups(2, side(l + 1), side(l + 1), cin, PWS_ACT_RELU);
    }
    auto enc = [&](int k, int s) { return E.group(Ek[k], s - 1); };                 // x_sk
    auto dec = [&](int l, int s) {                                                   // d_s(l), l = 8 .. 2
        if (l == 8) return enc(8, s);
        Tn skip = s == 3 && l == 2 ? enc(2, 2) : enc(l, s);                          // x32 == x22
        return Exec::cat(E.group(Vl[l], s - 1), skip);
    };
    // ---- encoders
    auto db1 = [&](const Tn &x11) {   // down_bottom1 (:178 == :200): once, into group 1 of E2
        Tn c = E.conv(L_DB1_CS, x11, PWS_ACT_LRELU);
        E.conv_groups(L_DB1_CS + 1, c, PWS_ACT_LRELU, 1, Ek[2], 1);
    };
    auto level3 = [&]() {   // conv_same_2 on (x12 | x22) in one launch; the two mpconvs apart (both read x22 as x_left)
        E.conv_groups(L_DB1_CS + 2, enc(2, 1), PWS_ACT_LRELU, 2, Ck[3], 0);
        E.conv_groups(L_DB1_CS + 3, Exec::cat(enc(2, 2), E.group(Ck[3], 0)), PWS_ACT_LRELU, 1, Ek[3], 1);
        E.conv_groups(L_DB1_CS + 3, Exec::cat(enc(2, 2), E.group(Ck[3], 1)), PWS_ACT_LRELU, 1, Ek[3], 2);
    };
    auto enc1 = [&](int k, const Tn &x11) { E.conv_groups(L_DOWN1 + (k - 2), k == 2 ? x11 : enc(k - 1, 1), PWS_ACT_LRELU, 1, Ek[k], 0); };
    E.use(0);
    Tn x11 = E.conv(L_TRANSFER, in, PWS_ACT_LRELU, x, input_nc);
    // queue 1 starts behind x14 (its large layers beside the deeper levels of stage 1), the merged levels behind x18.  (Measured against
    // queue 1 behind x13 / x15: fp32 1815 / 1826 against 1840 f/s, bf16 6238 / 6150 against 6252.)
    for (int k = 2; k <= 4; ++k) enc1(k, x11);
    E.order(0, 1);
    E.use(1);
    db1(x11);
    level3();
    E.use(0);
    for (int k = 5; k <= 8; ++k) enc1(k, x11);
    E.order(0, 1);
    E.use(1);
    if (is_training) {
        E.use(0);
        E.theta(enc(8, 1), 0, th1);
        E.use(1);
    }
    for (int k = 4; k <= 8; ++k) {   // levels 4 .. 8, merged, on queue 1
        const int db = k - 1;   // down_bottom index
        E.conv_groups(L_DB1_CS + 2 * (db - 1), enc(k - 1, 1), PWS_ACT_LRELU, 2, Ck[k], 0);
        E.conv_groups(L_DB1_CS + 2 * (db - 1) + 1, Exec::cat(enc(k - 1, 2), E.group(Ck[k], 0)), PWS_ACT_LRELU, 2, Ek[k], 1);
    }
    // (the theta heads of stages 2 / 3 -- 30 us of GEMV launches the field heads need at the very end -- are issued on queue 1 BEHIND the deep
    //  decoder levels, where that queue has nothing else to do: in front of them they sat on the critical path)
    // ---- stage 1 decoder (reference :166-174) on queue 0
    E.use(0);
    // (PWS_NETG_PRUNE_DEAD, inference: u12 = up2's output is read by up1 and stage 2's up_bottom1 only, reference :173,:196 -- both `if is_training`)
    const int l_last = (!is_training && E.prune_dead()) ? 3 : 2;
    for (int l = 7; l >= l_last; --l) {
        E.conv_groups(L_UP7 + (7 - l), dec(l + 1, 1), PWS_ACT_RELU, 1, Vl[l], 0);
        if (l == 6) E.order(0, 1);   // u17, u16: what the deep merged levels (7 .. 5, queue 1) read of stage 1
    }
    if (is_training) {
        Tn x111 = E.up(1, dec(2, 1), nullptr);
        E.field(x111, 0, th1, ac, resid, grids);
    }
    // ---- stages 2 / 3 decoder (reference :190-198, :212-219): levels 7 .. 5 on queue 1 (behind the encoder, beside the large levels of the
    // stage-1 decoder), levels 4 .. 2 on queue 0
    auto merged_level = [&](int l) {
        E.conv_groups(L_UB7_MP + 2 * (7 - l) + 1, dec(l + 1, 1), PWS_ACT_RELU, 2, Gl[l], 0);
        E.conv_groups(L_UB7_MP + 2 * (7 - l), Exec::cat(E.group(Gl[l], 0), dec(l + 1, 2)), PWS_ACT_RELU, 2, Vl[l], 1);
    };
    E.use(1);
    for (int l = 7; l >= 5; --l) merged_level(l);
    E.order(1, 0);
    E.use(1);
    if (is_training) E.theta(enc(8, 2), 1, th2);
    E.theta(enc(8, 3), 2, th3);
    hipEvent_t th_done = E.mark(1);
    E.use(0);
    for (int l = 4; l >= 2; --l) merged_level(l);
    // ---- level 1 and the field heads
    E.wait(0, th_done);
    if (is_training) {
        Tn x211 = E.up_bottom(1, dec(2, 1), dec(2, 2), nullptr);
        E.field(x211, 1, th2, ac, resid ? resid + gsz : nullptr, grids ? grids + gsz : nullptr);
    }
    Tn x311 = E.up_bottom(1, dec(2, 2), dec(2, 3), nullptr);
    if (is_training)
        E.field(x311, 2, th3, ac, resid ? resid + 2 * gsz : nullptr, grids ? grids + 2 * gsz : nullptr);
    else
        E.field(x311, 2, th3, ac, nullptr, grids);
}

void forward_graph(Exec &E, const FwdArgs &a) {
    const float *x = a.x;
    const int n = a.n, input_nc = a.input_nc, g = a.g, is_training = a.is_training, ac = a.ac;
    float *grids = a.grids, *resid = a.resid, *thetas = a.thetas;
    const bool caller_thetas = a.caller_thetas;
    const int S = 256;
    E.reserve_scratch(g, is_training != 0);
    const size_t gsz = (size_t)n * S * S * 2;
    float *th = (thetas || caller_thetas) ? thetas : E.alloc((size_t)3 * n * 6);
    float *th1 = th, *th2 = th ? th + (size_t)n * 6 : nullptr, *th3 = th ? th + (size_t)2 * n * 6 : nullptr;

    Tn in{};
    in.nseg = 1, in.h = S, in.w = S, in.seg[0] = Seg{nullptr, input_nc, 0};
    if (!E.bn_on() && !exp_is(EXP_NETG_PER_STAGE)) {   // (15: the per-stage schedule below, A/B; the BatchNorm path keeps it: statistics are per call)
        forward_lockstep(E, in, a, th1, th2, th3);
        return;
    }
    // Queue 0 (the caller's stream): stage-1 encoder, then the three decoders.  Queue 1: the stage-2 and stage-3 encoders,
    // which only need the previous stage's ENCODER outputs -- so stage 1's latency-bound deep layers and its decoder
    // overlap with stage 2's big conv_same layers, and stage 2's decoder overlaps with stage 3's encoder.
    // The thetas of stages 1 and 2 are only outputs of the training mode (reference :235) and are skipped otherwise.
    // ---- stage 1 encoder (reference :153-160)
    E.use(0);
    Tn x11 = E.conv(L_TRANSFER, in, PWS_ACT_LRELU, x, input_nc);
    Tn x12 = E.down(1, x11), x13 = E.down(2, x12), x14 = E.down(3, x13), x15 = E.down(4, x14);
    E.order(0, 1);  // x11..x15 ready: queue 1 may start stage 2's encoder while queue 0 finishes the deep levels
    // ---- stage 2 encoder, first levels (reference :178-181) on queue 1
    E.use(1);
    Tn x22 = E.down_bottom(1, nullptr, x11);
    Tn x23 = E.down_bottom(2, &x22, x12), x24 = E.down_bottom(3, &x23, x13), x25 = E.down_bottom(4, &x24, x14);
    E.use(0);
    Tn x16 = E.down(5, x15), x17 = E.down(6, x16), x18 = E.down(7, x17);
    E.order(0, 1);  // x16..x18
    // (the theta heads are needed by the field heads only: they are issued BEHIND the marks the other queue waits for -- 30 us of
    //  GEMV launches off the critical path of every stage)
    if (is_training) E.theta(x18, 0, th1);
    E.use(1);
    Tn x26 = E.down_bottom(5, &x25, x15), x27 = E.down_bottom(6, &x26, x16), x28 = E.down_bottom(7, &x27, x17);
    hipEvent_t enc2_done = E.mark(1);
    if (is_training) E.theta(x28, 1, th2);
    hipEvent_t th2_done = is_training ? E.mark(1) : nullptr;
    // ---- stage 1 decoder (reference :166-174) on queue 0, beside the stage-2 encoder
    E.use(0);
    Tn x177 = E.up(7, x18, &x17), x166 = E.up(6, x177, &x16), x155 = E.up(5, x166, &x15);
    Tn x144 = E.up(4, x155, &x14), x133 = E.up(3, x144, &x13), x122 = E.up(2, x133, &x12);
    if (is_training) {
        Tn x111 = E.up(1, x122, nullptr);
        E.field(x111, 0, th1, ac, resid, grids);
    }
    // ---- stage 3 encoder (reference :200-206) continues on queue 1; x32 == x22 (same weights, same input)
    E.use(1);
    const Tn &x32 = x22;
    Tn x33 = E.down_bottom(2, &x32, x22), x34 = E.down_bottom(3, &x33, x23), x35 = E.down_bottom(4, &x34, x24);
    Tn x36 = E.down_bottom(5, &x35, x25), x37 = E.down_bottom(6, &x36, x26), x38 = E.down_bottom(7, &x37, x27);
    hipEvent_t enc3_done = E.mark(1);
    // ---- stage 2 decoder (reference :190-198) on queue 0, beside the stage-3 encoder: waits for stage 2's encoder only
    E.wait(0, enc2_done);
    E.use(0);
    Tn x277 = E.up_bottom(7, x18, x28, &x27), x266 = E.up_bottom(6, x177, x277, &x26);
    Tn x255 = E.up_bottom(5, x166, x266, &x25);
    hipEvent_t dec2_deep = E.mark(0);
    // ---- stage 3 decoder (reference :212-219), deep levels: on queue 1 behind the stage-3 encoder, beside the LARGE levels of the stage-2
    // decoder on queue 0 (nine latency-bound launches on <= 8 x 8 maps under three chip-filling ones)
    const bool deep_on_q1 = !E.bn_on();
    Tn x377{}, x366{}, x355{};
    hipEvent_t dec3_deep = nullptr;
    if (deep_on_q1) {
        E.use(1);
        E.wait(1, dec2_deep);
        x377 = E.up_bottom(7, x28, x38, &x37), x366 = E.up_bottom(6, x277, x377, &x36), x355 = E.up_bottom(5, x266, x366, &x35);
        dec3_deep = E.mark(1);
        E.use(0);
    }
    Tn x244 = E.up_bottom(4, x155, x255, &x24);
    Tn x233 = E.up_bottom(3, x144, x244, &x23), x222 = E.up_bottom(2, x133, x233, &x22);
    if (is_training) {
        Tn x211 = E.up_bottom(1, x122, x222, nullptr);
        E.wait(0, th2_done);
        E.field(x211, 1, th2, ac, resid ? resid + gsz : nullptr, grids ? grids + gsz : nullptr);
    }
    E.use(1);
    E.theta(x38, 2, th3);   // (behind everything the other queue waits for)
    hipEvent_t th3_done = E.mark(1);
    E.use(0);
    // ---- stage 3 decoder, large levels: joins queue 1 (nothing is issued there after the theta head)
    E.wait(0, enc3_done);
    if (deep_on_q1) E.wait(0, dec3_deep);
    else x377 = E.up_bottom(7, x28, x38, &x37), x366 = E.up_bottom(6, x277, x377, &x36), x355 = E.up_bottom(5, x266, x366, &x35);
    Tn x344 = E.up_bottom(4, x255, x355, &x34);
    Tn x333 = E.up_bottom(3, x244, x344, &x33), x322 = E.up_bottom(2, x233, x333, &x32);
    Tn x311 = E.up_bottom(1, x222, x322, nullptr);
    E.wait(0, th3_done);
    if (is_training)
        E.field(x311, 2, th3, ac, resid ? resid + 2 * gsz : nullptr, grids ? grids + 2 * gsz : nullptr);
    else
        E.field(x311, 2, th3, ac, nullptr, grids);
}

}  // namespace pws

using namespace pws;

extern "C" size_t pws_netg_workspace_bytes(int n, int input_nc, int ngf, int is_training) {
    if (n <= 0 || !valid_shape(input_nc, ngf)) return 0;
    const LayerTable L = build_layers(input_nc, ngf);
    Exec E(nullptr, L, n, Arena{}, nullptr, EXEC_SIZE, NetgOpts{PWS_MATH_FP32, PWS_STORE_FP32, false});   // the arena layout does not depend on the mode
    forward_graph(E, FwdArgs{nullptr, n, input_nc, ngf, is_training});
    return E.used();
}

extern "C" int pws_netg_forward_opts(const float *packed, const float *x, int n, int input_nc, int ngf, int is_training,
                                     int align_corners, void *ws, size_t ws_bytes, float *grids, float *resid, float *thetas,
                                     const pws_netg_opts *opts, pws_stream_t stream) {
    PWS_REQUIRE(n >= 0, "pws_netg_forward: bad n %d", n);
    PWS_REQUIRE_SHAPE("pws_netg_forward", input_nc, ngf);
    NetgOpts o;
    if (int rc = opts_from(opts, &o)) return rc;
    if (n == 0) return PWS_OK;
    PWS_REQUIRE(packed && x && ws && grids, "pws_netg_forward: NULL pointer");
    PWS_REQUIRE(!is_training || (resid && thetas), "pws_netg_forward: resid and thetas must be given when is_training");
    PWS_REQUIRE(o.x_sample_stride == 0 || (!is_training && o.x_sample_stride % 4 == 0 && o.x_sample_stride < (1u << 30)),
                "pws_netg_opts: x_sample_stride %zu: inference forward only, a multiple of 4 floats", o.x_sample_stride);
    PWS_REQUIRE((reinterpret_cast<size_t>(ws) & 255) == 0, "pws_netg_forward: workspace must be 256-byte aligned");
    const LayerTable L = build_layers(input_nc, ngf);
    Exec E(packed, L, n, Arena{static_cast<char *>(ws), ws_bytes}, as_stream(stream), EXEC_RUN, o);
    forward_graph(E, FwdArgs{x, n, input_nc, ngf, is_training, align_corners, grids, resid, thetas});
    return E.rc();
}

extern "C" int pws_netg_forward_plan(int n, int input_nc, int ngf, int is_training, const pws_netg_opts *opts, int compute_units,
                                     pws_conv_choice *out, int max) {
    PWS_REQUIRE(n >= 0 && compute_units > 0 && max >= 0 && (out || max == 0), "pws_netg_forward_plan: bad n %d / compute_units %d / out", n, compute_units);
    PWS_REQUIRE_SHAPE("pws_netg_forward_plan", input_nc, ngf);
    NetgOpts o;
    if (int rc = opts_from(opts, &o)) return rc;
    if (n == 0) return 0;
    const LayerTable L = build_layers(input_nc, ngf);
    Exec E(reinterpret_cast<const float *>(plan_base(1)), L, n, Arena{plan_base(0), (size_t)1 << 40}, nullptr, EXEC_PLAN, o);
    E.plan_for(compute_units);
    float *grids = reinterpret_cast<float *>(plan_base(2)) + ((size_t)1 << 36);   // (the heads are not planned: any non-null address)
    forward_graph(E, FwdArgs{reinterpret_cast<const float *>(plan_base(2)), n, input_nc, ngf, is_training, 0, grids, grids, grids});
    if (E.rc() != PWS_OK) return E.rc();
    const int count = (int)E.plan().size();
    for (int i = 0; i < count && i < max; ++i) out[i] = E.plan()[i];
    return count;
}

extern "C" int pws_netg_forward(const float *packed, const float *x, int n, int input_nc, int ngf, int is_training,
                                int align_corners, void *ws, size_t ws_bytes, float *grids, float *resid, float *thetas,
                                pws_stream_t stream) {
    return pws_netg_forward_opts(packed, x, n, input_nc, ngf, is_training, align_corners, ws, ws_bytes, grids, resid, thetas, nullptr,
                                 stream);
}

// ---- use_BN=True training (BatchNorm2d after every conv, batch statistics): fp32 storage only
extern "C" int pws_netg_forward_bn(const float *packed, const float *bn_params, float *bn_running, float momentum, float eps,
                                   const float *x, int n, int input_nc, int ngf, int align_corners, void *ws, size_t ws_bytes,
                                   float *grids, float *resid, float *thetas, pws_stream_t stream) {
    return pws_netg_forward_bn_opts(packed, bn_params, bn_running, momentum, eps, x, n, input_nc, ngf, align_corners, ws, ws_bytes, grids, resid,
                                    thetas, nullptr, stream);
}

extern "C" int pws_netg_forward_bn_opts(const float *packed, const float *bn_params, float *bn_running, float momentum, float eps,
                                        const float *x, int n, int input_nc, int ngf, int align_corners, void *ws, size_t ws_bytes,
                                        float *grids, float *resid, float *thetas, const pws_netg_opts *opts, pws_stream_t stream) {
    PWS_REQUIRE(n >= 0, "pws_netg_forward_bn: bad n %d", n);
    PWS_REQUIRE_SHAPE("pws_netg_forward_bn", input_nc, ngf);
    if (n == 0) return PWS_OK;
    PWS_REQUIRE(n >= 2, "pws_netg_forward_bn: training-mode BatchNorm needs more than 1 value per channel (the theta head has one per "
                        "sample): n >= 2, as torch");
    PWS_REQUIRE(packed && bn_params && x && ws && grids && resid && thetas, "pws_netg_forward_bn: NULL pointer");
    PWS_REQUIRE((reinterpret_cast<size_t>(ws) & 255) == 0, "pws_netg_forward_bn: workspace must be 256-byte aligned");
    const LayerTable L = build_layers(input_nc, ngf);
    BnCfg bn;
    bn.params = bn_params, bn.running = bn_running, bn.momentum = momentum, bn.eps = eps;
    NetgOpts o;   // opts == NULL: fp32 whatever the process defaults say
    if (int rc = bn_opts_from(opts, &o)) return rc;
    Exec E(packed, L, n, Arena{static_cast<char *>(ws), ws_bytes}, as_stream(stream), EXEC_RUN, o, &bn);
    forward_graph(E, FwdArgs{x, n, input_nc, ngf, 1, align_corners, grids, resid, thetas});
    return E.rc();
}
