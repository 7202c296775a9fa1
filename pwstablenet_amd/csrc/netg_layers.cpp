// The generator's layer table and everything that only needs it: sizes of the packed buffers and of the gradient slab, the slab's
// layout, and the whole-generator pack / unpack entry points (kernels: netg_pack.hip).
#include "netg_layers.h"

#include "netg_pack.h"

namespace pws {

KindGeom kind_geom(int kind) {
    switch (kind) {
    case PWS_CONV_K3S1:
    case PWS_CONVT_K3S1: return {3, 9, 9, true};
    case PWS_CONV_K3S2: return {3, 9, 16, true};
    case PWS_CONVT_K4S2: return {4, 16, 16, true};
    case PWS_CONV_K5S1: return {5, 25, 0, true};
    case PWS_CONV_K2S1P0: return {2, 4, 0, false};
    case PWS_CONV_K1: return {1, 1, 0, false};
    default: return {3, 9, 0, false};   // PWS_CONV_K3S1_OUT
    }
}

// Same registration order as the reference's __init__ (lib/networks_cascading.py:112-149) / spec.py.
LayerTable build_layers(int input_nc, int g) {
    LayerTable T;
    size_t &off = T.packed, &dg = T.dgrad, &gr = T.grad;
    // ring: the layer runs on maps of whole 16 x 32 (or, two samples at a time, 16 x 16) units at the reference's 256 x 256 input (conv_wring.hip)
    auto add = [&](int kind, int cin, int cout, bool ring = false) {
        Layer l{kind, cin, cout, 0, 0, 0, 0, (size_t)-1, (size_t)-1, (size_t)-1, (size_t)-1, (size_t)-1};
        l.w_off = off;
        off = align_up(off + pws_packed_weight_floats(kind, cin, cout), 64);
        l.b_off = off;
        off = align_up(off + (size_t)cout, 64);
        l.gw_off = gr;
        gr = align_up(gr + pws_packed_weight_floats(kind, cin, cout), 64);
        l.gb_off = gr;
        gr = align_up(gr + (size_t)cout, 64);
        if (kind == PWS_CONV_K3S1 || kind == PWS_CONVT_K3S1) {
            l.ww_off = off;
            off = align_up(off + pws_packed_wino_floats(cin, cout), 64);
        }
        if (ring && pws_packed_wring_floats(kind, cin, cout)) {
            l.wr_off = off;
            off = align_up(off + pws_packed_wring_floats(kind, cin, cout), 64);
        }
        // (CONVT_K4S2 has a Winograd F(3x3,2x2) kernel too, conv_wino.hip MODE 1; measured slower than the direct kernel on
        //  this generator's 32..128-pixel maps, so its weights are not packed here)
        const KindGeom kg = kind_geom(kind);
        if (kg.bf16 && ((cin + 15) / 16 * 16) % 32 == 0) {
            l.wb_off = off;
            off = align_up(off + pws_packed_bf16_floats(kg.planes, (cin + 15) / 16 * 16, cout), 64);
        }
        const size_t d = pws_packed_dgrad_floats(kind, cin, cout);
        if (d) l.dg_off = dg, dg = align_up(dg + d, 64);
        if (d && kg.bf16 && cout % 32 == 0) {
            l.dgb_off = dg;
            dg = align_up(dg + pws_packed_bf16_floats(kg.dg_taps, cout, cin), 64);
        }
        T.L.push_back(l);
    };
    const int enc[7][2] = {{g, g}, {g, 2 * g}, {2 * g, 4 * g}, {4 * g, 4 * g}, {4 * g, 4 * g}, {4 * g, 4 * g}, {4 * g, 4 * g}};
    add(PWS_CONV_K5S1, input_nc, g, true);   // (ring: the F(2x2,5x5) weights of conv_first_wino.hip, where pws_packed_wring_floats covers the shape)
    for (int i = 0; i < 7; ++i) add(PWS_CONV_K3S2, enc[i][0], enc[i][1]);
    const int dec[7][2] = {{4 * g, 4 * g}, {8 * g, 4 * g}, {8 * g, 4 * g}, {8 * g, 4 * g}, {8 * g, 2 * g}, {4 * g, g}, {2 * g, g}};
    for (int j = 0; j < 7; ++j) add(PWS_CONVT_K4S2, dec[j][0], dec[j][1], j >= 3);  // up7..up1 (up4..up1: inputs of 16^2..128^2)
    add(PWS_CONV_K3S1_OUT, g, 2);
    for (int i = 0; i < 7; ++i) {
        add(PWS_CONV_K3S1, enc[i][0], enc[i][0], i < 4);   // down_bottom1..4.conv_same: maps of 256^2..32^2
        add(PWS_CONV_K3S2, i == 0 ? enc[i][0] : 2 * enc[i][0], enc[i][1]);
    }
    const int ub[7][3] = {{4 * g, 4 * g, 8 * g}, {8 * g, 4 * g, 16 * g}, {8 * g, 4 * g, 16 * g}, {8 * g, 4 * g, 16 * g},
                          {8 * g, 2 * g, 16 * g}, {4 * g, g, 8 * g}, {2 * g, g, 4 * g}};  // (input_nc, output_nc, inner_nc)
    for (int j = 0; j < 7; ++j) {
        add(PWS_CONVT_K4S2, ub[j][2], ub[j][1], j >= 3);   // up_bottom4..1: inputs of 16^2..128^2
        add(PWS_CONVT_K3S1, ub[j][0], ub[j][0], j >= 3);
    }
    add(PWS_CONV_K2S1P0, 4 * g, 8 * g);
    add(PWS_CONV_K1, 8 * g, 6);
    return T;
}

static unsigned off32(size_t off) { return off == (size_t)-1 ? kNoOff : (unsigned)off; }

// argument blocks of the whole-generator pack / unpack kernels (netg_pack.hip)
static void fill_pack_layers(const LayerTable &L, PackLayer *out) {
    for (int i = 0; i < L_COUNT; ++i) {
        const Layer &l = L[i];
        PackLayer &p = out[i];
        const KindGeom kg = kind_geom(l.kind);
        p.kind = l.kind, p.cin = l.cin, p.cin_pad = (l.cin + 15) / 16 * 16, p.cout = l.cout, p.k = kg.ksize;
        p.planes = kg.planes, p.dg_taps = l.dg_off == (size_t)-1 ? 0 : kg.dg_taps;
        p.w_off = off32(l.w_off), p.b_off = off32(l.b_off), p.ww_off = off32(l.ww_off), p.dg_off = off32(l.dg_off), p.wr_off = off32(l.wr_off);
    }
}

}  // namespace pws

using namespace pws;

extern "C" size_t pws_netg_packed_floats(int input_nc, int ngf) {
    return valid_shape(input_nc, ngf) ? build_layers(input_nc, ngf).packed : 0;
}

extern "C" size_t pws_netg_packed_dgrad_floats(int input_nc, int ngf) {
    return valid_shape(input_nc, ngf) ? build_layers(input_nc, ngf).dgrad : 0;
}

extern "C" int pws_netg_pack_weights(const float *const *params, float *packed, int input_nc, int ngf, pws_stream_t stream) {
    return pws_netg_pack_weights_for(params, packed, input_nc, ngf, -1, stream);
}

// skip (nullable, one flag per layer): layers another launch packs (pws_netg_pack_weights_train's one-pass kernel) get no blocks here
static int pack_weights_impl(const float *const *params, float *packed, int input_nc, int ngf, int math, pws_stream_t stream, const bool *skip) {
    PWS_REQUIRE(params && packed, "pws_netg_pack_weights: NULL pointer");
    PWS_REQUIRE_SHAPE("pws_netg_pack_weights", input_nc, ngf);
    const LayerTable L = build_layers(input_nc, ngf);
    PWS_REQUIRE(L.packed < 0xffffffffu, "pws_netg_pack_weights: packed buffer too large for 32-bit offsets");
    // three launches over all layers (netg_pack.hip): torch layouts -> packed fp32 (+ biases), Winograd, bf16.  Alignment gaps
    // between the regions are never read, so there is no zero-fill pass.
    PackAllArgs a{};
    Bf16AllArgs b{};
    a.nlayers = b.nlayers = L_COUNT;
    fill_pack_layers(L, a.layer);
    unsigned nb = 0, nbw = 0, nbb = 0;
    for (int i = 0; i < L_COUNT; ++i) {
        PWS_REQUIRE(params[2 * i] && params[2 * i + 1], "pws_netg_pack_weights: params[%d] is NULL", 2 * i);
        a.params[2 * i] = params[2 * i], a.params[2 * i + 1] = params[2 * i + 1];
        const PackLayer &p = a.layer[i];
        const bool sk = skip && skip[i];
        a.first_block[i] = nb;
        if (sk) ;
        else if (pack_tiled(p.kind)) nb += pack_tiles(p.kind, p.cin_pad, p.cout, p.k) + (unsigned)((p.cout + 255) / 256);   // tiles + bias blocks
        else nb += (unsigned)(((size_t)p.planes * p.cin_pad * p.cout + p.cout + 255) / 256);
        a.first_block_wino[i] = nbw;
        // (math == bf16: a layer with bf16 weights runs on them -- run_conv sets a.math whenever wb_off exists -- and never reads its Winograd copies)
        const bool skip_wino = sk || (math == PWS_MATH_BF16 && L[i].wb_off != (size_t)-1);
        if ((p.ww_off != kNoOff || p.wr_off != kNoOff) && !skip_wino) nbw += (unsigned)(((size_t)p.cin_pad * p.cout + 255) / 256);
        Bf16Layer &q = b.layer[i];
        q.planes = p.planes, q.krows = p.cin_pad, q.ncols = p.cout, q.kpad = (p.cin_pad + 31) / 32 * 32, q.npad = (p.cout + 63) / 64 * 64;
        q.src_off = p.w_off, q.dst_off = sk ? kNoOff : off32(L[i].wb_off);
        b.first_block[i] = nbb;
        if (q.dst_off != kNoOff && math != PWS_MATH_FP32) nbb += (unsigned)(q.planes * (q.kpad / 32) * (q.npad / 64));
    }
    a.total_blocks = nb, a.total_blocks_wino = nbw, b.total_blocks = nbb;
    int rc = launch_pack_all(a, packed, as_stream(stream));
    if (rc == PWS_OK && nbb) rc = launch_bf16_all(b, packed, packed, as_stream(stream));
    return rc;
}

extern "C" int pws_netg_pack_weights_for(const float *const *params, float *packed, int input_nc, int ngf, int math, pws_stream_t stream) {
    return pack_weights_impl(params, packed, input_nc, ngf, math, stream, nullptr);
}

static int pack_weights_dgrad_impl(const float *const *params, float *packed_dgrad, int input_nc, int ngf, pws_stream_t stream, const bool *skip) {
    PWS_REQUIRE(params && packed_dgrad, "pws_netg_pack_weights_dgrad: NULL pointer");
    PWS_REQUIRE_SHAPE("pws_netg_pack_weights_dgrad", input_nc, ngf);
    const LayerTable L = build_layers(input_nc, ngf);
    PWS_REQUIRE(L.dgrad < 0xffffffffu, "pws_netg_pack_weights_dgrad: buffer too large for 32-bit offsets");
    PackAllArgs a{};
    Bf16AllArgs b{};
    a.nlayers = b.nlayers = L_COUNT;
    fill_pack_layers(L, a.layer);
    unsigned nb = 0, nbb = 0;
    for (int i = 0; i < L_COUNT; ++i) {
        a.params[2 * i] = params[2 * i], a.params[2 * i + 1] = nullptr;
        const PackLayer &p = a.layer[i];
        a.first_block_dgrad[i] = nb;
        Bf16Layer &q = b.layer[i];
        q = Bf16Layer{};
        q.dst_off = kNoOff;
        b.first_block[i] = nbb;
        if (p.dg_off == kNoOff || (skip && skip[i])) continue;
        PWS_REQUIRE(params[2 * i], "pws_netg_pack_weights_dgrad: params[%d] is NULL", 2 * i);
        if (pack_tiled(p.kind)) nb += pack_tiles(p.kind, p.cin, p.cout, p.k);
        else nb += (unsigned)(((size_t)p.dg_taps * p.cin * p.cout + 255) / 256);
        q.planes = p.dg_taps, q.krows = p.cout, q.ncols = p.cin, q.kpad = (p.cout + 31) / 32 * 32, q.npad = (p.cin + 63) / 64 * 64;
        q.src_off = p.dg_off, q.dst_off = off32(L[i].dgb_off);
        if (q.dst_off != kNoOff) nbb += (unsigned)(q.planes * (q.kpad / 32) * (q.npad / 64));
    }
    a.total_blocks_dgrad = nb, b.total_blocks = nbb;
    int rc = nb ? launch_dgrad_all(a, packed_dgrad, as_stream(stream)) : PWS_OK;
    if (rc == PWS_OK) rc = launch_bf16_all(b, packed_dgrad, packed_dgrad, as_stream(stream));
    return rc;
}

extern "C" int pws_netg_pack_weights_dgrad(const float *const *params, float *packed_dgrad, int input_nc, int ngf,
                                           pws_stream_t stream) {
    return pack_weights_dgrad_impl(params, packed_dgrad, input_nc, ngf, stream, nullptr);
}

// Both buffers of a TRAINING step at once.  math == PWS_MATH_BF16: the conv layers whose padded extents are the real ones (every one of them
// at ngf % 64 == 0) go torch layout -> bf16 forward copy + bf16 data-gradient copy in ONE pass (pack16_all_kernel: one read of the 194 MB,
// no fp32 packed copies -- nothing reads them in this mode: run_conv and the data-gradient calls take the bf16 copies whenever they
// exist, and at these channel counts the bf16 kernels never decline: tests/test_conv_plan_cpu.py asserts it on the ladder's plan); the heads' small tensors and any layer that does not qualify take
// the ordinary path.  Otherwise: pws_netg_pack_weights_for + pws_netg_pack_weights_dgrad.
extern "C" int pws_netg_pack_weights_train(const float *const *params, float *packed, float *packed_dgrad, int input_nc, int ngf, int math,
                                           pws_stream_t stream) {
    PWS_REQUIRE(params && packed && packed_dgrad, "pws_netg_pack_weights_train: NULL pointer");
    PWS_REQUIRE_SHAPE("pws_netg_pack_weights_train", input_nc, ngf);
    bool fused[L_COUNT] = {};
    int nfused = 0;
    const LayerTable L = build_layers(input_nc, ngf);
    PWS_REQUIRE(L.packed < 0xffffffffu && L.dgrad < 0xffffffffu, "pws_netg_pack_weights_train: buffers too large for 32-bit offsets");
    Pack16Args f{};
    f.nlayers = L_COUNT;
    fill_pack_layers(L, f.layer);
    unsigned nb = 0;
    for (int i = 0; i < L_COUNT; ++i) {
        PWS_REQUIRE(params[2 * i] && params[2 * i + 1], "pws_netg_pack_weights_train: params[%d] is NULL", 2 * i);
        f.params[2 * i] = params[2 * i], f.params[2 * i + 1] = params[2 * i + 1];
        const PackLayer &p = f.layer[i];
        const Layer &l = L[i];
        const bool has_dg = l.dg_off != (size_t)-1;
        bool ok = math == PWS_MATH_BF16 && !exp_is(EXP_NO_PACK_ONE_PASS) && pack_tiled(p.kind) && l.wb_off != (size_t)-1 && p.cout % 64 == 0 && p.cin_pad % 32 == 0;
        if (ok && has_dg) ok = l.dgb_off != (size_t)-1 && p.cin % 64 == 0;   // (cout % 64 == 0 covers the data-gradient copy's k padding)
        // every source of the layer must be a multiple of 32 channels, or the bf16 kernels decline and fall back to the fp32 copies:
        // sources are sums of ngf multiples, ngf % 32 == 0 settles it
        ok = ok && ngf % 32 == 0;
        // the first layer reads the caller's NCHW window: run_conv takes its bf16 kernel only for windows of <= 32 channels (the NHWC-32 copy);
        // a wider window goes to the fp32 first-layer kernels, which read the fp32 packed copy -- so that copy must exist
        if (i == L_TRANSFER) ok = ok && input_nc <= 32;
        fused[i] = ok, nfused += ok ? 1 : 0;
        f.first_block[i] = nb;
        f.wb_off[i] = ok ? off32(l.wb_off) : kNoOff;
        f.dgb_off[i] = ok && has_dg ? off32(l.dgb_off) : kNoOff;
        if (ok) nb += pack_tiles(p.kind, p.cin_pad, p.cout, p.k) + (unsigned)((p.cout + 255) / 256);
    }
    f.total_blocks = nb;
    int rc = nfused ? launch_pack16_all(f, packed, packed_dgrad, as_stream(stream)) : PWS_OK;
    if (rc == PWS_OK) rc = pack_weights_impl(params, packed, input_nc, ngf, math, stream, nfused ? fused : nullptr);
    if (rc == PWS_OK) rc = pack_weights_dgrad_impl(params, packed_dgrad, input_nc, ngf, stream, nfused ? fused : nullptr);
    return rc;
}

extern "C" int pws_netg_unpack_grads(const float *dpacked, float *const *grads, int input_nc, int ngf, pws_stream_t stream) {
    PWS_REQUIRE(dpacked && grads, "pws_netg_unpack_grads: NULL pointer");
    PWS_REQUIRE_SHAPE("pws_netg_unpack_grads", input_nc, ngf);
    const LayerTable L = build_layers(input_nc, ngf);
    UnpackAllArgs a{};
    a.nlayers = L_COUNT;
    fill_pack_layers(L, a.layer);
    for (int i = 0; i < L_COUNT; ++i) a.layer[i].w_off = off32(L[i].gw_off), a.layer[i].b_off = off32(L[i].gb_off);   // the gradient slab's layout
    unsigned nb = 0;
    for (int i = 0; i < L_COUNT; ++i) {
        // a layer whose two pointers are both NULL is skipped (part-wise unpacking, pws_netg_backward_part)
        PWS_REQUIRE((grads[2 * i] != nullptr) == (grads[2 * i + 1] != nullptr), "pws_netg_unpack_grads: grads[%d], grads[%d]: one is NULL",
                    2 * i, 2 * i + 1);
        a.grads[2 * i] = grads[2 * i], a.grads[2 * i + 1] = grads[2 * i + 1];
        const PackLayer &p = a.layer[i];
        a.first_block[i] = nb;
        if (grads[2 * i] && pack_tiled(p.kind)) nb += pack_tiles(p.kind, p.cin, p.cout, p.k) + (unsigned)((p.cout + 255) / 256);
        else if (grads[2 * i]) nb += (unsigned)(((size_t)p.k * p.k * p.cin * p.cout + p.cout + 255) / 256);
    }
    a.total_blocks = nb;
    if (nb == 0) return PWS_OK;
    return launch_unpack_all(a, dpacked, as_stream(stream));  // one launch: up to 46 weights + 46 biases
}

// floats of the BatchNorm parameters of use_BN=True training, per layer [gamma(cout) | beta(cout)] (netg_exec.h BnCfg)
extern "C" size_t pws_netg_bn_floats(int input_nc, int ngf) {
    if (!valid_shape(input_nc, ngf)) return 0;
    size_t bn = 0;
    for (const Layer &l : build_layers(input_nc, ngf).L) bn += 2 * (size_t)l.cout;
    return bn;
}

extern "C" size_t pws_netg_grad_floats(int input_nc, int ngf) {
    return valid_shape(input_nc, ngf) ? build_layers(input_nc, ngf).grad : 0;
}

extern "C" int pws_netg_grad_layout(int input_nc, int ngf, size_t *first_float, size_t *floats) {
    PWS_REQUIRE_SHAPE("pws_netg_grad_layout", input_nc, ngf);
    PWS_REQUIRE(first_float && floats, "pws_netg_grad_layout: NULL pointer");
    const LayerTable L = build_layers(input_nc, ngf);
    for (int i = 0; i < L_COUNT; ++i) {
        first_float[i] = L[i].gw_off;
        floats[i] = (i + 1 < L_COUNT ? L[i + 1].gw_off : L.grad) - L[i].gw_off;   // weight, bias and their padding: adjacent layers abut
    }
    return PWS_OK;
}
