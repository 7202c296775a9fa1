// The generator's backward: a pure host PLAN of the reversed tape (which ops run, what each data-gradient call overwrites or
// accumulates and which act' it fuses, how the weight gradients pair up, where each layer's gradient becomes final), the LAUNCHER
// that walks a slice of that plan with the arena's addresses, and the backward entry points.
#include <algorithm>

#include "netg_exec.h"

namespace pws {

// upstream gradients of the six fields, one pointer per stage (NULL: that output has no gradient)
struct UpGrads {
    const float *grids[3] = {nullptr, nullptr, nullptr}, *resid[3] = {nullptr, nullptr, nullptr};
    UpGrads() = default;
    UpGrads(const float *g_grids, const float *g_resid, size_t gsz) {   // the stacked [3][n,256,256,2] form
        for (int k = 0; k < 3; ++k) grids[k] = g_grids ? g_grids + k * gsz : nullptr, resid[k] = g_resid ? g_resid + k * gsz : nullptr;
    }
    UpGrads(const float *const *g_grids, const float *const *g_resid) {   // HOST arrays of 3 device pointers (either may be NULL)
        for (int k = 0; k < 3; ++k) grids[k] = g_grids ? g_grids[k] : nullptr, resid[k] = g_resid ? g_resid[k] : nullptr;
    }
    bool any() const {
        for (int k = 0; k < 3; ++k)
            if (grids[k] || resid[k]) return true;
        return false;
    }
};

// ---------------------------------------------------------------- the plan
// What decides a backward besides the tape: which upstream gradients exist and the mode.
struct PlanMode {
    bool grid[3] = {true, true, true}, resid[3] = {true, true, true};
    bool fuse_act = false;   // bf16 storage: act' of a conv output is applied by the LAST data-gradient call that writes its gradient buffer
                             // (pws_dst.act_y) instead of by a separate pass over the buffer
    bool bn = false, deterministic = false;
};
// Weight gradient of a conv step.  A layer that stages 2 AND 3 run (down_bottom2..7, up_bottom7..1: the same modules, reference
// :178-214) comes by twice: its first weight gradient (stage 3, earlier in the reversed tape) is DEFERred and goes out WITH the second
// one as ONE launch over both operand pairs (pws_conv_bwd_weight_args.gout2: one prologue, one set of epilogue atomics -- 5-11 % less
// than two launches; the first pair's buffers stay untouched until then: a gradient buffer is final once its producer has been
// processed).  PWS_OPT_EXPERIMENT 89 and the kinds the ring kernels do not cover run the pair as two launches inside
// pws_conv2d_bwd_weight.  AFTER_PAIR: one pair's bias sum is already in, so there is no merged bias pass -- the deferred pair goes out
// by itself first.
enum { WG_NONE = 0, WG_ALONE, WG_DEFER, WG_MERGED, WG_AFTER_PAIR };
struct BwdDst {   // the gradient buffer of one source tensor of the op
    int prod = -1;             // tape position of the op that produced the tensor (tensors are identified by Seg::off, never by address)
    bool accumulate = false;   // an earlier step wrote the buffer (first consumer overwrites, later consumers accumulate)
    int act = PWS_ACT_NONE;    // the producer's act', fused into this call: the buffer then holds the gradient wrt the PRE-activation
};
struct BwdStep {
    int tape = 0, type = OP_CONV;
    bool runs = false;         // false: no upstream gradient reaches the op (a head without one, a conv nothing downstream asked of)
    int ndst = 0;              // (0 for the first layer: the window is data)
    BwdDst dst[4];
    bool out_preact = false;   // conv: the gradient of its output already is pre-activation -- the producer then needs the bias sum only,
    bool wgrad_bias = false;   //       which the weight-gradient kernel takes along (deterministic: an ordered pass of its own instead)
    int wgrad = WG_NONE, partner = -1;   // partner: tape position of the deferred pair (WG_MERGED, WG_AFTER_PAIR)
    int flush = -1;            // tape position of a deferred pair whose partner never came (its output got no gradient): this step is
                               // the layer's last, so the run that holds it launches the pair by itself, behind the run's steps
};
struct BwdPlan {
    std::vector<BwdStep> steps;   // index: reversed tape position
    int last_r[L_COUNT];          // reversed position of the last op that contributes to the layer's gradient (-1: none)
    // an nparts-run backward cuts the steps into runs of (almost) equal count: [begin(p), begin(p + 1))
    const BwdStep &at_tape(int ii) const { return steps[steps.size() - 1 - ii]; }
    size_t begin(int part, int nparts) const { return steps.size() * (size_t)part / nparts; }
    bool final_after(int layer, int part, int nparts) const { return last_r[layer] < 0 || (size_t)last_r[layer] < begin(part + 1, nparts); }
};

static BwdPlan plan_backward(const std::vector<Op> &tape, const LayerTable &L, const PlanMode &m) {
    const int T = (int)tape.size();
    BwdPlan P;
    P.steps.resize(T);
    std::fill(P.last_r, P.last_r + L_COUNT, -1);
    std::unordered_map<size_t, int> producer;   // Seg::off -> tape position
    int uses[L_COUNT] = {};
    for (int ii = 0; ii < T; ++ii)
        if (tape[ii].type == OP_CONV) producer[tape[ii].out.seg[0].off] = ii, ++uses[tape[ii].layer];
    // per tensor (by producer): a step has written its gradient buffer / the last step that writes it
    std::vector<char> written(T, 0), preact(T, 0);
    std::vector<int> last_writer(T, -1);
    bool have_dtheta[3] = {false, false, false};
    for (int r = 0; r < T; ++r) {
        const Op &op = tape[T - 1 - r];
        BwdStep &s = P.steps[r];
        s.tape = T - 1 - r, s.type = op.type;
        if (op.type == OP_FIELD) {
            P.last_r[L_OUT] = r;
            s.runs = m.grid[op.stage] || m.resid[op.stage];
            if (s.runs) have_dtheta[op.stage] = m.grid[op.stage];
        } else if (op.type == OP_THETA) {
            P.last_r[L_FLATTEN] = P.last_r[L_LINEAR] = r;
            s.runs = have_dtheta[op.stage];
        } else {
            P.last_r[op.layer] = r;
            s.runs = written[s.tape] != 0;
        }
        if (!s.runs || op.nchw) continue;
        s.ndst = op.type == OP_CONV ? op.in.nseg : 1;
        for (int i = 0; i < s.ndst; ++i) {
            const int p = producer.at(op.in.seg[i].off);
            s.dst[i].prod = p, s.dst[i].accumulate = written[p] != 0;
            written[p] = 1, last_writer[p] = r;
        }
    }
    // acts and weight gradients need every buffer's LAST writer, which the sweep above only knows at its end
    int pending[L_COUNT];   // reversed position of the layer's deferred step
    std::fill(pending, pending + L_COUNT, -1);
    for (int r = 0; r < T; ++r) {
        BwdStep &s = P.steps[r];
        if (!s.runs) continue;
        const Op &op = tape[s.tape];
        // (the theta head's (tiny) backward does not take the option; a conv without bf16 data-gradient weights runs an fp32 kernel)
        const bool can_fuse = m.fuse_act && op.type != OP_THETA && !(op.type == OP_CONV && L[op.layer].dgb_off == (size_t)-1);
        for (int i = 0; i < s.ndst; ++i) {
            const int p = s.dst[i].prod, pa = tape[p].act;
            if (can_fuse && last_writer[p] == r && (pa == PWS_ACT_LRELU || pa == PWS_ACT_RELU)) s.dst[i].act = pa, preact[p] = 1;
        }
        if (op.type != OP_CONV) continue;
        s.out_preact = preact[s.tape] != 0;
        s.wgrad_bias = !m.bn && s.out_preact && !m.deterministic;
        int &mine = pending[op.layer];
        if (m.bn || op.nchw || uses[op.layer] != 2) s.wgrad = WG_ALONE;
        else if (mine < 0) s.wgrad = WG_DEFER, mine = r;
        else {
            s.wgrad = P.steps[mine].wgrad_bias == s.wgrad_bias ? WG_MERGED : WG_AFTER_PAIR;
            s.partner = P.steps[mine].tape, mine = -1;
        }
    }
    for (int l = 0; l < L_COUNT; ++l)
        if (pending[l] >= 0) P.steps[P.last_r[l]].flush = P.steps[pending[l]].tape;
    return P;
}

// ---------------------------------------------------------------- the arena
// Where the backward's own buffers lie, behind the forward region: one gradient buffer per produced tensor (by tape position), then
// the scratch of the heads and of the bias-gradient reduction.  The Python host sizes its arena from this sequence of allocations.
struct BwdArena {
    std::vector<float *> g;
    float *gz_ws, *th_bwd_ws, *dtheta, *th_dx32, *abb_ws;
    size_t abb_bytes;
};
// Replays the training forward's allocation sequence on E (no launches: E recovers the tape and every activation's address), then
// allocates the backward's buffers.  (The training forward is always given a caller-owned thetas buffer: the replay must not reserve
// arena space for them either.)
static BwdArena lay_out_backward(Exec &E, const float *x, int n, int input_nc, int g, int ac) {
    const int S = 256;
    FwdArgs f{x, n, input_nc, g, 1, ac};
    f.caller_thetas = true;
    forward_graph(E, f);
    BwdArena A;
    A.g.assign(E.tape().size(), nullptr);
    for (size_t i = 0; i < E.tape().size(); ++i) {
        const Op &op = E.tape()[i];
        if (op.type == OP_CONV) A.g[i] = E.alloc((size_t)n * op.out.h * op.out.w * op.out.seg[0].c);
    }
    A.gz_ws = E.alloc((size_t)n * S * S * 2);
    A.th_bwd_ws = E.alloc((size_t)n * 8 * g);
    A.dtheta = E.alloc((size_t)3 * n * 6);
    A.th_dx32 = E.alloc((size_t)n * 16 * g);  // bf16 storage: fp32 gradient wrt x_s8 before it is folded into the bf16 buffer
    A.abb_bytes = pws_act_bwd_bias_ws_bytes(16 * g);  // slabs of the bias-gradient reduction (max cout <= 16 ngf)
    A.abb_ws = E.alloc(A.abb_bytes / sizeof(float));
    return A;
}
static size_t backward_arena_bytes(int n, int input_nc, int ngf, bool with_bn) {
    if (n <= 0 || !valid_shape(input_nc, ngf)) return 0;
    const LayerTable L = build_layers(input_nc, ngf);
    const BnCfg bn;
    Exec E(nullptr, L, n, Arena{}, nullptr, EXEC_SIZE, NetgOpts{PWS_MATH_FP32, PWS_STORE_FP32, false}, with_bn ? &bn : nullptr);   // the arena layout does not depend on the mode
    lay_out_backward(E, nullptr, n, input_nc, ngf, 0);
    return E.used();
}

// ---------------------------------------------------------------- the launcher
// One backward (or run `part` of an nparts-run backward: a data-parallel host all-reduces the weight gradients that are already final
// while the later runs still compute).  final_mask (nullable, one byte per layer): 1 once no op of a later run contributes to that
// layer's gradient.
struct BackwardArgs {
    const float *packed = nullptr, *packed_dgrad = nullptr, *x = nullptr;
    int n = 0, input_nc = 0, ngf = 0, ac = 0;
    Arena arena;
    const float *resid = nullptr, *thetas = nullptr;
    UpGrads up;
    float *dpacked = nullptr;
    hipStream_t st = nullptr;
    int part = 0, nparts = 1;
    unsigned char *final_mask = nullptr;
    const BnCfg *bn = nullptr;
    float *dbn = nullptr;
    NetgOpts opts;
};

class BwdLaunch {
  public:
    BwdLaunch(const BackwardArgs &a, const LayerTable &L, const Exec &E, const BwdArena &A) : a_(a), L_(L), E_(E), A_(A), st_(a.st), wst_(a.st) {
        // Weight gradients are leaves of the backward graph (only the optimizer reads them): they run on the side queue, each behind an
        // event recorded where its dy is final, while this queue goes on with the data-gradient chain -- whose deep levels are ~100
        // latency-bound launches that then sit beside chip-filling weight-gradient kernels instead of between them.  The queues join at
        // the end of the call.  (two_queues == 0: one queue.)
        if (a.opts.two_queues) {
            wside_ = &side_stream();
            if (hipStream_t q = wside_->pick(st_)) wst_ = q, wside_->begin(st_);
            else wside_ = nullptr;
        }
    }
    // the steps [r_begin, r_end) of the plan, then the deferred weight-gradient pairs those steps flush, then the join
    int run(const BwdPlan &P, size_t r_begin, size_t r_end) {
        int rc = PWS_OK;
        for (size_t r = r_begin; r < r_end && rc == PWS_OK; ++r) {
            const BwdStep &s = P.steps[r];
            if (!s.runs) continue;
            g_prof_tag = s.type == OP_CONV ? op(s).layer : -1;
            rc = s.type == OP_FIELD ? field(s) : s.type == OP_THETA ? theta(s) : conv(s, P);
            g_prof_tag = -1;
        }
        for (size_t r = r_begin; r < r_end && rc == PWS_OK; ++r) {
            if (P.steps[r].flush < 0) continue;
            const pws_conv_bwd_weight_args wa = weight_args(P.at_tape(P.steps[r].flush));
            rc = wgrad_fork();
            if (rc == PWS_OK) rc = pws_conv2d_bwd_weight(&wa, wst_);
        }
        if (wst_ != st_) {   // join: whatever follows on `st` (unpack, optimizer, the next part) sees every weight gradient
            hipEvent_t e = wside_->event();
            if (!e || hipEventRecord(e, wst_) != hipSuccess || hipStreamWaitEvent(st_, e, 0) != hipSuccess) {
                if (rc == PWS_OK) set_error("pws_netg_backward: joining the weight-gradient queue failed"), rc = PWS_EHIP;
            }
        }
        return rc;
    }

  private:
    const Op &op(const BwdStep &s) const { return E_.tape()[s.tape]; }
    const float *theta_k(const float *base, int k) const { return base + (size_t)k * a_.n * 6; }
    float *dtheta(int k) const { return A_.dtheta + (size_t)k * a_.n * 6; }
    // BatchNorm backward of `layer`: dy -> dz in place, dgamma / dbeta accumulated
    int bn_backward(int layer, float *dy, const float *y, const float *const *aux, int act, size_t pixels) {
        const int c = L_[layer].cout;
        float *dg = a_.dbn + E_.bn_off(layer);
        return pws_bn_train_bwd(dy, y, aux[0], aux[1], E_.gamma(layer), act, pixels, c, dg, dg + c, E_.bn_ws(0), E_.bn_ws_bytes(), st_);
    }
    int field(const BwdStep &s) {
        const Op &o = op(s);
        const int k = o.stage, n = a_.n, h = o.in.h, w = o.in.w;
        const float *gg = a_.up.grids[k], *gr = a_.up.resid[k], *resid = a_.resid + k * ((size_t)n * 256 * 256 * 2);
        const Seg &xs = o.in.seg[0];
        const BwdDst &d = s.dst[0];
        const Layer &l = L_[L_OUT];
        float *dth = gg ? dtheta(k) : nullptr;
        if (!a_.bn)
            return pws_field_head_bwd_act(xs.ptr, xs.ld, n, h, w, xs.c, a_.packed + l.w_off, resid, gg, gr, a_.ac, A_.g[d.prod], xs.c, d.accumulate,
                                          a_.dpacked + l.gw_off, a_.dpacked + l.gb_off, dth, A_.gz_ws, E_.store(), d.act, st_);
        int rc = field_bwd_gz(resid, gg, gr, n, h, w, a_.ac, A_.gz_ws, nullptr, dth, st_);
        if (rc == PWS_OK) rc = bn_backward(L_OUT, A_.gz_ws, nullptr, o.aux, PWS_ACT_NONE, (size_t)n * h * w);
        if (rc == PWS_OK)
            rc = field_bwd_dx_dw(xs.ptr, xs.ld, A_.gz_ws, n, h, w, xs.c, a_.packed + l.w_off, A_.g[d.prod], xs.c, d.accumulate, a_.dpacked + l.gw_off,
                                 E_.store(), st_);
        return rc;
    }
    int theta(const BwdStep &s) {
        const Op &o = op(s);
        const int k = o.stage, n = a_.n, acc = s.dst[0].accumulate;
        const Seg &xs = o.in.seg[0];
        float *gx = A_.g[s.dst[0].prod], *dp = a_.dpacked;
        const Layer &f = L_[L_FLATTEN], &l = L_[L_LINEAR];
        const float *wf = a_.packed + f.w_off, *wl = a_.packed + l.w_off;
        if (a_.bn) {
            float *dz2 = dtheta(k);   // overwritten by the BatchNorm backward
            int rc = bn_backward(L_LINEAR, dz2, theta_k(a_.thetas, k), o.aux + 2, PWS_ACT_LRELU, (size_t)n);
            if (rc == PWS_OK) rc = theta_bwd_bn_lin(dz2, E_.h_saved(k), n, f.cout, wl, dp + l.gw_off, A_.th_bwd_ws, st_);
            if (rc == PWS_OK) rc = bn_backward(L_FLATTEN, A_.th_bwd_ws, E_.h_saved(k), o.aux, PWS_ACT_LRELU, (size_t)n);
            if (rc == PWS_OK) rc = theta_bwd_flat(xs.ptr, n, xs.c, f.cout, wf, A_.th_bwd_ws, dp + f.gw_off, gx, acc, st_);
            return rc;
        }
        if (!E_.io16())
            return pws_theta_head_bwd(xs.ptr, n, xs.c, f.cout, wf, wl, E_.h_saved(k), theta_k(a_.thetas, k), dtheta(k), dp + f.gw_off, dp + f.gb_off,
                                      dp + l.gw_off, dp + l.gb_off, gx, acc, A_.th_bwd_ws, st_);
        // fp32 head on an fp32 copy of its bf16 input; its input gradient goes through an fp32 scratch
        const size_t cnt = (size_t)n * 4 * xs.c;
        int rc = pws_cvt_bf16_to_f32(xs.ptr, E_.theta_x32(0), cnt, st_);
        if (rc == PWS_OK)
            rc = pws_theta_head_bwd(E_.theta_x32(0), n, xs.c, f.cout, wf, wl, E_.h_saved(k), theta_k(a_.thetas, k), dtheta(k), dp + f.gw_off,
                                    dp + f.gb_off, dp + l.gw_off, dp + l.gb_off, A_.th_dx32, 0, A_.th_bwd_ws, st_);
        if (rc == PWS_OK) rc = pws_cvt_f32_to_bf16(A_.th_dx32, gx, cnt, acc, st_);
        return rc;
    }
    // the weight-gradient call of a conv step (its own operand pair)
    pws_conv_bwd_weight_args weight_args(const BwdStep &s) const {
        const Op &o = op(s);
        const Layer &l = L_[o.layer];
        pws_conv_bwd_weight_args wa{};
        wa.kind = l.kind, wa.n = a_.n, wa.h = o.in.h, wa.w = o.in.w, wa.nsrc = o.in.nseg, wa.src_nchw = o.nchw ? 1 : 0;
        for (int i = 0; i < o.in.nseg; ++i) wa.src[i] = pws_src{o.in.seg[i].ptr, o.in.seg[i].c, o.in.seg[i].ld};
        if (o.nchw) wa.src[0] = pws_src{a_.x, a_.input_nc, 0};
        if (o.nchw && a_.opts.math == PWS_MATH_BF16 && l.wb_off != (size_t)-1 && E_.x_nhwc() && a_.input_nc <= 32)
            wa.src_nchw = 0, wa.src[0] = pws_src{E_.x_nhwc(), 32, 32};  // the forward's NHWC copy
        wa.cout = l.cout, wa.gout = A_.g[s.tape], wa.gout_ld = l.cout, wa.dw_packed = a_.dpacked + l.gw_off;
        wa.math = a_.opts.math, wa.store = E_.store();
        wa.dbias = s.wgrad_bias ? a_.dpacked + l.gb_off : nullptr;
        return wa;
    }
    int wgrad_fork() {   // the side queue waits for everything issued on `st` so far
        if (wst_ == st_) return PWS_OK;
        hipEvent_t e = wside_->event();
        if (!e || hipEventRecord(e, st_) != hipSuccess || hipStreamWaitEvent(wst_, e, 0) != hipSuccess) {
            set_error("pws_netg_backward: event record / wait on the weight-gradient queue failed");
            return PWS_EHIP;
        }
        return PWS_OK;
    }
    int conv(const BwdStep &s, const BwdPlan &P) {
        const Op &o = op(s);
        const Layer &l = L_[o.layer];
        float *go = A_.g[s.tape], *dbias = a_.dpacked + l.gb_off;
        const size_t pixels = (size_t)a_.n * o.out.h * o.out.w;
        int rc = PWS_OK;
        if (a_.bn)   // the conv bias gets no gradient: BatchNorm removes any per-channel constant (torch returns rounding noise)
            rc = bn_backward(o.layer, go, o.out.seg[0].ptr, o.aux, o.act, pixels);
        else if (!s.out_preact)   // (a pre-activation gradient needs the bias sum only: the weight-gradient kernel takes it along)
            rc = pws_act_bwd_bias_s(go, o.out.seg[0].ptr, pixels, l.cout, o.act, dbias, E_.store(), A_.abb_ws, A_.abb_bytes, st_);
        else if (a_.opts.deterministic)
            // the weight-gradient kernels' bias sums arrive per parity class / class pair in any order: an ordered pass instead
            // (act = NONE: sums only, slab partials + ordered reduction)
            rc = pws_act_bwd_bias_s(go, go, pixels, l.cout, PWS_ACT_NONE, dbias, E_.store(), A_.abb_ws, A_.abb_bytes, st_);
        if (rc == PWS_OK && s.wgrad != WG_DEFER) {
            pws_conv_bwd_weight_args wa = weight_args(s), first{};
            if (s.partner >= 0) first = weight_args(P.at_tape(s.partner));
            if (s.wgrad == WG_MERGED) {
                for (int i = 0; i < wa.nsrc; ++i) wa.src2_ptr[i] = first.src[i].ptr;
                wa.gout2 = first.gout;
            }
            rc = wgrad_fork();
            if (rc == PWS_OK && s.wgrad == WG_AFTER_PAIR) rc = pws_conv2d_bwd_weight(&first, wst_);
            if (rc == PWS_OK) rc = pws_conv2d_bwd_weight(&wa, wst_);
        }
        return rc == PWS_OK ? data_grad(s) : rc;
    }
    int data_grad(const BwdStep &s) {
        const Op &o = op(s);
        if (o.nchw) return PWS_OK;   // the window is data: no gradient wrt the first layer's input
        const Layer &l = L_[o.layer];
        pws_conv_bwd_data_args da{};
        da.kind = l.kind, da.n = a_.n, da.h = o.in.h, da.w = o.in.w, da.cout = l.cout, da.gout = A_.g[s.tape], da.gout_ld = l.cout;
        da.w_dgrad = a_.packed_dgrad + l.dg_off, da.ndst = s.ndst;
        for (int i = 0; i < s.ndst; ++i) {
            const Seg &sg = o.in.seg[i];
            const BwdDst &d = s.dst[i];
            da.dst[i] = pws_dst{A_.g[d.prod], sg.c, sg.c, d.accumulate, nullptr, 0, PWS_ACT_NONE, nullptr, 0};
            if (d.act != PWS_ACT_NONE)
                da.dst[i].act_y = sg.ptr, da.dst[i].act_y_ld = sg.ld, da.dst[i].act = d.act, da.dst[i].act_sign = sg.sign, da.dst[i].act_sign_ld = sg.c / 8;
        }
        da.ws = E_.splitk_ws(), da.ws_bytes = E_.splitk_bytes();
        if (a_.opts.math == PWS_MATH_BF16 && l.dgb_off != (size_t)-1) da.math = PWS_MATH_BF16, da.w_dgrad_bf16 = a_.packed_dgrad + l.dgb_off;
        da.store = E_.store();
        return pws_conv2d_bwd_data(&da, st_);
    }

    const BackwardArgs &a_;
    const LayerTable &L_;
    const Exec &E_;
    const BwdArena &A_;
    hipStream_t st_, wst_;
    SideStream *wside_ = nullptr;
};

static int zero_async(float *p, size_t floats, hipStream_t st) {
    const hipError_t e = hipMemsetAsync(p, 0, floats * sizeof(float), st);
    if (e != hipSuccess) {
        set_error("pws_netg_backward: hipMemsetAsync: %s", hipGetErrorString(e));
        return PWS_EHIP;
    }
    return PWS_OK;
}

static int run_backward(const BackwardArgs &a) {
    const LayerTable L = build_layers(a.input_nc, a.ngf);
    DeterministicScope det_scope(a.opts.deterministic);   // PWS_NETG_DETERMINISTIC: every accumulating launcher of this call
    Exec E(a.packed, L, a.n, a.arena, a.st, EXEC_REPLAY, a.opts, a.bn);
    const BwdArena A = lay_out_backward(E, a.x, a.n, a.input_nc, a.ngf, a.ac);
    if (E.rc() != PWS_OK) return E.rc();
    int rc = PWS_OK;
    if (a.part == 0 && a.bn && a.dbn) rc = zero_async(a.dbn, E.bn_total(), a.st);
    if (a.part == 0 && rc == PWS_OK) rc = zero_async(a.dpacked, L.grad, a.st);
    if (rc != PWS_OK) return rc;
    PlanMode m;
    for (int k = 0; k < 3; ++k) m.grid[k] = a.up.grids[k] != nullptr, m.resid[k] = a.up.resid[k] != nullptr;
    m.fuse_act = E.io16() && !a.bn && a.opts.math == PWS_MATH_BF16;
    m.bn = a.bn != nullptr, m.deterministic = a.opts.deterministic;
    const BwdPlan P = plan_backward(E.tape(), L, m);
    if (a.final_mask)
        for (int i = 0; i < L_COUNT; ++i) a.final_mask[i] = P.final_after(i, a.part, a.nparts);
    return BwdLaunch(a, L, E, A).run(P, P.begin(a.part, a.nparts), P.begin(a.part + 1, a.nparts));
}

static int backward_entry(BackwardArgs &a, void *ws, const pws_netg_opts *opts, pws_stream_t stream) {
    PWS_REQUIRE(a.n >= 0, "pws_netg_backward: bad n %d", a.n);
    PWS_REQUIRE_SHAPE("pws_netg_backward", a.input_nc, a.ngf);
    PWS_REQUIRE(a.nparts >= 1 && a.part >= 0 && a.part < a.nparts, "pws_netg_backward: part %d of %d", a.part, a.nparts);
    if (int rc = opts_from(opts, &a.opts)) return rc;
    PWS_REQUIRE(a.opts.x_sample_stride == 0, "pws_netg_backward: x_sample_stride is an option of the inference forward (the backward reads a dense window)");
    if (a.n == 0) {
        if (a.final_mask)
            for (int i = 0; i < L_COUNT; ++i) a.final_mask[i] = 1;
        return PWS_OK;
    }
    PWS_REQUIRE(a.packed && a.packed_dgrad && a.x && ws && a.resid && a.thetas && a.dpacked, "pws_netg_backward: NULL pointer");
    PWS_REQUIRE(a.up.any(), "pws_netg_backward: no output gradient given");
    PWS_REQUIRE((reinterpret_cast<size_t>(ws) & 255) == 0, "pws_netg_backward: workspace must be 256-byte aligned");
    a.arena.ws = static_cast<char *>(ws), a.st = as_stream(stream);
    return run_backward(a);
}

}  // namespace pws

using namespace pws;

extern "C" size_t pws_netg_train_workspace_bytes(int n, int input_nc, int ngf) { return backward_arena_bytes(n, input_nc, ngf, false); }
extern "C" size_t pws_netg_train_workspace_bytes_bn(int n, int input_nc, int ngf) { return backward_arena_bytes(n, input_nc, ngf, true); }

// HOST only (no GPU call): the run of an nparts-run backward after which layer i's gradient is final (BwdPlan::final_after, the rule
// behind the backward's final_mask).
extern "C" int pws_netg_backward_plan(int input_nc, int ngf, int nparts, unsigned char *final_part) {
    PWS_REQUIRE_SHAPE("pws_netg_backward_plan", input_nc, ngf);
    PWS_REQUIRE(nparts >= 1 && nparts <= 255 && final_part, "pws_netg_backward_plan: nparts %d (1..255) / NULL pointer", nparts);
    const LayerTable L = build_layers(input_nc, ngf);
    Exec E(nullptr, L, 1, Arena{}, nullptr, EXEC_SIZE, NetgOpts{PWS_MATH_FP32, PWS_STORE_FP32, false});
    lay_out_backward(E, nullptr, 1, input_nc, ngf, 0);
    const BwdPlan P = plan_backward(E.tape(), L, PlanMode{});
    for (int i = 0; i < L_COUNT; ++i) {
        int part = 0;
        while (part < nparts - 1 && !P.final_after(i, part, nparts)) ++part;
        final_part[i] = (unsigned char)part;
    }
    return PWS_OK;
}

extern "C" int pws_netg_backward_lists(const float *packed, const float *packed_dgrad, const float *x, int n, int input_nc, int ngf,
                                       int align_corners, void *ws, size_t ws_bytes, const float *resid, const float *thetas,
                                       const float *const *g_grids, const float *const *g_resid, float *dpacked, int part, int nparts,
                                       unsigned char *final_mask, const pws_netg_opts *opts, pws_stream_t stream) {
    BackwardArgs a{packed, packed_dgrad, x, n, input_nc, ngf, align_corners, Arena{nullptr, ws_bytes}, resid, thetas, UpGrads(g_grids, g_resid),
                   dpacked, nullptr, part, nparts, final_mask};
    return backward_entry(a, ws, opts, stream);
}

extern "C" int pws_netg_backward_opts(const float *packed, const float *packed_dgrad, const float *x, int n, int input_nc, int ngf,
                                      int align_corners, void *ws, size_t ws_bytes, const float *resid, const float *thetas,
                                      const float *g_grids, const float *g_resid, float *dpacked, int part, int nparts,
                                      unsigned char *final_mask, const pws_netg_opts *opts, pws_stream_t stream) {
    BackwardArgs a{packed, packed_dgrad, x, n, input_nc, ngf, align_corners, Arena{nullptr, ws_bytes}, resid, thetas,
                   UpGrads(g_grids, g_resid, (size_t)(n > 0 ? n : 0) * 256 * 256 * 2), dpacked, nullptr, part, nparts, final_mask};
    return backward_entry(a, ws, opts, stream);
}

extern "C" int pws_netg_backward_part(const float *packed, const float *packed_dgrad, const float *x, int n, int input_nc, int ngf,
                                      int align_corners, void *ws, size_t ws_bytes, const float *resid, const float *thetas,
                                      const float *g_grids, const float *g_resid, float *dpacked, int part, int nparts,
                                      unsigned char *final_mask, pws_stream_t stream) {
    return pws_netg_backward_opts(packed, packed_dgrad, x, n, input_nc, ngf, align_corners, ws, ws_bytes, resid, thetas, g_grids, g_resid,
                                  dpacked, part, nparts, final_mask, nullptr, stream);
}

extern "C" int pws_netg_backward(const float *packed, const float *packed_dgrad, const float *x, int n, int input_nc, int ngf,
                                 int align_corners, void *ws, size_t ws_bytes, const float *resid, const float *thetas,
                                 const float *g_grids, const float *g_resid, float *dpacked, pws_stream_t stream) {
    return pws_netg_backward_opts(packed, packed_dgrad, x, n, input_nc, ngf, align_corners, ws, ws_bytes, resid, thetas, g_grids, g_resid,
                                  dpacked, 0, 1, nullptr, nullptr, stream);
}

// ---- use_BN=True training (BatchNorm2d after every conv, batch statistics): fp32 storage only
extern "C" int pws_netg_backward_bn_opts(const float *packed, const float *packed_dgrad, const float *bn_params, float eps, const float *x,
                                         int n, int input_nc, int ngf, int align_corners, void *ws, size_t ws_bytes, const float *resid,
                                         const float *thetas, const float *g_grids, const float *g_resid, float *dpacked, float *dbn,
                                         const pws_netg_opts *opts, pws_stream_t stream) {
    PWS_REQUIRE(n >= 2, "pws_netg_backward_bn: bad n %d", n);
    PWS_REQUIRE_SHAPE("pws_netg_backward_bn", input_nc, ngf);
    PWS_REQUIRE(packed && packed_dgrad && bn_params && x && ws && resid && thetas && dpacked && dbn, "pws_netg_backward_bn: NULL pointer");
    PWS_REQUIRE(g_grids || g_resid, "pws_netg_backward_bn: no output gradient given");
    PWS_REQUIRE((reinterpret_cast<size_t>(ws) & 255) == 0, "pws_netg_backward_bn: workspace must be 256-byte aligned");
    BnCfg bn;
    bn.params = bn_params, bn.eps = eps;
    BackwardArgs a{packed, packed_dgrad, x, n, input_nc, ngf, align_corners, Arena{static_cast<char *>(ws), ws_bytes}, resid, thetas,
                   UpGrads(g_grids, g_resid, (size_t)n * 256 * 256 * 2), dpacked, as_stream(stream), 0, 1, nullptr, &bn, dbn};
    if (int rc = bn_opts_from(opts, &a.opts)) return rc;
    return run_backward(a);
}

extern "C" int pws_netg_backward_bn(const float *packed, const float *packed_dgrad, const float *bn_params, float eps, const float *x,
                                    int n, int input_nc, int ngf, int align_corners, void *ws, size_t ws_bytes, const float *resid,
                                    const float *thetas, const float *g_grids, const float *g_resid, float *dpacked, float *dbn,
                                    pws_stream_t stream) {
    return pws_netg_backward_bn_opts(packed, packed_dgrad, bn_params, eps, x, n, input_nc, ngf, align_corners, ws, ws_bytes, resid, thetas, g_grids,
                                     g_resid, dpacked, dbn, nullptr, stream);
}
