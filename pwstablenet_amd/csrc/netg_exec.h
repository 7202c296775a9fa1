// Host-side executor of the cascading generator (netg_forward.cpp, netg_backward.cpp; layer table: netg_layers.h): sequences the HIP kernels of this library on one stream,
// with all activations in a caller-provided arena.  Mirrors UnetGenerator.forward of the reference
// (lib/networks_cascading.py:152-237) -- variable names below are the reference's -- and its autograd backward
// (loss_g.backward(), main_new.py:214).
//
// Differences in HOW (not in WHAT):
//   * activations are NHWC; a torch.cat([a, b], 1) is a list of (pointer, channels, stride) sources consumed
//     directly by the next convolution -- the reference's 43-44 concat copies per forward disappear;
//   * stage 3's first block (`x32 = down_bottom1(None, x11)`, reference :200) has the same weights and the same
//     input as stage 2's (`x22`, :178) and is bit-identical, so it is computed once (its gradient is the sum of
//     both uses, which falls out of x22 having one gradient buffer);
//   * `out` conv + tanh + tanh + permute + affine_grid + add run as one kernel (field head).
// Backward replays the forward's allocation sequence (no launches) to recover every activation's address in the
// arena, plans the recorded ops in reverse (netg_backward.cpp: plan_backward) and launches the plan: per layer act'/bias-grad,
// weight grad, data grad into the gradient buffers of the layer's sources (first consumer overwrites, later consumers
// accumulate -- no zero-fill pass).
// No allocation, no synchronisation: every launch is ordered after the caller's `stream`; the forward forks an internal
// second queue by events (stage k+1's encoder beside stage k's decoder) and joins it back before returning.
#pragma once
#include <cstdio>
#include <cstdlib>
#include <mutex>
#include <unordered_map>
#include <vector>

#include "netg_layers.h"

namespace pws {

// Mode of one forward / backward: carried by value from the entry point's arguments (pws_netg_opts) -- the executor reads no
// process-wide option, so two generators with different arithmetic can run from two host threads.
struct NetgOpts {
    int math, store;
    bool two_queues;
    bool deterministic = false;     // PWS_NETG_DETERMINISTIC
    size_t x_sample_stride = 0;     // floats between samples of the window (0 = dense)
    bool prune_dead = false;        // PWS_NETG_PRUNE_DEAD
};
inline NetgOpts opts_defaults() { return NetgOpts{g_math, g_store, g_two_queues}; }
inline int opts_from(const pws_netg_opts *o, NetgOpts *out) {
    if (!o) {
        *out = opts_defaults();
        return PWS_OK;
    }
    PWS_REQUIRE(o->math == PWS_MATH_FP32 || o->math == PWS_MATH_BF16, "pws_netg_opts: math %d", o->math);
    PWS_REQUIRE(o->store == PWS_STORE_FP32 || o->store == PWS_STORE_BF16, "pws_netg_opts: store %d", o->store);
    PWS_REQUIRE(o->store == PWS_STORE_FP32 || o->math == PWS_MATH_BF16, "pws_netg_opts: PWS_STORE_BF16 needs PWS_MATH_BF16");
    PWS_REQUIRE(o->two_queues >= -1 && o->two_queues <= 1 && (o->flags & ~(PWS_NETG_DETERMINISTIC | PWS_NETG_PRUNE_DEAD)) == 0, "pws_netg_opts: two_queues %d / flags %d",
                o->two_queues, o->flags);
    *out = NetgOpts{o->math, o->store, o->two_queues < 0 ? g_two_queues : o->two_queues != 0, (o->flags & PWS_NETG_DETERMINISTIC) != 0,
                    o->x_sample_stride, (o->flags & PWS_NETG_PRUNE_DEAD) != 0};
    return PWS_OK;
}

// mode of the BatchNorm training path: fp32 storage always (the BatchNorm kernels are fp32); the conv contractions in fp32 or on the
// bf16 matrix cores (operands rounded while they are staged, fp32 accumulation), as pws_netg_opts.math says
inline int bn_opts_from(const pws_netg_opts *opts, NetgOpts *o) {
    *o = NetgOpts{PWS_MATH_FP32, PWS_STORE_FP32, g_two_queues};
    if (!opts) return PWS_OK;
    NetgOpts u;
    if (int rc = opts_from(opts, &u)) return rc;
    PWS_REQUIRE(u.store == PWS_STORE_FP32 && u.x_sample_stride == 0,
                "pws_netg_*_bn_opts: the BatchNorm training path stores fp32 activations (store must be PWS_STORE_FP32) and reads a dense window");
    o->math = u.math, o->two_queues = u.two_queues, o->deterministic = u.deterministic;
    return PWS_OK;
}

constexpr size_t kNoTensor = (size_t)-1;
struct Seg {
    float *ptr;
    int c, ld;
    unsigned char *sign = nullptr;   // bf16 training: the tensor's sign bits (pws_conv_args.out_sign), c / 8 bytes per pixel; NULL = none
    size_t off = kNoTensor;          // the tensor's byte offset in the arena: its identity where there is no arena (a sizing or planning run)
};
struct Tn {  // a (virtually concatenated) NHWC tensor
    Seg seg[4];
    int nseg, h, w;
};

enum { OP_CONV = 0, OP_THETA = 1, OP_FIELD = 2 };
struct Op {
    int type, layer, act, stage;
    bool nchw;
    Tn in, out;
    // use_BN training: pre-normalisation values and saved (mean, invstd) of the BatchNorms of this op
    //   conv : aux[0] = z, aux[1] = stats          field: aux[0] = z, aux[1] = stats, aux[2] = BatchNorm output
    //   theta: aux[0] = z1, aux[1] = stats1, aux[2] = z2, aux[3] = stats2
    float *aux[4] = {nullptr, nullptr, nullptr, nullptr};
};

// Training-mode BatchNorm configuration of one forward / backward (use_BN=True, reference lib/networks_cascading.py:253-341).
// params / running: flat buffers, per layer in state-dict order [gamma(cout) | beta(cout)] resp. [running_mean | running_var].
struct BnCfg {
    const float *params = nullptr;
    float *running = nullptr;
    float momentum = 0.1f, eps = 1e-5f;
};

// Second in-order queue for the branch of the forward that does not depend on the current one (stage k+1's encoder
// runs beside stage k's decoder), plus the events that fork / join it.  Created lazily once per process (the only
// runtime objects this library owns); ordering against the caller's stream is by events only, never by a sync.
// The side QUEUE is one per device and process: the runtime deals streams to a few hardware queues round-robin, and a second side
// stream made late in a process with several streams alive (the backward's, on autograd's thread, in bench.py after its streaming
// leg) landed on the caller's hardware queue -- the two then serialise, barrier packets on top (configs[2] step 32.3 ms instead of
// 30.1; tools/_bin-style probe: 5 extra torch streams reproduce it).  So every host thread shares the stream made first; what a
// thread owns is its EVENT POOL (and a private side stream for calls made inside a graph capture: SideStream::pick).
inline hipStream_t shared_side_queue(int dev) {
    static std::mutex m;
    static std::unordered_map<int, hipStream_t> per_device;
    std::lock_guard<std::mutex> lock(m);
    auto it = per_device.find(dev);
    if (it != per_device.end()) return it->second;
    hipStream_t s = nullptr;
    if (hipStreamCreateWithFlags(&s, hipStreamNonBlocking) != hipSuccess) s = nullptr;
    per_device[dev] = s;
    return s;
}
struct SideStream {
    hipStream_t stream = nullptr;    // the device's shared side queue (eager calls)
    hipStream_t own = nullptr;       // this thread's private side stream: calls made inside a graph capture fork into it
    // Event pools, one per CALLER STREAM: a call re-records the pool's events from the first one on.  Waits made by an earlier call may
    // still be queued then -- harmless while the new record lands on the same queues as the old one (it is later in their order: the
    // queued wait can only become stricter).  With ONE pool per thread, a second call on ANOTHER stream re-recorded events that waits
    // of the first call had not consumed yet: autograd runs the backwards of all host threads on one worker thread per device, so two
    // training threads shared a pool, a weight-gradient launch of one waited for the other's stream and read its dy early (gradients
    // off by 1e-4..1e-1 of their size in 1 run of 10 of tests/test_hip_threads.py, tools/probes/thread_grad_probe.py, round 4).
    struct Pool {
        std::vector<hipEvent_t> events;
        size_t next = 0;
    };
    std::unordered_map<hipStream_t, Pool> pools;
    Pool *cur = nullptr;
    int dev = 0;
    void begin(hipStream_t st) { cur = &pools[st], cur->next = 0; }   // (references into an unordered_map survive a rehash)
    // The side queue to fork into beside `st`, or nullptr (run on one queue).  A call that is being CAPTURED never touches the shared
    // queue: forking joins the side stream to the caller's capture, and two host threads capturing at once would pull one stream into
    // two captures (both invalid) -- a captured call forks into the thread's own stream instead (a graph has no hardware queue of its
    // own to collide with: its nodes are scheduled when it is launched).  An eager call takes the shared queue, which therefore is never
    // part of anybody's capture; the capture status of `st` is the calling thread's own business, so nothing here is check-then-use
    // against another thread.
    hipStream_t pick(hipStream_t st) {
        hipStreamCaptureStatus cm = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing(st, &cm) != hipSuccess) return nullptr;
        if (cm == hipStreamCaptureStatusNone) {
            if (!stream) stream = shared_side_queue(dev);
            // the private stream is made HERE, on the thread's first eager call: creating a stream while a capture is open is one of
            // the calls a capture may not survive (a host captures after an eager warm-up on the same thread)
            if (!own && hipStreamCreateWithFlags(&own, hipStreamNonBlocking) != hipSuccess) own = nullptr;
            return stream;
        }
        if (cm != hipStreamCaptureStatusActive) return nullptr;
        return own;   // nullptr (one queue) when this thread never made an eager call
    }
    hipEvent_t event() {
        if (!cur) return nullptr;
        if (cur->next == cur->events.size()) {
            hipEvent_t e = nullptr;
            if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) return nullptr;
            cur->events.push_back(e);
        }
        return cur->events[cur->next++];
    }
};
// one event pool per host thread AND device
inline SideStream &side_stream() {
    static thread_local std::unordered_map<int, SideStream> per_device;
    int dev = 0;
    (void)hipGetDevice(&dev);
    SideStream &s = per_device[dev];
    s.dev = dev;
    return s;
}

struct Arena {
    char *ws = nullptr;
    size_t bytes = 0;
};
// EXEC_SIZE: no arena -- sizes, offsets and the tape only; EXEC_REPLAY: every address, no launch (the backward); EXEC_RUN: the forward;
// EXEC_PLAN: like EXEC_REPLAY over a stand-in arena, and every conv asks the dispatch ladder what it would launch (pws_netg_forward_plan)
enum ExecMode { EXEC_SIZE, EXEC_REPLAY, EXEC_RUN, EXEC_PLAN };
// the stand-in base of arena, weights and window in EXEC_PLAN: non-null and 256-byte aligned, as the real entry points require -- never dereferenced
inline char *plan_base(int which) { return reinterpret_cast<char *>((size_t)(which + 1) << 40); }   // 0 arena, 1 weights, 2 window

class Exec {
  public:
    Exec(const float *packed, const LayerTable &layers, int n, Arena arena, hipStream_t st, ExecMode mode, const NetgOpts &o, const BnCfg *bn = nullptr)
        : math_(o.math), x_sstride_(o.x_sample_stride), prune_dead_(o.prune_dead), packed_(packed), L_(layers), n_(n), ws_(arena.ws), cap_(arena.bytes),
          dry_(mode == EXEC_SIZE), launch_(mode == EXEC_RUN), plan_(mode == EXEC_PLAN) {
        if (bn) {
            bn_on_ = true, bn_ = *bn;
            size_t off = 0;
            for (int i = 0; i < L_COUNT; ++i) bn_off_[i] = off, off += 2 * (size_t)layers[i].cout;
            bn_total_ = off;
        }
        // bf16 storage of activations: only with bf16 math and when every conv layer is covered by the bf16 kernels
        io16_ = o.math == PWS_MATH_BF16 && o.store == PWS_STORE_BF16 && layers[L_DOWN1].cin % 32 == 0;
        streams_[0] = st, streams_[1] = st;
        if (launch_ && o.two_queues) {
            side_ = &side_stream();
            if (hipStream_t q = side_->pick(st)) streams_[1] = q, side_->begin(st);
        }
    }

    // ---- two-queue scheduling: ops go to queue `q`; fork/join are event record + wait (capturable, no host sync)
    void use(int q) { q_ = q; }
    bool two_queues() const { return streams_[1] != streams_[0]; }
    // mark(): "everything issued so far on queue `from`"; wait(): later work on queue `to` starts after that point
    hipEvent_t mark(int from) {
        if (!launch_ || !two_queues()) return nullptr;
        hipEvent_t e = side_->event();
        if (!e || hipEventRecord(e, streams_[from]) != hipSuccess) {
            if (rc_ == PWS_OK) set_error("pws_netg_forward: hipEventRecord failed"), rc_ = PWS_EHIP;
            return nullptr;
        }
        return e;
    }
    void wait(int to, hipEvent_t e) {
        if (!e) return;
        if (hipStreamWaitEvent(streams_[to], e, 0) != hipSuccess && rc_ == PWS_OK)
            set_error("pws_netg_forward: hipStreamWaitEvent failed"), rc_ = PWS_EHIP;
    }
    void order(int from, int to) { wait(to, mark(from)); }

    size_t used() const { return off_; }
    int rc() const { return rc_; }
    const std::vector<Op> &tape() const { return tape_; }
    void plan_for(int compute_units) { plan_cus_ = compute_units; }
    const std::vector<ConvChoice> &plan() const { return plan_out_; }
    float *splitk_ws() const { return splitk_ws_; }
    float *x_nhwc() const { return x_nhwc_; }
    bool io16() const { return io16_; }
    bool prune_dead() const { return prune_dead_; }
    int math() const { return math_; }
    int store() const { return io16_ ? PWS_STORE_BF16 : PWS_STORE_FP32; }
    float *theta_x32(int q) const { return theta_x32_[q]; }
    size_t splitk_bytes() const { return splitk_bytes_; }
    float *h_saved(int stage) const { return h_saved_[stage]; }
    bool bn_on() const { return bn_on_; }
    size_t bn_off(int layer) const { return bn_off_[layer]; }
    size_t bn_total() const { return bn_total_; }
    float *bn_ws(int q) const { return bn_ws_[q]; }
    size_t bn_ws_bytes() const { return bn_ws_bytes_; }
    const float *gamma(int layer) const { return bn_.params + bn_off_[layer]; }
    const float *beta(int layer) const { return bn_.params + bn_off_[layer] + L_[layer].cout; }
    // y = act(BatchNorm_train(z)) of `layer` on the current queue; stats saved, running statistics updated `repeat` times
    int bn_forward(int layer, const float *z, size_t pixels, int act, float *y, float *stats, int repeat) {
        const int c = L_[layer].cout;
        float *rm = bn_.running ? bn_.running + bn_off_[layer] : nullptr;
        return pws_bn_train_fwd(z, pixels, c, gamma(layer), beta(layer), act, y, stats, rm, rm ? rm + c : nullptr, bn_.momentum, bn_.eps,
                                repeat, bn_ws_[q_], bn_ws_bytes_, streams_[q_]);
    }

    float *alloc(size_t floats, size_t *at_out = nullptr) {
        const size_t bytes = align_up(floats * sizeof(float), 256);
        const size_t at = off_;
        off_ += bytes;
        if (at_out) *at_out = at;
        if (dry_) return nullptr;
        if (off_ > cap_) {
            if (rc_ == PWS_OK) {
                set_error("pws_netg: workspace too small (%zu B needed so far, %zu B given)", off_, cap_);
                rc_ = PWS_ENOMEM;
            }
            return nullptr;
        }
        return reinterpret_cast<float *>(ws_ + at);
    }

    static Tn cat(const Tn &a, const Tn &b) {  // torch.cat([a, b], dim=1)
        Tn o = a;
        for (int i = 0; i < b.nseg && o.nseg < 4; ++i) o.seg[o.nseg++] = b.seg[i];
        return o;
    }

    static void out_extent(int kind, const Tn &x, int *oh, int *ow) {
        *oh = x.h, *ow = x.w;
        if (kind == PWS_CONV_K3S2) *oh = (x.h - 1) / 2 + 1, *ow = (x.w - 1) / 2 + 1;
        if (kind == PWS_CONVT_K4S2) *oh = 2 * x.h, *ow = 2 * x.w;
    }
    Tn conv(int layer, const Tn &x, int act, const float *nchw_src = nullptr, int nchw_c = 0) {
        const Layer &l = L_[layer];
        int oh, ow;
        out_extent(l.kind, x, &oh, &ow);
        Tn o{};
        o.nseg = 1, o.h = oh, o.w = ow;
        o.seg[0] = Seg{nullptr, l.cout, l.cout};
        o.seg[0].ptr = alloc((size_t)n_ * oh * ow * l.cout, &o.seg[0].off);
        // bf16 training: the layers whose backward multiplies by act'(this output) read its SIGN BITS instead of the tensor (1/16 of the
        // bytes: the data-gradient epilogues of the large maps are read-modify-writes waiting on their loads).  Asked of the maps the
        // ring kernel takes and the first layer (they write them in their epilogues; the one-shot kernel and split-K launches are followed
        // by a pass over the output) -- PWS_OPT_EXPERIMENT 12: never.
        // (The arena holds the bytes in every training layout -- the workspace size does not depend on the storage mode.)
        if (wants_sign(act, l.cout, ow)) {
            unsigned char *sg = reinterpret_cast<unsigned char *>(alloc(((size_t)n_ * oh * ow * (l.cout / 8) + 3) / 4));
            if (io16_ && !exp_is(EXP_NO_SIGN_BITS)) o.seg[0].sign = sg;
        }
        return run_conv(layer, x, act, o, 1, nchw_src, nchw_c);
    }
    bool wants_sign(int act, int cout, int ow) const { return training_ && !bn_on_ && act != PWS_ACT_NONE && cout % 8 == 0 && ow >= 32; }

    // ---- stages 2 and 3 in LOCKSTEP (round 4).  They run the same modules (reference :178-214) on different inputs, and every input of
    // stage 3 at a level is an output of stage 2 at that level's predecessor -- so with the three stages' tensors of a level laid out as
    // sample GROUPS of one buffer [stage 1 | stage 2 | stage 3] (each n samples), "what stages 2 and 3 read" are the two batch-2n views
    // groups (0, 1) and groups (1, 2) of it, and ONE launch of batch 2n computes both stages' outputs into groups (1, 2) of the next
    // buffer.  23 of the 68 launches of an inference forward go; what is left of the deep levels runs on twice the pixels per launch.
    // The tape still holds one op per stage (the backward is per stage, as before).
    struct Groups {   // a [groups][n][h][w][c] buffer
        float *ptr = nullptr;
        unsigned char *sign = nullptr;
        int c = 0, h = 0, w = 0;
        size_t off = 0;   // byte offset of `ptr` in the arena
    };
    size_t esz() const { return io16_ ? 2 : 4; }
    Groups alloc_groups(int ngroups, int h, int w, int c, int act) {
        Groups t;
        t.c = c, t.h = h, t.w = w;
        t.ptr = alloc((size_t)ngroups * n_ * h * w * c, &t.off);
        if (wants_sign(act, c, w)) {
            unsigned char *sg = reinterpret_cast<unsigned char *>(alloc(((size_t)ngroups * n_ * h * w * (c / 8) + 3) / 4));
            if (io16_ && !exp_is(EXP_NO_SIGN_BITS)) t.sign = sg;
        }
        return t;
    }
    Tn group(const Groups &t, int g0) const {   // group g0 (read as batch 2n: groups g0 and g0 + 1)
        Tn o{};
        o.nseg = 1, o.h = t.h, o.w = t.w;
        const size_t shift = (size_t)g0 * n_ * t.h * t.w * t.c * esz();
        float *p = t.ptr ? reinterpret_cast<float *>(reinterpret_cast<char *>(t.ptr) + shift) : nullptr;
        o.seg[0] = Seg{p, t.c, t.c, t.sign ? t.sign + (size_t)g0 * n_ * t.h * t.w * (t.c / 8) : nullptr, t.off + shift};
        return o;
    }
    Tn shifted(const Tn &x, int k) const {   // the same (virtually concatenated) tensor k groups further
        Tn o = x;
        for (int i = 0; i < o.nseg; ++i) {
            Seg &sg = o.seg[i];
            const size_t shift = (size_t)k * n_ * x.h * x.w * sg.ld * esz();
            if (sg.ptr) sg.ptr = reinterpret_cast<float *>(reinterpret_cast<char *>(sg.ptr) + shift);
            if (sg.off != kNoTensor) sg.off += shift;
            if (sg.sign) sg.sign += (size_t)k * n_ * x.h * x.w * (sg.c / 8);
        }
        return o;
    }
    // layer on `ngroups` consecutive groups of x (batch ngroups * n) into group g0.. of dst; returns group g0's output
    Tn conv_groups(int layer, const Tn &x, int act, int ngroups, const Groups &dst, int g0) {
        return run_conv(layer, x, act, group(dst, g0), ngroups, nullptr, 0);
    }

    Tn run_conv(int layer, const Tn &x, int act, const Tn &o, int ngroups, const float *nchw_src, int nchw_c) {
        const Layer &l = L_[layer];
        const int oh = o.h, ow = o.w;
        Op op{OP_CONV, layer, act, 0, nchw_c > 0, x, o};
        if (bn_on_) op.aux[0] = alloc((size_t)n_ * oh * ow * l.cout), op.aux[1] = alloc(2 * (size_t)l.cout);
        tape_.push_back(op);
        for (int k = 1; k < ngroups; ++k) tape_.push_back(Op{OP_CONV, layer, act, 0, false, shifted(x, k), shifted(o, k)});
        if (!(launch_ || plan_) || rc_ != PWS_OK) return o;
        pws_conv_args a{};
        a.kind = l.kind, a.n = ngroups * n_, a.h = x.h, a.w = x.w;
        if (nchw_c > 0 && math_ == PWS_MATH_BF16 && l.wb_off != (size_t)-1 && x_nhwc_ && nchw_c <= 32) {
            // bf16 first layer: the NCHW window is re-laid once as a 32-channel NHWC source (kept for the weight gradient)
            if (launch_) rc_ = nchw_to_nhwc_pad_strided(nchw_src, x_sstride_, x_nhwc_, n_, nchw_c, x.h, x.w, 32, store(), streams_[q_]);
            if (rc_ != PWS_OK) return o;
            a.nsrc = 1, a.src[0] = pws_src{x_nhwc_, 32, 32};
        } else if (nchw_c > 0) {
            a.nsrc = 1, a.src_nchw = 1, a.src[0] = pws_src{nchw_src, nchw_c, (int)x_sstride_};
        } else {
            a.nsrc = x.nseg;
            for (int i = 0; i < x.nseg; ++i) a.src[i] = pws_src{x.seg[i].ptr, x.seg[i].c, x.seg[i].ld};
        }
        a.cout = l.cout, a.w_packed = packed_ + l.w_off, a.bias = packed_ + l.b_off, a.act = bn_on_ ? PWS_ACT_NONE : act;
        a.w_wino = l.ww_off != (size_t)-1 ? packed_ + l.ww_off : nullptr;
        a.w_wring = l.wr_off != (size_t)-1 ? packed_ + l.wr_off : nullptr;
        a.out = bn_on_ ? op.aux[0] : o.seg[0].ptr, a.out_ld = l.cout;
        a.ws = q_ ? splitk_ws2_ : splitk_ws_, a.ws_bytes = math_ == PWS_MATH_FP32 ? splitk_big_ : splitk_bytes_;
        if (math_ == PWS_MATH_BF16 && l.wb_off != (size_t)-1) {
            a.math = PWS_MATH_BF16, a.w_bf16 = packed_ + l.wb_off;
            // pws_netg_pack_weights_for(math = bf16) leaves this layer's Winograd copies out.  The bf16 kernels decline a call
            // with a source of channels % 32 != 0 (wb_off only needs the TOTAL cin % 32 == 0: ngf 16 / 48 in up_bottom1.conv_same);
            // pws_conv2d_fwd then falls through to the fp32 kernels, which must not find the stale Winograd pointers: the direct
            // kernel on w_packed (always packed) takes it (pinned by tests/test_conv_plan_cpu.py).
            a.w_wino = a.w_wring = nullptr;
        }
        a.store = store();
        a.out_sign = o.seg[0].sign, a.out_sign_ld = l.cout / 8;
        if (plan_) {   // what the ladder would launch, on plan_cus_ compute units
            ConvChoice c{};
            c.kernel_id = -1, c.tag = layer;
            rc_ = conv2d_fwd_impl(&a, ConvCtx{nullptr, plan_cus_, false, &c});
            plan_out_.push_back(c);
            return o;
        }
        g_prof_tag = layer;
        rc_ = pws_conv2d_fwd(&a, streams_[q_]);
        g_prof_tag = -1;
        if (bn_on_ && rc_ == PWS_OK) {
            // down_bottom1 is called twice per forward by the reference (x22, x32: same input, same weights) and computed once
            // here: its running statistics take both updates
            const int repeat = (layer == L_DB1_CS || layer == L_DB1_CS + 1) ? 2 : 1;
            rc_ = bn_forward(layer, op.aux[0], (size_t)n_ * oh * ow, act, o.seg[0].ptr, op.aux[1], repeat);
        }
        return o;
    }

    // down.forward (reference :262-264)
    Tn down(int i, const Tn &x) { return conv(L_DOWN1 + (i - 1), x, PWS_ACT_LRELU); }
    // down_bottom.forward (reference :291-298)
    Tn down_bottom(int k, const Tn *x_left, const Tn &x_up) {
        Tn c = conv(L_DB1_CS + 2 * (k - 1), x_up, PWS_ACT_LRELU);
        return conv(L_DB1_CS + 2 * (k - 1) + 1, x_left ? cat(*x_left, c) : c, PWS_ACT_LRELU);
    }
    // up.forward (reference :316-321)
    Tn up(int level, const Tn &x1, const Tn *x2) {
        Tn u = conv(L_UP7 + (7 - level), x1, PWS_ACT_RELU);
        return x2 ? cat(u, *x2) : u;
    }
    // up_bottom.forward (reference :344-350)
    Tn up_bottom(int level, const Tn &x_up, const Tn &x_left, const Tn *x_before) {
        Tn e = conv(L_UB7_MP + 2 * (7 - level) + 1, x_up, PWS_ACT_RELU);
        Tn v = conv(L_UB7_MP + 2 * (7 - level), cat(e, x_left), PWS_ACT_RELU);
        return x_before ? cat(v, *x_before) : v;
    }
    // theta = linear(flatten(x)) (reference :162-163)
    void theta(const Tn &x_s8, int stage, float *theta_out) {
        Op op{OP_THETA, L_FLATTEN, 0, stage, false, x_s8, Tn{}};
        if (bn_on_) {
            const int hidden = L_[L_FLATTEN].cout;
            op.aux[0] = alloc((size_t)n_ * hidden), op.aux[1] = alloc(2 * (size_t)hidden);
            op.aux[2] = alloc((size_t)n_ * 6), op.aux[3] = alloc(12);
        }
        tape_.push_back(op);
        if (!launch_ || rc_ != PWS_OK) return;
        const Layer &f = L_[L_FLATTEN], &l = L_[L_LINEAR];
        const float *xin = x_s8.seg[0].ptr;
        if (bn_on_) {
            // flatten -> BatchNorm over the n samples -> LeakyReLU -> linear -> BatchNorm -> LeakyReLU (reference :148-149 with use_BN)
            rc_ = theta_z1(xin, n_, x_s8.seg[0].c, f.cout, packed_ + f.w_off, packed_ + f.b_off, q_ ? theta_ws2_ : theta_ws_, op.aux[0],
                           streams_[q_]);
            if (rc_ == PWS_OK) rc_ = bn_forward(L_FLATTEN, op.aux[0], (size_t)n_, PWS_ACT_LRELU, h_saved_[stage], op.aux[1], 1);
            if (rc_ == PWS_OK) rc_ = theta_z2(h_saved_[stage], n_, f.cout, packed_ + l.w_off, packed_ + l.b_off, op.aux[2], streams_[q_]);
            if (rc_ == PWS_OK) rc_ = bn_forward(L_LINEAR, op.aux[2], (size_t)n_, PWS_ACT_LRELU, theta_out, op.aux[3], 1);
            return;
        }
        if (io16_) {  // the head is an fp32 GEMV: its 2x2xC input is converted once (n x 4C values)
            rc_ = pws_cvt_bf16_to_f32(xin, theta_x32_[q_], (size_t)n_ * 4 * x_s8.seg[0].c, streams_[q_]);
            if (rc_ != PWS_OK) return;
            xin = theta_x32_[q_];
        }
        rc_ = pws_theta_head_fwd_save(xin, n_, x_s8.seg[0].c, f.cout, packed_ + f.w_off, packed_ + f.b_off,
                                      packed_ + l.w_off, packed_ + l.b_off, q_ ? theta_ws2_ : theta_ws_, theta_out,
                                      h_saved_[stage], streams_[q_]);
    }
    // tanh(out(x)).permute(0,2,3,1) [+ affine_grid(theta)] (reference :174,235-237)
    void field(const Tn &x, int stage, const float *theta_k, int ac, float *resid, float *grid) {
        Op op{OP_FIELD, L_OUT, 0, stage, false, x, Tn{}};
        if (bn_on_) {
            const size_t e = (size_t)n_ * x.h * x.w * 2;
            op.aux[0] = alloc(e), op.aux[1] = alloc(4), op.aux[2] = alloc(e);
        }
        tape_.push_back(op);
        if (!launch_ || rc_ != PWS_OK) return;
        const Layer &o = L_[L_OUT];
        if (bn_on_) {
            // out conv -> BatchNorm(2) -> tanh, then the second tanh + permute + affine add (reference :128,174 with use_BN)
            rc_ = field_head_raw(x.seg[0].ptr, x.seg[0].ld, n_, x.h, x.w, x.seg[0].c, packed_ + o.w_off, packed_ + o.b_off, op.aux[0],
                                 streams_[q_]);
            if (rc_ == PWS_OK) rc_ = bn_forward(L_OUT, op.aux[0], (size_t)n_ * x.h * x.w, PWS_ACT_NONE, op.aux[2], op.aux[1], 1);
            if (rc_ == PWS_OK) rc_ = field_bn_finish(op.aux[2], theta_k, n_, x.h, x.w, ac, resid, grid, streams_[q_]);
            return;
        }
        rc_ = pws_field_head_fwd_s(x.seg[0].ptr, x.seg[0].ld, n_, x.h, x.w, x.seg[0].c, packed_ + o.w_off, packed_ + o.b_off,
                                   theta_k, ac, resid, grid, store(), streams_[q_]);
    }

    // scratch shared by all layers (launches are stream-ordered): split-K partial tiles, the theta head's partials,
    // and (training) the hidden activations of the three theta heads
    void reserve_scratch(int ngf, bool training) {
        training_ = training;
        splitk_bytes_ = (size_t)(2 * n_ > 8 ? 2 * n_ : 8) * (2u << 20);   // (2 n: stages 2 and 3 run as one launch of twice the batch)
        // fp32 math: four times that -- the Winograd ring kernel's two-class units of the transposed layers on 16 x 16 / 32 x 32 maps
        // split K four ways (33 MB of partial sums at batch 8; conv_wring.hip).  The bf16 kernels keep the smaller bound: deeper splits
        // of their small maps measured slower (configs[2] step +0.17 ms)
        // (training forwards in fp32 as well: netG(x, False) stays bit-equal to netG(x)[0][2], reference :237).  The deep splits are a
        // small-batch matter -- from batch 16 on those maps fill the chip without them -- so the extra is capped at the 48 MB batch 8
        // asks for: 2 x 176 MB of scratch at batch 64 instead of 2 x 512 MB in every arena
        splitk_big_ = splitk_bytes_ + ((size_t)48 << 20) < 4 * splitk_bytes_ ? splitk_bytes_ + ((size_t)48 << 20) : 4 * splitk_bytes_;
        splitk_ws_ = alloc(splitk_big_ / sizeof(float));
        splitk_ws2_ = alloc(splitk_big_ / sizeof(float));  // one scratch per queue: the two run concurrently
        theta_ws_ = alloc(pws_theta_head_ws_floats(n_, 4 * ngf, 8 * ngf));
        theta_ws2_ = alloc(pws_theta_head_ws_floats(n_, 4 * ngf, 8 * ngf));
        if (!splitk_ws_ || !splitk_ws2_) splitk_bytes_ = 0, splitk_big_ = 0;
        for (int s = 0; s < 3; ++s) h_saved_[s] = training ? alloc((size_t)n_ * 8 * ngf) : nullptr;
        x_nhwc_ = alloc((size_t)n_ * 256 * 256 * 32);  // bf16 math: NHWC copy of the window (unused in fp32 math)
        theta_x32_[0] = alloc((size_t)n_ * 16 * ngf), theta_x32_[1] = alloc((size_t)n_ * 16 * ngf);  // bf16 storage: fp32 copy of x_s8
        if (bn_on_) {
            bn_ws_bytes_ = pws_bn_ws_bytes(16 * ngf);   // slabs of the BatchNorm reductions, one scratch per queue
            bn_ws_[0] = alloc(bn_ws_bytes_ / sizeof(float)), bn_ws_[1] = alloc(bn_ws_bytes_ / sizeof(float));
        }
    }

  private:
    float *splitk_ws_ = nullptr, *splitk_ws2_ = nullptr, *theta_ws_ = nullptr, *theta_ws2_ = nullptr;
    float *h_saved_[3] = {nullptr, nullptr, nullptr};
    float *x_nhwc_ = nullptr;
    float *theta_x32_[2] = {nullptr, nullptr};
    bool bn_on_ = false;
    BnCfg bn_;
    size_t bn_off_[L_COUNT] = {}, bn_total_ = 0, bn_ws_bytes_ = 0;
    float *bn_ws_[2] = {nullptr, nullptr};
    bool io16_ = false, training_ = false;
    int math_ = PWS_MATH_FP32;
    size_t x_sstride_ = 0;
    bool prune_dead_ = false;
    SideStream *side_ = nullptr;
    hipStream_t streams_[2];
    int q_ = 0;
    size_t splitk_bytes_ = 0, splitk_big_ = 0;
    const float *packed_;
    const LayerTable &L_;
    int n_;
    char *ws_;
    size_t cap_, off_ = 0;
    bool dry_, launch_, plan_;
    int plan_cus_ = 0;
    int rc_ = PWS_OK;
    std::vector<Op> tape_;
    std::vector<ConvChoice> plan_out_;
};

// One forward: what the entry point was given.  thetas may be NULL (then they live in the arena).
// caller_thetas: the caller owns the thetas buffer even when `thetas` is NULL (a planning replay of the training forward: no arena space for them)
struct FwdArgs {
    const float *x = nullptr;
    int n = 0, input_nc = 0, g = 0, is_training = 0, ac = 0;
    float *grids = nullptr, *resid = nullptr, *thetas = nullptr;
    bool caller_thetas = false;
};
// Runs (or only plans) the forward over the arena of E (netg_forward.cpp).
void forward_graph(Exec &E, const FwdArgs &a);

}  // namespace pws
