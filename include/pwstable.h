/*
 * pwstable.h -- C ABI of libpwstable_hip.so: the MI355X (gfx950) implementation of PWStableNet's hot path.
 *
 * This is the drop-in boundary.  Plain pointers and sizes only (no torch types); every pointer is a
 * DEVICE pointer unless stated otherwise; every launch goes to the caller's HIP stream (`stream` is a
 * hipStream_t passed as void*, NULL = the default stream); nothing here allocates, frees or
 * synchronises -- scratch comes from the caller (`ws`), sized by the matching *_workspace_bytes().
 * Return value: 0 on success, negative errno-style code otherwise (pws_last_error() has the text).
 * Re-entrant per stream and per thread.  Global mutable state: the thread-local error string, the process-wide DEFAULTS of
 * pws_set_option() (read only by the entry points that take no pws_netg_opts; the *_opts entry points carry math / store / queue
 * mode in their arguments and read no global), the per-device side queue of the generator forward / backward (one stream per device
 * and process, shared by the EAGER calls of all host threads; every thread owns the events it orders it with -- one pool per CALLER
 * STREAM, so that calls a thread makes for different streams, as autograd's worker thread does, never re-record each other's events --
 * and a call made inside a hipGraph capture forks into a private stream of the calling thread instead, so the shared queue is never
 * part of anybody's capture) and the measurement hooks (pws_prof_*, off by default).
 * What is exercised (tests/test_hip_threads.py, results bit-equal to serial execution): concurrent eager forwards of two generators
 * and of ONE generator from two threads / streams, concurrent replays of graphs, two whole fp32 training steps beside graph replays.
 * NOT bit-reproducible: bf16-math work of one stream beside other GPU work.  While a kernel that leaves room on its CUs executes
 * v_mfma_f32_32x32x16_bf16 (conv_bf16_kernel above all), kernels of other streams -- of other PROCESSES too -- that keep many registers
 * live over long gather sequences compute other values in a few lanes (measured down to that one instruction:
 * profiles/r04_cross_stream_interference.txt; below this library's level, not host-side).  The effect is local to a compute unit: tenants
 * whose streams own DISJOINT CUs (hipExtStreamCreateWithCUMask; the generator on one queue, pws_netg_opts.two_queues = 0, since the side
 * queue is not masked) are bit-reproducible again -- 0 of 150 three-thread rounds against 1 in 10.  One training process per GPU, the
 * deployment this library is built for, never overlaps the two kinds of kernel in the first place.
 * Graph CAPTURE is the caller's: capture after one eager call on the same thread (the library makes its private stream then,
 * not while the capture is open) and while no other host thread issues GPU work -- on ROCm 7.0 captures that overlapped another
 * thread's capture, device-wide synchronisation or training step ended invalidated, crashed inside the runtime, or (1 run in 12)
 * perturbed the other thread's gradient sums (gpurun_out/r4c, tools/probes/thread_race_probe.py).
 *
 * Reference interfaces replaced (paths relative to the mindazhao/PWStableNet checkout; the reference has
 * no native code -- each entry point replaces the PyTorch/ATen op the reference dispatches at that line):
 *   pws_netg_forward              UnetGenerator.forward            lib/networks_cascading.py:152-237
 *   pws_conv2d_fwd                down / down_bottom / up / up_bottom blocks        :245-350
 *                                 (nn.Conv2d :248,269,274,285 ; nn.ConvTranspose2d :306,330,339 ;
 *                                  LeakyReLU :250,271 ; ReLU :305,328 ; torch.cat :296,321,346-350)
 *   pws_theta_head_fwd            flatten + linear -> theta        :148-149,162-163,186-187,208-209
 *   pws_field_head_fwd            out conv + tanh + tanh, permute, + F.affine_grid  :128,164,174,235-237
 *   pws_affine_grid               F.affine_grid                    :164,188,210 ; main_new.py:195
 *   pws_grid_sample_fwd / _bwd    F.grid_sample (+ autograd)       main_new.py:106,109,116,118,197,214,716
 *   pws_upsample_bilinear_ac      UpsamplingBilinear2d(size=...)   main_new.py:706-710
 *   pws_upsample_grid_sample_fwd  the two above fused (720p path)  main_new.py:706-716
 *   pws_upsample_grid_sample_bicubic_*  the fused path with grid_sample(mode="bicubic") (no counterpart in the reference)
 *   pws_border_keep_*             out[t] = covered ? warped[t] : out[t-1] over a scene's warped frames (no counterpart in the reference)
 *   pws_border_mosaic_*           uncovered pixels from the nearest covering frame within a radius, past or future (no counterpart in the reference)
 *   pws_border_edge_*             uncovered pixels from the source frame itself, clamped or mirrored beyond its rim (no counterpart in the reference)
 *   pws_adam_step / _multi / _d   optim.Adam(...).step()           main_new.py:63,216
 *   pws_field_homography          the automatic crop's per-frame findHomography + perspectiveTransform  main_new.py:550-603
 *   pws_scene_change              the window's end clamp, applied at hard cuts too (cut score)          main_new.py:627-633
 *   pws_block_motion / pws_motion_fit  global motion between consecutive window planes: the stability metric (no counterpart in the reference)
 *   pws_field_zoom                the warp field resampled over a per-frame window: zoom to fill (no counterpart in the reference)
 *   pws_field_rigid               the warp field blended towards its fitted homography: rigid warp mode (no counterpart in the reference)
 *   pws_field_wobble              the warp fields' non-rigid part low-passed along time: wobble suppression (no counterpart in the reference)
 *   pws_motion_fit_scaled / pws_path_smooth / pws_field_compose  path smoothing: the measured camera path, low-passed, folded into the warp fields (no counterpart in the reference)
 *   pws_l1_path / pws_l1_path_workspace  the L1-optimal camera path in pws_path_smooth's place: static, linear and parabolic pieces inside a box (no counterpart in the reference)
 *   pws_shutter_rates / pws_field_compose_rows  rolling-shutter correction: per-frame camera rates, and the composition with a correction per row (no counterpart in the reference)
 *   pws_shutter_terms / pws_shutter_estimate  rolling-shutter estimate: the readout share r from the block vectors smoothing has measured (no counterpart in the reference)
 *   pws_path_levels / pws_field_reach / pws_path_limit  crop-bounded smoothing: per frame the share of its correction that keeps a window covered (no counterpart in the reference)
 *   pws_pack_* / pws_netg_pack_weights   state_dict (OIHW / IOHW) -> kernel layout; main_new.py:60,471
 *
 * Layouts.  Frames / images: NCHW fp32 as in the reference.  Warp fields: N,H,W,2 fp32 (x then y,
 * normalised to [-1,1]) as in the reference.  Activations inside the generator: NHWC fp32 with an
 * explicit pixel stride `ld` (floats), so a torch.cat of feature maps is a list of sources, never a copy.
 */
#ifndef PWSTABLE_H
#define PWSTABLE_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PWS_VERSION 5   /* 2: pws_netg_opts carries flags + x_sample_stride (round 3); 4: dpacked is the compact gradient slab
                          (pws_netg_grad_floats / pws_netg_grad_layout), pws_netg_backward_lists (round 4); 5: pws_netg_backward_plan,
                          pws_netg_pack_weights_train (round 5; additions only).  Later additions that change no existing entry
                          point or struct keep the version: the warps' and stabiliser's entries, pws_conv2d_fwd_plan / _bwd_data_plan /
                          pws_netg_forward_plan */

#define PWS_OK 0
#define PWS_EINVAL (-22) /* bad argument / unsupported shape */
#define PWS_ENOMEM (-12) /* caller's workspace too small */
#define PWS_EHIP (-5)    /* HIP runtime reported an error at launch */

typedef void *pws_stream_t; /* hipStream_t */

int pws_version(void);
const char *pws_last_error(void); /* thread-local, never NULL */
/* Process-wide options.  PWS_OPT_TWO_QUEUES (default 1): the generator forward forks an internal second queue so that
 * stage k+1's encoder runs beside stage k's decoder; 0 = issue everything on the caller's stream (clean per-kernel timing). */
#define PWS_OPT_TWO_QUEUES 1
/* PWS_OPT_MATH (default PWS_MATH_FP32): arithmetic of the generator's conv / transposed-conv contractions inside
 * pws_netg_forward / pws_netg_backward.  PWS_MATH_BF16: operands rounded to bf16 (round-to-nearest-even) as they are
 * staged into LDS, products accumulated in fp32 on the bf16 matrix cores (v_mfma_f32_32x32x16_bf16); activations, biases,
 * gradients and master weights stay fp32 in memory.  (BASELINE configs 3/4: "bf16 with MFMA convs"; tolerance vs fp32
 * stated in tests/test_hip_bf16.py.)  Layers the bf16 kernels do not cover (first layer: 31-channel NCHW window; heads)
 * keep fp32 arithmetic. */
#define PWS_OPT_MATH 2
#define PWS_MATH_FP32 0
#define PWS_MATH_BF16 1
/* Element type of activations / gradients in HBM for the bf16 path (per call: the `store` fields; whole generator:
 * PWS_OPT_STORE, default PWS_STORE_FP32).  PWS_STORE_BF16 needs PWS_MATH_BF16. */
/* Whole generator (pws_netg_forward / _backward): with PWS_OPT_MATH = BF16 and PWS_OPT_STORE = BF16 (and ngf % 32 == 0) every
 * activation and activation gradient inside the arena is bf16; inputs, fields, thetas, weights and weight gradients stay fp32.
 * The arena size does not depend on the option (the bf16 tensors use half of their slots). */
#define PWS_OPT_STORE 3
#define PWS_STORE_FP32 0
#define PWS_STORE_BF16 1
/* Measurement only: selects a non-product kernel path, 0 = the product; the ids are listed in pwstablenet_amd/csrc/experiments.h. */
#define PWS_OPT_EXPERIMENT 100
int pws_set_option(int key, int value);
int pws_get_option(int key); /* current value, or PWS_EINVAL */
/* Number of compute units / XCDs the library sees on the current device (diagnostics). */
int pws_device_info(int *compute_units, int *arch_is_gfx950);

/* ---------------------------------------------------------------- activations fused into conv epilogues */
#define PWS_ACT_NONE 0
#define PWS_ACT_LRELU 1 /* LeakyReLU(0.2) */
#define PWS_ACT_RELU 2

/* ---------------------------------------------------------------- conv kinds (what the generator uses) */
#define PWS_CONV_K3S1 0  /* Conv2d k3 s1 p1            (down_bottom*.conv_same)                 */
#define PWS_CONV_K3S2 1  /* Conv2d k3 s2 p1            (down*, down_bottom*.mpconv)             */
#define PWS_CONV_K5S1 2  /* Conv2d k5 s1 p2            (transfer)                               */
#define PWS_CONVT_K3S1 3 /* ConvTranspose2d k3 s1 p1   (up_bottom*.conv_same) == flipped conv   */
#define PWS_CONVT_K4S2 4 /* ConvTranspose2d k4 s2 p1   (up*, up_bottom*.mpconv), 4 sub-pixel 2x2 convs */
#define PWS_CONV_K2S1P0 5 /* Conv2d k2 s1 p0 (flatten) -- packing only; run by pws_theta_head_fwd */
#define PWS_CONV_K1 6     /* Conv2d k1 (linear)        -- packing only                           */
#define PWS_CONV_K3S1_OUT 7 /* Conv2d k3 s1 p1, Cout=2 (out) -- packing only; run by pws_field_head_fwd */

/* Packed size (floats) of one layer's weight for the kernels: [class][tap][cin padded to 16][cout]. */
size_t pws_packed_weight_floats(int kind, int cin, int cout);
/* w_torch: OIHW (conv kinds) or IOHW (convT kinds), dense.  w_packed: pws_packed_weight_floats() floats. */
int pws_pack_conv_weight(const float *w_torch, float *w_packed, int kind, int cin, int cout,
                         pws_stream_t stream);

/* Winograd F(2x2,3x3) weights U = G g G^T as [16][cin padded to 16][cout], computed from the PACKED weights of a
 * K3S1 / CONVT_K3S1 layer (so the transposed conv's tap flip is already applied). */
size_t pws_packed_wino_floats(int cin, int cout);
int pws_pack_conv_weight_wino(const float *w_packed, float *w_wino, int cin, int cout, pws_stream_t stream);
/* The same for ConvTranspose2d k4 s2 p1 (CONVT_K4S2): each of the 4 output parity classes is a 2x2 correlation, run as
 * Winograd F(3x3,2x2) on 4x4 input patches; U as [4 classes][16][cin padded to 16][cout] from the PACKED weights. */
size_t pws_packed_wino_ct4_floats(int cin, int cout);
int pws_pack_conv_weight_wino_ct4(const float *w_packed, float *w_wino, int cin, int cout, pws_stream_t stream);

/* Winograd weights in the layout of the persistent LDS-ring kernel (second generation, taken when the map consists of whole
 * 16 x 32-pixel units and fills the chip): F(2x2,3x3) for K3S1 / CONVT_K3S1 (16 components), F(2x2,2x2) per output parity class
 * for CONVT_K4S2 (2 x 18 components), from the PACKED weights.  Needs cout % 32 == 0 (pws_packed_wring_floats returns 0
 * otherwise: leave pws_conv_args.w_wring NULL).
 * Round 5: also K5S1 with 17..32 input channels and exactly 64 output channels -- the generator's first layer (reference
 * lib/networks_cascading.py:21-23) as Winograd F(2x2,5x5), 36 components on the points {0, 1, -1, 2, -1/2, inf}, for fp32 NCHW
 * sources (pws_conv_args.src_nchw) whose maps are whole 8 x 16-pixel units, at least two per compute unit. */
size_t pws_packed_wring_floats(int kind, int cin, int cout);
int pws_pack_conv_weight_wring(const float *w_packed, float *w_wring, int kind, int cin, int cout, pws_stream_t stream);

/* bf16 copy of a packed weight for the bf16 matrix-core kernels: w_packed is [planes][krows][ncols] fp32 (the forward
 * layout: planes = taps (x4 classes for CONVT_K4S2), krows = cin padded to 16, ncols = cout; or the data-gradient layout:
 * planes = gradient taps, krows = cout, ncols = cin).  Result: [planes][ncols padded to 64][krows padded to 32] bf16
 * (k contiguous: one MFMA B fragment = 8 consecutive k = one 16-byte read), zero padded.  Size in FLOATS (2 bf16 each). */
size_t pws_packed_bf16_floats(int planes, int krows, int ncols);
int pws_pack_weight_bf16(const float *w_packed, void *w_bf16, int planes, int krows, int ncols, pws_stream_t stream);

/* NCHW fp32 [n,c,h,w] -> NHWC fp32 [n,h,w,cpad], channels c..cpad-1 zero (cpad a multiple of 4, c <= cpad <= 32): the bf16
 * first layer reads the 31-channel window (main_new.py:650) as a 32-channel NHWC source. */
int pws_nchw_to_nhwc_pad(const float *x, float *out, int n, int c, int h, int w, int cpad, pws_stream_t stream);
/* ..._s variants: `store` = PWS_STORE_FP32 | PWS_STORE_BF16 selects the element type of the NHWC activation / gradient
 * tensors (`out` here; x / dx of the heads; dy / y of pws_act_bwd_bias_s), everything else is unchanged and fp32. */
int pws_nchw_to_nhwc_pad_s(const float *x, float *out, int n, int c, int h, int w, int cpad, int store, pws_stream_t stream);
/* dst[i] = float(src[i]) for `count` bf16 values; dst (bf16, `count` even) = or += bf16(src[i]). */
int pws_cvt_bf16_to_f32(const void *src, float *dst, size_t count, pws_stream_t stream);
int pws_cvt_f32_to_bf16(const float *src, void *dst, size_t count, int accumulate, pws_stream_t stream);

/* One NHWC source of a (virtually concatenated) conv input: `channels` channels starting at `ptr`,
 * consecutive pixels `ld` floats apart.  ptr 16-byte aligned, ld % 4 == 0, channels % 16 == 0. */
typedef struct pws_src {
    const float *ptr;
    int channels;
    int ld;
} pws_src;

typedef struct pws_conv_args {
    int kind;         /* PWS_CONV_K3S1 | K3S2 | K5S1 | CONVT_K3S1 | CONVT_K4S2 */
    int n, h, w;      /* batch and INPUT height/width */
    int nsrc;         /* 1..4 sources, concatenated along channels in this order */
    pws_src src[4];
    int src_nchw;     /* 1: src[0] is an NCHW tensor with `channels` channels (any count), planes dense; nsrc==1.  src[0].ld: floats
                         between consecutive SAMPLES (0 = dense = channels * h * w; h * w for overlapping sliding windows) */
    int cout;         /* multiple of 4 */
    const float *w_packed;
    const float *bias; /* cout floats or NULL */
    int act;          /* PWS_ACT_* */
    float *out;       /* NHWC, output height/width implied by kind */
    int out_ld;       /* pixel stride of out in floats (>= cout) */
    const float *w_wino; /* optional: Winograd-domain weights from pws_pack_conv_weight_wino (K3S1 / CONVT_K3S1) or
                            pws_pack_conv_weight_wino_ct4 (CONVT_K4S2); when given and the map is large enough the
                            F(2x2,3x3) / F(3x3,2x2) kernel runs instead of the direct one */
    void *ws;         /* optional scratch for split-K partial tiles (16-B aligned) or NULL: small-spatial layers */
    size_t ws_bytes;  /* then run un-split.  Any size works; 64 x n*oh*ow*cout*4 bytes never limits the split. */
    int math;         /* PWS_MATH_FP32 (0) | PWS_MATH_BF16: needs w_bf16 and every source's channels % 32 == 0,
                         otherwise the launch runs in fp32 */
    const void *w_bf16; /* bf16 weights from pws_pack_weight_bf16(w_packed, planes, cin padded to 16, cout) or NULL */
    int store;        /* PWS_STORE_FP32 (0) | PWS_STORE_BF16: every src[].ptr and `out` then point to bf16 elements (channels /
                         ld / out_ld still count ELEMENTS; ld % 8 == 0, out_ld even).  Needs math == PWS_MATH_BF16 and a kind
                         the bf16 kernels cover.  Halves the activation traffic of the bf16 path. */
    const float *w_wring; /* optional: ring-layout Winograd weights from pws_pack_conv_weight_wring (K3S1 / CONVT_K3S1 / CONVT_K4S2,
                         fp32 NHWC sources; K5S1 of the first layer, fp32 NCHW source): tried before w_wino and the direct kernels */
    void *out_sign;   /* optional, store == PWS_STORE_BF16 and cout % 8 == 0 only: the SIGN BITS of `out`, written beside it -- bit (c & 7)
                         of byte out_sign[pixel * out_sign_ld + c / 8] = (out[pixel][c] > 0), for the rounded bf16 value.  What the
                         backward of a LeakyReLU / ReLU block needs of its forward tensor (pws_dst.act_sign): 1/16 of its bytes. */
    int out_sign_ld;  /* bytes per pixel of out_sign (>= cout / 8) */
} pws_conv_args;

int pws_conv2d_fwd(const pws_conv_args *args, pws_stream_t stream);

/* ---------------------------------------------------------------- backward of the conv blocks
 * (autograd of the reference's loss_g.backward(), main_new.py:214, through nn.Conv2d / nn.ConvTranspose2d /
 *  LeakyReLU / ReLU / torch.cat of lib/networks_cascading.py:245-350)
 *
 * Order per layer:  1. pws_act_bwd_bias   dy <- dy * act'(y) in place, db += sum_pixels dy
 *                   2. pws_conv2d_bwd_weight   dW_packed += x (*) dy
 *                   3. pws_conv2d_bwd_data     dx (scattered over the layer's concat sources) = dy (*) W
 * `kind` is always the FORWARD kind of the layer; n,h,w the forward INPUT extent; cout the forward cout. */

/* dy[i] *= act'(y[i]) (LeakyReLU(0.2): y>0 ? 1 : 0.2 ; ReLU: y>0 ? 1 : 0 ; NONE: 1); dbias[c] += sum over pixels.
 * dy, y: dense NHWC [pixels][c]; dbias (nullable): c floats, ACCUMULATED (fp32 atomics, one per workgroup and channel). */
int pws_act_bwd_bias(float *dy, const float *y, size_t pixels, int c, int act, float *dbias, pws_stream_t stream);
/* ws (optional, 16-byte aligned, pws_act_bwd_bias_ws_bytes(c) bytes): the workgroups' partial bias sums go through slabs
 * and a second small launch instead of contended atomics. */
size_t pws_act_bwd_bias_ws_bytes(int c);
int pws_act_bwd_bias_s(float *dy, const float *y, size_t pixels, int c, int act, float *dbias, int store, void *ws,
                       size_t ws_bytes, pws_stream_t stream);

/* Weights re-laid-out for the data-gradient convolution of a layer.  kind in {K3S1, K3S2, CONVT_K3S1, CONVT_K4S2}. */
size_t pws_packed_dgrad_floats(int kind, int cin, int cout);
int pws_pack_conv_weight_dgrad(const float *w_torch, float *w_packed, int kind, int cin, int cout, pws_stream_t stream);

typedef struct pws_dst {
    float *ptr;      /* NHWC gradient buffer of one forward source */
    int channels;
    int ld;
    int accumulate;  /* 0: overwrite, 1: add to what is there (a tensor consumed by several layers) */
    /* Optional, bf16 storage only (store == PWS_STORE_BF16): this call completes the gradient of the tensor `act_y` (the forward
     * tensor this destination is the gradient of, bf16 NHWC, pixel stride act_y_ld, same channels) -- the epilogue then
     * multiplies the (accumulated) sum by act'(act_y) for act = PWS_ACT_LRELU / PWS_ACT_RELU before the single rounding, which
     * saves the separate pws_act_bwd_bias pass over that tensor (a bias gradient, if one is needed, is then taken with
     * pws_act_bwd_bias_s(..., PWS_ACT_NONE, ...)).  act_y == NULL or act == PWS_ACT_NONE: plain gradient. */
    const void *act_y;
    int act_y_ld;
    int act;
    /* Optional beside act_y: its sign bits as written by pws_conv2d_fwd (pws_conv_args.out_sign, same layout, act_sign_ld bytes per
     * pixel).  A kernel that knows them reads one byte instead of 16 per 8 channels (the persistent ring kernel does when every
     * destination with an act has them); the others read act_y, which must be given as well.  Same result bit for bit. */
    const void *act_sign;
    int act_sign_ld;
} pws_dst;

typedef struct pws_conv_bwd_data_args {
    int kind;
    int n, h, w;       /* forward input extent */
    int cout;          /* forward output channels (multiple of 16) */
    const float *gout; /* dy, NHWC [n, oh, ow, cout], pixel stride gout_ld */
    int gout_ld;
    const float *w_dgrad; /* from pws_pack_conv_weight_dgrad */
    int ndst;          /* 1..4 destinations = the forward sources, in concat order */
    pws_dst dst[4];
    void *ws;          /* optional split-K scratch, as in pws_conv_args */
    size_t ws_bytes;
    int math;          /* as in pws_conv_args (bf16 needs w_dgrad_bf16 and cout % 32 == 0) */
    const void *w_dgrad_bf16; /* pws_pack_weight_bf16(w_dgrad, dgrad taps, cout, cin) or NULL */
    int store;         /* PWS_STORE_BF16: gout and every dst[].ptr hold bf16 elements (accumulation rounds to bf16) */
} pws_conv_bwd_data_args;
int pws_conv2d_bwd_data(const pws_conv_bwd_data_args *args, pws_stream_t stream);

/* ---------------------------------------------------------------- which kernel a conv call runs (host only, no GPU needed)
 * One conv launch as the dispatch ladder decides it (pwstablenet_amd/csrc/conv_dispatch.hip): the record a plan call reports is the
 * record the launching call acts on -- grid, workgroup and LDS are computed once, by the plan step of the chosen kernel family. */
#define PWS_FOLLOW_NONE 0
#define PWS_FOLLOW_REDUCE 1 /* splitk_reduce_kernel adds the K splits' partial sums (and runs the epilogue) */
#define PWS_FOLLOW_SIGN 2   /* sign_bits_kernel writes pws_conv_args.out_sign behind the launch(es) */
typedef struct pws_conv_choice {
    int kernel_id;    /* index for pws_prof_kernel_name() */
    int variant[4];   /* what the family's template switch keys on, unused entries 0.  Tiled kernels (conv_mfma_kernel, conv_bf16_kernel):
                         tile index of the candidate table (deep tiles: 8 + index), TH, TW, TN.  conv_ring_kernel: mode, pixels per unit,
                         tile width, sign-bit epilogue.  conv_ringf_kernel: mode, tile height, channels per unit / 32, half workgroups.
                         wino_ring_kernel: mode, 16-wide units, ablation.  One-shot kernels: pixel tiles, channel tiles and waves along M
                         per workgroup, taps held.  wino_kernel: mode. */
    unsigned grid[3];
    int threads;      /* workgroup size */
    int lds_bytes;    /* dynamic LDS of the launch */
    int ksplit;       /* K splits (1 = none) */
    int follow;       /* PWS_FOLLOW_* bits */
    int tag;          /* pws_netg_forward_plan: the layer index; else 0 */
} pws_conv_choice;
/* What pws_conv2d_fwd / pws_conv2d_bwd_data would launch for `args` on a device of `compute_units` CUs: same argument checks, same
 * return codes, no launch and no HIP call.  Pointers are inspected for NULL and alignment only, never dereferenced.  n == 0: PWS_OK and
 * kernel_id -1.  PWS_OPT_EXPERIMENT switches act as they do on a launch. */
int pws_conv2d_fwd_plan(const pws_conv_args *args, int compute_units, pws_conv_choice *out);
int pws_conv2d_bwd_data_plan(const pws_conv_bwd_data_args *args, int compute_units, pws_conv_choice *out);

typedef struct pws_conv_bwd_weight_args {
    int kind;          /* K3S1 | K3S2 | K5S1 | CONVT_K3S1 | CONVT_K4S2 */
    int n, h, w;       /* forward input extent */
    int nsrc;          /* forward sources (x), as in pws_conv_args */
    pws_src src[4];
    int src_nchw;      /* first layer: x is the dense NCHW window */
    int cout;
    const float *gout; /* dy (already multiplied by act'), NHWC dense, pixel stride gout_ld */
    int gout_ld;
    float *dw_packed;  /* gradient in the FORWARD packed layout (pws_packed_weight_floats), ACCUMULATED into
                          (fp32 atomics: several pixel ranges, and stages 2/3 share weights) */
    int math;          /* PWS_MATH_BF16: x and dy rounded to bf16 at LDS staging, fp32 accumulation; dW stays fp32 */
    int store;         /* PWS_STORE_BF16: src[].ptr and gout hold bf16 elements (dw_packed stays fp32) */
    float *dbias;      /* optional: dbias[co] += sum over the pixels of gout[., co] (fp32 atomics), taken from the dy tiles the
                          weight-gradient kernel stages anyway -- for a gout that already is the gradient wrt the pre-activation
                          (pws_dst.act_y) this replaces the pws_act_bwd_bias pass */
    int deterministic; /* 1: no pixel split -- every element of dw_packed / dbias receives exactly one fp32 atomic add from this
                          launch, so repeated runs are bit-identical (slower: one workgroup per channel block) */
    /* Optional SECOND operand pair of the same geometry (n, h, w, channels, strides as src[] / gout; ABI version 4): stages 2 and 3 of the
     * generator run the same modules (lib/networks_cascading.py:178-214), so a shared layer's weight gradient is the sum of two
     * contributions -- given both, the ring kernels walk the two tensors' tiles in ONE launch (one prologue, one set of epilogue
     * atomics: 5-11 % less than two launches on the decoder shapes); kinds the ring does not cover run as two launches.
     * gout2 == NULL: none. */
    const void *src2_ptr[4];
    const float *gout2;
} pws_conv_bwd_weight_args;
int pws_conv2d_bwd_weight(const pws_conv_bwd_weight_args *args, pws_stream_t stream);

/* Inverse of pws_pack_conv_weight: packed gradient -> torch layout (OIHW / IOHW), overwriting dw_torch. */
int pws_unpack_conv_weight(const float *w_packed, float *w_torch, int kind, int cin, int cout, pws_stream_t stream);

/* theta = LReLU(W2 . LReLU(W1 . vec(x) + b1) + b2)   x: NHWC [n,2,2,c] (ld == c), theta: [n,6].
 * w_flat packed as PWS_CONV_K2S1P0 (c -> hidden), w_lin packed as PWS_CONV_K1 (hidden -> 6).
 * ws: pws_theta_head_ws_floats(n, c, hidden) floats of scratch (K-split partial sums). */
size_t pws_theta_head_ws_floats(int n, int c, int hidden);
int pws_theta_head_fwd(const float *x, int n, int c, int hidden, const float *w_flat, const float *b_flat,
                       const float *w_lin, const float *b_lin, float *ws, float *theta, pws_stream_t stream);
/* Same, additionally saving the hidden activations h[n,hidden] (post-LeakyReLU) for pws_theta_head_bwd. */
int pws_theta_head_fwd_save(const float *x, int n, int c, int hidden, const float *w_flat, const float *b_flat,
                            const float *w_lin, const float *b_lin, float *ws, float *theta, float *h_saved,
                            pws_stream_t stream);
/* Backward of the theta head.  dtheta[n,6] in; dw_flat (packed K2S1P0 layout [4c][hidden]), db_flat, dw_lin
 * ([hidden][6]), db_lin ACCUMULATED; dx (nullable) [n,2,2,c] overwritten or accumulated; ws: n*hidden floats. */
int pws_theta_head_bwd(const float *x, int n, int c, int hidden, const float *w_flat, const float *w_lin,
                       const float *h_saved, const float *theta, const float *dtheta, float *dw_flat, float *db_flat,
                       float *dw_lin, float *db_lin, float *dx, int dx_accumulate, float *ws, pws_stream_t stream);

/* field = tanh(tanh(conv3x3(x; 2 outputs) + b)) as N,H,W,2, plus affine_grid(theta) when theta != NULL.
 * x: NHWC [n,h,w,c] pixel stride ld.  w_out packed as PWS_CONV_K3S1_OUT.  resid (nullable) receives the
 * field without the affine part; grid (nullable) receives resid + affine. */
int pws_field_head_fwd(const float *x, int ld, int n, int h, int w, int c, const float *w_out,
                       const float *b_out, const float *theta, int align_corners, float *resid, float *grid,
                       pws_stream_t stream);

int pws_field_head_fwd_s(const float *x, int ld, int n, int h, int w, int c, const float *w_out, const float *b_out,
                         const float *theta, int align_corners, float *resid, float *grid, int store, pws_stream_t stream);

/* Backward of pws_field_head_fwd.  resid: the forward's residual output; g_grid / g_resid (either nullable): gradients
 * wrt the two outputs.  dx (nullable) [n,h,w,c] overwritten or accumulated; dw_out (packed [9][c][2]) and db_out[2]
 * ACCUMULATED (atomics); dtheta (nullable) [n,6] overwritten; ws: n*h*w*2 floats. */
int pws_field_head_bwd(const float *x, int ld, int n, int h, int w, int c, const float *w_out, const float *resid,
                       const float *g_grid, const float *g_resid, int align_corners, float *dx, int dx_ld,
                       int dx_accumulate, float *dw_out, float *db_out, float *dtheta, float *ws, pws_stream_t stream);

int pws_field_head_bwd_s(const float *x, int ld, int n, int h, int w, int c, const float *w_out, const float *resid,
                         const float *g_grid, const float *g_resid, int align_corners, float *dx, int dx_ld, int dx_accumulate,
                         float *dw_out, float *db_out, float *dtheta, float *ws, int store, pws_stream_t stream);

/* The same; dx_act = PWS_ACT_LRELU / PWS_ACT_RELU (bf16 storage only): this call completes the gradient of x, which is the
 * output of that activation -- dx (after the accumulation) is multiplied by act'(x), as pws_dst.act_y does for the
 * data-gradient calls.  PWS_ACT_NONE: pws_field_head_bwd_s. */
int pws_field_head_bwd_act(const float *x, int ld, int n, int h, int w, int c, const float *w_out, const float *resid,
                           const float *g_grid, const float *g_resid, int align_corners, float *dx, int dx_ld, int dx_accumulate,
                           float *dw_out, float *db_out, float *dtheta, float *ws, int store, int dx_act, pws_stream_t stream);

/* F.affine_grid(theta[n,2,3], (n,*,h,w)) -> grid[n,h,w,2] */
int pws_affine_grid(const float *theta, float *grid, int n, int h, int w, int align_corners,
                    pws_stream_t stream);

/* F.grid_sample(input[n,c,h,w], grid[n,ho,wo,2]) -> out[n,c,ho,wo]; bilinear, zeros padding. */
int pws_grid_sample_fwd(const float *input, const float *grid, float *out, int n, int c, int h, int w, int ho,
                        int wo, int align_corners, pws_stream_t stream);
/* Backward.  ginput (nullable): [n,c,h,w], OVERWRITTEN (zeroed then scatter-added with atomics);
 * ggrid (nullable): [n,ho,wo,2], overwritten. */
int pws_grid_sample_bwd(const float *gout, const float *input, const float *grid, float *ginput, float *ggrid,
                        int n, int c, int h, int w, int ho, int wo, int align_corners, pws_stream_t stream);

/* Bilinear resize with align_corners=True of an NCHW tensor (reference resizes the field as NCHW). */
int pws_upsample_bilinear_ac(const float *in, float *out, int n, int c, int h, int w, int ho, int wo,
                             pws_stream_t stream);
/* Adjoint of pws_upsample_bilinear_ac: gin[n,c,h,w] (overwritten) from gout[n,c,ho,wo]; deterministic gather.  autograd of
 * torch.nn.UpsamplingBilinear2d when the reference's video loop runs with gradients enabled (main_new.py:697-710). */
int pws_upsample_bilinear_ac_bwd(const float *gout, float *gin, int n, int c, int h, int w, int ho, int wo,
                                 pws_stream_t stream);
/* Adjoint of pws_affine_grid: gtheta[n,6] (overwritten) = sum over h,w of ggrid[n,h,w,:] (x) [x_w, y_h, 1]; autograd of
 * F.affine_grid (lib/networks_cascading.py:164,188,210; main_new.py:195) for callers outside the fused field head. */
int pws_affine_grid_bwd(const float *ggrid, float *gtheta, int n, int h, int w, int align_corners, pws_stream_t stream);

/* Fused 720p path: field[n,fh,fw,2] is resized on the fly (align_corners=True) to (h,w) and applied to
 * input[n,c,h,w] -> out[n,c,h,w]; the resized field is never materialised. */
int pws_upsample_grid_sample_fwd(const float *input, const float *field, float *out, int n, int c, int h,
                                 int w, int fh, int fw, int align_corners, pws_stream_t stream);

/* The same for uint8 frames in the layout OpenCV hands over (main_new.py:679-684,717-721): frame_hwc / out_hwc are
 * [n,h,w,3] uint8; the blend runs in fp32 exactly as above and is truncated like numpy's astype(uint8).  swap_rb: output
 * channel c samples input channel 2-c (the reference's COLOR_BGR2RGB before the warp).  w % 4 == 0, out 4-byte aligned.
 * 6 bytes per pixel of frame traffic instead of 24. */
int pws_upsample_grid_sample_u8(const unsigned char *frame_hwc, const float *field, unsigned char *out_hwc, int n, int h, int w,
                                int fh, int fw, int swap_rb, int align_corners, pws_stream_t stream);

/* The image processing either side of the path in the reference's video loop, on the device (csrc/frameio.hip; follows
 * OpenCV 4.x's algorithms -- cv2 is not available to pin against):
 * out[n,oh,ow] = cv2.resize(cv2.cvtColor(frame, COLOR_BGR2GRAY), (ow, oh), INTER_AREA) [/255*2-1 when normalize]
 * (main_new.py:639-643,653-667); frames [n,h,w,3] uint8 as cv2 delivers them (swap_rb: they are RGB instead). */
int pws_gray_area_u8(const unsigned char *frames_hwc, float *out, int n, int h, int w, int oh, int ow, int normalize, int swap_rb,
                     pws_stream_t stream);
/* out[n,h/2,w/2,3] = cv2.resize(in, (w/2, h/2), INTER_AREA) [+ R<->B swap] (main_new.py:723-725) */
int pws_area_half_u8(const unsigned char *in_hwc, unsigned char *out_hwc, int n, int h, int w, int swap_rb, pws_stream_t stream);
/* out[n,oh,ow,3] = cv2.resize(in[n,h,w,3], (ow, oh), INTER_AREA) [+ R<->B swap] for ANY down-scaling ratio: the reference writes
 * every output frame at (640, 360) whatever the source size (main_new.py:723).  2 x 2 -> pws_area_half_u8; both ratios integer
 * (1080p, 2160p) -> OpenCV's integer-area path (int sum * float(1/area), round half to even); otherwise its area tables. */
int pws_area_resize_u8(const unsigned char *in_hwc, unsigned char *out_hwc, int n, int h, int w, int oh, int ow, int swap_rb,
                       pws_stream_t stream);

/* 4:2:0 YUV frames as decoders hand them over: [n][h*3/2][w] uint8, the Y plane (h x w) then the chroma -- layout 0 NV12 (h/2 rows of w
 * bytes, U and V interleaved), 1 I420 (the U plane h/2 x w/2, then the V plane).  BT.601 limited range, 8 bit.
 * out[n,oh,ow] = pws_gray_area_u8 of the BGR frame cv2.cvtColor(frame, COLOR_YUV2BGR_NV12 / _I420) gives (OpenCV 4.x's fixed point,
 * restated: csrc/frameio.hip), in one launch.  h and w even. */
int pws_gray_area_yuv420_u8(const unsigned char *frames, float *out, int n, int h, int w, int oh, int ow, int normalize, int layout,
                            pws_stream_t stream);
/* INTER_AREA (pws_area_resize_u8's algorithms) of a 1- or 2-channel byte plane [n][h][w][c] -> [n][oh][ow][c]; in / out point at sample 0's
 * plane, samples in_stride / out_stride bytes apart (the planes of packed YUV frames). */
int pws_area_resize_plane_u8(const unsigned char *in, size_t in_stride, unsigned char *out, size_t out_stride, int n, int h, int w, int c,
                             int oh, int ow, pws_stream_t stream);
/* pws_upsample_grid_sample_u8 for packed 4:2:0 frames (layout as pws_gray_area_yuv420_u8), YUV in and out: each plane is warped by the
 * field resized (align_corners=True) to the plane's own size, fp32 blend truncated; taps outside a plane read 16 (Y) / 128 (U, V), BT.601
 * black.  h even, w % 4 == 0, frames and out 4-byte aligned.  3 bytes of frame traffic per pixel. */
int pws_upsample_grid_sample_yuv420_u8(const unsigned char *frames, const float *field, unsigned char *out, int n, int h, int w, int fh,
                                       int fw, int layout, int align_corners, pws_stream_t stream);

/* 10-bit 4:2:0 frames [n][h*3/2][w] of little-endian 16-bit words in the 8-bit formats' plane order; layout 0 P010 (the Y plane, then h/2 rows
 * of interleaved U V; the sample in the HIGH 10 bits, word = v10 << 6; the low 6 bits of input words are ignored, output words have them
 * zero), 1 I010 / yuv420p10le (Y, U and V planes; the sample in the LOW 10 bits; input words above 1023 are clamped).  BT.601 limited range.
 * out[n,oh,ow] = pws_gray_area_yuv420_u8 of the frames' 8-bit reduction v8 = min(255, (v10 + 2) >> 2), fused into the loads: the planes of
 * the NV12 / I420 clip of the reduced samples bit for bit.  h and w even. */
int pws_gray_area_yuv420_u16(const unsigned short *frames, float *out, int n, int h, int w, int oh, int ow, int normalize, int layout,
                             pws_stream_t stream);
/* INTER_AREA of a 1- or 2-channel plane of 10-bit samples [n][h][w][c] -> [n][oh][ow][c] on the 10-bit values (cv::resize's dispatch for
 * 16-bit unsigned: 2 x 2 mean, integer-ratio block sum * float(1 / area), area tables), saturated to 0..1023 and stored in the layout's
 * placement; in / out point at sample 0's plane, samples in_stride / out_stride 16-bit WORDS apart (the planes of packed frames). */
int pws_area_resize_plane_u16(const unsigned short *in, size_t in_stride, unsigned short *out, size_t out_stride, int n, int h, int w, int c,
                              int oh, int ow, int layout, pws_stream_t stream);
/* pws_upsample_grid_sample_yuv420_u8 for 10-bit frames (layout as pws_gray_area_yuv420_u16), YUV in and out: each plane is warped by the
 * field resized (align_corners=True) to the plane's own size, fp32 blend of the 10-bit values truncated and clamped to 0..1023; taps outside
 * a plane read 64 (Y) / 512 (U, V), BT.601 black.  h even, w % 4 == 0, frames and out 8-byte aligned.  6 bytes of frame traffic per pixel. */
int pws_upsample_grid_sample_yuv420_u16(const unsigned short *frames, const float *field, unsigned short *out, int n, int h, int w, int fh,
                                        int fw, int layout, int align_corners, pws_stream_t stream);

/* Bicubic twins of the four fused warps above (csrc/warp_bicubic.hip): same arguments, layouts, alignment rules and error codes; the field
 * is resized and un-normalised with the same fp32 operations, then 4 x 4 taps are blended with Keys' cubic convolution, A = -0.75 -- torch's
 * F.grid_sample(mode="bicubic", padding_mode="zeros").  With x0 = floor(ix), t = ix - x0 the weights of columns x0-1 .. x0+2 are
 * [c2(t+1), c1(t), c1(1-t), c2(2-t)], c1(s) = ((A+2)s - (A+3))s^2 + 1, c2(s) = ((As - 5A)s + 8A)s - 4A, rows alike; a tap outside the plane reads
 * the pad value (0; 16 / 128 for 8-bit Y / chroma, 64 / 512 for 10-bit), a pixel whose 16 taps are all outside is the pad value exactly.  A
 * cubic overshoots: integer outputs are clamped to 0..255 / 0..1023, then truncated; float output is not clamped.  Forward only.  Every plane
 * must hold the 4-column window: w >= 4, and w >= 8 for the 4:2:0 formats (PWS_EINVAL otherwise). */
int pws_upsample_grid_sample_bicubic_fwd(const float *input, const float *field, float *out, int n, int c, int h, int w, int fh, int fw,
                                         int align_corners, pws_stream_t stream);
int pws_upsample_grid_sample_bicubic_u8(const unsigned char *frame_hwc, const float *field, unsigned char *out_hwc, int n, int h, int w,
                                        int fh, int fw, int swap_rb, int align_corners, pws_stream_t stream);
int pws_upsample_grid_sample_bicubic_yuv420_u8(const unsigned char *frames, const float *field, unsigned char *out, int n, int h, int w,
                                               int fh, int fw, int layout, int align_corners, pws_stream_t stream);
int pws_upsample_grid_sample_bicubic_yuv420_u16(const unsigned short *frames, const float *field, unsigned short *out, int n, int h, int w,
                                                int fh, int fw, int layout, int align_corners, pws_stream_t stream);

/* "Keep" borders for the fused byte warps above (csrc/border_keep.hip; no counterpart in the reference): n consecutive WARPED frames of one
 * scene, modified in place.  A pixel of frame t whose source position (ix, iy) -- formed from field[t] with the warps' own fp32 operations --
 * does not satisfy m <= ix <= w-1-m and m <= iy <= h-1-m (per plane: its own size and field resize; m = 0, or 1 with `bicubic`: all 4 / all 16
 * taps inside; NaN is outside) takes the value of frame t-1 after the same rule, frame -1 being `initial` (one frame in the frames' layout):
 * an earlier output frame, copied as it is, or -- initial_is_source -- a source frame read as the warp would write it (swap_rb; P010 words
 * masked to v10 << 6; I010 words clamped to 1023).  Coverage is binary: every output sample is a copy of one of those two samples.  `initial`
 * must not overlap `frames`.  Arguments, layouts, alignment rules (they hold for `initial` too) and error codes are the warps': w % 4 == 0,
 * even h for 4:2:0, and w >= 8 for 4:2:0 with `bicubic` (PWS_EINVAL otherwise).  One launch; the traffic is the fields plus the uncovered
 * pixels, not the frames. */
int pws_border_keep_u8(unsigned char *frames_hwc, const float *field, const unsigned char *initial, int initial_is_source, int n, int h, int w,
                       int fh, int fw, int swap_rb, int align_corners, int bicubic, pws_stream_t stream);
int pws_border_keep_yuv420_u8(unsigned char *frames, const float *field, const unsigned char *initial, int initial_is_source, int n, int h,
                              int w, int fh, int fw, int layout, int align_corners, int bicubic, pws_stream_t stream);
int pws_border_keep_yuv420_u16(unsigned short *frames, const float *field, const unsigned short *initial, int initial_is_source, int n, int h,
                               int w, int fh, int fw, int layout, int align_corners, int bicubic, pws_stream_t stream);

/* Packed YUV frames of any chroma subsampling: the *_yuv420_* entries above with `chroma` behind `layout` -- 0: 4:2:0 ([n][h*3/2][w], the
 * entries above bit for bit), 1: 4:2:2 ([n][2h][w]: Y, then h rows of w/2 interleaved U V pairs -- NV16 / P210, layout 0 -- or U and V planes
 * of h x w/2 -- I422 / I210, layout 1), 2: 4:4:4 ([n][3h][w]: Y, U, V planes of h x w -- I444 / I410, layout 1 only: interleaved 4:4:4, NV24 /
 * P410, is PWS_EINVAL).  Per plane the semantics are the 4:2:0 entries': a plane is warped by the field resized to the plane's OWN size, pads
 * with BT.601 black, 16-bit words are read and written as P010's (layout 0) / I010's (layout 1); the window planes decode pixel (x, y) with
 * the chroma sample (x >> cx, y >> cy), (cx, cy) = (1, 1), (1, 0), (0, 0).  One shape rule for every subsampling: h even, w % 4 == 0 (the
 * window planes: h and w even); the bicubic entries and the keep pass with `bicubic` need a chroma plane of 4 columns: w >= 8, any w at
 * 4:4:4.  Alignment rules as above. */
int pws_gray_area_yuv_u8(const unsigned char *frames, float *out, int n, int h, int w, int oh, int ow, int normalize, int layout, int chroma,
                         pws_stream_t stream);
int pws_gray_area_yuv_u16(const unsigned short *frames, float *out, int n, int h, int w, int oh, int ow, int normalize, int layout, int chroma,
                          pws_stream_t stream);
int pws_upsample_grid_sample_yuv_u8(const unsigned char *frames, const float *field, unsigned char *out, int n, int h, int w, int fh, int fw,
                                    int layout, int chroma, int align_corners, pws_stream_t stream);
int pws_upsample_grid_sample_yuv_u16(const unsigned short *frames, const float *field, unsigned short *out, int n, int h, int w, int fh, int fw,
                                     int layout, int chroma, int align_corners, pws_stream_t stream);
int pws_upsample_grid_sample_bicubic_yuv_u8(const unsigned char *frames, const float *field, unsigned char *out, int n, int h, int w, int fh,
                                            int fw, int layout, int chroma, int align_corners, pws_stream_t stream);
int pws_upsample_grid_sample_bicubic_yuv_u16(const unsigned short *frames, const float *field, unsigned short *out, int n, int h, int w, int fh,
                                             int fw, int layout, int chroma, int align_corners, pws_stream_t stream);
int pws_border_keep_yuv_u8(unsigned char *frames, const float *field, const unsigned char *initial, int initial_is_source, int n, int h, int w,
                           int fh, int fw, int layout, int chroma, int align_corners, int bicubic, pws_stream_t stream);
int pws_border_keep_yuv_u16(unsigned short *frames, const float *field, const unsigned short *initial, int initial_is_source, int n, int h, int w,
                            int fh, int fw, int layout, int chroma, int align_corners, int bicubic, pws_stream_t stream);

/* "Mosaic" borders for the fused integer warps (csrc/border_mosaic.hip; no counterpart in the reference): `frames` holds n contiguous WARPED
 * frames of one scene, as the black-border warps above wrote them, and `field` the n fields that warped them.  Planes, source positions and
 * coverage are pws_border_keep's (per plane: its own size and field resize; m = 0, or 1 with `bicubic`; NaN is outside).  Frames
 * [start, stop) are filled in place; all n frames are donors.  A position p of frame t that is not covered takes the sample of the nearest
 * frame that covers p: k = 1 .. radius in this order, frame t-k if t-k >= 0 and it covers p (the past wins a tie), else frame t+k if
 * t+k < n and it covers p.  Without a donor within `radius` the warp's sample stays and the position counts as unfilled.  Covered samples
 * are never modified and donors are read only where they are covered, so filled frames are as good donors as unfilled ones: the result
 * for [start, stop) depends on frames [start-radius, stop+radius) alone, and any chunking gives the same bytes.
 * unfilled: (stop - start) int32 in DEVICE memory, WRITTEN (cleared on the stream, then added to by the kernel): per frame the number of
 * Y-plane positions (BGR: pixel positions) without a donor.  `chroma` is 0 / 1 / 2 for 4:2:0 / 4:2:2 / 4:4:4 and is always passed.
 * Shapes, layouts, alignment rules and error codes are pws_border_keep's; PWS_EINVAL also for radius outside 1 .. 15 and a range that
 * does not satisfy 0 <= start <= stop <= n.  One launch (and a 4 (stop - start) byte clear); the traffic is the fields once plus the
 * uncovered samples and their donors, not the frames. */
int pws_border_mosaic_u8(unsigned char *frames_hwc, const float *field, int *unfilled, int n, int start, int stop, int radius, int h, int w,
                         int fh, int fw, int align_corners, int bicubic, pws_stream_t stream);
int pws_border_mosaic_yuv_u8(unsigned char *frames, const float *field, int *unfilled, int n, int start, int stop, int radius, int h, int w,
                             int fh, int fw, int layout, int chroma, int align_corners, int bicubic, pws_stream_t stream);
int pws_border_mosaic_yuv_u16(unsigned short *frames, const float *field, int *unfilled, int n, int start, int stop, int radius, int h, int w,
                              int fh, int fw, int layout, int chroma, int align_corners, int bicubic, pws_stream_t stream);

/* Edge modes for the fused integer warps (csrc/border_edge.hip; no counterpart in the reference): `frames` holds n contiguous WARPED frames
 * as the black-border warps above wrote them, `source` the n SOURCE frames they were warped from (same shape and layout) and `field` the n
 * fields that warped them.  Planes, source positions and coverage are pws_border_keep's (per plane: its own size and field resize; m = 0, or
 * 1 with `bicubic`; NaN is outside).  A covered sample and one with a non-finite coordinate stay as they are.  Every other sample is
 * replaced whole by the source plane sampled at (ix, iy) with the plane continued beyond its rim:
 *   Q( sum_i sum_j wy_i wx_j v(fold(y0 + i, h), fold(x0 + j, w)) ),  x0 = floor(ix), y0 = floor(iy); taps 0, 1 with weights (1 - t, t), or
 *   with `bicubic` taps -1 .. 2 with the Keys weights (A = -0.75) of the bicubic warps;
 *   edge 1 (clamp):  fold(i, n) = min(max(i, 0), n - 1)                          -- torch's padding_mode="border", OpenCV's BORDER_REPLICATE;
 *   edge 2 (mirror): k = i mod 2 (n - 1); fold = k < n ? k : 2 (n - 1) - k; 0 when n == 1  -- "reflection", BORDER_REFLECT_101;
 *   v: the source sample under the warps' read rules (swap_rb; P010 word >> 6; I010 min(word, 1023)); Q: clamp to 0 .. 255 / 0 .. 1023, then
 *   truncate, written as the warps write it (P010: v10 << 6).
 * Taps that all hold one value give that value exactly; every finite coordinate is defined (floor is bounded before the conversion, the fold
 * is integer arithmetic).  No other frame is read.  `source` must not overlap `frames` (PWS_EINVAL); edge other than 1 or 2 is PWS_EINVAL.
 * `chroma` is 0 / 1 / 2 for 4:2:0 / 4:2:2 / 4:4:4 and is always passed.  Shapes, layouts, alignment rules (they hold for `source` too) and
 * error codes are pws_border_keep's.  One launch; the traffic is the fields plus the uncovered samples and their taps, not the frames. */
int pws_border_edge_u8(unsigned char *frames_hwc, const unsigned char *source_hwc, const float *field, int n, int h, int w, int fh, int fw,
                       int swap_rb, int align_corners, int bicubic, int edge, pws_stream_t stream);
int pws_border_edge_yuv_u8(unsigned char *frames, const unsigned char *source, const float *field, int n, int h, int w, int fh, int fw, int layout,
                           int chroma, int align_corners, int bicubic, int edge, pws_stream_t stream);
int pws_border_edge_yuv_u16(unsigned short *frames, const unsigned short *source, const float *field, int n, int h, int w, int fh, int fw,
                            int layout, int chroma, int align_corners, int bicubic, int edge, pws_stream_t stream);

/* The automatic crop of the reference's video loop (main_new.py:484-606, a block it keeps inside a string literal), per frame
 * (csrc/homography.hip): field[n,fh,fw,2] resized to the h0 x w0 source frame as pws_upsample_bilinear_ac does is sampled on the
 * 20 x 20 lattice rows h0/2 + (a-10)*15, columns w0/2 + (b-10)*30 (p1, fp32); the homography M (m33 = 1) from p1 to the lattice's own
 * position in [-1,1] (p2) minimising sum |p2 - pi(M [p1,1])|^2 over the 400 points is fitted in fp64 (Hartley-normalised DLT, then
 * Gauss-Newton: cv2.findHomography's all-inlier result, unpinned: cv2 is not available), and the corners (-1,-1), (-1,.992),
 * (.992,.992), (.992,-1) mapped through it (|w| <= FLT_EPSILON -> 0, as cv2.perspectiveTransform) give the frame's bounds in source
 * pixels.  m_out[n,9] fp64 row-major; bounds_out[n,4] = top, bottom, left, right; pts_out[n,400,2] = p1 (may be NULL).  Samples
 * without spread, a normal matrix that is not positive definite or a result that is not finite give NaN M and bounds.
 * h0 >= 300 and w0 >= 600 (the lattice must fit); any fh, fw >= 1; n == 0 returns PWS_OK and launches nothing.  PWS_EINVAL: n < 0,
 * fh or fw < 1, a frame too small for the lattice, NULL field / m_out / bounds_out, field, pts_out or m_out not 8-byte aligned,
 * bounds_out not 4-byte aligned. */
int pws_field_homography(const float *field, int n, int fh, int fw, int h0, int w0, double *m_out, float *bounds_out, float *pts_out,
                         pws_stream_t stream);

/* Zoom to fill (csrc/field_zoom.hip; no counterpart in the reference).  Every fused warp above resizes its small field to the frame
 * (align_corners=True) before it samples, so a zoom into a window of the warped frame is a resampling of the FIELD over that window: the
 * field's values are kept, only its domain changes, and the warp that follows produces the zoomed frame in its single resampling pass.
 * field[n,fh,fw,2] -> out[n,fh,fw,2]; coef[n,4] = Ax, Bx, Ay, By of frame t, in DEVICE memory.  For node (i, j) of frame t:
 *   sx = clamp(fmaf(Bx, (float)j, Ax), 0, fw-1), x0 = floor(sx), x1 = x0 + (x0 < fw-1), lx = sx - x0, hx = 1 - lx; sy, y0, y1, ly, hy alike
 *   from Ay, By, i; out[t,i,j,c] = fma(ly, fma(lx, F[y1,x1], hx * F[y1,x0]), hy * fma(lx, F[y0,x1], hx * F[y0,x0])) per component c (the
 *   warps' own field interpolation).  Ax = Ay = 0, Bx = By = 1 returns a finite field bit for bit (a -0.0 may come back as +0.0).
 * NaN coefficients sample node 0; no coefficient can make the kernel read outside field[t].
 * uncovered (n, int32; may be NULL): uncovered[t] = the number of nodes of out[t] whose source position ix = unnormalize(out.x, w0),
 * iy = unnormalize(out.y, h0) (the warps' fp32 un-normalisation, `align_corners` theirs) does not satisfy margin <= ix <= w0-1-margin and
 * margin <= iy <= h0-1-margin (margin 0: the bilinear warp's 4 taps inside; 1: the bicubic warp's 16; NaN is not covered): pws_border_keep's
 * rule, taken at the field's nodes.  Integer counts: the same on every run.  h0, w0, align_corners and margin are read only then.
 * Any fh, fw >= 2; n == 0 returns PWS_OK and launches nothing.  PWS_EINVAL: NULL field / coef / out, fh or fw < 2, h0 or w0 < 1 or
 * margin < 0 with `uncovered`, field or out not 8-byte aligned, out overlapping field (the same pointer included).  One launch (and a
 * 4 n byte clear of `uncovered`). */
int pws_field_zoom(const float *field, int n, int fh, int fw, const float *coef, float *out, int h0, int w0, int align_corners, int margin,
                   int *uncovered, pws_stream_t stream);

/* Rigid warp mode (csrc/field_rigid.hip; no counterpart in the reference).  pws_field_homography's M is the globally rigid version of the
 * correction a frame's field holds; this blends the field towards it, node by node, and the warp that follows is untouched.
 * field[n,fh,fw,2] -> out[n,fh,fw,2]; m[n,9] fp64 in DEVICE memory, exactly as pws_field_homography writes it: M maps a field value
 * (normalised source coordinates) to the output position u = 2x/w0 - 1, v = 2y/h0 - 1 (no half-pixel term).  For node (i, j) of frame t:
 *   x = j (w0-1)/(fw-1), y = i (h0-1)/(fh-1) (the frame pixel at which the warps' align_corners=True resize reads exactly this node);
 *   A = adj(M) (M^-1 up to scale: no division), (X, Y, D) = A (u, v, 1), Dc = A[2][2]; P = (X/D, Y/D), fp64, each rounded once to fp32.
 *   Frame t is FITTED when M's nine entries are finite, det M is finite and non-zero and Dc != 0.  A node of a fitted frame is VALID when
 *   D/Dc >= 2^-20: on the frame centre's side of the horizon, and not on it.
 *   (The float64 sums of products behind X, Y, D may be contracted into FMAs: against another float64 evaluation P agrees to one
 *   float32 ulp, and the horizon decision within a relative 2^-52 of the threshold.)
 *   A valid node gets P when rigidity == 1 (exactly the homography, not F + (P - F)), F itself when rigidity == 0, and
 *   fmaf(rigidity, P - F, F) per component otherwise
 *   (a NaN in F is healed at 1 and propagates below it); every other node, and every node of an unfitted frame, keeps F bit for bit.
 * unfit (n, int32; may be NULL): the nodes of frame t that kept F for that reason (fh * fw for an unfitted frame).
 * residual (n, fp32; may be NULL): the largest max(|Fx - Px| * (w0/2), |Fy - Py| * (h0/2)) -- fp32: one subtraction, one product -- over the
 * valid nodes of frame t whose F is finite, 0 without any: how far the field was from rigid, in source pixels.  An integer atomic max on the
 * bits of a non-negative float, and integer counts: the same on every run.  Both are cleared by the call.
 * The kernel is element-wise: out == field is allowed.  Any fh, fw >= 2; n == 0 returns PWS_OK, launches nothing and writes nothing.
 * PWS_EINVAL: NULL field / m / out, n < 0, fh or fw < 2, h0 or w0 < 1, rigidity outside [0, 1] or NaN, field / out / m not 8-byte
 * aligned, residual / unfit not 4-byte aligned, out overlapping field in part.  One launch (and a 4 n byte clear per statistic). */
int pws_field_rigid(const float *field, int n, int fh, int fw, const double *m, float rigidity, int h0, int w0, float *out, float *residual,
                    int *unfit, pws_stream_t stream);

/* Wobble suppression (csrc/field_wobble.hip; no counterpart in the reference).  The generator regresses every frame's field from that
 * frame's own window, and nothing ties the NON-RIGID part of consecutive fields together: the local, per-pixel part changes from frame to
 * frame, which reads as wobble.  This low-passes that part along time and leaves the rigid part -- the fitted homography -- as it is.
 * One call is ONE scene of n frames (the caller slices at its cuts).  field[n,fh,fw,2] -> out[n,fh,fw,2]; m[n,9] fp64 in device memory as
 * pws_field_homography writes it; (h0, w0) the frame; sigma in (0, 5] frames, the Gaussian's width.
 *   R = ceil(3 sigma) (fp64), 1 .. 15: the filter looks no further than the generator's own window of +-15 frames.
 *   g_k = exp(-k^2 / (2 sigma^2)), k = -R .. R, in fp64 on the host, each rounded to fp32; g_0 = 1.
 *   P[t] at node (i, j), and the notions FITTED (frame) and VALID (node), are pws_field_rigid's, word for word: the adjugate in fp64,
 *   D/Dc >= 2^-20, P rounded once to fp32 (the same device code: csrc/rigid_position.h).
 *   A (frame, node) pair is USABLE when the frame is fitted, the node is valid and both components of F are finite.
 *   For a usable pair E = F - P: one fp32 subtraction per component.
 *   A node that is not usable at t: out = F bit for bit, and the node counts in unfit[t] (a node with a NaN in F included).
 *   A node usable at t: S = sum g_k E[t+k] and W = sum g_k, both over the k, in ascending order, with 0 <= t+k < n and (t+k, node) usable;
 *   fp32: S by fmaf(g_k, E, S) per component from 0, W by plain additions from 0; W >= 1 since k = 0 counts.  out = P[t] + S / W (one
 *   IEEE division, one addition).  Frames outside the scene and unusable taps drop out of both sums: no reflection, no padding, and a
 *   scene of one frame returns float32(P + (F - P)).
 * removed (n, fp32; may be NULL): the largest max(|out_x - F_x| * (w0/2), |out_y - F_y| * (h0/2)) -- fp32: one subtraction, one product; a
 * NaN drops out -- over the usable nodes of frame t, 0 without any: how much the filter moved the field, in source pixels; the number
 * to choose sigma by.  unfit (n, int32; may be NULL) as above.  An integer atomic max on the bits of a non-negative float and integer
 * counts; the sums run in a fixed order and no floating-point atomic is used: the same bits on every run.  Both are cleared by the call.
 * The filter acts at fixed OUTPUT positions (field nodes), not along scene points: a real, fast change of parallax is smoothed too.
 * The kernel reads neighbouring frames, so it cannot run in place.  Its time segments are PWS_WOBBLE_SEGMENT output frames long.
 * Any fh, fw >= 2; n == 0 returns PWS_OK, launches nothing and writes nothing.  PWS_EINVAL: NULL field / m / out, n < 0, fh or fw < 2,
 * h0 or w0 < 1, sigma outside (0, 5] or NaN, field / out / m not 8-byte aligned, removed / unfit not 4-byte aligned, out overlapping
 * field (the same pointer included).  One launch (and a 4 n byte clear per statistic). */
#define PWS_WOBBLE_SEGMENT 32
int pws_field_wobble(const float *field, int n, int fh, int fw, const double *m, double sigma, int h0, int w0, float *out, float *removed,
                     int *unfit, pws_stream_t stream);

/* Scene-cut score for edited footage (csrc/scene.hip).  The reference clamps a frame's 31-plane window at the clip's first and last frame
 * only (main_new.py:627-633); the streaming stabiliser applies the same clamp at every hard cut, which it finds from the L1 distance of
 * block-wise histograms of consecutive window planes (motion-tolerant, unlike a pixel difference).
 * planes: (n, h, w) fp32 contiguous, nominally in [-1, 1] (window_planes).  h % 4 == 0, w % 4 == 0.
 * hist: (n, 16, 32) uint32 -- block (by*4+bx) of the 4 x 4 grid of (h/4) x (w/4) blocks, 32 bins: the bin of a sample v is 0 if
 *       !(x >= 0) with x = (v + 1.0f) * 16.0f in fp32 (NaN, anything below -1), else min(31, (int)x).
 * sad:  (n) uint32 -- sad[0] = 0, sad[t] = sum over the 512 counters |hist[t] - hist[t-1]|.
 * Integer arithmetic after the bin: exact, the same bits on every run.  planes and sad 4-byte aligned, hist 8-byte aligned. */
int pws_scene_change(const float *planes, int n, int h, int w, unsigned *hist, unsigned *sad, pws_stream_t stream);

/* Block motion between consecutive planes (csrc/motion.hip): the measurement behind the stability metric.  The generator regresses a warp
 * and never measures motion; this does, on the planes the stabiliser already keeps.
 * planes: (n, h, w) fp32 contiguous, nominally in [-1, 1] (window_planes).  radius R: 1 .. 16.
 * Samples are quantised once, q = min(255, max(0, floor((v + 1) * 127.5 + 0.5))) in fp32 with one rounding per step (no contraction), 0 for
 * NaN; everything after q is integer arithmetic: exact, the same bits on every run and under any schedule.
 * Blocks are 16 x 16: nby = (h - 2R) / 16, nbx = (w - 2R) / 16 (both >= 1), block (by, bx) has its top-left at (R + 16 by, R + 16 bx); a
 * remainder strip is not covered.  For t >= 1 and every block, S(dx, dy) = sum over the block of |q[t][y, x] - q[t-1][y + dy, x + dx]|, dx and
 * dy in [-R, R] (the block of the current frame is searched in the previous one); the best candidate minimises S * 2048 + rank, rank = the
 * candidate's position in the order sorted by (dx^2 + dy^2, dy, dx): ties go to the shorter vector, and a flat block gets (0, 0).
 * mv:       (n, nby, nbx, 2) int16 = (dx, dy).
 * sad:      (n, nby, nbx, 5) int32 = S at the best candidate and at its x-1, x+1, y-1, y+1 neighbours; -1 for a neighbour outside the range.
 * activity: (n, nby, nbx) int32 = sum over the block of |q[y, x+1] - q[y, x]| (16 x 15 pairs) + |q[y+1, x] - q[y, x]| (15 x 16 pairs), every
 *           frame, frame 0 included.
 * Row 0 of mv and sad is zero.  n == 0 returns PWS_OK and launches nothing.  PWS_EINVAL: a bad shape, a radius outside 1 .. 16, a plane
 * without a block, more than 2^20 blocks, a NULL pointer, a pointer that is not 4-byte aligned.  One launch (per 32768 frames). */
int pws_block_motion(const float *planes, int n, int h, int w, int radius, short *mv, int *sad, int *activity, pws_stream_t stream);

/* The similarity that the block vectors of each frame pair agree on, in fp64 (csrc/motion.hip).  mv, sad, activity: as pws_block_motion
 * wrote them for (n, h, w) planes and this radius.
 * A block is VALID if activity[t] >= min_activity, |dx| < R and |dy| < R (a best match on the rim of the search range means the motion
 * lies outside it), and the match is sharp: 2 ((l - 2c + h)_x + (l - 2c + h)_y) >= activity[t], in integers.  Around a true match S rises
 * like the block's summed gradient, so the two second differences together reach about the activity; a block whose content is not in the
 * window (motion beyond the range) settles on a chance match, around which S is flat (measured 0.10 .. 0.41 of the activity on noise, against
 * 0.95 .. 2.2 at true matches).  Its sub-pixel vector d adds, per axis, off = 0.5 (l - h) / (l - 2c + h) from S at the best candidate (c) and its two
 * neighbours (l, h) when both exist, the denominator is positive and c > 0 (an exact match keeps its whole-pixel vector), else 0, clipped
 * to +-0.5.
 * A block centre p, relative to the plane centre ((w-1)/2, (h-1)/2), maps to p + d in the previous frame; p' = [[a, -b], [b, a]] p + (tx, ty)
 * is fitted by least squares (the 4 x 4 normal system, solved in closed form).  Three rounds: round 0 uses all valid blocks; rounds 1 and 2
 * the valid blocks whose squared residual under the previous round's fit is at most max(1.0, 4 * the mean squared residual of the blocks
 * that round used).  Fewer than 8 blocks in any round: a NaN row with inliers 0.
 * motion:  (n, 4) fp64 = (a, b, tx, ty), in plane pixels.   inliers: (n) int32, the blocks of the last round.
 * Row 0 is (1, 0, 0, 0) with inliers 0.  The sums are taken in one fixed order: the same bits on every run.
 * PWS_EINVAL: as pws_block_motion, and motion not 8-byte aligned.  One launch. */
int pws_motion_fit(const short *mv, const int *sad, const int *activity, int n, int h, int w, int radius, int min_activity, double *motion,
                   int *inliers, pws_stream_t stream);

/* pws_motion_fit in FRAME pixels (csrc/motion.hip).  The planes are a resize of the frame, non-uniform unless the source is square: a
 * rotation of a 16:9 frame is no similarity between its 256 x 256 planes, and the plane-space fit mis-reads it.  (sx, sy) = frame pixels per
 * plane pixel, (W0 / w, H0 / h): every block centre p and every sub-pixel vector d is multiplied by (sx, sy), component by component, before
 * the normal sums; the fit, the residuals and motion = (a, b, tx, ty) are then in frame pixels, relative to the frame centre.  The outlier
 * threshold's floor, one squared plane pixel, becomes sx * sy: max(sx * sy, 4 * the mean squared residual).  Validity, the three rounds, the
 * summation order and the NaN rule are pws_motion_fit's.  A product with 1.0 is exact: (1, 1) returns pws_motion_fit's bits.
 * PWS_EINVAL: as pws_motion_fit, and sx or sy not in (0, 1e6] (NaN included).  One launch. */
int pws_motion_fit_scaled(const short *mv, const int *sad, const int *activity, int n, int h, int w, int radius, int min_activity, double sx,
                          double sy, double *motion, int *inliers, pws_stream_t stream);

/* Path smoothing (csrc/path_smooth.hip; no counterpart in the reference): the camera path of ONE scene of n frames from its per-pair
 * motion, the path's Gaussian low-pass, and per frame the correction from the measured path to the smooth one.  All fp64, in DEVICE
 * memory, no synchronisation.
 * motion: (n, 4) = (a, b, tx, ty) as pws_motion_fit[_scaled] writes it: row k maps a point of frame k to frame k-1.  Row 0 is not read; a
 *   row with an entry that is not finite counts as (1, 0, 0, 0).
 * path:   (n, 4) = P[k] = (lambda, theta, cx, cy), the pose C_k = C_{k-1} o motion[k] of frame k in frame 0's coordinates: P[0] = 0 and, with
 *   s = exp(lambda[k-1]), c = cos(theta[k-1]), sn = sin(theta[k-1]):  cx[k] = cx[k-1] + s (c tx - sn ty),  cy[k] = cy[k-1] + s (sn tx + c ty),
 *   lambda[k] = lambda[k-1] + log(hypot(a, b)),  theta[k] = theta[k-1] + atan2(b, a).
 * Smoothing: Re = min(ceil(3 sigma), n-1), g(j) = exp(-0.5 (j / sigma)^2), P^[k] = (sum_{j=-Re..Re} g(j) P*(k+j)) / (sum_j g(j)), both sums in
 *   ascending j, per component; P*(i) = P[i] inside the scene, 2 P[0] - P[-i] before it, 2 P[n-1] - P[2(n-1) - i] behind it (odd reflection:
 *   a constant velocity is its own average at every frame, the ends included).
 * d:      (n, 6) = D[k] = C_k^-1 o C^_k, row-major 2 x 3: the linear part exp(lambda^ - lambda) Rot(theta^ - theta), the translation
 *   exp(-lambda) Rot(-theta) (c^ - c).  It maps a position of the smoothed frame to the position of the measured frame that shows the same
 *   point, both relative to the frame centre, in the pixels of `motion` (pws_field_compose takes it as it is).
 * Products and sums are rounded once each, in one fixed order: the same bits on every run.  n == 1 gives the identity; n == 0 returns
 * PWS_OK and launches nothing.  PWS_EINVAL: n < 0 or above 2^24, sigma outside (0, 256] (NaN included), a NULL pointer, a pointer that is
 * not 8-byte aligned.  motion, path and d must not overlap.  One launch of one workgroup (the scan is sequential). */
int pws_path_smooth(const double *motion, int n, double sigma, double *path, double *d, pws_stream_t stream);

/* The L1-optimal camera path (csrc/path_l1.hip; Grundmann, Kwatra, Essa, "Auto-directed video stabilization with robust L1 optimal camera
 * paths", CVPR 2011; OpenCV videostab's LpMotionStabilizer; no counterpart in the reference): pws_path_smooth with another path model.  ONE
 * scene of n frames; all fp64, in DEVICE memory except `bound` and `weights`, which are read on the host; no synchronisation.
 * motion, path: as for pws_path_smooth -- the same scan (csrc/path_pose.h), the same rule for a row that is not finite, the same bits.
 * bound:   4 half-widths b > 0 of the box |P^ - P| <= b, per component (lambda, theta, cx, cy).  stream.optimal_path forms them from
 *   reach = c in (0, 0.5], the share of an H x W frame per axis that the path may move away from the measured one:
 *   b = (-log(1 - c), c min(H, W) / max(H, W), c W / 2, c H / 2).  Each half-width alone spends the whole share; their combination is no
 *   coverage guarantee (pws_path_limit is the coverage rule).  The default c = 0.1 is a judgement that no footage here can fit.
 * weights: (w1, w2, w3), each finite and > 0; the paper's (10, 1, 100) are the default of stream.optimal_path.
 * Problem, per component, the four independent: with x = (P^ - P) / b and q = P / b,
 *     minimise  w1 |D1 (x + q)|_1 + w2 |D2 (x + q)|_1 + w3 |D3 (x + q)|_1   subject to  -1 <= x <= 1,
 *   D_k the k-th forward difference, n - k rows: (D1 y)[j] = y[j+1] - y[j], (D2 y)[j] = (y[j] - 2 y[j+1]) + y[j+2],
 *   (D3 y)[j] = ((y[j+3] - 3 y[j+2]) + 3 y[j+1]) - y[j].  The minimiser is made of static, constant-velocity and constant-acceleration
 *   pieces.  n <= 3: P^ = P, D is the identity (1, 0, 0, 0, 1, 0) exactly, info = (0, 0, 0, 1).
 * Solver: the LP with slack variables e_k >= |D_k (x + q)|, m = 8 n - 12 constraints  e_k -+ D_k (x + q) >= 0, 1 -+ x >= 0, by a primal-dual
 *   interior-point method.  Every constraint keeps its slack s > 0 and its multiplier l > 0 as state.
 *   Start: x = 0, e_k = |D_k q| + 1, s+ = e_k - D_k q, s- = e_k + D_k q, s = 1 for the box, every l = 1 / s.
 *   Per step: eta = s . l, f = sum_k w_k sum_j e_k[j], the dual residual r = (sum_k D_k^T (l+_k - l-_k) + lU - lL; w_k - l+_k - l-_k).
 *   Stop, converged, when eta <= 1e-9 max(1, f) and |r|_2 <= 1e-9 max(1, max w); stop after 64 steps.  Otherwise t = 10 m / max(eta, 1e-9
 *   max(1, f)) -- 10 m / eta until the gap's criterion is met, held from there on, see below -- and with
 *   g = l / s and v = 1 / (t s) per constraint, G = g+ + g-, be = (v+ + v-) - w_k:  the slacks' elimination leaves the SPD band
 *     (sum_k D_k^T Theta_k D_k + diag(gU + gL)) dx = (vL - vU) - sum_k D_k^T ((v+ - v-) + (g- - g+) be / G),   Theta = 4 g+ g- / G,
 *   three sub-diagonals wide, solved by LDL^T without pivoting; then a = D_k dx, de = (be + (g+ - g-) a) / G, ds+ = de - a, ds- = de + a,
 *   dl = (v - l) - g ds for every constraint (dsU = -dx, dsL = dx).  The step is alpha = min(1, 0.99 min over ds < 0 of s / -ds and over
 *   dl < 0 of l / -dl) on x, e, s and l alike: every iterate is strictly feasible.
 *   Skipped pivots: where the optimum is not unique (a static path anywhere inside the box) the band becomes singular to working precision
 *   as the iteration converges, and a pivot falls below the rounding of its own sum.  A pivot D_i that is not above 2^-44 A_ii is replaced
 *   by 1e128, which leaves dx_i = 0 for that step (S. Wright, "Modified Cholesky factorizations in interior-point algorithms for linear
 *   programming", SIAM J. Optim. 9, 1999).  The case on record: a constant path, n = 40, stops unconverged at eta = 1.5e-5 after 11 steps
 *   without the rule and converges in 16 with it; the cases with a unique optimum never meet it.
 *   Held t: while t grows with every step the band's conditioning (1e14 and more) keeps |r|_2 at a rounding floor, which at n = 200 and
 *   w = 100 is 1e-7 .. 3e-7, the criterion's own size: a random walk plus pan plus sine of 200 frames in a box of 20 px then stops after 40
 *   steps, or runs out of its 64, as the order of the sums falls.  A step at the t that met the gap's criterion only centres; its dx tends
 *   to 0 and the rounding with it, and |r|_2 falls to 1e-9 and below in one or two steps (that case: 32 steps in every order).
 *   On record: a shaky pan of 2 048 frames leaves two components at 64 steps, eta = 2e-5 .. 6e-5, converged = 0: short steps, a valid path
 *   within 2e-6 of the optimum.  No residual backtracking is built: it shortens steps and would not help there.
 *   Breakdown: a pivot or a step that is not finite ends the iteration, and the last iterate stands -- a valid path, since every iterate
 *   is feasible.  x is clamped to [-1, 1] at the end, and P^ - P = b x: |P^ - P| <= b holds exactly.
 * d:      (n, 6) = D[k] = C_k^-1 o C^_k as for pws_path_smooth, from P and P^ - P.
 * info:   (4, 4): per component (Newton steps taken, the final eta, the final f, converged 1 / 0).
 * workspace: pws_l1_path_workspace(n) bytes (144 doubles per frame: P^ - P, and per component the solver's state), 8-byte aligned.  Its
 *   contents on return are not defined.
 * Every sum -- eta, f, |r|^2 -- is taken in one fixed order (thread i mod 256 adds its frames in ascending order, then the 256 partial sums
 * are halved), every band entry sums its at most 9 terms in a fixed order, the step length is a min: the same bits on every run, no
 * atomics.  n == 0 returns PWS_OK and launches nothing.  PWS_EINVAL: n < 0 or above 65 536 (the band solve is sequential: one lane), a
 * bound or weight that is not finite and > 0, a NULL pointer, a pointer that is not 8-byte aligned, a workspace that is too small.  motion,
 * path, d, info and workspace must not overlap.  Three launches: the scan on one lane, the solver (one workgroup of 256 threads per
 * component), D over frames. */
size_t pws_l1_path_workspace(int n);
int pws_l1_path(const double *motion, int n, const double *bound, const double *weights, double *path, double *d, double *info,
                void *workspace, size_t workspace_bytes, pws_stream_t stream);

/* Field composition (csrc/field_compose.hip; no counterpart in the reference): a per-frame affine correction of the OUTPUT frame folded
 * into the warp field; the warp that follows is untouched and still resamples the source once.
 * field[n,fh,fw,2] -> out[n,fh,fw,2]; d[n,6] fp64 in DEVICE memory = D of frame t, row-major 2 x 3, in frame pixels relative to the frame
 * centre ((w0-1)/2, (h0-1)/2), as pws_path_smooth writes it.  For node (i, j) of frame t, in fp64:
 *   x = j (w0-1)/(fw-1) - (w0-1)/2, y = i (h0-1)/(fh-1) - (h0-1)/2 (the frame pixel at which the warps' align_corners=True resize reads
 *   exactly this node); x' = d0 x + d1 y + d2, y' = d3 x + d4 y + d5; sx = (x' + (w0-1)/2) (fw-1)/(w0-1), sy alike, each rounded ONCE to fp32.
 *   x0 = clamp(floor(sx), 0, fw-2), lx = sx - x0 (fp32, NOT clamped), hx = 1 - lx; y0, ly, hy alike;
 *   out[t,i,j,c] = fma(ly, fma(lx, F[y0+1,x0+1], hx * F[y0+1,x0]), hy * fma(lx, F[y0,x0+1], hx * F[y0,x0])) (the warps' field interpolation).
 *   Outside the lattice the field is continued linearly from its rim cell: an affine field composes exactly, and the wedges the
 *   correction opens reach the warp as out-of-range coordinates rather than as a smeared rim.
 * A frame whose six coefficients are exactly (1, 0, 0, 0, 1, 0) is copied bit for bit; a node whose sx or sy is not finite (NaN or
 * overflowing coefficients) keeps F[i,j].  floor(sx) is bounded as a float before it becomes an integer: no d can make the kernel read
 * outside field[t].
 * uncovered (n, int32; may be NULL): pws_field_zoom's count, rule and clearing, on out[t].  align_corners and margin are read only then.
 * Any fh, fw >= 2; n == 0 returns PWS_OK and launches nothing.  PWS_EINVAL: NULL field / d / out, fh or fw < 2, h0 or w0 < 2, margin < 0
 * with `uncovered`, field / out / d not 8-byte aligned, out overlapping field (the same pointer included).  One launch (and a 4 n byte
 * clear of `uncovered`). */
int pws_field_compose(const float *field, int n, int fh, int fw, const double *d, float *out, int h0, int w0, int align_corners, int margin,
                      int *uncovered, pws_stream_t stream);

/* Rolling-shutter rates (csrc/path_smooth.hip; no counterpart in the reference): per frame of ONE scene of n frames the camera's velocity
 * in that frame's own coordinates, per frame interval, from the scene's per-pair motion.  All fp64, in DEVICE memory, no synchronisation.
 * motion: (n, 4) = (a, b, tx, ty) as for pws_path_smooth: row k maps a point of frame k to frame k-1.  Row 0 is not read; a row with an
 *   entry that is not finite counts as (1, 0, 0, 0).
 * rates:  (n, 2, 4) = (ldot, wdot, xdot, ydot) -- log scale, angle, translation -- twice per frame k:
 *   rates[k][0], forward, from motion[k+1]:  (log hypot(a, b), atan2(b, a), tx, ty);
 *   rates[k][1], backward, from motion[k], with s = hypot(a, b), f = atan2(b, a):
 *     (log s, f, (cos f * tx + sin f * ty) / s, (-sin f * tx + cos f * ty) / s) -- the same velocity in frame k's coordinates instead of
 *     frame k-1's.
 *   The scene's first frame takes its forward row as its backward row, its last frame its backward row as its forward row; n == 1 gives
 *   zeros.  Rates never cross a scene cut: call once per scene.
 * Every product and sum is rounded once, nothing is summed across threads: the same bits on every run.  n == 0 returns PWS_OK and
 * launches nothing.  PWS_EINVAL: n < 0 or above 2^24, a NULL pointer, a pointer that is not 8-byte aligned.  motion and rates must not
 * overlap.  One launch. */
int pws_shutter_rates(const double *motion, int n, double *rates, pws_stream_t stream);

/* pws_field_compose with a rolling-shutter correction that depends on the row (csrc/field_compose.hip; no counterpart in the reference).
 * r in [-1, 1] is the share of the frame interval that the sensor's readout takes from the top row to the bottom row (negative: bottom
 * to top); rates[n,2,4] fp64 in DEVICE memory as pws_shutter_rates writes them.  For node (i, j) of frame t, in fp64:
 *   p0 = D q, exactly as pws_field_compose computes (x', y'): the global-shutter answer, relative to the frame centre;
 *   delta = r * clamp(p0.y / (h0-1), -1/2, 1/2), the time offset of the row that p0 lies on, in frame intervals;
 *   (ldot, wdot, xdot, ydot) = rates[t][0] if delta >= 0, else rates[t][1];
 *   p = p0 - delta * (ldot * p0 + wdot * (-p0.y, p0.x) + (xdot, ydot)): the camera's velocity field times the row's time offset, taken out.
 * sx = (p.x + (w0-1)/2) (fw-1)/(w0-1), sy alike, each rounded ONCE to fp32; the cell, lx / ly (not clamped), the interpolation, the linear
 * continuation, the rule for sx or sy that is not finite and `uncovered` are pws_field_compose's.
 * Deliberate approximations: the row's time is taken from p0 (no fixed-point iteration); the model is first order in delta (exact for a
 * translation; at |delta| <= 1/2 and 0.01 rad per frame the second-order term stays below 0.01 pixel at 720p); the path is linear between
 * frames.  The row is that of the frame the motion was measured on.
 * A frame is copied bit for bit only if its D is exactly the identity AND (r == 0 or all eight of its rates are zero): a steady pan has
 * D = I and is still unskewed.  r == 0 launches pws_field_compose's kernel, and all-zero rates give its bits.
 * PWS_EINVAL: as pws_field_compose; r outside [-1, 1] (NaN included); with n > 0, rates NULL or not 8-byte aligned.  n == 0 returns PWS_OK
 * and launches nothing.  One launch (and a 4 n byte clear of `uncovered`). */
int pws_field_compose_rows(const float *field, int n, int fh, int fw, const double *d, const double *rates, double r, float *out, int h0, int w0,
                           int align_corners, int margin, int *uncovered, pws_stream_t stream);

/* Rolling-shutter estimate, step 1 (csrc/shutter_estimate.hip; no counterpart in the reference): per pair of ONE scene of n frames what
 * the pair's block vectors say about r, the share of the frame interval that the readout takes from the top row to the bottom row (signed).
 * All in DEVICE memory, no synchronisation.
 * mv, sad, activity: the scene's rows as pws_block_motion wrote them for (n, h, w) planes and this radius.  motion (n, 4) as
 *   pws_motion_fit[_scaled] returned it for these blocks with this min_activity and (sx, sy); rates (n, 2, 4) as pws_shutter_rates returns
 *   it for this scene.  (sx, sy): the pixel scale of the fit, (1, 1) for pws_motion_fit.  h0: the frame height in motion's pixels (h at
 *   scale 1, the frame's own height for the scaled fit).
 * Pair k is USABLE when 2 <= k <= n - 2 and rows k-1, k, k+1 of motion are finite: both velocity differences below then come from real
 *   pairs, never from a scene end's duplicated rate.  Every other pair writes a zero row.
 * Blocks: those that pass pws_motion_fit's validity rule (one shared device function, csrc/motion_blocks.h), each with its centre p = (x, y)
 *   relative to the centre and its sub-pixel vector v, both times (sx, sy).  Fewer than 8: a zero row.  With f = (motion[k][0] - 1,
 *   motion[k][1..3]) and res2 pws_motion_fit's squared residual, the KEPT blocks are those with res2 <= max(sx sy, 4 * the mean of res2 over
 *   the valid blocks): the rule of the fit's own rounds.  Fewer than 8 kept blocks, or centres that span no area: a zero row.
 * Per kept block: c = clamp(y / (h0 - 1), -1/2, 1/2); (dl, dw, dx, dy) = rates[k][s] - rates[k-1][s] with s = 0 where c >= 0, else 1;
 *   z = c (dl p + dw (-y, x) + (dx, dy)), as (c * ((dl x - dw y) + dx), c * ((dl y + dw x) + dy)).
 *   e = v - (the least-squares similarity fitted to v over the kept blocks), z_perp = z - (the one fitted to z): pws_motion_fit's closed
 *   form, a block's residual taken as u - ((a1 x - b y) + tx), u' - ((b x + a1 y) + ty).
 * terms: (n, 4) fp64; terms[k] = (sum e . z_perp, sum z_perp . z_perp, sum e . e, the number of kept blocks).
 * Every product and sum is rounded once; the sums are pws_motion_fit's: a lane's blocks in index order, then a fixed butterfly.  The same
 * bits on every run; no atomics.  n == 0 returns PWS_OK and launches nothing; n < 4 writes zero rows.  PWS_EINVAL: as pws_motion_fit_scaled;
 * h0 outside (1, 1e9] (NaN included); n above 2^24; motion, rates or terms not 8-byte aligned.  One launch, one workgroup per pair. */
int pws_shutter_terms(const short *mv, const int *sad, const int *activity, const double *motion, const double *rates, int n, int h, int w,
                      int radius, int min_activity, double sx, double sy, double h0, double *terms, pws_stream_t stream);

/* Rolling-shutter estimate, step 2 (csrc/shutter_estimate.hip): the clip's estimate from the terms of all its pairs (every scene's rows, n in
 * all).  N, D, E, cnt = the four column sums over the rows in index order; m = the rows whose count is positive.
 * out4: (4) fp64 = (r_hat, se, D, cnt), r_hat = N / D, se = sqrt(max(0, E - r_hat N) / (2 cnt - 4 m - 1) / D); (NaN, +inf, D, cnt) when D or
 *   the degrees of freedom 2 cnt - 4 m - 1 are not positive (n == 0 included).
 * se is the least-squares standard error under independent, unbiased block errors.  The real errors -- a first-order model, correlated
 * sub-pixel bias -- are systematic and several times larger: se tells a clip with information from one without (a tripod, a steady pan);
 * it is NOT an error bar.  PWS_EINVAL: n < 0 or above 2^24, NULL out4 (terms with n > 0), a pointer that is not 8-byte aligned.  One launch
 * of one workgroup. */
int pws_shutter_estimate(const double *terms, int n, double *out4, pws_stream_t stream);

/* Crop-bounded smoothing, step 1 (csrc/path_limit.hip; no counterpart in the reference): the corrections of n frames scaled back to
 * levels + 1 shares of themselves.  All fp64, in DEVICE memory, no synchronisation.
 * d:     (n, 6) = D of frame t, row-major 2 x 3, as pws_path_smooth writes it: a SIMILARITY (d4 == d0, d1 == -d3).  Only d0, d3, d2, d5 are
 *   read for the levels in between; any other matrix is replaced there by the similarity those four entries give.
 * table: (n, levels+1, 6); table[t, l] = D_t(l / levels).  For a row whose six entries are finite, with ls = log(hypot(d0, d3)) and
 *   phi = atan2(d3, d0), D(lam) has the linear part exp(lam ls) Rot(lam phi) and the translation lam (d2, d5):
 *   s = exp(lam * ls), c = cos(lam * phi), sn = sin(lam * phi);  D(lam) = (s c, 0 - s sn, lam d2, s sn, s c, lam d5),
 *   every product and sum rounded once.  Level 0 is exactly (1, 0, 0, 0, 1, 0); level `levels` is the row of d verbatim.  A row with an entry
 *   that is not finite is copied to every level, level 0 included (pws_field_compose keeps such frames' nodes).
 * Nothing is summed across threads: the same bits on every run.  n == 0 returns PWS_OK and launches nothing.  PWS_EINVAL: n < 0 or above
 * 2^24, levels outside 1 .. 64, a NULL pointer, a pointer that is not 8-byte aligned.  d and table must not overlap.  One launch. */
int pws_path_levels(const double *d, int n, int levels, double *table, pws_stream_t stream);

/* Crop-bounded smoothing, step 2 (csrc/field_reach.hip; no counterpart in the reference): per frame and level, how many nodes of a
 * rectangle of the lattice would sample outside the source if the field were composed with that level's correction.
 * field[n,fh,fw,2] fp32; table[n,levels+1,6] fp64 as pws_path_levels writes it (any finite or non-finite 2 x 3 rows are accepted);
 * counts[n,levels+1] int32; all in DEVICE memory.  counts[t, l] = the number of nodes (i, j) with i0 <= i <= i1 and j0 <= j <= j1 for
 * which the value that pws_field_compose would write at that node of frame t for D = table[t, l] -- with rates != NULL and r != 0: the
 * value that pws_field_compose_rows would write, rates[n,2,4] and r as there -- is uncovered by pws_field_zoom's rule: the warps' fp32
 * un-normalisation with `align_corners`, margin <= ix <= w0-1-margin and margin <= iy <= h0-1-margin, NaN not covered.  The value is
 * computed by the function that pws_field_compose's kernel calls (csrc/compose_node.h) -- the fp64 position, the single rounding to fp32,
 * the cell clamp, the unclamped lx / ly, the fma chain, the linear continuation, the rule for positions that are not finite, the copy of
 * an identity level -- and is never stored.  levels == 0 with a one-entry table counts one correction per frame.
 * counts is cleared by the call; the integer counts are summed per workgroup and added with integer atomics: the same on every run.  The
 * cell is bounded as a float before it becomes an integer and the rectangle is checked against the lattice: no table, rectangle or
 * field value can make the kernel read outside field[t].
 * Any fh, fw >= 2; n == 0 returns PWS_OK and launches nothing.  PWS_EINVAL: NULL field / table / counts, fh or fw < 2, h0 or w0 < 2,
 * margin < 0, levels outside 0 .. 64, r outside [-1, 1] (NaN included), a rectangle that is empty (i1 < i0 or j1 < j0) or leaves the
 * lattice (i0 < 0, i1 > fh-1, j0 < 0, j1 > fw-1), field / table / rates not 8-byte aligned, counts not 4-byte aligned.  One launch and a
 * 4 n (levels+1) byte clear of `counts`. */
int pws_field_reach(const float *field, int n, int fh, int fw, const double *table, int levels, const double *rates, double r, int i0, int i1,
                    int j0, int j1, int h0, int w0, int align_corners, int margin, int *counts, pws_stream_t stream);

/* Crop-bounded smoothing, step 3 (csrc/path_limit.hip; no counterpart in the reference): from pws_field_reach's counts the share of its
 * correction that each frame of ONE scene of n frames can take, eased over time, and the corrections scaled to it.  DEVICE memory, no
 * synchronisation.  d (n, 6) fp64 and counts (n, levels+1) int32 as above.
 * need:     (n) int32; need[t] = the largest l such that counts[t, l'] == 0 for every l' <= l (the prefix rule: every smaller level is
 *   feasible too), -1 if counts[t, 0] > 0 (the field alone does not cover the rectangle).  A row of d that is not finite: need[t] = levels.
 * strength: (n) fp64; with s[t] = max(need[t], 0) / levels, the largest sequence with strength[t] <= s[t] and |strength[t] -
 *   strength[t-1]| <= relax: a forward sweep strength[t] = min(s[t], strength[t-1] + relax), then the same sweep backward.
 * d_out:    (n, 6) fp64; d[t] verbatim when strength[t] == 1.0, otherwise D_t(strength[t]) by pws_path_levels' formulas (exactly the
 *   identity at 0; a row that is not finite is copied).
 * strength[t] lies between grid levels after the sweeps, where the counts say nothing: count again with pws_field_reach(levels = 0).
 * Strengths never relax across a scene cut: call once per scene.  One fixed order: the same bits on every run.  n == 0 returns PWS_OK
 * and launches nothing.  PWS_EINVAL: n < 0 or above 2^24, levels outside 1 .. 64, relax outside (0, 1] (NaN included), a NULL pointer, d /
 * strength / d_out not 8-byte aligned, counts / need not 4-byte aligned.  d_out must not overlap d.  One launch of one workgroup (the
 * sweeps are sequential). */
int pws_path_limit(const double *d, const int *counts, int n, int levels, double relax, int *need, double *strength, double *d_out,
                   pws_stream_t stream);

/* Deblurring (csrc/deblur.hip; no counterpart in the reference; OpenCV videostab's WeightingDeblurer with bilinear donors): a blurred SOURCE
 * frame borrows detail from the sharper frames of its scene around it, aligned by the clip's global motion, before the warp reads it.
 * Three steps -- sharpness, plan, blend -- all in DEVICE memory, no synchronisation.  tests/deblur_ref.py restates them.
 *
 * Sharpness.  S[t] = sum over the interior 1 <= x <= w-2, 1 <= y <= h-2 of (I[y,x+1] - I[y,x-1])^2 + (I[y+1,x] - I[y-1,x])^2, with I an
 * integer intensity, accumulated in 64-bit integers into sharpness (n) int64, which the entry zeroes itself.  Exact integer arithmetic:
 * workgroup partials are added with vector 64-bit atomics, and the result does not depend on their order -- the same bits on every run.
 *   pws_frame_sharpness_u8:  frames (n, h, w, 3) bytes, I = (29 c0 + 150 c1 + 77 c2 + 128) >> 8 (BGR order; rgb != 0 swaps the 29 and the 77).
 *   pws_plane_sharpness_u8:  a plane of h x w bytes per frame, frame t at planes + t * frame_stride (in samples; the Y plane of a packed
 *     frame with its packed size as the stride), I = the byte.
 *   pws_plane_sharpness_u16: the same for 16-bit words; layout 0: I = word >> 6 (P010, P210), 1: I = min(word, 1023) (I010, I210, I410).
 * h, w >= 3.  n == 0 returns PWS_OK and launches nothing.  PWS_EINVAL: n < 0 or above 65535, h or w below 3, h w >= 2^31, a stride smaller
 * than the plane, a layout other than 0 / 1, a NULL pointer, sharpness not 8-byte aligned, 16-bit planes or their stride not 2-byte
 * aligned.  One memset and one launch. */
int pws_frame_sharpness_u8(const unsigned char *frames_hwc, int n, int h, int w, int rgb, long long *sharpness, pws_stream_t stream);
int pws_plane_sharpness_u8(const unsigned char *planes, size_t frame_stride, int n, int h, int w, long long *sharpness, pws_stream_t stream);
int pws_plane_sharpness_u16(const unsigned short *planes, size_t frame_stride, int n, int h, int w, int layout, long long *sharpness,
                            pws_stream_t stream);

/* The deblurring plan of ONE scene of n frames (call once per scene, as pws_path_smooth).
 * motion:    (n, 4) fp64 = (a, b, tx, ty) as pws_motion_fit_scaled writes it: row k maps a position of frame k, relative to the frame centre
 *   ((w-1)/2, (h-1)/2) and in frame pixels, to frame k-1: p' = [[a, -b], [b, a]] p + (tx, ty).  Row 0 is not read.
 * sharpness: (n) int64, S as above.     radius: R = 1 .. 15.
 * maps:      (n, 2R+1, 6) fp64, row-major 2 x 3: maps[t, R+k] takes a centred position of frame t to frame t+k.  Column R is the identity.
 *   Both chains are walked OUTWARD from t, one step per column, C_j = step_j o C_{j-1} with C_0 the identity: to the past step_j = motion[t-j+1]
 *   (so that C_j = motion[t-j+1] o ... o motion[t]); to the future step_j = motion[t+j]^-1 = (ia, ib, -(ia tx + ib ty); -ib, ia, ib tx - ia ty)
 *   with d = a a + b b, ia = a / d, ib = b / d.  A composition is l = s0 c0 + s1 c3, ..., the translation (s0 c2 + s1 c5) + s2; every product
 *   and every sum is rounded once, in this order.
 * A chain stops at the scene's ends, and at the first step whose motion row is not finite or whose hypot(a, b) lies outside [0.5, 2]: from
 *   that column outward the map is NaN and the gain 0.  (Smoothing counts such a row as the identity; a donor that is not aligned is worse
 *   than none.)
 * gain:      (n, 2R+1) fp32: (float)(1 - (double)S[t] / (double)S[t+k]) where the chain reaches frame t+k and S[t+k] > S[t], else 0; column R is 0.
 * donors:    (n) int32, the gains of the row that are positive.
 * One fixed order: the same bits on every run.  n == 1 gives the identity and no donor; n == 0 returns PWS_OK and launches nothing.
 * PWS_EINVAL: n < 0 or above 2^24, radius outside 1 .. 15, a NULL pointer, motion / sharpness / maps not 8-byte aligned, gain / donors not
 * 4-byte aligned.  The outputs must not overlap the inputs.  Two launches. */
int pws_deblur_plan(const double *motion, const long long *sharpness, int n, int radius, double *maps, float *gain, int *donors,
                    pws_stream_t stream);

/* The deblurring blend.  frames: n consecutive SOURCE frames; maps (stop - start, 2R+1, 6) fp64 and gain (stop - start, 2R+1) fp32: the plan's
 * rows of frames [start, stop); out: stop - start frames of the frames' layout, not overlapping frames.  Every read is of `frames`, so calls
 * over [start, stop) pieces of a clip that is padded by R frames give the bytes of one call.  Per sample position p = (x, y) of frame t:
 *   acc = own sample(s), wsum = 1; then k = -R .. -1, 1 .. R in this order, only where gain[t, k] > 0 and 0 <= t+k < n:
 *   q = maps[t, k] (p - c) + c with c = ((w-1)/2, (h-1)/2), in fp64 as qx = (m0 dx + (m1 dy + m2)) + cx, qy = (m3 dx + (m4 dy + m5)) + cy, each
 *     product and sum rounded once; each coordinate is then rounded ONCE to fp32.  The donor counts only if 0 <= qx <= w-1 and
 *     0 <= qy <= h-1 on those fp32 values (NaN: no donor).
 *   The donor frame is sampled bilinearly in fp32 at x0 = clamp(floor(qx), 0, w-2), lx = qx - x0 (y alike): taps that hold one value give it.
 *   weight = gain s / (s + |I_q - I_0|), I the sample itself (planes) or (29 c0 + 150 c1 + 77 c2) / 256 of the own resp. the interpolated
 *     channels (3-byte pixels); s = sensitivity in 8-bit gray levels, times 4 for 16-bit planes (10-bit samples).
 *   acc += weight sample, wsum += weight.
 * The output is acc / wsum rounded to the NEAREST integer (ties to even) and clamped to the sample range 0 .. 255 resp. 0 .. 1023: a blend
 * of frames that truncated would come out half a level darker than the frames beside it that have no donor.
 *   pws_deblur_u8:        (n, h, w, 3) bytes; the three channels are blended with one weight.
 *   pws_deblur_plane_u8:  frames of `rows` rows of w bytes whose first h rows are the plane to blend: a packed YUV frame with its packed rows,
 *     whose LUMA is blended and whose chroma rows are copied from the frame's own source.  w % 4 == 0.
 *   pws_deblur_plane_u16: the same for 16-bit words; layout 0: the sample is word >> 6 and is written back << 6, 1: min(word, 1023).
 * A frame without a donor (no positive gain inside [0, n)) is copied word for word.  h, w >= 2.  start == stop returns PWS_OK and launches
 * nothing.  PWS_EINVAL: a bad shape or range, radius outside 1 .. 15, a sensitivity that is not finite and positive, w % 4 != 0 (planes),
 * rows < h, rows w (3 h w for pixels) >= 2^31, n above 65535, a NULL pointer, maps not 8-byte or gain not 4-byte aligned, frames / out not 4-byte
 * (u8 planes) resp. 8-byte (u16 planes) aligned.  One launch. */
int pws_deblur_u8(const unsigned char *frames_hwc, const double *maps, const float *gain, unsigned char *out, int n, int start, int stop,
                  int radius, int h, int w, double sensitivity, pws_stream_t stream);
int pws_deblur_plane_u8(const unsigned char *frames, const double *maps, const float *gain, unsigned char *out, int n, int start, int stop,
                        int radius, int rows, int h, int w, double sensitivity, pws_stream_t stream);
int pws_deblur_plane_u16(const unsigned short *frames, const double *maps, const float *gain, unsigned short *out, int n, int start, int stop,
                         int radius, int rows, int h, int w, int layout, double sensitivity, pws_stream_t stream);

/* Adam (no weight decay / amsgrad) on a flat fp32 buffer, in place; step counts from 1. */
int pws_adam_step(float *p, const float *g, float *m, float *v, size_t count, float lr, float beta1,
                  float beta2, float eps, int step, pws_stream_t stream);

/* The same update for `ntensors` tensors in one launch per 48 tensors (p, g, m, v, counts: HOST arrays of DEVICE pointers /
 * element counts): a generator has 92 tensors, most of them small. */
int pws_adam_step_multi(float *const *p, const float *const *g, float *const *m, float *const *v, const size_t *counts,
                        int ntensors, float lr, float beta1, float beta2, float eps, int step, pws_stream_t stream);

/* pws_adam_step / pws_adam_step_multi with the hyper-parameters as the DOUBLES the caller wrote (what optim.Adam calls).  torch's
 * formulation: m = beta1 m + (1 - beta1) g;  v = beta2 v + (1 - beta2) g^2;  p -= lr / (1 - beta1^step) * m / (sqrt(v) / sqrt(1 -
 * beta2^step) + eps).  The host rounds beta and 1 - beta to fp32 each on its own, and forms lr / (1 - beta1^step) and 1 / sqrt(1 -
 * beta2^step) in double; state and arithmetic on the device are fp32.  A float entry cannot do this: (float)0.999 no longer says what
 * 1 - 0.999 was (1.f - 0.999f = 0.99998713e-3 against 1.00000005e-3: 1.3e-5 of every v, 6e-6 of every update).  The float entries above
 * forward here with (double) of their arguments, which gives the kernels the scalars those entries always gave them.  Every element gets
 * the same roundings whether it is updated in a float4 or alone (a ragged tail, buffers that are not 16-byte aligned).  Same errors as the float entries (PWS_EINVAL: step < 1, a NULL
 * pointer with a non-zero count; pws_adam_step_d: buffers not 16-byte aligned with count > 256). */
int pws_adam_step_d(float *p, const float *g, float *m, float *v, size_t count, double lr, double beta1, double beta2, double eps,
                    int step, pws_stream_t stream);
int pws_adam_step_multi_d(float *const *p, const float *const *g, float *const *m, float *const *v, const size_t *counts, int ntensors,
                          double lr, double beta1, double beta2, double eps, int step, pws_stream_t stream);

/* ---------------------------------------------------------------- training objective around the path
 * The per-step losses the reference's train() wraps round netG + grid_sample (main_new.py:101-118,184-212;
 * lib/utils.py:246-255,339-362,405-447), generator part, no GAN; the VGG perceptual term stays with the caller (it gets
 * the warped frames and hands back a gradient through `gextra`).  All tensors carry m samples (the reference's two
 * forwards per item pair batched: branch 1 = samples [0,n), branch 2 = [n,2n)), fields [m,h,w,2], frames [m,3,h,w].
 * Sums are accumulated into caller-zeroed DOUBLE slot arrays of PWS_OBJ_SLOTS entries per quantity (one f64 atomic per
 * workgroup, spread over the slots); pws_objective_finalize reduces them. */
#define PWS_OBJ_SLOTS 64
/* images.float()*(1/255)*2-1 (lib/utils.py:247) for `per_sample` contiguous bytes of each of m samples; strides in elements */
int pws_u8_normalize(const unsigned char *src, size_t src_nstride, float *dst, size_t dst_nstride, int m, size_t per_sample,
                     pws_stream_t stream);
/* fake = grid_sample((src+1)*127.5, grid)/127.5 - 1 (main_new.py:106-107); src: 3 planes per sample, sample i at
 * src + i*src_nstride (a view of image_unstable[:, period+1 : period+4]).  target/l1_slots (both or neither):
 * l1_slots += sum|target - fake| (lib/utils.py:349), target sample i at target + i*tgt_nstride. */
int pws_warp_norm_fwd(const float *src, size_t src_nstride, const float *grid, float *fake, const float *target,
                      size_t tgt_nstride, double *l1_slots, int m, int h, int w, pws_stream_t stream);
/* `scale` in the backward entry points: nullable DEVICE pointer to one float that multiplies the host coefficient (the
 * upstream gradient of the loss, which autograd holds on the device: reading it there avoids a host synchronisation).
 * ggrid (=, or += when accumulate) (d fake/d grid)^T (c_l1*scale*sign(fake - target) + gextra); target, gextra nullable */
int pws_warp_norm_bwd(const float *src, size_t src_nstride, const float *grid, const float *target, size_t tgt_nstride,
                      float c_l1, const float *scale, const float *gextra, float *ggrid, int accumulate, int m, int h, int w,
                      pws_stream_t stream);
/* slots += sum|grid_sample(fake2, affine_grid(theta[n,6])) - fake1| (main_new.py:195-198); fake1, fake2: [n,3,h,w] */
int pws_temporal_l1_fwd(const float *fake1, const float *fake2, const float *theta, double *slots, int n, int h, int w,
                        pws_stream_t stream);
/* gfake1 -= c*sign(d) (plain read-modify-write), gfake2 += c*sign(d)*bilinear weights (atomics): both must be initialised */
int pws_temporal_l1_bwd(const float *fake1, const float *fake2, const float *theta, float c, const float *scale, float *gfake1,
                        float *gfake2, int n, int h, int w, pws_stream_t stream);
/* The same gradients without atomics: the scatter into gfake2 runs as an ordered gather (one lane per source pixel walks the output
 * pixels whose taps can hit it), so repeated runs are bit-identical.  scratch: n * 3 * h * w floats.  Slower (deterministic mode). */
int pws_temporal_l1_bwd_det(const float *fake1, const float *fake2, const float *theta, float c, const float *scale, float *gfake1,
                            float *gfake2, float *scratch, int n, int h, int w, pws_stream_t stream);
/* features [m,nf,6] = [stable x,y,1, unstable x,y,1] (lib/utils.py:225); slots += sum_k |unstable_k - grid[stable_k]|^2
 * with the reference's index int((coord+1)*size/2) (lib/utils.py:341-345) */
int pws_feature_loss_fwd(const float *grid, const float *features, double *slots, int m, int nf, int h, int w,
                         pws_stream_t stream);
/* ggrid += c * d(sum)/d grid (atomics; ggrid must be initialised) */
int pws_feature_loss_bwd(const float *grid, const float *features, float c, const float *scale, float *ggrid, int m, int nf,
                         int h, int w, pws_stream_t stream);
/* The same without atomics: one lane per sample adds its points in order (bit-identical runs; deterministic mode). */
int pws_feature_loss_bwd_det(const float *grid, const float *features, float c, const float *scale, float *ggrid, int m, int nf,
                             int h, int w, pws_stream_t stream);
/* slots_dx += sum|grid[:,:,1:]-grid[:,:,:-1]|, slots_dy likewise along h (lib/utils.py:351-357; reported, not optimised) */
int pws_field_smoothness(const float *grid, double *slots_dx, double *slots_dy, int m, int h, int w, pws_stream_t stream);
/* loss_pixel1 (lib/utils.py:405-425): fp64 L1 residual of the least-squares fit of generate_affine_matrix's bilinear
 * corner basis to every (size/block)^2-pixel block of resid [m,size,size,2]; requires size == block*block as the
 * reference's basis does.  bwd: gresid = c * d(sum)/d resid, overwritten. */
int pws_shape_loss_fwd(const float *resid, double *slots, int m, int size, int block, pws_stream_t stream);
int pws_shape_loss_bwd(const float *resid, double c, const float *scale, float *gresid, int m, int size, int block,
                       pws_stream_t stream);
/* out[j] = sum_q coef[j*nq+q] * (sum of the PWS_OBJ_SLOTS slots of quantity q), j < nout <= 64; slots [nq][PWS_OBJ_SLOTS],
 * coef [nout][nq] device doubles */
int pws_objective_finalize(const double *slots, int nq, const double *coef, int nout, float *out, pws_stream_t stream);

/* ---- VGG-16 perceptual term (lib/utils.py:11-32): the 13 conv3x3+ReLU layers run on pws_conv2d_fwd /
 * pws_conv2d_bwd_data (frozen weights: no weight gradient); these are the remaining pieces.  NHWC fp32. */
/* nn.MaxPool2d(2, 2): y[n,h/2,w/2,c]; h, w even, c % 4 == 0 */
int pws_maxpool2x2_fwd(const float *x, float *y, int n, int h, int w, int c, pws_stream_t stream);
/* dx (overwritten) = dy routed to the first maximum of each window in row-major scan order (ATen's argmax), 0 elsewhere */
int pws_maxpool2x2_bwd(const float *x, const float *dy, float *dx, int n, int h, int w, int c, pws_stream_t stream);
/* the same with the element type of x / y / dy / dx given by `store` (PWS_STORE_BF16: bf16 elements, c % 8 == 0) */
int pws_maxpool2x2_fwd_s(const void *x, void *y, int n, int h, int w, int c, int store, pws_stream_t stream);
/* relu_mask != 0 (bf16 storage only): x is a ReLU output and dx is the gradient wrt the pre-activation, dx *= (x > 0) */
int pws_maxpool2x2_bwd_s(const void *x, const void *dy, void *dx, int n, int h, int w, int c, int store, int relu_mask,
                         pws_stream_t stream);
/* nn.MSELoss pieces: slots[PWS_OBJ_SLOTS] (caller-zeroed doubles) += sum (a-b)^2 ;  ga = c * (*scale) * 2 (a-b) */
int pws_sqdiff_sum(const float *a, const float *b, size_t count, double *slots, pws_stream_t stream);
int pws_sqdiff_bwd(const float *a, const float *b, size_t count, float c, const float *scale, float *ga, pws_stream_t stream);

/* ---- training-mode BatchNorm2d + activation (the use_BN variant, lib/networks_cascading.py:253-341: conv -> BatchNorm2d ->
 * LeakyReLU / ReLU in every block), NHWC fp32 [pixels][c], any c.  ws: pws_bn_ws_bytes(c) bytes of scratch.
 * fwd: stats[2c] = (batch mean, 1/sqrt(biased var + eps)) saved for backward; y = act(gamma * xhat + beta); running_mean /
 *      running_var (nullable pair) updated `repeat` times with momentum and the UNBIASED variance, as torch does per call.
 * bwd: dy is overwritten by dz; dgamma / dbeta (nullable) are ACCUMULATED (a module used by several stages adds up).
 * pixels == 1 is refused like torch ("Expected more than 1 value per channel when training"). */
size_t pws_bn_ws_bytes(int c);
int pws_bn_train_fwd(const float *z, size_t pixels, int c, const float *gamma, const float *beta, int act, float *y, float *stats,
                     float *running_mean, float *running_var, float momentum, float eps, int repeat, void *ws, size_t ws_bytes,
                     pws_stream_t stream);
int pws_bn_train_bwd(float *dy, const float *y, const float *z, const float *stats, const float *gamma, int act, size_t pixels, int c,
                     float *dgamma, float *dbeta, void *ws, size_t ws_bytes, pws_stream_t stream);

/* ---------------------------------------------------------------- whole generator */
/* Floats needed for all 46 packed layer weights + 46 biases of a generator (input_nc, ngf). */
size_t pws_netg_packed_floats(int input_nc, int ngf);
/* params: HOST array of 92 DEVICE pointers in state-dict order (weight, bias per layer; torch layouts). */
int pws_netg_pack_weights(const float *const *params, float *packed, int input_nc, int ngf,
                          pws_stream_t stream);
/* The same for a buffer that will serve forwards of ONE math mode only (a training loop re-packs after every optimizer step): `math`
 * PWS_MATH_BF16 leaves out the Winograd-domain copies of the layers that have bf16 weights (those layers never read them in that mode),
 * PWS_MATH_FP32 leaves out the bf16 copies; anything else packs everything (= pws_netg_pack_weights).  Running a forward of the other
 * mode on such a buffer reads stale copies: re-pack when the mode changes. */
int pws_netg_pack_weights_for(const float *const *params, float *packed, int input_nc, int ngf, int math,
                              pws_stream_t stream);
size_t pws_netg_workspace_bytes(int n, int input_nc, int ngf, int is_training);
/* x: [n,input_nc,256,256] NCHW.  grids: is_training ? [3][n,256,256,2] : [n,256,256,2] (stage 3).
 * resid: is_training ? [3][n,256,256,2] : ignored (may be NULL).  thetas (nullable): [3][n,6]. */
int pws_netg_forward(const float *packed, const float *x, int n, int input_nc, int ngf, int is_training,
                     int align_corners, void *ws, size_t ws_bytes, float *grids, float *resid, float *thetas,
                     pws_stream_t stream);

/* The same forward with its mode in the ARGUMENTS instead of the process-wide pws_set_option() defaults: two generators with
 * different arithmetic may run from two host threads (or on two devices) at once.  opts == NULL: as pws_netg_forward. */
typedef struct pws_netg_opts {
    int math;       /* PWS_MATH_FP32 / PWS_MATH_BF16 */
    int store;      /* PWS_STORE_FP32 / PWS_STORE_BF16 (needs PWS_MATH_BF16 and ngf % 32 == 0) */
    int two_queues; /* 1: fork the internal second queue (forward: the stage-2/3 encoder -- stages 2 and 3 run in lockstep, their shared
                       layers as one launch of batch 2n -- and the deep decoder levels beside stage 1's encoder / decoder;
                       backward: every weight gradient beside the data-gradient chain; the queues join before the
                       call's last launch on the caller's stream / at the end of the call); 0: caller's stream only;
                       -1: the process default (PWS_OPT_TWO_QUEUES) */
    int flags;      /* bit set of PWS_NETG_*; unknown bits are refused */
    size_t x_sample_stride; /* floats between consecutive samples of the window tensor x; 0 = dense (input_nc * 256 * 256).  The
                               windows of a video are OVERLAPPING views of one plane buffer (window b = planes b .. b+30,
                               main_new.py:627-673): stride 256 * 256 reads them in place instead of from a gathered copy.
                               Inference forward only (the backward reads x dense). */
} pws_netg_opts;
#define PWS_NETG_DETERMINISTIC 1   /* backward: every weight / bias gradient element receives exactly ONE fp32 atomic add per
                                      launch (no pixel split across workgroups), so two runs give bit-identical gradients; slower */
#define PWS_NETG_PRUNE_DEAD 2      /* inference forward (is_training = 0) only: do not compute stage 1's `up2` (x122, reference
                                      lib/networks_cascading.py:171): its only consumers are `up1` (:173) and stage 2's `up_bottom1`
                                      (:196), both under `if is_training` -- the returned field is bit-identical, 2.147 of the 94.48 GFLOP
                                      per frame are not spent.  Off by default: the reference executes the layer. */
int pws_netg_forward_opts(const float *packed, const float *x, int n, int input_nc, int ngf, int is_training, int align_corners,
                          void *ws, size_t ws_bytes, float *grids, float *resid, float *thetas, const pws_netg_opts *opts,
                          pws_stream_t stream);
/* The conv launches pws_netg_forward_opts would issue for this configuration on a device of `compute_units` CUs, in issue order:
 * one pws_conv_choice per conv launch (tag = layer index; the heads are not conv launches) into out[0 .. max).  Walks the forward's
 * graph over a fixed 256-byte aligned stand-in for arena, weights and window (the alignment the real call requires) and asks the
 * dispatch ladder without launching: no HIP call, no stream, no event.  Returns the number of conv launches (may exceed max) or a
 * negative error.  out may be NULL when max == 0. */
int pws_netg_forward_plan(int n, int input_nc, int ngf, int is_training, const pws_netg_opts *opts, int compute_units,
                          pws_conv_choice *out, int max);

/* ---- training: backward of the whole generator (is_training=1 forward must have run on the SAME ws, untouched since).
 * Data-gradient weights: a second packed buffer (pws_netg_packed_dgrad_floats) filled by pws_netg_pack_weights_dgrad.
 * g_grids / g_resid: [3][n,256,256,2] each, or NULL as a whole (no gradient wrt that output list).
 * dpacked: the GRADIENT SLAB (pws_netg_grad_floats floats, overwritten): per layer in state-dict order the weight gradient in the
 * forward packed layout with the bias gradient behind it and nothing else (no Winograd / bf16 copies as in `packed`), so that a
 * data-parallel host all-reduces the slab -- or the ranges pws_netg_grad_layout reports for the layers a run finished -- IN PLACE
 * (replaces nn.DataParallel's reduce to GPU 0, lib/networks_cascading.py:51-52) and unpacks once;
 * pws_netg_unpack_grads converts it to 92 torch-layout tensors.  dx (nullable): gradient wrt the input window is not
 * needed by the reference (the window is data) and is not computed. */
size_t pws_netg_packed_dgrad_floats(int input_nc, int ngf);
size_t pws_netg_grad_floats(int input_nc, int ngf);
/* first_float[46], floats[46] (HOST): the contiguous range of the gradient slab that holds layer i's weight + bias gradient (with
 * its alignment padding, which stays zero); consecutive layers abut, so the layers a backward run reports final merge into a few
 * large ranges. */
int pws_netg_grad_layout(int input_nc, int ngf, size_t *first_float, size_t *floats);
/* final_part[46] (HOST; no GPU call): the run of an nparts-run backward (pws_netg_backward_opts / _lists with part = 0 .. nparts-1)
 * after which layer i's range of the slab is final, i.e. the run whose final_mask first reports it -- lets a data-parallel host
 * plan its messages (and a CPU rehearsal replay them) without a device. */
int pws_netg_backward_plan(int input_nc, int ngf, int nparts, unsigned char *final_part);
int pws_netg_pack_weights_dgrad(const float *const *params, float *packed_dgrad, int input_nc, int ngf,
                                pws_stream_t stream);
/* Both buffers of a training step at once (ABI 5).  math == PWS_MATH_BF16 and ngf % 64 == 0: the conv layers go torch layout -> bf16
 * forward copy + bf16 data-gradient copy in ONE pass, without the fp32 packed copies nothing reads in that mode (so the buffers then
 * serve bf16-math calls only, as pws_netg_pack_weights_for(.., PWS_MATH_BF16, ..) already implies); otherwise the two calls above. */
int pws_netg_pack_weights_train(const float *const *params, float *packed, float *packed_dgrad, int input_nc, int ngf, int math,
                                pws_stream_t stream);
size_t pws_netg_train_workspace_bytes(int n, int input_nc, int ngf);
int pws_netg_backward(const float *packed, const float *packed_dgrad, const float *x, int n, int input_nc, int ngf,
                      int align_corners, void *ws, size_t ws_bytes, const float *resid, const float *thetas,
                      const float *g_grids, const float *g_resid, float *dpacked, pws_stream_t stream);
/* The same backward cut into `nparts` consecutive runs of the reversed layer tape; call part = 0 .. nparts-1 in order on the
 * same arguments.  final_mask (nullable, HOST, 46 bytes, one per layer in state-dict order): set to 1 for every layer whose
 * weight / bias gradient in `dpacked` is complete once this run has executed -- a data-parallel host unpacks and all-reduces
 * those on a second stream while the next run computes (gradient exchange overlapped with backward). */
int pws_netg_backward_part(const float *packed, const float *packed_dgrad, const float *x, int n, int input_nc, int ngf,
                           int align_corners, void *ws, size_t ws_bytes, const float *resid, const float *thetas,
                           const float *g_grids, const float *g_resid, float *dpacked, int part, int nparts,
                           unsigned char *final_mask, pws_stream_t stream);
/* pws_netg_backward / pws_netg_backward_part with the mode of the forward that filled `ws` passed explicitly (opts must equal the
 * forward's; NULL: the process defaults).  part = 0, nparts = 1, final_mask = NULL is the whole backward. */
int pws_netg_backward_opts(const float *packed, const float *packed_dgrad, const float *x, int n, int input_nc, int ngf,
                           int align_corners, void *ws, size_t ws_bytes, const float *resid, const float *thetas,
                           const float *g_grids, const float *g_resid, float *dpacked, int part, int nparts,
                           unsigned char *final_mask, const pws_netg_opts *opts, pws_stream_t stream);
/* pws_netg_backward_opts with the six upstream gradients as two HOST arrays of 3 DEVICE pointers ([n,256,256,2] each; an entry, or a
 * whole array, may be NULL: that output has no gradient) -- autograd hands them over as separate tensors (main_new.py:214), so no
 * stacked copy and no zero-filled stand-ins are needed. */
int pws_netg_backward_lists(const float *packed, const float *packed_dgrad, const float *x, int n, int input_nc, int ngf,
                            int align_corners, void *ws, size_t ws_bytes, const float *resid, const float *thetas,
                            const float *const *g_grids, const float *const *g_resid, float *dpacked, int part, int nparts,
                            unsigned char *final_mask, const pws_netg_opts *opts, pws_stream_t stream);
/* ---- use_BN=True training (lib/cfg.py:37; lib/networks_cascading.py:253-341: BatchNorm2d after every conv, batch statistics).
 * bn_params / bn_running / dbn: flat buffers of pws_netg_bn_floats() floats, per layer in state-dict order
 * [gamma(cout) | beta(cout)], [running_mean | running_var], [dgamma | dbeta].  The forward is the is_training one (6 fields) and
 * updates bn_running (nullable) with `momentum` once per call of a module, as torch does (down_bottom1, which the reference
 * evaluates twice on the same input, is computed once and updated twice); n >= 2 (the theta head has one value per sample and
 * channel).  `packed` holds the raw (un-folded) conv weights.  fp32 math / storage only; arena:
 * pws_netg_train_workspace_bytes_bn.  dpacked's bias entries stay zero: a bias in front of a BatchNorm has no gradient. */
size_t pws_netg_bn_floats(int input_nc, int ngf);
size_t pws_netg_train_workspace_bytes_bn(int n, int input_nc, int ngf);
int pws_netg_forward_bn(const float *packed, const float *bn_params, float *bn_running, float momentum, float eps, const float *x,
                        int n, int input_nc, int ngf, int align_corners, void *ws, size_t ws_bytes, float *grids, float *resid,
                        float *thetas, pws_stream_t stream);
int pws_netg_backward_bn(const float *packed, const float *packed_dgrad, const float *bn_params, float eps, const float *x, int n,
                         int input_nc, int ngf, int align_corners, void *ws, size_t ws_bytes, const float *resid, const float *thetas,
                         const float *g_grids, const float *g_resid, float *dpacked, float *dbn, pws_stream_t stream);
/* The same two with their mode in the arguments: opts->math = PWS_MATH_BF16 runs the conv contractions (forward, data and weight
 * gradients) on the bf16 matrix cores -- operands rounded while they are staged, fp32 accumulation; activations, BatchNorm
 * statistics and gradients stay fp32 (opts->store must be PWS_STORE_FP32).  opts == NULL: fp32. */
int pws_netg_forward_bn_opts(const float *packed, const float *bn_params, float *bn_running, float momentum, float eps, const float *x,
                             int n, int input_nc, int ngf, int align_corners, void *ws, size_t ws_bytes, float *grids, float *resid,
                             float *thetas, const pws_netg_opts *opts, pws_stream_t stream);
int pws_netg_backward_bn_opts(const float *packed, const float *packed_dgrad, const float *bn_params, float eps, const float *x, int n,
                              int input_nc, int ngf, int align_corners, void *ws, size_t ws_bytes, const float *resid,
                              const float *thetas, const float *g_grids, const float *g_resid, float *dpacked, float *dbn,
                              const pws_netg_opts *opts, pws_stream_t stream);
/* grads: HOST array of 92 DEVICE pointers (torch layouts, state-dict order), overwritten; a layer whose weight AND bias
 * pointers are NULL is skipped. */
int pws_netg_unpack_grads(const float *dpacked, float *const *grads, int input_nc, int ngf, pws_stream_t stream);

/* ---------------------------------------------------------------- measurement hooks (bench / tests only)
 * When enabled, every kernel launch of this library is bracketed by two hipEvents on the launch stream and
 * tagged with its algorithmic work.  Process-global and not thread-safe: a measurement facility, off by
 * default, never enabled by the product path. */
typedef struct pws_prof_record {
    int kernel_id;  /* index for pws_prof_kernel_name() */
    int tag;        /* caller-defined (the generator executor passes the layer index) */
    double flops;   /* algorithmic floating-point operations of this launch */
    double bytes;   /* algorithmic HBM bytes of this launch (each tensor touched once) */
    float ms;       /* hipEventElapsedTime between the two events */
} pws_prof_record;
int pws_prof_enable(int on);
/* Synchronises the recorded events, copies up to max_records records (launch order), clears the log,
 * returns the number of records that were pending (may exceed max_records) or a negative error. */
int pws_prof_collect(pws_prof_record *out, int max_records);
const char *pws_prof_kernel_name(int kernel_id);

#ifdef __cplusplus
}
#endif
#endif /* PWSTABLE_H */
