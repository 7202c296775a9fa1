// Registry of PWS_OPT_EXPERIMENT ids: every non-product path the library can be switched to, by name.  0 is the product.
// Included from common.h.  g_experiment is named only here and in abi.cpp; every other read goes through exp_is / exp_in / exp_mask
// with an entry of this enum.  Ids and ranges are pairwise disjoint (tests/test_experiments_cpu.py); pwstablenet_amd/hipabi.py's
// class Exp mirrors the enum by hand.
//
// One line per entry: the id or range base, [n] = the size of a range, the file(s) that read it, a class, what it selects.  A measured
// alternative that was not kept stays only while a test compares the product against it (REFERENCE); otherwise it is deleted.
//   REFERENCE  a test compares the product against this path
//   FORCE      a test forces a product kernel onto shapes it would not take
//   ABLATE     timing only, results are meaningless
//   MEASURE    a measurement aid of tools/: the results are the product's
#pragma once

namespace pws {

extern int g_experiment;  // abi.cpp: PWS_OPT_EXPERIMENT

enum Exp : int {
    EXP_GS_BWD_GENERAL = 2,        // grid_sample.hip REFERENCE: the general backward kernel for the field-only gradient; never non-temporal
    EXP_U8_CVT_SHIFT = 4,          // grid_sample.hip REFERENCE: uint8 warp, float -> byte by (int) + clamp + shift; never non-temporal
    EXP_GS_ROWWIN = 5,             // grid_sample.hip REFERENCE: grid_sample_fwd2_kernel's row window + wave shuffle
    EXP_NO_SIGN_BITS = 12,         // netg_exec.h, conv_ring.hip REFERENCE: sign-bit epilogues off
    EXP_NETG_PER_STAGE = 15,       // netg_forward.cpp REFERENCE: the per-stage forward schedule instead of the lockstep one
    EXP_RING_OFF = 20,             // conv_ring.hip REFERENCE: conv_bf16_kernel instead of the bf16 ring kernel
    EXP_RING_SMALL = 21,           // conv_ring.hip FORCE: the ring kernel also for launches too small to fill the chip
    EXP_RINGF_OFF = 22,            // conv_ring_f32.hip REFERENCE: conv_mfma_kernel instead of the fp32 ring kernel
    EXP_RINGF_8X32 = 23,           // conv_ring_f32.hip FORCE: the fp32 ring kernel on small launches, 8 x 32 tiles
    EXP_RINGF_16X32 = 24,          // conv_ring_f32.hip FORCE: the fp32 ring kernel on small launches, 16 x 32 tiles
    EXP_FIRST_MFMA = 25,           // conv_first.hip, conv_first_wino.hip REFERENCE: conv_mfma_kernel<k5s1, NCHW> for the first layer
    EXP_FIRST_NO_WINO = 26,        // conv_first_wino.hip REFERENCE: conv_first_kernel instead of wino5_first_kernel
    EXP_RINGF_32CH = 27,           // conv_ring_f32.hip FORCE: the stride-2 kind's units of 32 output channels
    EXP_FIRST_SMALL = 29,          // conv_first.hip FORCE: conv_first_kernel on launches of few units
    EXP_WINO5_SMALL = 30,          // conv_first_wino.hip FORCE: wino5_first_kernel on launches of few units
    EXP_HEAD_V1 = 35,              // head.hip REFERENCE: the field head's first cut
    EXP_GS_U8_LANE_WINDOWS = 49,   // grid_sample.hip REFERENCE: the uint8 warp's per-lane field windows
    EXP_WRING_OFF = 50,            // conv_wring.hip REFERENCE: no Winograd ring kernel
    EXP_WRING_FORCE = 58,          // conv_wring.hip FORCE: the Winograd ring kernel whatever the number of units
    EXP_WRING_MODE2 = 59,          // conv_wring.hip FORCE: as 58, one parity class per unit
    EXP_SKINNY_OFF = 70,           // conv_skinny.hip REFERENCE: no fp32 one-shot kernel
    EXP_SKINNY16_OFF = 71,         // conv_skinny16.hip REFERENCE: no bf16 one-shot kernel
    EXP_SKINNY16_4096 = 72,        // conv_skinny16.hip FORCE: the bf16 one-shot kernel up to 4096 pixels
    EXP_SKINNY_SKIP = 73,          // conv_skinny.hip ABLATE: the fp32 one-shot launch is skipped
    EXP_WGRAD_RING_OFF = 80,       // wgrad_ring.hip REFERENCE: no ring weight-gradient kernel
    EXP_WGRAD_RING_FORCE = 81,     // wgrad_ring.hip FORCE: the ring weight-gradient kernel on every launch it covers
    EXP_HEAD_VALU = 90,            // head.hip REFERENCE: the field head's VALU kernels
    EXP_HEAD_BWD_VALU = 91,        // head_bwd.hip REFERENCE: the head backward's VALU kernels
    EXP_HEAD_ONE_TILE = 92,        // head.hip REFERENCE: one tile per workgroup
    EXP_DEEP_TILE_ALWAYS = 96,     // conv_bf16.hip FORCE: the deep maps' 256-pixel tiles whenever the map fits
    EXP_SHAPE_GENERAL = 97,        // objective.hip REFERENCE: the general shape-loss kernel
    EXP_TL1_TILED = 98,            // objective.hip REFERENCE: temporal_l1_bwd_tiled_kernel
    EXP_RING_8WAVE = 105,          // conv_ring.hip REFERENCE: the eight-wave kernel on 32-wide tiles
    EXP_SMOOTH_ONE_PIXEL = 110,    // objective.hip REFERENCE: field smoothness with one pixel per lane
    EXP_NO_PACK_ONE_PASS = 120,    // netg_layers.cpp REFERENCE: no one-pass bf16 weight packing
    EXP_RING_UNIT256 = 186,        // conv_ring.hip FORCE: units of 256 pixels
    EXP_RING_UNIT128 = 187,        // conv_ring.hip FORCE: units of 128 pixels
    EXP_WGRAD_NO_MERGE = 188,      // wgrad_bf16.hip REFERENCE: a shared layer's operand pairs as two launches
    EXP_WGRAD_MIN_TILES = 190,     // [10] wgrad_bf16.hip REFERENCE: tiles-per-workgroup floor 190 + t (product: 6)
    EXP_FIRST_ABLATE = 1100,       // [16] conv_first.hip ABLATE: 1100 + mask
    EXP_FIRST_CLOCK = 1200,        // conv_first.hip MEASURE: conv_first_kernel reports its shader clock
    EXP_WINO5_ABLATE = 1300,       // [64] conv_first_wino.hip ABLATE: 1300 + mask (16: every wave in the same order, not timing only)
    EXP_WGRAD_WIDE_ABLATE = 1400,  // [16] wgrad_ring.hip ABLATE: 1400 + mask on the wide kernel (masks 1..5, 7, 8, 15)
    EXP_RING_ABLATE = 1500,        // [32] conv_ring.hip ABLATE: 1500 + mask (16: no act' loads, wrong data gradients)
    EXP_WINO_ABLATE = 1600,        // [16] conv_wino.hip ABLATE: 1600 + mask
    EXP_BF16_PROBE = 2100,         // [64] conv_bf16.hip, conv_ring.hip ABLATE: 2100 + probe variant (-DPWS_INTERFERENCE_PROBE builds)
    EXP_RINGF_VARIANT = 2200,      // [48] conv_ring_f32.hip REFERENCE: 2200 + 16 v + mask; v = 1 full, 2 half workgroups; mask 1..7 ABLATE
    EXP_PARITY_LEDGER = 3000,      // [32] conv_mfma.hip MEASURE: 3000 + bits: those kernel families back to conv_mfma_kernel
    EXP_WRING_ABLATE = 4000,       // [1024] conv_wring.hip ABLATE: 4000 + mask (10 bits; instantiated masks only)
};

inline bool exp_is(Exp e) { return g_experiment == e; }
// the id lies in [base, base + n)
inline bool exp_in(Exp base, int n) { return g_experiment >= base && g_experiment < base + n; }
// the id's offset in [base, base + n), 0 outside
inline int exp_mask(Exp base, int n) { return exp_in(base, n) ? g_experiment - base : 0; }

}  // namespace pws
