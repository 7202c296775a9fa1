// Implicit-GEMM convolution / transposed convolution for gfx950 on the exact-fp32 matrix cores
// (v_mfma_f32_32x32x2_f32), NHWC activations, fused bias + activation, virtual concat on the read side.
//
// Replaces the ATen conv2d / conv_transpose2d + LeakyReLU / ReLU + torch.cat sequence of the reference
// blocks (reference lib/networks_cascading.py:245-350).
//
// GEMM view:  M = output pixels (n,y,x)   N = cout   K = taps x cin.
//   * A workgroup owns a TN x TH x TW block of output pixels (BM = TN*TH*TW) and BN = 64 output channels.
//   * K is walked in chunks of CK input channels.  Per chunk the (halo'd) input tile [pixels][CK] and the
//     weight slab [taps][CK][BN] are staged in LDS once and reused by all taps (an input pixel is read from
//     HBM/L2 ~1.3x instead of 9x).  LDS rows are padded to CK+1 floats so that the MFMA A-fragment read
//     (lane = pixel, one float per lane) is bank-conflict-free.
//   * Chunk c+1 is fetched global->registers while chunk c is being multiplied (the f32 MFMA is 64 cycles
//     per instruction, so a chunk is thousands of cycles of matrix work); two workgroups per CU cover the rest.
//   * A "virtual concat": the input channels come from up to 4 NHWC sources with their own pixel strides,
//     so torch.cat never copies.  The first layer reads the reference's NCHW input directly.
//   * ConvTranspose2d k4 s2 p1 runs as 4 independent sub-pixel 2x2 convolutions (one output parity class per
//     workgroup), ConvTranspose2d k3 s1 p1 as a 3x3 convolution with flipped taps (done at pack time).
//   * Tile shape is picked per launch so that the grid fills 256 CUs; the deep, small-spatial layers
//     (<= 16x16 outputs: M is tiny, K is 2304..16384, the weights are the traffic) additionally split K over
//     workgroups: every split streams its own slice of the weights and writes an fp32 partial tile, and a
//     small reduce kernel adds the partials, the bias and the activation (deterministic; no atomics).
//
// Numerics: fp32 in / fp32 accumulate; v_mfma_f32_32x32x2_f32 is bit-for-bit an fmaf chain in k order.
#include "conv_common.h"

namespace pws {

// SUBPIX: 0 = ordinary convolution; 1 = ConvTranspose2d k4 s2 p1 forward (output parity class (py,px) is a 2x2
// convolution whose window starts at (y+py-1, x+px-1)); 2 = data gradient of Conv2d k3 s2 p1 (class (py,px) is a 2x2
// window starting at (y, x) of which the even parity uses only the first tap).
template <int KS_, int STRIDE_, int PAD_, int SUBPIX_, int TH_, int TW_, int TN_, int CK_, int WM_, int WN_, int MT_,
          int NT_, bool NCHW_ = false>
struct ConvCfg {
    static constexpr int KS = KS_, STRIDE = STRIDE_, PAD = PAD_, TH = TH_, TW = TW_, TN = TN_, CK = CK_;
    static constexpr int SUBPIX = SUBPIX_;
    static constexpr bool CONVT = SUBPIX_ != 0, NCHW = NCHW_;
    static constexpr int WM = WM_, WN = WN_, MT = MT_, NT = NT_;
    static constexpr int THREADS = 64 * WM * WN;
    static constexpr int BM = TH * TW * TN, BN = 32 * NT * WN;
    static_assert(BM == 32 * MT * WM, "tile pixels must equal the M extent of the wave grid");
    static constexpr int IH = (TH - 1) * STRIDE + KS, IW = (TW - 1) * STRIDE + KS;
    static constexpr int PIX = TN * IH * IW;
    static constexpr int CKP = CK + 1;
    static constexpr int TAPS = KS * KS;
    static constexpr int LDS_IN = (PIX * CKP + 3) / 4 * 4;  // floats, keeps the weight slab 16-B aligned
    static constexpr int LDS_W = TAPS * CK * BN;
    static constexpr int LDS_BYTES = (LDS_IN + LDS_W) * 4;
    static constexpr int C4 = CK / 4;
    static constexpr int ITEMS_IN = (PIX * C4 + THREADS - 1) / THREADS;
    static constexpr int ITEMS_W = (TAPS * CK * (BN / 4) + THREADS - 1) / THREADS;
    static constexpr int ITEMS_NCHW = (PIX * CK + THREADS - 1) / THREADS;
};

template <class C>
__global__ void __launch_bounds__(C::THREADS, 2) conv_mfma_kernel(const ConvKParams p) {
    extern __shared__ float lds[];
    float *lds_in = lds;
    float *lds_w = lds + C::LDS_IN;

    const int tid = threadIdx.x;
    const int lane = tid & 63, wv = tid >> 6;
    const int l31 = lane & 31, hi = lane >> 5;
    const int wm = wv / C::WN, wn = wv % C::WN;

    // ---- which tile / output-channel group / parity class / K split
    unsigned tile;
    int cls, split;
    conv_block_coords(p, C::CONVT, tile, cls, split);
    const int tx_i = tile % p.tiles_x;
    const int ty_i = (tile / p.tiles_x) % p.tiles_y;
    const int tn_i = tile / (p.tiles_x * p.tiles_y);
    const int n0 = tn_i * C::TN, y0 = ty_i * C::TH, x0 = tx_i * C::TW;
    const int co0 = blockIdx.y * C::BN;
    const int py = cls >> 1, px = cls & 1;
    const int pad_y = C::SUBPIX == 1 ? 1 - py : (C::SUBPIX == 2 ? 0 : C::PAD);
    const int pad_x = C::SUBPIX == 1 ? 1 - px : (C::SUBPIX == 2 ? 0 : C::PAD);
    const int iy0 = y0 * C::STRIDE - pad_y, ix0 = x0 * C::STRIDE - pad_x;

    // ---- hoisted per-thread staging descriptors (pixel decode is chunk independent).
    // Loads are UNCONDITIONAL (out-of-image / out-of-range items read a valid dummy address and are zeroed by a select
    // afterwards): a conditional load makes hipcc branch around it and wait vmcnt(0) before the next one, which
    // serialises the whole prefetch (cdna_hip_programming.md, "register or load" trap).
    int g_pix[C::ITEMS_IN];   // global pixel index (n*H+iy)*W+ix, 0 when masked
    int l_off[C::ITEMS_IN];   // LDS float offset, -1 for items past the tile
    int g_c4[C::ITEMS_IN];
    unsigned ok_mask = 0;
#pragma unroll
    for (int it = 0; it < C::ITEMS_IN; ++it) {
        const int item = tid + it * C::THREADS;
        const int pix = item / C::C4, c4 = item % C::C4;
        const int lx = pix % C::IW, ly = (pix / C::IW) % C::IH, tn = pix / (C::IW * C::IH);
        const int n = n0 + tn, iy = iy0 + ly, ix = ix0 + lx;
        const bool ok = item < C::PIX * C::C4 && n < p.N && iy >= 0 && iy < p.H && ix >= 0 && ix < p.W;
        g_pix[it] = ok ? (n * p.H + iy) * p.W + ix : 0;
        ok_mask |= ok ? (1u << it) : 0u;
        l_off[it] = item < C::PIX * C::C4 ? pix * C::CKP + c4 * 4 : -1;
        g_c4[it] = c4 * 4;
    }
    static_assert(C::ITEMS_IN <= 32 && C::ITEMS_W <= 32, "mask width");
    // weight-slab items: offset inside one [tap][CK][cout] slab, 0 (a valid address) when masked
    int w_off[C::ITEMS_W];
    unsigned w_mask = 0;
#pragma unroll
    for (int it = 0; it < C::ITEMS_W; ++it) {
        const int item = tid + it * C::THREADS;
        const int row = item / (C::BN / 4), q = item % (C::BN / 4);
        const int tap = row / C::CK, c = row % C::CK;
        const bool ok = item < C::TAPS * C::CK * (C::BN / 4) && (co0 + q * 4) < p.cout;
        w_off[it] = ok ? (tap * p.cin_pad + c) * p.cout + co0 + q * 4 : 0;
        w_mask |= ok ? (1u << it) : 0u;
    }
    const float *w_cls = p.w + (size_t)cls * C::TAPS * p.cin_pad * p.cout;
    float4 r_in[C::NCHW ? 1 : C::ITEMS_IN];
    float4 r_w[C::ITEMS_W];
    float r_nchw[C::NCHW ? C::ITEMS_NCHW : 1];

    auto load_chunk = [&](int s, int c0, int wrow) {
        if constexpr (C::NCHW) {
            const int Creal = p.src_c[0];
            const size_t sstride = p.src_ld[0] ? (size_t)p.src_ld[0] : (size_t)Creal * p.H * p.W;   // floats between samples
#pragma unroll
            for (int it = 0; it < C::ITEMS_NCHW; ++it) {
                const int item = tid + it * C::THREADS;
                const int c = item / C::PIX, pix = item % C::PIX;
                const int lx = pix % C::IW, ly = (pix / C::IW) % C::IH, tn = pix / (C::IW * C::IH);
                const int n = n0 + tn, iy = iy0 + ly, ix = ix0 + lx;
                const bool ok = item < C::PIX * C::CK && (c0 + c) < Creal && n < p.N && iy >= 0 && iy < p.H && ix >= 0 &&
                                ix < p.W;
                const size_t off = ok ? (size_t)n * sstride + ((size_t)(c0 + c) * p.H + iy) * p.W + ix : 0;
                const float v = p.src_ptr[0][off];  // unconditional load, masked by a select
                r_nchw[it] = ok ? v : 0.f;
            }
        } else {
            const float *sp = p.src_ptr[s] + c0;
            const size_t ld = p.src_ld[s];
#pragma unroll
            for (int it = 0; it < C::ITEMS_IN; ++it)
                r_in[it] = *reinterpret_cast<const float4 *>(sp + (size_t)g_pix[it] * ld + g_c4[it]);
        }
        const float *wp = w_cls + (size_t)wrow * p.cout;
#pragma unroll
        for (int it = 0; it < C::ITEMS_W; ++it) r_w[it] = *reinterpret_cast<const float4 *>(wp + w_off[it]);
    };
    auto store_chunk = [&]() {
        if constexpr (C::NCHW) {
#pragma unroll
            for (int it = 0; it < C::ITEMS_NCHW; ++it) {
                const int item = tid + it * C::THREADS;
                const int c = item / C::PIX, pix = item % C::PIX;
                if (item < C::PIX * C::CK) lds_in[pix * C::CKP + c] = r_nchw[it];
            }
        } else {
#pragma unroll
            for (int it = 0; it < C::ITEMS_IN; ++it) {
                if (l_off[it] >= 0) {
                    const bool ok = (ok_mask >> it) & 1u;
                    float *d = lds_in + l_off[it];
                    d[0] = ok ? r_in[it].x : 0.f, d[1] = ok ? r_in[it].y : 0.f, d[2] = ok ? r_in[it].z : 0.f,
                    d[3] = ok ? r_in[it].w : 0.f;
                }
            }
        }
#pragma unroll
        for (int it = 0; it < C::ITEMS_W; ++it) {
            const int item = tid + it * C::THREADS;
            if (item < C::TAPS * C::CK * (C::BN / 4)) {
                const bool ok = (w_mask >> it) & 1u;
                *reinterpret_cast<float4 *>(lds_w + item * 4) =
                    ok ? r_w[it] : make_float4(0.f, 0.f, 0.f, 0.f);
            }
        }
    };

    // ---- accumulators and fragment bases
    f32x16 acc[C::MT][C::NT];
#pragma unroll
    for (int mt = 0; mt < C::MT; ++mt)
#pragma unroll
        for (int nt = 0; nt < C::NT; ++nt)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[mt][nt][r] = 0.f;

    int a_base[C::MT];
#pragma unroll
    for (int mt = 0; mt < C::MT; ++mt) {
        const int m = (wm * C::MT + mt) * 32 + l31;
        const int tx = m % C::TW, ty = (m / C::TW) % C::TH, tn = m / (C::TW * C::TH);
        a_base[mt] = ((tn * C::IH + ty * C::STRIDE) * C::IW + tx * C::STRIDE) * C::CKP + hi;
    }
    const int b_base = hi * C::BN + wn * C::NT * 32 + l31;

    // ---- K loop over this split's (source, channel chunk) range
    int total_chunks = 0;
    if constexpr (C::NCHW) {
        total_chunks = p.cin_pad / C::CK;
    } else {
        for (int s = 0; s < p.nsrc; ++s) total_chunks += p.src_c[s] / C::CK;
    }
    const int ch_begin = split * p.chunks_per_split;
    const int ch_end = min(total_chunks, ch_begin + p.chunks_per_split);
    int s = 0, c0 = ch_begin * C::CK, wrow = ch_begin * C::CK;
    if constexpr (!C::NCHW) {
        while (s < p.nsrc - 1 && c0 >= p.src_c[s]) c0 -= p.src_c[s], ++s;
    }
    if (ch_begin < ch_end) load_chunk(s, c0, wrow);
    for (int ch = ch_begin; ch < ch_end; ++ch) {
        __syncthreads();  // everyone finished reading the previous chunk from LDS
        store_chunk();
        __syncthreads();
        // advance and prefetch the next chunk into registers while this one is multiplied
        c0 += C::CK, wrow += C::CK;
        if (!C::NCHW && c0 >= p.src_c[s]) ++s, c0 = 0;
        if (ch + 1 < ch_end) load_chunk(s, c0, wrow);

#pragma unroll
        for (int tap = 0; tap < C::TAPS; ++tap) {
            if (C::SUBPIX == 2 && ((!py && tap / C::KS) || (!px && tap % C::KS))) continue;  // block-uniform
            const int toff = ((tap / C::KS) * C::IW + (tap % C::KS)) * C::CKP;
#pragma unroll
            for (int kk = 0; kk < C::CK / 2; ++kk) {
                float a[C::MT], b[C::NT];
#pragma unroll
                for (int mt = 0; mt < C::MT; ++mt) a[mt] = lds_in[a_base[mt] + toff + 2 * kk];
#pragma unroll
                for (int nt = 0; nt < C::NT; ++nt) b[nt] = lds_w[b_base + (tap * C::CK + 2 * kk) * C::BN + nt * 32];
#pragma unroll
                for (int mt = 0; mt < C::MT; ++mt)
#pragma unroll
                    for (int nt = 0; nt < C::NT; ++nt)
                        acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[mt], b[nt], acc[mt][nt], 0, 0, 0);
            }
        }
    }

    // ---- epilogue: bias + activation / gradient scatter (or raw partial sums when K is split), NHWC store
    //      (32 lanes = 32 consecutive channels = 128 B per pixel)
    const bool partial = p.ksplit > 1;
    float *part = p.out + (size_t)split * p.split_stride;
#pragma unroll
    for (int nt = 0; nt < C::NT; ++nt) {
        const int co = co0 + (wn * C::NT + nt) * 32 + l31;
        const bool co_ok = co < p.cout;
#pragma unroll
        for (int mt = 0; mt < C::MT; ++mt) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int m = (wm * C::MT + mt) * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi;
                const int tx = m % C::TW, ty = (m / C::TW) % C::TH, tn = m / (C::TW * C::TH);
                const int n = n0 + tn, y = y0 + ty, x = x0 + tx;
                const int oy = C::CONVT ? 2 * y + py : y, ox = C::CONVT ? 2 * x + px : x;
                if (co_ok && n < p.N && y < p.LH && x < p.LW && oy < p.OH && ox < p.OW) {
                    const size_t pix = (size_t)(n * p.OH + oy) * p.OW + ox;
                    if (partial)
                        part[pix * p.cout + co] = acc[mt][nt][r];
                    else
                        epi_store(p, pix, co, acc[mt][nt][r]);
                }
            }
        }
    }
}

// Split-K reduce: sum the partial tiles (in split order: deterministic) and run the ordinary epilogue.
// partial[s] is dense [pixels][cout]; 4 consecutive channels per lane.
__global__ void __launch_bounds__(256) splitk_reduce_kernel(const ConvKParams p, const float *__restrict__ partial,
                                                            size_t total4) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total4) return;
    float4 a = reinterpret_cast<const float4 *>(partial)[i];
    for (int s = 1; s < p.ksplit; ++s) {
        const float4 b = reinterpret_cast<const float4 *>(partial + (size_t)s * p.split_stride)[i];
        a.x += b.x, a.y += b.y, a.z += b.z, a.w += b.w;
    }
    const size_t pix = (i * 4) / p.cout;
    const int co = (int)((i * 4) % p.cout);
    if (p.io_bf16) {  // bf16 storage (conv_bf16.hip): channel pairs as dwords
        epi_store_pair16(p, pix, co, a.x, a.y), epi_store_pair16(p, pix, co + 2, a.z, a.w);
        return;
    }
    epi_store(p, pix, co, a.x), epi_store(p, pix, co + 1, a.y), epi_store(p, pix, co + 2, a.z), epi_store(p, pix, co + 3, a.w);
}

int launch_splitk_reduce(const ConvKParams &kp, const float *partial, size_t total4, hipStream_t st) {
    hipLaunchKernelGGL(splitk_reduce_kernel, dim3((unsigned)((total4 + 255) / 256)), dim3(256), 0, st, kp, partial, total4);
    return check_launch("splitk_reduce_kernel");
}

// ------------------------------------------------------------------------------------------------ host side
template <class C>
static int run_cfg(const ConvKParams &kp, const ConvChoice &c, hipStream_t st) { return launch_planned<&conv_mfma_kernel<C>>(kp, c, st, "conv_mfma_kernel"); }

template <class C, int KID>
static constexpr TileChoice choice() {
    return TileChoice{C::TH, C::TW, C::TN, C::CK, C::BN, KID, {{C::THREADS, C::LDS_BYTES}, {C::THREADS, C::LDS_BYTES}}, &run_cfg<C>};
}

//                        KS S  P  subpix TH  TW  TN  CK WM WN MT NT
using K3S1_T256 = ConvCfg<3, 1, 1, 0, 16, 16, 1, 16, 4, 1, 2, 2>;
using K3S1_T128 = ConvCfg<3, 1, 1, 0, 8, 16, 1, 16, 4, 1, 1, 2>;
using K3S1_T64 = ConvCfg<3, 1, 1, 0, 8, 8, 1, 16, 2, 2, 1, 1>;
using K3S1_T64N4 = ConvCfg<3, 1, 1, 0, 4, 4, 4, 16, 2, 2, 1, 1>;
using K3S1_T64N16 = ConvCfg<3, 1, 1, 0, 2, 2, 16, 16, 2, 2, 1, 1>;
using K3S2_T256 = ConvCfg<3, 2, 1, 0, 16, 16, 1, 8, 4, 1, 2, 2>;
using K3S2_T128 = ConvCfg<3, 2, 1, 0, 8, 16, 1, 16, 4, 1, 1, 2>;
using K3S2_T64 = ConvCfg<3, 2, 1, 0, 8, 8, 1, 16, 2, 2, 1, 1>;
using K3S2_T64N4 = ConvCfg<3, 2, 1, 0, 4, 4, 4, 16, 2, 2, 1, 1>;
using K3S2_T64N16 = ConvCfg<3, 2, 1, 0, 2, 2, 16, 16, 2, 2, 1, 1>;
using K5S1_T256 = ConvCfg<5, 1, 2, 0, 16, 16, 1, 8, 4, 1, 2, 2>;
using K5S1_T256_NCHW = ConvCfg<5, 1, 2, 0, 16, 16, 1, 8, 4, 1, 2, 2, true>;
using CT4_T256 = ConvCfg<2, 1, 0, 1, 16, 16, 1, 16, 4, 1, 2, 2>;
using CT4_T128 = ConvCfg<2, 1, 0, 1, 8, 16, 1, 16, 4, 1, 1, 2>;
using CT4_T64 = ConvCfg<2, 1, 0, 1, 8, 8, 1, 16, 2, 2, 1, 1>;
using CT4_T64N4 = ConvCfg<2, 1, 0, 1, 4, 4, 4, 16, 2, 2, 1, 1>;
using CT4_T64N16 = ConvCfg<2, 1, 0, 1, 2, 2, 16, 16, 2, 2, 1, 1>;

// data-gradient kernels: conv k4 s2 p1 (gradient of ConvTranspose2d k4 s2 p1) and the sub-pixel gradient of conv k3 s2 p1
using K4S2_T256 = ConvCfg<4, 2, 1, 0, 16, 16, 1, 8, 4, 1, 2, 2>;
using K4S2_T128 = ConvCfg<4, 2, 1, 0, 8, 16, 1, 8, 4, 1, 1, 2>;
using K4S2_T64 = ConvCfg<4, 2, 1, 0, 8, 8, 1, 8, 2, 2, 1, 1>;
using K4S2_T64N4 = ConvCfg<4, 2, 1, 0, 4, 4, 4, 8, 2, 2, 1, 1>;
using K4S2_T64N16 = ConvCfg<4, 2, 1, 0, 2, 2, 16, 8, 2, 2, 1, 1>;
using SP3_T256 = ConvCfg<2, 1, 0, 2, 16, 16, 1, 16, 4, 1, 2, 2>;
using SP3_T128 = ConvCfg<2, 1, 0, 2, 8, 16, 1, 16, 4, 1, 1, 2>;
using SP3_T64 = ConvCfg<2, 1, 0, 2, 8, 8, 1, 16, 2, 2, 1, 1>;
using SP3_T64N4 = ConvCfg<2, 1, 0, 2, 4, 4, 4, 16, 2, 2, 1, 1>;
using SP3_T64N16 = ConvCfg<2, 1, 0, 2, 2, 2, 16, 16, 2, 2, 1, 1>;

// candidates ordered from the largest tile (best operand reuse) to the smallest
static const TileChoice kK3S1[] = {choice<K3S1_T256, KID_CONV_K3S1_BIG>(), choice<K3S1_T128, KID_CONV_K3S1_BIG>(),
                                   choice<K3S1_T64, KID_CONV_K3S1_SMALL>(), choice<K3S1_T64N4, KID_CONV_K3S1_SMALL>(),
                                   choice<K3S1_T64N16, KID_CONV_K3S1_SMALL>()};
static const TileChoice kK3S2[] = {choice<K3S2_T256, KID_CONV_K3S2_BIG>(), choice<K3S2_T128, KID_CONV_K3S2_BIG>(),
                                   choice<K3S2_T64, KID_CONV_K3S2_SMALL>(), choice<K3S2_T64N4, KID_CONV_K3S2_SMALL>(),
                                   choice<K3S2_T64N16, KID_CONV_K3S2_SMALL>()};
static const TileChoice kCT4[] = {choice<CT4_T256, KID_CONVT4_BIG>(), choice<CT4_T128, KID_CONVT4_BIG>(),
                                  choice<CT4_T64, KID_CONVT4_SMALL>(), choice<CT4_T64N4, KID_CONVT4_SMALL>(),
                                  choice<CT4_T64N16, KID_CONVT4_SMALL>()};
static const TileChoice kK4S2[] = {choice<K4S2_T256, KID_DGRAD_K4S2>(), choice<K4S2_T128, KID_DGRAD_K4S2>(),
                                   choice<K4S2_T64, KID_DGRAD_K4S2>(), choice<K4S2_T64N4, KID_DGRAD_K4S2>(),
                                   choice<K4S2_T64N16, KID_DGRAD_K4S2>()};
static const TileChoice kSP3[] = {choice<SP3_T256, KID_DGRAD_SP3>(), choice<SP3_T128, KID_DGRAD_SP3>(),
                                  choice<SP3_T64, KID_DGRAD_SP3>(), choice<SP3_T64N4, KID_DGRAD_SP3>(),
                                  choice<SP3_T64N16, KID_DGRAD_SP3>()};
static const TileChoice kK5[] = {choice<K5S1_T256, KID_CONV_K5S1>()};
static const TileChoice kK5N[] = {choice<K5S1_T256_NCHW, KID_CONV_K5S1>()};

// The direct kernel takes every launch: the end of the ladder (which has checked that the kind is a runnable one).
bool conv_mfma(int kind, bool dgrad, bool nchw, ConvKParams &kp, int cin_total, float *final_out, float *ws, size_t ws_floats, const ProfInfo &pi,
               const ConvCtx &cx, int *status) {
    const bool s1 = kind == PWS_CONV_K3S1 || kind == PWS_CONVT_K3S1, k5 = kind == PWS_CONV_K5S1;
    const TileChoice *cands = s1 ? kK3S1 : k5 ? (nchw ? kK5N : kK5) : kind == PWS_CONV_K3S2 ? (dgrad ? kSP3 : kK3S2) : (dgrad ? kK4S2 : kCT4);
    const int ncand = k5 ? 1 : 5;
    ConvChoice c;
    const TileChoice *t = plan_tiles(cands, ncand, kp, cin_total, final_out, ws, ws_floats, kFillBlocks, 0, &c);
    return conv_accept(cx, c, pi, status, [&] { return run_tiles(*t, c, kp, final_out, ws, cx.stream); });
}

}  // namespace pws
