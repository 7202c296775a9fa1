// Edge modes for the fused warps (grid_sample.hip, warp_bicubic.hip): an output pixel whose taps do not all lie inside the source is sampled
// again from the SOURCE frame continued beyond its rim -- "clamp" repeats the edge sample, "mirror" reflects about it -- instead of the blend
// with the pad colour the warp wrote.  No other frame is read: nothing crosses a frame.
//
// Definition (restated in tests/edge_ref.py).  Planes, source positions and coverage are border_keep.hip's: (ix, iy) is formed with the warps'
// fp32 operations (warp_common.h: yuv_field4, then one fma with the plane's un-normalisation constants); a pixel is covered iff
// m <= ix <= W-1-m and m <= iy <= H-1-m, m = 0 for the bilinear warp, 1 for the bicubic one; NaN is not covered.  A covered pixel keeps the
// warp's bytes, and so does one with a non-finite coordinate.  Every other pixel becomes
//   Q( sum_i sum_j wy_i wx_j v(fold(y0 + i, H), fold(x0 + j, W)) ),   x0 = floor(ix), y0 = floor(iy),
// taps 0, 1 with weights (1 - t, t) for bilinear, taps -1 .. 2 with the Keys weights (A = -0.75, warp_bicubic.hip's) for bicubic;
// fold(i, n) = min(max(i, 0), n - 1) for clamp; for mirror k = i mod 2 (n - 1), k < n ? k : 2 (n - 1) - k, and 0 when n == 1 (reflection
// without repeating the edge sample); v the source sample under the warp's read rule (swap_rb; P010 word >> 6; I010 min(word, 1023)); Q the
// byte paths' rule, clamp to the sample range and truncate, written as the warp writes it (P010: v10 << 6).
//
// Exactness.  The fp32 cubic weights do not sum to 1, so a row of taps is blended as the first tap plus weighted differences from it, and the
// rows likewise: taps that all hold one value give that value exactly.  floor(ix) is bounded to +-2^30 before the conversion to int (t is
// taken from the unbounded floor and is 0 out there), the mirror's period 2 (n - 1) is below 2^25 and the remainder is taken once per axis in
// int, so no finite coordinate overflows anything.
//
// Launch shape: keep's -- a wave owns 256 consecutive pixels of ONE plane row, a lane 4 of them; there is no recurrence, so the frames are the
// grid's z.  A lane forms its 4 coordinates and is done when none of them is to be filled.  For a pixel to fill it gathers the folded taps
// from the source frame with scalar byte / short loads (wedge-only traffic), blends in fp32 and quantises.  Only a lane that holds both
// kinds of pixel loads the current bytes to merge.  A lane reads any source sample and writes its own 4 pixels of `frames` alone.
#include "common.h"
#include "warp_common.h"
#include "border_lane.h"

namespace pws {
namespace edge {

using keep::PLANE_BGR;
using keep::load_lane;
using keep::store_lane;

constexpr float A = -0.75f;   // warp_bicubic.hip's weights, in its order of operations
__device__ __forceinline__ float c1(float s) { return ((A + 2.f) * s - (A + 3.f)) * s * s + 1.f; }
__device__ __forceinline__ float c2(float s) { return ((A * s - 5.f * A) * s + 8.f * A) * s - 4.f * A; }

// tap indices first .. first + NT - 1 of an axis of n samples, folded into [0, n): |first| <= 2^30 + 1, n < 2^24
template <int NT>
__device__ __forceinline__ void fold_taps(int first, int n, bool mirror, int idx[NT]) {
    if (!mirror) {
#pragma unroll
        for (int j = 0; j < NT; ++j) idx[j] = min(max(first + j, 0), n - 1);
        return;
    }
    const int period = 2 * (n - 1);
    if (period == 0) {
#pragma unroll
        for (int j = 0; j < NT; ++j) idx[j] = 0;
        return;
    }
    int k = first % period;   // (C++ remainder: the dividend's sign)
    k += k < 0 ? period : 0;
#pragma unroll
    for (int j = 0; j < NT; ++j) {
        idx[j] = k < n ? k : period - k;
        k = k + 1 == period ? 0 : k + 1;
    }
}

// the first tap, the fraction and the weights of one axis.  w[0] is not used: tap 0 is the base the others are differenced from.
template <bool BICUBIC>
__device__ __forceinline__ int axis(float c, float w[BICUBIC ? 4 : 2]) {
    const float fl = floorf(c), t = c - fl;   // (c finite; t = 0 where fl == c, as it is from 2^23 on)
    const int i0 = (int)__builtin_amdgcn_fmed3f(fl, -1073741824.f, 1073741824.f);
    if constexpr (BICUBIC) {
        const float u = 1.f - t;
        w[0] = c2(t + 1.f), w[1] = c1(t), w[2] = c1(u), w[3] = c2(u + 1.f);
        return i0 - 1;
    } else {
        w[0] = 1.f - t, w[1] = t;
        return i0;
    }
}

template <int SB, int LAYOUT>
__device__ __forceinline__ float read_sample(const unsigned char *p) {
    if constexpr (SB == 1) return (float)*p;
    const unsigned word = *reinterpret_cast<const unsigned short *>(p);
    return (float)(LAYOUT == 0 ? word >> 6 : min(word, 1023u));
}

template <int SB, int LAYOUT>
__device__ __forceinline__ unsigned quantise(float v) {   // clamp, truncate, place
    if constexpr (SB == 1) return (unsigned)fminf(fmaxf(v, 0.f), 255.f);
    const unsigned q = (unsigned)fminf(fmaxf(v, 0.f), 1023.f);
    return LAYOUT == 0 ? q << 6 : q;
}

// One wave's row chunk of one plane kind of one frame.  SB: bytes per sample; LAYOUT (SB 2): 0 the P010 placement, 1 I010's.
template <int KIND, int SB, int LAYOUT, bool BICUBIC>
__device__ __forceinline__ void edge_row(unsigned char *frame, const unsigned char *__restrict__ src, const float *__restrict__ field, const yuv::Plane &P,
                                         int fmode, unsigned t, unsigned oy, int ox0, int fh, int fw, bool swap, bool mirror) {
    constexpr int NCI = KIND == PLANE_BGR ? 3 : (KIND == yuv::PLANE_NV12_UV ? 2 : 1), NP = KIND == yuv::PLANE_I420_UV ? 2 : 1;
    constexpr int NDW = NCI * SB;   // dwords of a lane's 4 pixels in one source plane = bytes per pixel
    constexpr bool BYTES = KIND == yuv::PLANE_I420_UV && SB == 1;
    constexpr int NT = BICUBIC ? 4 : 2;
    const int W = P.w, H = P.h;
    const bool active = ox0 < W;
    if (fmode < 2 && !active) return;   // (modes 2 / 3: every lane fetches and serves field columns)
    const bool full = ox0 + 4 <= W;     // chroma rows of width 2 mod 4: the row's last lane owns 2 pixels
    const unsigned own = !active ? 0u : (full ? 0xfu : 0x3u);
    const float m = BICUBIC ? 1.f : 0.f;
    const float xhi = (float)(W - 1) - m, yhi = (float)(H - 1) - m;
    f32x2 gx[2], gy[2];
    if (fmode == 2) yuv_field4<2>(field, t, oy, ox0, W - 1, fh, fw, P.ry, P.rx, gx, gy);
    else if (fmode == 3) yuv_field4<3>(field, t, oy, ox0, W - 1, fh, fw, P.ry, P.rx, gx, gy);
    else yuv_field4<0>(field, t, oy, ox0, W - 1, fh, fw, P.ry, P.rx, gx, gy);
    float cx[4], cy[4];
    unsigned fill = 0u;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const float g0 = i & 1 ? gx[i >> 1].y : gx[i >> 1].x, g1 = i & 1 ? gy[i >> 1].y : gy[i >> 1].x;
        const float ix = fmaf(g0, P.kx, P.kx1), iy = fmaf(g1, P.ky, P.ky1);   // (the warps' pk_fma, per component)
        const bool covered = ix >= m && ix <= xhi && iy >= m && iy <= yhi;    // (false for NaN)
        const bool finite = fabsf(ix) <= 3.4028234664e38f && fabsf(iy) <= 3.4028234664e38f;   // (false for NaN and inf)
        fill |= !covered && finite ? 1u << i : 0u;
        cx[i] = ix, cy[i] = iy;
    }
    fill &= own;
    if (fill == 0u) return;
    unsigned res[NP][NDW];
#pragma unroll
    for (int p = 0; p < NP; ++p)
#pragma unroll
        for (int k = 0; k < NDW; ++k) res[p][k] = 0u;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        if (!((fill >> i) & 1u)) continue;
        float wx[NT], wy[NT];
        int xs[NT], ys[NT];
        fold_taps<NT>(axis<BICUBIC>(cx[i], wx), W, mirror, xs);
        fold_taps<NT>(axis<BICUBIC>(cy[i], wy), H, mirror, ys);
#pragma unroll
        for (int c = 0; c < NCI * NP; ++c) {
            // byte offset of source sample (row 0, column 0) of channel c, and the byte step of a column
            const unsigned base = (KIND == yuv::PLANE_I420_UV && c == 1 ? P.off1 : P.off0) +
                                  (KIND == PLANE_BGR ? (swap ? 2u - (unsigned)c : (unsigned)c) : (KIND == yuv::PLANE_NV12_UV ? (unsigned)(c * SB) : 0u));
            float rows[NT];
#pragma unroll
            for (int a = 0; a < NT; ++a) {
                const unsigned char *row = src + base + (unsigned)ys[a] * P.pitch;
                const float v0 = read_sample<SB, LAYOUT>(row + (unsigned)xs[0] * NDW);
                float r = v0;   // the first tap plus weighted differences from it: equal taps give their value exactly
#pragma unroll
                for (int b = 1; b < NT; ++b) r = fmaf(wx[b], read_sample<SB, LAYOUT>(row + (unsigned)xs[b] * NDW) - v0, r);
                rows[a] = r;
            }
            float v = rows[0];
#pragma unroll
            for (int a = 1; a < NT; ++a) v = fmaf(wy[a], rows[a] - rows[0], v);
            const unsigned q = quantise<SB, LAYOUT>(v);
            // sample (pixel i, channel c) is element e of SB bytes among the lane's bytes of its source plane
            const int p = KIND == yuv::PLANE_I420_UV ? c : 0, e = KIND == yuv::PLANE_I420_UV ? i : i * NCI + c;
            res[p][e * SB / 4] |= q << (8 * (e * SB % 4));
        }
    }
    const unsigned ob = P.off0 + oy * P.pitch + (unsigned)ox0 * NDW;
    const unsigned shift1 = P.off1 - P.off0;
    unsigned char *cur = frame + ob;
    if (fill != own) {   // the wedge's edge: covered pixels (and those with a non-finite coordinate) keep the warp's bytes
        unsigned mask[NDW];
#pragma unroll
        for (int k = 0; k < NDW; ++k) {
            mask[k] = 0u;
#pragma unroll
            for (int b = 0; b < 4; ++b) mask[k] |= (fill >> ((4 * k + b) / NDW)) & 1u ? 0xffu << (8 * b) : 0u;   // byte 4 k + b: pixel (4 k + b) / NDW
        }
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            unsigned c[NDW];
            load_lane<NDW, BYTES>(cur + (p ? shift1 : 0u), full, c);
#pragma unroll
            for (int k = 0; k < NDW; ++k) res[p][k] = (res[p][k] & mask[k]) | (c[k] & ~mask[k]);
        }
    }
#pragma unroll
    for (int p = 0; p < NP; ++p) store_lane<NDW, BYTES>(cur + (p ? shift1 : 0u), full, res[p]);
}

template <bool BICUBIC>
__global__ void __launch_bounds__(256) edge_u8_kernel(unsigned char *frames, const unsigned char *__restrict__ source, const float *__restrict__ field,
                                                      yuv::Plane P, int fmode, int fh, int fw, unsigned fbytes, int swap, int mirror) {
    const unsigned rg = xcd_remap(blockIdx.x, gridDim.x);
    const unsigned oy = __builtin_amdgcn_readfirstlane(rg * 4u + (threadIdx.x >> 6));
    if (rg >= P.nrg || oy >= (unsigned)P.h) return;
    const int ox0 = (int)(blockIdx.y * 256u + (threadIdx.x & 63u) * 4u);
    const size_t fo = (size_t)blockIdx.z * fbytes;
    edge_row<PLANE_BGR, 1, 0, BICUBIC>(frames + fo, source + fo, field, P, fmode, blockIdx.z, oy, ox0, fh, fw, swap != 0, mirror != 0);
}

template <int SB, int LAYOUT, bool BICUBIC>   // SB 1: LAYOUT 0 NV12, 1 I420 and their 4:2:2 / 4:4:4 kin; SB 2: 0 P010, 1 I010 and theirs
__global__ void __launch_bounds__(256) edge_yuv_kernel(unsigned char *frames, const unsigned char *__restrict__ source, const float *__restrict__ field,
                                                       yuv::Plane py, yuv::Plane pc, int fmy, int fmc, int fh, int fw, unsigned fbytes, int mirror) {
    const unsigned rg = xcd_remap(blockIdx.x, gridDim.x);
    const int ox0 = (int)(blockIdx.y * 256u + (threadIdx.x & 63u) * 4u);
    const size_t fo = (size_t)blockIdx.z * fbytes;
    if (rg < py.nrg) {
        const unsigned oy = __builtin_amdgcn_readfirstlane(rg * 4u + (threadIdx.x >> 6));
        if (oy >= (unsigned)py.h || blockIdx.y * 256u >= (unsigned)py.w) return;
        edge_row<yuv::PLANE_Y, SB, LAYOUT, BICUBIC>(frames + fo, source + fo, field, py, fmy, blockIdx.z, oy, ox0, fh, fw, false, mirror != 0);
    } else if (rg < py.nrg + pc.nrg) {
        const unsigned oy = __builtin_amdgcn_readfirstlane((rg - py.nrg) * 4u + (threadIdx.x >> 6));
        if (oy >= (unsigned)pc.h || blockIdx.y * 256u >= (unsigned)pc.w) return;
        edge_row<LAYOUT == 0 ? yuv::PLANE_NV12_UV : yuv::PLANE_I420_UV, SB, LAYOUT, BICUBIC>(frames + fo, source + fo, field, pc, fmc, blockIdx.z, oy, ox0,
                                                                                             fh, fw, false, mirror != 0);
    }
}

// what the three entries check alike: the edge mode, and that the n frames of `source` do not overlap the n of `frames`
static int check_mode(const char *what, int edge) {
    PWS_REQUIRE(edge == 1 || edge == 2, "%s: edge must be 1 (clamp) or 2 (mirror), got %d", what, edge);
    return PWS_OK;
}
static int check_overlap(const char *what, const void *frames, const void *source, int n, size_t fbytes) {
    const size_t a = reinterpret_cast<size_t>(frames), b = reinterpret_cast<size_t>(source), len = (size_t)n * fbytes;
    PWS_REQUIRE(a + len <= b || b + len <= a, "%s: source must not overlap frames", what);
    return PWS_OK;
}

template <int SB, int LAYOUT>
static void launch(const yuv::LaunchYuv &L, int n, int bicubic, pws_stream_t stream, unsigned char *fr, const unsigned char *src, const float *field, int fh,
                   int fw, int mirror) {
    const dim3 grid(L.gx, L.cpr, (unsigned)n);
    if (bicubic)
        hipLaunchKernelGGL((edge_yuv_kernel<SB, LAYOUT, true>), grid, dim3(256), 0, as_stream(stream), fr, src, field, L.py, L.pc, L.fmy, L.fmc, fh, fw,
                           L.fbytes, mirror);
    else
        hipLaunchKernelGGL((edge_yuv_kernel<SB, LAYOUT, false>), grid, dim3(256), 0, as_stream(stream), fr, src, field, L.py, L.pc, L.fmy, L.fmc, fh, fw,
                           L.fbytes, mirror);
}

// SB: bytes per sample; chroma: 0 4:2:0, 1 4:2:2, 2 4:4:4.  Checks and plane geometry are the warps' (yuv::launch_yuv), as in border_keep.hip:
// folded taps lie inside their plane of source frame t, a lane writes its own 4 pixels of frame t.
template <int SB>
static int edge_yuv(const char *what, void *frames, const void *source, const float *field, int n, int h, int w, int fh, int fw, int layout, int chroma,
                    int align_corners, int bicubic, int edge, pws_stream_t stream) {
    int rc = check_mode(what, edge);
    if (rc != PWS_OK) return rc;
    yuv::LaunchYuv L;
    rc = yuv::launch_yuv<SB>(what, frames, field, source, "source", n, h, w, fh, fw, layout, chroma, align_corners, bicubic ? 4 : 0,
                                 "with the bicubic margin", L);
    if (rc != PWS_OK || n == 0) return rc;
    rc = check_overlap(what, frames, source, n, L.fbytes);
    if (rc != PWS_OK) return rc;
    unsigned char *fr = reinterpret_cast<unsigned char *>(frames);
    const unsigned char *src = reinterpret_cast<const unsigned char *>(source);
    if (layout == 0) launch<SB, 0>(L, n, bicubic, stream, fr, src, field, fh, fw, edge == 2);
    else launch<SB, 1>(L, n, bicubic, stream, fr, src, field, fh, fw, edge == 2);
    return check_launch("edge_yuv_kernel");
}

}  // namespace edge
}  // namespace pws

using namespace pws;

extern "C" int pws_border_edge_u8(unsigned char *frames_hwc, const unsigned char *source_hwc, const float *field, int n, int h, int w, int fh, int fw,
                                  int swap_rb, int align_corners, int bicubic, int edge, pws_stream_t stream) {
    const char *what = "pws_border_edge_u8";
    int rc = edge::check_mode(what, edge);
    if (rc != PWS_OK) return rc;
    PWS_REQUIRE(n >= 0 && h > 0 && w > 0 && fh > 0 && fw > 0, "pws_border_edge_u8: bad shape");
    PWS_REQUIRE((size_t)h * w < (1u << 29) && w >= 4 && w % 4 == 0, "pws_border_edge_u8: w must be a multiple of 4 (got %d)", w);
    if (n == 0) return PWS_OK;
    PWS_REQUIRE(frames_hwc && field && source_hwc, "pws_border_edge_u8: NULL pointer");
    PWS_REQUIRE(((reinterpret_cast<size_t>(frames_hwc) | reinterpret_cast<size_t>(source_hwc)) & 3) == 0,
                "pws_border_edge_u8: frames and source must be 4-byte aligned");
    const unsigned cpr = (unsigned)((w + 255) / 256);
    PWS_REQUIRE(n < 65536 && cpr < 65536 && (size_t)w * 3 < (1u << 24) && h < (1 << 24), "pws_border_edge_u8: frame or batch too large");
    const yuv::Plane P = yuv::make_plane(h, w, 0u, 0u, 3u * (unsigned)w, fh, fw, align_corners);
    const unsigned gx = (P.nrg + 7u) & ~7u, fbytes = (unsigned)((size_t)h * w * 3);
    rc = edge::check_overlap(what, frames_hwc, source_hwc, n, fbytes);
    if (rc != PWS_OK) return rc;
    const dim3 grid(gx, cpr, (unsigned)n);
    if (bicubic)
        hipLaunchKernelGGL(edge::edge_u8_kernel<true>, grid, dim3(256), 0, as_stream(stream), frames_hwc, source_hwc, field, P, yuv_fmode(P.rx), fh, fw,
                           fbytes, swap_rb, edge == 2);
    else
        hipLaunchKernelGGL(edge::edge_u8_kernel<false>, grid, dim3(256), 0, as_stream(stream), frames_hwc, source_hwc, field, P, yuv_fmode(P.rx), fh, fw,
                           fbytes, swap_rb, edge == 2);
    return check_launch("edge_u8_kernel");
}

extern "C" int pws_border_edge_yuv_u8(unsigned char *frames, const unsigned char *source, const float *field, int n, int h, int w, int fh, int fw,
                                      int layout, int chroma, int align_corners, int bicubic, int edge, pws_stream_t stream) {
    return edge::edge_yuv<1>("pws_border_edge_yuv_u8", frames, source, field, n, h, w, fh, fw, layout, chroma, align_corners, bicubic, edge, stream);
}

extern "C" int pws_border_edge_yuv_u16(unsigned short *frames, const unsigned short *source, const float *field, int n, int h, int w, int fh, int fw,
                                       int layout, int chroma, int align_corners, int bicubic, int edge, pws_stream_t stream) {
    return edge::edge_yuv<2>("pws_border_edge_yuv_u16", frames, source, field, n, h, w, fh, fw, layout, chroma, align_corners, bicubic, edge, stream);
}
