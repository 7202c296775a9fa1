// "Keep" borders for the fused warps (grid_sample.hip, warp_bicubic.hip): an output pixel whose taps do not all lie inside the source keeps
// the value the previous OUTPUT frame of its scene had there, instead of the blend with the pad colour the warp wrote.
//
// Definition (restated in tests/keep_ref.py).  For a plane of H x W samples and frame t the source position (ix, iy) of a pixel is formed
// with the warps' fp32 operations (warp_common.h: yuv_field4, then one fma with the plane's un-normalisation constants), so the warp and the
// coverage agree on it bit for bit.  A pixel is covered iff m <= ix <= W-1-m and m <= iy <= H-1-m, m = 0 for the bilinear warp (4 taps inside),
// 1 for the bicubic one (16 taps inside); a NaN coordinate is not covered.  out[t] = covered ? warped[t] : out[t-1], and out[-1] is the
// `initial` frame: an earlier output frame, taken as it is, or -- `initial_is_source` -- a source frame read as the warp would write it
// (swap_rb for BGR, P010 words masked to v10 << 6, I010 words clamped to 1023).  Coverage is binary: every output sample is a copy of one of
// two existing samples, there is no arithmetic on samples and nothing that could drift along the recurrence.
//
// Launch shape: the warps' -- a wave owns 256 consecutive pixels of ONE plane row, a lane 4 of them, in EVERY frame of the segment, and walks
// t in order; one launch covers all planes.  Per frame a lane forms its 4 coordinates (the field's row pair is fetched once per wave where
// the plane's width allows it) and does nothing else while they are covered.  For an uncovered pixel it needs out[t-1]: the register it
// stored at t-1, or -- if frame t-1 was covered in all 4 pixels and is therefore final in memory as the warp left it -- a load from there.
// The current frame's bytes are loaded only by lanes with BOTH kinds of pixel (the wedge's edge), merged and stored; a lane with 4 uncovered
// pixels stores its registers.  Traffic is the fields plus the wedges, not the frames.  A lane reads and writes its own 4 pixels only.
#include "common.h"
#include "warp_common.h"
#include "border_lane.h"

namespace pws {
namespace keep {

// a source frame's bytes as the warp would write them
template <int KIND, int SB, int LAYOUT, int NDW>
__device__ __forceinline__ void as_written(unsigned d[NDW], bool swap) {
    if constexpr (KIND == PLANE_BGR) {
        if (swap) {   // output channel c is input channel 2 - c: byte 3 i + c of the lane's 12 takes byte 3 i + 2 - c
            unsigned o[3] = {0u, 0u, 0u};
#pragma unroll
            for (int b = 0; b < 12; ++b) {
                const int s = b / 3 * 3 + 2 - b % 3;
                o[b >> 2] |= ((d[s >> 2] >> (8 * (s & 3))) & 0xffu) << (8 * (b & 3));
            }
            d[0] = o[0], d[1] = o[1], d[2] = o[2];
        }
    } else if constexpr (SB == 2) {
#pragma unroll
        for (int k = 0; k < NDW; ++k) {
            if constexpr (LAYOUT == 0) d[k] &= 0xffc0ffc0u;                                     // P010: v10 << 6
            else d[k] = min(d[k] & 0xffffu, 1023u) | min(d[k] >> 16, 1023u) << 16;              // I010: min(word, 1023)
        }
    }
}

// One wave's row chunk of one plane kind through the T frames of the segment.  SB: bytes per sample; LAYOUT (SB 2): 0 P010, 1 I010.
template <int KIND, int SB, int LAYOUT>
__device__ __forceinline__ void keep_row(unsigned char *frames, const float *__restrict__ field, const unsigned char *initial, const yuv::Plane &P,
                                         int fmode, int T, unsigned oy, int ox0, int fh, int fw, size_t fbytes, bool source, bool swap, float m) {
    constexpr int NCI = KIND == PLANE_BGR ? 3 : (KIND == yuv::PLANE_NV12_UV ? 2 : 1), NP = KIND == yuv::PLANE_I420_UV ? 2 : 1;
    constexpr int NDW = NCI * SB;   // dwords of a lane's 4 pixels in one source plane = bytes per pixel
    constexpr bool BYTES = KIND == yuv::PLANE_I420_UV && SB == 1;
    const int W = P.w;
    const bool active = ox0 < W;
    if (fmode < 2 && !active) return;   // (modes 2 / 3: every lane fetches and serves field columns)
    const bool full = ox0 + 4 <= W;     // chroma rows of width 2 mod 4: the row's last lane owns 2 pixels
    const unsigned own = !active ? 0u : (full ? 0xfu : 0x3u);
    const unsigned ob = P.off0 + oy * P.pitch + (unsigned)ox0 * NDW;
    const unsigned shift1 = P.off1 - P.off0;
    const float xhi = (float)(W - 1) - m, yhi = (float)(P.h - 1) - m;
    unsigned prev[NP][NDW];   // out[t-1] of the lane's pixels, valid while `have`
#pragma unroll
    for (int p = 0; p < NP; ++p)
#pragma unroll
        for (int k = 0; k < NDW; ++k) prev[p][k] = 0u;
    bool have = false;
    for (int t = 0; t < T; ++t) {
        f32x2 gx[2], gy[2];
        if (fmode == 2) yuv_field4<2>(field, (unsigned)t, oy, ox0, W - 1, fh, fw, P.ry, P.rx, gx, gy);
        else if (fmode == 3) yuv_field4<3>(field, (unsigned)t, oy, ox0, W - 1, fh, fw, P.ry, P.rx, gx, gy);
        else yuv_field4<0>(field, (unsigned)t, oy, ox0, W - 1, fh, fw, P.ry, P.rx, gx, gy);
        unsigned unc = 0u;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float g0 = i & 1 ? gx[i >> 1].y : gx[i >> 1].x, g1 = i & 1 ? gy[i >> 1].y : gy[i >> 1].x;
            const float ix = fmaf(g0, P.kx, P.kx1), iy = fmaf(g1, P.ky, P.ky1);   // (the warps' pk_fma, per component)
            const bool covered = ix >= m && ix <= xhi && iy >= m && iy <= yhi;    // (false for NaN)
            unc |= covered ? 0u : 1u << i;
        }
        unc &= own;
        if (unc != 0u) {
            unsigned char *cur = frames + (size_t)t * fbytes + ob;
            if (!have) {
                const unsigned char *src = t == 0 ? initial + ob : cur - fbytes;
    #pragma unroll
                for (int p = 0; p < NP; ++p) {
                    load_lane<NDW, BYTES>(src + (p ? shift1 : 0u), full, prev[p]);
                    if (t == 0 && source) as_written<KIND, SB, LAYOUT, NDW>(prev[p], swap);
                }
            }
            if (unc != own) {   // the wedge's edge: covered pixels keep the warp's bytes
                unsigned mask[NDW];
    #pragma unroll
                for (int k = 0; k < NDW; ++k) {
                    mask[k] = 0u;
    #pragma unroll
                    for (int b = 0; b < 4; ++b) mask[k] |= (unc >> ((4 * k + b) / NDW)) & 1u ? 0xffu << (8 * b) : 0u;   // byte 4 k + b: pixel (4 k + b) / NDW
                }
    #pragma unroll
                for (int p = 0; p < NP; ++p) {
                    unsigned c[NDW];
                    load_lane<NDW, BYTES>(cur + (p ? shift1 : 0u), full, c);
    #pragma unroll
                    for (int k = 0; k < NDW; ++k) prev[p][k] = (prev[p][k] & mask[k]) | (c[k] & ~mask[k]);
                }
            }
    #pragma unroll
            for (int p = 0; p < NP; ++p) store_lane<NDW, BYTES>(cur + (p ? shift1 : 0u), full, prev[p]);
            have = true;
        } else {
            have = false;   // frame t is final as the warp wrote it: a later frame reads it from memory
        }
    }
}

__global__ void __launch_bounds__(256) keep_u8_kernel(unsigned char *frames, const float *__restrict__ field, const unsigned char *initial,
                                                      yuv::Plane P, int fmode, int T, int fh, int fw, unsigned fbytes, int source, int swap,
                                                      float m) {
    const unsigned rg = xcd_remap(blockIdx.x, gridDim.x);
    const unsigned oy = __builtin_amdgcn_readfirstlane(rg * 4u + (threadIdx.x >> 6));
    if (rg >= P.nrg || oy >= (unsigned)P.h) return;
    const int ox0 = (int)(blockIdx.y * 256u + (threadIdx.x & 63u) * 4u);
    keep_row<PLANE_BGR, 1, 0>(frames, field, initial, P, fmode, T, oy, ox0, fh, fw, fbytes, source != 0, swap != 0, m);
}

template <int SB, int LAYOUT>   // SB 1: LAYOUT 0 NV12, 1 I420; SB 2: 0 P010, 1 I010
__global__ void __launch_bounds__(256) keep_yuv420_kernel(unsigned char *frames, const float *__restrict__ field, const unsigned char *initial,
                                                          yuv::Plane py, yuv::Plane pc, int fmy, int fmc, int T, int fh, int fw, unsigned fbytes,
                                                          int source, float m) {
    const unsigned rg = xcd_remap(blockIdx.x, gridDim.x);
    const int ox0 = (int)(blockIdx.y * 256u + (threadIdx.x & 63u) * 4u);
    if (rg < py.nrg) {
        const unsigned oy = __builtin_amdgcn_readfirstlane(rg * 4u + (threadIdx.x >> 6));
        if (oy >= (unsigned)py.h || blockIdx.y * 256u >= (unsigned)py.w) return;
        keep_row<yuv::PLANE_Y, SB, LAYOUT>(frames, field, initial, py, fmy, T, oy, ox0, fh, fw, fbytes, source != 0, false, m);
    } else if (rg < py.nrg + pc.nrg) {
        const unsigned oy = __builtin_amdgcn_readfirstlane((rg - py.nrg) * 4u + (threadIdx.x >> 6));
        if (oy >= (unsigned)pc.h || blockIdx.y * 256u >= (unsigned)pc.w) return;
        keep_row<LAYOUT == 0 ? yuv::PLANE_NV12_UV : yuv::PLANE_I420_UV, SB, LAYOUT>(frames, field, initial, pc, fmc, T, oy, ox0, fh, fw, fbytes,
                                                                                   source != 0, false, m);
    }
}

// SB: bytes per sample; chroma: 0 4:2:0, 1 4:2:2, 2 4:4:4.  Checks and plane geometry are the warps' (yuv::launch_yuv; with the bicubic margin
// a chroma plane is 4 samples wide or more, as the bicubic warps ask: w >= 8, at 4:4:4 any valid w).  A lane touches its own 4 pixels alone.
template <int SB>
static int keep_yuv(const char *what, void *frames, const float *field, const void *initial, int initial_is_source, int n, int h, int w, int fh,
                    int fw, int layout, int chroma, int align_corners, int bicubic, pws_stream_t stream) {
    yuv::LaunchYuv L;
    const int rc = yuv::launch_yuv<SB>(what, frames, field, initial, "initial", n, h, w, fh, fw, layout, chroma, align_corners, bicubic ? 4 : 0,
                                       "with the bicubic margin", L);
    if (rc != PWS_OK || n == 0) return rc;
    const float m = bicubic ? 1.f : 0.f;
    unsigned char *fr = reinterpret_cast<unsigned char *>(frames);
    const unsigned char *ini = reinterpret_cast<const unsigned char *>(initial);
    if (layout == 0)
        hipLaunchKernelGGL((keep::keep_yuv420_kernel<SB, 0>), dim3(L.gx, L.cpr, 1), dim3(256), 0, as_stream(stream), fr, field, ini, L.py, L.pc, L.fmy,
                           L.fmc, n, fh, fw, L.fbytes, initial_is_source, m);
    else
        hipLaunchKernelGGL((keep::keep_yuv420_kernel<SB, 1>), dim3(L.gx, L.cpr, 1), dim3(256), 0, as_stream(stream), fr, field, ini, L.py, L.pc, L.fmy,
                           L.fmc, n, fh, fw, L.fbytes, initial_is_source, m);
    return check_launch("keep_yuv420_kernel");
}

}  // namespace keep
}  // namespace pws

using namespace pws;

extern "C" int pws_border_keep_u8(unsigned char *frames_hwc, const float *field, const unsigned char *initial, int initial_is_source, int n, int h,
                                  int w, int fh, int fw, int swap_rb, int align_corners, int bicubic, pws_stream_t stream) {
    PWS_REQUIRE(n >= 0 && h > 0 && w > 0 && fh > 0 && fw > 0, "pws_border_keep_u8: bad shape");
    PWS_REQUIRE((size_t)h * w < (1u << 29) && w >= 4 && w % 4 == 0, "pws_border_keep_u8: w must be a multiple of 4 (got %d)", w);
    if (n == 0) return PWS_OK;
    PWS_REQUIRE(frames_hwc && field && initial, "pws_border_keep_u8: NULL pointer");
    PWS_REQUIRE(((reinterpret_cast<size_t>(frames_hwc) | reinterpret_cast<size_t>(initial)) & 3) == 0,
                "pws_border_keep_u8: frames and initial must be 4-byte aligned");
    const unsigned cpr = (unsigned)((w + 255) / 256);
    PWS_REQUIRE(n < 65536 && cpr < 65536 && (size_t)w * 3 < (1u << 24) && h < (1 << 24), "pws_border_keep_u8: frame or batch too large");
    const yuv::Plane P = yuv::make_plane(h, w, 0u, 0u, 3u * (unsigned)w, fh, fw, align_corners);
    const unsigned gx = (P.nrg + 7u) & ~7u, fbytes = (unsigned)((size_t)h * w * 3);
    hipLaunchKernelGGL(keep::keep_u8_kernel, dim3(gx, cpr, 1), dim3(256), 0, as_stream(stream), frames_hwc, field, initial, P, yuv_fmode(P.rx), n, fh,
                       fw, fbytes, initial_is_source, swap_rb, bicubic ? 1.f : 0.f);
    return check_launch("keep_u8_kernel");
}

extern "C" int pws_border_keep_yuv420_u8(unsigned char *frames, const float *field, const unsigned char *initial, int initial_is_source, int n, int h,
                                         int w, int fh, int fw, int layout, int align_corners, int bicubic, pws_stream_t stream) {
    return keep::keep_yuv<1>("pws_border_keep_yuv420_u8", frames, field, initial, initial_is_source, n, h, w, fh, fw, layout, 0, align_corners, bicubic,
                             stream);
}

extern "C" int pws_border_keep_yuv_u8(unsigned char *frames, const float *field, const unsigned char *initial, int initial_is_source, int n, int h,
                                      int w, int fh, int fw, int layout, int chroma, int align_corners, int bicubic, pws_stream_t stream) {
    return keep::keep_yuv<1>("pws_border_keep_yuv_u8", frames, field, initial, initial_is_source, n, h, w, fh, fw, layout, chroma, align_corners, bicubic,
                             stream);
}

extern "C" int pws_border_keep_yuv420_u16(unsigned short *frames, const float *field, const unsigned short *initial, int initial_is_source, int n,
                                          int h, int w, int fh, int fw, int layout, int align_corners, int bicubic, pws_stream_t stream) {
    return keep::keep_yuv<2>("pws_border_keep_yuv420_u16", frames, field, initial, initial_is_source, n, h, w, fh, fw, layout, 0, align_corners, bicubic,
                             stream);
}

extern "C" int pws_border_keep_yuv_u16(unsigned short *frames, const float *field, const unsigned short *initial, int initial_is_source, int n,
                                       int h, int w, int fh, int fw, int layout, int chroma, int align_corners, int bicubic, pws_stream_t stream) {
    return keep::keep_yuv<2>("pws_border_keep_yuv_u16", frames, field, initial, initial_is_source, n, h, w, fh, fw, layout, chroma, align_corners, bicubic,
                             stream);
}
