// "Mosaic" borders for the fused warps (grid_sample.hip, warp_bicubic.hip): an output pixel whose taps do not all lie inside the source takes
// the value of the temporally nearest warped frame of its scene that does cover the position, at most `radius` frames into the past or the
// future, instead of the blend with the pad colour the warp wrote.
//
// Definition (restated in tests/mosaic_ref.py).  Planes, source positions and coverage are border_keep.hip's: (ix, iy) is formed with the
// warps' fp32 operations (warp_common.h: yuv_field4, then one fma with the plane's un-normalisation constants); a position is covered iff
// m <= ix <= W-1-m and m <= iy <= H-1-m, m = 0 for the bilinear warp, 1 for the bicubic one; NaN is not covered.  With W[t] the frames as the
// black-border warp wrote them, C[t] their coverage, frames 0 .. n-1 one scene and R the radius (1 .. 15), position p of frame t:
//   C[t][p]:   out[t][p] = W[t][p] (untouched);
//   otherwise: k = 1 .. R in this order -- t-k >= 0 and C[t-k][p]: out[t][p] = W[t-k][p] (the past wins a tie); else t+k < n and C[t+k][p]:
//              out[t][p] = W[t+k][p];
//   no donor within R: out[t][p] = W[t][p], and the position counts as unfilled.
// Coverage is binary, every output sample is a copy of one existing sample, donors are read only where they are covered and covered samples
// are never modified: the pass runs in place, a frame that has been filled is as good a donor as one that has not, and frames [start, stop)
// depend on frames [start-R, stop+R) of the scene alone.
//
// Launch shape: keep_row's -- a wave owns 256 consecutive positions of ONE plane row, a lane 4 of them, in EVERY frame, and walks the frames in
// order; one launch covers all planes.  Step s forms the coverage of frame s (the field's row pair is fetched once per wave where the
// plane's width allows it: the loop over s is wave-uniform) and shifts it into one 32-bit window per pixel: after step s bit j is the coverage
// of frame s-2R+j, so bit R is frame t = s-R, bits below it the past, bits above it the future; frames outside [0, n) shift in as 0.  Then
// frame t is finished if start <= t < stop: for an uncovered pixel the nearest set bit on either side names the donor frame; the lane loads
// its bytes of each of its 4 pixels' frames (frame t itself for a pixel that stays), four independent loads, takes each pixel's bytes from
// its own and stores.  Lanes without an uncovered pixel
// that has a donor touch no frame.  Traffic is the fields once, plus the wedges and their donors, not the frames.  A lane reads and writes its
// own 4 pixels only.  Per frame the Y plane's (BGR: the pixels') positions without a donor are counted with a ballot per pixel slot and added
// to unfilled[t - start] by the wave's first lane.
#include "common.h"
#include "warp_common.h"
#include "border_lane.h"

namespace pws {
namespace mosaic {

using keep::PLANE_BGR;
using keep::load_lane;
using keep::store_lane;

// One wave's row chunk of one plane kind through the frames.  SB: bytes per sample.  COUNT: this plane's unfilled positions are counted.
template <int KIND, int SB>
__device__ __forceinline__ void mosaic_row(unsigned char *frames, const float *__restrict__ field, int *unfilled, const yuv::Plane &P, int fmode, int n,
                                           int start, int stop, int R, unsigned oy, int ox0, int fh, int fw, size_t fbytes, float m) {
    constexpr int NCI = KIND == PLANE_BGR ? 3 : (KIND == yuv::PLANE_NV12_UV ? 2 : 1), NP = KIND == yuv::PLANE_I420_UV ? 2 : 1;
    constexpr int NDW = NCI * SB;   // dwords of a lane's 4 pixels in one source plane = bytes per pixel
    constexpr bool BYTES = KIND == yuv::PLANE_I420_UV && SB == 1;
    constexpr bool COUNT = KIND == PLANE_BGR || KIND == yuv::PLANE_Y;
    const int W = P.w;
    const bool active = ox0 < W;
    if (fmode < 2 && !active) return;   // (modes 2 / 3: every lane fetches and serves field columns)
    const bool full = ox0 + 4 <= W;     // chroma rows of width 2 mod 4: the row's last lane owns 2 pixels
    const unsigned own = !active ? 0u : (full ? 0xfu : 0x3u);
    const unsigned ob = P.off0 + oy * P.pitch + (unsigned)ox0 * NDW;
    const unsigned shift1 = P.off1 - P.off0;
    const float xhi = (float)(W - 1) - m, yhi = (float)(P.h - 1) - m;
    const int lo = max(start - R, 0), hi = min(stop + R, n);   // the frames whose coverage matters
    const unsigned pastmask = (1u << R) - 1u;
    unsigned win[4] = {0u, 0u, 0u, 0u};
    for (int s = lo; s < stop + R; ++s) {   // (wave-uniform: s, lo, hi, start, stop, R are)
        unsigned cov = 0u;
        if (s < hi) {
            f32x2 gx[2], gy[2];
            if (fmode == 2) yuv_field4<2>(field, (unsigned)s, oy, ox0, W - 1, fh, fw, P.ry, P.rx, gx, gy);
            else if (fmode == 3) yuv_field4<3>(field, (unsigned)s, oy, ox0, W - 1, fh, fw, P.ry, P.rx, gx, gy);
            else yuv_field4<0>(field, (unsigned)s, oy, ox0, W - 1, fh, fw, P.ry, P.rx, gx, gy);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float g0 = i & 1 ? gx[i >> 1].y : gx[i >> 1].x, g1 = i & 1 ? gy[i >> 1].y : gy[i >> 1].x;
                const float ix = fmaf(g0, P.kx, P.kx1), iy = fmaf(g1, P.ky, P.ky1);   // (the warps' pk_fma, per component)
                const bool covered = ix >= m && ix <= xhi && iy >= m && iy <= yhi;    // (false for NaN)
                cov |= covered ? 1u << i : 0u;
            }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) win[i] = (win[i] >> 1) | (((cov >> i) & 1u) << (2 * R));
        const int t = s - R;
        if (t < start) continue;
        unsigned unc = 0u;
#pragma unroll
        for (int i = 0; i < 4; ++i) unc |= ((win[i] >> R) & 1u) == 0u ? 1u << i : 0u;
        unc &= own;
        // the donor of each uncovered pixel: -k / +k frames; `none` where no frame within R covers it
        int donor[4] = {0, 0, 0, 0};
        unsigned fill = 0u, none = 0u;
        if (unc != 0u) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const unsigned past = win[i] & pastmask, future = win[i] >> (R + 1);
                const int kp = past ? R - (31 - __clz((int)past)) : 64, kf = future ? __ffs((int)future) : 64;
                donor[i] = kp <= kf ? -kp : kf;
                fill |= (kp < 64 || kf < 64) ? 1u << i : 0u;
            }
            none = unc & ~fill, fill &= unc;
        }
        if constexpr (COUNT) {
            if (__any(none != 0u)) {   // (wave-uniform)
                int cnt = 0;
#pragma unroll
                for (int i = 0; i < 4; ++i) cnt += __popcll(__ballot((none >> i) & 1u));
                if ((threadIdx.x & 63u) == 0u) atomicAdd(unfilled + (t - start), cnt);   // (lane 0 of a launched chunk is active)
            }
        }
        if (fill != 0u) {
            unsigned char *cur = frames + (size_t)t * fbytes + ob;
            // pixel i takes its bytes from frame t + d_i, d_i = 0 for the pixels that stay: four independent loads, all in flight at once
            // (a chain of dependent ones made the wedge's waves the launch's critical path)
            unsigned out[NP][NDW], don[4][NP][NDW];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int d = (fill >> i) & 1u ? donor[i] : 0;
                const unsigned char *src = frames + (size_t)(t + d) * fbytes + ob;
#pragma unroll
                for (int p = 0; p < NP; ++p) load_lane<NDW, BYTES>(src + (p ? shift1 : 0u), full, don[i][p]);
            }
#pragma unroll
            for (int p = 0; p < NP; ++p)
#pragma unroll
                for (int k = 0; k < NDW; ++k) {
                    unsigned v = 0u;
#pragma unroll
                    for (int b = 0; b < 4; ++b) v |= don[(4 * k + b) / NDW][p][k] & (0xffu << (8 * b));   // byte 4 k + b: pixel (4 k + b) / NDW
                    out[p][k] = v;
                }
#pragma unroll
            for (int p = 0; p < NP; ++p) store_lane<NDW, BYTES>(cur + (p ? shift1 : 0u), full, out[p]);
        }
    }
}

__global__ void __launch_bounds__(256) mosaic_u8_kernel(unsigned char *frames, const float *__restrict__ field, int *unfilled, yuv::Plane P, int fmode,
                                                        int n, int start, int stop, int R, int fh, int fw, unsigned fbytes, float m) {
    const unsigned rg = xcd_remap(blockIdx.x, gridDim.x);
    const unsigned oy = __builtin_amdgcn_readfirstlane(rg * 4u + (threadIdx.x >> 6));
    if (rg >= P.nrg || oy >= (unsigned)P.h) return;
    const int ox0 = (int)(blockIdx.y * 256u + (threadIdx.x & 63u) * 4u);
    mosaic_row<PLANE_BGR, 1>(frames, field, unfilled, P, fmode, n, start, stop, R, oy, ox0, fh, fw, fbytes, m);
}

template <int SB, int LAYOUT>   // SB 1: LAYOUT 0 NV12, 1 I420 and their 4:2:2 / 4:4:4 kin; SB 2: 0 P010, 1 I010 and theirs
__global__ void __launch_bounds__(256) mosaic_yuv_kernel(unsigned char *frames, const float *__restrict__ field, int *unfilled, yuv::Plane py,
                                                         yuv::Plane pc, int fmy, int fmc, int n, int start, int stop, int R, int fh, int fw,
                                                         unsigned fbytes, float m) {
    const unsigned rg = xcd_remap(blockIdx.x, gridDim.x);
    const int ox0 = (int)(blockIdx.y * 256u + (threadIdx.x & 63u) * 4u);
    if (rg < py.nrg) {
        const unsigned oy = __builtin_amdgcn_readfirstlane(rg * 4u + (threadIdx.x >> 6));
        if (oy >= (unsigned)py.h || blockIdx.y * 256u >= (unsigned)py.w) return;
        mosaic_row<yuv::PLANE_Y, SB>(frames, field, unfilled, py, fmy, n, start, stop, R, oy, ox0, fh, fw, fbytes, m);
    } else if (rg < py.nrg + pc.nrg) {
        const unsigned oy = __builtin_amdgcn_readfirstlane((rg - py.nrg) * 4u + (threadIdx.x >> 6));
        if (oy >= (unsigned)pc.h || blockIdx.y * 256u >= (unsigned)pc.w) return;
        mosaic_row<LAYOUT == 0 ? yuv::PLANE_NV12_UV : yuv::PLANE_I420_UV, SB>(frames, field, unfilled, pc, fmc, n, start, stop, R, oy, ox0, fh, fw,
                                                                              fbytes, m);
    }
}

// what the three entries check alike, before the format's own rules
static int check_range(const char *what, const void *unfilled, int n, int start, int stop, int radius) {
    PWS_REQUIRE(radius >= 1 && radius <= 15, "%s: radius must be 1 .. 15 (one window bit per frame, 2 radius + 1 of them), got %d", what, radius);
    PWS_REQUIRE(0 <= start && start <= stop && stop <= n, "%s: the range must satisfy 0 <= start <= stop <= n, got [%d, %d) of %d", what, start, stop, n);
    PWS_REQUIRE(stop == start || unfilled, "%s: NULL pointer", what);
    PWS_REQUIRE((reinterpret_cast<size_t>(unfilled) & 3) == 0, "%s: unfilled must be 4-byte aligned", what);
    return PWS_OK;
}

// unfilled[0 .. count) = 0 on the stream, ahead of the pass that adds to it
__global__ void __launch_bounds__(256) clear_kernel(int *p, int count) {
    for (int i = (int)threadIdx.x; i < count; i += 256) p[i] = 0;
}

static int clear_unfilled(const char *what, int *unfilled, int count, pws_stream_t stream) {
    hipLaunchKernelGGL(clear_kernel, dim3(1), dim3(256), 0, as_stream(stream), unfilled, count);
    return check_launch("mosaic::clear_kernel");
}

// SB: bytes per sample; chroma: 0 4:2:0, 1 4:2:2, 2 4:4:4.  Checks and plane geometry are the warps' (yuv::launch_yuv), as in border_keep.hip.
template <int SB>
static int mosaic_yuv(const char *what, void *frames, const float *field, int *unfilled, int n, int start, int stop, int radius, int h, int w, int fh,
                      int fw, int layout, int chroma, int align_corners, int bicubic, pws_stream_t stream) {
    int rc = check_range(what, unfilled, n, start, stop, radius);
    if (rc != PWS_OK) return rc;
    yuv::LaunchYuv L;
    rc = yuv::launch_yuv<SB>(what, frames, field, frames, "frames", n, h, w, fh, fw, layout, chroma, align_corners, bicubic ? 4 : 0,
                             "with the bicubic margin", L);
    if (rc != PWS_OK || n == 0 || start == stop) return rc;
    rc = clear_unfilled(what, unfilled, stop - start, stream);
    if (rc != PWS_OK) return rc;
    const float m = bicubic ? 1.f : 0.f;
    unsigned char *fr = reinterpret_cast<unsigned char *>(frames);
    if (layout == 0)
        hipLaunchKernelGGL((mosaic::mosaic_yuv_kernel<SB, 0>), dim3(L.gx, L.cpr, 1), dim3(256), 0, as_stream(stream), fr, field, unfilled, L.py, L.pc,
                           L.fmy, L.fmc, n, start, stop, radius, fh, fw, L.fbytes, m);
    else
        hipLaunchKernelGGL((mosaic::mosaic_yuv_kernel<SB, 1>), dim3(L.gx, L.cpr, 1), dim3(256), 0, as_stream(stream), fr, field, unfilled, L.py, L.pc,
                           L.fmy, L.fmc, n, start, stop, radius, fh, fw, L.fbytes, m);
    return check_launch("mosaic_yuv_kernel");
}

}  // namespace mosaic
}  // namespace pws

using namespace pws;

extern "C" int pws_border_mosaic_u8(unsigned char *frames_hwc, const float *field, int *unfilled, int n, int start, int stop, int radius, int h, int w,
                                    int fh, int fw, int align_corners, int bicubic, pws_stream_t stream) {
    const char *what = "pws_border_mosaic_u8";
    int rc = mosaic::check_range(what, unfilled, n, start, stop, radius);
    if (rc != PWS_OK) return rc;
    PWS_REQUIRE(n >= 0 && h > 0 && w > 0 && fh > 0 && fw > 0, "pws_border_mosaic_u8: bad shape");
    PWS_REQUIRE((size_t)h * w < (1u << 29) && w >= 4 && w % 4 == 0, "pws_border_mosaic_u8: w must be a multiple of 4 (got %d)", w);
    if (n == 0 || start == stop) return PWS_OK;
    PWS_REQUIRE(frames_hwc && field, "pws_border_mosaic_u8: NULL pointer");
    PWS_REQUIRE((reinterpret_cast<size_t>(frames_hwc) & 3) == 0, "pws_border_mosaic_u8: frames must be 4-byte aligned");
    const unsigned cpr = (unsigned)((w + 255) / 256);
    PWS_REQUIRE(n < 65536 && cpr < 65536 && (size_t)w * 3 < (1u << 24) && h < (1 << 24), "pws_border_mosaic_u8: frame or batch too large");
    rc = mosaic::clear_unfilled(what, unfilled, stop - start, stream);
    if (rc != PWS_OK) return rc;
    const yuv::Plane P = yuv::make_plane(h, w, 0u, 0u, 3u * (unsigned)w, fh, fw, align_corners);
    const unsigned gx = (P.nrg + 7u) & ~7u, fbytes = (unsigned)((size_t)h * w * 3);
    hipLaunchKernelGGL(mosaic::mosaic_u8_kernel, dim3(gx, cpr, 1), dim3(256), 0, as_stream(stream), frames_hwc, field, unfilled, P, yuv_fmode(P.rx), n,
                       start, stop, radius, fh, fw, fbytes, bicubic ? 1.f : 0.f);
    return check_launch("mosaic_u8_kernel");
}

extern "C" int pws_border_mosaic_yuv_u8(unsigned char *frames, const float *field, int *unfilled, int n, int start, int stop, int radius, int h, int w,
                                        int fh, int fw, int layout, int chroma, int align_corners, int bicubic, pws_stream_t stream) {
    return mosaic::mosaic_yuv<1>("pws_border_mosaic_yuv_u8", frames, field, unfilled, n, start, stop, radius, h, w, fh, fw, layout, chroma, align_corners,
                                 bicubic, stream);
}

extern "C" int pws_border_mosaic_yuv_u16(unsigned short *frames, const float *field, int *unfilled, int n, int start, int stop, int radius, int h,
                                         int w, int fh, int fw, int layout, int chroma, int align_corners, int bicubic, pws_stream_t stream) {
    return mosaic::mosaic_yuv<2>("pws_border_mosaic_yuv_u16", frames, field, unfilled, n, start, stop, radius, h, w, fh, fw, layout, chroma, align_corners,
                                 bicubic, stream);
}
