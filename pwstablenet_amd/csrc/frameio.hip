// Frame pre- / post-processing of the reference's video loop on the device (HBM-bound byte kernels), so that only the
// uint8 frames cross PCIe and no per-frame image processing is left on the host:
//   gray_area_u8     cv2.resize(cv2.cvtColor(frame, COLOR_BGR2GRAY), (256, 256), interpolation=INTER_AREA) then
//                    x / 255 * 2 - 1                                   (reference main_new.py:639,653-656,664-667)
//   area_half_u8     cv2.resize(samples, (w/2, h/2), INTER_AREA) + cv2.cvtColor(COLOR_BGR2RGB)   (main_new.py:723-725)
// OpenCV is not in this image, so these follow OpenCV 4.x's documented algorithms and are pinned to a numpy restatement of
// them (oracle/frameio_ref.py), not to cv2 itself ("parity unpinned" against the reference for these two steps):
//   * BGR2GRAY, 8-bit: (B*3735 + G*19235 + R*9798 + 2^14) >> 15                       (imgproc color_rgb: RGB2Gray<uchar>)
//   * INTER_AREA, non-integer ratio: computeResizeAreaTab / ResizeArea_Invoker -- per destination cell the covered source
//     pixels with fractional weights in float, horizontal pass first, rows accumulated in order, saturate_cast<uchar>
//     (round half to even); every product is rounded before it is added (mul_rounded, common.h: no FMA contraction), as the
//     scalar C++ does
//   * INTER_AREA, ratio 2 x 2, 8-bit: (a + b + c + d + 2) >> 2                              (ResizeAreaFastVec_SIMD_8u)
#include "common.h"

namespace pws {

constexpr int AREA_MAX_TAPS = 12;   // source pixels per destination cell and axis (scale <= 10)

// computeResizeAreaTab for ONE destination index d (double arithmetic, float weights), source size ssize, scale = ssize/dsize:
// an optional partially covered first pixel, the fully covered ones sx1 .. sx2-1, an optional partially covered last one.
// Kept as scalars (no per-lane arrays: dynamic indexing would put them in scratch).
struct AreaAxis {
    int n, sx1, nfull, sx2;
    bool first;
    float a_first, a_full, a_last;
    __device__ __forceinline__ void tap(int k, int &si, float &alpha) const {
        if (first) {
            if (k == 0) {
                si = sx1 - 1, alpha = a_first;
                return;
            }
            --k;
        }
        if (k < nfull) si = sx1 + k, alpha = a_full;
        else si = sx2, alpha = a_last;
    }
};
__device__ __forceinline__ AreaAxis area_axis(int d, int ssize, double scale) {
    const double fsx1 = d * scale, fsx2 = fsx1 + scale;
    const double cell = fmin(scale, (double)ssize - fsx1);
    int sx1 = (int)ceil(fsx1), sx2 = (int)floor(fsx2);
    sx2 = min(sx2, ssize - 1);
    sx1 = min(sx1, sx2);
    AreaAxis a;
    a.sx1 = sx1, a.sx2 = sx2, a.nfull = sx2 - sx1;
    a.first = sx1 - fsx1 > 1e-3;
    a.a_first = (float)((sx1 - fsx1) / cell), a.a_full = (float)(1.0 / cell);
    const bool last = fsx2 - sx2 > 1e-3;
    a.a_last = (float)(fmin(fmin(fsx2 - sx2, 1.0), cell) / cell);
    a.n = (a.first ? 1 : 0) + a.nfull + (last ? 1 : 0);
    return a;
}

__device__ __forceinline__ int gray_u8(const unsigned char *p, int swap_rb) {  // p: B, G, R (or R, G, B when swap_rb)
    const int b = swap_rb ? p[2] : p[0], g = p[1], r = swap_rb ? p[0] : p[2];
    return (b * 3735 + g * 19235 + r * 9798 + (1 << 14)) >> 15;
}

// one lane per destination pixel
__global__ void __launch_bounds__(256) gray_area_u8_kernel(const unsigned char *__restrict__ frames, float *__restrict__ out, int H,
                                                           int W, int OH, int OW, double sy, double sx, int normalize, int swap_rb,
                                                           size_t total) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int dx = (int)(i % OW), dy = (int)((i / OW) % OH);
    const size_t n = i / ((size_t)OW * OH);
    const AreaAxis tx = area_axis(dx, W, sx), ty = area_axis(dy, H, sy);
    const unsigned char *f = frames + n * (size_t)H * W * 3;
    float sum = 0.f;
    for (int j = 0; j < ty.n; ++j) {
        int sj, sk;
        float beta, alpha;
        ty.tap(j, sj, beta);
        const unsigned char *row = f + (size_t)sj * W * 3;
        float buf = 0.f;
        for (int k = 0; k < tx.n; ++k) {
            tx.tap(k, sk, alpha);
            buf = buf + mul_rounded((float)gray_u8(row + (size_t)sk * 3, swap_rb), alpha);
        }
        sum = j == 0 ? mul_rounded(beta, buf) : sum + mul_rounded(beta, buf);
    }
    const float g8 = fminf(fmaxf(rintf(sum), 0.f), 255.f);   // saturate_cast<uchar>: round half to even, clamp
    out[i] = normalize ? g8 / 255 * 2 - 1 : g8;              // main_new.py:643: x.float() / 255 * 2 - 1
}

// one lane per destination pixel (3 channels): 2 x 2 mean with rounding, optional R <-> B swap
__global__ void __launch_bounds__(256) area_half_u8_kernel(const unsigned char *__restrict__ in, unsigned char *__restrict__ out, int H,
                                                           int W, int swap_rb, size_t total) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int OW = W / 2, OH = H / 2;
    const int ox = (int)(i % OW), oy = (int)((i / OW) % OH);
    const size_t n = i / ((size_t)OW * OH);
    const unsigned char *p = in + ((n * H + 2 * oy) * (size_t)W + 2 * ox) * 3;
    const unsigned char *q = p + (size_t)W * 3;
    unsigned char r[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) r[c] = (unsigned char)((p[c] + p[3 + c] + q[c] + q[3 + c] + 2) >> 2);
    unsigned char *o = out + i * 3;
    o[0] = swap_rb ? r[2] : r[0], o[1] = r[1], o[2] = swap_rb ? r[0] : r[2];
}

// ---- cv2.resize(frame, (ow, oh), INTER_AREA) of a 3-channel 8-bit frame for ANY down-scaling ratio (reference main_new.py:723:
// every output frame goes to (640, 360) whatever the source size).  OpenCV 4.x, imgproc/resize.cpp:
//   * both ratios integer (1080p -> 3 x 3, 2160p -> 6 x 6): resizeAreaFast_<uchar, int, ...>: the int sum of the iscale_y x iscale_x
//     source pixels times float(1 / area), saturate_cast<uchar> (cvRound: half to even).  (2 x 2 has its own SIMD path,
//     (a + b + c + d + 2) >> 2: area_half_u8_kernel above.)
//   * otherwise computeResizeAreaTab + ResizeArea_Invoker per channel, exactly as gray_area_u8_kernel does for one plane.
// one lane per destination pixel (3 channels)
__global__ void __launch_bounds__(256) area_int_u8_kernel(const unsigned char *__restrict__ in, unsigned char *__restrict__ out, int H, int W,
                                                          int OH, int OW, int ky, int kx, float scale, int swap_rb, size_t total) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int ox = (int)(i % OW), oy = (int)((i / OW) % OH);
    const size_t n = i / ((size_t)OW * OH);
    const unsigned char *p = in + ((n * H + (size_t)oy * ky) * W + (size_t)ox * kx) * 3;
    int s0 = 0, s1 = 0, s2 = 0;
    for (int j = 0; j < ky; ++j) {
        const unsigned char *q = p + (size_t)j * W * 3;
        for (int k = 0; k < kx; ++k) s0 += q[3 * k], s1 += q[3 * k + 1], s2 += q[3 * k + 2];
    }
    const float r0 = fminf(fmaxf(rintf(mul_rounded((float)s0, scale)), 0.f), 255.f);
    const float r1 = fminf(fmaxf(rintf(mul_rounded((float)s1, scale)), 0.f), 255.f);
    const float r2 = fminf(fmaxf(rintf(mul_rounded((float)s2, scale)), 0.f), 255.f);
    unsigned char *o = out + i * 3;
    o[0] = (unsigned char)(swap_rb ? r2 : r0), o[1] = (unsigned char)r1, o[2] = (unsigned char)(swap_rb ? r0 : r2);
}

__global__ void __launch_bounds__(256) area_tab_u8_kernel(const unsigned char *__restrict__ in, unsigned char *__restrict__ out, int H, int W,
                                                          int OH, int OW, double sy, double sx, int swap_rb, size_t total) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int dx = (int)(i % OW), dy = (int)((i / OW) % OH);
    const size_t n = i / ((size_t)OW * OH);
    const AreaAxis tx = area_axis(dx, W, sx), ty = area_axis(dy, H, sy);
    const unsigned char *f = in + n * (size_t)H * W * 3;
    float sum[3] = {0.f, 0.f, 0.f};
    for (int j = 0; j < ty.n; ++j) {
        int sj, sk;
        float beta, alpha;
        ty.tap(j, sj, beta);
        const unsigned char *row = f + (size_t)sj * W * 3;
        float buf[3] = {0.f, 0.f, 0.f};
        for (int k = 0; k < tx.n; ++k) {
            tx.tap(k, sk, alpha);
#pragma unroll
            for (int c = 0; c < 3; ++c) buf[c] = buf[c] + mul_rounded((float)row[(size_t)sk * 3 + c], alpha);
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) sum[c] = j == 0 ? mul_rounded(beta, buf[c]) : sum[c] + mul_rounded(beta, buf[c]);
    }
    unsigned char r[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) r[c] = (unsigned char)fminf(fmaxf(rintf(sum[c]), 0.f), 255.f);
    unsigned char *o = out + i * 3;
    o[0] = swap_rb ? r[2] : r[0], o[1] = r[1], o[2] = swap_rb ? r[0] : r[2];
}


// ---- 4:2:0 YUV frames ([n][h*3/2][w] uint8: Y plane, then NV12's interleaved UV rows or I420's U and V planes), as decoders hand them over.
// Gray window planes: the gray of the BGR frame cv2.cvtColor(frame, COLOR_YUV2BGR_NV12 / _I420) would give, then the same INTER_AREA and
// x / 255 * 2 - 1 as gray_area_u8_kernel, fused in one launch, so a YUV clip gets the fields of its BGR decode bit for bit.  Unpinned against
// cv2 like the rest of this file: the conversion restates OpenCV 4.x's 8-bit BT.601 limited-range fixed point (imgproc color_yuv:
// ITUR_BT_601_CY / CVR / CVG / CUG / CUB, shift 20), chroma taken from sample (x/2, y/2) without interpolation:
//   y = max(0, Y - 16) * 1220542, u = U - 128, v = V - 128
//   R = sat((y + 1673527 v + 2^19) >> 20), G = sat((y - 852492 v - 409993 u + 2^19) >> 20), B = sat((y + 2116026 u + 2^19) >> 20)
__device__ __forceinline__ int sat_u8(int v) { return min(max(v, 0), 255); }
// 4:2:2 and 4:4:4 frames ([n][2 h][w], [n][3 h][w]: the chroma planes are (h >> CY) x (w >> CX) samples, (CX, CY) = (1, 0) and (0, 0)) take
// the same arithmetic with the chroma of sample (x >> CX, y >> CY); 4:2:0 is (1, 1).
template <int LAYOUT, int CX, int CY>   // LAYOUT 0: U V interleaved (NV12, NV16), 1: U plane, V plane (I420, I422, I444)
__device__ __forceinline__ int gray_yuv(const unsigned char *f, int H, int W, int x, int y) {
    const int Y = f[(size_t)y * W + x];
    const unsigned char *c = f + (size_t)H * W;
    int U, V;
    if (LAYOUT == 0) {
        const unsigned char *p = c + (size_t)(y >> CY) * (2 * (W >> CX)) + 2 * (x >> CX);
        U = p[0], V = p[1];
    } else {
        const size_t o = (size_t)(y >> CY) * (W >> CX) + (x >> CX);
        U = c[o], V = c[o + (size_t)(H >> CY) * (W >> CX)];
    }
    const int yy = max(0, Y - 16) * 1220542, u = U - 128, v = V - 128;
    const int r = sat_u8((yy + 1673527 * v + (1 << 19)) >> 20);
    const int g = sat_u8((yy - 852492 * v - 409993 * u + (1 << 19)) >> 20);
    const int b = sat_u8((yy + 2116026 * u + (1 << 19)) >> 20);
    return (b * 3735 + g * 19235 + r * 9798 + (1 << 14)) >> 15;   // gray_u8 above
}

// one lane per destination pixel, gray_area_u8_kernel's arithmetic in its order
template <int LAYOUT, int CX, int CY>
__global__ void __launch_bounds__(256) gray_area_yuv_kernel(const unsigned char *__restrict__ frames, float *__restrict__ out, int H, int W,
                                                            int OH, int OW, double sy, double sx, int normalize, size_t total) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int dx = (int)(i % OW), dy = (int)((i / OW) % OH);
    const size_t n = i / ((size_t)OW * OH);
    const AreaAxis tx = area_axis(dx, W, sx), ty = area_axis(dy, H, sy);
    const unsigned char *f = frames + n * ((size_t)H * W + 2 * (size_t)(H >> CY) * (W >> CX));   // (4:2:0: H W 3 / 2, H and W even)
    float sum = 0.f;
    for (int j = 0; j < ty.n; ++j) {
        int sj, sk;
        float beta, alpha;
        ty.tap(j, sj, beta);
        float buf = 0.f;
        for (int k = 0; k < tx.n; ++k) {
            tx.tap(k, sk, alpha);
            buf = buf + mul_rounded((float)gray_yuv<LAYOUT, CX, CY>(f, H, W, sk, sj), alpha);
        }
        sum = j == 0 ? mul_rounded(beta, buf) : sum + mul_rounded(beta, buf);
    }
    const float g8 = fminf(fmaxf(rintf(sum), 0.f), 255.f);
    out[i] = normalize ? g8 / 255 * 2 - 1 : g8;
}

// INTER_AREA of a C-channel byte plane (C = 1: Y, I420's U or V; C = 2: NV12's UV), the 3-channel kernels' algorithms above: 2 x 2 mean,
// integer-ratio sum * float(1 / area), area tables.  in / out: the plane of sample 0; samples ist / ost bytes apart.  One lane per pixel.
template <int C>
__global__ void __launch_bounds__(256) area_half_plane_kernel(const unsigned char *__restrict__ in, size_t ist, unsigned char *__restrict__ out,
                                                              size_t ost, int H, int W, size_t total) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int OW = W / 2, OH = H / 2;
    const int ox = (int)(i % OW), oy = (int)((i / OW) % OH);
    const size_t n = i / ((size_t)OW * OH);
    const unsigned char *p = in + n * ist + ((size_t)2 * oy * W + 2 * ox) * C;
    const unsigned char *q = p + (size_t)W * C;
    unsigned char *o = out + n * ost + ((size_t)oy * OW + ox) * C;
#pragma unroll
    for (int c = 0; c < C; ++c) o[c] = (unsigned char)((p[c] + p[C + c] + q[c] + q[C + c] + 2) >> 2);
}

template <int C>
__global__ void __launch_bounds__(256) area_int_plane_kernel(const unsigned char *__restrict__ in, size_t ist, unsigned char *__restrict__ out,
                                                             size_t ost, int H, int W, int OH, int OW, int ky, int kx, float scale, size_t total) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int ox = (int)(i % OW), oy = (int)((i / OW) % OH);
    const size_t n = i / ((size_t)OW * OH);
    const unsigned char *p = in + n * ist + ((size_t)oy * ky * W + (size_t)ox * kx) * C;
    int s[C] = {};
    for (int j = 0; j < ky; ++j) {
        const unsigned char *q = p + (size_t)j * W * C;
        for (int k = 0; k < kx; ++k)
#pragma unroll
            for (int c = 0; c < C; ++c) s[c] += q[C * k + c];
    }
    unsigned char *o = out + n * ost + ((size_t)oy * OW + ox) * C;
#pragma unroll
    for (int c = 0; c < C; ++c) o[c] = (unsigned char)fminf(fmaxf(rintf(mul_rounded((float)s[c], scale)), 0.f), 255.f);
}

template <int C>
__global__ void __launch_bounds__(256) area_tab_plane_kernel(const unsigned char *__restrict__ in, size_t ist, unsigned char *__restrict__ out,
                                                             size_t ost, int H, int W, int OH, int OW, double sy, double sx, size_t total) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int dx = (int)(i % OW), dy = (int)((i / OW) % OH);
    const size_t n = i / ((size_t)OW * OH);
    const AreaAxis tx = area_axis(dx, W, sx), ty = area_axis(dy, H, sy);
    const unsigned char *f = in + n * ist;
    float sum[C] = {};
    for (int j = 0; j < ty.n; ++j) {
        int sj, sk;
        float beta, alpha;
        ty.tap(j, sj, beta);
        const unsigned char *row = f + (size_t)sj * W * C;
        float buf[C] = {};
        for (int k = 0; k < tx.n; ++k) {
            tx.tap(k, sk, alpha);
#pragma unroll
            for (int c = 0; c < C; ++c) buf[c] = buf[c] + mul_rounded((float)row[(size_t)sk * C + c], alpha);
        }
#pragma unroll
        for (int c = 0; c < C; ++c) sum[c] = j == 0 ? mul_rounded(beta, buf[c]) : sum[c] + mul_rounded(beta, buf[c]);
    }
    unsigned char *o = out + n * ost + ((size_t)dy * OW + dx) * C;
#pragma unroll
    for (int c = 0; c < C; ++c) o[c] = (unsigned char)fminf(fmaxf(rintf(sum[c]), 0.f), 255.f);
}

// ---- 10-bit 4:2:0 frames ([n][h*3/2][w] little-endian 16-bit words, the 8-bit formats' plane order): LAYOUT 0 P010 (the sample in the HIGH 10 bits
// of its word, word = v10 << 6, as hardware decoders deliver it; the low 6 bits of an input word are ignored), 1 I010 / yuv420p10le (the sample in the
// LOW 10 bits; words above 1023 are clamped).  BT.601 limited range like the 8-bit path.
template <int LAYOUT>
__device__ __forceinline__ int sample10(unsigned short word) { return LAYOUT == 0 ? word >> 6 : min((int)word, 1023); }
template <int LAYOUT>
__device__ __forceinline__ unsigned short place10(int v10) { return (unsigned short)(LAYOUT == 0 ? v10 << 6 : v10); }
// the 8-bit reduction the generator sees (it was trained on 8-bit gray): round to nearest, saturate
template <int LAYOUT>
__device__ __forceinline__ int reduce8(unsigned short word) { return min(255, (sample10<LAYOUT>(word) + 2) >> 2); }

// gray_yuv above on the reduced samples, the reduction fused into the loads (no 8-bit copy of the frames)
template <int LAYOUT, int CX, int CY>   // LAYOUT 0: P010 / P210 (NV12's plane order), 1: I010 / I210 / I410 (I420's)
__device__ __forceinline__ int gray_yuv_u16(const unsigned short *f, int H, int W, int x, int y) {
    const int Y = reduce8<LAYOUT>(f[(size_t)y * W + x]);
    const unsigned short *c = f + (size_t)H * W;
    int U, V;
    if (LAYOUT == 0) {
        const unsigned short *p = c + (size_t)(y >> CY) * (2 * (W >> CX)) + 2 * (x >> CX);
        U = reduce8<LAYOUT>(p[0]), V = reduce8<LAYOUT>(p[1]);
    } else {
        const size_t o = (size_t)(y >> CY) * (W >> CX) + (x >> CX);
        U = reduce8<LAYOUT>(c[o]), V = reduce8<LAYOUT>(c[o + (size_t)(H >> CY) * (W >> CX)]);
    }
    const int yy = max(0, Y - 16) * 1220542, u = U - 128, v = V - 128;
    const int r = sat_u8((yy + 1673527 * v + (1 << 19)) >> 20);
    const int g = sat_u8((yy - 852492 * v - 409993 * u + (1 << 19)) >> 20);
    const int b = sat_u8((yy + 2116026 * u + (1 << 19)) >> 20);
    return (b * 3735 + g * 19235 + r * 9798 + (1 << 14)) >> 15;
}

// one lane per destination pixel, gray_area_yuv_kernel's arithmetic in its order: the planes of the 8-bit clip of the reduced samples bit for bit
template <int LAYOUT, int CX, int CY>
__global__ void __launch_bounds__(256) gray_area_yuv_u16_kernel(const unsigned short *__restrict__ frames, float *__restrict__ out, int H, int W,
                                                                int OH, int OW, double sy, double sx, int normalize, size_t total) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int dx = (int)(i % OW), dy = (int)((i / OW) % OH);
    const size_t n = i / ((size_t)OW * OH);
    const AreaAxis tx = area_axis(dx, W, sx), ty = area_axis(dy, H, sy);
    const unsigned short *f = frames + n * ((size_t)H * W + 2 * (size_t)(H >> CY) * (W >> CX));
    float sum = 0.f;
    for (int j = 0; j < ty.n; ++j) {
        int sj, sk;
        float beta, alpha;
        ty.tap(j, sj, beta);
        float buf = 0.f;
        for (int k = 0; k < tx.n; ++k) {
            tx.tap(k, sk, alpha);
            buf = buf + mul_rounded((float)gray_yuv_u16<LAYOUT, CX, CY>(f, H, W, sk, sj), alpha);
        }
        sum = j == 0 ? mul_rounded(beta, buf) : sum + mul_rounded(beta, buf);
    }
    const float g8 = fminf(fmaxf(rintf(sum), 0.f), 255.f);
    out[i] = normalize ? g8 / 255 * 2 - 1 : g8;
}

// INTER_AREA of a C-channel plane of 10-bit samples (C = 1: Y, I010's U or V; C = 2: P010's UV), cv::resize's dispatch for 16-bit unsigned on the
// 10-bit VALUES: 2 x 2 mean (ResizeAreaFastVec_SIMD_16u), integer ratios the block sum * float(1 / area) (resizeAreaFast_<ushort, float>: the float
// sum of a block of 10-bit values is exact), else the area tables; saturate to 0..1023, stored in the layout's placement.  in / out: the plane of
// sample 0; samples ist / ost WORDS apart.  One lane per pixel.
template <int C, int LAYOUT>
__global__ void __launch_bounds__(256) area_half_plane_u16_kernel(const unsigned short *__restrict__ in, size_t ist, unsigned short *__restrict__ out,
                                                                  size_t ost, int H, int W, size_t total) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int OW = W / 2, OH = H / 2;
    const int ox = (int)(i % OW), oy = (int)((i / OW) % OH);
    const size_t n = i / ((size_t)OW * OH);
    const unsigned short *p = in + n * ist + ((size_t)2 * oy * W + 2 * ox) * C;
    const unsigned short *q = p + (size_t)W * C;
    unsigned short *o = out + n * ost + ((size_t)oy * OW + ox) * C;
#pragma unroll
    for (int c = 0; c < C; ++c)
        o[c] = place10<LAYOUT>((sample10<LAYOUT>(p[c]) + sample10<LAYOUT>(p[C + c]) + sample10<LAYOUT>(q[c]) + sample10<LAYOUT>(q[C + c]) + 2) >> 2);
}

template <int C, int LAYOUT>
__global__ void __launch_bounds__(256) area_int_plane_u16_kernel(const unsigned short *__restrict__ in, size_t ist, unsigned short *__restrict__ out,
                                                                 size_t ost, int H, int W, int OH, int OW, int ky, int kx, float scale, size_t total) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int ox = (int)(i % OW), oy = (int)((i / OW) % OH);
    const size_t n = i / ((size_t)OW * OH);
    const unsigned short *p = in + n * ist + ((size_t)oy * ky * W + (size_t)ox * kx) * C;
    int s[C] = {};
    for (int j = 0; j < ky; ++j) {
        const unsigned short *q = p + (size_t)j * W * C;
        for (int k = 0; k < kx; ++k)
#pragma unroll
            for (int c = 0; c < C; ++c) s[c] += sample10<LAYOUT>(q[C * k + c]);
    }
    unsigned short *o = out + n * ost + ((size_t)oy * OW + ox) * C;
#pragma unroll
    for (int c = 0; c < C; ++c) o[c] = place10<LAYOUT>((int)fminf(fmaxf(rintf(mul_rounded((float)s[c], scale)), 0.f), 1023.f));
}

template <int C, int LAYOUT>
__global__ void __launch_bounds__(256) area_tab_plane_u16_kernel(const unsigned short *__restrict__ in, size_t ist, unsigned short *__restrict__ out,
                                                                 size_t ost, int H, int W, int OH, int OW, double sy, double sx, size_t total) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int dx = (int)(i % OW), dy = (int)((i / OW) % OH);
    const size_t n = i / ((size_t)OW * OH);
    const AreaAxis tx = area_axis(dx, W, sx), ty = area_axis(dy, H, sy);
    const unsigned short *f = in + n * ist;
    float sum[C] = {};
    for (int j = 0; j < ty.n; ++j) {
        int sj, sk;
        float beta, alpha;
        ty.tap(j, sj, beta);
        const unsigned short *row = f + (size_t)sj * W * C;
        float buf[C] = {};
        for (int k = 0; k < tx.n; ++k) {
            tx.tap(k, sk, alpha);
#pragma unroll
            for (int c = 0; c < C; ++c) buf[c] = buf[c] + mul_rounded((float)sample10<LAYOUT>(row[(size_t)sk * C + c]), alpha);
        }
#pragma unroll
        for (int c = 0; c < C; ++c) sum[c] = j == 0 ? mul_rounded(beta, buf[c]) : sum[c] + mul_rounded(beta, buf[c]);
    }
    unsigned short *o = out + n * ost + ((size_t)dy * OW + dx) * C;
#pragma unroll
    for (int c = 0; c < C; ++c) o[c] = place10<LAYOUT>((int)fminf(fmaxf(rintf(sum[c]), 0.f), 1023.f));
}

}  // namespace pws

using namespace pws;

extern "C" int pws_gray_area_u8(const unsigned char *frames_hwc, float *out, int n, int h, int w, int oh, int ow, int normalize,
                                int swap_rb, pws_stream_t stream) {
    PWS_REQUIRE(n >= 0 && h > 0 && w > 0 && oh > 0 && ow > 0 && oh <= h && ow <= w, "pws_gray_area_u8: bad shape (down-scaling only)");
    PWS_REQUIRE((double)h / oh <= AREA_MAX_TAPS - 2 && (double)w / ow <= AREA_MAX_TAPS - 2, "pws_gray_area_u8: scale above %d",
                AREA_MAX_TAPS - 2);
    if (n == 0) return PWS_OK;
    PWS_REQUIRE(frames_hwc && out, "pws_gray_area_u8: NULL pointer");
    const size_t total = (size_t)n * oh * ow;
    // cv::resize: inv_scale = (double)dsize / ssize, scale = 1. / inv_scale
    const double sy = 1.0 / ((double)oh / h), sx = 1.0 / ((double)ow / w);
    ProfScope prof(KID_OBJECTIVE, 10.0 * n * h * w, 3.0 * n * h * w + 4.0 * total, as_stream(stream));
    hipLaunchKernelGGL(gray_area_u8_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, as_stream(stream), frames_hwc, out, h, w,
                       oh, ow, sy, sx, normalize, swap_rb, total);
    return check_launch("gray_area_u8_kernel");
}

extern "C" int pws_area_half_u8(const unsigned char *in_hwc, unsigned char *out_hwc, int n, int h, int w, int swap_rb,
                                pws_stream_t stream) {
    PWS_REQUIRE(n >= 0 && h > 0 && w > 0 && h % 2 == 0 && w % 2 == 0, "pws_area_half_u8: h and w must be even");
    if (n == 0) return PWS_OK;
    PWS_REQUIRE(in_hwc && out_hwc, "pws_area_half_u8: NULL pointer");
    const size_t total = (size_t)n * (h / 2) * (w / 2);
    ProfScope prof(KID_OBJECTIVE, 12.0 * total, 15.0 * total, as_stream(stream));
    hipLaunchKernelGGL(area_half_u8_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, as_stream(stream), in_hwc, out_hwc, h, w,
                       swap_rb, total);
    return check_launch("area_half_u8_kernel");
}

extern "C" int pws_area_resize_u8(const unsigned char *in_hwc, unsigned char *out_hwc, int n, int h, int w, int oh, int ow, int swap_rb,
                                  pws_stream_t stream) {
    PWS_REQUIRE(n >= 0 && h > 0 && w > 0 && oh > 0 && ow > 0 && oh <= h && ow <= w, "pws_area_resize_u8: bad shape (down-scaling only)");
    if (n == 0) return PWS_OK;
    PWS_REQUIRE(in_hwc && out_hwc, "pws_area_resize_u8: NULL pointer");
    if (h == 2 * oh && w == 2 * ow) return pws_area_half_u8(in_hwc, out_hwc, n, h, w, swap_rb, stream);   // OpenCV's 2 x 2 SIMD path
    const size_t total = (size_t)n * oh * ow;
    const unsigned nb = (unsigned)((total + 255) / 256);
    ProfScope prof(KID_OBJECTIVE, 3.0 * n * h * w, 3.0 * n * h * w + 3.0 * total, as_stream(stream));
    if (h % oh == 0 && w % ow == 0) {
        // cv::resize: is_area_fast when both scale factors are integers; scale = 1.f / (iscale_x * iscale_y)
        const int ky = h / oh, kx = w / ow;
        hipLaunchKernelGGL(area_int_u8_kernel, dim3(nb), dim3(256), 0, as_stream(stream), in_hwc, out_hwc, h, w, oh, ow, ky, kx,
                           1.f / (float)(kx * ky), swap_rb, total);
        return check_launch("area_int_u8_kernel");
    }
    PWS_REQUIRE((double)h / oh <= AREA_MAX_TAPS - 2 && (double)w / ow <= AREA_MAX_TAPS - 2, "pws_area_resize_u8: scale above %d",
                AREA_MAX_TAPS - 2);
    const double sy = 1.0 / ((double)oh / h), sx = 1.0 / ((double)ow / w);
    hipLaunchKernelGGL(area_tab_u8_kernel, dim3(nb), dim3(256), 0, as_stream(stream), in_hwc, out_hwc, h, w, oh, ow, sy, sx, swap_rb, total);
    return check_launch("area_tab_u8_kernel");
}

// The window planes of packed YUV frames, both depths.  SB: bytes per sample; chroma: 0 4:2:0, 1 4:2:2, 2 4:4:4 (interleaved 4:4:4 is not
// offered).  One rule for every subsampling: h and w even.  One lane per destination pixel reads its own taps' samples; every index is inside
// the frame (taps are inside H x W, chroma indices are theirs shifted right).
template <int SB>
static int gray_area_yuv(const char *what, const void *frames, float *out, int n, int h, int w, int oh, int ow, int normalize, int layout, int chroma,
                         pws_stream_t stream) {
    PWS_REQUIRE(n >= 0 && h > 0 && w > 0 && oh > 0 && ow > 0 && oh <= h && ow <= w, "%s: bad shape (down-scaling only)", what);
    PWS_REQUIRE(h % 2 == 0 && w % 2 == 0, "%s: h and w must be even (got %d x %d)", what, w, h);
    PWS_REQUIRE(layout == 0 || layout == 1, "%s: layout must be 0 (%s) or 1 (%s), got %d", what, SB == 1 ? "NV12" : "P010", SB == 1 ? "I420" : "I010", layout);
    PWS_REQUIRE(chroma >= 0 && chroma <= 2, "%s: chroma must be 0 (4:2:0), 1 (4:2:2) or 2 (4:4:4), got %d", what, chroma);
    PWS_REQUIRE(!(chroma == 2 && layout == 0), "%s: interleaved 4:4:4 (%s) is not offered: layout 0 needs chroma 0 or 1", what, SB == 1 ? "NV24" : "P410");
    PWS_REQUIRE((double)h / oh <= AREA_MAX_TAPS - 2 && (double)w / ow <= AREA_MAX_TAPS - 2, "%s: scale above %d", what, AREA_MAX_TAPS - 2);
    if (n == 0) return PWS_OK;
    PWS_REQUIRE(frames && out, "%s: NULL pointer", what);
    if (SB == 2) PWS_REQUIRE((reinterpret_cast<size_t>(frames) & 1) == 0, "%s: frames must be 2-byte aligned", what);
    const size_t total = (size_t)n * oh * ow;
    const double sy = 1.0 / ((double)oh / h), sx = 1.0 / ((double)ow / w);
    // (frame I/O has no kernel id of its own: the 16-bit entries are booked under KID_OBJECTIVE like their 8-bit neighbours, on purpose)
    const double spp = chroma == 0 ? 1.5 : (chroma == 1 ? 2.0 : 3.0);   // samples read per source pixel
    ProfScope prof(KID_OBJECTIVE, (SB == 1 ? 16.0 : 19.0) * n * h * w, spp * SB * n * h * w + 4.0 * total, as_stream(stream));
    const dim3 grid((unsigned)((total + 255) / 256));
#define PWS_GRAY_YUV(L_, CX_, CY_)                                                                                                              \
    do {                                                                                                                                        \
        if constexpr (SB == 1)                                                                                                                  \
            hipLaunchKernelGGL((gray_area_yuv_kernel<L_, CX_, CY_>), grid, dim3(256), 0, as_stream(stream),                                     \
                               reinterpret_cast<const unsigned char *>(frames), out, h, w, oh, ow, sy, sx, normalize, total);                   \
        else                                                                                                                                    \
            hipLaunchKernelGGL((gray_area_yuv_u16_kernel<L_, CX_, CY_>), grid, dim3(256), 0, as_stream(stream),                                 \
                               reinterpret_cast<const unsigned short *>(frames), out, h, w, oh, ow, sy, sx, normalize, total);                  \
    } while (0)
    if (chroma == 0) {
        if (layout == 0) PWS_GRAY_YUV(0, 1, 1);
        else PWS_GRAY_YUV(1, 1, 1);
    } else if (chroma == 1) {
        if (layout == 0) PWS_GRAY_YUV(0, 1, 0);
        else PWS_GRAY_YUV(1, 1, 0);
    } else {
        PWS_GRAY_YUV(1, 0, 0);
    }
#undef PWS_GRAY_YUV
    return check_launch(SB == 1 ? "gray_area_yuv_kernel" : "gray_area_yuv_u16_kernel");
}

extern "C" int pws_gray_area_yuv420_u8(const unsigned char *frames, float *out, int n, int h, int w, int oh, int ow, int normalize, int layout,
                                       pws_stream_t stream) {
    return gray_area_yuv<1>("pws_gray_area_yuv420_u8", frames, out, n, h, w, oh, ow, normalize, layout, 0, stream);
}

extern "C" int pws_gray_area_yuv_u8(const unsigned char *frames, float *out, int n, int h, int w, int oh, int ow, int normalize, int layout,
                                    int chroma, pws_stream_t stream) {
    return gray_area_yuv<1>("pws_gray_area_yuv_u8", frames, out, n, h, w, oh, ow, normalize, layout, chroma, stream);
}

extern "C" int pws_area_resize_plane_u8(const unsigned char *in, size_t in_stride, unsigned char *out, size_t out_stride, int n, int h, int w,
                                        int c, int oh, int ow, pws_stream_t stream) {
    PWS_REQUIRE(n >= 0 && h > 0 && w > 0 && oh > 0 && ow > 0 && oh <= h && ow <= w, "pws_area_resize_plane_u8: bad shape (down-scaling only)");
    PWS_REQUIRE(c == 1 || c == 2, "pws_area_resize_plane_u8: 1 or 2 channels, got %d", c);
    if (n == 0) return PWS_OK;
    PWS_REQUIRE(in && out, "pws_area_resize_plane_u8: NULL pointer");
    const size_t total = (size_t)n * oh * ow;
    const dim3 grid((unsigned)((total + 255) / 256)), blk(256);
    hipStream_t st = as_stream(stream);
    ProfScope prof(KID_OBJECTIVE, (double)c * n * h * w, (double)c * ((double)n * h * w + (double)total), st);
    if (h == 2 * oh && w == 2 * ow) {   // OpenCV's 2 x 2 SIMD path
        if (c == 1) hipLaunchKernelGGL(area_half_plane_kernel<1>, grid, blk, 0, st, in, in_stride, out, out_stride, h, w, total);
        else hipLaunchKernelGGL(area_half_plane_kernel<2>, grid, blk, 0, st, in, in_stride, out, out_stride, h, w, total);
        return check_launch("area_half_plane_kernel");
    }
    if (h % oh == 0 && w % ow == 0) {
        const int ky = h / oh, kx = w / ow;
        const float scale = 1.f / (float)(kx * ky);
        if (c == 1) hipLaunchKernelGGL(area_int_plane_kernel<1>, grid, blk, 0, st, in, in_stride, out, out_stride, h, w, oh, ow, ky, kx, scale, total);
        else hipLaunchKernelGGL(area_int_plane_kernel<2>, grid, blk, 0, st, in, in_stride, out, out_stride, h, w, oh, ow, ky, kx, scale, total);
        return check_launch("area_int_plane_kernel");
    }
    PWS_REQUIRE((double)h / oh <= AREA_MAX_TAPS - 2 && (double)w / ow <= AREA_MAX_TAPS - 2, "pws_area_resize_plane_u8: scale above %d",
                AREA_MAX_TAPS - 2);
    const double sy = 1.0 / ((double)oh / h), sx = 1.0 / ((double)ow / w);
    if (c == 1) hipLaunchKernelGGL(area_tab_plane_kernel<1>, grid, blk, 0, st, in, in_stride, out, out_stride, h, w, oh, ow, sy, sx, total);
    else hipLaunchKernelGGL(area_tab_plane_kernel<2>, grid, blk, 0, st, in, in_stride, out, out_stride, h, w, oh, ow, sy, sx, total);
    return check_launch("area_tab_plane_kernel");
}

extern "C" int pws_gray_area_yuv420_u16(const unsigned short *frames, float *out, int n, int h, int w, int oh, int ow, int normalize, int layout,
                                        pws_stream_t stream) {
    return gray_area_yuv<2>("pws_gray_area_yuv420_u16", frames, out, n, h, w, oh, ow, normalize, layout, 0, stream);
}

extern "C" int pws_gray_area_yuv_u16(const unsigned short *frames, float *out, int n, int h, int w, int oh, int ow, int normalize, int layout,
                                     int chroma, pws_stream_t stream) {
    return gray_area_yuv<2>("pws_gray_area_yuv_u16", frames, out, n, h, w, oh, ow, normalize, layout, chroma, stream);
}

extern "C" int pws_area_resize_plane_u16(const unsigned short *in, size_t in_stride, unsigned short *out, size_t out_stride, int n, int h, int w,
                                         int c, int oh, int ow, int layout, pws_stream_t stream) {
    PWS_REQUIRE(n >= 0 && h > 0 && w > 0 && oh > 0 && ow > 0 && oh <= h && ow <= w, "pws_area_resize_plane_u16: bad shape (down-scaling only)");
    PWS_REQUIRE(c == 1 || c == 2, "pws_area_resize_plane_u16: 1 or 2 channels, got %d", c);
    PWS_REQUIRE(layout == 0 || layout == 1, "pws_area_resize_plane_u16: layout must be 0 (P010) or 1 (I010), got %d", layout);
    if (n == 0) return PWS_OK;
    PWS_REQUIRE(in && out, "pws_area_resize_plane_u16: NULL pointer");
    PWS_REQUIRE(((reinterpret_cast<size_t>(in) | reinterpret_cast<size_t>(out)) & 1) == 0, "pws_area_resize_plane_u16: in and out must be 2-byte aligned");
    const size_t total = (size_t)n * oh * ow;
    const dim3 grid((unsigned)((total + 255) / 256)), blk(256);
    hipStream_t st = as_stream(stream);
    ProfScope prof(KID_OBJECTIVE, (double)c * n * h * w, 2.0 * c * ((double)n * h * w + (double)total), st);
#define PWS_AREA16(KERNEL_, ...)                                                                                       \
    do {                                                                                                               \
        if (c == 1 && layout == 0) hipLaunchKernelGGL((KERNEL_<1, 0>), grid, blk, 0, st, in, in_stride, out, out_stride, __VA_ARGS__);      \
        else if (c == 1) hipLaunchKernelGGL((KERNEL_<1, 1>), grid, blk, 0, st, in, in_stride, out, out_stride, __VA_ARGS__);                \
        else if (layout == 0) hipLaunchKernelGGL((KERNEL_<2, 0>), grid, blk, 0, st, in, in_stride, out, out_stride, __VA_ARGS__);           \
        else hipLaunchKernelGGL((KERNEL_<2, 1>), grid, blk, 0, st, in, in_stride, out, out_stride, __VA_ARGS__);                            \
    } while (0)
    if (h == 2 * oh && w == 2 * ow) {   // OpenCV's 2 x 2 SIMD path
        PWS_AREA16(area_half_plane_u16_kernel, h, w, total);
        return check_launch("area_half_plane_u16_kernel");
    }
    if (h % oh == 0 && w % ow == 0) {
        const int ky = h / oh, kx = w / ow;
        const float scale = 1.f / (float)(kx * ky);
        PWS_REQUIRE((size_t)kx * ky <= 16384, "pws_area_resize_plane_u16: block of %d x %d too large", kx, ky);   // (the float sum stays exact)
        PWS_AREA16(area_int_plane_u16_kernel, h, w, oh, ow, ky, kx, scale, total);
        return check_launch("area_int_plane_u16_kernel");
    }
    PWS_REQUIRE((double)h / oh <= AREA_MAX_TAPS - 2 && (double)w / ow <= AREA_MAX_TAPS - 2, "pws_area_resize_plane_u16: scale above %d",
                AREA_MAX_TAPS - 2);
    const double sy = 1.0 / ((double)oh / h), sx = 1.0 / ((double)ow / w);
    PWS_AREA16(area_tab_plane_u16_kernel, h, w, oh, ow, sy, sx, total);
#undef PWS_AREA16
    return check_launch("area_tab_plane_u16_kernel");
}
