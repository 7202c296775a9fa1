// Deblurring (stream.frame_sharpness, stream.deblur_plan, functional.deblur_frames): shake blurs some frames and leaves their neighbours
// sharp; a blurred SOURCE frame borrows detail from the sharper frames around it, aligned by the clip's global motion, before the warp
// reads it.  OpenCV videostab's WeightingDeblurer with bilinear donors and every read from the original frames.  No counterpart in the
// reference.  include/pwstable.h has the definitions in full; tests/deblur_ref.py restates them.
//
//  * sharpness: S[t] = sum over the interior of (I[y,x+1] - I[y,x-1])^2 + (I[y+1,x] - I[y-1,x])^2 of an integer intensity I, in 64-bit
//    integers.  Integer sums do not depend on their order: workgroup partials go out through vector 64-bit atomic adds, the same bits on
//    every run.
//  * plan: per frame t and offset k = -R .. R the 2 x 3 map from frame t to frame t+k (chains of the per-pair similarities, walked outward
//    from t) and the gain 1 - S[t] / S[t+k] of a sharper donor.  One thread per frame and direction, fp64, every product and sum rounded once.
//  * blend: a gather.  Maps and gains are uniform per frame (blockIdx.z): the compiler keeps them in scalar registers, and a donor without
//    gain is skipped by the whole wave.  Under a near-translation adjacent lanes read adjacent donor samples.  A frame without donors is a copy.
#include <cstdint>

#include "common.h"

namespace pws {
namespace {

constexpr int DB_THREADS = 256, DB_RMAX = 15;

#pragma clang fp contract(off)   // every product and every sum rounded once, as the float64 restatement does

// ---- sharpness -------------------------------------------------------------------------------------------------------------------------
// KIND 0: interleaved 3-byte pixels, (w0 c0 + 150 c1 + w2 c2 + 128) >> 8; 1: bytes; 2: 16-bit words >> 6; 3: 16-bit words clamped to 1023
template <int KIND>
__device__ __forceinline__ int intensity(const void *frame, size_t i, int w0, int w2) {
    if constexpr (KIND == 0) {
        const uint8_t *p = static_cast<const uint8_t *>(frame) + 3 * i;
        return (w0 * (int)p[0] + 150 * (int)p[1] + w2 * (int)p[2] + 128) >> 8;
    } else if constexpr (KIND == 1) {
        return (int)static_cast<const uint8_t *>(frame)[i];
    } else if constexpr (KIND == 2) {
        return (int)(static_cast<const uint16_t *>(frame)[i] >> 6);
    } else {
        const int v = (int)static_cast<const uint16_t *>(frame)[i];
        return v < 1023 ? v : 1023;
    }
}

// grid (row blocks, frames): a workgroup takes interior rows 1 + blockIdx.x, + gridDim.x, ...; its threads the interior columns in turn
template <int KIND>
__global__ void __launch_bounds__(DB_THREADS) sharpness_kernel(const void *__restrict__ frames, size_t frame_bytes, int h, int w, int w0, int w2,
                                                               unsigned long long *__restrict__ sharp) {
    __shared__ unsigned long long part[DB_THREADS / kWave];
    const void *frame = static_cast<const uint8_t *>(frames) + (size_t)blockIdx.y * frame_bytes;
    unsigned long long acc = 0;
    for (int y = 1 + (int)blockIdx.x; y <= h - 2; y += (int)gridDim.x) {
        for (int x = 1 + (int)threadIdx.x; x <= w - 2; x += DB_THREADS) {
            const size_t c = (size_t)y * w + x;   // (every read is at x +- 1 or y +- 1 of an interior position: inside the plane)
            const int gx = intensity<KIND>(frame, c + 1, w0, w2) - intensity<KIND>(frame, c - 1, w0, w2);
            const int gy = intensity<KIND>(frame, c + w, w0, w2) - intensity<KIND>(frame, c - w, w0, w2);
            acc += (unsigned long long)(unsigned)(gx * gx + gy * gy);   // (at most 2 * 1023^2)
        }
    }
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) acc += __shfl_down(acc, off, kWave);
    if ((threadIdx.x & (kWave - 1)) == 0) part[threadIdx.x / kWave] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long sum = 0;
#pragma unroll
        for (int i = 0; i < DB_THREADS / kWave; ++i) sum += part[i];
        if (sum) atomicAdd(sharp + blockIdx.y, sum);   // integers: the order of the adds does not show
    }
}

template <int KIND>
int launch_sharpness(const char *what, const void *frames, size_t frame_bytes, size_t min_bytes, int align, int n, int h, int w, int w0, int w2,
                     long long *sharp, pws_stream_t stream) {
    PWS_REQUIRE(n >= 0 && h >= 3 && w >= 3, "%s: bad shape (n %d, h %d, w %d; a frame has an interior from 3 x 3 on)", what, n, h, w);
    if (n == 0) return PWS_OK;
    PWS_REQUIRE(frames && sharp, "%s: NULL pointer", what);
    PWS_REQUIRE((size_t)h * w < ((size_t)1 << 31) && n < 65536, "%s: frame or batch too large", what);
    PWS_REQUIRE(frame_bytes >= min_bytes, "%s: the frame stride is smaller than a plane of %d x %d", what, w, h);
    PWS_REQUIRE((reinterpret_cast<size_t>(sharp) & 7) == 0 && ((reinterpret_cast<size_t>(frames) | frame_bytes) & (size_t)(align - 1)) == 0,
                "%s: sharpness must be 8-byte aligned, frames and their stride %d-byte aligned", what, align);
    hipError_t e = hipMemsetAsync(sharp, 0, (size_t)n * sizeof(long long), as_stream(stream));
    if (e != hipSuccess) {
        set_error("%s: hipMemsetAsync: %s", what, hipGetErrorString(e));
        return PWS_EHIP;
    }
    const int rows = h - 2, gx = rows < 256 ? rows : 256;
    hipLaunchKernelGGL(sharpness_kernel<KIND>, dim3((unsigned)gx, (unsigned)n), dim3(DB_THREADS), 0, as_stream(stream), frames, frame_bytes, h, w,
                       w0, w2, reinterpret_cast<unsigned long long *>(sharp));
    return check_launch("sharpness_kernel");
}

// ---- plan ------------------------------------------------------------------------------------------------------------------------------
// a motion row that a chain may pass: finite, and a scale in [0.5, 2] (a fit that failed, or one that no consecutive pair of a video has)
__device__ __forceinline__ bool plan_row_ok(const double *m) {
    if (!(isfinite(m[0]) && isfinite(m[1]) && isfinite(m[2]) && isfinite(m[3]))) return false;
    const double s = hypot(m[0], m[1]);
    return s >= 0.5 && s <= 2.0;
}

// thread (t, direction): the chain from frame t into the past (dir -1) or the future (+1), outward, one step per column
__global__ void __launch_bounds__(DB_THREADS) deblur_plan_kernel(const double *__restrict__ motion, const long long *__restrict__ sharp, int n, int R,
                                                                 double *__restrict__ maps, float *__restrict__ gain) {
    const int id = (int)(blockIdx.x * DB_THREADS + threadIdx.x);
    if (id >= 2 * n) return;
    const int t = id >> 1, dir = (id & 1) ? 1 : -1, K = 2 * R + 1;
    double *mp = maps + (size_t)t * K * 6;
    float *gp = gain + (size_t)t * K;
    if (dir < 0) {   // the centre column: the identity, and no gain
        double *o = mp + (size_t)R * 6;
        o[0] = 1.0, o[1] = 0.0, o[2] = 0.0, o[3] = 0.0, o[4] = 1.0, o[5] = 0.0;
        gp[R] = 0.f;
    }
    const long long st = sharp[t];
    double c[6] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0};
    bool alive = true;
    for (int j = 1; j <= R; ++j) {
        const int u = t + dir * j, col = R + dir * j;
        const double *m = nullptr;
        alive = alive && u >= 0 && u < n;
        if (alive) {
            m = motion + (size_t)(dir < 0 ? u + 1 : u) * 4;   // the pair between frame u and the frame before it on the chain: rows 1 .. n-1
            alive = plan_row_ok(m);
        }
        double *o = mp + (size_t)col * 6;
        if (!alive) {
            const double nan = __builtin_nan("");
#pragma unroll
            for (int q = 0; q < 6; ++q) o[q] = nan;
            gp[col] = 0.f;
            continue;
        }
        const double a = m[0], b = m[1], tx = m[2], ty = m[3];
        double s[6];
        if (dir < 0) {   // motion[u + 1] maps frame u+1 to frame u
            s[0] = a, s[1] = 0.0 - b, s[2] = tx, s[3] = b, s[4] = a, s[5] = ty;
        } else {         // the inverse of motion[u], which maps frame u to frame u-1
            const double d = a * a + b * b, ia = a / d, ib = b / d;
            s[0] = ia, s[1] = ib, s[2] = 0.0 - (ia * tx + ib * ty), s[3] = 0.0 - ib, s[4] = ia, s[5] = ib * tx - ia * ty;
        }
        const double n0 = s[0] * c[0] + s[1] * c[3], n1 = s[0] * c[1] + s[1] * c[4], n2 = (s[0] * c[2] + s[1] * c[5]) + s[2];
        const double n3 = s[3] * c[0] + s[4] * c[3], n4 = s[3] * c[1] + s[4] * c[4], n5 = (s[3] * c[2] + s[4] * c[5]) + s[5];
        c[0] = n0, c[1] = n1, c[2] = n2, c[3] = n3, c[4] = n4, c[5] = n5;
#pragma unroll
        for (int q = 0; q < 6; ++q) o[q] = c[q];
        const long long sd = sharp[u];
        gp[col] = sd > st ? (float)(1.0 - (double)st / (double)sd) : 0.f;
    }
}

__global__ void __launch_bounds__(DB_THREADS) deblur_donors_kernel(const float *__restrict__ gain, int n, int K, int *__restrict__ donors) {
    const int t = (int)(blockIdx.x * DB_THREADS + threadIdx.x);
    if (t >= n) return;
    int cnt = 0;
    for (int k = 0; k < K; ++k) cnt += gain[(size_t)t * K + k] > 0.f ? 1 : 0;
    donors[t] = cnt;
}

// ---- blend -----------------------------------------------------------------------------------------------------------------------------
struct Blend {          // what the three kernels share of a call
    int n, start, R;    // frames given; the first frame to write; the radius
    int h, w;           // the blended plane
    float s;            // the sensitivity, in sample units
};

// does frame t have a donor at all?  (wave-uniform: t is the workgroup's)
__device__ __forceinline__ bool has_donor(const float *__restrict__ gp, int t, int n, int R) {
    bool any = false;
    for (int k = -R; k <= R; ++k) any = any || (k != 0 && t + k >= 0 && t + k < n && gp[R + k] > 0.f);
    return any;
}

// the donor position of the centred position (dx, dy): fp64, each coordinate rounded once to fp32; false outside the plane (NaN included)
__device__ __forceinline__ bool donor_position(const double *__restrict__ m, double dx, double dy, double cx, double cy, int h, int w, int &x0,
                                               int &y0, float &lx, float &ly) {
    const float qx = (float)((m[0] * dx + (m[1] * dy + m[2])) + cx), qy = (float)((m[3] * dx + (m[4] * dy + m[5])) + cy);
    if (!(qx >= 0.f && qx <= (float)(w - 1) && qy >= 0.f && qy <= (float)(h - 1))) return false;
    x0 = min(max((int)floorf(qx), 0), w - 2), y0 = min(max((int)floorf(qy), 0), h - 2);   // (taps x0, x0 + 1 and y0, y0 + 1: inside the plane)
    lx = qx - (float)x0, ly = qy - (float)y0;
    return true;
}

__device__ __forceinline__ float lerp2(float a, float b, float c, float d, float lx, float ly) {
    const float top = (1.f - lx) * a + lx * b, bot = (1.f - lx) * c + lx * d;
    return (1.f - ly) * top + ly * bot;
}

// nearest integer (ties to even), clamped to [0, hi]
__device__ __forceinline__ unsigned round_clamp(float v, float hi) { return (unsigned)fminf(fmaxf(rintf(v), 0.f), hi); }

// interleaved 3-byte pixels, one pixel per thread; grid (pixel blocks, 1, frames to write)
__global__ void __launch_bounds__(DB_THREADS) deblur_bgr_kernel(const uint8_t *__restrict__ frames, const double *__restrict__ maps,
                                                                const float *__restrict__ gain, uint8_t *__restrict__ out, Blend B) {
    const int i = (int)blockIdx.z, t = B.start + i, K = 2 * B.R + 1;
    const size_t hw = (size_t)B.h * B.w, pix = (size_t)blockIdx.x * DB_THREADS + threadIdx.x;
    if (pix >= hw) return;
    const float *gp = gain + (size_t)i * K;
    const double *mp = maps + (size_t)i * K * 6;
    const uint8_t *own = frames + ((size_t)t * hw + pix) * 3;
    uint8_t *o = out + ((size_t)i * hw + pix) * 3;
    if (!has_donor(gp, t, B.n, B.R)) {
        o[0] = own[0], o[1] = own[1], o[2] = own[2];
        return;
    }
    const int y = (int)(pix / (size_t)B.w), x = (int)(pix - (size_t)y * B.w);
    const double cx = 0.5 * (double)(B.w - 1), cy = 0.5 * (double)(B.h - 1), dx = (double)x - cx, dy = (double)y - cy;
    const float b0 = (float)own[0], g0 = (float)own[1], r0 = (float)own[2];
    const float i0 = (29.f * b0 + 150.f * g0 + 77.f * r0) * (1.f / 256.f);
    float ab = b0, ag = g0, ar = r0, ws = 1.f;
    for (int c = 0; c < 2 * B.R; ++c) {
        const int k = c < B.R ? c - B.R : c - B.R + 1, u = t + k;
        const float g = gp[B.R + k];
        if (!(g > 0.f) || u < 0 || u >= B.n) continue;   // the whole wave
        int x0, y0;
        float lx, ly;
        if (!donor_position(mp + (size_t)(B.R + k) * 6, dx, dy, cx, cy, B.h, B.w, x0, y0, lx, ly)) continue;
        const uint8_t *d0 = frames + ((size_t)u * hw + (size_t)y0 * B.w + x0) * 3, *d1 = d0 + (size_t)B.w * 3;
        const float vb = lerp2((float)d0[0], (float)d0[3], (float)d1[0], (float)d1[3], lx, ly);
        const float vg = lerp2((float)d0[1], (float)d0[4], (float)d1[1], (float)d1[4], lx, ly);
        const float vr = lerp2((float)d0[2], (float)d0[5], (float)d1[2], (float)d1[5], lx, ly);
        const float iq = (29.f * vb + 150.f * vg + 77.f * vr) * (1.f / 256.f);
        const float wgt = g * B.s / (B.s + fabsf(iq - i0));
        ab += wgt * vb, ag += wgt * vg, ar += wgt * vr, ws += wgt;
    }
    o[0] = (uint8_t)round_clamp(ab / ws, 255.f), o[1] = (uint8_t)round_clamp(ag / ws, 255.f), o[2] = (uint8_t)round_clamp(ar / ws, 255.f);
}

// LAYOUT 0: the sample is word >> 6 and is written back << 6 (P010, P210); 1: the word clamped to 1023 (I010, I210, I410).  Bytes: as they are.
template <typename T, int LAYOUT>
__device__ __forceinline__ float plane_sample(T v) {
    if constexpr (sizeof(T) == 1) return (float)v;
    else if constexpr (LAYOUT == 0) return (float)(v >> 6);
    else return (float)(v < 1023 ? v : 1023);
}

// a frame of `rows` rows of w samples whose first h rows are the plane to blend (the Y plane of a packed frame; the rows behind it are its
// chroma, copied); 4 consecutive samples per thread (w % 4 == 0); grid (quad blocks, 1, frames to write)
template <typename T, int LAYOUT>
__global__ void __launch_bounds__(DB_THREADS) deblur_plane_kernel(const T *__restrict__ frames, const double *__restrict__ maps,
                                                                  const float *__restrict__ gain, T *__restrict__ out, Blend B, int rows) {
    struct __attribute__((aligned(4 * sizeof(T)))) Quad {
        T v[4];
    };
    const int i = (int)blockIdx.z, t = B.start + i, K = 2 * B.R + 1, wq = B.w >> 2;
    const size_t quad = (size_t)blockIdx.x * DB_THREADS + threadIdx.x, fsize = (size_t)rows * B.w;
    if (quad >= (size_t)rows * wq) return;
    const int y = (int)(quad / (size_t)wq), x = (int)(quad - (size_t)y * wq) * 4;
    const float *gp = gain + (size_t)i * K;
    const double *mp = maps + (size_t)i * K * 6;
    const Quad own = *reinterpret_cast<const Quad *>(frames + (size_t)t * fsize + (size_t)y * B.w + x);
    Quad *o = reinterpret_cast<Quad *>(out + (size_t)i * fsize + (size_t)y * B.w + x);
    if (y >= B.h || !has_donor(gp, t, B.n, B.R)) {   // chroma rows, and a frame without donors: the source's words
        *o = own;
        return;
    }
    constexpr float HI = sizeof(T) == 1 ? 255.f : 1023.f;
    const double cx = 0.5 * (double)(B.w - 1), cy = 0.5 * (double)(B.h - 1), dy = (double)y - cy;
    float v0[4], acc[4], ws[4];
#pragma unroll
    for (int p = 0; p < 4; ++p) v0[p] = plane_sample<T, LAYOUT>(own.v[p]), acc[p] = v0[p], ws[p] = 1.f;
    for (int c = 0; c < 2 * B.R; ++c) {
        const int k = c < B.R ? c - B.R : c - B.R + 1, u = t + k;
        const float g = gp[B.R + k];
        if (!(g > 0.f) || u < 0 || u >= B.n) continue;   // the whole wave
        const double *m = mp + (size_t)(B.R + k) * 6;
        const T *donor = frames + (size_t)u * fsize;
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            int x0, y0;
            float lx, ly;
            if (!donor_position(m, (double)(x + p) - cx, dy, cx, cy, B.h, B.w, x0, y0, lx, ly)) continue;
            const T *d0 = donor + (size_t)y0 * B.w + x0, *d1 = d0 + B.w;
            const float v = lerp2(plane_sample<T, LAYOUT>(d0[0]), plane_sample<T, LAYOUT>(d0[1]), plane_sample<T, LAYOUT>(d1[0]),
                                  plane_sample<T, LAYOUT>(d1[1]), lx, ly);
            const float wgt = g * B.s / (B.s + fabsf(v - v0[p]));
            acc[p] += wgt * v, ws[p] += wgt;
        }
    }
    Quad r;
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const unsigned q = round_clamp(acc[p] / ws[p], HI);
        r.v[p] = (T)(sizeof(T) == 2 && LAYOUT == 0 ? q << 6 : q);
    }
    *o = r;
}

int check_blend(const char *what, const void *frames, const double *maps, const float *gain, const void *out, int n, int start, int stop,
                int radius, int rows, int h, int w, double sensitivity, int align) {
    PWS_REQUIRE(n >= 0 && h >= 2 && w >= 2 && rows >= h, "%s: bad shape (n %d, rows %d, h %d, w %d; the bilinear taps need 2 x 2)", what, n, rows, h, w);
    PWS_REQUIRE(0 <= start && start <= stop && stop <= n, "%s: the range must satisfy 0 <= start <= stop <= %d, got [%d, %d)", what, n, start, stop);
    PWS_REQUIRE(radius >= 1 && radius <= DB_RMAX, "%s: radius must be 1 .. %d, got %d", what, DB_RMAX, radius);
    PWS_REQUIRE(sensitivity > 0.0 && sensitivity <= 3.0e38, "%s: sensitivity must be finite and positive, got %g", what, sensitivity);
    if (start == stop) return PWS_OK;
    PWS_REQUIRE(frames && maps && gain && out, "%s: NULL pointer", what);
    PWS_REQUIRE((size_t)rows * w < ((size_t)1 << 31) && n < 65536, "%s: frame or batch too large", what);
    PWS_REQUIRE((reinterpret_cast<size_t>(maps) & 7) == 0 && (reinterpret_cast<size_t>(gain) & 3) == 0, "%s: maps must be 8-byte and gain 4-byte aligned", what);
    PWS_REQUIRE(((reinterpret_cast<size_t>(frames) | reinterpret_cast<size_t>(out)) & (size_t)(align - 1)) == 0, "%s: frames and out must be %d-byte aligned",
                what, align);
    return PWS_OK;
}

template <typename T, int LAYOUT>
int launch_plane(const T *frames, const double *maps, const float *gain, T *out, const Blend &B, int stop, int rows, pws_stream_t stream) {
    const size_t quads = (size_t)rows * (B.w >> 2);
    hipLaunchKernelGGL((deblur_plane_kernel<T, LAYOUT>), dim3((unsigned)((quads + DB_THREADS - 1) / DB_THREADS), 1u, (unsigned)(stop - B.start)),
                       dim3(DB_THREADS), 0, as_stream(stream), frames, maps, gain, out, B, rows);
    return check_launch("deblur_plane_kernel");
}

}  // namespace
}  // namespace pws

using namespace pws;

extern "C" int pws_frame_sharpness_u8(const unsigned char *frames, int n, int h, int w, int rgb, long long *sharpness, pws_stream_t stream) {
    const size_t fb = (size_t)(h > 0 ? h : 0) * (size_t)(w > 0 ? w : 0) * 3;
    return launch_sharpness<0>("pws_frame_sharpness_u8", frames, fb, fb, 1, n, h, w, rgb ? 77 : 29, rgb ? 29 : 77, sharpness, stream);
}

extern "C" int pws_plane_sharpness_u8(const unsigned char *planes, size_t frame_stride, int n, int h, int w, long long *sharpness,
                                      pws_stream_t stream) {
    return launch_sharpness<1>("pws_plane_sharpness_u8", planes, frame_stride, (size_t)(h > 0 ? h : 0) * (size_t)(w > 0 ? w : 0), 1, n, h, w, 0, 0, sharpness,
                               stream);
}

extern "C" int pws_plane_sharpness_u16(const unsigned short *planes, size_t frame_stride, int n, int h, int w, int layout, long long *sharpness,
                                       pws_stream_t stream) {
    PWS_REQUIRE(layout == 0 || layout == 1, "pws_plane_sharpness_u16: layout must be 0 (word >> 6) or 1 (word clamped to 1023), got %d", layout);
    PWS_REQUIRE(frame_stride < ((size_t)1 << 40), "pws_plane_sharpness_u16: frame or batch too large");
    const size_t min_bytes = (size_t)(h > 0 ? h : 0) * (size_t)(w > 0 ? w : 0) * 2;
    if (layout == 0) return launch_sharpness<2>("pws_plane_sharpness_u16", planes, frame_stride * 2, min_bytes, 2, n, h, w, 0, 0, sharpness, stream);
    return launch_sharpness<3>("pws_plane_sharpness_u16", planes, frame_stride * 2, min_bytes, 2, n, h, w, 0, 0, sharpness, stream);
}

extern "C" int pws_deblur_plan(const double *motion, const long long *sharpness, int n, int radius, double *maps, float *gain, int *donors,
                               pws_stream_t stream) {
    PWS_REQUIRE(n >= 0, "pws_deblur_plan: bad shape (n %d)", n);
    PWS_REQUIRE(radius >= 1 && radius <= DB_RMAX, "pws_deblur_plan: radius must be 1 .. %d, got %d", DB_RMAX, radius);
    if (n == 0) return PWS_OK;
    PWS_REQUIRE(motion && sharpness && maps && gain && donors, "pws_deblur_plan: NULL pointer");
    PWS_REQUIRE(((reinterpret_cast<size_t>(motion) | reinterpret_cast<size_t>(sharpness) | reinterpret_cast<size_t>(maps)) & 7) == 0 &&
                    ((reinterpret_cast<size_t>(gain) | reinterpret_cast<size_t>(donors)) & 3) == 0,
                "pws_deblur_plan: motion, sharpness and maps must be 8-byte aligned, gain and donors 4-byte aligned");
    PWS_REQUIRE(n <= (1 << 24), "pws_deblur_plan: a scene of %d frames, at most 2^24", n);
    hipLaunchKernelGGL(deblur_plan_kernel, dim3((unsigned)((2 * n + DB_THREADS - 1) / DB_THREADS)), dim3(DB_THREADS), 0, as_stream(stream), motion,
                       sharpness, n, radius, maps, gain);
    int rc = check_launch("deblur_plan_kernel");
    if (rc != PWS_OK) return rc;
    hipLaunchKernelGGL(deblur_donors_kernel, dim3((unsigned)((n + DB_THREADS - 1) / DB_THREADS)), dim3(DB_THREADS), 0, as_stream(stream), gain, n,
                       2 * radius + 1, donors);
    return check_launch("deblur_donors_kernel");
}

extern "C" int pws_deblur_u8(const unsigned char *frames, const double *maps, const float *gain, unsigned char *out, int n, int start, int stop,
                             int radius, int h, int w, double sensitivity, pws_stream_t stream) {
    int rc = check_blend("pws_deblur_u8", frames, maps, gain, out, n, start, stop, radius, h, h, w, sensitivity, 1);
    if (rc != PWS_OK || start == stop) return rc;
    PWS_REQUIRE((size_t)h * w * 3 < ((size_t)1 << 31), "pws_deblur_u8: frame or batch too large");
    const Blend B = {n, start, radius, h, w, (float)sensitivity};
    const size_t hw = (size_t)h * w;
    hipLaunchKernelGGL(deblur_bgr_kernel, dim3((unsigned)((hw + DB_THREADS - 1) / DB_THREADS), 1u, (unsigned)(stop - start)), dim3(DB_THREADS), 0,
                       as_stream(stream), frames, maps, gain, out, B);
    return check_launch("deblur_bgr_kernel");
}

extern "C" int pws_deblur_plane_u8(const unsigned char *frames, const double *maps, const float *gain, unsigned char *out, int n, int start,
                                   int stop, int radius, int rows, int h, int w, double sensitivity, pws_stream_t stream) {
    int rc = check_blend("pws_deblur_plane_u8", frames, maps, gain, out, n, start, stop, radius, rows, h, w, sensitivity, 4);
    if (rc != PWS_OK) return rc;
    PWS_REQUIRE(w % 4 == 0, "pws_deblur_plane_u8: w must be a multiple of 4, got %d", w);
    if (start == stop) return PWS_OK;
    const Blend B = {n, start, radius, h, w, (float)sensitivity};
    return launch_plane<unsigned char, 0>(frames, maps, gain, out, B, stop, rows, stream);
}

extern "C" int pws_deblur_plane_u16(const unsigned short *frames, const double *maps, const float *gain, unsigned short *out, int n, int start,
                                    int stop, int radius, int rows, int h, int w, int layout, double sensitivity, pws_stream_t stream) {
    int rc = check_blend("pws_deblur_plane_u16", frames, maps, gain, out, n, start, stop, radius, rows, h, w, sensitivity, 8);
    if (rc != PWS_OK) return rc;
    PWS_REQUIRE(w % 4 == 0, "pws_deblur_plane_u16: w must be a multiple of 4, got %d", w);
    PWS_REQUIRE(layout == 0 || layout == 1, "pws_deblur_plane_u16: layout must be 0 (word >> 6) or 1 (word clamped to 1023), got %d", layout);
    if (start == stop) return PWS_OK;
    const Blend B = {n, start, radius, h, w, 4.f * (float)sensitivity};   // the sensitivity is in 8-bit gray levels
    if (layout == 0) return launch_plane<unsigned short, 0>(frames, maps, gain, out, B, stop, rows, stream);
    return launch_plane<unsigned short, 1>(frames, maps, gain, out, B, stop, rows, stream);
}
