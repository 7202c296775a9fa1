// Automatic crop of the reference's process() (main_new.py:484-606; constants :451-455), per frame: the warp field resized to the
// source frame is sampled on a 20 x 20 lattice, a homography is fitted from those samples to their pixel positions, and the frame's
// four corners mapped through it give the frame's crop bounds (the recurrence over the clip runs on the host, stream.py).
//
// The reference fits with cv2.findHomography(p1, p2, RANSAC, 3.0).  With a 3.0 threshold on coordinates of magnitude ~1 every sample
// of an in-frame field is an inlier, so this fits all 400: a Hartley-normalised DLT (m33 = 1) refined by Gauss-Newton on the forward
// reprojection error sum |p2 - pi(M [p1, 1])|^2, in fp64.  One 64-lane wave per frame:
//   * lane l owns lattice points l, l + 64, ... (7 at most): p1 with upsample_bilinear_ac_kernel's arithmetic (grid_sample.hip), so the
//     samples are the live resize's values bit for bit; p2 rounded to fp32 as the reference's np.float32 array;
//   * the 36 + 8 sums of each 8 x 8 normal system: per-lane partials in registers, reduced through LDS in a fixed order (deterministic);
//   * every lane solves the system redundantly by Cholesky, fully unrolled (registers only, no scratch), so the iteration's control flow
//     is wave-uniform.
// A frame whose samples have no spread, whose normal matrix is not positive definite or whose result is not finite gets NaN M and bounds.
#include <cfloat>

#include "common.h"

namespace pws {

namespace {

constexpr int HG_SIDE = 20, HG_PTS = HG_SIDE * HG_SIDE;     // num_sample (main_new.py:452)
constexpr int HG_STRIDE_Y = 15, HG_STRIDE_X = 30;           // stride_sample, and twice it across (main_new.py:453,556-560)
constexpr int HG_PER_LANE = (HG_PTS + kWave - 1) / kWave;   // 7
constexpr int HG_SUMS = 44;                                 // 36 upper-triangle entries of the 8 x 8 normal matrix + 8 right-hand sides
constexpr int HG_MAX_ITERS = 20;

// index of N[r][c], r <= c, in the packed upper triangle
__host__ __device__ constexpr int sym8(int r, int c) { return r * 8 - r * (r - 1) / 2 + (c - r); }

// The resize's blend hy * (hx * a + lx * b) + ly * (hx * c + lx * d) (a, b: row y0; c, d: row y1) with the roundings hipcc gives it in
// upsample_bilinear_ac_kernel (read off its ISA: the rows as one fma on a rounded product each, the outer blend as two rounded products
// and an add), spelled out so that the samples are that kernel's values bit for bit.
__device__ __forceinline__ float blend(float hy, float ly, float hx, float lx, float a, float b, float c, float d) {
    const float r0 = __builtin_fmaf(b, lx, mul_rounded(a, hx)), r1 = __builtin_fmaf(c, hx, mul_rounded(d, lx));
    return mul_rounded(hy, r0) + mul_rounded(ly, r1);
}

__device__ __forceinline__ void accum_row(double (&acc)[HG_SUMS], const double (&a)[8], double b) {
#pragma unroll
    for (int r = 0; r < 8; ++r) {
#pragma unroll
        for (int c = r; c < 8; ++c) acc[sym8(r, c)] = fma(a[r], a[c], acc[sym8(r, c)]);
        acc[36 + r] = fma(a[r], b, acc[36 + r]);
    }
}

// v[k] <- sum over the wave's 64 lanes of v[k], in lane order; every lane receives the totals.
template <int NS>
__device__ __forceinline__ void wave_sum(double (&v)[NS], double (*red)[kWave + 1], double *tot, int lane) {
#pragma unroll
    for (int k = 0; k < NS; ++k) red[k][lane] = v[k];
    __syncthreads();
    if (lane < NS) {
        double s = 0.0;
        for (int j = 0; j < kWave; ++j) s += red[lane][j];
        tot[lane] = s;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < NS; ++k) v[k] = tot[k];
    __syncthreads();   // red / tot are reused by the next reduction
}

// Solves N d = g by Cholesky (N: packed upper triangle tot[0..35], g: tot[36..43]).  False when a pivot is not positive relative to
// its diagonal entry (not positive definite, numerically) or is NaN.
__device__ __forceinline__ bool chol_solve8(const double (&tot)[HG_SUMS], double (&d)[8]) {
    double L[8][8];
    bool ok = true;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
#pragma unroll
        for (int j = 0; j <= i; ++j) {
            double s = tot[sym8(j, i)];
#pragma unroll
            for (int k = 0; k < j; ++k) s -= L[i][k] * L[j][k];
            if (i == j) {
                ok = ok && (s > 1e-12 * tot[sym8(i, i)]);
                L[i][i] = sqrt(fmax(s, 0.0));
            } else {
                L[i][j] = s / L[j][j];
            }
        }
    }
    double y[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        double s = tot[36 + i];
#pragma unroll
        for (int k = 0; k < i; ++k) s -= L[i][k] * y[k];
        y[i] = s / L[i][i];
    }
#pragma unroll
    for (int i = 7; i >= 0; --i) {
        double s = y[i];
#pragma unroll
        for (int k = i + 1; k < 8; ++k) s -= L[k][i] * d[k];
        d[i] = s / L[i][i];
    }
    return ok;
}

__global__ void __launch_bounds__(kWave) field_homography_kernel(const float *__restrict__ field, int fh, int fw, int h0, int w0, float ry,
                                                                 float rx, double *__restrict__ m_out, float *__restrict__ bounds_out,
                                                                 float *__restrict__ pts_out) {
    __shared__ double red[HG_SUMS][kWave + 1];
    __shared__ double tot_s[HG_SUMS];
    const int f = blockIdx.x, lane = threadIdx.x;
    const float *F = field + (size_t)f * fh * fw * 2;

    // ---- samples: p1 = F_resized[r, c] (fp32), p2 = the lattice pixel in [-1, 1] (rounded to fp32)
    double p1x[HG_PER_LANE], p1y[HG_PER_LANE], p2x[HG_PER_LANE], p2y[HG_PER_LANE];
    double s4[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int j = 0; j < HG_PER_LANE; ++j) {
        const int k = lane + kWave * j;
        const bool valid = k < HG_PTS;
        const int kk = valid ? k : 0;
        const int a = kk / HG_SIDE, b = kk % HG_SIDE;
        const int r = h0 / 2 + (a - HG_SIDE / 2) * HG_STRIDE_Y, c = w0 / 2 + (b - HG_SIDE / 2) * HG_STRIDE_X;
        const float sy = mul_rounded(ry, (float)r), sx = mul_rounded(rx, (float)c);
        const int y0 = (int)sy, x0 = (int)sx;
        const int y1 = y0 + (y0 < fh - 1 ? 1 : 0), x1 = x0 + (x0 < fw - 1 ? 1 : 0);
        const float ly = sy - y0, hy = 1.f - ly, lx = sx - x0, hx = 1.f - lx;
        const float2 t00 = *reinterpret_cast<const float2 *>(F + ((size_t)y0 * fw + x0) * 2);
        const float2 t01 = *reinterpret_cast<const float2 *>(F + ((size_t)y0 * fw + x1) * 2);
        const float2 t10 = *reinterpret_cast<const float2 *>(F + ((size_t)y1 * fw + x0) * 2);
        const float2 t11 = *reinterpret_cast<const float2 *>(F + ((size_t)y1 * fw + x1) * 2);
        const float qx = blend(hy, ly, hx, lx, t00.x, t01.x, t10.x, t11.x);
        const float qy = blend(hy, ly, hx, lx, t00.y, t01.y, t10.y, t11.y);
        if (valid && pts_out) *reinterpret_cast<float2 *>(pts_out + ((size_t)f * HG_PTS + k) * 2) = make_float2(qx, qy);
        // main_new.py:561-563: x from the float W0/2, y from the integer H0//2
        const float ux = (float)((0.5 * w0 + (double)((b - HG_SIDE / 2) * HG_STRIDE_X)) / w0 * 2.0 - 1.0);
        const float uy = (float)((double)r / h0 * 2.0 - 1.0);
        p1x[j] = qx, p1y[j] = qy, p2x[j] = ux, p2y[j] = uy;
        if (valid) s4[0] += p1x[j], s4[1] += p1y[j], s4[2] += p2x[j], s4[3] += p2y[j];
    }

    // ---- Hartley normalisation of both point sets (centroid at 0, mean distance sqrt(2))
    wave_sum<4>(s4, red, tot_s, lane);
    const double c1x = s4[0] / HG_PTS, c1y = s4[1] / HG_PTS, c2x = s4[2] / HG_PTS, c2y = s4[3] / HG_PTS;
    double s2[2] = {0.0, 0.0};
#pragma unroll
    for (int j = 0; j < HG_PER_LANE; ++j) {
        if (lane + kWave * j < HG_PTS) {
            s2[0] += sqrt((p1x[j] - c1x) * (p1x[j] - c1x) + (p1y[j] - c1y) * (p1y[j] - c1y));
            s2[1] += sqrt((p2x[j] - c2x) * (p2x[j] - c2x) + (p2y[j] - c2y) * (p2y[j] - c2y));
        }
    }
    wave_sum<2>(s2, red, tot_s, lane);
    const double md1 = s2[0] / HG_PTS, md2 = s2[1] / HG_PTS;
    // samples that coincide to within fp32 resolution (a constant field) carry no homography
    bool ok = md1 > 1e-6 * (1.0 + fmax(fabs(c1x), fabs(c1y))) && md2 > 0.0;
    const double n1 = ok ? 1.4142135623730951 / md1 : 0.0, n2 = ok ? 1.4142135623730951 / md2 : 0.0;
#pragma unroll
    for (int j = 0; j < HG_PER_LANE; ++j) {
        p1x[j] = (p1x[j] - c1x) * n1, p1y[j] = (p1y[j] - c1y) * n1;
        p2x[j] = (p2x[j] - c2x) * n2, p2y[j] = (p2y[j] - c2y) * n2;
    }

    // ---- DLT with h33 = 1 in the normalised coordinates
    double h[8];
    {
        double acc[HG_SUMS];
#pragma unroll
        for (int k = 0; k < HG_SUMS; ++k) acc[k] = 0.0;
#pragma unroll
        for (int j = 0; j < HG_PER_LANE; ++j) {
            if (lane + kWave * j < HG_PTS) {
                const double x = p1x[j], y = p1y[j], u = p2x[j], v = p2y[j];
                const double au[8] = {x, y, 1.0, 0.0, 0.0, 0.0, -x * u, -y * u};
                const double av[8] = {0.0, 0.0, 0.0, x, y, 1.0, -x * v, -y * v};
                accum_row(acc, au, u);
                accum_row(acc, av, v);
            }
        }
        wave_sum<HG_SUMS>(acc, red, tot_s, lane);
        ok = chol_solve8(acc, h) && ok;
    }

    // ---- Gauss-Newton on the reprojection error (the same minimiser in normalised coordinates: they scale it by n2^2)
    for (int it = 0; it < HG_MAX_ITERS && ok; ++it) {
        double acc[HG_SUMS];
#pragma unroll
        for (int k = 0; k < HG_SUMS; ++k) acc[k] = 0.0;
#pragma unroll
        for (int j = 0; j < HG_PER_LANE; ++j) {
            if (lane + kWave * j < HG_PTS) {
                const double x = p1x[j], y = p1y[j];
                const double iw = 1.0 / (h[6] * x + h[7] * y + 1.0);
                const double u = (h[0] * x + h[1] * y + h[2]) * iw, v = (h[3] * x + h[4] * y + h[5]) * iw;
                const double xi = x * iw, yi = y * iw;
                const double ju[8] = {xi, yi, iw, 0.0, 0.0, 0.0, -xi * u, -yi * u};
                const double jv[8] = {0.0, 0.0, 0.0, xi, yi, iw, -xi * v, -yi * v};
                accum_row(acc, ju, p2x[j] - u);
                accum_row(acc, jv, p2y[j] - v);
            }
        }
        wave_sum<HG_SUMS>(acc, red, tot_s, lane);
        double d[8];
        ok = chol_solve8(acc, d);
        double dmax = 0.0, hmax = 0.0;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            h[k] += d[k];
            dmax = fmax(dmax, fabs(d[k])), hmax = fmax(hmax, fabs(h[k]));
        }
        if (dmax < 1e-12 * (1.0 + hmax)) break;
    }

    // ---- back to pixel-normalised coordinates: M = T2^-1 Hn T1, m33 = 1
    double m[9];
    {
        const double a0 = h[0] * n1, a1 = h[1] * n1, a2 = h[2] - n1 * (c1x * h[0] + c1y * h[1]);
        const double a3 = h[3] * n1, a4 = h[4] * n1, a5 = h[5] - n1 * (c1x * h[3] + c1y * h[4]);
        const double a6 = h[6] * n1, a7 = h[7] * n1, a8 = 1.0 - n1 * (c1x * h[6] + c1y * h[7]);
        const double i2 = 1.0 / n2, s = 1.0 / a8;
        m[0] = (a0 * i2 + c2x * a6) * s, m[1] = (a1 * i2 + c2x * a7) * s, m[2] = (a2 * i2 + c2x * a8) * s;
        m[3] = (a3 * i2 + c2y * a6) * s, m[4] = (a4 * i2 + c2y * a7) * s, m[5] = (a5 * i2 + c2y * a8) * s;
        m[6] = a6 * s, m[7] = a7 * s, m[8] = 1.0;
    }
#pragma unroll
    for (int k = 0; k < 9; ++k) ok = ok && isfinite(m[k]);

    // ---- corners (main_new.py:572-574: np.float32 points, cv2.perspectiveTransform) and the frame's bounds in source pixels
    const double e = (double)0.992f;
    const double cx[4] = {-1.0, -1.0, e, e}, cy[4] = {-1.0, e, e, -1.0};
    double X[4], Y[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const double w = m[6] * cx[q] + m[7] * cy[q] + m[8];
        const double iw = fabs(w) > (double)FLT_EPSILON ? 1.0 / w : 0.0;
        const float x = (float)((m[0] * cx[q] + m[1] * cy[q] + m[2]) * iw), y = (float)((m[3] * cx[q] + m[4] * cy[q] + m[5]) * iw);
        X[q] = ((double)x + 1.0) * w0 / 2.0, Y[q] = ((double)y + 1.0) * h0 / 2.0;
        ok = ok && isfinite(X[q]) && isfinite(Y[q]);
    }
    if (lane == 0) {
        const double nan = __builtin_nan("");
#pragma unroll
        for (int k = 0; k < 9; ++k) m_out[(size_t)f * 9 + k] = ok ? m[k] : nan;
        const float fnan = __builtin_nanf("");
        float *bo = bounds_out + (size_t)f * 4;
        bo[0] = ok ? (float)fmax(Y[0], Y[3]) : fnan;   // top
        bo[1] = ok ? (float)fmin(Y[1], Y[2]) : fnan;   // bottom
        bo[2] = ok ? (float)fmax(X[0], X[1]) : fnan;   // left
        bo[3] = ok ? (float)fmin(X[2], X[3]) : fnan;   // right
    }
}

}  // namespace
}  // namespace pws

using namespace pws;

extern "C" int pws_field_homography(const float *field, int n, int fh, int fw, int h0, int w0, double *m_out, float *bounds_out,
                                    float *pts_out, pws_stream_t stream) {
    PWS_REQUIRE(n >= 0 && fh > 0 && fw > 0, "pws_field_homography: bad shape");
    PWS_REQUIRE(h0 >= 300 && w0 >= 600, "pws_field_homography: the 20 x 20 sampling lattice needs a frame of at least 600 x 300 (got %d x %d)",
                w0, h0);
    if (n == 0) return PWS_OK;
    PWS_REQUIRE(field && m_out && bounds_out, "pws_field_homography: NULL pointer");
    PWS_REQUIRE((reinterpret_cast<size_t>(field) & 7) == 0 && (reinterpret_cast<size_t>(pts_out) & 7) == 0,
                "pws_field_homography: field and pts_out must be 8-byte aligned");
    PWS_REQUIRE((reinterpret_cast<size_t>(m_out) & 7) == 0 && (reinterpret_cast<size_t>(bounds_out) & 3) == 0,
                "pws_field_homography: m_out must be 8-byte aligned and bounds_out 4-byte aligned");
    // the resize's source scale, as pws_upsample_bilinear_ac / the fused warps compute it
    const float ry = (float)(fh - 1) / (float)(h0 - 1), rx = (float)(fw - 1) / (float)(w0 - 1);
    ProfScope prof(KID_FIELD_HOMOGRAPHY, (double)n * (HG_MAX_ITERS + 1) * HG_PTS * 2 * HG_SUMS * 2, (double)n * HG_PTS * 4 * 8,
                   as_stream(stream));
    hipLaunchKernelGGL(field_homography_kernel, dim3((unsigned)n), dim3(kWave), 0, as_stream(stream), field, fh, fw, h0, w0, ry, rx, m_out,
                       bounds_out, pts_out);
    return check_launch("field_homography_kernel");
}
