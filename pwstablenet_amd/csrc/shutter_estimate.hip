// Rolling-shutter estimate (stream.estimate_rolling_shutter; VideoStabilizer(rolling_shutter="auto")): the share r of the frame interval
// that the readout takes from the top row to the bottom row, from what smoothing has already measured.  No counterpart in the reference.
//
// Definition (restated in tests/shutter_est_ref.py; include/pwstable.h pws_shutter_terms has it in full).  A block of frame k on a row
// exposed r c later than the centre row, c = clamp(y / (H0 - 1), -1/2, 1/2), is found in frame k-1 on nearly the same row: between the two
// exposures the camera moved by the pair's motion plus r c times the change of its velocity, dV = rates[k] - rates[k-1].  The similarity
// that motion_fit_kernel fitted absorbs the first; z = c (dl p + dw J p + (dx, dy)) it cannot.  r is the one coefficient of z after the
// vectors and z have each had their own least-squares similarity taken out, shared by all pairs of the clip.
//
//   shutter_terms_kernel     one workgroup per pair of ONE scene, 256 threads, the blocks dealt over the lanes (any number of blocks).  Three
//                            passes over the pair's blocks, each ending in motion_fit_kernel's sum: the valid blocks' mean squared residual
//                            against the pair's motion (the inlier threshold); the normal sums of the kept blocks' vectors and of z; the
//                            products of the two residuals.  The validity rule and the sums are motion_blocks.h's, shared with the fit.
//   shutter_estimate_kernel  one workgroup: the four columns' sums over all pairs in index order, then r_hat, its formal standard error,
//                            and the two sums that say how much the clip knew.
// fp64, every product and sum rounded once, one fixed order: the same bits on every run.  No atomics; all stores are plain vector stores.
#include "motion_blocks.h"

namespace pws {
namespace {

#pragma clang fp contract(off)   // as the float64 restatement rounds

__device__ __forceinline__ bool finite_row(const double *v) {
    return isfinite(v[0]) && isfinite(v[1]) && isfinite(v[2]) && isfinite(v[3]);
}

// z of a block: its row's share c of the readout times the velocity change's field at its centre
__device__ __forceinline__ void regressor(const Blk &b, const double (*dv)[4], double hm1, double &zx, double &zy) {
    const double q = b.y / hm1;
    const double c = q > 0.5 ? 0.5 : (q < -0.5 ? -0.5 : q);
    const double *v = dv[c >= 0.0 ? 0 : 1];
    zx = c * ((v[0] * b.x - v[1] * b.y) + v[2]);
    zy = c * ((v[0] * b.y + v[1] * b.x) + v[3]);
}

// the fit's closed-form normal equations (motion_fit_kernel's), from N, Sx, Sy, den and the four sums of the fitted vectors
__device__ __forceinline__ Sim similarity(double s0, double sx, double sy, double den, double sdx, double sdy, double c, double d) {
    Sim f;
    f.a1 = (c - (sx * sdx + sy * sdy) / s0) / den;
    f.b = (d - (sx * sdy - sy * sdx) / s0) / den;
    f.tx = ((sdx - f.a1 * sx) + f.b * sy) / s0;
    f.ty = ((sdy - f.b * sx) - f.a1 * sy) / s0;
    return f;
}

__global__ void __launch_bounds__(MO_THREADS) shutter_terms_kernel(const short *__restrict__ mv, const int *__restrict__ sad,
                                                                   const int *__restrict__ activity, const double *__restrict__ motion,
                                                                   const double *__restrict__ rates, int n, int h, int w, int R, int nby, int nbx,
                                                                   int min_activity, double sx, double sy, double h0,
                                                                   double *__restrict__ terms) {
    __shared__ double part[MO_WAVES][8];
    const int tid = threadIdx.x, k = blockIdx.x;
    double *o = terms + (size_t)k * 4;
    // (uniform from here on: every thread reads the same rows and gets the same sums, so every thread takes every barrier)
    bool ok = k >= 2 && k <= n - 2;   // both velocity differences come from real pairs of the scene
    if (ok) ok = finite_row(motion + (size_t)(k - 1) * 4) && finite_row(motion + (size_t)k * 4) && finite_row(motion + (size_t)(k + 1) * 4);
    double out[4] = {0.0, 0.0, 0.0, 0.0};
    if (ok) {
        const int nb = nby * nbx;
        const double cx0 = 0.5 * (double)(w - 1), cy0 = 0.5 * (double)(h - 1), hm1 = h0 - 1.0;
        const double *m = motion + (size_t)k * 4;
        const Sim fit = {m[0] - 1.0, m[1], m[2], m[3]};
        double q[2] = {0.0, 0.0};   // the valid blocks and their squared residuals against the pair's motion
        for (int i = tid; i < nb; i += MO_THREADS) {
            const Blk b = load_block(mv, sad, activity, (size_t)k * nb + i, i, nbx, R, min_activity, cx0, cy0, sx, sy);
            if (!b.valid) continue;
            q[0] += 1.0, q[1] += residual2(fit, b);
        }
        block_sum<2>(q, part);
        ok = (int)q[0] >= MO_MIN_BLOCKS;
        if (ok) {
            const double m4 = 4.0 * (q[1] / q[0]), floor2 = sx * sy;
            const double thr = m4 > floor2 ? m4 : floor2;   // the rule of the fit's own rounds
            double dv[2][4];
#pragma unroll
            for (int s = 0; s < 2; ++s) {
#pragma unroll
                for (int c = 0; c < 4; ++c) dv[s][c] = rates[(size_t)k * 8 + s * 4 + c] - rates[(size_t)(k - 1) * 8 + s * 4 + c];
            }
            double s[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // N, Sx, Sy, S(x^2 + y^2), Sdx, Sdy, S(x dx + y dy), S(x dy - y dx)
            double u[4] = {0, 0, 0, 0};               // Szx, Szy, S(x zx + y zy), S(x zy - y zx)
            for (int i = tid; i < nb; i += MO_THREADS) {
                const Blk b = load_block(mv, sad, activity, (size_t)k * nb + i, i, nbx, R, min_activity, cx0, cy0, sx, sy);
                if (!b.valid || !(residual2(fit, b) <= thr)) continue;
                double zx, zy;
                regressor(b, dv, hm1, zx, zy);
                s[0] += 1.0, s[1] += b.x, s[2] += b.y, s[3] += b.x * b.x + b.y * b.y, s[4] += b.dx, s[5] += b.dy;
                s[6] += b.x * b.dx + b.y * b.dy, s[7] += b.x * b.dy - b.y * b.dx;
                u[0] += zx, u[1] += zy, u[2] += b.x * zx + b.y * zy, u[3] += b.x * zy - b.y * zx;
            }
            block_sum<8>(s, part);
            block_sum<4>(u, part);
            const double den = s[3] - (s[1] * s[1] + s[2] * s[2]) / s[0];
            ok = (int)s[0] >= MO_MIN_BLOCKS && den > 0.0;
            if (ok) {
                const Sim fv = similarity(s[0], s[1], s[2], den, s[4], s[5], s[6], s[7]);
                const Sim fz = similarity(s[0], s[1], s[2], den, u[0], u[1], u[2], u[3]);
                double t[3] = {0.0, 0.0, 0.0};   // S e . z_perp, S z_perp . z_perp, S e . e
                for (int i = tid; i < nb; i += MO_THREADS) {
                    const Blk b = load_block(mv, sad, activity, (size_t)k * nb + i, i, nbx, R, min_activity, cx0, cy0, sx, sy);
                    if (!b.valid || !(residual2(fit, b) <= thr)) continue;
                    double zx, zy;
                    regressor(b, dv, hm1, zx, zy);
                    const double ex = b.dx - ((fv.a1 * b.x - fv.b * b.y) + fv.tx), ey = b.dy - ((fv.b * b.x + fv.a1 * b.y) + fv.ty);
                    const double px = zx - ((fz.a1 * b.x - fz.b * b.y) + fz.tx), py = zy - ((fz.b * b.x + fz.a1 * b.y) + fz.ty);
                    t[0] += ex * px + ey * py, t[1] += px * px + py * py, t[2] += ex * ex + ey * ey;
                }
                block_sum<3>(t, part);
                out[0] = t[0], out[1] = t[1], out[2] = t[2], out[3] = s[0];
            }
        }
    }
    if (tid == 0) o[0] = out[0], o[1] = out[1], o[2] = out[2], o[3] = out[3];
}

// the clip's estimate: lane c sums column c over the rows in index order
__global__ void __launch_bounds__(kWave) shutter_estimate_kernel(const double *__restrict__ terms, int n, double *__restrict__ out4) {
    __shared__ double col[4];
    __shared__ int rows;
    const int tid = threadIdx.x;
    if (tid < 4) {
        double s = 0.0;
        int m = 0;
        for (int k = 0; k < n; ++k) {
            const double v = terms[(size_t)k * 4 + tid];
            s += v;
            m += v > 0.0 ? 1 : 0;
        }
        col[tid] = s;
        if (tid == 3) rows = m;   // the rows whose count is positive
    }
    __syncthreads();
    if (tid == 0) {
        const double N = col[0], D = col[1], E = col[2], cnt = col[3];
        const double dof = (2.0 * cnt - 4.0 * (double)rows) - 1.0;
        const bool ok = D > 0.0 && dof > 0.0;
        const double r = N / D, rest = E - r * N;
        out4[0] = ok ? r : __longlong_as_double(0x7ff8000000000000LL);
        out4[1] = ok ? sqrt(((rest > 0.0 ? rest : 0.0) / dof) / D) : __longlong_as_double(0x7ff0000000000000LL);
        out4[2] = D, out4[3] = cnt;
    }
}

}  // namespace
}  // namespace pws

using namespace pws;

extern "C" int pws_shutter_terms(const short *mv, const int *sad, const int *activity, const double *motion, const double *rates, int n, int h,
                                 int w, int radius, int min_activity, double sx, double sy, double h0, double *terms, pws_stream_t stream) {
    PWS_REQUIRE(n >= 0 && h > 0 && w > 0, "pws_shutter_terms: bad shape (n %d, h %d, w %d)", n, h, w);
    PWS_REQUIRE(radius >= 1 && radius <= MO_RMAX, "pws_shutter_terms: radius must be 1 .. %d, got %d", MO_RMAX, radius);
    const long long nby = ((long long)h - 2 * radius) / MO_B, nbx = ((long long)w - 2 * radius) / MO_B;
    PWS_REQUIRE(h - 2 * radius >= MO_B && w - 2 * radius >= MO_B, "pws_shutter_terms: a %d x %d plane holds no 16 x 16 block inside a margin of %d", h,
                w, radius);
    PWS_REQUIRE(nby * nbx <= (1 << 20), "pws_shutter_terms: %lld x %lld blocks per plane, at most 2^20", nby, nbx);
    PWS_REQUIRE(sx > 0.0 && sy > 0.0 && sx <= 1e6 && sy <= 1e6, "pws_shutter_terms: the pixel scale must be positive and finite, got (%g, %g)", sx, sy);
    PWS_REQUIRE(h0 > 1.0 && h0 <= 1e9, "pws_shutter_terms: the frame height must lie in (1, 1e9], got %g", h0);
    PWS_REQUIRE(n <= (1 << 24), "pws_shutter_terms: a scene of %d frames, at most 2^24", n);
    if (n == 0) return PWS_OK;
    PWS_REQUIRE(mv && sad && activity && motion && rates && terms, "pws_shutter_terms: NULL pointer");
    PWS_REQUIRE(((reinterpret_cast<size_t>(mv) | reinterpret_cast<size_t>(sad) | reinterpret_cast<size_t>(activity)) & 3) == 0 &&
                    ((reinterpret_cast<size_t>(motion) | reinterpret_cast<size_t>(rates) | reinterpret_cast<size_t>(terms)) & 7) == 0,
                "pws_shutter_terms: mv, sad and activity must be 4-byte aligned, motion, rates and terms 8-byte aligned");
    hipLaunchKernelGGL(shutter_terms_kernel, dim3((unsigned)n), dim3(MO_THREADS), 0, as_stream(stream), mv, sad, activity, motion, rates, n, h, w,
                       radius, (int)nby, (int)nbx, min_activity, sx, sy, h0, terms);
    return check_launch("shutter_terms_kernel");
}

extern "C" int pws_shutter_estimate(const double *terms, int n, double *out4, pws_stream_t stream) {
    PWS_REQUIRE(n >= 0 && n <= (1 << 24), "pws_shutter_estimate: bad shape (n %d), at most 2^24 rows", n);
    PWS_REQUIRE(out4 && (terms || n == 0), "pws_shutter_estimate: NULL pointer");
    PWS_REQUIRE(((reinterpret_cast<size_t>(terms) | reinterpret_cast<size_t>(out4)) & 7) == 0, "pws_shutter_estimate: terms and out4 must be 8-byte aligned");
    hipLaunchKernelGGL(shutter_estimate_kernel, dim3(1), dim3(kWave), 0, as_stream(stream), terms, n, out4);
    return check_launch("shutter_estimate_kernel");
}
