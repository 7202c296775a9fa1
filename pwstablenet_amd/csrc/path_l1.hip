// The L1-optimal camera path (stream.optimal_path; Grundmann, Kwatra, Essa, CVPR 2011): per scene and per pose component the path inside a box
// around the measured one whose first, second and third differences have the least weighted L1 norms -- static, constant-velocity and
// constant-acceleration pieces -- and per frame the correction onto it.  No counterpart in the reference.
//
// Definition (restated in tests/l1_path_ref.py; include/pwstable.h pws_l1_path has it in full).  P is path_pose.h's scan.  Per component, with
// x = (P^ - P) / b and q = P / b:  minimise sum_k w_k |D_k (x + q)|_1, k = 1, 2, 3, subject to -1 <= x <= 1, as the LP with e_k >= |D_k (x + q)|,
// by a primal-dual interior-point method.  Every constraint keeps its slack s and multiplier l as state of its own (s is never formed again
// from e - D_k (x + q): at the optimum it lies far below that difference's rounding).  Per Newton step the slacks' elimination leaves the SPD
// band  (sum_k D_k^T Theta_k D_k + diag(gU + gL)) dx = rhs,  Theta = 4 g+ g- / (g+ + g-), g = l / s,  three sub-diagonals wide.
//
// Three stream-ordered launches: the scan on one lane; the solver, one workgroup of 256 threads per component; D over frames.  In the solver
// the threads take the frames in turn for everything that is local -- the weights, the band, the right-hand side, the slack and multiplier
// steps, the step length, the update -- and one lane runs the LDL^T factor and the two substitutions, whose chain (three pivots, three
// sub-diagonal entries, three solution values) stays in registers while its operands, which do not depend on the chain, are loaded four rows
// ahead.  The state, 35 doubles per frame and component, is in the workspace.  Every sum is taken in one order (thread i % 256 over its
// frames, then a halving tree) and the step length is a min: the same bits on every run, no atomics.
#include <cmath>

#include "common.h"
#include "path_pose.h"

namespace pws {
namespace {

constexpr int L1_THREADS = 256, L1_MAX_STEPS = 64, L1_MAX_FRAMES = 65536, L1_AHEAD = 4;
constexpr double L1_MU = 10.0, L1_TOL = 1e-9, L1_KEEP = 0.99;
constexpr double L1_PIVOT_FLOOR = 0x1p-44, L1_PIVOT_HUGE = 1e128;   // a pivot below that share of its diagonal entry is rounding noise: the row is skipped

// the workspace: (n, 4) U = P^ - P, then per component L1_ARRAYS arrays of n doubles (row j of D_k at index j)
enum {
    L1_X = 0, L1_E = 1, L1_SP = 4, L1_SM = 7, L1_LP = 10, L1_LM = 13,   // x; per k = 1, 2, 3: e, s+, s-, l+, l-
    L1_SU = 16, L1_SL, L1_LU, L1_LL,                                   // the box: slacks 1 - x, 1 + x and their multipliers
    L1_TH = 20, L1_Y = 23,                                             // per k: Theta, and the right-hand side's term per row
    L1_A = 26, L1_RHS = 30, L1_L = 31, L1_DX = 34, L1_ARRAYS = 35      // the band A_d[i] = H[i, i + d]; rhs; L's three sub-diagonals; dx
};

#pragma clang fp contract(off)   // every product and every sum rounded once, as the float64 restatement does

struct L1Params {
    double b[4], w[3];
};

__device__ __forceinline__ double l1_coef(int k, int a) {   // the k-th forward difference: row j over columns j .. j + k
    return k == 1 ? (a == 0 ? -1.0 : 1.0) : k == 2 ? (a == 1 ? -2.0 : 1.0) : (a == 0 ? -1.0 : a == 1 ? 3.0 : a == 2 ? -3.0 : 1.0);
}

template <class F>
__device__ __forceinline__ double l1_diff(int k, int j, F y) {
    if (k == 1) return y(j + 1) - y(j);
    if (k == 2) return (y(j) - 2.0 * y(j + 1)) + y(j + 2);
    return ((y(j + 3) - 3.0 * y(j + 2)) + 3.0 * y(j + 1)) - y(j);
}

// (sum_k D_k^T col_k)[i]: k = 1, 2, 3 and per k the columns a = 0 .. k of row j = i - a
template <class F>
__device__ __forceinline__ double l1_dt(int i, int n, F col) {
    double acc = 0.0;
#pragma unroll
    for (int k = 1; k <= 3; ++k)
#pragma unroll
        for (int a = 0; a <= k; ++a) {
            const int j = i - a;
            if (j >= 0 && j < n - k) acc = acc + l1_coef(k, a) * col(k, j);
        }
    return acc;
}

// three sums (or minima) over the workgroup at once, in one fixed order; every thread gets the results
template <bool MIN>
__device__ __forceinline__ void l1_reduce(double (*red)[L1_THREADS], double &a, double &b, double &c) {
    const int tid = threadIdx.x;
    red[0][tid] = a, red[1][tid] = b, red[2][tid] = c;
    __syncthreads();
    for (int s = L1_THREADS / 2; s >= 1; s >>= 1) {
        if (tid < s) {
#pragma unroll
            for (int v = 0; v < 3; ++v) red[v][tid] = MIN ? fmin(red[v][tid], red[v][tid + s]) : red[v][tid] + red[v][tid + s];
        }
        __syncthreads();
    }
    a = red[0][0], b = red[1][0], c = red[2][0];
    __syncthreads();
}

// what row j of D_k contributes to a Newton step, from its slacks and multipliers
struct L1Row {
    double gp, gm, vp, vm, G, be;
};
__device__ __forceinline__ L1Row l1_row(const double *W, size_t n, int k, int j, double t, double wk) {
    const double sp = W[(L1_SP + k - 1) * n + j], sm = W[(L1_SM + k - 1) * n + j], lp = W[(L1_LP + k - 1) * n + j], lm = W[(L1_LM + k - 1) * n + j];
    L1Row r;
    r.gp = lp / sp, r.gm = lm / sm;
    r.vp = 1.0 / (t * sp), r.vm = 1.0 / (t * sm);
    r.G = r.gp + r.gm;
    r.be = (r.vp + r.vm) - wk;
    return r;
}

// the steps of row j of D_k once dx stands: (de, ds+, ds-, dl+, dl-)
__device__ __forceinline__ void l1_row_step(const double *W, size_t n, int k, int j, double t, double wk, double *o) {
    const L1Row r = l1_row(W, n, k, j, t, wk);
    const double *dx = W + L1_DX * n;
    const double a = l1_diff(k, j, [&](int i) { return dx[i]; });
    o[0] = (r.be + (r.gp - r.gm) * a) / r.G;
    o[1] = o[0] - a, o[2] = o[0] + a;
    o[3] = (r.vp - W[(L1_LP + k - 1) * n + j]) - r.gp * o[1];
    o[4] = (r.vm - W[(L1_LM + k - 1) * n + j]) - r.gm * o[2];
}
// the box's steps at frame i: (dsU, dsL, dlU, dlL)
__device__ __forceinline__ void l1_box_step(const double *W, size_t n, int i, double t, double *o) {
    const double sU = W[L1_SU * n + i], sL = W[L1_SL * n + i], lU = W[L1_LU * n + i], lL = W[L1_LL * n + i], dx = W[L1_DX * n + i];
    const double gU = lU / sU, gL = lL / sL, vU = 1.0 / (t * sU), vL = 1.0 / (t * sL);
    o[0] = 0.0 - dx, o[1] = dx;
    o[2] = (vU - lU) + gU * dx, o[3] = (vL - lL) - gL * dx;
}

__device__ __forceinline__ void l1_ratio(double val, double d, double &rmin, double &fin) {
    if (!isfinite(d)) fin = 0.0;
    if (d < 0.0) rmin = fmin(rmin, val / (0.0 - d));
}

// LDL^T without pivoting of the band and both substitutions, on the calling lane.  Returns false when a pivot was not finite.
__device__ bool l1_band_solve(double *__restrict__ W, size_t n_, int n) {
    const double *__restrict__ A0 = W + (L1_A + 0) * n_, *__restrict__ A1 = W + (L1_A + 1) * n_, *__restrict__ A2 = W + (L1_A + 2) * n_,
                 *__restrict__ A3 = W + (L1_A + 3) * n_, *__restrict__ rhs = W + L1_RHS * n_;
    double *__restrict__ l1 = W + (L1_L + 0) * n_, *__restrict__ l2 = W + (L1_L + 1) * n_, *__restrict__ l3 = W + (L1_L + 2) * n_,
           *__restrict__ dx = W + L1_DX * n_;
    double D1 = 1.0, D2 = 1.0, D3 = 1.0;      // D[i-1], D[i-2], D[i-3]
    double l1p = 0.0, l2p = 0.0, l1pp = 0.0;   // l1[i-1], l2[i-1], l1[i-2]
    double z1 = 0.0, z2 = 0.0, z3 = 0.0;
    bool ok = true;
    double cur[L1_AHEAD][5], nxt[L1_AHEAD][5];   // per row: A0[i], A1[i-1], A2[i-2], A3[i-3], rhs[i]
    auto fetch = [&](int i, double *o) {
        const bool in = i < n;
        o[0] = in ? A0[i] : 1.0, o[1] = in && i >= 1 ? A1[i - 1] : 0.0, o[2] = in && i >= 2 ? A2[i - 2] : 0.0, o[3] = in && i >= 3 ? A3[i - 3] : 0.0;
        o[4] = in ? rhs[i] : 0.0;
    };
#pragma unroll
    for (int r = 0; r < L1_AHEAD; ++r) fetch(r, cur[r]);
    for (int i0 = 0; i0 < n; i0 += L1_AHEAD) {
#pragma unroll
        for (int r = 0; r < L1_AHEAD; ++r) fetch(i0 + L1_AHEAD + r, nxt[r]);
#pragma unroll
        for (int r = 0; r < L1_AHEAD; ++r) {
            const int i = i0 + r;
            if (i < n) {
                const double u3 = cur[r][3];
                const double c3 = u3 / D3;
                const double u2 = cur[r][2] - u3 * l1pp;
                const double c2 = u2 / D2;
                const double u1 = (cur[r][1] - u3 * l2p) - u2 * l1p;
                const double c1 = u1 / D1;
                double D = ((cur[r][0] - u3 * c3) - u2 * c2) - u1 * c1;
                const double z = ((cur[r][4] - c1 * z1) - c2 * z2) - c3 * z3;
                if (!(D > L1_PIVOT_FLOOR * cur[r][0])) {   // (also a NaN)
                    ok = ok && isfinite(D);
                    D = L1_PIVOT_HUGE;
                }
                l1[i] = c1, l2[i] = c2, l3[i] = c3, dx[i] = z / D;
                D3 = D2, D2 = D1, D1 = D;
                l1pp = l1p, l1p = c1, l2p = c2;
                z3 = z2, z2 = z1, z1 = z;
            }
        }
#pragma unroll
        for (int r = 0; r < L1_AHEAD; ++r)
#pragma unroll
            for (int v = 0; v < 5; ++v) cur[r][v] = nxt[r][v];
    }
    // L^T dx = w, in place, from the last row up: row i reads w[i], l1[i+1], l2[i+2], l3[i+3] (this lane's own stores), four rows ahead again
    double x1 = 0.0, x2 = 0.0, x3 = 0.0;
    auto fetch_up = [&](int i, double *o) {
        o[0] = i >= 0 ? dx[i] : 0.0;
        o[1] = i >= 0 && i + 1 < n ? l1[i + 1] : 0.0, o[2] = i >= 0 && i + 2 < n ? l2[i + 2] : 0.0, o[3] = i >= 0 && i + 3 < n ? l3[i + 3] : 0.0;
    };
#pragma unroll
    for (int r = 0; r < L1_AHEAD; ++r) fetch_up(n - 1 - r, cur[r]);
    for (int i0 = n - 1; i0 >= 0; i0 -= L1_AHEAD) {
#pragma unroll
        for (int r = 0; r < L1_AHEAD; ++r) fetch_up(i0 - L1_AHEAD - r, nxt[r]);
#pragma unroll
        for (int r = 0; r < L1_AHEAD; ++r) {
            const int i = i0 - r;
            if (i >= 0) {
                const double v = ((cur[r][0] - cur[r][1] * x1) - cur[r][2] * x2) - cur[r][3] * x3;
                dx[i] = v;
                x3 = x2, x2 = x1, x1 = v;
            }
        }
#pragma unroll
        for (int r = 0; r < L1_AHEAD; ++r)
#pragma unroll
            for (int v = 0; v < 4; ++v) cur[r][v] = nxt[r][v];
    }
    return ok;
}

__global__ void __launch_bounds__(64) l1_scan_kernel(const double *__restrict__ motion, int n, double *path) {
    if (threadIdx.x == 0) pose_scan(motion, n, path);
}

__global__ void __launch_bounds__(L1_THREADS) l1_solve_kernel(const double *__restrict__ path, int n, L1Params prm, double *ws, double *info) {
    __shared__ double red[3][L1_THREADS];
    __shared__ int solved;
    const int tid = threadIdx.x, c = blockIdx.x;
    const size_t n_ = (size_t)n;
    double *U = ws;
    double *W = ws + 4 * n_ + (size_t)c * L1_ARRAYS * n_;
    if (n <= 3) {   // no third difference: the measured path itself
        for (int i = tid; i < n; i += L1_THREADS) U[(size_t)i * 4 + c] = 0.0;
        if (tid == 0) info[c * 4 + 0] = 0.0, info[c * 4 + 1] = 0.0, info[c * 4 + 2] = 0.0, info[c * 4 + 3] = 1.0;
        return;
    }
    const double b = prm.b[c];
    const double wmax = fmax(prm.w[0], fmax(prm.w[1], prm.w[2]));
    // the start: x = 0, e_k = |D_k q| + 1, every multiplier 1 / s
    for (int i = tid; i < n; i += L1_THREADS) {
        W[L1_X * n_ + i] = 0.0;
        W[L1_SU * n_ + i] = 1.0, W[L1_SL * n_ + i] = 1.0, W[L1_LU * n_ + i] = 1.0, W[L1_LL * n_ + i] = 1.0;
#pragma unroll
        for (int k = 1; k <= 3; ++k)
            if (i < n - k) {
                const double r = l1_diff(k, i, [&](int j) { return path[(size_t)j * 4 + c] / b; });
                const double e = fabs(r) + 1.0, sp = e - r, sm = e + r;
                W[(L1_E + k - 1) * n_ + i] = e, W[(L1_SP + k - 1) * n_ + i] = sp, W[(L1_SM + k - 1) * n_ + i] = sm;
                W[(L1_LP + k - 1) * n_ + i] = 1.0 / sp, W[(L1_LM + k - 1) * n_ + i] = 1.0 / sm;
            }
    }
    __syncthreads();
    const double m = (double)(8 * n - 12);   // constraints: 2 (n-1 + n-2 + n-3) + 2 n
    int steps = 0;
    double eta = 0.0, f = 0.0, conv = 0.0;
    for (;;) {
        // the surrogate gap eta = s . l, the scaled objective f, the dual residual's squared norm
        double a_eta = 0.0, a_f = 0.0, a_res = 0.0;
        for (int i = tid; i < n; i += L1_THREADS) {
            double re2[3] = {0.0, 0.0, 0.0};
#pragma unroll
            for (int k = 1; k <= 3; ++k)
                if (i < n - k) {
                    const double sp = W[(L1_SP + k - 1) * n_ + i], sm = W[(L1_SM + k - 1) * n_ + i], lp = W[(L1_LP + k - 1) * n_ + i],
                                 lm = W[(L1_LM + k - 1) * n_ + i];
                    a_eta = a_eta + sp * lp;
                    a_eta = a_eta + sm * lm;
                    a_f = a_f + prm.w[k - 1] * W[(L1_E + k - 1) * n_ + i];
                    const double re = (prm.w[k - 1] - lp) - lm;
                    re2[k - 1] = re * re;
                }
            const double lU = W[L1_LU * n_ + i], lL = W[L1_LL * n_ + i];
            a_eta = a_eta + W[L1_SU * n_ + i] * lU;
            a_eta = a_eta + W[L1_SL * n_ + i] * lL;
            const double rx = l1_dt(i, n, [&](int k, int j) { return W[(L1_LP + k - 1) * n_ + j] - W[(L1_LM + k - 1) * n_ + j]; }) + (lU - lL);
            a_res = a_res + rx * rx;
#pragma unroll
            for (int k = 1; k <= 3; ++k)
                if (i < n - k) a_res = a_res + re2[k - 1];
        }
        l1_reduce<false>(red, a_eta, a_f, a_res);
        eta = a_eta, f = a_f;
        if (eta <= L1_TOL * fmax(1.0, f) && sqrt(a_res) <= L1_TOL * fmax(1.0, wmax)) {
            conv = 1.0;
            break;
        }
        if (steps == L1_MAX_STEPS) break;
        // (held once the gap's criterion is met: while t grows the band's conditioning keeps the dual residual at its rounding floor, about
        // 2e-7 at n = 200 and w = 100; a step at the same t only centres, and takes the residual to 1e-9 and below)
        const double t = (L1_MU * m) / fmax(eta, L1_TOL * fmax(1.0, f));
        // per row of every difference: Theta and the right-hand side's term
        for (int j = tid; j < n; j += L1_THREADS) {
#pragma unroll
            for (int k = 1; k <= 3; ++k)
                if (j < n - k) {
                    const L1Row r = l1_row(W, n_, k, j, t, prm.w[k - 1]);
                    W[(L1_TH + k - 1) * n_ + j] = ((4.0 * r.gp) * r.gm) / r.G;
                    W[(L1_Y + k - 1) * n_ + j] = (r.vp - r.vm) + ((r.gm - r.gp) * r.be) / r.G;
                }
        }
        __syncthreads();
        // per frame: the band's four entries (at most 9 terms each, k = 1, 2, 3 and per k the rows j = i - a) and the right-hand side
        for (int i = tid; i < n; i += L1_THREADS) {
#pragma unroll
            for (int d = 0; d <= 3; ++d) {
                double acc = 0.0;
#pragma unroll
                for (int k = 1; k <= 3; ++k)
#pragma unroll
                    for (int a = 0; a <= 3; ++a)
                        if (a + d <= k) {
                            const int j = i - a;
                            if (j >= 0 && j < n - k) acc = acc + W[(L1_TH + k - 1) * n_ + j] * (l1_coef(k, a) * l1_coef(k, a + d));
                        }
                if (d == 0) {
                    const double gU = W[L1_LU * n_ + i] / W[L1_SU * n_ + i], gL = W[L1_LL * n_ + i] / W[L1_SL * n_ + i];
                    acc = acc + (gU + gL);
                }
                W[(L1_A + d) * n_ + i] = acc;
            }
            const double vU = 1.0 / (t * W[L1_SU * n_ + i]), vL = 1.0 / (t * W[L1_SL * n_ + i]);
            W[L1_RHS * n_ + i] = (vL - vU) - l1_dt(i, n, [&](int k, int j) { return W[(L1_Y + k - 1) * n_ + j]; });
        }
        __syncthreads();
        if (tid == 0) solved = l1_band_solve(W, n_, n) ? 1 : 0;
        __syncthreads();
        // the largest step <= 1 that keeps 0.99 of every slack's and multiplier's distance to zero
        double rmin = INFINITY, fin = 1.0, unused = 0.0;
        for (int i = tid; i < n; i += L1_THREADS) {
            double o[5];
            if (!isfinite(W[L1_DX * n_ + i])) fin = 0.0;
#pragma unroll
            for (int k = 1; k <= 3; ++k)
                if (i < n - k) {
                    l1_row_step(W, n_, k, i, t, prm.w[k - 1], o);
                    if (!isfinite(o[0])) fin = 0.0;
                    l1_ratio(W[(L1_SP + k - 1) * n_ + i], o[1], rmin, fin);
                    l1_ratio(W[(L1_SM + k - 1) * n_ + i], o[2], rmin, fin);
                    l1_ratio(W[(L1_LP + k - 1) * n_ + i], o[3], rmin, fin);
                    l1_ratio(W[(L1_LM + k - 1) * n_ + i], o[4], rmin, fin);
                }
            l1_box_step(W, n_, i, t, o);
            l1_ratio(W[L1_SU * n_ + i], o[0], rmin, fin);
            l1_ratio(W[L1_SL * n_ + i], o[1], rmin, fin);
            l1_ratio(W[L1_LU * n_ + i], o[2], rmin, fin);
            l1_ratio(W[L1_LL * n_ + i], o[3], rmin, fin);
        }
        l1_reduce<true>(red, rmin, fin, unused);
        const double alpha = fmin(1.0, L1_KEEP * rmin);
        if (!solved || fin == 0.0 || !isfinite(alpha)) break;   // breakdown: the last iterate stands
        // the update: every row and frame from its own state and dx, which no thread writes here
        for (int i = tid; i < n; i += L1_THREADS) {
            double o[5];
#pragma unroll
            for (int k = 1; k <= 3; ++k)
                if (i < n - k) {
                    l1_row_step(W, n_, k, i, t, prm.w[k - 1], o);
                    double *e = W + (L1_E + k - 1) * n_ + i, *sp = W + (L1_SP + k - 1) * n_ + i, *sm = W + (L1_SM + k - 1) * n_ + i,
                           *lp = W + (L1_LP + k - 1) * n_ + i, *lm = W + (L1_LM + k - 1) * n_ + i;
                    *e = *e + alpha * o[0], *sp = *sp + alpha * o[1], *sm = *sm + alpha * o[2], *lp = *lp + alpha * o[3], *lm = *lm + alpha * o[4];
                }
            l1_box_step(W, n_, i, t, o);
            W[L1_X * n_ + i] = W[L1_X * n_ + i] + alpha * W[L1_DX * n_ + i];
            W[L1_SU * n_ + i] = W[L1_SU * n_ + i] + alpha * o[0], W[L1_SL * n_ + i] = W[L1_SL * n_ + i] + alpha * o[1];
            W[L1_LU * n_ + i] = W[L1_LU * n_ + i] + alpha * o[2], W[L1_LL * n_ + i] = W[L1_LL * n_ + i] + alpha * o[3];
        }
        __syncthreads();
        ++steps;
    }
    for (int i = tid; i < n; i += L1_THREADS) U[(size_t)i * 4 + c] = b * fmin(fmax(W[L1_X * n_ + i], -1.0), 1.0);
    if (tid == 0) info[c * 4 + 0] = (double)steps, info[c * 4 + 1] = eta, info[c * 4 + 2] = f, info[c * 4 + 3] = conv;
}

__global__ void __launch_bounds__(L1_THREADS) l1_correction_kernel(const double *__restrict__ path, const double *__restrict__ u, int n,
                                                                   double *__restrict__ d) {
    const int k = (int)(blockIdx.x * L1_THREADS + threadIdx.x);
    if (k >= n) return;
    const double *v = u + (size_t)k * 4;
    pose_correction(path + (size_t)k * 4, v[0], v[1], v[2], v[3], d + (size_t)k * 6);
}

}  // namespace
}  // namespace pws

using namespace pws;

extern "C" size_t pws_l1_path_workspace(int n) {
    return n > 0 ? (size_t)n * (4 + 4 * L1_ARRAYS) * sizeof(double) : 0;
}

extern "C" int pws_l1_path(const double *motion, int n, const double *bound, const double *weights, double *path, double *d, double *info,
                           void *workspace, size_t workspace_bytes, pws_stream_t stream) {
    PWS_REQUIRE(n >= 0, "pws_l1_path: bad shape (n %d)", n);
    PWS_REQUIRE(bound && weights, "pws_l1_path: NULL bound or weights");
    L1Params prm;
    for (int c = 0; c < 4; ++c) {
        PWS_REQUIRE(std::isfinite(bound[c]) && bound[c] > 0.0, "pws_l1_path: bound[%d] must be finite and > 0, got %g", c, bound[c]);
        prm.b[c] = bound[c];
    }
    for (int k = 0; k < 3; ++k) {
        PWS_REQUIRE(std::isfinite(weights[k]) && weights[k] > 0.0, "pws_l1_path: weights[%d] must be finite and > 0, got %g", k, weights[k]);
        prm.w[k] = weights[k];
    }
    if (n == 0) return PWS_OK;
    PWS_REQUIRE(motion && path && d && info && workspace, "pws_l1_path: NULL pointer");
    PWS_REQUIRE(((reinterpret_cast<size_t>(motion) | reinterpret_cast<size_t>(path) | reinterpret_cast<size_t>(d) | reinterpret_cast<size_t>(info) |
                  reinterpret_cast<size_t>(workspace)) & 7) == 0,
                "pws_l1_path: motion, path, d, info and workspace must be 8-byte aligned");
    PWS_REQUIRE(n <= L1_MAX_FRAMES, "pws_l1_path: a scene of %d frames, at most %d (the solver's band solve is sequential)", n, L1_MAX_FRAMES);
    PWS_REQUIRE(workspace_bytes >= pws_l1_path_workspace(n), "pws_l1_path: workspace of %zu bytes, pws_l1_path_workspace(%d) is %zu",
                workspace_bytes, n, pws_l1_path_workspace(n));
    double *ws = static_cast<double *>(workspace);
    hipLaunchKernelGGL(l1_scan_kernel, dim3(1), dim3(64), 0, as_stream(stream), motion, n, path);
    int rc = check_launch("l1_scan_kernel");
    if (rc != PWS_OK) return rc;
    hipLaunchKernelGGL(l1_solve_kernel, dim3(4), dim3(L1_THREADS), 0, as_stream(stream), path, n, prm, ws, info);
    rc = check_launch("l1_solve_kernel");
    if (rc != PWS_OK) return rc;
    hipLaunchKernelGGL(l1_correction_kernel, dim3((unsigned)((n + L1_THREADS - 1) / L1_THREADS)), dim3(L1_THREADS), 0, as_stream(stream), path, ws, n,
                       d);
    return check_launch("l1_correction_kernel");
}
