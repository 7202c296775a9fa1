// The two ends that every path model shares (path_smooth.hip: the Gaussian low-pass; path_l1.hip: the L1-optimal path): the scan that
// adds a scene's per-pair motion up to the measured pose P[k] = (lambda, theta, cx, cy), and the correction D[k] = C_k^-1 o C^_k from the
// measured pose and the model's change of it.  include/pwstable.h pws_path_smooth has the definitions; tests/path_ref.py restates them.
#pragma once
#include "common.h"

namespace pws {

#pragma clang fp contract(off)   // every product and every sum rounded once, as the float64 restatement does

__device__ __forceinline__ bool finite4(const double *v) {
    return isfinite(v[0]) && isfinite(v[1]) && isfinite(v[2]) && isfinite(v[3]);
}

// P[0 .. n-1] from motion[1 .. n-1], on the calling lane: strictly sequential (a scene is thousands of frames at most).  A row that is not
// finite counts as (1, 0, 0, 0).
__device__ __forceinline__ void pose_scan(const double *__restrict__ motion, int n, double *path) {
    double lam = 0.0, th = 0.0, cx = 0.0, cy = 0.0;
    path[0] = 0.0, path[1] = 0.0, path[2] = 0.0, path[3] = 0.0;
    for (int k = 1; k < n; ++k) {
        const double *m = motion + (size_t)k * 4;
        const bool ok = finite4(m);
        const double a = ok ? m[0] : 1.0, b = ok ? m[1] : 0.0, tx = ok ? m[2] : 0.0, ty = ok ? m[3] : 0.0;
        const double s = exp(lam), c = cos(th), sn = sin(th);
        cx = cx + s * (c * tx - sn * ty);
        cy = cy + s * (sn * tx + c * ty);
        lam = lam + log(hypot(a, b));
        th = th + atan2(b, a);
        double *p = path + (size_t)k * 4;
        p[0] = lam, p[1] = th, p[2] = cx, p[3] = cy;
    }
}

// D (row-major 2 x 3) of one frame: p = its measured pose, (dlam, dth, ux, uy) = P^ - P
__device__ __forceinline__ void pose_correction(const double *p, double dlam, double dth, double ux, double uy, double *o) {
    const double lam = p[0], th = p[1];
    const double s = exp(dlam), e = exp(-lam), c = cos(th), sn = sin(th);
    o[0] = s * cos(dth), o[1] = 0.0 - s * sin(dth), o[2] = e * (c * ux + sn * uy);
    o[3] = s * sin(dth), o[4] = s * cos(dth), o[5] = e * (c * uy - sn * ux);
}

}  // namespace pws
