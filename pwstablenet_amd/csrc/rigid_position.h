// The rigid position P of a field node under a frame's fitted homography, and the notions FITTED (frame) and VALID (node): the one device
// restatement of pws_field_rigid's definition (include/pwstable.h), shared by field_rigid.hip and field_wobble.hip so that both evaluate the
// same expressions and give the same bits.
//
// M (nine fp64, row-major, as pws_field_homography writes it) maps a field VALUE to the output position u = 2x/w0 - 1, v = 2y/h0 - 1.
// A = adj(M), (X, Y, D) = A (u, v, 1), Dc = A[2][2], P = (X/D, Y/D) in fp64, each rounded once to fp32.  Everything that depends on the
// frame (rigid_frame) and on the row (rigid_row) is wave-uniform where a wave owns one row of one frame: M arrives through scalar loads and
// the fp64 arithmetic on it is uniform VALU work (gfx950 has no scalar fp64 unit).  X, Y and D are sums of products that the compiler
// contracts into FMAs.
#pragma once
#include "common.h"

namespace pws {

struct RigidFrame {
    double a00, a01, a02, a10, a11, a12, a20, a21, a22;   // adj(M)
    bool fitted;   // M's nine entries and det M finite, det M != 0, Dc = a22 != 0
};
struct RigidRow {
    double xr, yr, dr;   // the row's share of X, Y, D: A[.][1] v + A[.][2]
};

__device__ __forceinline__ RigidFrame rigid_frame(const double *__restrict__ M) {
    const double m0 = M[0], m1 = M[1], m2 = M[2], m3 = M[3], m4 = M[4], m5 = M[5], m6 = M[6], m7 = M[7], m8 = M[8];
    RigidFrame f;
    f.a00 = m4 * m8 - m5 * m7, f.a01 = m2 * m7 - m1 * m8, f.a02 = m1 * m5 - m2 * m4;
    f.a10 = m5 * m6 - m3 * m8, f.a11 = m0 * m8 - m2 * m6, f.a12 = m2 * m3 - m0 * m5;
    f.a20 = m3 * m7 - m4 * m6, f.a21 = m1 * m6 - m0 * m7, f.a22 = m0 * m4 - m1 * m3;
    const double det = m0 * f.a00 + m1 * f.a10 + m2 * f.a20;
    bool fitted = __builtin_isfinite(det) && det != 0.0 && f.a22 != 0.0;
    fitted = fitted && __builtin_isfinite(m0) && __builtin_isfinite(m1) && __builtin_isfinite(m2) && __builtin_isfinite(m3) &&
             __builtin_isfinite(m4) && __builtin_isfinite(m5) && __builtin_isfinite(m6) && __builtin_isfinite(m7) && __builtin_isfinite(m8);
    f.fitted = fitted;
    return f;
}

// The node-to-frame scale (host): node j stands for u = 2 (j (w0-1)/(fw-1)) / w0 - 1 = j su - 1; rows alike with sv
inline void node_scale(int fh, int fw, int h0, int w0, double *su, double *sv) {
    *su = 2.0 * (double)(w0 - 1) / ((double)(fw - 1) * (double)w0), *sv = 2.0 * (double)(h0 - 1) / ((double)(fh - 1) * (double)h0);
}

// v = i sv - 1 of the node's row
__device__ __forceinline__ RigidRow rigid_row(const RigidFrame &f, double v) {
    return RigidRow{f.a01 * v + f.a02, f.a11 * v + f.a12, f.a21 * v + f.a22};
}

// u = j su - 1 of the node's column.  Returns whether the node is VALID (false for NaN); P is computed either way (true fp64 divisions: the
// definition's quotients, rounded once).
__device__ __forceinline__ bool rigid_node(const RigidFrame &f, const RigidRow &r, double u, float &px, float &py) {
    const double X = f.a00 * u + r.xr, Y = f.a10 * u + r.yr, D = f.a20 * u + r.dr;
    px = (float)(X / D), py = (float)(Y / D);
    return f.fitted && D / f.a22 >= 0x1p-20;
}

}  // namespace pws
