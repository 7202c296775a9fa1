// One node of the field composition (include/pwstable.h pws_field_compose / pws_field_compose_rows have the definition): the fp64 position
// under D, the row-dependent rolling-shutter step, the single rounding to fp32, the cell bounded as a float, the unclamped lx / ly, the
// warps' field_lerp and the rule for positions that are not finite.  field_compose.hip stores the value; field_reach.hip only classifies
// it.  Both include this one function, so that what is counted is what would be written, bit for bit.
#pragma once
#include "field_lattice.h"

namespace pws {

struct ComposeGeo {   // host-computed, fp64: the node's frame pixel, the frame centre, the lattice coordinate of a frame pixel
    double kx, ky, cx, cy, ikx, iky;
};

struct ComposeRows {   // ROWS: the frames' rates (n, 2, 4), the readout share r (never 0 here) and 1 / (h0 - 1)
    const double *rates;
    double r, ih;
};

static ComposeGeo compose_geo(int fh, int fw, int h0, int w0) {
    ComposeGeo geo;
    geo.kx = (double)(w0 - 1) / (double)(fw - 1), geo.ky = (double)(h0 - 1) / (double)(fh - 1);
    geo.cx = 0.5 * (double)(w0 - 1), geo.cy = 0.5 * (double)(h0 - 1);
    geo.ikx = (double)(fw - 1) / (double)(w0 - 1), geo.iky = (double)(fh - 1) / (double)(h0 - 1);
    return geo;
}

// A frame is copied when its D is exactly the identity and, ROWS, its camera stands still (both workgroup-uniform).
__device__ __forceinline__ bool compose_identity(const double *dt) {
    return dt[0] == 1.0 && dt[1] == 0.0 && dt[2] == 0.0 && dt[3] == 0.0 && dt[4] == 1.0 && dt[5] == 0.0;
}

// ROWS: the frame's eight rates into v, and whether all of them are zero (nothing to take out); otherwise true, v untouched
template <bool ROWS>
__device__ __forceinline__ bool compose_still(const double *rates_t, double (&v)[2][4]) {
    bool still = true;
    if constexpr (ROWS) {
#pragma unroll
        for (int c = 0; c < 8; ++c) v[c >> 2][c & 3] = rates_t[c], still = still && v[c >> 2][c & 3] == 0.0;
    }
    return still;
}

// The value of node (i, j) of frame `ft` under D = dt (six fp64 coefficients); y = (double)i * geo.ky - geo.cy, the row's frame pixel.
// ROWS (pws_field_compose_rows): the rolling-shutter correction between D and the lattice.  p0 = D q lies on a row exposed delta = r
// clamp(p0.y / (h0-1), -1/2, 1/2) of a frame interval away from the centre row's instant; the camera's velocity field there -- the frame's
// forward rates for delta >= 0, its backward rates otherwise -- times delta is taken out of p0, in fp64.
template <bool ROWS>
__device__ __forceinline__ void compose_node(const float *ft, int fh, int fw, int i, int j, double y, const double *dt, bool same,
                                             const ComposeGeo &geo, const ComposeRows &rows, const double (&v)[2][4], float &gx, float &gy) {
    const double d0 = dt[0], d1 = dt[1], d2 = dt[2], d3 = dt[3], d4 = dt[4], d5 = dt[5];
    const double x = (double)j * geo.kx - geo.cx;
    float sx, sy;
    if constexpr (ROWS) {
        const double px = d0 * x + d1 * y + d2, py = d3 * x + d4 * y + d5;   // p0 = D q: the affine kernel's, and its bits at zero rates
        const double delta = rows.r * fmin(fmax(py * rows.ih, -0.5), 0.5);
        const bool fwd = delta >= 0.0;
        const double ld = fwd ? v[0][0] : v[1][0], wd = fwd ? v[0][1] : v[1][1], xd = fwd ? v[0][2] : v[1][2], yd = fwd ? v[0][3] : v[1][3];
        const double vx = (ld * px - wd * py) + xd, vy = (ld * py + wd * px) + yd;
        sx = (float)(((px - delta * vx) + geo.cx) * geo.ikx), sy = (float)(((py - delta * vy) + geo.cy) * geo.iky);
    } else {
        sx = (float)(((d0 * x + d1 * y + d2) + geo.cx) * geo.ikx), sy = (float)(((d3 * x + d4 * y + d5) + geo.cy) * geo.iky);
    }
    const bool keep = same || !(isfinite(sx) && isfinite(sy));   // the node keeps F[i, j]: its own cell, picked below
    // the cell, bounded as a FLOAT before it becomes an integer: in [0, fw-2] x [0, fh-2] whatever d holds
    const float fx = keep ? (float)min(j, fw - 2) : fminf(fmaxf(floorf(sx), 0.f), (float)(fw - 2));
    const float fy = keep ? (float)min(i, fh - 2) : fminf(fmaxf(floorf(sy), 0.f), (float)(fh - 2));
    const int x0 = (int)fx, y0 = (int)fy;
    const float *f0 = ft + ((size_t)y0 * fw + x0) * 2;
    const F32x4a8 r0 = *reinterpret_cast<const F32x4a8 *>(f0), r1 = *reinterpret_cast<const F32x4a8 *>(f0 + (size_t)fw * 2);
    if (keep) {
        const F32x4a8 r = i == y0 ? r0 : r1;
        gx = j == x0 ? r.x : r.z, gy = j == x0 ? r.y : r.w;
    } else {
        const float lx = sx - fx, hx = 1.f - lx, ly = sy - fy, hy = 1.f - ly;   // (not clamped: linear continuation outside the lattice)
        gx = field_lerp(hy, ly, hx, lx, r0.x, r0.z, r1.x, r1.z);
        gy = field_lerp(hy, ly, hx, lx, r0.y, r0.w, r1.y, r1.w);
    }
}

}  // namespace pws
