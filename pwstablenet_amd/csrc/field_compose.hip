// Field composition (functional.compose_fields): a per-frame affine correction D of the OUTPUT frame folded into the warp field, so that the
// fused warps (grid_sample.hip, warp_bicubic.hip) produce the corrected frame in their single resampling pass.  Path smoothing
// (path_smooth.hip) is its user: D moves a frame from the measured camera path onto the smooth one.  No counterpart in the reference.
//
// Definition (restated in tests/path_ref.py; include/pwstable.h pws_field_compose has it in full).  d[t] = D row-major 2 x 3, fp64, in
// frame pixels relative to the frame centre.  Node (i, j) of out[t] stands for frame pixel x = j (w0-1)/(fw-1), y alike (the warps resize the
// field with align_corners=True); (x', y') = D (x - cx, y - cy) + (cx, cy) is where the uncorrected output shows what the corrected one shows
// there, in fp64; on the field's lattice that is sx = x' (fw-1)/(w0-1), sy alike, each rounded ONCE to fp32.  The node takes the field there,
// with the warps' own field_lerp on the cell x0 = clamp(floor(sx), 0, fw-2), lx = sx - x0 NOT clamped: outside the lattice the field is
// continued linearly, so an affine field composes exactly and the correction's wedges reach the warp as out-of-range coordinates.
// A frame whose D is exactly the identity is copied; a node whose sx or sy is not finite keeps F[i, j].
//
// Launch shape: field_lattice.h's, 4 rows per workgroup, with its exact workgroup sum for the count.  Under a rotation the cell differs per
// lane in both axes: per node two 16-byte loads, columns x0 and x0 + 1 of rows y0 and y0 + 1.  The fp64 work is the 2 x 3 product and two
// scalings per node.
//
// Rolling shutter (pws_field_compose_rows, functional.compose_fields(rates=, rolling_shutter=)): the same kernel, instantiated with a
// row-dependent step between D and the lattice -- the camera's velocity field times the time offset of the row that D q lies on, taken out
// of D q: a dozen fp64 FMAs per node more, no transcendental, the same loads and stores.  r = 0 launches the affine instantiation.
#include "compose_node.h"

namespace pws {
namespace {

constexpr int FC_ROWS = 4;   // rows (waves) per workgroup

typedef ComposeGeo Geo;
typedef ComposeRows Rows;

// The node itself -- position, rounding, cell, interpolation, the ROWS step -- is compose_node.h's compose_node, shared with field_reach.hip.
template <bool ROWS>
__global__ void __launch_bounds__(kWave *FC_ROWS) field_compose_kernel(const float *__restrict__ field, const double *__restrict__ d,
                                                                        float *__restrict__ out, int fh, int fw, unsigned nrg, Geo geo, int h0,
                                                                        int w0, int align_corners, float m, int *__restrict__ uncovered, Rows rows) {
    __shared__ int cnt[FC_ROWS];
    const LatticePos p = lattice_pos<FC_ROWS>(nrg);
    const unsigned t = p.t;
    const int i = p.i, j0 = p.j0;
    int unc = 0;
    if (i < fh && j0 < fw) {
        const double *dt = d + (size_t)t * 6;
        double v[2][4] = {};
        const bool still = compose_still<ROWS>(ROWS ? rows.rates + (size_t)t * 8 : nullptr, v);
        const bool same = compose_identity(dt) && still;   // (uniform over the workgroup)
        const double y = (double)i * geo.ky - geo.cy;
        const float *ft = field + (size_t)t * fh * fw * 2;
        const bool ac = align_corners != 0;
        const float xhi = (float)(w0 - 1) - m, yhi = (float)(h0 - 1) - m;
        float g[kLaneNodes][2];
#pragma unroll
        for (int q = 0; q < kLaneNodes; ++q) {
            const int j = min(j0 + q, fw - 1);   // (a row of odd width: the last lane's second node repeats its first, and is dropped)
            compose_node<ROWS>(ft, fh, fw, i, j, y, dt, same, geo, rows, v, g[q][0], g[q][1]);
            if (uncovered && j0 + q < fw) unc += node_covered(g[q][0], g[q][1], h0, w0, ac, m, xhi, yhi) ? 0 : 1;
        }
        store_pair(out + (((size_t)t * fh + i) * fw + j0) * 2, j0 + 1 < fw, F32x4a8{g[0][0], g[0][1], g[1][0], g[1][1]});
    }
    if (uncovered) block_sum<FC_ROWS>(p, unc, cnt, uncovered);   // (kernel argument: uniform, every thread of the workgroup arrives)
}

// the checks, the clear and the launch of both exports; `rows` NULL: the affine kernel
int compose(const char *who, const float *field, int n, int fh, int fw, const double *d, float *out, int h0, int w0, int align_corners, int margin,
            int *uncovered, pws_stream_t stream, const Rows *rows) {
    if (int rc = lattice_shape(who, n, fh, fw)) return rc;
    PWS_REQUIRE(h0 >= 2 && w0 >= 2, "%s: the frame must be at least 2 x 2 pixels (got %d x %d)", who, w0, h0);
    PWS_REQUIRE(!uncovered || margin >= 0, "%s: bad margin %d for the uncovered count", who, margin);
    if (n == 0) return PWS_OK;
    if (int rc = lattice_pointers(who, field && d && out, addr(field) | addr(out) | addr(d), addr(uncovered),
                                  "field, out and d must be 8-byte aligned, uncovered 4-byte aligned"))
        return rc;
    if (int rc = lattice_overlap(who, field, out, n, fh, fw, false)) return rc;
    unsigned nrg, chunks;
    if (int rc = lattice_grid(who, fh, fw, FC_ROWS, (size_t)n, 1, "batch", nrg, chunks)) return rc;
    if (int rc = lattice_clear(who, "uncovered", (size_t)n * sizeof(int), as_stream(stream), uncovered)) return rc;
    const Geo geo = compose_geo(fh, fw, h0, w0);
    const dim3 grid((unsigned)n * nrg, chunks, 1), block(kWave * FC_ROWS);
    if (rows) {
        hipLaunchKernelGGL(field_compose_kernel<true>, grid, block, 0, as_stream(stream), field, d, out, fh, fw, nrg, geo, h0, w0, align_corners,
                           (float)margin, uncovered, *rows);
        return check_launch("field_compose_kernel<rows>");
    }
    hipLaunchKernelGGL(field_compose_kernel<false>, grid, block, 0, as_stream(stream), field, d, out, fh, fw, nrg, geo, h0, w0, align_corners,
                       (float)margin, uncovered, Rows{nullptr, 0.0, 0.0});
    return check_launch("field_compose_kernel");
}

}  // namespace
}  // namespace pws

using namespace pws;

extern "C" int pws_field_compose(const float *field, int n, int fh, int fw, const double *d, float *out, int h0, int w0, int align_corners, int margin,
                                 int *uncovered, pws_stream_t stream) {
    return compose("pws_field_compose", field, n, fh, fw, d, out, h0, w0, align_corners, margin, uncovered, stream, nullptr);
}

extern "C" int pws_field_compose_rows(const float *field, int n, int fh, int fw, const double *d, const double *rates, double r, float *out, int h0,
                                      int w0, int align_corners, int margin, int *uncovered, pws_stream_t stream) {
    PWS_REQUIRE(r >= -1.0 && r <= 1.0, "pws_field_compose_rows: r must lie in [-1, 1], got %g", r);   // (false for NaN)
    PWS_REQUIRE(n <= 0 || (rates && (reinterpret_cast<size_t>(rates) & 7) == 0), "pws_field_compose_rows: rates must be non-NULL and 8-byte aligned");
    const Rows rows{rates, r, h0 >= 2 ? 1.0 / (double)(h0 - 1) : 0.0};
    return compose("pws_field_compose_rows", field, n, fh, fw, d, out, h0, w0, align_corners, margin, uncovered, stream, r == 0.0 ? nullptr : &rows);
}
