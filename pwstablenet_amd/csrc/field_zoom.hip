// Zoom to fill: the warp field resampled over a per-frame window, so that the fused warps (grid_sample.hip, warp_bicubic.hip), which resize
// the field to the frame before they sample, produce the zoomed frame in their single resampling pass.  No counterpart in the reference.
//
// Definition (restated in tests/zoom_ref.py).  coef[t] = Ax, Bx, Ay, By.  Node (i, j) of out[t] takes the field of frame t at
// sx = clamp(fma(Bx, j, Ax), 0, fw-1), sy = clamp(fma(By, i, Ay), 0, fh-1), interpolated with the warps' own field_lerp (warp_common.h) on the
// corners x0 = floor(sx), x1 = x0 + (x0 < fw-1), rows alike.  The field's VALUES are kept, only its domain changes: an output pixel samples
// the source where the pixel it stands for in the unzoomed warped frame would have.  With (0, 1, 0, 1) sx = j, lx = 0 and the blend returns
// F[i, j] itself.  `uncovered[t]` counts the nodes of out[t] whose un-normalised source position lies outside [m, w0-1-m] x [m, h0-1-m]
// (border_keep.hip's rule at the field's nodes; NaN is outside).
//
// Launch shape: field_lattice.h's, 4 rows per workgroup.  The row's sy, y0, ly are wave-uniform.  Per node and field row a lane loads the 16
// bytes of columns min(x0, fw-2) and the next one -- both corners at once; at the last column (lx = 0) both corners are the second half.
// The count is field_lattice.h's exact workgroup sum.
#include "field_lattice.h"

namespace pws {
namespace {

constexpr int FZ_ROWS = 4;   // rows (waves) per workgroup

__device__ __forceinline__ float clamp_pos(float v, float hi) { return fminf(fmaxf(v, 0.f), hi); }   // (NaN -> 0)

__global__ void __launch_bounds__(kWave *FZ_ROWS) field_zoom_kernel(const float *__restrict__ field, const float *__restrict__ coef,
                                                                     float *__restrict__ out, int fh, int fw, unsigned nrg, int h0, int w0,
                                                                     int align_corners, float m, int *__restrict__ uncovered) {
    __shared__ int cnt[FZ_ROWS];
    const LatticePos p = lattice_pos<FZ_ROWS>(nrg);
    const unsigned t = p.t;
    const int i = p.i, j0 = p.j0;
    int unc = 0;
    if (i < fh && j0 < fw) {
        const float ax = coef[(size_t)t * 4], bx = coef[(size_t)t * 4 + 1], ay = coef[(size_t)t * 4 + 2], by = coef[(size_t)t * 4 + 3];
        const float sy = clamp_pos(fmaf(by, (float)i, ay), (float)(fh - 1));
        const int y0 = min(max((int)sy, 0), fh - 1), y1 = y0 + (y0 < fh - 1 ? 1 : 0);   // (the integer clamp: in bounds whatever coef holds)
        const float ly = sy - (float)y0, hy = 1.f - ly;
        const float *f0 = field + ((size_t)t * fh + y0) * fw * 2, *f1 = field + ((size_t)t * fh + y1) * fw * 2;
        const bool ac = align_corners != 0;
        const float xhi = (float)(w0 - 1) - m, yhi = (float)(h0 - 1) - m;
        float g[kLaneNodes][2];
#pragma unroll
        for (int q = 0; q < kLaneNodes; ++q) {
            const int j = min(j0 + q, fw - 1);   // (a row of odd width: the last lane's second node repeats its first, and is dropped)
            const float sx = clamp_pos(fmaf(bx, (float)j, ax), (float)(fw - 1));
            const int x0 = min(max((int)sx, 0), fw - 1), xb = min(x0, fw - 2);
            const float lx = sx - (float)x0, hx = 1.f - lx;
            const F32x4a8 r0 = *reinterpret_cast<const F32x4a8 *>(f0 + (size_t)xb * 2), r1 = *reinterpret_cast<const F32x4a8 *>(f1 + (size_t)xb * 2);
            const bool last = x0 > xb;   // x0 = x1 = fw-1
            const float a0 = last ? r0.z : r0.x, a1 = last ? r0.w : r0.y, c0 = last ? r1.z : r1.x, c1 = last ? r1.w : r1.y;
            g[q][0] = field_lerp(hy, ly, hx, lx, a0, r0.z, c0, r1.z);
            g[q][1] = field_lerp(hy, ly, hx, lx, a1, r0.w, c1, r1.w);
            if (uncovered && j0 + q < fw) unc += node_covered(g[q][0], g[q][1], h0, w0, ac, m, xhi, yhi) ? 0 : 1;
        }
        store_pair(out + (((size_t)t * fh + i) * fw + j0) * 2, j0 + 1 < fw, F32x4a8{g[0][0], g[0][1], g[1][0], g[1][1]});
    }
    if (uncovered) block_sum<FZ_ROWS>(p, unc, cnt, uncovered);   // (kernel argument: uniform, every thread of the workgroup arrives)
}

}  // namespace
}  // namespace pws

using namespace pws;

extern "C" int pws_field_zoom(const float *field, int n, int fh, int fw, const float *coef, float *out, int h0, int w0, int align_corners, int margin,
                              int *uncovered, pws_stream_t stream) {
    const char *who = "pws_field_zoom";
    if (int rc = lattice_shape(who, n, fh, fw)) return rc;
    PWS_REQUIRE(!uncovered || (h0 >= 1 && w0 >= 1 && margin >= 0), "pws_field_zoom: bad frame size %d x %d or margin %d for the uncovered count", w0,
                h0, margin);
    if (n == 0) return PWS_OK;
    if (int rc = lattice_pointers(who, field && coef && out, addr(field) | addr(out), addr(coef) | addr(uncovered),
                                  "field and out must be 8-byte aligned, coef and uncovered 4-byte aligned"))
        return rc;
    if (int rc = lattice_overlap(who, field, out, n, fh, fw, false)) return rc;
    unsigned nrg, chunks;
    if (int rc = lattice_grid(who, fh, fw, FZ_ROWS, (size_t)n, 1, "batch", nrg, chunks)) return rc;
    if (int rc = lattice_clear(who, "uncovered", (size_t)n * sizeof(int), as_stream(stream), uncovered)) return rc;
    hipLaunchKernelGGL(field_zoom_kernel, dim3((unsigned)n * nrg, chunks, 1), dim3(kWave * FZ_ROWS), 0, as_stream(stream), field, coef, out, fh, fw,
                       nrg, h0, w0, align_corners, (float)margin, uncovered);
    return check_launch("field_zoom_kernel");
}
