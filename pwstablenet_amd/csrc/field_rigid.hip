// Rigid warp mode: each frame's warp field pulled towards the homography fitted to it (pws_field_homography's M), so that the fused warps
// (grid_sample.hip, warp_bicubic.hip), which resize the field to the frame before they sample, warp the frame rigidly.  No counterpart in
// the reference.
//
// Definition (restated in tests/rigid_ref.py).  M[t] maps a field VALUE (normalised source coordinates) to the output position u = 2x/w0 - 1,
// v = 2y/h0 - 1 (the reference's convention: no half-pixel term).  Node (i, j) stands for frame pixel x = j (w0-1)/(fw-1), y = i (h0-1)/(fh-1)
// (where the warps' align_corners=True resize reads exactly that node).  A = adj(M) (M^-1 up to scale), (X, Y, D) = A (u, v, 1), Dc = A[2][2],
// P = (X/D, Y/D), all in fp64, P rounded once to fp32.  A frame is FITTED when M's nine entries and det M are finite, det M != 0 and Dc != 0;
// a node of a fitted frame is VALID when D/Dc >= 2^-20 (the frame centre's side of the horizon, and not on it).  A valid node gets P itself
// when r == 1, F itself when r == 0 and fmaf(r, P - F, F) otherwise; any other node keeps F bit for bit and is
// counted in unfit[t].  residual[t] = the largest
// max(|Fx - Px| w0/2, |Fy - Py| h0/2) (fp32: one subtraction, one product) over the valid nodes whose F is finite, 0 without any.
//
// Launch shape: field_lattice.h's, 4 rows per workgroup.  The kernel is element-wise -- a lane reads its two nodes, then writes them -- so
// out may be field itself (neither pointer is __restrict__).  M, the adjugate, the fitted test and the row's v terms depend on blockIdx and the
// wave's index alone: M arrives through scalar loads and the fp64 arithmetic on it is uniform VALU work (gfx950 has no scalar fp64 unit), about
// 30 instructions per wave next to the two nodes' 2 x (3 FMAs, three divisions).  X, Y and D are sums of products that the compiler contracts
// into FMAs, so against another float64 evaluation of the same formulas P agrees to one float32 ulp (a rounding tie can fall the other way),
// and the horizon test within a relative 2^-52 of the threshold.  Measured on an MI355X (profiles/rigid_bench.json): 32 x 256 x 256 nodes take
// 8.6 us, 2.0 x a device copy of their 32 MB; 37 us with both statistics, whose 4096 atomics on 32 words dominate then.  The statistics are
// field_lattice.h's exact workgroup sum and max.
//
// hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage: 40 VGPRs, 52 SGPRs, 0 bytes of scratch, 32 bytes of LDS,
// 8 waves per SIMD.
#include "field_lattice.h"
#include "rigid_position.h"

namespace pws {
namespace {

constexpr int FG_ROWS = 4;   // rows (waves) per workgroup

__global__ void __launch_bounds__(kWave *FG_ROWS) field_rigid_kernel(const float *field, const double *__restrict__ m, float *out, int fh, int fw,
                                                                      unsigned nrg, float r, double su, double sv, float half_w, float half_h,
                                                                      int *__restrict__ residual_bits, int *__restrict__ unfit) {
    __shared__ int cnt[FG_ROWS];
    __shared__ float big[FG_ROWS];
    const LatticePos p = lattice_pos<FG_ROWS>(nrg);
    const unsigned t = p.t;
    const int i = p.i, j0 = p.j0;
    int kept = 0;
    float res = 0.f;
    if (i < fh && j0 < fw) {
        // ---- wave-uniform: the adjugate, the fitted test, the row's terms
        const RigidFrame frame = rigid_frame(m + (size_t)t * 9);   // (rigid_position.h: shared with field_wobble.hip)
        const RigidRow row = rigid_row(frame, (double)i * sv - 1.0);
        // ---- the lane's two nodes
        const bool two = j0 + 1 < fw;   // (a row of odd width: its last lane holds one node)
        const float *f = field + (((size_t)t * fh + i) * fw + j0) * 2;
        const F32x4a8 F = load_pair(f, two);
        float g[kLaneNodes][2];
#pragma unroll
        for (int q = 0; q < kLaneNodes; ++q) {
            const float fx = q ? F.z : F.x, fy = q ? F.w : F.y;
            float px, py;
            const bool valid = rigid_node(frame, row, (double)(j0 + q) * su - 1.0, px, py);
            const bool live = q == 0 || two;
            if (valid) {
                if (r == 1.f) {   // (kernel argument: uniform.  Full rigidity is the homography itself, not F + (P - F))
                    g[q][0] = px, g[q][1] = py;
                } else if (r == 0.f) {   // (uniform.  No rigidity is the field itself, whatever P is: 0 * inf would be NaN)
                    g[q][0] = fx, g[q][1] = fy;
                } else {
                    g[q][0] = __builtin_fmaf(r, px - fx, fx), g[q][1] = __builtin_fmaf(r, py - fy, fy);
                }
                if (live && __builtin_isfinite(fx) && __builtin_isfinite(fy))
                    res = fmaxf(res, fmaxf(fabsf(fx - px) * half_w, fabsf(fy - py) * half_h));   // (fmaxf drops a NaN)
            } else {
                g[q][0] = fx, g[q][1] = fy;
                kept += live ? 1 : 0;
            }
        }
        store_pair(out + (((size_t)t * fh + i) * fw + j0) * 2, two, F32x4a8{g[0][0], g[0][1], g[1][0], g[1][1]});
    }
    // (kernel arguments: uniform, every thread of the workgroup arrives)
    if (residual_bits || unfit) block_sum_max<FG_ROWS>(p, kept, res, cnt, big, unfit, residual_bits);
}

}  // namespace
}  // namespace pws

using namespace pws;

extern "C" int pws_field_rigid(const float *field, int n, int fh, int fw, const double *m, float rigidity, int h0, int w0, float *out,
                               float *residual, int *unfit, pws_stream_t stream) {
    const char *who = "pws_field_rigid";
    if (int rc = lattice_shape(who, n, fh, fw)) return rc;
    PWS_REQUIRE(h0 >= 1 && w0 >= 1, "pws_field_rigid: bad frame size %d x %d", w0, h0);
    PWS_REQUIRE(rigidity >= 0.f && rigidity <= 1.f, "pws_field_rigid: rigidity must lie in [0, 1], got %g", (double)rigidity);   // (false for NaN)
    if (n == 0) return PWS_OK;
    if (int rc = lattice_pointers(who, field && m && out, addr(field) | addr(out) | addr(m), addr(residual) | addr(unfit),
                                  "field, out and m must be 8-byte aligned, residual and unfit 4-byte aligned"))
        return rc;
    if (int rc = lattice_overlap(who, field, out, n, fh, fw, true)) return rc;
    unsigned nrg, chunks;
    if (int rc = lattice_grid(who, fh, fw, FG_ROWS, (size_t)n, 1, "batch", nrg, chunks)) return rc;
    if (int rc = lattice_clear(who, "the statistics", (size_t)n * 4, as_stream(stream), residual, unfit)) return rc;
    double su, sv;
    node_scale(fh, fw, h0, w0, &su, &sv);
    hipLaunchKernelGGL(field_rigid_kernel, dim3((unsigned)n * nrg, chunks, 1), dim3(kWave * FG_ROWS), 0, as_stream(stream), field, m, out, fh, fw,
                       nrg, rigidity, su, sv, 0.5f * (float)w0, 0.5f * (float)h0, reinterpret_cast<int *>(residual), unfit);
    return check_launch("field_rigid_kernel");
}
