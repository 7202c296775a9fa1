// Field reach (stream.limit_path; C: pws_field_reach): how many nodes of a rectangle of the lattice would sample outside the source if a
// frame's field were composed with each of levels + 1 candidate corrections -- pws_field_compose's value at the node, classified by
// field_lattice.h's coverage rule (pws_field_zoom's), and never stored.  Crop-bounded smoothing reads the counts to choose, per frame, the
// largest share of the smoothing correction that keeps a window of the output covered.  No counterpart in the reference.
//
// Definition (restated in tests/limit_ref.py; include/pwstable.h pws_field_reach has it in full).  table[t, l] = D of frame t at level l,
// row-major 2 x 3, fp64; counts[t, l] = the number of nodes (i, j), i0 <= i <= i1, j0 <= j <= j1, whose composed value under table[t, l]
// is not covered.  The node is compose_node.h's function, the one field_compose.hip stores: the same bits are classified.
//
// Launch shape: field_lattice.h's over the rectangle, 4 rows per workgroup.  Each lane keeps its two nodes and walks the levels; the
// frame's table (at most 65 x 6 fp64) is in LDS and every read of it is a broadcast.  The field is read with the composition's two 16-byte
// loads per node and level: the frame's 512 KB stay in L2 across the levels, and nothing is written but the counts.  Per level a wave
// counts with two ballots; lane 0 puts the sum into the wave's LDS slot, and after the loop one thread per level adds the workgroup's four
// slots to counts with one integer atomic: integer sums, the same on every run.
#include "compose_node.h"

namespace pws {
namespace {

constexpr int FR_ROWS = 4, FR_LMAX = 64;   // rows (waves) per workgroup, the most levels

template <bool ROWS>
__global__ void __launch_bounds__(kWave *FR_ROWS) field_reach_kernel(const float *__restrict__ field, const double *__restrict__ table,
                                                                      int *__restrict__ counts, int fh, int fw, int levels, int i0, int i1, int j0,
                                                                      int j1, unsigned nrg, ComposeGeo geo, int h0, int w0, int align_corners, float m,
                                                                      ComposeRows rows) {
    __shared__ double tab[(FR_LMAX + 1) * 6];
    __shared__ int cnt[FR_ROWS][FR_LMAX + 1];
    const LatticePos p = lattice_pos<FR_ROWS>(nrg, i0, j0);
    const unsigned t = p.t;
    const int tid = (int)threadIdx.x, nl = levels + 1, wave = p.wave, lane = p.lane, i = p.i, jb = p.j0;
    for (int k = tid; k < nl * 6; k += kWave * FR_ROWS) tab[k] = table[(size_t)t * nl * 6 + k];
    for (int k = tid; k < FR_ROWS * (FR_LMAX + 1); k += kWave * FR_ROWS) (&cnt[0][0])[k] = 0;
    __syncthreads();
    if (i <= i1) {   // (uniform over the wave; its first lane always owns a node: the grid has no chunk beyond j1)
        double v[2][4] = {};
        const bool still = compose_still<ROWS>(ROWS ? rows.rates + (size_t)t * 8 : nullptr, v);
        const double y = (double)i * geo.ky - geo.cy;
        const float *ft = field + (size_t)t * fh * fw * 2;
        const bool ac = align_corners != 0;
        const float xhi = (float)(w0 - 1) - m, yhi = (float)(h0 - 1) - m;
        const bool own[kLaneNodes] = {jb <= j1, jb + 1 <= j1};
        const int jq[kLaneNodes] = {min(jb, j1), min(jb + 1, j1)};   // (a node beyond the rectangle repeats its last one, and is dropped)
        for (int l = 0; l < nl; ++l) {
            const double *dt = tab + l * 6;
            const bool same = compose_identity(dt) && still;
            int c = 0;
#pragma unroll
            for (int q = 0; q < kLaneNodes; ++q) {
                float gx, gy;
                compose_node<ROWS>(ft, fh, fw, i, jq[q], y, dt, same, geo, rows, v, gx, gy);
                const bool unc = own[q] && !node_covered(gx, gy, h0, w0, ac, m, xhi, yhi);
                c += (int)__builtin_popcountll(__ballot(unc));
            }
            if (lane == 0) cnt[wave][l] = c;
        }
    }
    __syncthreads();
    if (tid < nl) {
        int tot = 0;
#pragma unroll
        for (int w = 0; w < FR_ROWS; ++w) tot += cnt[w][tid];
        if (tot != 0) atomicAdd(counts + (size_t)t * nl + tid, tot);
    }
}

}  // namespace
}  // namespace pws

using namespace pws;

extern "C" int pws_field_reach(const float *field, int n, int fh, int fw, const double *table, int levels, const double *rates, double r, int i0,
                               int i1, int j0, int j1, int h0, int w0, int align_corners, int margin, int *counts, pws_stream_t stream) {
    const char *who = "pws_field_reach";
    if (int rc = lattice_shape(who, n, fh, fw)) return rc;
    PWS_REQUIRE(h0 >= 2 && w0 >= 2, "%s: the frame must be at least 2 x 2 pixels (got %d x %d)", who, w0, h0);
    PWS_REQUIRE(margin >= 0, "%s: bad margin %d", who, margin);
    PWS_REQUIRE(levels >= 0 && levels <= FR_LMAX, "%s: levels must lie in 0 .. %d, got %d", who, FR_LMAX, levels);
    PWS_REQUIRE(r >= -1.0 && r <= 1.0, "%s: r must lie in [-1, 1], got %g", who, r);   // (false for NaN)
    PWS_REQUIRE(0 <= i0 && i0 <= i1 && i1 <= fh - 1 && 0 <= j0 && j0 <= j1 && j1 <= fw - 1,
                "%s: the rectangle rows %d .. %d, columns %d .. %d is empty or leaves the %d x %d lattice", who, i0, i1, j0, j1, fw, fh);
    if (n == 0) return PWS_OK;
    if (int rc = lattice_pointers(who, field && table && counts, addr(field) | addr(table) | addr(rates), addr(counts),
                                  "field, table and rates must be 8-byte aligned, counts 4-byte aligned"))
        return rc;
    unsigned nrg, chunks;
    if (int rc = lattice_grid(who, i1 - i0 + 1, j1 - j0 + 1, FR_ROWS, (size_t)n, 1, "batch", nrg, chunks)) return rc;
    if (int rc = lattice_clear(who, "counts", (size_t)n * (levels + 1) * sizeof(int), as_stream(stream), counts)) return rc;
    const ComposeGeo geo = compose_geo(fh, fw, h0, w0);
    const dim3 grid((unsigned)n * nrg, chunks, 1), block(kWave * FR_ROWS);
    if (rates && r != 0.0) {
        hipLaunchKernelGGL(field_reach_kernel<true>, grid, block, 0, as_stream(stream), field, table, counts, fh, fw, levels, i0, i1, j0, j1, nrg, geo,
                           h0, w0, align_corners, (float)margin, ComposeRows{rates, r, 1.0 / (double)(h0 - 1)});
        return check_launch("field_reach_kernel<rows>");
    }
    hipLaunchKernelGGL(field_reach_kernel<false>, grid, block, 0, as_stream(stream), field, table, counts, fh, fw, levels, i0, i1, j0, j1, nrg, geo, h0,
                       w0, align_corners, (float)margin, ComposeRows{nullptr, 0.0, 0.0});
    return check_launch("field_reach_kernel");
}
