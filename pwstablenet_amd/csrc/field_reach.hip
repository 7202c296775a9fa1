// Field reach (stream.limit_path; C: pws_field_reach): how many nodes of a rectangle of the lattice would sample outside the source if a
// frame's field were composed with each of levels + 1 candidate corrections -- pws_field_compose's value at the node, classified by
// pws_field_zoom's coverage rule, and never stored.  Crop-bounded smoothing reads the counts to choose, per frame, the largest share of
// the smoothing correction that keeps a window of the output covered.  No counterpart in the reference.
//
// Definition (restated in tests/limit_ref.py; include/pwstable.h pws_field_reach has it in full).  table[t, l] = D of frame t at level l,
// row-major 2 x 3, fp64; counts[t, l] = the number of nodes (i, j), i0 <= i <= i1, j0 <= j <= j1, whose composed value under table[t, l]
// is not covered.  The node is compose_node.h's function, the one field_compose.hip stores: the same bits are classified.
//
// Launch shape: field_compose.hip's, over the rectangle -- a wave owns 128 consecutive nodes of one row of one frame, a lane 2 adjacent
// ones, a workgroup is 4 waves = 4 rows.  Each lane keeps its two nodes and walks the levels; the frame's table (at most 65 x 6 fp64) is in
// LDS and every read of it is a broadcast.  The field is read with the composition's two 16-byte loads per node and level: the frame's
// 512 KB stay in L2 across the levels, and nothing is written but the counts.  Per level a wave counts with two ballots; lane 0 puts the
// sum into the wave's LDS slot, and after the loop one thread per level adds the workgroup's four slots to counts with one integer
// atomic: integer sums, the same on every run.
#include "compose_node.h"

namespace pws {
namespace {

constexpr int FR_PER_LANE = 2, FR_CHUNK = kWave * FR_PER_LANE, FR_ROWS = 4, FR_LMAX = 64;

template <bool ROWS>
__global__ void __launch_bounds__(kWave *FR_ROWS) field_reach_kernel(const float *__restrict__ field, const double *__restrict__ table,
                                                                      int *__restrict__ counts, int fh, int fw, int levels, int i0, int i1, int j0,
                                                                      int j1, unsigned nrg, ComposeGeo geo, int h0, int w0, int align_corners, float m,
                                                                      ComposeRows rows) {
    __shared__ double tab[(FR_LMAX + 1) * 6];
    __shared__ int cnt[FR_ROWS][FR_LMAX + 1];
    const unsigned t = blockIdx.x / nrg, rg = blockIdx.x - t * nrg;
    const int tid = (int)threadIdx.x, nl = levels + 1;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    for (int k = tid; k < nl * 6; k += kWave * FR_ROWS) tab[k] = table[(size_t)t * nl * 6 + k];
    for (int k = tid; k < FR_ROWS * (FR_LMAX + 1); k += kWave * FR_ROWS) (&cnt[0][0])[k] = 0;
    __syncthreads();
    const int i = i0 + (int)rg * FR_ROWS + wave, jb = j0 + (int)blockIdx.y * FR_CHUNK + lane * FR_PER_LANE;
    if (i <= i1) {   // (uniform over the wave; its first lane always owns a node: the grid has no chunk beyond j1)
        double v[2][4] = {};
        const bool still = compose_still<ROWS>(ROWS ? rows.rates + (size_t)t * 8 : nullptr, v);
        const double y = (double)i * geo.ky - geo.cy;
        const float *ft = field + (size_t)t * fh * fw * 2;
        const bool ac = align_corners != 0;
        const float xhi = (float)(w0 - 1) - m, yhi = (float)(h0 - 1) - m;
        const bool own[FR_PER_LANE] = {jb <= j1, jb + 1 <= j1};
        const int jq[FR_PER_LANE] = {min(jb, j1), min(jb + 1, j1)};   // (a node beyond the rectangle repeats its last one, and is dropped)
        for (int l = 0; l < nl; ++l) {
            const double *dt = tab + l * 6;
            const bool same = compose_identity(dt) && still;
            int c = 0;
#pragma unroll
            for (int q = 0; q < FR_PER_LANE; ++q) {
                float gx, gy;
                compose_node<ROWS>(ft, fh, fw, i, jq[q], y, dt, same, geo, rows, v, gx, gy);
                const bool unc = own[q] && !compose_covered(gx, gy, h0, w0, ac, m, xhi, yhi);
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
    PWS_REQUIRE(n >= 0, "%s: bad shape", who);
    PWS_REQUIRE(fh >= 2 && fw >= 2, "%s: the field needs at least 2 x 2 nodes (got %d x %d)", who, fw, fh);
    PWS_REQUIRE(h0 >= 2 && w0 >= 2, "%s: the frame must be at least 2 x 2 pixels (got %d x %d)", who, w0, h0);
    PWS_REQUIRE(margin >= 0, "%s: bad margin %d", who, margin);
    PWS_REQUIRE(levels >= 0 && levels <= FR_LMAX, "%s: levels must lie in 0 .. %d, got %d", who, FR_LMAX, levels);
    PWS_REQUIRE(r >= -1.0 && r <= 1.0, "%s: r must lie in [-1, 1], got %g", who, r);   // (false for NaN)
    PWS_REQUIRE(0 <= i0 && i0 <= i1 && i1 <= fh - 1 && 0 <= j0 && j0 <= j1 && j1 <= fw - 1,
                "%s: the rectangle rows %d .. %d, columns %d .. %d is empty or leaves the %d x %d lattice", who, i0, i1, j0, j1, fw, fh);
    if (n == 0) return PWS_OK;
    PWS_REQUIRE(field && table && counts, "%s: NULL pointer", who);
    PWS_REQUIRE(((reinterpret_cast<size_t>(field) | reinterpret_cast<size_t>(table) | reinterpret_cast<size_t>(rates)) & 7) == 0 &&
                    (reinterpret_cast<size_t>(counts) & 3) == 0,
                "%s: field, table and rates must be 8-byte aligned, counts 4-byte aligned", who);
    const unsigned nrg = (unsigned)((i1 - i0 + FR_ROWS) / FR_ROWS), chunks = (unsigned)((j1 - j0 + FR_CHUNK) / FR_CHUNK);
    PWS_REQUIRE((size_t)n * nrg < (1u << 31) && chunks < 65536, "%s: field or batch too large", who);
    const hipError_t e = hipMemsetAsync(counts, 0, (size_t)n * (levels + 1) * sizeof(int), as_stream(stream));
    if (e != hipSuccess) {
        set_error("%s: clearing counts: %s", who, hipGetErrorString(e));
        return PWS_EHIP;
    }
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
