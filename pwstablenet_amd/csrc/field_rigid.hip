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
// Launch shape (field_zoom.hip's): a wave owns 128 consecutive nodes of ONE row of one frame, a lane 2 adjacent ones (one 16-byte load, one
// 16-byte store); a workgroup is 4 waves = 4 rows.  The kernel is element-wise -- a lane reads its two nodes, then writes them -- so out may
// be field itself (neither pointer is __restrict__).  M, the adjugate, the fitted test and the row's v terms depend on blockIdx and the
// wave's index alone: M arrives through scalar loads and the fp64 arithmetic on it is uniform VALU work (gfx950 has no scalar fp64 unit), about
// 30 instructions per wave next to the two nodes' 2 x (3 FMAs, three divisions).  X, Y and D are sums of products that the compiler contracts
// into FMAs, so against another float64 evaluation of the same formulas P agrees to one float32 ulp (a rounding tie can fall the other way),
// and the horizon test within a relative 2^-52 of the threshold.  Measured on an MI355X (profiles/rigid_bench.json): 32 x 256 x 256 nodes take
// 8.6 us, 2.0 x a device copy of their 32 MB; 37 us with both statistics, whose 4096 atomics on 32 words dominate then.  The statistics are reduced per wave by shuffles and per workgroup through LDS, then one integer
// atomic each per workgroup that has anything to report: a sum of counts, and a max on the bit pattern of a non-negative float, which
// orders as the float does.  Both are exact and the same on every run.
//
// hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage: 40 VGPRs, 52 SGPRs, 0 bytes of scratch, 32 bytes of LDS,
// 8 waves per SIMD.
#include "common.h"
#include "rigid_position.h"

namespace pws {
namespace {

constexpr int FR_PER_LANE = 2, FR_CHUNK = kWave * FR_PER_LANE, FR_ROWS = 4;   // nodes per lane / per wave, rows (waves) per workgroup

typedef float F32x4a8 __attribute__((ext_vector_type(4), aligned(8)));   // 16 bytes at the field's 8-byte alignment (rows of odd width)

__global__ void __launch_bounds__(kWave *FR_ROWS) field_rigid_kernel(const float *field, const double *__restrict__ m, float *out, int fh, int fw,
                                                                      unsigned nrg, float r, double su, double sv, float half_w, float half_h,
                                                                      int *__restrict__ residual_bits, int *__restrict__ unfit) {
    __shared__ int cnt[FR_ROWS];
    __shared__ float big[FR_ROWS];
    const unsigned t = blockIdx.x / nrg, rg = blockIdx.x - t * nrg;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = (int)(threadIdx.x & 63u);
    const int i = (int)rg * FR_ROWS + wave, j0 = (int)blockIdx.y * FR_CHUNK + lane * FR_PER_LANE;
    int kept = 0;
    float res = 0.f;
    if (i < fh && j0 < fw) {
        // ---- wave-uniform: the adjugate, the fitted test, the row's terms
        const RigidFrame frame = rigid_frame(m + (size_t)t * 9);   // (rigid_position.h: shared with field_wobble.hip)
        const RigidRow row = rigid_row(frame, (double)i * sv - 1.0);
        // ---- the lane's two nodes
        const bool two = j0 + 1 < fw;   // (a row of odd width: its last lane holds one node)
        const float *f = field + (((size_t)t * fh + i) * fw + j0) * 2;
        F32x4a8 F;
        if (two) {
            F = *reinterpret_cast<const F32x4a8 *>(f);
        } else {
            const float2 h = *reinterpret_cast<const float2 *>(f);
            F = F32x4a8{h.x, h.y, h.x, h.y};
        }
        float g[FR_PER_LANE][2];
#pragma unroll
        for (int q = 0; q < FR_PER_LANE; ++q) {
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
        float *o = out + (((size_t)t * fh + i) * fw + j0) * 2;
        if (two) *reinterpret_cast<F32x4a8 *>(o) = F32x4a8{g[0][0], g[0][1], g[1][0], g[1][1]};
        else *reinterpret_cast<float2 *>(o) = make_float2(g[0][0], g[0][1]);
    }
    if (residual_bits || unfit) {   // (kernel arguments: uniform, every thread of the workgroup arrives)
        int s = kept;
        float b = res;
#pragma unroll
        for (int d = kWave / 2; d > 0; d >>= 1) {
            s += __shfl_xor(s, d, kWave);
            b = fmaxf(b, __shfl_xor(b, d, kWave));
        }
        if (lane == 0) cnt[wave] = s, big[wave] = b;
        __syncthreads();
        if (threadIdx.x == 0) {
            int tot = 0;
            float top = 0.f;
#pragma unroll
            for (int w = 0; w < FR_ROWS; ++w) tot += cnt[w], top = fmaxf(top, big[w]);
            if (unfit && tot != 0) atomicAdd(unfit + t, tot);
            if (residual_bits && top > 0.f) atomicMax(residual_bits + t, __float_as_int(top));   // (top >= 0: its bits order as ints)
        }
    }
}

}  // namespace
}  // namespace pws

using namespace pws;

extern "C" int pws_field_rigid(const float *field, int n, int fh, int fw, const double *m, float rigidity, int h0, int w0, float *out,
                               float *residual, int *unfit, pws_stream_t stream) {
    PWS_REQUIRE(n >= 0, "pws_field_rigid: bad shape");
    PWS_REQUIRE(fh >= 2 && fw >= 2, "pws_field_rigid: the field needs at least 2 x 2 nodes (got %d x %d)", fw, fh);
    PWS_REQUIRE(h0 >= 1 && w0 >= 1, "pws_field_rigid: bad frame size %d x %d", w0, h0);
    PWS_REQUIRE(rigidity >= 0.f && rigidity <= 1.f, "pws_field_rigid: rigidity must lie in [0, 1], got %g", (double)rigidity);   // (false for NaN)
    if (n == 0) return PWS_OK;
    PWS_REQUIRE(field && m && out, "pws_field_rigid: NULL pointer");
    PWS_REQUIRE(((reinterpret_cast<size_t>(field) | reinterpret_cast<size_t>(out) | reinterpret_cast<size_t>(m)) & 7) == 0 &&
                    ((reinterpret_cast<size_t>(residual) | reinterpret_cast<size_t>(unfit)) & 3) == 0,
                "pws_field_rigid: field, out and m must be 8-byte aligned, residual and unfit 4-byte aligned");
    const size_t bytes = (size_t)n * fh * fw * 2 * sizeof(float);
    const char *fb = reinterpret_cast<const char *>(field), *ob = reinterpret_cast<const char *>(out);
    PWS_REQUIRE(ob == fb || ob + bytes <= fb || fb + bytes <= ob, "pws_field_rigid: out must be field itself or must not overlap it");
    const unsigned nrg = (unsigned)((fh + FR_ROWS - 1) / FR_ROWS), chunks = (unsigned)((fw + FR_CHUNK - 1) / FR_CHUNK);
    PWS_REQUIRE((size_t)n * nrg < (1u << 31) && chunks < 65536, "pws_field_rigid: field or batch too large");
    void *const stats[2] = {residual, unfit};
    for (void *stat : stats) {
        if (!stat) continue;
        const hipError_t e = hipMemsetAsync(stat, 0, (size_t)n * 4, as_stream(stream));   // (0.0f and 0 alike)
        if (e != hipSuccess) {
            set_error("pws_field_rigid: clearing the statistics: %s", hipGetErrorString(e));
            return PWS_EHIP;
        }
    }
    // node j -> u = 2 (j (w0-1)/(fw-1)) / w0 - 1 = j su - 1; rows alike
    const double su = 2.0 * (double)(w0 - 1) / ((double)(fw - 1) * (double)w0), sv = 2.0 * (double)(h0 - 1) / ((double)(fh - 1) * (double)h0);
    hipLaunchKernelGGL(field_rigid_kernel, dim3((unsigned)n * nrg, chunks, 1), dim3(kWave * FR_ROWS), 0, as_stream(stream), field, m, out, fh, fw,
                       nrg, rigidity, su, sv, 0.5f * (float)w0, 0.5f * (float)h0, reinterpret_cast<int *>(residual), unfit);
    return check_launch("field_rigid_kernel");
}
