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
// Launch shape: a wave owns 128 consecutive nodes of ONE row of one frame, a lane 2 adjacent ones (one 16-byte store); a workgroup is 4
// waves = 4 rows.  The row's sy, y0, ly are wave-uniform.  Per node and field row a lane loads the 16 bytes of columns min(x0, fw-2) and the
// next one -- both corners at once; at the last column (lx = 0) both corners are the second half.  The count is summed per wave by ballot,
// per workgroup through LDS, and added with one integer atomic per workgroup that found any: exact, the same on every run.
#include "common.h"
#include "warp_common.h"

namespace pws {
namespace {

constexpr int FZ_PER_LANE = 2, FZ_CHUNK = kWave * FZ_PER_LANE, FZ_ROWS = 4;   // nodes per lane / per wave, rows (waves) per workgroup

typedef float F32x4a8 __attribute__((ext_vector_type(4), aligned(8)));   // 16 bytes at the field's 8-byte alignment (rows of odd width)

__device__ __forceinline__ float clamp_pos(float v, float hi) { return fminf(fmaxf(v, 0.f), hi); }   // (NaN -> 0)

__global__ void __launch_bounds__(kWave *FZ_ROWS) field_zoom_kernel(const float *__restrict__ field, const float *__restrict__ coef,
                                                                     float *__restrict__ out, int fh, int fw, unsigned nrg, int h0, int w0,
                                                                     int align_corners, float m, int *__restrict__ uncovered) {
    __shared__ int cnt[FZ_ROWS];
    const unsigned t = blockIdx.x / nrg, rg = blockIdx.x - t * nrg;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = (int)(threadIdx.x & 63u);
    const int i = (int)rg * FZ_ROWS + wave, j0 = (int)blockIdx.y * FZ_CHUNK + lane * FZ_PER_LANE;
    int unc = 0;
    if (i < fh && j0 < fw) {
        const float ax = coef[(size_t)t * 4], bx = coef[(size_t)t * 4 + 1], ay = coef[(size_t)t * 4 + 2], by = coef[(size_t)t * 4 + 3];
        const float sy = clamp_pos(fmaf(by, (float)i, ay), (float)(fh - 1));
        const int y0 = min(max((int)sy, 0), fh - 1), y1 = y0 + (y0 < fh - 1 ? 1 : 0);   // (the integer clamp: in bounds whatever coef holds)
        const float ly = sy - (float)y0, hy = 1.f - ly;
        const float *f0 = field + ((size_t)t * fh + y0) * fw * 2, *f1 = field + ((size_t)t * fh + y1) * fw * 2;
        const bool ac = align_corners != 0;
        const float xhi = (float)(w0 - 1) - m, yhi = (float)(h0 - 1) - m;
        float g[FZ_PER_LANE][2];
#pragma unroll
        for (int q = 0; q < FZ_PER_LANE; ++q) {
            const int j = min(j0 + q, fw - 1);   // (a row of odd width: the last lane's second node repeats its first, and is dropped)
            const float sx = clamp_pos(fmaf(bx, (float)j, ax), (float)(fw - 1));
            const int x0 = min(max((int)sx, 0), fw - 1), xb = min(x0, fw - 2);
            const float lx = sx - (float)x0, hx = 1.f - lx;
            const F32x4a8 r0 = *reinterpret_cast<const F32x4a8 *>(f0 + (size_t)xb * 2), r1 = *reinterpret_cast<const F32x4a8 *>(f1 + (size_t)xb * 2);
            const bool last = x0 > xb;   // x0 = x1 = fw-1
            const float a0 = last ? r0.z : r0.x, a1 = last ? r0.w : r0.y, c0 = last ? r1.z : r1.x, c1 = last ? r1.w : r1.y;
            g[q][0] = field_lerp(hy, ly, hx, lx, a0, r0.z, c0, r1.z);
            g[q][1] = field_lerp(hy, ly, hx, lx, a1, r0.w, c1, r1.w);
            if (uncovered && j0 + q < fw) {
                const float ix = unnormalize(g[q][0], w0, ac), iy = unnormalize(g[q][1], h0, ac);
                const bool covered = ix >= m && ix <= xhi && iy >= m && iy <= yhi;   // (false for NaN)
                unc += covered ? 0 : 1;
            }
        }
        float *o = out + (((size_t)t * fh + i) * fw + j0) * 2;
        if (j0 + 1 < fw) *reinterpret_cast<F32x4a8 *>(o) = F32x4a8{g[0][0], g[0][1], g[1][0], g[1][1]};
        else *reinterpret_cast<float2 *>(o) = make_float2(g[0][0], g[0][1]);
    }
    if (uncovered) {   // (kernel argument: uniform, every thread of the workgroup arrives)
        int s = unc;
#pragma unroll
        for (int d = kWave / 2; d > 0; d >>= 1) s += __shfl_xor(s, d, kWave);
        if (lane == 0) cnt[wave] = s;
        __syncthreads();
        if (threadIdx.x == 0) {
            int tot = 0;
#pragma unroll
            for (int w = 0; w < FZ_ROWS; ++w) tot += cnt[w];
            if (tot != 0) atomicAdd(uncovered + t, tot);
        }
    }
}

}  // namespace
}  // namespace pws

using namespace pws;

extern "C" int pws_field_zoom(const float *field, int n, int fh, int fw, const float *coef, float *out, int h0, int w0, int align_corners, int margin,
                              int *uncovered, pws_stream_t stream) {
    PWS_REQUIRE(n >= 0, "pws_field_zoom: bad shape");
    PWS_REQUIRE(fh >= 2 && fw >= 2, "pws_field_zoom: the field needs at least 2 x 2 nodes (got %d x %d)", fw, fh);
    PWS_REQUIRE(!uncovered || (h0 >= 1 && w0 >= 1 && margin >= 0), "pws_field_zoom: bad frame size %d x %d or margin %d for the uncovered count", w0,
                h0, margin);
    if (n == 0) return PWS_OK;
    PWS_REQUIRE(field && coef && out, "pws_field_zoom: NULL pointer");
    PWS_REQUIRE(((reinterpret_cast<size_t>(field) | reinterpret_cast<size_t>(out)) & 7) == 0 && (reinterpret_cast<size_t>(coef) & 3) == 0 &&
                    (reinterpret_cast<size_t>(uncovered) & 3) == 0,
                "pws_field_zoom: field and out must be 8-byte aligned, coef and uncovered 4-byte aligned");
    const size_t bytes = (size_t)n * fh * fw * 2 * sizeof(float);
    const char *fb = reinterpret_cast<const char *>(field), *ob = reinterpret_cast<const char *>(out);
    PWS_REQUIRE(ob + bytes <= fb || fb + bytes <= ob, "pws_field_zoom: out must not overlap field");
    const unsigned nrg = (unsigned)((fh + FZ_ROWS - 1) / FZ_ROWS), chunks = (unsigned)((fw + FZ_CHUNK - 1) / FZ_CHUNK);
    PWS_REQUIRE((size_t)n * nrg < (1u << 31) && chunks < 65536, "pws_field_zoom: field or batch too large");
    if (uncovered) {
        const hipError_t e = hipMemsetAsync(uncovered, 0, (size_t)n * sizeof(int), as_stream(stream));
        if (e != hipSuccess) {
            set_error("pws_field_zoom: clearing uncovered: %s", hipGetErrorString(e));
            return PWS_EHIP;
        }
    }
    hipLaunchKernelGGL(field_zoom_kernel, dim3((unsigned)n * nrg, chunks, 1), dim3(kWave * FZ_ROWS), 0, as_stream(stream), field, coef, out, fh, fw,
                       nrg, h0, w0, align_corners, (float)margin, uncovered);
    return check_launch("field_zoom_kernel");
}
