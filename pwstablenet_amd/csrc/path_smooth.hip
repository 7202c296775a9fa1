// Path smoothing (stream.smooth_path): the camera path that a scene's per-pair global motion (motion.hip) adds up to, its Gaussian low-pass,
// and per frame the correction that moves the frame from the measured path onto the smooth one.  No counterpart in the reference.
//
// Definition (restated in tests/path_ref.py; include/pwstable.h pws_path_smooth has it in full).  motion[k] = (a, b, tx, ty) maps a point
// of frame k to frame k-1.  The pose C_k = C_{k-1} o motion[k] maps frame k to frame 0; it is kept as P[k] = (lambda, theta, cx, cy): log
// scale, angle, translation.  P^[k] is the normalised Gaussian average of P over k-Re .. k+Re, with P continued beyond the scene's ends by
// odd reflection, so that a constant velocity is its own average at every frame.  D[k] = C_k^-1 o C^_k, row-major 2 x 3, maps a position
// of the smoothed frame to the position of the measured frame that shows the same point.
//
// One workgroup, one launch: lane 0 walks the scan (strictly sequential; a scene is thousands of frames at most), then the workgroup's
// threads take the frames in turn; the Gaussian's Re + 1 weights are in LDS.  Every sum has one fixed order: the same bits on every run.
#include "common.h"
#include "path_pose.h"

namespace pws {
namespace {

constexpr int PS_THREADS = 256, PS_RMAX = 768;   // Re <= ceil(3 * 256)

#pragma clang fp contract(off)   // every product and every sum rounded once, as the float64 restatement does

// P*(j), component c: P inside the scene, its odd reflection about the first / last frame outside (Re <= n-1 keeps both inside)
__device__ __forceinline__ double path_at(const double *path, int n, int j, int c) {
    if (j < 0) return 2.0 * path[c] - path[(size_t)(-j) * 4 + c];
    if (j > n - 1) return 2.0 * path[(size_t)(n - 1) * 4 + c] - path[(size_t)(2 * (n - 1) - j) * 4 + c];
    return path[(size_t)j * 4 + c];
}

__global__ void __launch_bounds__(PS_THREADS) path_smooth_kernel(const double *__restrict__ motion, int n, double sigma, int Re, double *path,
                                                                 double *__restrict__ d) {
    __shared__ double g[PS_RMAX + 1];
    const int tid = threadIdx.x;
    for (int k = tid; k <= Re; k += PS_THREADS) {
        const double r = (double)k / sigma;
        g[k] = exp(-0.5 * (r * r));
    }
    if (tid == 0) pose_scan(motion, n, path);   // (path_pose.h: shared with the L1-optimal path)
    __syncthreads();   // (the path is in global memory: written by this workgroup, read by this workgroup)
    for (int k = tid; k < n; k += PS_THREADS) {
        double acc[4] = {0.0, 0.0, 0.0, 0.0}, wsum = 0.0;
        for (int dl = -Re; dl <= Re; ++dl) {
            const double w = g[dl < 0 ? -dl : dl];
#pragma unroll
            for (int c = 0; c < 4; ++c) acc[c] = acc[c] + w * path_at(path, n, k + dl, c);
            wsum = wsum + w;
        }
        const double *p = path + (size_t)k * 4;
        pose_correction(p, acc[0] / wsum - p[0], acc[1] / wsum - p[1], acc[2] / wsum - p[2], acc[3] / wsum - p[3], d + (size_t)k * 6);
    }
}

// Rolling-shutter rates (stream.shutter_rates; include/pwstable.h pws_shutter_rates has the definition, tests/shutter_ref.py restates it):
// per frame k the camera's velocity (log scale, angle, x, y per frame interval) in frame k's own coordinates, once from the pair ahead --
// motion[k+1], which maps frame k+1 into frame k: (log s, f, tx, ty) -- and once from the pair behind -- motion[k], which maps frame k into
// frame k-1: the same generator seen from frame k, (log s, f, Rot(-f) (tx, ty) / s).  A scene's ends have one pair and use it twice.
// One thread per frame, nothing summed across threads: the same bits on every run.
__device__ __forceinline__ void rate_forward(const double *m, double *o) {
    const bool ok = finite4(m);
    const double a = ok ? m[0] : 1.0, b = ok ? m[1] : 0.0;
    o[0] = log(hypot(a, b)), o[1] = atan2(b, a), o[2] = ok ? m[2] : 0.0, o[3] = ok ? m[3] : 0.0;
}

__device__ __forceinline__ void rate_backward(const double *m, double *o) {
    const bool ok = finite4(m);
    const double a = ok ? m[0] : 1.0, b = ok ? m[1] : 0.0, tx = ok ? m[2] : 0.0, ty = ok ? m[3] : 0.0;
    const double s = hypot(a, b), f = atan2(b, a), c = cos(f), sn = sin(f);
    o[0] = log(s), o[1] = f, o[2] = (c * tx + sn * ty) / s, o[3] = ((0.0 - sn) * tx + c * ty) / s;
}

__global__ void __launch_bounds__(PS_THREADS) shutter_rates_kernel(const double *__restrict__ motion, int n, double *__restrict__ rates) {
    const int k = (int)(blockIdx.x * PS_THREADS + threadIdx.x);
    if (k >= n) return;
    double fwd[4] = {0.0, 0.0, 0.0, 0.0}, bwd[4] = {0.0, 0.0, 0.0, 0.0};
    const bool ahead = k + 1 < n, behind = k >= 1;   // (row 0 of a scene is not read, as in the path)
    if (ahead) rate_forward(motion + (size_t)(k + 1) * 4, fwd);
    if (behind) rate_backward(motion + (size_t)k * 4, bwd);
    double *o = rates + (size_t)k * 8;
#pragma unroll
    for (int c = 0; c < 4; ++c) o[c] = ahead ? fwd[c] : bwd[c], o[4 + c] = behind ? bwd[c] : fwd[c];
}

}  // namespace
}  // namespace pws

using namespace pws;

extern "C" int pws_shutter_rates(const double *motion, int n, double *rates, pws_stream_t stream) {
    PWS_REQUIRE(n >= 0, "pws_shutter_rates: bad shape (n %d)", n);
    if (n == 0) return PWS_OK;
    PWS_REQUIRE(motion && rates, "pws_shutter_rates: NULL pointer");
    PWS_REQUIRE(((reinterpret_cast<size_t>(motion) | reinterpret_cast<size_t>(rates)) & 7) == 0,
                "pws_shutter_rates: motion and rates must be 8-byte aligned");
    PWS_REQUIRE(n <= (1 << 24), "pws_shutter_rates: a scene of %d frames, at most 2^24", n);
    hipLaunchKernelGGL(shutter_rates_kernel, dim3((unsigned)((n + PS_THREADS - 1) / PS_THREADS)), dim3(PS_THREADS), 0, as_stream(stream), motion, n,
                       rates);
    return check_launch("shutter_rates_kernel");
}

extern "C" int pws_path_smooth(const double *motion, int n, double sigma, double *path, double *d, pws_stream_t stream) {
    PWS_REQUIRE(n >= 0, "pws_path_smooth: bad shape (n %d)", n);
    PWS_REQUIRE(sigma > 0.0 && sigma <= 256.0, "pws_path_smooth: sigma must lie in (0, 256], got %g", sigma);
    if (n == 0) return PWS_OK;
    PWS_REQUIRE(motion && path && d, "pws_path_smooth: NULL pointer");
    PWS_REQUIRE(((reinterpret_cast<size_t>(motion) | reinterpret_cast<size_t>(path) | reinterpret_cast<size_t>(d)) & 7) == 0,
                "pws_path_smooth: motion, path and d must be 8-byte aligned");
    PWS_REQUIRE(n <= (1 << 24), "pws_path_smooth: a scene of %d frames, at most 2^24", n);
    const int r3 = (int)ceil(3.0 * sigma), Re = r3 < n - 1 ? r3 : n - 1;
    hipLaunchKernelGGL(path_smooth_kernel, dim3(1), dim3(PS_THREADS), 0, as_stream(stream), motion, n, sigma, Re, path, d);
    return check_launch("path_smooth_kernel");
}
