// Crop-bounded smoothing (stream.limit_path): the smoothing correction D of a frame scaled back to a share lam of itself, the table of
// such corrections that pws_field_reach classifies, and -- from its counts -- per frame the largest share that keeps the chosen window of
// the output covered, eased over time.  No counterpart in the reference.
//
// Definition (restated in tests/limit_ref.py; include/pwstable.h pws_path_levels / pws_path_limit have it in full).  D is a similarity, as
// pws_path_smooth writes it: ls = log(hypot(d0, d3)), phi = atan2(d3, d0); D(lam) has the linear part exp(lam ls) Rot(lam phi) and the
// translation lam (d2, d5) -- the geodesic from the identity to D in (log scale, angle, translation).  D(0) is exactly the identity; a row
// that is not finite is its own D(lam) for every lam (the composition keeps such frames' nodes).
//
// pws_path_limit is path_smooth_kernel's shape: one workgroup, one launch; the threads take the frames in turn for `need` and the raw
// strength, lane 0 walks the two sweeps (strictly sequential), the threads take the frames in turn again for d_out.
#include "common.h"

namespace pws {
namespace {

constexpr int PL_THREADS = 256, PL_LMAX = 64;

#pragma clang fp contract(off)   // every product and every sum rounded once, as the float64 restatement does

__device__ __forceinline__ bool finite6(const double *v) {
    return isfinite(v[0]) && isfinite(v[1]) && isfinite(v[2]) && isfinite(v[3]) && isfinite(v[4]) && isfinite(v[5]);
}

// o = D(lam) of the row d
__device__ __forceinline__ void level_row(const double *d, double lam, double *o) {
    if (!finite6(d)) {
#pragma unroll
        for (int c = 0; c < 6; ++c) o[c] = d[c];
        return;
    }
    if (lam == 0.0) {
        o[0] = 1.0, o[1] = 0.0, o[2] = 0.0, o[3] = 0.0, o[4] = 1.0, o[5] = 0.0;
        return;
    }
    const double ls = log(hypot(d[0], d[3])), phi = atan2(d[3], d[0]);
    const double s = exp(lam * ls), c = cos(lam * phi), sn = sin(lam * phi);
    o[0] = s * c, o[1] = 0.0 - s * sn, o[2] = lam * d[2];
    o[3] = s * sn, o[4] = s * c, o[5] = lam * d[5];
}

__global__ void __launch_bounds__(PL_THREADS) path_levels_kernel(const double *__restrict__ d, int n, int levels, double *__restrict__ table) {
    const size_t k = (size_t)blockIdx.x * PL_THREADS + threadIdx.x, nl = (size_t)levels + 1;
    if (k >= (size_t)n * nl) return;
    const size_t t = k / nl;
    const int l = (int)(k - t * nl);
    const double *dt = d + t * 6;
    double *o = table + k * 6;
    if (l == levels) {   // the row itself, verbatim
#pragma unroll
        for (int c = 0; c < 6; ++c) o[c] = dt[c];
        return;
    }
    level_row(dt, (double)l / (double)levels, o);
}

__global__ void __launch_bounds__(PL_THREADS) path_limit_kernel(const double *__restrict__ d, const int *__restrict__ counts, int n, int levels,
                                                                double relax, int *__restrict__ need, double *strength, double *__restrict__ d_out) {
    const int tid = threadIdx.x, nl = levels + 1;
    for (int t = tid; t < n; t += PL_THREADS) {
        int nd = levels;
        if (finite6(d + (size_t)t * 6)) {
            const int *c = counts + (size_t)t * nl;
            nd = -1;
            while (nd < levels && c[nd + 1] == 0) ++nd;   // the largest l with counts[t, l'] == 0 for every l' <= l
        }
        need[t] = nd;
        strength[t] = (double)(nd > 0 ? nd : 0) / (double)levels;
    }
    __syncthreads();   // (strength is in global memory: written by this workgroup, read by this workgroup)
    if (tid == 0) {
        for (int t = 1; t < n; ++t) {
            const double up = strength[t - 1] + relax;
            if (up < strength[t]) strength[t] = up;
        }
        for (int t = n - 2; t >= 0; --t) {
            const double up = strength[t + 1] + relax;
            if (up < strength[t]) strength[t] = up;
        }
    }
    __syncthreads();
    for (int t = tid; t < n; t += PL_THREADS) {
        const double *dt = d + (size_t)t * 6;
        double *o = d_out + (size_t)t * 6;
        const double lam = strength[t];
        if (lam == 1.0) {
#pragma unroll
            for (int c = 0; c < 6; ++c) o[c] = dt[c];
        } else {
            level_row(dt, lam, o);
        }
    }
}

}  // namespace
}  // namespace pws

using namespace pws;

extern "C" int pws_path_levels(const double *d, int n, int levels, double *table, pws_stream_t stream) {
    PWS_REQUIRE(n >= 0, "pws_path_levels: bad shape (n %d)", n);
    PWS_REQUIRE(levels >= 1 && levels <= PL_LMAX, "pws_path_levels: levels must lie in 1 .. %d, got %d", PL_LMAX, levels);
    if (n == 0) return PWS_OK;
    PWS_REQUIRE(d && table, "pws_path_levels: NULL pointer");
    PWS_REQUIRE(((reinterpret_cast<size_t>(d) | reinterpret_cast<size_t>(table)) & 7) == 0, "pws_path_levels: d and table must be 8-byte aligned");
    PWS_REQUIRE(n <= (1 << 24), "pws_path_levels: %d frames, at most 2^24", n);
    const size_t total = (size_t)n * (levels + 1);
    hipLaunchKernelGGL(path_levels_kernel, dim3((unsigned)((total + PL_THREADS - 1) / PL_THREADS)), dim3(PL_THREADS), 0, as_stream(stream), d, n, levels,
                       table);
    return check_launch("path_levels_kernel");
}

extern "C" int pws_path_limit(const double *d, const int *counts, int n, int levels, double relax, int *need, double *strength, double *d_out,
                              pws_stream_t stream) {
    PWS_REQUIRE(n >= 0, "pws_path_limit: bad shape (n %d)", n);
    PWS_REQUIRE(levels >= 1 && levels <= PL_LMAX, "pws_path_limit: levels must lie in 1 .. %d, got %d", PL_LMAX, levels);
    PWS_REQUIRE(relax > 0.0 && relax <= 1.0, "pws_path_limit: relax must lie in (0, 1], got %g", relax);   // (false for NaN)
    if (n == 0) return PWS_OK;
    PWS_REQUIRE(d && counts && need && strength && d_out, "pws_path_limit: NULL pointer");
    PWS_REQUIRE(((reinterpret_cast<size_t>(d) | reinterpret_cast<size_t>(strength) | reinterpret_cast<size_t>(d_out)) & 7) == 0 &&
                    ((reinterpret_cast<size_t>(counts) | reinterpret_cast<size_t>(need)) & 3) == 0,
                "pws_path_limit: d, strength and d_out must be 8-byte aligned, counts and need 4-byte aligned");
    PWS_REQUIRE(n <= (1 << 24), "pws_path_limit: a scene of %d frames, at most 2^24", n);
    hipLaunchKernelGGL(path_limit_kernel, dim3(1), dim3(PL_THREADS), 0, as_stream(stream), d, counts, n, levels, relax, need, strength, d_out);
    return check_launch("path_limit_kernel");
}
