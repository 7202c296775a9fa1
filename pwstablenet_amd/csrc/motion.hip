// Global motion between consecutive window planes (stream.py block_motion / global_motion): the stabiliser shapes its output in a dozen ways
// and had nothing that measures whether a clip came out steadier than it went in.  The generator regresses a warp; it never measures
// motion.  This file measures it, on the 256 x 256 window planes the stabiliser already keeps, in two launches:
//
//   block_motion_kernel   one workgroup per (16 x 16 block, frame), 256 threads.  The samples are quantised to bytes ONCE (q = floor((v + 1) *
//                         127.5 + 0.5), clamped, NaN -> 0; the multiply and the adds are single roundings, never contracted): the block of
//                         frame t and the (16 + 2R)^2 search window of frame t-1 go to LDS as packed bytes, the window as four byte-shifted
//                         copies, so that the four dwords of a block row under ANY horizontal offset are aligned dword reads.  The (2R + 1)^2
//                         candidates are dealt over the lanes; a candidate is 64 v_sad_u8 against the block, which the lane holds in registers.
//                         The best candidate minimises (S, dx^2 + dy^2, dy, dx) lexicographically -- the order of S * 2048 + rank with rank =
//                         the candidate's position sorted by (dx^2 + dy^2, dy, dx), without a rank table -- by a wave and LDS reduction of one
//                         64-bit key.  Everything after q is integer arithmetic: exact, and the same bits under any schedule.
//   motion_fit_kernel     one workgroup per frame: a similarity p' = [[a, -b], [b, a]] p + t fitted in fp64 to the blocks' sub-pixel vectors
//                         in three rounds (all valid blocks; then twice the blocks within max(1, 4 x mean squared residual) of the previous
//                         fit).  Every sum is taken in one fixed order: a lane's blocks in index order, then a fixed butterfly.
//                         pws_motion_fit_scaled: the same kernel with the blocks' centres and vectors multiplied by (sx, sy) first -- the fit
//                         in FRAME pixels, of which the planes are a non-uniform resize -- and the floor 1 replaced by sx sy; (1, 1) is exact.
//                         The validity rule, the sub-pixel vector, the residual and the workgroup sum live in motion_blocks.h, which the
//                         rolling-shutter estimate (shutter_estimate.hip) shares.
// No global atomics; all stores are plain vector stores.
#include "motion_blocks.h"

namespace pws {

namespace {

constexpr int MO_WMAX = MO_B + 2 * MO_RMAX;   // 48: the search window's side at the largest radius
constexpr int MO_WD = 13;                     // dwords per window row in LDS (12 used; odd, so that rows spread over the banks)
constexpr int MO_CAND = (2 * MO_RMAX + 1) * (2 * MO_RMAX + 1);   // 1089

__device__ __forceinline__ unsigned quant(float v) {
    const float c = __fadd_rn(__fmul_rn(__fadd_rn(v, 1.0f), 127.5f), 0.5f);
    return c >= 0.0f ? (c < 255.0f ? (unsigned)floorf(c) : 255u) : 0u;   // (NaN fails the first comparison)
}

__device__ __forceinline__ unsigned long long wave_min(unsigned long long k) {
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) {
        const unsigned long long other = __shfl_xor(k, o);
        k = other < k ? other : k;
    }
    return k;
}

__global__ void __launch_bounds__(MO_THREADS) block_motion_kernel(const float *__restrict__ planes, int t0, int h, int w, int R, int nbx,
                                                                  short *__restrict__ mv, int *__restrict__ sad, int *__restrict__ activity) {
    __shared__ unsigned win[4][MO_WMAX][MO_WD];   // copy s, row r, dword j = the window row's bytes 4j + s .. 4j + s + 3
    __shared__ unsigned cur[MO_B][MO_B / 4];
    __shared__ int sads[MO_CAND];
    __shared__ unsigned long long best[MO_WAVES];
    __shared__ int act[MO_WAVES];
    const int tid = threadIdx.x, lane = tid % kWave, wave = tid / kWave;
    const int blk = blockIdx.x, t = t0 + (int)blockIdx.y;
    const int by = blk / nbx, bx = blk % nbx;
    const int W = MO_B + 2 * R, side = 2 * R + 1, ncand = side * side;
    const size_t plane = (size_t)h * w;
    unsigned char *curb = reinterpret_cast<unsigned char *>(&cur[0][0]);
    {   // the block of frame t: one sample per thread
        const int y = tid / MO_B, x = tid % MO_B;
        curb[tid] = (unsigned char)quant(planes[(size_t)t * plane + (size_t)(R + MO_B * by + y) * w + (R + MO_B * bx + x)]);
    }
    if (t > 0) {   // the search window of frame t-1 (rows 16 by .., columns 16 bx ..: inside the plane by the lattice's definition)
        const float *src = planes + (size_t)(t - 1) * plane + (size_t)(MO_B * by) * w + MO_B * bx;
        for (int i = tid; i < W * W; i += MO_THREADS) {
            const int r = i / W, c = i % W;
            const unsigned char q = (unsigned char)quant(src[(size_t)r * w + c]);
#pragma unroll
            for (int s = 0; s < 4; ++s)
                if (c >= s) reinterpret_cast<unsigned char *>(&win[s][r][0])[c - s] = q;
        }
    }
    __syncthreads();
    {   // activity of the block of frame t: |right - here| over 16 x 15 pairs, |below - here| over 15 x 16
        const int y = tid / MO_B, x = tid % MO_B;
        const int q = curb[tid];
        int a = 0;
        if (x + 1 < MO_B) a += abs((int)curb[tid + 1] - q);
        if (y + 1 < MO_B) a += abs((int)curb[tid + MO_B] - q);
#pragma unroll
        for (int o = kWave / 2; o > 0; o >>= 1) a += __shfl_xor(a, o);
        if (lane == 0) act[wave] = a;
    }
    const size_t ob = ((size_t)t * gridDim.x + blk);
    if (t == 0) {   // (uniform: no pair ends at frame 0; its rows of mv and sad are zero)
        __syncthreads();
        if (tid == 0) {
            activity[ob] = act[0] + act[1] + act[2] + act[3];
            *reinterpret_cast<unsigned *>(mv + ob * 2) = 0u;
        }
        if (tid < 5) sad[ob * 5 + tid] = 0;
        return;
    }
    unsigned c[MO_B][MO_B / 4];   // the block, in registers
#pragma unroll
    for (int y = 0; y < MO_B; ++y) {
        const uint4 v = *reinterpret_cast<const uint4 *>(&cur[y][0]);
        c[y][0] = v.x, c[y][1] = v.y, c[y][2] = v.z, c[y][3] = v.w;
    }
    unsigned long long key = ~0ull;
    for (int ci = tid; ci < ncand; ci += MO_THREADS) {
        const int cy = ci / side, cx = ci % side;   // = dy + R, dx + R: the window row and byte column of the candidate's top-left
        const unsigned *p = &win[cx & 3][cy][cx >> 2];
        unsigned s = 0;
#pragma unroll
        for (int y = 0; y < MO_B; ++y) {
#pragma unroll
            for (int j = 0; j < MO_B / 4; ++j) s = __builtin_amdgcn_sad_u8(c[y][j], p[y * MO_WD + j], s);
        }
        sads[ci] = (int)s;
        const int dx = cx - R, dy = cy - R;
        const unsigned long long k = ((unsigned long long)s << 32) | ((unsigned)(dx * dx + dy * dy) << 12) | ((unsigned)cy << 6) | (unsigned)cx;
        key = k < key ? k : key;
    }
    key = wave_min(key);
    if (lane == 0) best[wave] = key;
    __syncthreads();
    if (tid < 5) {
        unsigned long long k = best[0];
#pragma unroll
        for (int i = 1; i < MO_WAVES; ++i) k = best[i] < k ? best[i] : k;
        const int cy = (int)((k >> 6) & 63u), cx = (int)(k & 63u);
        // S at the best candidate and at its x-1, x+1, y-1, y+1 neighbours (-1 outside the search range)
        const int ny = cy + (tid == 3 ? -1 : tid == 4 ? 1 : 0), nx = cx + (tid == 1 ? -1 : tid == 2 ? 1 : 0);
        sad[ob * 5 + tid] = (ny >= 0 && ny < side && nx >= 0 && nx < side) ? sads[ny * side + nx] : -1;
        if (tid == 0) {
            *reinterpret_cast<unsigned *>(mv + ob * 2) = ((unsigned)(cx - R) & 0xffffu) | ((unsigned)(cy - R) << 16);
            activity[ob] = act[0] + act[1] + act[2] + act[3];
        }
    }
}

#pragma clang fp contract(off)   // the fit below rounds every product and every sum once, as the float64 restatement does

__global__ void __launch_bounds__(MO_THREADS) motion_fit_kernel(const short *__restrict__ mv, const int *__restrict__ sad,
                                                                const int *__restrict__ activity, int h, int w, int R, int nby, int nbx,
                                                                int min_activity, double sx, double sy, double *__restrict__ motion,
                                                                int *__restrict__ inliers) {
    __shared__ double part[MO_WAVES][8];
    const int tid = threadIdx.x, t = blockIdx.x;
    double *mo = motion + (size_t)t * 4;
    if (t == 0) {   // (uniform) no pair ends at frame 0
        if (tid == 0) mo[0] = 1.0, mo[1] = 0.0, mo[2] = 0.0, mo[3] = 0.0, inliers[0] = 0;
        return;
    }
    const int nb = nby * nbx;
    const double cx0 = 0.5 * (double)(w - 1), cy0 = 0.5 * (double)(h - 1);
    Sim fit = {0.0, 0.0, 0.0, 0.0}, prev = fit;   // this round's fit, and the one that chose this round's blocks
    double thr = 0.0;
    int count = 0;
    bool ok = true;
    for (int round = 0; round < 3 && ok; ++round) {   // (uniform: the sums are the same in every thread, so every thread takes every barrier)
        double s[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // N, Sx, Sy, S(x^2 + y^2), Sdx, Sdy, S(x dx + y dy), S(x dy - y dx)
        for (int i = tid; i < nb; i += MO_THREADS) {
            const Blk b = load_block(mv, sad, activity, (size_t)t * nb + i, i, nbx, R, min_activity, cx0, cy0, sx, sy);
            if (!b.valid || (round > 0 && !(residual2(prev, b) <= thr))) continue;
            s[0] += 1.0, s[1] += b.x, s[2] += b.y, s[3] += b.x * b.x + b.y * b.y, s[4] += b.dx, s[5] += b.dy;
            s[6] += b.x * b.dx + b.y * b.dy, s[7] += b.x * b.dy - b.y * b.dx;
        }
        block_sum<8>(s, part);
        count = (int)s[0];
        const double den = s[3] - (s[1] * s[1] + s[2] * s[2]) / s[0];
        if (count < MO_MIN_BLOCKS || !(den > 0.0)) {
            ok = false;
            break;
        }
        // the 4 x 4 normal system of (a, b, tx, ty), solved in closed form: the translation eliminated, then a - 1 and b from the centred sums
        fit.a1 = (s[6] - (s[1] * s[4] + s[2] * s[5]) / s[0]) / den;
        fit.b = (s[7] - (s[1] * s[5] - s[2] * s[4]) / s[0]) / den;
        fit.tx = ((s[4] - fit.a1 * s[1]) + fit.b * s[2]) / s[0];
        fit.ty = ((s[5] - fit.b * s[1]) - fit.a1 * s[2]) / s[0];
        if (round == 2) break;
        double q[1] = {0.0};   // the squared residuals of the blocks this round used, under this round's fit
        for (int i = tid; i < nb; i += MO_THREADS) {
            const Blk b = load_block(mv, sad, activity, (size_t)t * nb + i, i, nbx, R, min_activity, cx0, cy0, sx, sy);
            if (!b.valid || (round > 0 && !(residual2(prev, b) <= thr))) continue;
            q[0] += residual2(fit, b);
        }
        block_sum<1>(q, part);
        const double m4 = 4.0 * (q[0] / s[0]);
        const double floor2 = sx * sy;   // one squared plane pixel, in frame pixels
        thr = m4 > floor2 ? m4 : floor2;
        prev = fit;
    }
    if (tid == 0) {
        const double nan = __longlong_as_double(0x7ff8000000000000LL);
        mo[0] = ok ? 1.0 + fit.a1 : nan, mo[1] = ok ? fit.b : nan, mo[2] = ok ? fit.tx : nan, mo[3] = ok ? fit.ty : nan;
        inliers[t] = ok ? count : 0;
    }
}

}  // namespace
}  // namespace pws

using namespace pws;

extern "C" int pws_block_motion(const float *planes, int n, int h, int w, int radius, short *mv, int *sad, int *activity, pws_stream_t stream) {
    PWS_REQUIRE(n >= 0 && h > 0 && w > 0, "pws_block_motion: bad shape (n %d, h %d, w %d)", n, h, w);
    PWS_REQUIRE(radius >= 1 && radius <= MO_RMAX, "pws_block_motion: radius must be 1 .. %d, got %d", MO_RMAX, radius);
    const long long nby = ((long long)h - 2 * radius) / MO_B, nbx = ((long long)w - 2 * radius) / MO_B;
    PWS_REQUIRE(h - 2 * radius >= MO_B && w - 2 * radius >= MO_B, "pws_block_motion: a %d x %d plane holds no 16 x 16 block inside a margin of %d", h, w,
                radius);
    PWS_REQUIRE(nby * nbx <= (1 << 20), "pws_block_motion: %lld x %lld blocks per plane, at most 2^20", nby, nbx);
    PWS_REQUIRE((long long)h * w <= 0x7fffffffLL, "pws_block_motion: a plane of %d x %d samples overflows 32-bit indices", h, w);
    if (n == 0) return PWS_OK;
    PWS_REQUIRE(planes && mv && sad && activity, "pws_block_motion: NULL pointer");
    PWS_REQUIRE(((reinterpret_cast<size_t>(planes) | reinterpret_cast<size_t>(mv) | reinterpret_cast<size_t>(sad) | reinterpret_cast<size_t>(activity)) & 3) == 0,
                "pws_block_motion: planes, mv, sad and activity must be 4-byte aligned");
    hipStream_t st = as_stream(stream);
    constexpr int kSlab = 32768;   // frames per launch (grid.y is limited to 65535)
    for (int t0 = 0; t0 < n; t0 += kSlab) {
        const int cnt = n - t0 < kSlab ? n - t0 : kSlab;
        hipLaunchKernelGGL(block_motion_kernel, dim3((unsigned)(nby * nbx), (unsigned)cnt), dim3(MO_THREADS), 0, st, planes, t0, h, w, radius, (int)nbx,
                           mv, sad, activity);
        const int rc = check_launch("block_motion_kernel");
        if (rc != PWS_OK) return rc;
    }
    return PWS_OK;
}

static int motion_fit(const char *what, const short *mv, const int *sad, const int *activity, int n, int h, int w, int radius, int min_activity,
                      double sx, double sy, double *motion, int *inliers, pws_stream_t stream) {
    PWS_REQUIRE(n >= 0 && h > 0 && w > 0, "%s: bad shape (n %d, h %d, w %d)", what, n, h, w);
    PWS_REQUIRE(radius >= 1 && radius <= MO_RMAX, "%s: radius must be 1 .. %d, got %d", what, MO_RMAX, radius);
    const long long nby = ((long long)h - 2 * radius) / MO_B, nbx = ((long long)w - 2 * radius) / MO_B;
    PWS_REQUIRE(h - 2 * radius >= MO_B && w - 2 * radius >= MO_B, "%s: a %d x %d plane holds no 16 x 16 block inside a margin of %d", what, h, w, radius);
    PWS_REQUIRE(nby * nbx <= (1 << 20), "%s: %lld x %lld blocks per plane, at most 2^20", what, nby, nbx);
    PWS_REQUIRE(sx > 0.0 && sy > 0.0 && sx <= 1e6 && sy <= 1e6, "%s: the pixel scale must be positive and finite, got (%g, %g)", what, sx, sy);
    if (n == 0) return PWS_OK;
    PWS_REQUIRE(mv && sad && activity && motion && inliers, "%s: NULL pointer", what);
    PWS_REQUIRE(((reinterpret_cast<size_t>(mv) | reinterpret_cast<size_t>(sad) | reinterpret_cast<size_t>(activity) | reinterpret_cast<size_t>(inliers)) & 3) == 0 &&
                    (reinterpret_cast<size_t>(motion) & 7) == 0,
                "%s: mv, sad, activity and inliers must be 4-byte aligned, motion 8-byte aligned", what);
    hipLaunchKernelGGL(motion_fit_kernel, dim3((unsigned)n), dim3(MO_THREADS), 0, as_stream(stream), mv, sad, activity, h, w, radius, (int)nby, (int)nbx,
                       min_activity, sx, sy, motion, inliers);
    return check_launch("motion_fit_kernel");
}

extern "C" int pws_motion_fit(const short *mv, const int *sad, const int *activity, int n, int h, int w, int radius, int min_activity, double *motion,
                              int *inliers, pws_stream_t stream) {
    return motion_fit("pws_motion_fit", mv, sad, activity, n, h, w, radius, min_activity, 1.0, 1.0, motion, inliers, stream);
}

extern "C" int pws_motion_fit_scaled(const short *mv, const int *sad, const int *activity, int n, int h, int w, int radius, int min_activity, double sx,
                                     double sy, double *motion, int *inliers, pws_stream_t stream) {
    return motion_fit("pws_motion_fit_scaled", mv, sad, activity, n, h, w, radius, min_activity, sx, sy, motion, inliers, stream);
}
