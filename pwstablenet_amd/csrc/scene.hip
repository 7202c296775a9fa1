// Scene-cut score of the streaming stabiliser (stream.py scene_scores): the reference clamps a frame's 31-plane window at the clip's first
// and last frame only (main_new.py:627-633,653-660); edited footage needs the same clamp at every hard cut, and the planes a detector can
// read exist only on the device.  The input is shaky by definition, so a pixel difference says nothing; the score is the L1 distance of
// BLOCK-WISE HISTOGRAMS of consecutive window planes: a 4 x 4 grid of blocks, 32 bins each, 512 counters per frame.
//
//   scene_hist_kernel   one workgroup per (block, frame), 256 threads.  Lanes read float4 (a 256-wide plane: 16 lanes per block row), bin the
//                       four samples and count into the wave's PRIVATE 32-counter histogram in LDS.  Neighbouring pixels of a smooth frame
//                       fall into one to three bins, so the wave aggregates first: the lanes that hold the leader's bin are counted with a
//                       ballot and ONE lane adds that count -- one LDS atomic per distinct bin, not 64 colliding ones.  The four wave
//                       histograms are summed and stored with plain vector stores: no global atomics.
//   scene_sad_kernel    one workgroup per frame t >= 1: sum |hist[t] - hist[t-1]| over the 512 counters.
// Everything after the bin is integer arithmetic: the counters and the distance are exact, independent of order and equal from run to run.
#include "common.h"

namespace pws {

namespace {

constexpr int SC_GRID = 4, SC_BLOCKS = SC_GRID * SC_GRID, SC_BINS = 32, SC_THREADS = 256, SC_WAVES = SC_THREADS / kWave;

// bin of a sample v in [-1, 1]: x = (v + 1) * 16, bin 0 if !(x >= 0) (NaN and everything below -1), else min(31, (int)x).
// The multiply is by a power of two, so fmaf(v, 16, 16) and the two-step form round identically (scaling by 16 is exact: one rounding,
// that of v + 1, either way): the compiler's contraction cannot change a bin.
__device__ __forceinline__ int scene_bin(float v) {
    const float x = (v + 1.0f) * 16.0f;
    return x >= 0.0f ? (x < (float)SC_BINS ? (int)x : SC_BINS - 1) : 0;   // (x >= 32, +inf included, never reaches the conversion)
}

// counts the wave's samples (one per lane where `valid`) into its histogram: one add per distinct bin among the lanes
__device__ __forceinline__ void wave_count(unsigned *hw, int bin, bool valid, int lane) {
    unsigned long long todo = __ballot(valid);
    while (todo) {   // (wave-uniform)
        const int leader = __ffsll((long long)todo) - 1;
        const int lb = __builtin_amdgcn_readlane(bin, leader);
        const unsigned long long same = __ballot(valid && bin == lb);
        if (lane == leader) atomicAdd(&hw[lb], (unsigned)__popcll(same));
        todo &= ~same;
    }
}

template <bool VEC4>
__global__ void __launch_bounds__(SC_THREADS) scene_hist_kernel(const float *__restrict__ planes, int h, int w, unsigned *__restrict__ hist,
                                                                unsigned *__restrict__ sad0) {
    __shared__ unsigned hw[SC_WAVES][SC_BINS];
    const int tid = threadIdx.x, lane = tid % kWave, wave = tid / kWave;
    const int blk = blockIdx.x, t = blockIdx.y;
    const int bh = h / SC_GRID, bw = w / SC_GRID;
    if (tid < SC_WAVES * SC_BINS) (&hw[0][0])[tid] = 0u;
    __syncthreads();
    const float *src = planes + (size_t)t * h * w + (size_t)(blk / SC_GRID) * bh * w + (size_t)(blk % SC_GRID) * bw;
    if constexpr (VEC4) {
        const int vpr = bw / 4, items = bh * vpr;
        for (int i0 = 0; i0 < items; i0 += SC_THREADS) {   // (uniform trip count: the ballots see every lane)
            const int i = i0 + tid;
            const bool valid = i < items;
            const int r = valid ? i / vpr : 0, c = valid ? i % vpr : 0;
            const float4 v = *reinterpret_cast<const float4 *>(src + (size_t)r * w + c * 4);
            wave_count(hw[wave], scene_bin(v.x), valid, lane);
            wave_count(hw[wave], scene_bin(v.y), valid, lane);
            wave_count(hw[wave], scene_bin(v.z), valid, lane);
            wave_count(hw[wave], scene_bin(v.w), valid, lane);
        }
    } else {
        const int items = bh * bw;
        for (int i0 = 0; i0 < items; i0 += SC_THREADS) {
            const int i = i0 + tid;
            const bool valid = i < items;
            const int r = valid ? i / bw : 0, c = valid ? i % bw : 0;
            wave_count(hw[wave], scene_bin(src[(size_t)r * w + c]), valid, lane);
        }
    }
    __syncthreads();
    if (tid < SC_BINS) {
        unsigned s = 0;
#pragma unroll
        for (int k = 0; k < SC_WAVES; ++k) s += hw[k][tid];
        hist[((size_t)t * SC_BLOCKS + blk) * SC_BINS + tid] = s;
    }
    if (sad0 && blk == 0 && t == 0 && tid == 0) *sad0 = 0u;
}

__global__ void __launch_bounds__(SC_THREADS) scene_sad_kernel(const unsigned *__restrict__ hist, unsigned *__restrict__ sad) {
    __shared__ unsigned part[SC_WAVES];
    const int tid = threadIdx.x, lane = tid % kWave, wave = tid / kWave;
    const size_t t = (size_t)blockIdx.x + 1;
    constexpr int N = SC_BLOCKS * SC_BINS;   // 512 = 2 per thread
    const uint2 a = *reinterpret_cast<const uint2 *>(hist + t * N + tid * 2);
    const uint2 b = *reinterpret_cast<const uint2 *>(hist + (t - 1) * N + tid * 2);
    unsigned s = (a.x > b.x ? a.x - b.x : b.x - a.x) + (a.y > b.y ? a.y - b.y : b.y - a.y);
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if (lane == 0) part[wave] = s;
    __syncthreads();
    if (tid == 0) {
        unsigned tot = 0;
#pragma unroll
        for (int k = 0; k < SC_WAVES; ++k) tot += part[k];
        sad[t] = tot;
    }
}

}  // namespace
}  // namespace pws

using namespace pws;

extern "C" int pws_scene_change(const float *planes, int n, int h, int w, unsigned *hist, unsigned *sad, pws_stream_t stream) {
    PWS_REQUIRE(n >= 0 && h > 0 && w > 0, "pws_scene_change: bad shape (n %d, h %d, w %d)", n, h, w);
    PWS_REQUIRE(h % SC_GRID == 0 && w % SC_GRID == 0, "pws_scene_change: h and w must be multiples of 4 (the 4 x 4 block grid), got %d x %d",
                h, w);
    PWS_REQUIRE((long long)h * w <= 0x7fffffffLL, "pws_scene_change: a plane of %d x %d samples overflows the 32-bit counters", h, w);
    if (n == 0) return PWS_OK;
    PWS_REQUIRE(planes && hist && sad, "pws_scene_change: NULL pointer");
    PWS_REQUIRE((reinterpret_cast<size_t>(planes) & 3) == 0 && (reinterpret_cast<size_t>(hist) & 7) == 0 &&
                    (reinterpret_cast<size_t>(sad) & 3) == 0,
                "pws_scene_change: planes and sad must be 4-byte aligned, hist 8-byte aligned");
    hipStream_t st = as_stream(stream);
    // float4 loads need block rows that start and end on 16 bytes: (w / 4) % 4 == 0 (then w % 4 == 0 too) and an aligned base
    const bool vec4 = (w / SC_GRID) % 4 == 0 && (reinterpret_cast<size_t>(planes) & 15) == 0;
    constexpr int kSlab = 32768;   // frames per launch (grid.y is limited to 65535)
    for (int t0 = 0; t0 < n; t0 += kSlab) {
        const int cnt = n - t0 < kSlab ? n - t0 : kSlab;
        const float *p = planes + (size_t)t0 * h * w;
        unsigned *hp = hist + (size_t)t0 * SC_BLOCKS * SC_BINS;
        unsigned *s0 = t0 == 0 ? sad : nullptr;
        if (vec4)
            hipLaunchKernelGGL(scene_hist_kernel<true>, dim3(SC_BLOCKS, (unsigned)cnt), dim3(SC_THREADS), 0, st, p, h, w, hp, s0);
        else
            hipLaunchKernelGGL(scene_hist_kernel<false>, dim3(SC_BLOCKS, (unsigned)cnt), dim3(SC_THREADS), 0, st, p, h, w, hp, s0);
        const int rc = check_launch("scene_hist_kernel");
        if (rc != PWS_OK) return rc;
    }
    if (n > 1) {
        hipLaunchKernelGGL(scene_sad_kernel, dim3((unsigned)(n - 1)), dim3(SC_THREADS), 0, st, hist, sad);
        return check_launch("scene_sad_kernel");
    }
    return PWS_OK;
}
