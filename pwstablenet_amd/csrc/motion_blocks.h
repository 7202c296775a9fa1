// What the global-motion fit (motion.hip) and the rolling-shutter estimate (shutter_estimate.hip) share: the blocks' lattice, the ONE
// validity rule and sub-pixel vector of a block, the residual against a similarity, and the workgroup sum in a fixed order.
#pragma once
#include "common.h"

namespace pws {

constexpr int MO_B = 16, MO_RMAX = 16, MO_THREADS = 256, MO_WAVES = MO_THREADS / kWave;
constexpr int MO_MIN_BLOCKS = 8;

// the sum of V doubles per thread over the workgroup, in a fixed order (butterfly inside the wave, then the waves in index order); every
// thread gets the totals
template <int V>
__device__ __forceinline__ void block_sum(double (&v)[V], double (*part)[8]) {
    const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
#pragma unroll
    for (int i = 0; i < V; ++i) {
#pragma unroll
        for (int o = kWave / 2; o > 0; o >>= 1) v[i] += __shfl_xor(v[i], o);
    }
    __syncthreads();   // (the previous call's totals have been read)
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < V; ++i) part[wave][i] = v[i];
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < V; ++i) {
        double s = part[0][i];
#pragma unroll
        for (int k = 1; k < MO_WAVES; ++k) s += part[k][i];
        v[i] = s;
    }
}


#pragma clang fp contract(off)   // the fit below rounds every product and every sum once, as the float64 restatement does

struct Sim {
    double a1, b, tx, ty;   // a - 1, b and the translation: a block centre p maps to p + (a1 x - b y + tx, b x + a1 y + ty)
};

struct Blk {
    bool valid;
    double x, y, dx, dy;   // the block's centre relative to the plane's, and its sub-pixel vector
};

__device__ __forceinline__ Blk load_block(const short *__restrict__ mv, const int *__restrict__ sad, const int *__restrict__ activity, size_t o,
                                          int i, int nbx, int R, int min_activity, double cx0, double cy0, double sx, double sy) {
    Blk b;
    const int dxi = mv[o * 2], dyi = mv[o * 2 + 1];
    // a best match on the rim of the search range means that the motion lies outside the range
    b.valid = activity[o] >= min_activity && abs(dxi) < R && abs(dyi) < R;
    const int *sd = sad + o * 5;
    const int c0 = sd[0];
    // ... and the match must be SHARP.  Around a true match S rises like |d| times the block's summed gradient along d, so its second
    // difference on an axis is at least that axis's gradient sum and the two together at least about the activity; a block whose content is
    // not in the window at all (motion beyond the range, an occlusion) settles on the best of (2R + 1)^2 chance matches, around which S is
    // flat.  Half the bound is asked for -- integers, like everything before the fit.  (Inside the rim all four neighbours exist.)
    b.valid = b.valid && 2 * ((sd[1] - 2 * c0 + sd[2]) + (sd[3] - 2 * c0 + sd[4])) >= activity[o];
    double off[2];
#pragma unroll
    for (int ax = 0; ax < 2; ++ax) {   // the parabola through S at the best candidate and its two neighbours on this axis
        const int lo = sd[1 + 2 * ax], hi = sd[2 + 2 * ax];
        const int den = lo - 2 * c0 + hi;
        // (S = 0 is an exact match: the vector is the whole-pixel one, and the neighbours' S says nothing about a fraction)
        const double f = (c0 > 0 && lo >= 0 && hi >= 0 && den > 0) ? 0.5 * (double)(lo - hi) / (double)den : 0.0;
        off[ax] = f > 0.5 ? 0.5 : (f < -0.5 ? -0.5 : f);
    }
    // (sx, sy): the plane is a resize of the frame, non-uniform for any source that is not square; centres and vectors go to frame pixels
    // here, before the sums.  A product with 1.0 is exact: at (1, 1) every sum below has the bits it had without the factors.
    b.dx = ((double)dxi + off[0]) * sx, b.dy = ((double)dyi + off[1]) * sy;
    b.x = (((double)(R + MO_B * (i % nbx)) + 7.5) - cx0) * sx, b.y = (((double)(R + MO_B * (i / nbx)) + 7.5) - cy0) * sy;
    return b;
}

__device__ __forceinline__ double residual2(const Sim &f, const Blk &b) {
    const double rx = ((f.a1 * b.x - f.b * b.y) + f.tx) - b.dx, ry = ((f.b * b.x + f.a1 * b.y) + f.ty) - b.dy;
    return rx * rx + ry * ry;
}

}  // namespace pws
