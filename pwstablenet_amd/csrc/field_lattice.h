// What the field-domain kernels (field_zoom.hip, field_compose.hip, field_rigid.hip, field_wobble.hip, field_reach.hip) have in common: how
// a workgroup is laid over the lattice of a field (n, fh, fw, 2), the access to a lane's pair of nodes, the exact reduction of per-frame
// statistics, the coverage rule, and the host checks that every export makes before it launches.  A new field operator is its node
// function, a ROWS and an export that lists these checks ("The field kernels: a lattice header, then a node").
//
// The lattice.  A wave owns kWaveNodes = 128 consecutive nodes of ONE row of one frame, a lane kLaneNodes = 2 adjacent ones: 16 bytes, one
// load or store.  A workgroup is ROWS waves = ROWS rows (the kernel's constant: 4, or 2 for the time-walking field_wobble.hip); blockIdx.y is
// the chunk of 128 columns.  A frame's rows start at 8-byte boundaries only (odd fw), hence F32x4a8; the last lane of a row of odd width
// holds ONE node (`two` false): load_pair repeats it, store_pair writes 8 bytes.
//
// The statistics.  Per wave a butterfly of shuffles, one LDS slot per wave, thread 0 sums the slots, then one integer atomic per workgroup
// that has something to report: a sum of counts, and a max on the bit pattern of a non-negative float, which orders as the float does.
// Integer arithmetic in a fixed tree: exact, the same on every run.
#pragma once
#include "common.h"
#include "warp_common.h"

namespace pws {

typedef float F32x4a8 __attribute__((ext_vector_type(4), aligned(8)));   // 16 bytes at the field's 8-byte alignment (rows of odd width)

constexpr int kLaneNodes = 2, kWaveNodes = kWave * kLaneNodes;   // nodes per lane / per wave

struct LatticePos {
    unsigned t;             // frame
    int wave, lane, i, j0;  // wave of the workgroup (uniform: an SGPR), lane; the lane's row and the first of its two columns
};

// Row group `rg` of frame `t` of a rectangle of the lattice whose first row and column are (i0, j0): for grids that are not lattice_pos's.
template <int ROWS>
__device__ __forceinline__ LatticePos lattice_rows(unsigned t, unsigned rg, int i0 = 0, int j0 = 0) {
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = (int)(threadIdx.x & 63u);
    return LatticePos{t, wave, lane, i0 + (int)rg * ROWS + wave, j0 + (int)blockIdx.y * kWaveNodes + lane * kLaneNodes};
}

// The grid (n * nrg, chunks) that lattice_grid sizes: blockIdx.x = frame * nrg + row group.
template <int ROWS>
__device__ __forceinline__ LatticePos lattice_pos(unsigned nrg, int i0 = 0, int j0 = 0) {
    const unsigned t = blockIdx.x / nrg;
    return lattice_rows<ROWS>(t, blockIdx.x - t * nrg, i0, j0);
}

__device__ __forceinline__ F32x4a8 load_pair(const float *f, bool two) {
    if (two) return *reinterpret_cast<const F32x4a8 *>(f);
    const float2 h = *reinterpret_cast<const float2 *>(f);
    return F32x4a8{h.x, h.y, h.x, h.y};
}

__device__ __forceinline__ void store_pair(float *o, bool two, const F32x4a8 &g) {
    if (two) *reinterpret_cast<F32x4a8 *>(o) = g;
    else *reinterpret_cast<float2 *>(o) = make_float2(g.x, g.y);
}

__device__ __forceinline__ int wave_sum(int s) {
#pragma unroll
    for (int d = kWave / 2; d > 0; d >>= 1) s += __shfl_xor(s, d, kWave);
    return s;
}

__device__ __forceinline__ void wave_sum_max(int &s, float &b) {   // (fmaxf drops a NaN)
#pragma unroll
    for (int d = kWave / 2; d > 0; d >>= 1) {
        s += __shfl_xor(s, d, kWave);
        b = fmaxf(b, __shfl_xor(b, d, kWave));
    }
}

// The workgroup's sum of `s` added to sum[p.t] if it is not 0.  `cnt`: ROWS words of LDS.  EVERY thread of the workgroup must arrive (a
// barrier): call it under a uniform condition only.
template <int ROWS>
__device__ __forceinline__ void block_sum(const LatticePos &p, int s, int *cnt, int *sum) {
    s = wave_sum(s);
    if (p.lane == 0) cnt[p.wave] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        int tot = 0;
#pragma unroll
        for (int w = 0; w < ROWS; ++w) tot += cnt[w];
        if (tot != 0) atomicAdd(sum + p.t, tot);
    }
}

// The same with the workgroup's largest b >= 0 raised into max_bits[p.t]; either destination may be NULL.
template <int ROWS>
__device__ __forceinline__ void block_sum_max(const LatticePos &p, int s, float b, int *cnt, float *big, int *sum, int *max_bits) {
    wave_sum_max(s, b);
    if (p.lane == 0) cnt[p.wave] = s, big[p.wave] = b;
    __syncthreads();
    if (threadIdx.x == 0) {
        int tot = 0;
        float top = 0.f;
#pragma unroll
        for (int w = 0; w < ROWS; ++w) tot += cnt[w], top = fmaxf(top, big[w]);
        if (sum && tot != 0) atomicAdd(sum + p.t, tot);
        if (max_bits && top > 0.f) atomicMax(max_bits + p.t, __float_as_int(top));   // (top >= 0: its bits order as ints)
    }
}

// The coverage rule at one field value: the warps' fp32 un-normalisation, inside [m, w0-1-m] x [m, h0-1-m] = [m, xhi] x [m, yhi]
// (border_keep.hip's rule at the field's nodes); NaN is not covered.
__device__ __forceinline__ bool node_covered(float gx, float gy, int h0, int w0, bool ac, float m, float xhi, float yhi) {
    const float ix = unnormalize(gx, w0, ac), iy = unnormalize(gy, h0, ac);
    return ix >= m && ix <= xhi && iy >= m && iy <= yhi;   // (false for NaN)
}

// ---- the host side of an export: each check returns PWS_OK or PWS_EINVAL / PWS_EHIP with the thread's message set, `who` in front

inline size_t addr(const void *p) { return reinterpret_cast<size_t>(p); }

inline int lattice_shape(const char *who, int n, int fh, int fw) {
    PWS_REQUIRE(n >= 0, "%s: bad shape", who);
    PWS_REQUIRE(fh >= 2 && fw >= 2, "%s: the field needs at least 2 x 2 nodes (got %d x %d)", who, fw, fh);
    return PWS_OK;
}

// `given`: no required pointer is NULL; a8 / a4: the addresses that must be 8- / 4-byte aligned, ORed (NULL passes); `rule` names them
inline int lattice_pointers(const char *who, bool given, size_t a8, size_t a4, const char *rule) {
    PWS_REQUIRE(given, "%s: NULL pointer", who);
    PWS_REQUIRE((a8 & 7) == 0 && (a4 & 3) == 0, "%s: %s", who, rule);
    return PWS_OK;
}

// out against the n fields; in_place: out may be field itself (an element-wise kernel); `rule`: the sentence, where it is not the usual one
inline int lattice_overlap(const char *who, const float *field, const float *out, int n, int fh, int fw, bool in_place, const char *rule = nullptr) {
    const size_t bytes = (size_t)n * fh * fw * 2 * sizeof(float);
    const char *fb = reinterpret_cast<const char *>(field), *ob = reinterpret_cast<const char *>(out);
    if (!rule) rule = in_place ? "out must be field itself or must not overlap it" : "out must not overlap field";
    PWS_REQUIRE((in_place && ob == fb) || ob + bytes <= fb || fb + bytes <= ob, "%s: %s", who, rule);
    return PWS_OK;
}

// rows x cols nodes per frame in row groups of `per` rows and chunks of 128 columns; nx * nrg blocks along x, nz along z; `unit`: what n counts
inline int lattice_grid(const char *who, int rows, int cols, int per, size_t nx, unsigned nz, const char *unit, unsigned &nrg, unsigned &chunks) {
    nrg = (unsigned)((rows + per - 1) / per), chunks = (unsigned)((cols + kWaveNodes - 1) / kWaveNodes);
    PWS_REQUIRE(nx * nrg < (1u << 31) && chunks < 65536 && nz < 65536, "%s: field or %s too large", who, unit);
    return PWS_OK;
}

// `bytes` of zeros (0.0f and 0 alike) into each statistics buffer that is given
inline int lattice_clear(const char *who, const char *what, size_t bytes, hipStream_t st, void *a, void *b = nullptr) {
    void *const stats[2] = {a, b};
    for (void *stat : stats) {
        if (!stat) continue;
        const hipError_t e = hipMemsetAsync(stat, 0, bytes, st);
        if (e != hipSuccess) {
            set_error("%s: clearing %s: %s", who, what, hipGetErrorString(e));
            return PWS_EHIP;
        }
    }
    return PWS_OK;
}

}  // namespace pws
