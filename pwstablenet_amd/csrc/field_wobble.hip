// Wobble suppression: the non-rigid part of a scene's warp fields -- each field minus the homography fitted to it (pws_field_homography's M)
// -- low-passed along TIME with a Gaussian, the rigid part kept as it is.  What the generator regresses frame by frame from each frame's own
// window has nothing that ties the local, per-pixel part of consecutive fields together; this does, without giving up the per-pixel warp as
// rigid mode (field_rigid.hip) does.  No counterpart in the reference.
//
// Definition (restated in tests/wobble_ref.py; include/pwstable.h has it in full).  One call is one scene of n frames.  R = ceil(3 sigma)
// <= 15, g_k = exp(-k^2 / (2 sigma^2)) for |k| <= R, computed in fp64 on the host, rounded to fp32, passed as kernel arguments.  P[t] at
// node (i, j), FITTED and VALID are pws_field_rigid's (rigid_position.h: the same device code).  A (frame, node) pair is USABLE when the
// frame is fitted, the node valid and both components of F finite; then E = F - P (one fp32 subtraction per component).  A node that is not
// usable at t keeps F bit for bit and counts in unfit[t].  A usable one gets P[t] + S / W with S = sum g_k E[t+k] (fmaf(g_k, E, S)) and
// W = sum g_k (a plain fp32 addition), both over the k = -R .. R, ascending, with 0 <= t+k < n and (t+k, node) usable: no reflection, no
// padding.  removed[t] = the largest max(|out_x - F_x| w0/2, |out_y - F_y| h0/2) over the usable nodes of t (fmaxf: a NaN drops out), 0
// without any.
//
// Launch shape: a time-walking kernel on field_lattice.h's rows and lanes (16-byte loads and stores); a workgroup is 2 waves = 2 rows and
// the grid is (row groups, chunks, segments).  Segments in time supply the parallelism that the 512 waves of a 256 x 256 field lack: blockIdx.z is a segment of FW_L = 32 output frames, and a lane walks its 32 + 2R input frames once:
//   load F[tin], evaluate P[tin] (three fp64 divisions per node: ONCE per frame the lane visits, not once per tap), E[tin] into the ring;
//   then frame tout = tin - R has all its taps in the ring: sum, divide, store.
// The ring of the last 2R+1 residuals lives in REGISTERS: the kernel is a template on R and the walk is unrolled by the ring length 2R+1 --
// one template step per ring slot -- so that every ring index is static (a dynamically indexed array would go to scratch).  The usable flags are one bit per ring slot and node in
// two 32-bit masks.  Where all 2R+1 taps of a node are usable -- every interior frame of an ordinary clip -- W is the constant full sum.
// P[tout] is needed again R steps after it was computed: it waits in LDS (a delay line of R+1 slots x 16 bytes per lane, read only by the
// lane that wrote it: no barrier); F[tout] is read again from memory (a second read of the field, mostly from L2 / MALL).
// Re-read factor of the field and of the fp64 work: (L + 2R) / L = 1.06 (R = 1) .. 1.38 (sigma 2, R = 6) .. 1.94 (sigma 5, R = 15), plus the
// second read of F.  A scene of n <= 32 frames is one segment: 512 waves at 256 x 256.
// Statistics: per output frame and wave field_lattice.h's shuffle reduction, then lane 0 adds the count if it is not 0 and raises the
// maximum -- an integer atomic max on the bits of a non-negative float, attempted only when a relaxed load shows a smaller value (the value only grows, so a stale
// read costs one needless atomic at worst).  Exact, and the same on every run.  No floating-point atomics anywhere.
//
// Measured on an MI355X (profiles/wobble_bench.json), 128 x 256 x 256 nodes (64 MB in, 64 MB out): sigma 2 takes 61 us (0.48 us per frame),
// sigma 5 87 us, beside pws_field_rigid's 28 us and a device copy's 19 us on the same bytes: 2.2 x / 3.1 x rigid mode, which evaluates P once
// per node too.  With both statistics 207 / 221 us: 65 536 wave-level atomics on 128 adjacent words dominate then, as they do in
// field_rigid.hip (28 -> 70 us); a per-workgroup workspace and a finishing pass would remove them and was not tried.  The kernel's values
// were bit-equal to the float32 restatement (tests/wobble_ref.py wobble32) on every test case.
//
// hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage, per instantiation R: VGPRs / waves per SIMD / LDS bytes per block;
// 0 bytes of scratch in all fifteen (the ring's 4 (2R+1) registers are what the VGPR count follows):
//   R  1:  68 / 7 /  4096    R  2:  76 / 6 /  6144    R  3:  84 / 5 /  8192    R  4:  92 / 5 / 10240    R  5: 106 / 4 / 12288
//   R  6: 114 / 4 / 14336    R  7: 126 / 4 / 16384    R  8: 134 / 3 / 18432    R  9: 146 / 3 / 20480    R 10: 162 / 3 / 22528
//   R 11: 172 / 2 / 24576    R 12: 185 / 2 / 26624    R 13: 194 / 2 / 28672    R 14: 205 / 2 / 30720    R 15: 215 / 2 / 32768
// (An earlier form, `#pragma unroll` over the ring slots, was left rolled by the optimiser from R = 13 on and put the ring in scratch, 448 ..
// 512 bytes per lane: hence the template steps.)
#include "field_lattice.h"
#include "rigid_position.h"

#include <cmath>
#include <utility>

namespace pws {
namespace {

constexpr int FW_ROWS = 2;                   // rows (waves) per workgroup
constexpr int FW_L = PWS_WOBBLE_SEGMENT;    // output frames per segment
constexpr int FW_MAX_R = 15;                 // sigma <= 5

struct WobbleWeights {
    float g[FW_MAX_R + 1];   // g[|k|]; g[0] = 1
};

// One lane's walk.  The ring slot of step q is q mod (2R+1); step<S> is the step whose slot is S, so that every ring index below is a
// template constant and the ring stays in registers whatever the optimiser's unrolling budget says.
template <int R>
struct WobbleWalk {
    static constexpr int RING = 2 * R + 1;
    static constexpr unsigned FULL = (1u << RING) - 1u;   // (RING <= 31)
    const float *__restrict__ field;
    const double *__restrict__ m;
    float *__restrict__ out;
    f32x4 *pline;   // P of the last R+1 frames: this lane's column of the delay line in LDS, slots kWave * FW_ROWS apart
    int *__restrict__ removed_bits, *__restrict__ unfit;
    WobbleWeights wt;
    size_t node, frame_stride;
    double v, u0, u1;
    float half_w, half_h, wfull;
    int n, t0, steps, lane;
    bool active, two;
    float e[RING][4];      // the ring: E of the last 2R+1 frames, (x, y) of node 0, (x, y) of node 1; 0 where not usable
    unsigned use0, use1;   // bit s: ring slot s holds a usable residual of node 0 / node 1
    int pw;                // the delay line's slot of this step's P: q mod (R+1)

    __device__ __forceinline__ F32x4a8 load(int t) const {
        return load_pair(field + (size_t)t * frame_stride + node, two);
    }

    template <int S>
    __device__ __forceinline__ void step(int base) {
        const int q = base + S;
        if (q >= steps) return;   // (uniform)
        const int tin = t0 - R + q, tout = tin - R;
        // ---- the new frame's residual into slot S
        float ex0 = 0.f, ey0 = 0.f, ex1 = 0.f, ey1 = 0.f;
        bool us0 = false, us1 = false;
        if (tin >= 0 && tin < n && active) {   // (frames outside the scene are taps that drop out)
            const RigidFrame frame = rigid_frame(m + (size_t)tin * 9);
            const RigidRow row = rigid_row(frame, v);
            const F32x4a8 F = load(tin);
            float px0, py0, px1, py1;
            const bool v0 = rigid_node(frame, row, u0, px0, py0), v1 = rigid_node(frame, row, u1, px1, py1);
            us0 = v0 && __builtin_isfinite(F.x) && __builtin_isfinite(F.y);
            us1 = v1 && two && __builtin_isfinite(F.z) && __builtin_isfinite(F.w);
            if (us0) ex0 = F.x - px0, ey0 = F.y - py0;
            if (us1) ex1 = F.z - px1, ey1 = F.w - py1;
            pline[pw * (kWave * FW_ROWS)] = f32x4{px0, py0, px1, py1};
        }
        e[S][0] = ex0, e[S][1] = ey0, e[S][2] = ex1, e[S][3] = ey1;
        use0 = (use0 & ~(1u << S)) | (us0 ? 1u << S : 0u);
        use1 = (use1 & ~(1u << S)) | (us1 ? 1u << S : 0u);
        const int pr = pw == R ? 0 : pw + 1;   // (q - R) mod (R+1): where P[tout] waits
        pw = pr;                               // ... and the next step's slot
        if (tout < t0) return;   // (uniform: the lead-in.  tout < t1 by `steps`)
        // ---- frame tout: its taps k = -R .. R sit in slots (S + 1 + k + R) mod RING
        int kept = 0;
        float big = 0.f;
        if (active) {
            constexpr int C = (S + 1 + R) % RING;   // the centre tap's slot
            const F32x4a8 F = load(tout);
            const f32x4 P = pline[pr * (kWave * FW_ROWS)];
            float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
#pragma unroll
            for (int k = -R; k <= R; ++k) {
                const int slot = (S + 1 + k + R) % RING;
                const float g = wt.g[k < 0 ? -k : k];
                s0 = __builtin_fmaf(g, e[slot][0], s0), s1 = __builtin_fmaf(g, e[slot][1], s1);
                s2 = __builtin_fmaf(g, e[slot][2], s2), s3 = __builtin_fmaf(g, e[slot][3], s3);
            }
            float w0 = wfull, w1 = wfull;
            if (use0 != FULL || use1 != FULL) {   // (the scene's ends, unfitted frames, NaN nodes, the last lane of an odd row)
                w0 = w1 = 0.f;
#pragma unroll
                for (int k = -R; k <= R; ++k) {
                    const int slot = (S + 1 + k + R) % RING;
                    const float g = wt.g[k < 0 ? -k : k];
                    w0 += (use0 >> slot) & 1u ? g : 0.f;
                    w1 += (use1 >> slot) & 1u ? g : 0.f;
                }
            }
            float o0 = F.x, o1 = F.y, o2 = F.z, o3 = F.w;
            if ((use0 >> C) & 1u) {
                o0 = P.x + s0 / w0, o1 = P.y + s1 / w0;
                big = fmaxf(big, fmaxf(fabsf(o0 - F.x) * half_w, fabsf(o1 - F.y) * half_h));   // (fmaxf drops a NaN)
            } else {
                kept += 1;
            }
            if ((use1 >> C) & 1u) {
                o2 = P.z + s2 / w1, o3 = P.w + s3 / w1;
                big = fmaxf(big, fmaxf(fabsf(o2 - F.z) * half_w, fabsf(o3 - F.w) * half_h));
            } else {
                kept += two ? 1 : 0;
            }
            store_pair(out + (size_t)tout * frame_stride + node, two, F32x4a8{o0, o1, o2, o3});
        }
        if (removed_bits || unfit) {   // (kernel arguments: uniform)
            wave_sum_max(kept, big);
            if (lane == 0) {
                if (unfit && kept != 0) atomicAdd(unfit + tout, kept);
                // (big >= 0: its bits order as ints.  The value only grows: a stale read costs one needless atomic at worst)
                if (removed_bits && big > 0.f && __float_as_int(big) > __atomic_load_n(removed_bits + tout, __ATOMIC_RELAXED))
                    atomicMax(removed_bits + tout, __float_as_int(big));
            }
        }
    }

    template <int... S>
    __device__ __forceinline__ void round(int base, std::integer_sequence<int, S...>) {
        (step<S>(base), ...);
    }
};

template <int R>
__global__ void __launch_bounds__(kWave *FW_ROWS) field_wobble_kernel(const float *__restrict__ field, const double *__restrict__ m,
                                                                       float *__restrict__ out, int n, int fh, int fw, WobbleWeights wt,
                                                                       double su, double sv, float half_w, float half_h,
                                                                       int *__restrict__ removed_bits, int *__restrict__ unfit) {
    constexpr int RING = 2 * R + 1;
    __shared__ f32x4 pline[R + 1][kWave * FW_ROWS];
    const LatticePos p = lattice_rows<FW_ROWS>(0, blockIdx.x);
    const int i = p.i, j0 = p.j0;
    WobbleWalk<R> w;
    w.field = field, w.m = m, w.out = out, w.pline = &pline[0][threadIdx.x], w.removed_bits = removed_bits, w.unfit = unfit, w.wt = wt;
    w.active = i < fh && j0 < fw, w.two = j0 + 1 < fw;   // (a row of odd width: its last lane holds one node)
    w.node = w.active ? ((size_t)i * fw + j0) * 2 : 0, w.frame_stride = (size_t)fh * fw * 2;
    w.v = (double)i * sv - 1.0, w.u0 = (double)j0 * su - 1.0, w.u1 = (double)(j0 + 1) * su - 1.0;
    w.half_w = half_w, w.half_h = half_h, w.n = n, w.lane = p.lane;
    w.t0 = (int)blockIdx.z * FW_L;
    w.steps = (min(n, w.t0 + FW_L) - w.t0) + 2 * R;   // input frames t0 - R .. t1 - 1 + R, one per step; step q >= 2R also writes frame t0 + q - 2R
    w.wfull = 0.f;   // W where every tap is usable: the same ascending fp32 sum
#pragma unroll
    for (int k = -R; k <= R; ++k) w.wfull += wt.g[k < 0 ? -k : k];
#pragma unroll
    for (int s = 0; s < RING; ++s) w.e[s][0] = w.e[s][1] = w.e[s][2] = w.e[s][3] = 0.f;
    w.use0 = w.use1 = 0u, w.pw = 0;
    for (int base = 0; base < w.steps; base += RING) w.round(base, std::make_integer_sequence<int, RING>{});
}

template <int R>
void launch_wobble(dim3 grid, hipStream_t st, const float *field, const double *m, float *out, int n, int fh, int fw, const WobbleWeights &wt,
                   double su, double sv, float half_w, float half_h, int *removed_bits, int *unfit) {
    hipLaunchKernelGGL(field_wobble_kernel<R>, grid, dim3(kWave * FW_ROWS), 0, st, field, m, out, n, fh, fw, wt, su, sv, half_w, half_h,
                       removed_bits, unfit);
}

}  // namespace
}  // namespace pws

using namespace pws;

extern "C" int pws_field_wobble(const float *field, int n, int fh, int fw, const double *m, double sigma, int h0, int w0, float *out,
                                float *removed, int *unfit, pws_stream_t stream) {
    const char *who = "pws_field_wobble";
    if (int rc = lattice_shape(who, n, fh, fw)) return rc;
    PWS_REQUIRE(h0 >= 1 && w0 >= 1, "pws_field_wobble: bad frame size %d x %d", w0, h0);
    PWS_REQUIRE(sigma > 0.0 && sigma <= 5.0, "pws_field_wobble: sigma must lie in (0, 5] frames, got %g", sigma);   // (false for NaN)
    if (n == 0) return PWS_OK;
    if (int rc = lattice_pointers(who, field && m && out, addr(field) | addr(out) | addr(m), addr(removed) | addr(unfit),
                                  "field, out and m must be 8-byte aligned, removed and unfit 4-byte aligned"))
        return rc;
    if (int rc = lattice_overlap(who, field, out, n, fh, fw, false,
                                 "out must not overlap field (the filter reads neighbouring frames: it cannot run in place)"))
        return rc;
    const unsigned nseg = (unsigned)((n + FW_L - 1) / FW_L);
    unsigned nrg, chunks;
    if (int rc = lattice_grid(who, fh, fw, FW_ROWS, 1, nseg, "scene", nrg, chunks)) return rc;
    if (int rc = lattice_clear(who, "the statistics", (size_t)n * 4, as_stream(stream), removed, unfit)) return rc;
    const int R = (int)std::ceil(3.0 * sigma);   // 1 .. 15
    WobbleWeights wt;
    for (int k = 0; k <= FW_MAX_R; ++k) wt.g[k] = k <= R ? (float)std::exp(-(double)(k * k) / (2.0 * sigma * sigma)) : 0.f;
    double su, sv;
    node_scale(fh, fw, h0, w0, &su, &sv);
    const dim3 grid(nrg, chunks, nseg);
    const float half_w = 0.5f * (float)w0, half_h = 0.5f * (float)h0;
    int *const rb = reinterpret_cast<int *>(removed);
    const hipStream_t st = as_stream(stream);
#define PWS_WOBBLE_CASE(r) \
    case r: launch_wobble<r>(grid, st, field, m, out, n, fh, fw, wt, su, sv, half_w, half_h, rb, unfit); break;
    switch (R) {
        PWS_WOBBLE_CASE(1) PWS_WOBBLE_CASE(2) PWS_WOBBLE_CASE(3) PWS_WOBBLE_CASE(4) PWS_WOBBLE_CASE(5)
        PWS_WOBBLE_CASE(6) PWS_WOBBLE_CASE(7) PWS_WOBBLE_CASE(8) PWS_WOBBLE_CASE(9) PWS_WOBBLE_CASE(10)
        PWS_WOBBLE_CASE(11) PWS_WOBBLE_CASE(12) PWS_WOBBLE_CASE(13) PWS_WOBBLE_CASE(14) PWS_WOBBLE_CASE(15)
        default:
            set_error("pws_field_wobble: radius %d out of range", R);
            return PWS_EINVAL;
    }
#undef PWS_WOBBLE_CASE
    return check_launch("field_wobble_kernel");
}
