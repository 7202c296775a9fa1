// Bicubic twins of the fused "resize the field to the plane and warp" kernels of grid_sample.hip: Keys cubic convolution with A = -0.75,
// torch's F.grid_sample(mode="bicubic"), for fp32 NCHW frames, BGR bytes, NV12 / I420 and P010 / I010.
//
// Definition (restated in tests/bicubic_ref.py).  The field is resized to the plane's own size (align_corners=True) and un-normalised with the
// operations of the bilinear kernels (warp_common.h), so both interpolations sample at the same (ix, iy).  x0 = floor(ix), t = ix - x0, the
// weights of columns x0-1 .. x0+2 are [c2(t+1), c1(t), c1(1-t), c2(2-t)] with c1(s) = ((A+2)s - (A+3))s^2 + 1, c2(s) = ((As - 5A)s + 8A)s - 4A,
// rows alike; out = pad + sum_i wy_i sum_j wx_j (v_ij - pad), a tap outside the plane contributing nothing (it reads `pad`: 0 for float and
// BGR, BT.601 black for YUV), so a pixel whose 16 taps all lie outside is `pad` exactly.  Integer outputs are clamped to the format's range
// (a cubic overshoots) and then truncated, the byte paths' rule.
//
// Launch shape of the byte kernels: that of their twins -- a wave owns 256 consecutive pixels of ONE plane row, a lane 4 of them; row, sample,
// plane and the field's row pair are wave-uniform; consecutive row groups stay on one XCD.  A pixel's 4 taps of one row are 4 adjacent samples:
// ONE aligned load of the dwords they start in plus the next one, and v_alignbyte (BGR: 12 bytes at any byte offset, a 16-byte load; 8-bit Y
// and I420 chroma: 4 bytes, 8; NV12 UV and 10-bit Y / I010 chroma: 8 bytes, 12; P010 UV: 16 bytes at a 4-byte offset, exactly those) -- 16
// vector memory instructions per lane and plane, the count that bounds these launches (profiles/r06_warp_u8_rewrite.txt).  The window of 4
// columns is clamped into the plane (v_med3_i32) and the weights follow it: window column k takes the weight of the tap that lands on it, or
// zero; rows are clamped one by one and an outside row's weight is zero.  Addresses are therefore inside the plane whatever the coordinate.
// A wave whose lanes' 4 x 4 footprints are all inside skips clamps and selects (wave-uniform branch).  The aligned loads read up to 4 bytes
// behind a window: only in the last rows of the LAST sample can those lie outside the caller's buffer, and a wave of that sample in which some
// lane would read there takes exact 4-byte loads instead.
#include "common.h"
#include "warp_common.h"

namespace pws {
namespace bic {

constexpr int PLANE_BGR = 3;   // (beside yuv::PLANE_Y / PLANE_NV12_UV / PLANE_I420_UV)
constexpr float A = -0.75f;

__device__ __forceinline__ float c1(float s) { return ((A + 2.f) * s - (A + 3.f)) * s * s + 1.f; }
__device__ __forceinline__ float c2(float s) { return ((A * s - 5.f * A) * s + 8.f * A) * s - 4.f * A; }
__device__ __forceinline__ void weights(float t, float w[4]) {   // (torch's order of operations: 2 - t as (1 - t) + 1)
    const float u = 1.f - t;
    w[0] = c2(t + 1.f), w[1] = c1(t), w[2] = c1(u), w[3] = c2(u + 1.f);
}

// One pixel's source: first column / row of the 4 x 4 footprint (x0 - 1, y0 - 1) and the weights.  floor(ix) is clamped to [-4, size + 4] before
// the conversion: from -3 down and from size + 1 up every tap is outside anyway, and a huge coordinate cannot overflow the integer.
struct Foot {
    int xm, ym;
    float wx[4], wy[4];
};
__device__ __forceinline__ Foot make_foot(float ix, float iy, int H, int W) {
    Foot f;
    const float fx = floorf(ix), fy = floorf(iy);
    weights(ix - fx, f.wx), weights(iy - fy, f.wy);
    f.xm = (int)__builtin_amdgcn_fmed3f(fx, -4.f, (float)(W + 4)) - 1;
    f.ym = (int)__builtin_amdgcn_fmed3f(fy, -4.f, (float)(H + 4)) - 1;
    return f;
}
// Border form: the window's first column xs = clamp(xm, 0, W - 4) (W >= 4); window column k holds tap k + xs - xm, or no tap of this pixel.
__device__ __forceinline__ int clamp_window(Foot &f, int W) {
    const int xs = med3_i32(f.xm, W - 4), d = xs - f.xm;
    float w[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int j = k + d;
        w[k] = j == 0 ? f.wx[0] : (j == 1 ? f.wx[1] : (j == 2 ? f.wx[2] : (j == 3 ? f.wx[3] : 0.f)));
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) f.wx[k] = w[k];
    return xs;
}

typedef unsigned U32x4u __attribute__((ext_vector_type(4), aligned(4)));   // 16 / 12 / 8 bytes at dword alignment
typedef unsigned U32x3u __attribute__((ext_vector_type(3), aligned(4)));
typedef unsigned U32x2u __attribute__((ext_vector_type(2), aligned(4)));
typedef float F32x4u __attribute__((ext_vector_type(4), aligned(4)));

// the ND dwords that start at byte offset o of `base` (a 4-byte aligned address): NL = ND + 1 aligned dwords and v_alignbyte, or -- EXACT --
// ND 4-byte loads at byte alignment, which read nothing behind the window
template <int ND, bool EXACT>
__device__ __forceinline__ void load_window(const unsigned char *__restrict__ base, unsigned o, unsigned d[ND]) {
    if constexpr (EXACT) {
#pragma unroll
        for (int k = 0; k < ND; ++k) d[k] = reinterpret_cast<const U8x4 *>(base + o + 4 * k)->v;
    } else if constexpr (ND == 4) {   // P010 UV: o is a multiple of 4
        const U32x4u t = *reinterpret_cast<const U32x4u *>(base + o);
        d[0] = t.x, d[1] = t.y, d[2] = t.z, d[3] = t.w;
    } else {
        unsigned a[ND + 1];
        const unsigned char *p = base + (o & ~3u);
        if constexpr (ND == 3) {
            const U32x4u t = *reinterpret_cast<const U32x4u *>(p);
            a[0] = t.x, a[1] = t.y, a[2] = t.z, a[3] = t.w;
        } else if constexpr (ND == 2) {
            const U32x3u t = *reinterpret_cast<const U32x3u *>(p);
            a[0] = t.x, a[1] = t.y, a[2] = t.z;
        } else {
            const U32x2u t = *reinterpret_cast<const U32x2u *>(p);
            a[0] = t.x, a[1] = t.y;
        }
#pragma unroll
        for (int k = 0; k < ND; ++k) d[k] = __builtin_amdgcn_alignbyte(a[k + 1], a[k], o);   // (shifts by the low two bits of o)
    }
}

// One wave's row chunk of one plane kind.  SB: bytes per sample (1; 2 for P010 / I010, whose LAYOUT is 0 / 1); NCI: interleaved channels of a
// pixel (BGR 3, NV12 / P010 chroma 2); NP: source planes (I420 / I010 chroma 2).  fmode: yuv_field4's field access (wave-uniform).
template <int KIND, int SB, int LAYOUT, bool SWAP>
__device__ __forceinline__ void warp_row(const unsigned char *__restrict__ frame, unsigned char *__restrict__ ofr, const float *__restrict__ field,
                                         const yuv::Plane &P, int fmode, unsigned n, unsigned oy, int ox0, int fh, int fw, unsigned fbytes,
                                         bool last_sample) {
    constexpr int NCI = KIND == PLANE_BGR ? 3 : (KIND == yuv::PLANE_NV12_UV ? 2 : 1), NP = KIND == yuv::PLANE_I420_UV ? 2 : 1;
    constexpr int ND = NCI * SB, NL = ND == 4 ? 4 : ND + 1, NCH = NCI * NP;
    constexpr float PAD = KIND == PLANE_BGR ? 0.f : (KIND == yuv::PLANE_Y ? 16.f : 128.f) * (SB == 2 ? 4.f : 1.f);   // BT.601 black
    const int H = P.h, W = P.w;
    if (fmode < 2 && ox0 >= W) return;   // (modes 2 / 3: every lane fetches and serves field columns first)
    f32x2 gx[2], gy[2];
    if (fmode == 2) yuv_field4<2>(field, n, oy, ox0, W - 1, fh, fw, P.ry, P.rx, gx, gy);
    else if (fmode == 3) yuv_field4<3>(field, n, oy, ox0, W - 1, fh, fw, P.ry, P.rx, gx, gy);
    else yuv_field4<0>(field, n, oy, ox0, W - 1, fh, fw, P.ry, P.rx, gx, gy);
    if (ox0 >= W) return;
    Foot f[4];
    bool inner = true;   // this lane's 4 footprints lie inside the plane
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const float g0 = i & 1 ? gx[i >> 1].y : gx[i >> 1].x, g1 = i & 1 ? gy[i >> 1].y : gy[i >> 1].x;
        f[i] = make_foot(fmaf(g0, P.kx, P.kx1), fmaf(g1, P.ky, P.ky1), H, W);   // (the twins' pk_fma, per component)
        inner = inner && (unsigned)f[i].xm <= (unsigned)(W - 4) && (unsigned)f[i].ym <= (unsigned)(H - 4);
    }
    unsigned off[4][4];   // [row][pixel]: byte offset of the window from the frame's start (first source plane)
    if (H >= 4 && __builtin_amdgcn_ballot_w64(!inner) == 0) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            off[0][i] = P.off0 + __umul24((unsigned)f[i].ym, P.pitch) + (unsigned)f[i].xm * ND;
#pragma unroll
            for (int r = 1; r < 4; ++r) off[r][i] = off[r - 1][i] + P.pitch;
        }
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const unsigned xb = P.off0 + (unsigned)clamp_window(f[i], W) * ND;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int y = f[i].ym + r;
                f[i].wy[r] = (unsigned)y < (unsigned)H ? f[i].wy[r] : 0.f;
                off[r][i] = xb + __umul24((unsigned)med3_i32(y, H - 1), P.pitch);
            }
        }
    }
    bool exact = false;
    if (NL > ND && last_sample) {
        unsigned m = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) m = max(m, off[3][i] + (NP == 2 ? P.off1 - P.off0 : 0u));   // (row 3 of a pixel is never above its others)
        exact = __builtin_amdgcn_ballot_w64((m & ~3u) + 4u * NL > fbytes) != 0;
    }
    float acc[NCH][4];
#pragma unroll
    for (int ch = 0; ch < NCH; ++ch)
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[ch][i] = 0.f;
#pragma unroll
    for (int p = 0; p < NP; ++p) {
        const unsigned shift = p ? P.off1 - P.off0 : 0u;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            unsigned d[4][ND];
            if (!exact) {
#pragma unroll
                for (int i = 0; i < 4; ++i) load_window<ND, false>(frame, off[r][i] + shift, d[i]);
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i) load_window<ND, true>(frame, off[r][i] + shift, d[i]);
            }
#pragma unroll
            for (int c = 0; c < NCI; ++c) {
                const int ci = SWAP ? NCI - 1 - c : c;   // (BGR only) output channel c samples input channel 2 - c
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    float s = 0.f;
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const int e = k * NCI + ci;   // sample k, channel ci of the window: byte (SB 1) or 16-bit half (SB 2) e
                        float v;
                        if constexpr (SB == 1) v = (float)((d[i][e >> 2] >> (8 * (e & 3))) & 0xffu);
                        else v = yuv::sample10f<LAYOUT>(d[i][e >> 1], e & 1);
                        s = k == 0 ? f[i].wx[0] * (v - PAD) : fmaf(f[i].wx[k], v - PAD, s);
                    }
                    acc[NP == 2 ? p : c][i] = fmaf(f[i].wy[r], s, acc[NP == 2 ? p : c][i]);
                }
            }
        }
    }
    // clamp, truncate, store: the twins' stores
    const bool full = ox0 + 4 <= W;   // chroma rows of width 2 mod 4: the row's last lane owns 2 pixels
    const unsigned ob = P.off0 + oy * P.pitch + (unsigned)ox0 * ND;
    if constexpr (SB == 1) {
        unsigned ow[NCH] = {};
#pragma unroll
        for (int ch = 0; ch < NCH; ++ch)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int b = NP == 2 ? i : i * NCI + ch;   // byte inside the lane's output bytes of this plane (compile-time)
                cvt_u8_into(b & 3, ow[NP == 2 ? ch : b >> 2], fminf(acc[ch][i] + PAD, 255.f));   // (the conversion saturates at 0 and truncates)
            }
        if constexpr (KIND == PLANE_BGR) {
            unsigned *o = reinterpret_cast<unsigned *>(ofr + ob);   // 12 bytes, 4-byte aligned (w % 4 == 0)
            o[0] = ow[0], o[1] = ow[1], o[2] = ow[2];
        } else if constexpr (KIND == yuv::PLANE_Y) {
            *reinterpret_cast<unsigned *>(ofr + ob) = ow[0];
        } else if constexpr (KIND == yuv::PLANE_NV12_UV) {
            unsigned *o = reinterpret_cast<unsigned *>(ofr + ob);
            o[0] = ow[0];
            if (full) o[1] = ow[1];
        } else {
#pragma unroll
            for (int p = 0; p < 2; ++p) {
                unsigned char *o = ofr + ob + (p ? P.off1 - P.off0 : 0u);   // (2-byte aligned only at 4:2:0: the V plane starts at h w + h w / 4; 4 at 4:2:2 / 4:4:4, not relied on)
                if (full) reinterpret_cast<U8x4 *>(o)->v = ow[p];
                else reinterpret_cast<U8x2 *>(o)->v = (unsigned short)ow[p];
            }
        }
    } else {
        unsigned res[NCH][4];
#pragma unroll
        for (int ch = 0; ch < NCH; ++ch)
#pragma unroll
            for (int i = 0; i < 4; ++i) res[ch][i] = yuv::place10<LAYOUT>(fmaxf(acc[ch][i] + PAD, 0.f));   // (place10 clamps at 1023)
        if constexpr (KIND == yuv::PLANE_Y) {
            *reinterpret_cast<uint2 *>(ofr + ob) = uint2{res[0][0] | res[0][1] << 16, res[0][2] | res[0][3] << 16};   // (8-byte aligned: w % 4 == 0)
        } else if constexpr (KIND == yuv::PLANE_NV12_UV) {
            const unsigned w0 = res[0][0] | res[1][0] << 16, w1 = res[0][1] | res[1][1] << 16;
            if (full) *reinterpret_cast<yuv::U32x4 *>(ofr + ob) = yuv::U32x4{w0, w1, res[0][2] | res[1][2] << 16, res[0][3] | res[1][3] << 16};
            else *reinterpret_cast<yuv::U32x2 *>(ofr + ob) = yuv::U32x2{w0, w1};
        } else {
#pragma unroll
            for (int p = 0; p < 2; ++p) {
                unsigned char *o = ofr + ob + (p ? P.off1 - P.off0 : 0u);   // (4-byte aligned: the chroma planes' pitch and size are multiples of 4 bytes, at every subsampling)
                const unsigned w0 = res[p][0] | res[p][1] << 16;
                if (full) *reinterpret_cast<yuv::U32x2 *>(o) = yuv::U32x2{w0, res[p][2] | res[p][3] << 16};
                else *reinterpret_cast<unsigned *>(o) = w0;
            }
        }
    }
}

template <bool SWAP>
__global__ void __launch_bounds__(256) bicubic_u8_kernel(const unsigned char *__restrict__ input, const float *__restrict__ field,
                                                         unsigned char *__restrict__ out, yuv::Plane P, int fmode, int fh, int fw, unsigned fbytes) {
    const unsigned rg = xcd_remap(blockIdx.x, gridDim.x);
    const unsigned oy = __builtin_amdgcn_readfirstlane(rg * 4u + (threadIdx.x >> 6));
    const unsigned n = blockIdx.z;
    if (rg >= P.nrg || oy >= (unsigned)P.h) return;
    const int ox0 = (int)(blockIdx.y * 256u + (threadIdx.x & 63u) * 4u);
    warp_row<PLANE_BGR, 1, 0, SWAP>(input + (size_t)n * fbytes, out + (size_t)n * fbytes, field, P, fmode, n, oy, ox0, fh, fw, fbytes,
                                    n + 1 == gridDim.z);
}

template <int SB, int LAYOUT>   // SB 1: LAYOUT 0 NV12, 1 I420; SB 2: 0 P010, 1 I010
__global__ void __launch_bounds__(256) bicubic_yuv420_kernel(const unsigned char *__restrict__ input, const float *__restrict__ field,
                                                             unsigned char *__restrict__ out, yuv::Plane py, yuv::Plane pc, int fmy, int fmc, int fh,
                                                             int fw, unsigned fbytes) {
    const unsigned rg = xcd_remap(blockIdx.x, gridDim.x);
    const unsigned n = blockIdx.z;
    const int ox0 = (int)(blockIdx.y * 256u + (threadIdx.x & 63u) * 4u);
    const unsigned char *frame = input + (size_t)n * fbytes;
    unsigned char *ofr = out + (size_t)n * fbytes;
    const bool last = n + 1 == gridDim.z;
    if (rg < py.nrg) {
        const unsigned oy = __builtin_amdgcn_readfirstlane(rg * 4u + (threadIdx.x >> 6));
        if (oy >= (unsigned)py.h || blockIdx.y * 256u >= (unsigned)py.w) return;
        warp_row<yuv::PLANE_Y, SB, LAYOUT, false>(frame, ofr, field, py, fmy, n, oy, ox0, fh, fw, fbytes, last);
    } else if (rg < py.nrg + pc.nrg) {
        const unsigned oy = __builtin_amdgcn_readfirstlane((rg - py.nrg) * 4u + (threadIdx.x >> 6));
        if (oy >= (unsigned)pc.h || blockIdx.y * 256u >= (unsigned)pc.w) return;
        warp_row<LAYOUT == 0 ? yuv::PLANE_NV12_UV : yuv::PLANE_I420_UV, SB, LAYOUT, false>(frame, ofr, field, pc, fmc, n, oy, ox0, fh, fw, fbytes, last);
    }
}

// fp32 NCHW: the bilinear twin's mapping (a lane owns PPT consecutive pixels of a row, the field's four corners per pixel, scalar field_lerp);
// a row's 4 taps are ONE 16-byte load at dword alignment (the window is clamped into the plane, so nothing is read outside it).
template <int PPT>
__global__ void __launch_bounds__(256) bicubic_fwd_kernel(const float *__restrict__ input, const float *__restrict__ field, float *__restrict__ out,
                                                          int C, int H, int W, int fh, int fw, float ry, float rx, size_t total_groups,
                                                          unsigned nblocks, int ac) {
    const unsigned blk = xcd_remap(blockIdx.x, nblocks);
    const size_t gidx = (size_t)blk * 256 + threadIdx.x;
    if (gidx >= total_groups) return;
    const int HW = H * W;
    const size_t p0 = gidx * PPT;
    const int n = (int)(p0 / HW);
    const int hw = (int)(p0 % HW);
    const int oy = hw / W, ox0 = hw % W;  // W % PPT == 0: the group stays inside one row
    const float sy = mul_rounded(ry, (float)oy);
    const int y0 = (int)sy, y1 = y0 + (y0 < fh - 1 ? 1 : 0);
    const float ly = sy - y0, hy = 1.f - ly;
    const float2 *f0 = reinterpret_cast<const float2 *>(field) + ((size_t)n * fh + y0) * fw;
    const float2 *f1 = reinterpret_cast<const float2 *>(field) + ((size_t)n * fh + y1) * fw;
    Foot f[PPT];
    int ro[PPT][4];   // offsets of the four windows inside a channel plane
#pragma unroll
    for (int i = 0; i < PPT; ++i) {
        const float sx = mul_rounded(rx, (float)(ox0 + i));
        const int x0 = (int)sx, x1 = x0 + (x0 < fw - 1 ? 1 : 0);
        const float lx = sx - x0, hx = 1.f - lx;
        const float2 a = f0[x0], b = f0[x1], c = f1[x0], d = f1[x1];
        const float gx = field_lerp(hy, ly, hx, lx, a.x, b.x, c.x, d.x);
        const float gy = field_lerp(hy, ly, hx, lx, a.y, b.y, c.y, d.y);
        f[i] = make_foot(unnormalize(gx, W, ac != 0), unnormalize(gy, H, ac != 0), H, W);
        const int xs = min(max(f[i].xm, 0), W - 4), dlt = xs - f[i].xm;
        float w[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int j = k + dlt;
            w[k] = j == 0 ? f[i].wx[0] : (j == 1 ? f[i].wx[1] : (j == 2 ? f[i].wx[2] : (j == 3 ? f[i].wx[3] : 0.f)));
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) f[i].wx[k] = w[k];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int y = f[i].ym + r;
            f[i].wy[r] = (unsigned)y < (unsigned)H ? f[i].wy[r] : 0.f;
            ro[i][r] = min(max(y, 0), H - 1) * W + xs;
        }
    }
    for (int c = 0; c < C; ++c) {
        const float *ip = input + ((size_t)n * C + c) * HW;
        float r_[PPT];
#pragma unroll
        for (int i = 0; i < PPT; ++i) {
            float acc = 0.f;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const F32x4u v = *reinterpret_cast<const F32x4u *>(ip + ro[i][r]);
                const float s = fmaf(f[i].wx[3], v.w, fmaf(f[i].wx[2], v.z, fmaf(f[i].wx[1], v.y, f[i].wx[0] * v.x)));
                acc = fmaf(f[i].wy[r], s, acc);
            }
            r_[i] = acc;
        }
        float *op = out + ((size_t)n * C + c) * HW + hw;
        if constexpr (PPT == 4) {
            *reinterpret_cast<f32x4 *>(op) = f32x4{r_[0], r_[1], r_[2], r_[3]};
        } else {
#pragma unroll
            for (int i = 0; i < PPT; ++i) op[i] = r_[i];
        }
    }
}

}  // namespace bic
}  // namespace pws

using namespace pws;

extern "C" int pws_upsample_grid_sample_bicubic_fwd(const float *input, const float *field, float *out, int n, int c, int h, int w, int fh,
                                                    int fw, int align_corners, pws_stream_t stream) {
    PWS_REQUIRE(n >= 0 && c > 0 && h > 0 && w > 0 && fh > 0 && fw > 0, "pws_upsample_grid_sample_bicubic_fwd: bad shape");
    if (n == 0) return PWS_OK;
    PWS_REQUIRE(input && field && out, "pws_upsample_grid_sample_bicubic_fwd: NULL pointer");
    PWS_REQUIRE((size_t)h * w < (1u << 31) && w >= 4, "pws_upsample_grid_sample_bicubic_fwd: plane too large or w < 4 (the 4-tap window)");
    const float ry = h > 1 ? (float)(fh - 1) / (float)(h - 1) : 0.f;
    const float rx = w > 1 ? (float)(fw - 1) / (float)(w - 1) : 0.f;
    const size_t total = (size_t)n * h * w;
    ProfScope prof(KID_UPSAMPLE_GRID_SAMPLE_FWD, (double)total * (80.0 + 40.0 * c), (double)total * 8.0 * c + 8.0 * (double)n * fh * fw,
                   as_stream(stream));
    if (w % 4 == 0 && (reinterpret_cast<size_t>(out) & 15) == 0) {
        const size_t groups = total / 4;
        const unsigned nb = (unsigned)((groups + 255) / 256);
        hipLaunchKernelGGL(bic::bicubic_fwd_kernel<4>, dim3(nb), dim3(256), 0, as_stream(stream), input, field, out, c, h, w, fh, fw, ry, rx,
                           groups, nb, align_corners);
    } else {
        const unsigned nb = (unsigned)((total + 255) / 256);
        hipLaunchKernelGGL(bic::bicubic_fwd_kernel<1>, dim3(nb), dim3(256), 0, as_stream(stream), input, field, out, c, h, w, fh, fw, ry, rx,
                           total, nb, align_corners);
    }
    return check_launch("bicubic_fwd_kernel");
}

extern "C" int pws_upsample_grid_sample_bicubic_u8(const unsigned char *frame_hwc, const float *field, unsigned char *out_hwc, int n, int h,
                                                   int w, int fh, int fw, int swap_rb, int align_corners, pws_stream_t stream) {
    PWS_REQUIRE(n >= 0 && h > 0 && w > 0 && fh > 0 && fw > 0, "pws_upsample_grid_sample_bicubic_u8: bad shape");
    if (n == 0) return PWS_OK;
    PWS_REQUIRE(frame_hwc && field && out_hwc, "pws_upsample_grid_sample_bicubic_u8: NULL pointer");
    PWS_REQUIRE((size_t)h * w < (1u << 29) && w >= 4 && w % 4 == 0, "pws_upsample_grid_sample_bicubic_u8: w must be a multiple of 4 (got %d)", w);
    PWS_REQUIRE((reinterpret_cast<size_t>(out_hwc) & 3) == 0, "pws_upsample_grid_sample_bicubic_u8: out must be 4-byte aligned");
    const unsigned cpr = (unsigned)((w + 255) / 256);
    PWS_REQUIRE(n < 65536 && cpr < 65536 && (size_t)w * 3 < (1u << 24) && h < (1 << 24), "pws_upsample_grid_sample_bicubic_u8: frame or batch too large");
    const yuv::Plane P = yuv::make_plane(h, w, 0u, 0u, 3u * (unsigned)w, fh, fw, align_corners);
    const unsigned gx = (P.nrg + 7u) & ~7u, fbytes = (unsigned)((size_t)h * w * 3);
    const int fmode = yuv_fmode(P.rx);
    const size_t total = (size_t)n * h * w;
    ProfScope prof(KID_UPSAMPLE_GRID_SAMPLE_U8, (double)total * (80.0 + 40.0 * 3), (double)total * 6.0 + 8.0 * (double)n * fh * fw,
                   as_stream(stream));
    if (swap_rb)
        hipLaunchKernelGGL(bic::bicubic_u8_kernel<true>, dim3(gx, cpr, (unsigned)n), dim3(256), 0, as_stream(stream), frame_hwc, field, out_hwc, P,
                           fmode, fh, fw, fbytes);
    else
        hipLaunchKernelGGL(bic::bicubic_u8_kernel<false>, dim3(gx, cpr, (unsigned)n), dim3(256), 0, as_stream(stream), frame_hwc, field, out_hwc, P,
                           fmode, fh, fw, fbytes);
    return check_launch("bicubic_u8_kernel");
}

// SB: bytes per sample; chroma: 0 4:2:0, 1 4:2:2, 2 4:4:4.  Checks and plane geometry are the twins' (yuv::launch_yuv).  On top: a chroma
// plane holds the 4-column window (clamp_window: W >= 4), which is w >= 8 at 4:2:0 and 4:2:2 and w >= 4 -- any valid w -- at 4:4:4; plane
// heights below 4 take the clamped branch of warp_row (H >= 4 is tested there), so 4:2:2's and 4:4:4's taller chroma planes change nothing.
template <int SB>
static int bicubic_yuv(const char *what, const void *frames, const float *field, void *out, int n, int h, int w, int fh, int fw, int layout,
                       int chroma, int align_corners, pws_stream_t stream) {
    yuv::LaunchYuv L;
    const int rc = yuv::launch_yuv<SB>(what, frames, field, out, "out", n, h, w, fh, fw, layout, chroma, align_corners, 4,
                                       "(the chroma planes hold the 4-tap window)", L);
    if (rc != PWS_OK || n == 0) return rc;
    const size_t total = (size_t)n * h * w;
    ProfScope prof(KID_UPSAMPLE_GRID_SAMPLE_U8, (double)total * L.spp * (80.0 + 40.0), (double)total * 2.0 * L.spp * SB + 8.0 * (double)n * fh * fw,
                   as_stream(stream));
    const unsigned char *src = reinterpret_cast<const unsigned char *>(frames);
    unsigned char *dst = reinterpret_cast<unsigned char *>(out);
    if (layout == 0)
        hipLaunchKernelGGL((bic::bicubic_yuv420_kernel<SB, 0>), dim3(L.gx, L.cpr, (unsigned)n), dim3(256), 0, as_stream(stream), src, field, dst, L.py, L.pc,
                           L.fmy, L.fmc, fh, fw, L.fbytes);
    else
        hipLaunchKernelGGL((bic::bicubic_yuv420_kernel<SB, 1>), dim3(L.gx, L.cpr, (unsigned)n), dim3(256), 0, as_stream(stream), src, field, dst, L.py, L.pc,
                           L.fmy, L.fmc, fh, fw, L.fbytes);
    return check_launch("bicubic_yuv420_kernel");
}

extern "C" int pws_upsample_grid_sample_bicubic_yuv420_u8(const unsigned char *frames, const float *field, unsigned char *out, int n, int h, int w,
                                                          int fh, int fw, int layout, int align_corners, pws_stream_t stream) {
    return bicubic_yuv<1>("pws_upsample_grid_sample_bicubic_yuv420_u8", frames, field, out, n, h, w, fh, fw, layout, 0, align_corners, stream);
}

extern "C" int pws_upsample_grid_sample_bicubic_yuv_u8(const unsigned char *frames, const float *field, unsigned char *out, int n, int h, int w,
                                                       int fh, int fw, int layout, int chroma, int align_corners, pws_stream_t stream) {
    return bicubic_yuv<1>("pws_upsample_grid_sample_bicubic_yuv_u8", frames, field, out, n, h, w, fh, fw, layout, chroma, align_corners, stream);
}

extern "C" int pws_upsample_grid_sample_bicubic_yuv420_u16(const unsigned short *frames, const float *field, unsigned short *out, int n, int h, int w,
                                                           int fh, int fw, int layout, int align_corners, pws_stream_t stream) {
    return bicubic_yuv<2>("pws_upsample_grid_sample_bicubic_yuv420_u16", frames, field, out, n, h, w, fh, fw, layout, 0, align_corners, stream);
}

extern "C" int pws_upsample_grid_sample_bicubic_yuv_u16(const unsigned short *frames, const float *field, unsigned short *out, int n, int h, int w,
                                                        int fh, int fw, int layout, int chroma, int align_corners, pws_stream_t stream) {
    return bicubic_yuv<2>("pws_upsample_grid_sample_bicubic_yuv_u16", frames, field, out, n, h, w, fh, fw, layout, chroma, align_corners, stream);
}
