// What the bilinear warp kernels (grid_sample.hip) and the bicubic ones (warp_bicubic.hip) share, so that both form a pixel's source
// position (ix, iy) with the same fp32 operations: the field's interpolation (mul_rounded of common.h, field_lerp / pk_field_lerp and the
// wave-shared fetch yuv_field4), the un-normalisation, the plane geometry of packed 4:2:0 / 4:2:2 / 4:4:4 frames with the launchers' shared checks (yuv::make_plane,
// yuv::launch_yuv), and the byte / 10-bit conversions.
#pragma once
#include "common.h"

namespace pws {

__device__ __forceinline__ float unnormalize(float g, int size, bool align_corners) {
    // align_corners=False: ((g+1)*size-1)/2 ; True: (g+1)/2*(size-1) -- evaluated with one rounding
    return align_corners ? fmaf(g, 0.5f * (float)(size - 1), 0.5f * (float)(size - 1))
                         : fmaf(g, 0.5f * (float)size, 0.5f * (float)(size - 1));
}

// The field's bilinear interpolation with its roundings spelled out (one fma chain): left as a plain expression, hipcc contracted
// it differently in different instantiations of the kernels below, and a last-ulp difference of a coordinate flips a byte of the
// uint8 output where the blend lands on an integer.
__device__ __forceinline__ float field_lerp(float hy, float ly, float hx, float lx, float a, float b, float c, float d) {
    const float top = fmaf(lx, b, hx * a), bot = fmaf(lx, d, hx * c);
    return fmaf(ly, bot, hy * top);
}

struct __attribute__((packed, aligned(1))) U8x4 {
    unsigned v;
};
struct __attribute__((packed, aligned(1))) U8x2 {
    unsigned short v;
};
struct __attribute__((aligned(4))) U32x3 {
    unsigned x, y, z;
};
typedef float f32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ f32x2 pk_fma(f32x2 a, f32x2 b, f32x2 c) { return __builtin_elementwise_fma(a, b, c); }
__device__ __forceinline__ f32x2 pk_splat(float v) { return f32x2{v, v}; }
__device__ __forceinline__ f32x2 pk_floor(f32x2 v) { return f32x2{floorf(v.x), floorf(v.y)}; }
__device__ __forceinline__ f32x2 pk_mul_rounded(f32x2 a, f32x2 b) {   // (mul_rounded of common.h, two at a time)
    f32x2 p = a * b;
    asm volatile("" : "+v"(p));
    return p;
}
__device__ __forceinline__ f32x2 pk_field_lerp(f32x2 hy, f32x2 ly, f32x2 hx, f32x2 lx, f32x2 a, f32x2 b, f32x2 c, f32x2 d) {
    const f32x2 top = pk_fma(lx, b, hx * a), bot = pk_fma(lx, d, hx * c);   // field_lerp above, per component
    return pk_fma(ly, bot, hy * top);
}
// float -> byte B of `word`, truncating like astype(uint8) (the blend is in [0, 255.0001]; v_cvt_u32_f32 truncates and saturates at 0): one
// SDWA instruction converts and writes the byte in place.  (v_cvt_pk_u8_f32 rounds to NEAREST -- measured -- and would need a floor in front.)
__device__ __forceinline__ void cvt_u8_into(int B, unsigned &word, float v) {   // (B: a constant once the caller's loops are unrolled)
    if (B == 0) asm("v_cvt_u32_f32_sdwa %0, %1 dst_sel:BYTE_0 dst_unused:UNUSED_PRESERVE src0_sel:DWORD" : "+v"(word) : "v"(v));
    if (B == 1) asm("v_cvt_u32_f32_sdwa %0, %1 dst_sel:BYTE_1 dst_unused:UNUSED_PRESERVE src0_sel:DWORD" : "+v"(word) : "v"(v));
    if (B == 2) asm("v_cvt_u32_f32_sdwa %0, %1 dst_sel:BYTE_2 dst_unused:UNUSED_PRESERVE src0_sel:DWORD" : "+v"(word) : "v"(v));
    if (B == 3) asm("v_cvt_u32_f32_sdwa %0, %1 dst_sel:BYTE_3 dst_unused:UNUSED_PRESERVE src0_sel:DWORD" : "+v"(word) : "v"(v));
}

__device__ __forceinline__ int med3_i32(int x, int hi) {   // clamp to [0, hi], hi >= 0 and wave-uniform: one instruction (hipcc emits max + min)
    int r;
    asm("v_med3_i32 %0, %1, 0, %2" : "=v"(r) : "v"(x), "s"(hi));
    return r;
}

namespace yuv {
constexpr int PLANE_Y = 0, PLANE_NV12_UV = 1, PLANE_I420_UV = 2;
struct Plane {      // one plane kind's geometry inside a frame (byte offsets from the frame's start)
    int h, w;       // plane rows and pixels per row
    unsigned off0, off1, pitch;   // first (and for I420 chroma: second) source plane, row pitch in bytes
    float ry, rx, kx, kx1, ky, ky1;
    unsigned nrg;   // row groups of 4 rows
};
}  // namespace yuv

// the field at 4 consecutive pixels ox0 .. ox0+3 (clamped to the row) of plane row oy: the BGR kernel's arithmetic (its FMODE 0 and 2), plus
// FMODE 3 (the chroma planes of 1280-wide frames span up to 103 field columns per wave)
template <int FMODE>   // 0 four corners per pixel; 2 / 3 the wave's row pair, one / two columns per lane
__device__ __forceinline__ void yuv_field4(const float *__restrict__ field, unsigned n, unsigned oy, int ox0, int wlast, int fh, int fw,
                                           float ry, float rx, f32x2 gx[2], f32x2 gy[2]) {
    const float sy = mul_rounded(ry, (float)oy);
    const int y0 = __builtin_amdgcn_readfirstlane((int)sy), y1 = y0 + (y0 < fh - 1 ? 1 : 0);
    const float ly = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, sy - (float)y0))), hy = 1.f - ly;
    const float2 *f0 = reinterpret_cast<const float2 *>(field) + ((size_t)n * fh + y0) * fw;
    const float2 *f1 = reinterpret_cast<const float2 *>(field) + ((size_t)n * fh + y1) * fw;
    const f32x2 ly2 = pk_splat(ly), hy2 = pk_splat(hy), one2 = pk_splat(1.f);
    const float xl = (float)wlast;   // pixels past the row's end (chroma rows of width 2 mod 4) take the last pixel's field: never stored
    const float oxf = (float)ox0;
    const f32x2 px[2] = {f32x2{fminf(oxf, xl), fminf(oxf + 1.f, xl)}, f32x2{fminf(oxf + 2.f, xl), fminf(oxf + 3.f, xl)}};
    if constexpr (FMODE != 0) {
        f32x2 sx[2], fl[2];
        sx[0] = pk_mul_rounded(pk_splat(rx), px[0]), sx[1] = pk_mul_rounded(pk_splat(rx), px[1]);
        fl[0] = pk_floor(sx[0]), fl[1] = pk_floor(sx[1]);
        const unsigned cb = (unsigned)(int)fl[0].x;
        {
            // lane L holds field column c0 + L (FMODE 3: and c0 + 64 + L) of the row pair, clamped to the last column
            const unsigned c0 = __builtin_amdgcn_readfirstlane(cb);
            const unsigned lane = threadIdx.x & 63u, last = (unsigned)(fw - 1);
            const float2 a0 = f0[min(c0 + lane, last)], a1 = f1[min(c0 + lane, last)];
            float2 b0 = a0, b1 = a1;
            if constexpr (FMODE == 3) b0 = f0[min(c0 + 64u + lane, last)], b1 = f1[min(c0 + 64u + lane, last)];
            const int v[8] = {__builtin_bit_cast(int, a0.x), __builtin_bit_cast(int, a0.y), __builtin_bit_cast(int, a1.x), __builtin_bit_cast(int, a1.y),
                              __builtin_bit_cast(int, b0.x), __builtin_bit_cast(int, b0.y), __builtin_bit_cast(int, b1.x), __builtin_bit_cast(int, b1.y)};
            // value k (0: row 0 x, 1: row 0 y, 2: row 1 x, 3: row 1 y) of field column c0 + j (byte address 4 j)
            auto take = [&](int addr, int k) {
                const float lo = __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute(addr, v[k]));
                if constexpr (FMODE == 3) {
                    const float hi = __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute(addr, v[4 + k]));
                    return addr >= 256 ? hi : lo;
                }
                return lo;
            };
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                const f32x2 lx = sx[q] - fl[q], hx = one2 - lx;
                const int j0 = ((int)fl[q].x - (int)c0) * 4, j1 = ((int)fl[q].y - (int)c0) * 4;
                gx[q] = pk_field_lerp(hy2, ly2, hx, lx, f32x2{take(j0, 0), take(j1, 0)}, f32x2{take(j0 + 4, 0), take(j1 + 4, 0)},
                                      f32x2{take(j0, 2), take(j1, 2)}, f32x2{take(j0 + 4, 2), take(j1 + 4, 2)});
                gy[q] = pk_field_lerp(hy2, ly2, hx, lx, f32x2{take(j0, 1), take(j1, 1)}, f32x2{take(j0 + 4, 1), take(j1 + 4, 1)},
                                      f32x2{take(j0, 3), take(j1, 3)}, f32x2{take(j0 + 4, 3), take(j1 + 4, 3)});
            }
        }
    } else {
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const f32x2 sx = pk_mul_rounded(pk_splat(rx), px[q]);
            const f32x2 fl = pk_floor(sx), lx = sx - fl, hx = one2 - lx;
            const unsigned xa = (unsigned)(int)fl.x, xb = (unsigned)(int)fl.y;
            const unsigned xa1 = xa + ((int)xa < fw - 1 ? 1u : 0u), xb1 = xb + ((int)xb < fw - 1 ? 1u : 0u);
            const float2 a0 = f0[xa], b0 = f0[xa1], c0 = f1[xa], d0 = f1[xa1];
            const float2 a1 = f0[xb], b1 = f0[xb1], c1 = f1[xb], d1 = f1[xb1];
            gx[q] = pk_field_lerp(hy2, ly2, hx, lx, f32x2{a0.x, a1.x}, f32x2{b0.x, b1.x}, f32x2{c0.x, c1.x}, f32x2{d0.x, d1.x});
            gy[q] = pk_field_lerp(hy2, ly2, hx, lx, f32x2{a0.y, a1.y}, f32x2{b0.y, b1.y}, f32x2{c0.y, c1.y}, f32x2{d0.y, d1.y});
        }
    }
}

// field access mode for a plane of width w: 2 / 3 when a wave's 256 pixels touch at most 64 / 128 field columns, 1 when a lane's 4 touch
// (the BGR kernel's rule, plus the two-column mode for the chroma planes and 854-wide frames), else 0
static int yuv_fmode(float rx) {
    if (255.f * rx + 3.f <= 63.f) return 2;
    return 255.f * rx + 3.f <= 127.f ? 3 : 0;   // (the BGR kernel's FMODE 1, rx < 1/3, always meets one of these)
}

namespace yuv {
struct __attribute__((packed, aligned(2))) U16x2 {   // two samples at 2-byte alignment (the exact loads at the end of the last sample)
    unsigned v;
};
struct __attribute__((aligned(8))) U32x4 {           // 16 bytes at 8-byte alignment (P010 chroma rows: the pitch is 2 w bytes, a multiple of 8)
    unsigned x, y, z, w;
};
// 8 bytes at dword alignment (the tap pairs' loads, the I010 chroma store): uint2 would promise 8.  A vector type, not a struct: a struct's
// store is two member stores to the compiler, which it then shares between the `full` branches instead of pairing them into one dwordx2.
typedef unsigned U32x2 __attribute__((ext_vector_type(2), aligned(4)));
template <int LAYOUT>
__device__ __forceinline__ float sample10f(unsigned word, int half) {   // the 10-bit sample in 16-bit half `half` of a 32-bit word, as float
    const unsigned v = LAYOUT == 0 ? (word >> (16 * half + 6)) & 0x3ffu : min((word >> (16 * half)) & 0xffffu, 1023u);
    return (float)v;
}
template <int LAYOUT>
__device__ __forceinline__ unsigned place10(float blend) {   // truncate (the blend is >= 0), clamp to 10 bits, the layout's placement
    const unsigned v = min((unsigned)blend, 1023u);
    return LAYOUT == 0 ? v << 6 : v;
}

// ---- host side: the geometry of a plane, and what the launchers of the packed-YUV kernels (bilinear, bicubic, keep) check and derive alike
static Plane make_plane(int ph, int pw, unsigned off0, unsigned off1, unsigned pitch, int fh, int fw, int align_corners) {
    Plane p;   // (the field's resize ratios and the un-normalisation constants: every kernel gets the same fp32 products)
    p.h = ph, p.w = pw, p.off0 = off0, p.off1 = off1, p.pitch = pitch;
    p.ry = ph > 1 ? (float)(fh - 1) / (float)(ph - 1) : 0.f;
    p.rx = pw > 1 ? (float)(fw - 1) / (float)(pw - 1) : 0.f;
    p.kx = align_corners ? 0.5f * (float)(pw - 1) : 0.5f * (float)pw, p.kx1 = 0.5f * (float)(pw - 1);
    p.ky = align_corners ? 0.5f * (float)(ph - 1) : 0.5f * (float)ph, p.ky1 = 0.5f * (float)(ph - 1);
    p.nrg = (unsigned)((ph + 3) / 4);
    return p;
}

struct LaunchYuv {   // one launch over every plane of every frame: grid (gx, cpr, frames or 1), 256 threads
    Plane py, pc;
    unsigned fbytes, gx, cpr;   // bytes per frame, row groups of Y then chroma (padded to the 8 XCDs), 256-pixel chunks per Y row
    int fmy, fmc;               // field access mode of the Y / chroma planes
    double spp;                 // samples per pixel (1.5, 2, 3): what the callers' ProfScope books per pixel
};
// SB: bytes per sample (1: NV12 / I420 and their 4:2:2 / 4:4:4 kin, 2: P010 / I010 and theirs).  chroma: 0 4:2:0, 1 4:2:2, 2 4:4:4 -- the chroma
// planes are (h >> cy) x (w >> cx) samples, (cx, cy) = (1, 1), (1, 0), (0, 0).  `other`: the second frame pointer (`other_name`: "out" /
// "initial").  min_cw > 0: the caller's own minimum width of a CHROMA plane (the bicubic window: 4), asked of w as min_cw << cx, `min_w_why`
// the words after "w must be at least <that> ".  PWS_OK with n == 0 means: nothing to launch.
//
// What the row functions (yuv_warp_row, yuv16_warp_row, bic::warp_row, keep::keep_row) assume of a geometry, derived here for all three
// subsamplings from h even, w % 4 == 0 (so h w is a multiple of 8 and cw = w >> cx is even; cw is a multiple of 4 at 4:4:4):
//  * 32-bit byte offsets.  A frame is (h w + 2 ch cw) SB bytes: 1.5, 2 or 3 h w SB.  With h w SB < 2^29 (the check below) that is below
//    1.5 * 2^30, and so is every offset the row functions form; the largest sum they compare, (m & ~3) + 16 with m < fbytes (the exact-load
//    tests), stays far below 2^32.  Frame n starts at n * fbytes in size_t.  __umul24(row, pitch): rows < h < 2^24 (checked), pitch <= w SB < 2^23
//    (checked; the interleaved 4:4:4 row of 2 w SB is not offered).
//  * Alignment.  Plane starts and pitches, in bytes: Y 0 and w SB; interleaved chroma h w SB and 2 cw SB; planar U h w SB, V (h w + ch cw) SB,
//    pitch cw SB.  8 bit: everything but the planar chroma is a multiple of 4 (their 4-byte stores; frames are 4-byte aligned and fbytes is a
//    multiple of 4 -- 12, 16, 24 times h w / 8); planar chroma is a multiple of 2 at 4:2:0 (ch cw = h w / 4 may be 2 mod 4), of 4 at 4:2:2 and
//    4:4:4, and is accessed through the byte-aligned U8x4 / U8x2 either way.  16 bit: Y rows and interleaved chroma rows are multiples of 8 bytes
//    (uint2 / U32x4 stores; frames are 8-byte aligned, fbytes a multiple of 8), planar chroma of 4 (cw SB = 2 cw, cw even; plane sizes ch cw SB
//    likewise), its stores are dword-aligned U32x2.  The tap loads align their own address down to 4 bytes from the frame's start.
//  * Reads behind a tap pair / window (up to 6 bytes, bilinear 8 bit; 4 bytes, the others) are inside the frame, or inside the next frame,
//    everywhere but at the end of the LAST plane of the LAST sample: the row functions compare the largest offset a wave reads -- taken in the
//    V plane (off1) for planar chroma -- with fbytes, whatever the geometry, and fall back to exact loads.  The chroma planes are the frame's
//    last bytes in every layout here (V ends at fbytes; interleaved UV ends at fbytes), so "fbytes" is the only fact that rule needs, and
//    the exact loads touch the pair / window alone, which the clamps (x <= W - 2 resp. W - 4, y <= H - 1) keep inside the plane.
//  * Writes: a lane stores its own 4 pixels (2 in the last lane of a chroma row of width 2 mod 4: 4:2:0 and 4:2:2 only) and nothing else.
//  * Grid: a chroma row takes (cw + 255) / 256 of the cpr chunks -- half of them at 4:2:0 and 4:2:2, ALL of them at 4:4:4; the kernels
//    return for chunks past a plane's width.
template <int SB>
static int launch_yuv(const char *what, const void *frames, const float *field, const void *other, const char *other_name, int n, int h, int w,
                      int fh, int fw, int layout, int chroma, int align_corners, int min_cw, const char *min_w_why, LaunchYuv &L) {
    PWS_REQUIRE(n >= 0 && h > 0 && w > 0 && fh > 0 && fw > 0, "%s: bad shape", what);
    PWS_REQUIRE(layout == 0 || layout == 1, "%s: layout must be 0 (%s) or 1 (%s), got %d", what, SB == 1 ? "NV12" : "P010", SB == 1 ? "I420" : "I010", layout);
    PWS_REQUIRE(chroma >= 0 && chroma <= 2, "%s: chroma must be 0 (4:2:0), 1 (4:2:2) or 2 (4:4:4), got %d", what, chroma);
    PWS_REQUIRE(!(chroma == 2 && layout == 0), "%s: interleaved 4:4:4 (%s) is not offered: layout 0 needs chroma 0 or 1", what, SB == 1 ? "NV24" : "P410");
    PWS_REQUIRE(h % 2 == 0 && w % 4 == 0 && h >= 2, "%s: h must be even and w a multiple of 4 (got %d x %d)", what, w, h);
    const int cx = chroma == 2 ? 0 : 1, cy = chroma == 0 ? 1 : 0;
    PWS_REQUIRE(w >= (min_cw << cx), "%s: w must be at least %d %s, got %d", what, min_cw << cx, min_w_why, w);
    if (n == 0) return PWS_OK;
    PWS_REQUIRE(frames && field && other, "%s: NULL pointer", what);
    PWS_REQUIRE(((reinterpret_cast<size_t>(frames) | reinterpret_cast<size_t>(other)) & (SB == 1 ? 3 : 7)) == 0, "%s: frames and %s must be %d-byte aligned",
                what, other_name, SB == 1 ? 4 : 8);
    PWS_REQUIRE((size_t)h * w < (1u << (SB == 1 ? 29 : 28)) && w < (1 << (SB == 1 ? 23 : 22)) && h < (1 << 24) && n < 65536,
                "%s: frame or batch too large", what);
    const unsigned hw = (unsigned)(h * w) * SB, hc = (unsigned)(h >> cy), wc = (unsigned)(w >> cx);   // byte offsets and pitches
    L.fbytes = hw + 2u * hc * wc * SB;   // (4:2:0: h w 3 / 2 samples.  16 bit: a multiple of 8, every frame starts 8-byte aligned)
    L.spp = 1.0 + 2.0 / (double)(1 << (cx + cy));
    L.py = make_plane(h, w, 0u, 0u, (unsigned)w * SB, fh, fw, align_corners);
    L.pc = layout == 0 ? make_plane((int)hc, (int)wc, hw, hw, 2u * wc * SB, fh, fw, align_corners)
                       : make_plane((int)hc, (int)wc, hw, hw + hc * wc * SB, wc * SB, fh, fw, align_corners);
    L.gx = (L.py.nrg + L.pc.nrg + 7u) & ~7u, L.cpr = (unsigned)((w + 255) / 256);   // (chroma rows need half the chunks, all at 4:4:4: the rest return)
    L.fmy = yuv_fmode(L.py.rx), L.fmc = yuv_fmode(L.pc.rx);
    return PWS_OK;
}
}  // namespace yuv
}  // namespace pws
