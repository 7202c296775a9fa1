// What the border passes (border_keep.hip, border_mosaic.hip) share: a lane's bytes of one source plane -- its 4 pixels of one row -- loaded
// and stored at the warps' alignment rules, and the byte mask of one of those pixels.
#pragma once
#include "common.h"
#include "warp_common.h"

namespace pws {
namespace keep {

constexpr int PLANE_BGR = 3;   // (beside yuv::PLANE_Y / PLANE_NV12_UV / PLANE_I420_UV)

typedef unsigned U32x4u __attribute__((ext_vector_type(4), aligned(4)));   // 16 / 12 / 8 bytes at dword alignment
typedef unsigned U32x3u __attribute__((ext_vector_type(3), aligned(4)));
typedef unsigned U32x2u __attribute__((ext_vector_type(2), aligned(4)));

// A lane's bytes of one source plane: NDW dwords for 4 pixels (`full`), the first half of them for the 2 pixels a chroma row of width 2 mod 4
// ends with.  BYTES: 8-bit I420 chroma, 4 (2) bytes at 2-byte alignment; everything else is 4-byte aligned (the warps' alignment rules).
template <int NDW, bool BYTES>
__device__ __forceinline__ void load_lane(const unsigned char *p, bool full, unsigned d[NDW]) {
    if constexpr (BYTES) {
        d[0] = full ? reinterpret_cast<const U8x4 *>(p)->v : (unsigned)reinterpret_cast<const U8x2 *>(p)->v;
    } else if constexpr (NDW == 1) {
        d[0] = *reinterpret_cast<const unsigned *>(p);
    } else if constexpr (NDW == 2) {
        if (full) {
            const U32x2u t = *reinterpret_cast<const U32x2u *>(p);
            d[0] = t.x, d[1] = t.y;
        } else {
            d[0] = *reinterpret_cast<const unsigned *>(p), d[1] = 0u;
        }
    } else if constexpr (NDW == 3) {
        const U32x3u t = *reinterpret_cast<const U32x3u *>(p);
        d[0] = t.x, d[1] = t.y, d[2] = t.z;
    } else {
        if (full) {
            const U32x4u t = *reinterpret_cast<const U32x4u *>(p);
            d[0] = t.x, d[1] = t.y, d[2] = t.z, d[3] = t.w;
        } else {
            const U32x2u t = *reinterpret_cast<const U32x2u *>(p);
            d[0] = t.x, d[1] = t.y, d[2] = 0u, d[3] = 0u;
        }
    }
}
template <int NDW, bool BYTES>
__device__ __forceinline__ void store_lane(unsigned char *p, bool full, const unsigned d[NDW]) {
    if constexpr (BYTES) {
        if (full) reinterpret_cast<U8x4 *>(p)->v = d[0];
        else reinterpret_cast<U8x2 *>(p)->v = (unsigned short)d[0];
    } else if constexpr (NDW == 1) {
        *reinterpret_cast<unsigned *>(p) = d[0];
    } else if constexpr (NDW == 2) {
        if (full) *reinterpret_cast<U32x2u *>(p) = U32x2u{d[0], d[1]};
        else *reinterpret_cast<unsigned *>(p) = d[0];
    } else if constexpr (NDW == 3) {
        *reinterpret_cast<U32x3u *>(p) = U32x3u{d[0], d[1], d[2]};
    } else {
        if (full) *reinterpret_cast<U32x4u *>(p) = U32x4u{d[0], d[1], d[2], d[3]};
        else *reinterpret_cast<U32x2u *>(p) = U32x2u{d[0], d[1]};
    }
}

}  // namespace keep
}  // namespace pws
