// The generator's layer table: the 46 layers in the reference's registration order, where each one's weights live in the packed
// buffers and in the gradient slab, and the facts about a conv kind that the packing and the executor share.
#pragma once
#include <vector>

#include "common.h"

namespace pws {

struct Layer {
    int kind, cin, cout;
    size_t w_off, b_off;  // float offsets into the packed buffer
    size_t gw_off, gb_off;  // float offsets into the GRADIENT slab (pws_netg_grad_floats): weight gradient in the forward packed layout,
                            // bias gradient right behind it -- the slab holds nothing else, so a data-parallel host all-reduces it in place
    size_t dg_off;        // float offset into the data-gradient weight buffer (or SIZE_MAX)
    size_t ww_off;        // float offset of the Winograd-domain weights inside the packed buffer (or SIZE_MAX)
    size_t wr_off;        // ... of the ring-layout Winograd weights (conv_wring.hip; or SIZE_MAX)
    size_t wb_off;        // float offset of the bf16 weights inside the packed buffer (or SIZE_MAX)
    size_t dgb_off;       // float offset of the bf16 data-gradient weights inside the data-gradient buffer (or SIZE_MAX)
};

enum {
    L_TRANSFER = 0,
    L_DOWN1 = 1,   // down1..down7 = 1..7
    L_UP7 = 8,     // up7..up1 = 8..14   (level l -> 8 + (7 - l))
    L_OUT = 15,
    L_DB1_CS = 16,  // down_bottom k: conv_same 16+2(k-1), mpconv 17+2(k-1)
    L_UB7_MP = 30,  // up_bottom level l: mpconv 30+2(7-l), conv_same 31+2(7-l)
    L_FLATTEN = 44,
    L_LINEAR = 45,
    L_COUNT = 46
};

// What a conv kind fixes: the kernel edge, the planes (taps) of its forward packed layout, the taps of its data-gradient layout
// (0: the kind has no data gradient) and whether the bf16 kernels cover it.
struct KindGeom {
    int ksize, planes, dg_taps;
    bool bf16;
};
KindGeom kind_geom(int kind);

struct LayerTable {
    std::vector<Layer> L;
    size_t packed = 0, dgrad = 0, grad = 0;   // floats of the packed buffer, the data-gradient buffer and the gradient slab
    const Layer &operator[](int i) const { return L[i]; }
};
LayerTable build_layers(int input_nc, int ngf);

inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }
inline bool valid_shape(int input_nc, int ngf) { return input_nc > 0 && ngf > 0 && ngf % 16 == 0; }
#define PWS_REQUIRE_SHAPE(who, input_nc, ngf) \
    PWS_REQUIRE(pws::valid_shape(input_nc, ngf), who ": input_nc must be positive and ngf a positive multiple of 16 (got %d / %d)", input_nc, ngf)

}  // namespace pws
