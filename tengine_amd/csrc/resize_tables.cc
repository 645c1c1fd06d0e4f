// The host-built operands of a nearest Resize node (resize_ref.c: nearest_neighbor_resize_int8 :261-320, _uint8 :322-381; run :398-486).
// The reference dequantises the whole input to float, moves floats -- output pixel (i, j) takes input pixel
// (min((int)(i * scale_y), h - 1), min((int)(j * scale_x), w - 1)) with scale_y = 1.f / scale_h, scale_x = 1.f / scale_w -- and
// requantises every output element.  No value is computed, so, as for nearest Interp (interp_tables.cc), the device keeps no formula: a
// 256-entry byte map and two index vectors are built here at prerun and the kernels (interp.hip, resize.hip) only look things up.
//
// What differs from Interp is the index rule (a product with a reciprocal and a clamp, where Interp divides and does not clamp) and the
// shape rule (resize.c:47-48).  What does NOT differ are the two lines of the byte map -- ((float)q - (float)zero) * scale, then
// round(f / scale + zero) with the int32 zero point converted to float, clamped to +-127 | 0 .. 255 --: tamd_resize_table is
// tamd_interp_table's implementation (interp_tables.cc: interp_rounded) behind a check that every entry is defined.
//
// Plain C++ (no HIP), compiled with -ffp-contract=off (build.py).  There is no multiply-add in any of these lines, so nothing could
// contract; the flag is stated all the same.  Links with interp_tables.cc alone (tests/csrc/resize_rules_check.cc runs both under the
// sanitizers).
#include "resize_tables.h"

#include <math.h>

#include "interp_tables.h"

namespace tamd {

bool resize_out_extent(int in_extent, float scale, int* out)
{
    if (!(scale > 0.f) || !isfinite(scale) || in_extent < 0) return false;
    const float f = (float)in_extent * scale;
    if (!(f >= 0.f && f < 2147483648.f)) return false;
    *out = (int)f;
    return true;
}

}  // namespace tamd

extern "C" int tamd_resize_table(int dtype, float in_scale, int in_zp, float out_scale, int out_zp, unsigned char table[256])
{
    if (!table || (dtype != TAMD_DT_INT8 && dtype != TAMD_DT_UINT8)) return -1;
    for (int b = 0; b < 256; b++) {                          // int idata = round(..): undefined outside int, and for a NaN
        const double d = tamd::interp_rounded(dtype == TAMD_DT_INT8 ? (int)(signed char)(unsigned char)b : b, in_scale, in_zp, out_scale, out_zp);
        if (!(d >= -2147483648.0 && d <= 2147483647.0)) return -2;
    }
    return tamd_interp_table(dtype, in_scale, in_zp, out_scale, out_zp, table);
}

extern "C" int tamd_resize_indices(int in_extent, int out_extent, float scale, int* idx)
{
    if (!idx || in_extent < 1 || out_extent < 1 || !(scale > 0.f) || !isfinite(scale)) return -1;
    const float inv = 1.f / scale;                           // :409-410: scale_x = 1.f / scale_w, scale_y = 1.f / scale_h
    for (int o = 0; o < out_extent; o++) {
        const float q = (float)o * inv;                      // :298 / :301: int * float, truncated by the cast
        if (!(q >= 0.f && q < 2147483648.f)) return -1;      // (a NaN -- 0 * inf -- fails both comparisons)
        const int s = (int)q;
        idx[o] = s < in_extent - 1 ? s : in_extent - 1;      // T_MIN(.., h - 1)
    }
    return 0;
}
