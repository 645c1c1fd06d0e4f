// The host-built operands of a nearest Interp node (interp_ref.c: ref_interp_int8 :249-360, ref_interp_uint8 :362-469).  The reference
// dequantises the whole input to float, picks for every output pixel the source pixel (int)(h / height_scale), (int)(w / width_scale),
// and requantises the whole output.  Nearest mode moves values, it computes none: the output byte is a function of the input byte and
// the two tensors' (scale, zero point), and the source pixel a function of the output row and column alone.  So the device keeps no
// formula: a 256-entry byte map and two index vectors are built here at prerun, with the reference's own types and the order of its
// conversions, and the kernels (interp.hip) only look things up.
//
// Plain C++ (no HIP), compiled with -ffp-contract=off (build.py): nothing may be fused that the reference rounds twice.  The file
// links alone (tests/csrc/interp_tables_check.cc runs it under the sanitizers).
#include "interp_tables.h"

#include <math.h>
#include <stdint.h>

namespace {

// (int)d as x86-64 converts it (cvttsd2si, what the reference's compiled code does): out of int's range, or a NaN, gives INT_MIN -- a
// scale of 0 gets there; in range it is the plain truncation
int to_int(double d) { return d >= -2147483648.0 && d < 2147483648.0 ? (int)d : INT32_MIN; }

int requant(int q, float in_scale, int in_zp, float out_scale, int out_zp) { return to_int(tamd::interp_rounded(q, in_scale, in_zp, out_scale, out_zp)); }

}  // namespace

namespace tamd {

// interp_ref.c:271 / :380 then :348 / :457 for one element: ((float)q - (float)zero) * scale; round(f / scale + zero) -- the division
// and the addition in float (the zero point converted to float), then the DOUBLE round of libm
double interp_rounded(int q, float in_scale, int in_zp, float out_scale, int out_zp)
{
    const float f = ((float)q - (float)in_zp) * in_scale;
    const float scaled = f / out_scale + (float)out_zp;
    return round((double)scaled);
}

bool interp_resolve(const tamd_interp_param& p, int in_h, int in_w, InterpGeom* g)
{
    if (in_h < 1 || in_w < 1) return false;
    const bool by_scale = p.height_scale != 0 && p.width_scale != 0;               // interp.c:51
    if (!by_scale && (p.output_height < 1 || p.output_width < 1)) return false;
    g->height_scale = by_scale ? p.height_scale : (float)p.output_height / (float)in_h;
    g->width_scale = by_scale ? p.width_scale : (float)p.output_width / (float)in_w;
    g->out_h = to_int((double)((float)in_h * g->height_scale));                     // :53-54: int * float, truncated by the assignment
    g->out_w = to_int((double)((float)in_w * g->width_scale));
    if (g->out_h < 1 || g->out_w < 1) return false;
    return by_scale || (g->out_h == p.output_height && g->out_w == p.output_width);
}

}  // namespace tamd

extern "C" int tamd_interp_table(int dtype, float in_scale, int in_zp, float out_scale, int out_zp, unsigned char table[256])
{
    if (!table || (dtype != TAMD_DT_INT8 && dtype != TAMD_DT_UINT8)) return -1;
    for (int b = 0; b < 256; b++) {
        if (dtype == TAMD_DT_INT8) {                         // :349-353: +-127, so the byte -128 never comes out
            int v = requant((int8_t)b, in_scale, in_zp, out_scale, out_zp);
            if (v > 127) v = 127;
            else if (v < -127) v = -127;
            table[b] = (unsigned char)(int8_t)v;
        } else {                                             // :458-462
            int v = requant(b, in_scale, in_zp, out_scale, out_zp);
            if (v > 255) v = 255;
            else if (v < 0) v = 0;
            table[b] = (unsigned char)v;
        }
    }
    return 0;
}

extern "C" int tamd_interp_indices(int in_extent, int out_extent, float scale, int* idx)
{
    if (!idx || in_extent < 1 || out_extent < 1) return -1;
    for (int o = 0; o < out_extent; o++) {
        const float q = (float)o / scale;                    // :292-293 / :401-402: int / float, truncated by the assignment
        if (!(q >= 0.f && q < (float)in_extent)) return -1;  // (a NaN -- 0 / 0 -- fails both comparisons)
        idx[o] = (int)q;
        if (idx[o] >= in_extent) return -1;                  // ((float)in_extent may have rounded up)
    }
    return 0;
}
