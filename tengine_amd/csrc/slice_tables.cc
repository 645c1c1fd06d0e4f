// The byte map of the uint8 Slice (slice_ref.c:475-509).  The reference dequantises the whole input to floats, moves floats and
// requantises the output, so every output byte is a function of ONE input byte and the two tensors' parameters: the device keeps no
// formula, the 256 results are built here at prerun and slice.hip only moves bytes through them.
//
// Plain C++ (no HIP), compiled with -ffp-contract=off (build.py).  The reference's two lines hold a product, a quotient and a sum in
// separate statements or around a division, so its compiler cannot contract any of them either: every operation below rounds by itself.
#include "slice_tables.h"

#include <math.h>

extern "C" int tamd_slice_table(float in_scale, int in_zp, float out_scale, int out_zp, unsigned char table[256])
{
    if (!table) return -1;
    if (!(in_scale > 0.f) || !(out_scale > 0.f) || isinf(in_scale) || isinf(out_scale)) return -1;
    unsigned char t[256];
    for (int b = 0; b < 256; b++) {
        const float f = ((float)(unsigned char)b - (float)in_zp) * in_scale;      // :492  input_fp32[i] = ((float)u - (float)zero) * scale
        const float q = f / out_scale;                                            // :499  output_fp32[i] / output_scale, a float division
        const float r = q + (float)out_zp;                                        //       + output_zero: the int converts to float
        const double d = round((double)r);                                        //       round(): the double one
        if (!(d >= -2147483648.0 && d <= 2147483647.0)) return -1;                // int udata = ..: undefined outside int, and for NaN
        int v = (int)d;
        if (v > 255) v = 255;
        else if (v < 0) v = 0;
        t[b] = (unsigned char)v;
    }
    for (int b = 0; b < 256; b++) table[b] = t[b];
    return 0;
}
