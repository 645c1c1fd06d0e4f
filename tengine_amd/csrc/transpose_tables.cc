// The byte map of the quantised Transpose (transpose_ref.c: ref_transpose_int8 :270-329, ref_transpose_uint8 :331-387).  The reference
// dequantises the whole input to floats, moves floats by one loop nest per rank and requantises every output element -- the identity
// order included, there is no memcpy shortcut --, so every output byte is a function of ONE input byte and the two tensors' parameters:
// the device keeps no formula, the 256 results are built here at prerun and transpose.hip only moves bytes through them.
//
// Plain C++ (no HIP), compiled with -ffp-contract=off (build.py).  The reference's lines are a difference times a scale and a quotient
// plus a converted int: neither is a product followed by a sum, so its compiler has nothing to contract either (compared against the
// built reference on all 256 bytes of every parameter pair of tests/transpose_helpers.py, both types: tests/test_transpose_cpu.py).  Every operation below rounds
// by itself.  The uint8 lines are those of tamd_slice_table; they are restated here so that the two types read side by side.
#include "transpose_tables.h"

#include <math.h>

extern "C" int tamd_transpose_table(int dtype, float in_scale, int in_zp, float out_scale, int out_zp, unsigned char table[256])
{
    if (!table || (dtype != TAMD_DT_INT8 && dtype != TAMD_DT_UINT8)) return -1;
    const bool i8 = dtype == TAMD_DT_INT8;
    unsigned char t[256];
    for (int b = 0; b < 256; b++) {
        const float raw = i8 ? (float)(signed char)(unsigned char)b : (float)(unsigned char)b;
        const float f = (raw - (float)in_zp) * in_scale;                 // :290 / :348  input[i] = ((float)q - (float)input_zero) * input_scale
        const float q = f / out_scale;                                    // :317 / :375  output[i] / output_scale, a float division
        const float r = q + (float)out_zp;                                //              + output_zero: the int32_t converts to float
        const double d = round((double)r);                                //              round(): the double one
        if (!(d >= -2147483648.0 && d <= 2147483647.0)) return -1;        // int idata = ..: undefined outside int, and for NaN
        int v = (int)d;
        if (i8) v = v > 127 ? 127 : (v < -127 ? -127 : v);                // :318-321: -128 never comes out
        else v = v > 255 ? 255 : (v < 0 ? 0 : v);                         // :376-379
        t[b] = (unsigned char)v;
    }
    for (int b = 0; b < 256; b++) table[b] = t[b];
    return 0;
}
