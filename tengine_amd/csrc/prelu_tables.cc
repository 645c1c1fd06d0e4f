// The quantised PReLU of the reference (prelu_ref.c: ref_prelu_int8 :317-384, ref_prelu_uint8 :160-315), restated for ONE input byte of
// ONE channel.  Both kernels dequantise a byte, apply  y = MAX(x, 0) + slope[c] * MIN(x, 0.f)  in float and requantise, so the output
// byte depends on the input byte, the channel's slope and the two tensors' (scale, zero point) alone.  tamd_prelu_table is that
// function over all 256 bytes: the uint8 kernel (prelu.hip: prelu_u8) maps bytes through it, the int8 kernel (prelu_i8) computes the
// same chain on the device and is tested against it byte for byte.
//
// The slope tensor is fp16 in both quantised modes and the reference widens it with its own routine, which is not IEEE:
// tamd_prelu_slope restates it branch by branch, quirks included.
//
// Plain C++ (no HIP), compiled with -ffp-contract=off (build.py) like lut_tables.cc: float where the reference computes in float, the
// double round of libm where it calls round on a float.
#include "prelu_tables.h"

#include <math.h>
#include <stdint.h>
#include <string.h>

namespace {

// (int)d as x86-64 converts it (cvttsd2si, what the reference's compiled code does): out of int's range, or NaN, gives INT_MIN -- a
// scale of 0 or a denormal one gets there; in range it is the plain truncation (lut_tables.cc: to_int)
int to_int(double d) { return d >= -2147483648.0 && d < 2147483648.0 ? (int)d : INT32_MIN; }

float from_bits(uint32_t b)
{
    float f;
    memcpy(&f, &b, 4);
    return f;
}

// MAX(x, 0) + slope * MIN(x, 0.f).  One of the two addends is always zero -- x > 0: slope * 0; x <= 0: MAX gives 0 -- so the sum is
// the other addend (or a zero), and a contraction of the multiply and the add into one fused operation, which the reference's build
// (-mfma) allows its compiler, rounds once where this rounds once: the same value either way.  (Holds for a finite slope; inf and NaN
// are refused before they get here.)
float prelu(float x, float slope)
{
    const float pos = x > 0 ? x : 0;
    const float neg = x < 0.f ? x : 0.f;
    return pos + slope * neg;
}

}  // namespace

// fp16_to_fp32 of source/utility/float.c:41-104, the routine an x86 build of the reference widens the slopes with.  Its branches in
// its order:
//  - zero: a zero of the half's sign;
//  - "normalized": taken only when the fraction is NOT zero (the condition reads 0 != frac): exponent rebiased, fraction << 13;
//  - infinity; NaN (fraction 1);
//  - sub-normal: the fraction is shifted up until bit 9 is set, then (frac << 1) & 0x3ff lands in the LOW bits of the 23-bit field --
//    the shift by 13 is missing -- with exponent 112 - shifts: 0x0003 gives 0x34000200, not 0x34400000;
//  - everything else falls through every branch: the normal halves whose fraction is zero, i.e. the exact powers of two (0.25, 0.5, 1,
//    2, ...).  The function then returns a value it never assigned.  The object code of the BUILT reference (gcc, -O3) returns +0.0f
//    there, whatever the sign, and that is what is written below: a PReLU whose slope is 0.25 is a ReLU in the reference.
//    tests/test_prelu_cpu.py sweeps all 65 536 patterns against the built library's own symbol, so another compiler that decides
//    otherwise fails that test instead of letting the device drift.
extern "C" float tamd_prelu_slope(unsigned short half_bits)
{
    const uint32_t sign = (uint32_t)(half_bits >> 15) << 31, exp = (half_bits >> 10) & 0x1fu, frac = half_bits & 0x3ffu;
    if (exp == 0 && frac == 0) return from_bits(sign);
    if (exp != 31 && exp != 0 && frac != 0) return from_bits(sign | (exp + 112u) << 23 | frac << 13);
    if (exp == 31 && frac == 0) return from_bits(sign | 0xffu << 23);
    if (exp == 31) return from_bits(sign | 0xffu << 23 | 1u);
    if (exp == 0) {
        uint32_t f = frac, shifts = 0;
        while (!(f & 0x200u)) { f <<= 1; shifts++; }
        return from_bits(sign | (112u - shifts) << 23 | ((f << 1) & 0x3ffu));
    }
    return +0.0f;                // the fall-through: what the built reference's object code returns (see above)
}

namespace tamd {
bool prelu_slopes_finite(const unsigned short* half_bits, size_t count)
{
    for (size_t i = 0; i < count; i++)
        if (!isfinite(tamd_prelu_slope(half_bits[i]))) return false;
    return true;
}
}  // namespace tamd

extern "C" int tamd_prelu_table(int dtype, unsigned short slope_bits, float in_scale, int in_zp, float out_scale, int out_zp, unsigned char table[256])
{
    const float slope = tamd_prelu_slope(slope_bits);
    if (!table || !isfinite(slope) || (dtype != TAMD_DT_INT8 && dtype != TAMD_DT_UINT8)) return -1;
    for (int b = 0; b < 256; b++) {
        if (dtype == TAMD_DT_INT8) {
            // :341 (float)q * scale; :369-374 round(y / scale) -- the division in float, the DOUBLE round of libm -- saturated to
            // +-127: -128 never comes out, whatever goes in
            const float y = prelu((float)(int8_t)b * in_scale, slope);
            int v = to_int(round((double)(y / out_scale)));
            if (v > 127) v = 127;
            else if (v < -127) v = -127;
            table[b] = (unsigned char)(int8_t)v;
        } else {
            // :184 ((float)q - (float)zero) * scale with the zero points as uint32_t; :302-307 round(y / scale + zero), 0 .. 255
            const float y = prelu(((float)b - (float)(uint32_t)in_zp) * in_scale, slope);
            const float scaled = y / out_scale + (uint32_t)out_zp;
            int v = to_int(round((double)scaled));
            if (v > 255) v = 255;
            else if (v < 0) v = 0;
            table[b] = (unsigned char)v;
        }
    }
    return 0;
}
