// The byte maps of the quantised Sigmoid / Clip / HardSwish / Mish nodes.  In the reference each of these kernels dequantises one byte,
// applies a scalar function and requantises: the output byte depends on the input byte and on the two tensors' (scale, zero point)
// alone.  So the device keeps no formula: it maps bytes through the 256-entry table built here at prerun (misc_kernels.hip: lut_u8).
//
// Every builder below restates ONE reference kernel for one input byte, with the reference's types and the order of its
// conversions -- float where it computes in float, the double exp / log / round of libm where it calls those on a float, tanhf where
// it calls tanhf -- and runs on the host through the same libm, so the table holds the reference's bytes by construction, its
// oddities included.  The file is plain C++ (no HIP) and is compiled with -ffp-contract=off (build.py): nothing may be fused into a
// multiply-add that the reference rounds twice.  (C++ overloads exp / log / round on float: the casts to double below are what C's
// implicit conversion does in the reference.)
#include "lut_tables.h"

#include <math.h>
#include <stdint.h>

namespace {

// (int)d as x86-64 converts it (cvttsd2si / cvttss2si, what the reference's compiled code does): a value out of int's range, or a
// NaN, gives INT_MIN -- a scale of 0 or a denormal one gets there; in range it is the plain truncation
int to_int(double d) { return d >= -2147483648.0 && d < 2147483648.0 ? (int)d : INT32_MIN; }

struct Quant { float in_scale; int in_zp; float out_scale; int out_zp; };

// "input dequant" of every kernel below: ((float)q - (float)zero) * scale
float dequant(int q, const Quant& t) { return ((float)q - (float)t.in_zp) * t.in_scale; }

// the requantisation of sigmoid_ref.c, hardswish_kernel_ref_uint8.c and mish_kernel_ref_uint8.c: round(f / scale + zero) -- the
// division and the addition in float (the zero point converted to float), then the DOUBLE round of libm
int quant_round(float f, const Quant& t)
{
    const float scaled = f / t.out_scale + t.out_zp;
    return to_int(round((double)scaled));
}

// sigmoid_ref.c:99-110 / :144-155.  The clamp is two assignments from the INPUT: the result of the first, SIGMOID_MIN(x, 30), is
// overwritten by the second, SIGMOID_MAX(x, -30), so only the lower bound holds.  exp is the double routine on a float argument, the
// quotient is rounded to float by the store
float sigmoid(float x)
{
    float o = x > -30.0f ? x : -30.0f;
    o = 1 / (1 + exp((double)-o));
    return o;
}

// sigmoid_ref.c:84-127: +-127 saturation
unsigned char sigmoid_i8(unsigned char b, const Quant& t, const void*)
{
    int v = quant_round(sigmoid(dequant((int8_t)b, t)), t);
    if (v > 127) v = 127;
    else if (v < -127) v = -127;
    return (unsigned char)(int8_t)v;
}

// sigmoid_ref.c:129-172
unsigned char sigmoid_u8(unsigned char b, const Quant& t, const void*)
{
    int v = quant_round(sigmoid(dequant(b, t)), t);
    if (v > 255) v = 255;
    else if (v < 0) v = 0;
    return (unsigned char)v;
}

// clip_kernel_ref_int8.c:56-74 and clip_kernel_ref_uint8.c:56-74 are the same lines over int8_t / uint8_t: max first, then min;
// (int)roundf(f / scale) + zero; saturated ONLY above 255 and then narrowed to the element type -- a quotient below 0 wraps in uint8,
// and in int8 one in 128 .. 255 wraps negative (255 itself, and everything above it, is -1).  Both narrowings keep the low byte
unsigned char clip_byte(float x, const Quant& t, const tamd_clip_param& p)
{
    float o = x;
    if (o > p.max) o = p.max;
    if (o < p.min) o = p.min;
    const int v = (int)((unsigned)to_int(roundf(o / t.out_scale)) + (unsigned)t.out_zp);
    return (unsigned char)(v > 255 ? 255 : v);
}
unsigned char clip_i8(unsigned char b, const Quant& t, const void* p) { return clip_byte(dequant((int8_t)b, t), t, *(const tamd_clip_param*)p); }
unsigned char clip_u8(unsigned char b, const Quant& t, const void* p) { return clip_byte(dequant(b, t), t, *(const tamd_clip_param*)p); }

// hardswish_kernel_ref_uint8.c:55-79: x * (clamp(x + 3, 0, 6) / 6) in float; alpha / beta of the node are not read
unsigned char hardswish_u8(unsigned char b, const Quant& t, const void*)
{
    float x = dequant(b, t);
    float tmp = x + 3.f;
    if (tmp < 0.f) tmp = 0.f;
    if (tmp > 6.f) tmp = 6.f;
    x = x * (tmp / 6.f);
    int v = quant_round(x, t);
    if (v > 255) v = 255;
    else if (v < 0) v = 0;
    return (unsigned char)v;
}

// mish_kernel_ref_uint8.c:63-90: x * tanhf(log(1 + exp(x))) -- exp and log are the double routines, their result is narrowed to
// float for tanhf, the product is float
unsigned char mish_u8(unsigned char b, const Quant& t, const void*)
{
    float x = dequant(b, t);
    x = x * tanhf((float)log(1 + exp((double)x)));
    int v = quant_round(x, t);
    if (v > 255) v = 255;
    else if (v < 0) v = 0;
    return (unsigned char)v;
}

// the one list: which (operator, type) pairs the device runs, and the reference kernel each restates
struct Builder { int op, dtype; bool needs_param; unsigned char (*fn)(unsigned char, const Quant&, const void*); };
const Builder kBuilders[] = {
    {TAMD_OP_SIGMOID, TAMD_DT_INT8, false, sigmoid_i8},     {TAMD_OP_SIGMOID, TAMD_DT_UINT8, false, sigmoid_u8},
    {TAMD_OP_CLIP, TAMD_DT_INT8, true, clip_i8},            {TAMD_OP_CLIP, TAMD_DT_UINT8, true, clip_u8},
    {TAMD_OP_HARDSWISH, TAMD_DT_UINT8, false, hardswish_u8}, {TAMD_OP_MISH, TAMD_DT_UINT8, false, mish_u8},
};

const Builder* find_builder(int op, int dtype)
{
    for (const Builder& b : kBuilders)
        if (b.op == op && b.dtype == dtype) return &b;
    return nullptr;
}

}  // namespace

namespace tamd {
bool lut_op_on_device(int op, int dtype) { return find_builder(op, dtype) != nullptr; }
}  // namespace tamd

extern "C" int tamd_lut_table(int op, int dtype, const void* param, float in_scale, int in_zp, float out_scale, int out_zp, unsigned char table[256])
{
    const Builder* b = find_builder(op, dtype);
    if (!b || !table || (b->needs_param && !param)) return -1;
    const Quant t{in_scale, in_zp, out_scale, out_zp};
    for (int i = 0; i < 256; i++) table[i] = b->fn((unsigned char)i, t, param);
    return 0;
}
