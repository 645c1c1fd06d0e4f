// The byte maps of the quantised Sigmoid / Clip / HardSwish / Mish nodes, and (further down) of an Eltwise with a constant scalar or of a
// unary type.  In the reference each of these kernels dequantises one byte,
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

// ---- Eltwise with a constant scalar, and the unary Eltwise types (eltwise_ref.c:311-587 uint8, :589-847 int8) ----
// Both kernels dequantise every operand into float arrays, run one loop of the operator over them and requantise in a third loop:
// three statements with a store between them, so nothing is contracted across them -- but inside the POWER line the compiler of the
// built reference (-O3 -mfma) does make shift + scale * x one fused multiply-add, and so does eltwise_value below.
namespace {

enum { kProd = 0, kProdScalar = 1, kSum = 2, kSumScalar = 3, kSub = 4, kSubScalar = 5, kMax = 6, kRsqrt = 7, kMinScalar = 8, kLast = 9, kDiv = 10,
       kLog = 11, kExp = 12, kSqrt = 13, kFloor = 14, kSquare = 15, kPow = 16, kPower = 17 };

// "input dequant": uint8 (u - zero) * scale with the subtraction in int (:332, :343), int8 (float)q * scale (:607, :615)
float elt_dequant(int dtype, unsigned char b, float scale, int zp)
{
    if (dtype == TAMD_DT_INT8) return (float)(int8_t)b * scale;
    return (float)((int)b - zp) * scale;
}

// "output quant": round(f / scale) -- a float division, the double round -- + zero in double, converted to int (:573 | :833); false
// where that conversion is undefined (NaN, or outside int)
bool elt_requant(int dtype, float f, float out_scale, int out_zp, unsigned char* byte)
{
    const float q = f / out_scale;
    const double d = dtype == TAMD_DT_INT8 ? round((double)q) : round((double)q) + (double)out_zp;
    if (!(d > -2147483649.0 && d < 2147483648.0)) return false;
    int v = (int)d;
    if (dtype == TAMD_DT_INT8) {
        if (v > 127) v = 127;
        else if (v < -127) v = -127;
        *byte = (unsigned char)(int8_t)v;
    } else {
        if (v > 255) v = 255;
        else if (v < 0) v = 0;
        *byte = (unsigned char)v;
    }
    return true;
}

// the operator line of a scalar or unary type on one dequantised value; s: in1[0].  false: the kernels have no such line.  sqrt, pow,
// exp, log and floor are the double routines on a float argument, their result narrowed to float by the store into out_ptr
bool eltwise_value(int type, float x, float s, const tamd_eltwise_param* p, float* out)
{
    switch (type) {
    case kProd: case kProdScalar: *out = x * s; return true;
    case kSum: *out = x + s; return true;
    case kSub: case kSubScalar: *out = x - s; return true;
    case kMinScalar: *out = x < s ? x : s; return true;
    case kDiv: *out = x / s; return true;
    case kRsqrt: *out = (float)(1 / sqrt((double)x)); return true;
    case kLog: *out = (float)log((double)x); return true;
    case kExp: *out = (float)exp((double)x); return true;
    case kSqrt: *out = (float)sqrt((double)x); return true;
    case kFloor: *out = (float)floor((double)x); return true;
    case kSquare: *out = (float)pow((double)x, 2); return true;
    case kPower:
        if (!p) return false;
        *out = (float)pow((double)fmaf(p->scale, x, p->shift), (double)p->power);
        return true;
    default: return false;
    }
}

}  // namespace

namespace tamd {
bool eltwise_scalar_type(int type) { return type == kProd || type == kProdScalar || type == kSum || type == kSub || type == kSubScalar || type == kMinScalar || type == kDiv; }
bool eltwise_unary_type(int type) { return type == kRsqrt || (type >= kLog && type <= kSquare) || type == kPower; }
}  // namespace tamd

extern "C" int tamd_eltwise_table(int type, int dtype, const tamd_eltwise_param* param, float scalar, float in_scale, int in_zp, float out_scale, int out_zp,
                                  unsigned char table[256])
{
    if (!table || (dtype != TAMD_DT_INT8 && dtype != TAMD_DT_UINT8)) return -1;
    if (!tamd::eltwise_scalar_type(type) && !tamd::eltwise_unary_type(type)) return -1;
    if (type == kPower && !param) return -1;
    unsigned char t[256];
    for (int b = 0; b < 256; b++) {
        float f;
        if (!eltwise_value(type, elt_dequant(dtype, (unsigned char)b, in_scale, in_zp), scalar, param, &f)) return -1;
        if (!elt_requant(dtype, f, out_scale, out_zp, &t[b])) return -2;
    }
    for (int b = 0; b < 256; b++) table[b] = t[b];
    return 0;
}

extern "C" int tamd_eltwise_scalar(int const_dtype, const void* value, float scale, int zp, float* scalar)
{
    if (!value || !scalar) return -1;
    if (const_dtype == TAMD_DT_FP32) { *scalar = *(const float*)value; return 0; }                       // :345-351
    if (const_dtype == TAMD_DT_UINT8) { *scalar = elt_dequant(TAMD_DT_UINT8, *(const unsigned char*)value, scale, zp); return 0; }
    if (const_dtype == TAMD_DT_INT8) { *scalar = elt_dequant(TAMD_DT_INT8, *(const unsigned char*)value, scale, 0); return 0; }
    return -1;
}

extern "C" int tamd_eltwise_pair(int type, int dtype, unsigned char a, float a_scale, int a_zp, unsigned char b, float b_scale, int b_zp, float out_scale, int out_zp)
{
    if (dtype != TAMD_DT_INT8 && dtype != TAMD_DT_UINT8) return -1;
    const float fa = elt_dequant(dtype, a, a_scale, a_zp), fb = elt_dequant(dtype, b, b_scale, b_zp);
    float f;
    switch (type) {
    case kProd: f = fa * fb; break;
    case kSum: f = fa + fb; break;
    case kSub: f = fa - fb; break;
    case kMax: f = fa > fb ? fa : fb; break;
    default: return -1;
    }
    unsigned char byte;
    if (!elt_requant(dtype, f, out_scale, out_zp, &byte)) return -2;
    return byte;
}

// ---- uint8 BatchNorm: one byte map per channel (batchnorm_ref.c:76-86 prerun, batchnorm_kernel_ref_uint8.c:57-101) ----
// The built reference (-O3 -mfma) contracts every a * b + c of these lines into one fused multiply-add: var * rescale + eps under the
// sqrtf, s_beta + s_gamma * s_mean, and data * s_val2 + s_val1; they are written out as fmaf here (the file itself is compiled with
// contraction off).  The quotient and the zero point are added in float (the int converts), roundf, (int).
extern "C" int tamd_batchnorm_table(const tamd_batchnorm_param* p, float gamma, float beta, float mean, float var, float in_scale, int in_zp, float out_scale,
                                    int out_zp, unsigned char table[256])
{
    if (!p || !table) return -1;
    const float rescale = p->rescale_factor ? 1 / p->rescale_factor : 0;
    const float scale_var_inv = 1.f / sqrtf(fmaf(var, rescale, p->eps));
    const float scale_mean = -mean * (rescale * scale_var_inv);
    float s1 = scale_mean, s2 = scale_var_inv;
    if (!p->caffe_flavor) {
        s1 = fmaf(gamma, scale_mean, beta);
        s2 = gamma * scale_var_inv;
    }
    if (!isfinite(s1) || !isfinite(s2)) return -2;
    unsigned char t[256];
    for (int b = 0; b < 256; b++) {
        const float x = ((float)b - (float)in_zp) * in_scale;
        const float v = fmaf(x, s2, s1);
        const float r = roundf(v / out_scale + (float)out_zp);
        if (!(r >= -2147483648.f && r < 2147483648.f)) return -2;
        int u = (int)r;
        if (u > 255) u = 255;
        else if (u < 0) u = 0;
        t[b] = (unsigned char)u;
    }
    for (int b = 0; b < 256; b++) table[b] = t[b];
    return 0;
}

extern "C" int tamd_lut_table(int op, int dtype, const void* param, float in_scale, int in_zp, float out_scale, int out_zp, unsigned char table[256])
{
    const Builder* b = find_builder(op, dtype);
    if (!b || !table || (b->needs_param && !param)) return -1;
    const Quant t{in_scale, in_zp, out_scale, out_zp};
    for (int i = 0; i < 256; i++) table[i] = b->fn((unsigned char)i, t, param);
    return 0;
}
