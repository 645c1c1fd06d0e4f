// Node-local rules that the support query (graph.hip: tamd_node_supported), validate_graph and the planners all apply: each is
// stated here once, with the reason for its number.  Only rules that are written at more than one site live here; what a single
// planner alone decides stays in that planner.
#pragma once
#include <math.h>

#include <vector>

#include "kernels.h"
#include "chanmap_tables.h"
#include "instnorm_tables.h"
#include "interp_tables.h"
#include "lut_tables.h"
#include "prelu_tables.h"
#include "resize_tables.h"
#include "slice_tables.h"
#include "transpose_tables.h"

namespace tamd {

// Eltwise: the binary forms over two tensors of one shape -- ELT_PROD 0, ELT_SUM 2, ELT_SUB 4, ELT_MAX 6 (eltwise_param.h); the odd
// values next to them are the tensor-with-scalar forms, 7 and up the unary ones: byte maps by table, below (eltwise_refusal)
inline bool eltwise_type_on_device(int type) { return type == 0 || type == 2 || type == 4 || type == 6; }
// .. and the channel gate of a Squeeze-and-Excitation block: x (N, C, H, W) op gate (N, C, 1, 1), int8 and uint8 graphs (chan_gate.hip).
// fp32 graphs keep it on the CPU device (their Sigmoid is there anyway)
inline bool chan_gate_on_device(int dtype) { return dtype == TAMD_DT_INT8 || dtype == TAMD_DT_UINT8; }
// One Eltwise node: nullptr when the device runs it, else the reason.  *gated: -1 (kEltSame) for the same-shape form, 0 | 1: which input
// is x, the operand with more elements, of the gate form -- the other one is the gate --, kEltScalar / kEltUnary for the two table forms
// below.  a / b: inputs 0 / 1 (b_*: unread with one input); b_dtype: the data type of input 1.
// eltwise_ref.c: run() makes the operand with more elements in0, whichever input it is, and hands over input_chan = dims[-4] * dims[-3]
// (N * C), input_hw = H * W and input1_count4 = the smaller operand's element count; the branch input_chan == input1_count4 of
// ref_eltwise_int8 / _uint8 computes out[i] = in0[i] op in1[i / input_hw] for PROD, SUM and SUB: always x op gate, for SUB too.
//  - MAX has no such branch: its loop reads in1[i] over the larger count, past the gate's end -- no bytes to equal
//  - the gate listed first takes input_chan = dims[1] (C, not N * C): at batch > 1 PROD and SUB fail and SUM leaves most of the output
//    unwritten
//  - a smaller operand of another shape (2-D, (1, N * C, 1, 1), one element, a row of H * W) takes other branches of the reference, or
//    the same one with a meaning the device tensors' layout does not carry: each is refused by its own name
//
// The scalar form (*gated = kEltScalar) and the unary form (*gated = kEltUnary), int8 and uint8 graphs: both kernels dequantise, run the
// operator's line against in1[0] or against nothing, and requantise -- one byte in, one byte out, so the device maps bytes through
// tamd_eltwise_table with one lut_u8 launch.  The two kernels have the same cases (eltwise_ref.c:359-568, :619-828):
//  - scalar: inputs [x, c], x a 4-D activation, c a CONSTANT of one element.  PROD_SCALAR 1, SUB_SCALAR 5 and MIN_SCALAR 8 read in1[0]
//    whatever the count; PROD 0, SUM 2, SUB 4 and DIV 10 have the branch input1_count4 == 1.  (Where N * C == 1 SUB takes the channel
//    branch in1[i / input_hw] first, and on a one-element x every type the same-shape one: in1[0] in both.)  The uint8 kernel takes a
//    uint8 or an fp32 constant (:336-351); the int8 kernel reads the buffer as int8 whatever its type, so an fp32 constant is refused
//  - unary: one input.  RSQRT 7, LOG 11, EXP 12, SQRT 13, FLOOR 14, SQUARE 15, POWER 17 (shift, scale, power)
//  - SUM_SCALAR 3 has no case in either kernel (the output is requantised from a buffer nobody wrote); MAX 6 reads in1[i] over the
//    larger count, past a one-element operand's end; the one-element loops of POW 16 run over the wrong count; LAST 9 is no operator
//  - a one-element operand that is not a constant, or is listed first, stays refused: the table is built at prerun from the value
//  - a table entry the reference does not define -- the float result NaN or infinite, or the rounded value outside int, where its
//    float-to-int conversion is undefined behaviour: RSQRT or LOG of a tensor whose zero-point byte is 0.0, a division by 0 --
//    refuses the node: there are no bytes to equal
// v: the values the table is built from, where the caller has them (a support query may not: then the table is not checked, and prerun
// refuses by name what the query let through); table[256]: the byte map (may be null)
enum { kEltSame = -1, kEltScalar = -2, kEltUnary = -3 };
struct EltwiseValues {
    float x_scale; int x_zp; float out_scale; int out_zp;
    const void* c_data; float c_scale; int c_zp;                  // the constant's first element and its one pair (scalar form)
};
inline const char* eltwise_table_refusal(const tamd_eltwise_param* p, int dtype, int c_dtype, const EltwiseValues& v, unsigned char* table)
{
    float s = 0.f;
    if (c_dtype >= 0 && tamd_eltwise_scalar(c_dtype, v.c_data, v.c_scale, v.c_zp, &s)) return "Eltwise: the constant's value cannot be read";
    unsigned char map[256];
    const int rc = tamd_eltwise_table(p->type, dtype, p, s, v.x_scale, v.x_zp, v.out_scale, v.out_zp, map);
    if (rc == -2) return "Eltwise: the table holds a value the reference does not define (NaN, infinite or outside int before its conversion)";
    if (rc) return "Eltwise: the reference's quantised kernels have no case for this type";
    if (table) for (int b = 0; b < 256; b++) table[b] = map[b];
    return nullptr;
}
inline const char* eltwise_refusal(const tamd_eltwise_param* p, int dtype, int input_num, int a_dim_num, const int* a_dims, bool a_const, size_t a_quant, int b_dim_num,
                                   const int* b_dims, bool b_const, size_t b_quant, size_t out_quant, int* gated, int b_dtype = -1, const EltwiseValues* v = nullptr,
                                   unsigned char* table = nullptr)
{
    *gated = kEltSame;
    if (!p) return "Eltwise needs its parameter";
    const bool quantised = chan_gate_on_device(dtype);
    if (p->type == 3) return "Eltwise SUM_SCALAR: alone of the scalar and unary types it has no case in either quantised kernel of the reference";
    if (p->type == 9) return "Eltwise LAST is no operator: of the scalar and unary types only those with a case in the reference run on the device";
    if (p->type == 16) return "Eltwise POW does not run on the device: its one-element loops in the reference run over the wrong count";
    if (eltwise_unary_type(p->type)) {
        if (input_num != 1) return "the scalar and unary Eltwise types run in their own form only: a unary type takes one input";
        if (!quantised) return "the scalar and unary forms of Eltwise run on the device in int8 and uint8 graphs only";
        if (a_const) return "Eltwise: the input of a unary type must not be a constant";
        if (a_dim_num != 4) return "the scalar and unary forms of Eltwise take a 4-D activation";
        if (a_quant != 1 || out_quant != 1) return "the scalar and unary forms of Eltwise need per-tensor quant params on both sides";
        if (v) { const char* why = eltwise_table_refusal(p, dtype, -1, *v, table); if (why) return why; }
        *gated = kEltUnary;
        return nullptr;
    }
    if (input_num != 2) return "Eltwise runs on the device on two tensors";
    auto elems = [](int n, const int* d) { size_t e = 1; for (int i = 0; i < n; i++) e *= (size_t)d[i]; return e; };
    const size_t ea = elems(a_dim_num, a_dims), eb = elems(b_dim_num, b_dims);
    if (a_const && ea == 1 && !b_const) return "an Eltwise whose one-element constant is listed first does not run on the device";
    if (b_const && eb == 1 && !a_const) {
        if (!quantised) return "the scalar and unary forms of Eltwise run on the device in int8 and uint8 graphs only";
        if (p->type == 6) return "Eltwise MAX with a one-element operand does not run on the device: the reference reads in1[i] past its end";
        if (!eltwise_scalar_type(p->type)) return "Eltwise: the reference's quantised kernels have no case for this type with a one-element operand";
        if (a_dim_num != 4) return "the scalar and unary forms of Eltwise take a 4-D activation";
        if (a_quant != 1 || out_quant != 1) return "the scalar and unary forms of Eltwise need per-tensor quant params on both sides";
        if (dtype == TAMD_DT_INT8 && b_dtype == TAMD_DT_FP32) return "an int8 Eltwise reads its constant as int8: an fp32 constant does not run on the device";
        if (dtype == TAMD_DT_INT8 ? b_dtype != TAMD_DT_INT8 : (b_dtype != TAMD_DT_UINT8 && b_dtype != TAMD_DT_FP32))
            return "Eltwise: the one-element constant must be uint8 or fp32 in a uint8 graph, int8 in an int8 graph";
        if (b_dtype != TAMD_DT_FP32 && b_quant != 1) return "Eltwise: a quantised one-element constant needs one (scale, zero point) pair";
        if (v && v->c_data) { const char* why = eltwise_table_refusal(p, dtype, b_dtype, *v, table); if (why) return why; }
        *gated = kEltScalar;
        return nullptr;
    }
    bool same = a_dim_num == b_dim_num;
    for (int i = 0; same && i < a_dim_num; i++) same = a_dims[i] == b_dims[i];
    if (!eltwise_type_on_device(p->type)) {
        if ((ea == 1 || eb == 1) && !a_const && !b_const) return "an Eltwise with a one-element operand that is not a constant does not run on the device";
        return "the scalar and unary Eltwise types run in their own form only: a 4-D activation, then a constant of one element";
    }
    if (a_const || b_const) return "Eltwise: neither operand may be a constant";
    if (same) return nullptr;                                     // PROD, SUM, SUB, MAX of two tensors of one shape, every graph type
    const int big = ea >= eb ? 0 : 1;
    const int xn = big ? b_dim_num : a_dim_num, gn = big ? a_dim_num : b_dim_num;
    const int* xd = big ? b_dims : a_dims;
    const int* gd = big ? a_dims : b_dims;
    const size_t eg = big ? ea : eb;
    if (!chan_gate_on_device(dtype)) return "Eltwise operands of different shapes run on the device in int8 and uint8 graphs only";
    if (ea == eb) return "Eltwise operands of one size and different shapes do not run on the device";
    if (eg == 1) return "an Eltwise with a one-element operand does not run on the device";
    if (p->type == 6) return "Eltwise MAX has no channel-gate form: the reference reads past the gate's end";
    if (xn != 4 || (size_t)xd[2] * xd[3] <= 1) return "a gated Eltwise operand must be 4-D (N, C, H, W) with H * W > 1";
    if (eg != (size_t)xd[0] * xd[1]) {
        const size_t ghw = gn >= 2 ? (size_t)gd[gn - 2] * gd[gn - 1] : gn == 1 ? (size_t)gd[0] : 0;      // (run(): input_hw_1)
        if (ghw == (size_t)xd[2] * xd[3]) return "the row form of Eltwise (input_hw == input_hw_1) does not run on the device";
        return "Eltwise operands of different shapes: the smaller one must be a channel gate (N, C, 1, 1)";
    }
    if (gn != 4 || gd[0] != xd[0] || gd[1] != xd[1] || gd[2] != 1 || gd[3] != 1) return "an Eltwise gate must be 4-D with dims exactly (N, C, 1, 1)";
    if (a_quant != 1 || b_quant != 1 || out_quant != 1) return "a gated Eltwise needs per-tensor quant params on all three tensors";
    if (big == 1 && xd[0] != 1) return "an Eltwise gate listed first is defined for batch 1 only";
    *gated = big;
    return nullptr;
}

// BatchNorm: the uint8 kernel of the reference (batchnorm_kernel_ref_uint8.c:40-107; chan_lut.hip, prelu.hip).  There is no int8 kernel
// (run() writes nothing), and fp32 graphs keep the node on the CPU device
inline bool batchnorm_on_device(int dtype) { return dtype == TAMD_DT_UINT8; }
// one of the four statistics of a BatchNorm node (inputs 1 .. 4: gamma, beta, mean, var); data: its payload where the caller has it
struct BnStat { int dtype; bool is_const; size_t elems; const float* data; };
// One BatchNorm node: nullptr when the device runs it, else the reason.  st[4]: gamma, beta, mean, var.  v (may be null): the scales and
// zero points of x and of the output; with them and every payload the C tables are built (tables: [C][64] dwords, may be null) and a
// channel whose s1 / s2 or table is not finite refuses the node: the reference's (int) conversion is undefined there.
//  - 2-D [N,C], 3-D [N,C,W], 4-D [N,C,H,W]: the three cases of batchnorm_ref.c:117-141; any other rank fails there
//  - caffe_flavor: gamma and beta are never read (prerun :88-95), so only mean and var must be fp32 constants of C elements
inline const char* batchnorm_refusal(const tamd_batchnorm_param* p, int dtype, int input_num, int x_dim_num, const int* x_dims, bool x_const, size_t x_quant,
                                     size_t out_quant, const BnStat* st, const EltwiseValues* v, std::vector<unsigned>* tables)
{
    if (!p) return "BatchNorm needs its parameter";
    if (dtype == TAMD_DT_INT8) return "BatchNorm does not run on the device in int8 graphs: the reference has no int8 kernel";
    if (!batchnorm_on_device(dtype)) return "BatchNorm runs on the device in uint8 graphs only";
    if (input_num != 5) return "BatchNorm takes five inputs: the data, gamma, beta, mean and var";
    if (x_dim_num < 2 || x_dim_num > 4) return "BatchNorm runs on a 2-D [N,C], 3-D [N,C,W] or 4-D [N,C,H,W] tensor only";
    if (x_const) return "BatchNorm: the data tensor must not be a constant";
    if (x_quant != 1 || out_quant != 1) return "BatchNorm needs per-tensor quant params on both sides";
    for (int i = 0; i < x_dim_num; i++) if (x_dims[i] < 1) return "BatchNorm: every dimension must be at least 1";
    const size_t C = (size_t)x_dims[1];
    for (int k = p->caffe_flavor ? 2 : 0; k < 4; k++)
        if (st[k].dtype != TAMD_DT_FP32 || !st[k].is_const || st[k].elems != C) return "BatchNorm: gamma, beta, mean and var must be fp32 constants of C elements";
    bool values = v != nullptr;
    for (int k = p->caffe_flavor ? 2 : 0; k < 4; k++) values = values && st[k].data;
    if (!values) return nullptr;
    if (tables) tables->assign(C * 64, 0u);
    unsigned char map[256];
    for (size_t c = 0; c < C; c++) {
        const float gamma = p->caffe_flavor ? 1.f : st[0].data[c], beta = p->caffe_flavor ? 0.f : st[1].data[c];
        if (tamd_batchnorm_table(p, gamma, beta, st[2].data[c], st[3].data[c], v->x_scale, v->x_zp, v->out_scale, v->out_zp, map))
            return "BatchNorm: a channel's s1 / s2 or table is not finite (the reference's conversion to int is undefined there)";
        if (tables) for (int b = 0; b < 256; b++) ((unsigned char*)tables->data())[c * 256 + b] = map[b];
    }
    return nullptr;
}

// Permute: NCHW -> NHWC, the one order SSD heads use (Permute -> Flatten -> Concat)
inline bool permute_order_on_device(const int* o) { return o[0] == 0 && o[1] == 2 && o[2] == 3 && o[3] == 1; }

// uint8 FC: fc_u8 keeps the dequantised input row of one image in LDS as floats (u8_kernels.hip: xrow), 4 bytes per value, inside
// the 64 KB a block may take
inline bool fc_u8_row_fits_lds(size_t hidden) { return hidden * 4 <= 60000; }

// int8 implicit GEMM: the (ky, kx) offsets of a kernel window sit in an LDS table of 128 entries (conv_igemm.hip: tap_lut).  The
// first-layer, depthwise and generic direct forms have no such table.
inline bool conv_i8_gemm_taps_fit(int kernel_h, int kernel_w) { return kernel_h * kernel_w <= 128; }

// int8 softmax: the exponentials of one axis live in LDS as floats (kSoftmaxI8MaxC, kernels.h)
inline bool softmax_i8_axis_fits(int len) { return len >= 1 && len <= kSoftmaxI8MaxC; }

// Upsample: nearest neighbour by a whole factor >= 1 (upsample_ref.c indexes with 1 / scale; the device kernels take an int, and
// shape inference multiplies by it)
inline bool upsample_factor_on_device(float scale) { return scale >= 1.f && scale == (float)(int)scale; }

// Sigmoid / Clip / HardSwish / Mish: byte maps through a 256-entry table (lut_tables.cc builds it, misc_kernels.hip: lut_u8 applies it).
// Which (operator, type) pairs run there is lut_op_on_device (lut_tables.h: the list of table builders itself)
inline bool is_lut_op(int op) { return op == TAMD_OP_SIGMOID || op == TAMD_OP_CLIP || op == TAMD_OP_HARDSWISH || op == TAMD_OP_MISH; }
// Mish: mish_kernel_ref_uint8.c:43-51 sizes its loops from dims[0..3] -- on a tensor of another rank the reference reads dimensions that
// are not there, and there are no bytes to equal; the other three kernels run over elem_num
inline bool lut_rank_on_device(int op, int dim_num) { return op != TAMD_OP_MISH || dim_num == 4; }

// Interp: the nearest mode of the two quantised kernels (interp_ref.c; interp.hip).  fp32 graphs keep the node on the CPU device
inline bool interp_on_device(int dtype) { return dtype == TAMD_DT_INT8 || dtype == TAMD_DT_UINT8; }
// .. and one node of it: nullptr when the device runs it (*geom: the scales and the output size, interp_tables.h; *iy / *ix: the source
// row of every output row, the source column of every output column), else the reason.  in_dims: the input's shape; in_quant /
// out_quant: how many (scale, zero point) pairs the two tensors carry.  interp_ref.c reads dims[2] and dims[3] and nothing else, so the
// tensor is 4-D; bilinear (resize_type 2 | 4) is undefined at batch > 1 there and is not built; an index outside the input is a read
// out of bounds in the reference: no bytes to equal
inline const char* interp_refusal(const tamd_interp_param* p, int dtype, int in_dim_num, const int* in_dims, bool in_const, size_t in_quant,
                                  size_t out_quant, InterpGeom* geom, std::vector<int>* iy, std::vector<int>* ix)
{
    if (!p) return "Interp needs its parameter";
    if (!interp_on_device(dtype)) return "Interp runs on the device in int8 and uint8 graphs only";
    if (p->resize_type != 1) return "only nearest Interp (resize_type 1) runs on the device";
    if (in_dim_num != 4 || in_const) return "Interp takes a 4-D tensor that is not a constant";
    if (in_quant != 1 || out_quant != 1) return "Interp needs per-tensor quant params on both sides";
    if (!interp_resolve(*p, in_dims[2], in_dims[3], geom)) return "Interp: the reference does not keep this output size when it infers the shape again";
    iy->resize((size_t)geom->out_h); ix->resize((size_t)geom->out_w);
    if (tamd_interp_indices(in_dims[2], geom->out_h, geom->height_scale, iy->data()) || tamd_interp_indices(in_dims[3], geom->out_w, geom->width_scale, ix->data()))
        return "Interp: a source index leaves the input";
    return nullptr;
}

// Split and ShuffleChannel: byte movers of the quantised graphs (split_ref.c, shuffle_channel_ref.c; chanmap.hip).  fp32 graphs keep both
// on the CPU device
inline bool chanmap_on_device(int dtype) { return dtype == TAMD_DT_INT8 || dtype == TAMD_DT_UINT8; }
// One Split node: nullptr when the device runs it, else the reason.  out_quant: the (scale, zero point) pair count of every output.
//  - is_caffe (num -1): every output is a full copy of the input -- not a channel mover, it stays on the CPU device
//  - no split_sizes (num 0): split.c:80-117 gives every output the INPUT's shape, and the kernel then copies past the input's end
//  - axis 1 only: split.c:60 indexes the shape with the axis as it stands, so -3 reads in front of the array there
//  - uint8 at batch > 1: ref_split_uint8 ignores out_offset (:99 writes output_data[i]) and leaves images 1.. unwritten
inline const char* split_refusal(const tamd_split_param* p, int dtype, int in_dim_num, const int* in_dims, bool in_const, size_t in_quant, int output_num,
                                 const size_t* out_quant)
{
    if (!p) return "Split needs its parameter";
    if (!chanmap_on_device(dtype)) return "Split runs on the device in int8 and uint8 graphs only";
    if (p->num == -1) return "an is_caffe Split (every output a full copy) does not run on the device";
    if (p->num == 0) return "a Split without split_sizes does not run on the device";
    if (in_dim_num != 4 || in_const) return "Split takes a 4-D tensor that is not a constant";
    if (p->axis != 1) return "Split runs on the device along the channel axis (axis 1) only";
    if (p->num < 1 || p->num > TAMD_SPLIT_MAX || p->num != output_num) return "Split: between 1 and 8 split_sizes, one per output";
    long sum = 0;
    for (int i = 0; i < p->num; i++) {
        if (p->sizes[i] < 1) return "Split: every size must be at least 1";
        sum += p->sizes[i];
    }
    if (sum != in_dims[1]) return "Split: the sizes do not add up to the input's channels";
    if (in_quant != 1) return "Split needs per-tensor quant params on every tensor";
    for (int i = 0; i < output_num; i++)
        if (out_quant[i] != 1) return "Split needs per-tensor quant params on every tensor";
    if (dtype == TAMD_DT_UINT8 && in_dims[0] != 1) return "a uint8 Split is defined for batch 1 only";
    return nullptr;
}
// One ShuffleChannel node.  channels % group != 0: the reference never writes the last channels, no bytes to equal
inline const char* shuffle_refusal(const tamd_shufflechannel_param* p, int dtype, int in_dim_num, const int* in_dims, bool in_const, size_t in_quant,
                                   size_t out_quant)
{
    if (!p) return "ShuffleChannel needs its parameter";
    if (!chanmap_on_device(dtype)) return "ShuffleChannel runs on the device in int8 and uint8 graphs only";
    if (in_dim_num != 4 || in_const) return "ShuffleChannel takes a 4-D tensor that is not a constant";
    if (p->group < 1 || in_dims[1] < 1 || in_dims[1] % p->group != 0) return "ShuffleChannel: the group count must divide the channels";
    if (in_quant != 1 || out_quant != 1) return "ShuffleChannel needs per-tensor quant params on both sides";
    return nullptr;
}

// Slice: the onnx form of a uint8 graph (slice_ref.c; slice.hip).  The reference has no int8 kernel (its run fails), and fp32 graphs keep
// the node on the CPU device
inline bool slice_on_device(int dtype) { return dtype == TAMD_DT_UINT8; }
// what slice_refusal resolves for its callers: the strided box along the one axis that is cut, the output's dims, and whether the node
// is the reference's raw copy (out dims == in dims: a memcpy, no requantisation whatever the parameters, slice_ref.c:440-445)
struct SliceGeom {
    int axis, start, stop, step;
    int out_dims[4];
    bool raw_copy;
};
// One Slice node: nullptr when the device runs it (*geom resolved, table[256]: the byte map between the two tensors, the identity for
// the raw copy; table may be null), else the reason.  p is what the reference holds AFTER its infer_shape: axis in [0, 4), or as a file
// stores it (negative: counted from the back, slice.c:52-53).  out_dims: the output's dims where the caller has them (null: not checked).
//  - caffe form: outputs 1.. get floats written into byte tensors (slice_ref.c:494-505 requantises output 0 only); mxnet: the 4-D
//    branch copies start_3 - stop_3 bytes, a negative length; tf: its own off-by-one -- no bytes to equal in any of them
//  - begin >= stop: infer_shape turns an extent of 0 into the input's dimension and a negative one into a negative dimension
//  - begin < 0, step < 0: the reference indexes in front of the input, or never ends
inline const char* slice_refusal(const tamd_slice_param* p, int dtype, int in_dim_num, const int* in_dims, bool in_const, size_t in_quant, float in_scale, int in_zp,
                                 int output_num, size_t out_quant, float out_scale, int out_zp, int out_dim_num, const int* out_dims, SliceGeom* geom,
                                 unsigned char* table)
{
    if (!p) return "Slice needs its parameter";
    if (!slice_on_device(dtype)) return "Slice runs on the device in uint8 graphs only";
    if (p->iscaffe) return "the caffe form of Slice (slice points, several outputs) does not run on the device";
    if (p->ismxnet) return "the mxnet form of Slice does not run on the device";
    if (!p->isonnx) return "the tf form of Slice (begin and size vectors) does not run on the device";
    if (output_num != 1) return "Slice runs on the device with one output only";
    if (in_dim_num != 4) return "Slice runs on the device on a 4-D tensor only";
    if (in_const) return "Slice: the input must not be a constant";
    if (in_quant != 1 || out_quant != 1) return "Slice needs per-tensor quant params on both sides";
    for (int i = 0; i < 4; i++)
        if (in_dims[i] < 1) return "Slice: every input dimension must be at least 1";
    int axis = p->axis;
    if (axis < -4 || axis >= 4) return "Slice: the axis is outside the tensor's rank";
    axis = (axis + 4) % 4;                                        // slice.c:52-53
    if (p->step < 0) return "Slice: a negative step does not run on the device";
    if (p->begin < 0) return "Slice: a negative begin does not run on the device";
    const int dim = in_dims[axis];
    const int end = p->end > dim ? dim : p->end;                  // slice.c:124-128 clips, and run() reads the clipped value
    const int stop = end > 0 ? end : dim + end;                   // slice_ref.c:248-251
    const int step = p->step > 1 ? p->step : 1;
    if (p->begin >= stop) return "Slice: begin is not below the resolved end (an empty or negative extent)";
    SliceGeom sg;
    sg.axis = axis; sg.start = p->begin; sg.stop = stop; sg.step = step;
    for (int i = 0; i < 4; i++) sg.out_dims[i] = in_dims[i];
    sg.out_dims[axis] = (stop - p->begin - 1) / step + 1;         // slice.c:131-145, the same count the element loops of onnx_run write
    sg.raw_copy = sg.out_dims[axis] == dim;
    if (out_dims) {
        if (out_dim_num != 4) return "Slice: the output does not have the dims the reference infers";
        for (int i = 0; i < 4; i++)
            if (out_dims[i] != sg.out_dims[i]) return "Slice: the output does not have the dims the reference infers";
    }
    unsigned char map[256];
    if (sg.raw_copy) {
        for (int b = 0; b < 256; b++) map[b] = (unsigned char)b;
    } else if (tamd_slice_table(in_scale, in_zp, out_scale, out_zp, map)) {
        return "Slice: the quantisation parameters give a value the reference cannot convert to int";
    }
    if (table) for (int b = 0; b < 256; b++) table[b] = map[b];
    if (geom) *geom = sg;
    return nullptr;
}

// Transpose: the two quantised kernels of the reference (transpose_ref.c; transpose.hip).  fp32 graphs keep the node on the CPU device
inline bool transpose_on_device(int dtype) { return dtype == TAMD_DT_INT8 || dtype == TAMD_DT_UINT8; }
// what transpose_refusal resolves for its callers: the output's dims as the reference infers them (out_dims[i] = in_dims[order[i]]) and
// the CANONICAL geometry of the move -- nd (extent, input stride) pairs in output order, outermost first: axes of size 1 are dropped,
// and output axes that are neighbours in the input too (stride[i] == extent[i + 1] * stride[i + 1]) are merged into one.  unit: which of
// them carries input stride 1, -1: none (a source whose innermost axis is padded and of size 1).  One element: nd 1, extent 1
struct TransposeGeom {
    int rank;
    int out_dims[8];
    int nd;
    int extent[6];
    long stride[6];
    int unit;
};
// the canonical geometry of reading a tensor of `rank` axes (in_dims, in_strides: elements per step of every INPUT axis, any layout) in
// the order `order`.  The dense strides give what transpose_refusal resolves; the int8 planner calls it again with the strides of a
// convolution-stack buffer (n: H * W * cs, c: 1, h: W * cs, w: cs)
inline void transpose_canon(int rank, const int* in_dims, const long* in_strides, const int* order, TransposeGeom* g)
{
    int nd = 0;
    for (int i = 0; i < rank; i++) {
        const int e = in_dims[order[i]];
        const long s = in_strides[order[i]];
        if (e == 1) continue;
        if (nd > 0 && g->stride[nd - 1] == (long)e * s) { g->extent[nd - 1] *= e; g->stride[nd - 1] = s; }
        else { g->extent[nd] = e; g->stride[nd] = s; nd++; }
    }
    if (nd == 0) { g->extent[0] = 1; g->stride[0] = 1; nd = 1; }
    g->nd = nd; g->unit = -1;
    for (int i = 0; i < nd; i++) if (g->stride[i] == 1) g->unit = i;
    for (int i = nd; i < 6; i++) { g->extent[i] = 1; g->stride[i] = 0; }
}
// One Transpose node: nullptr when the device runs it (*geom resolved for a dense input, table[256]: the byte map between the two
// tensors; either may be null), else the reason.  out_dims: the output's dims where the caller has them (null: not checked).
//  - rank 2 .. 6: run() switches on the INPUT's rank and has a loop nest for these five; for any other the output is quantised from
//    memory nobody wrote
//  - a tr_shape of another length: infer_shape gives the output tr_shape_size dims while the loops index permute[0 .. rank - 1] -- past
//    the vector, or short of the tensor
//  - a repeated or out-of-range entry: the loops read outside the input or leave output elements unwritten
inline const char* transpose_refusal(const tamd_transpose_param* p, int dtype, int in_dim_num, const int* in_dims, bool in_const, size_t in_quant, float in_scale,
                                     int in_zp, size_t out_quant, float out_scale, int out_zp, int out_dim_num, const int* out_dims, TransposeGeom* geom,
                                     unsigned char* table)
{
    if (!p) return "Transpose needs its parameter";
    if (!transpose_on_device(dtype)) return "Transpose runs on the device in int8 and uint8 graphs only";
    if (in_dim_num == 1) return "a Transpose of a 1-D tensor does not run on the device (the reference has no loop for rank 1)";
    if (in_dim_num > 6) return "a Transpose of a tensor of more than 6 dimensions does not run on the device (the reference has no loop above rank 6)";
    if (in_dim_num < 1) return "Transpose: the input has no shape";
    if (p->dim_num != in_dim_num) return "Transpose: tr_shape must have one entry per input dimension";
    unsigned seen = 0;
    for (int i = 0; i < in_dim_num; i++) {
        if (p->order[i] < 0 || p->order[i] >= in_dim_num) return "Transpose: a tr_shape entry is outside the tensor's rank";
        if (seen & 1u << p->order[i]) return "Transpose: tr_shape repeats an axis (it is not a permutation)";
        seen |= 1u << p->order[i];
    }
    if (in_const) return "Transpose: the input must not be a constant";
    if (in_quant != 1 || out_quant != 1) return "Transpose needs per-tensor quant params on both sides";
    size_t elems = 1;
    for (int i = 0; i < in_dim_num; i++) {
        if (in_dims[i] < 1) return "Transpose: every input dimension must be at least 1";
        elems *= (size_t)in_dims[i];
        if (elems > 0x7fffffffu - 64) return "Transpose: the tensor has more than 2^31 elements";      // 32-bit positions in the kernels
    }
    TransposeGeom tg;
    tg.rank = in_dim_num;
    for (int i = 0; i < 8; i++) tg.out_dims[i] = i < in_dim_num ? in_dims[p->order[i]] : 0;        // transpose.c:45-48
    if (out_dims) {
        if (out_dim_num != in_dim_num) return "Transpose: the output does not have the dims the reference infers";
        for (int i = 0; i < in_dim_num; i++)
            if (out_dims[i] != tg.out_dims[i]) return "Transpose: the output does not have the dims the reference infers";
    }
    long strides[8];
    long s = 1;
    for (int i = in_dim_num - 1; i >= 0; i--) { strides[i] = s; s *= in_dims[i]; }
    transpose_canon(in_dim_num, in_dims, strides, p->order, &tg);
    unsigned char map[256];
    if (tamd_transpose_table(dtype, in_scale, in_zp, out_scale, out_zp, map)) return "Transpose: the quantisation parameters give a value the reference cannot convert to int";
    if (table) for (int b = 0; b < 256; b++) table[b] = map[b];
    if (geom) *geom = tg;
    return nullptr;
}

// Crop: the uint8 kernel of the reference (crop_ref.c:147-253).  There is no int8 kernel (run() writes nothing), and fp32 graphs keep the
// node on the CPU device
inline bool crop_on_device(int dtype) { return dtype == TAMD_DT_UINT8; }
// what crop_refusal resolves for its callers: the box of the data tensor that the output is, on N, C, H, W
struct CropGeom {
    int start[4], out_dims[4];
};
// One Crop node: nullptr when the device runs it (*geom resolved; may be null), else the reason.  x: input 0, the data; like: input 1, of
// which only the shape is read (crop.c:37).  out_dims: the output's dims where the caller has them (null: not checked).  The bytes are
// the data's own: no quantisation VALUE of either tensor is read, only that both carry one pair.
//  - num_args 1 (the centre crop): crop.c:37 takes input 1 unconditionally, and such a node has none
//  - any other flag, axis or num_args: ref_crop_uint8 has no branch for it and writes nothing
//  - a negative offset, or a box that leaves the data on any axis: the reference reads out of bounds (the caffe form has no guard at all;
//    the MXNet guard offset + out <= in, crop_ref.c:190, fails silently and leaves the output unwritten; neither form looks at C or N)
inline const char* crop_refusal(const tamd_crop_param* p, int dtype, int input_num, int x_dim_num, const int* x_dims, bool x_const, size_t x_quant, int like_dim_num,
                                const int* like_dims, size_t out_quant, int out_dim_num, const int* out_dims, CropGeom* geom)
{
    if (!p) return "Crop needs its parameter";
    if (!crop_on_device(dtype)) return "Crop runs on the device in uint8 graphs only";
    if (p->flag == 1 && p->num_args == 1) return "the centre crop (MXNet form, num_args 1) does not run on the device";
    if (p->flag != 0 && p->flag != 1) return "Crop: a flag other than 0 (caffe) and 1 (MXNet) has no kernel in the reference";
    if (p->flag == 1 && p->num_args != 2) return "Crop: the MXNet form runs with num_args 2 only";
    if (p->flag == 0 && p->axis != 1 && p->axis != 2) return "Crop: the caffe form runs with axis 1 or 2 only";
    if (input_num != 2) return "Crop takes two inputs: the data and the tensor whose shape it takes";
    if (x_dim_num != 4 || like_dim_num != 4) return "Crop runs on the device on 4-D tensors only";
    if (x_const) return "Crop: the data input must not be a constant";
    if (x_quant != 1 || out_quant != 1) return "Crop needs per-tensor quant params on the data and the output";
    CropGeom cg;
    cg.start[0] = 0;
    cg.start[1] = p->flag == 0 && p->axis == 1 ? p->offset_c : 0;
    cg.start[2] = p->offset_h;
    cg.start[3] = p->offset_w;
    for (int i = 0; i < 4; i++) {
        cg.out_dims[i] = like_dims[i];                            // crop.c:70-73: N and C of input 1 too
        if (x_dims[i] < 1 || like_dims[i] < 1) return "Crop: every dimension must be at least 1";
        if (cg.start[i] < 0) return "Crop: a negative offset does not run on the device";
    }
    if (like_dims[0] != x_dims[0]) return "Crop: the two inputs must have the same batch";
    for (int i = 1; i < 4; i++)
        if ((long)cg.start[i] + (long)cg.out_dims[i] > (long)x_dims[i]) return "Crop: the box leaves the data tensor";
    if (out_dims) {
        if (out_dim_num != 4) return "Crop: the output does not have the dims the reference infers";
        for (int i = 0; i < 4; i++)
            if (out_dims[i] != cg.out_dims[i]) return "Crop: the output does not have the dims the reference infers";
    }
    if (geom) *geom = cg;
    return nullptr;
}

// DepthToSpace: the two quantised kernels of the reference (depthtospace_ref.c; d2s.hip).  fp32 graphs keep the node on the CPU device
inline bool depthtospace_on_device(int dtype) { return dtype == TAMD_DT_INT8 || dtype == TAMD_DT_UINT8; }
// what depthtospace_refusal resolves for its callers: the block size, the output's dims as the reference infers them
// (N, C / r^2, H * r, W * r: depthtospace.c infer_shape) and the move as the SIX axes of x.reshape(N, outc, r, r, H, W) in the output's
// order (0, 1, 4, 2, 5, 3): view_dims[] and order[] are what transpose_canon takes (the form-0 baseline of the planners)
struct DepthToSpaceGeom {
    int r;
    int out_dims[4];
    int view_dims[6], order[6];
};
// One DepthToSpace node: nullptr when the device runs it (*geom resolved; may be null), else the reason.  out_dims: the output's dims
// where the caller has them (null: not checked).  The bytes are the input's own (depthtospace_ref.c reads no quantisation VALUE of either
// tensor, and the int8 byte -128 stays -128), so the two tensors' parameters may differ; only that both carry one pair is asked.
//  - another rank: run() indexes dims[0 .. 3] whatever the tensor has
//  - block_size < 1: the reference divides by it
//  - C % r^2 != 0: the reference computes outc = C / r^2 rounded down and silently drops the channels behind outc * r^2
inline const char* depthtospace_refusal(const tamd_depthtospace_param* p, int dtype, int in_dim_num, const int* in_dims, bool in_const, size_t in_quant, size_t out_quant,
                                        int out_dim_num, const int* out_dims, DepthToSpaceGeom* geom)
{
    if (!p) return "DepthToSpace needs its parameter";
    if (!depthtospace_on_device(dtype)) return "DepthToSpace runs on the device in int8 and uint8 graphs only";
    if (in_dim_num != 4) return "DepthToSpace runs on the device on 4-D tensors only";
    if (p->block_size < 1) return "DepthToSpace: the block size must be at least 1";
    for (int i = 0; i < 4; i++) if (in_dims[i] < 1) return "DepthToSpace: every dimension must be at least 1";
    const long r = p->block_size;
    if (r > 0x7fff || (long)in_dims[1] % (r * r) != 0) return "DepthToSpace: the channel count is not a multiple of the block size squared (the reference would drop channels)";
    if (in_const) return "DepthToSpace: the input must not be a constant";
    if (in_quant != 1 || out_quant != 1) return "DepthToSpace needs per-tensor quant params on both sides";
    const long oh = (long)in_dims[2] * r, ow = (long)in_dims[3] * r;
    if ((long)in_dims[0] * in_dims[1] > 0x7fffffffL - 64 || (long)in_dims[0] * in_dims[1] * in_dims[2] > 0x7fffffffL - 64
        || (long)in_dims[0] * in_dims[1] * in_dims[2] * in_dims[3] > 0x7fffffffL - 64 || oh > 0x7fffffffL - 64 || ow > 0x7fffffffL - 64)
        return "DepthToSpace: the tensor has more than 2^31 elements";                             // 32-bit positions in the kernels
    DepthToSpaceGeom dg;
    dg.r = (int)r;
    dg.out_dims[0] = in_dims[0]; dg.out_dims[1] = (int)(in_dims[1] / (r * r)); dg.out_dims[2] = (int)oh; dg.out_dims[3] = (int)ow;
    const int view[6] = {in_dims[0], dg.out_dims[1], (int)r, (int)r, in_dims[2], in_dims[3]}, order[6] = {0, 1, 4, 2, 5, 3};
    for (int i = 0; i < 6; i++) { dg.view_dims[i] = view[i]; dg.order[i] = order[i]; }
    if (out_dims) {
        if (out_dim_num != 4) return "DepthToSpace: the output does not have the dims the reference infers";
        for (int i = 0; i < 4; i++)
            if (out_dims[i] != dg.out_dims[i]) return "DepthToSpace: the output does not have the dims the reference infers";
    }
    if (geom) *geom = dg;
    return nullptr;
}

// Resize: the nearest mode of the two quantised kernels (resize_ref.c:261-381; interp.hip fed with Resize's operands, resize.hip).  fp32
// graphs keep the node on the CPU device
inline bool resize_on_device(int dtype) { return dtype == TAMD_DT_INT8 || dtype == TAMD_DT_UINT8; }
// what resize_refusal resolves for its callers: the output's dims as the reference infers them ((int)(H * scale_h), (int)(W * scale_w):
// resize.c:47-48), the source row of every output row and the source column of every output column (tamd_resize_indices), the byte map
// (tamd_resize_table; have_table: the caller gave the quantisation values) and, where the two index vectors ARE i / sh and j / sw for
// whole numbers sh, sw >= 1 with OH == H * sh and OW == W * sw, those two numbers (else 0, 0): the replicate form of resize.hip is legal
// exactly there -- decided on the vectors themselves, not on the scales
struct ResizeGeom {
    int out_dims[4];
    std::vector<int> iy, ix;
    unsigned char table[256];
    bool have_table;
    int sh, sw;
};
// the quantisation values of the two tensors, where the caller has them (a support query may not: then the table is not checked, and
// prerun refuses by name what the query let through)
struct ResizeQuant { float in_scale; int in_zp; float out_scale; int out_zp; };
// One Resize node: nullptr when the device runs it (*geom resolved; may be null), else the reason.  out_dims: the output's dims where the
// caller has them (null: not checked).
//  - batch > 1: run() calls the whole-tensor routine once per image, and that routine moves the channels of image 0 only; the floats of
//    the other images are an uninitialised malloc.  No bytes to equal
//  - type 1 (bilinear): reachable only from a graph built in memory -- the tm2 loader never reads the field -- and not built
//  - another rank: run() and infer_shape index dims[0 .. 3] whatever the tensor has
//  - a scale that is not finite and positive: the reference divides 1.f by it
//  - an output extent of 0: (int)(H * scale_h) with a small scale.  An extent outside int is undefined in the reference
//  - a table entry that is not finite or lies outside int before its conversion: undefined in the reference
// Every index lies inside the input by construction (T_MIN(.., h - 1), and a positive scale keeps it >= 0); tamd_resize_indices refuses
// a product that leaves int
inline const char* resize_refusal(const tamd_resize_param* p, int dtype, int in_dim_num, const int* in_dims, bool in_const, size_t in_quant, size_t out_quant,
                                  const ResizeQuant* q, int out_dim_num, const int* out_dims, ResizeGeom* geom)
{
    if (!p) return "Resize needs its parameter";
    if (!resize_on_device(dtype)) return "Resize runs on the device in int8 and uint8 graphs only";
    if (p->type == 1) return "only nearest Resize (type 0) runs on the device: bilinear stays on the CPU device";
    if (p->type != 0) return "Resize: the type is neither nearest (0) nor bilinear (1)";
    if (in_dim_num != 4) return "Resize runs on the device on 4-D tensors only";
    for (int i = 0; i < 4; i++) if (in_dims[i] < 1) return "Resize: every dimension must be at least 1";
    if (in_dims[0] != 1) return "Resize: the reference defines the operator for batch 1 only";
    if (in_const) return "Resize: the input must not be a constant";
    if (!(p->scale_h > 0.f) || !(p->scale_w > 0.f) || !isfinite(p->scale_h) || !isfinite(p->scale_w)) return "Resize: both scales must be finite and positive";
    if (in_quant != 1 || out_quant != 1) return "Resize needs per-tensor quant params on both sides";
    int oh = 0, ow = 0;
    if (!resize_out_extent(in_dims[2], p->scale_h, &oh) || !resize_out_extent(in_dims[3], p->scale_w, &ow)) return "Resize: an output extent lies outside int";
    if (oh < 1 || ow < 1) return "Resize: the output is empty";
    if ((double)in_dims[1] * in_dims[2] * in_dims[3] > (double)(0x7fffffffL - 64) || (double)in_dims[1] * oh * ow > (double)(0x7fffffffL - 64))
        return "Resize: the tensor has more than 2^31 elements";                                      // 32-bit positions in the kernels
    if (out_dims) {
        if (out_dim_num != 4 || out_dims[0] != 1 || out_dims[1] != in_dims[1] || out_dims[2] != oh || out_dims[3] != ow)
            return "Resize: the output does not have the dims the reference infers";
    }
    unsigned char table[256];
    if (q) {
        const int rc = tamd_resize_table(dtype, q->in_scale, q->in_zp, q->out_scale, q->out_zp, table);
        if (rc) return "Resize: a table entry is not finite or lies outside int (the reference's conversion is undefined there)";
    }
    ResizeGeom mine;
    if (!geom) geom = &mine;                                 // (a caller that wants nothing back: the index products are checked all the same)
    geom->iy.assign((size_t)oh, 0); geom->ix.assign((size_t)ow, 0);
    if (tamd_resize_indices(in_dims[2], oh, p->scale_h, geom->iy.data()) || tamd_resize_indices(in_dims[3], ow, p->scale_w, geom->ix.data())) return "Resize: a source index leaves int";
    geom->out_dims[0] = 1; geom->out_dims[1] = in_dims[1]; geom->out_dims[2] = oh; geom->out_dims[3] = ow;
    geom->have_table = q != nullptr;
    for (int b = 0; b < 256; b++) geom->table[b] = q ? table[b] : 0;
    int sh = oh % in_dims[2] == 0 ? oh / in_dims[2] : 0, sw = ow % in_dims[3] == 0 ? ow / in_dims[3] : 0;
    for (int i = 0; i < oh && sh; i++) if (geom->iy[(size_t)i] != i / sh) sh = 0;
    for (int j = 0; j < ow && sw; j++) if (geom->ix[(size_t)j] != j / sw) sw = 0;
    geom->sh = sh && sw ? sh : 0; geom->sw = sh && sw ? sw : 0;
    return nullptr;
}

// PReLU: the two quantised kernels of the reference (prelu_ref.c; prelu.hip).  fp32 graphs keep the node on the CPU device
inline bool prelu_on_device(int dtype) { return dtype == TAMD_DT_INT8 || dtype == TAMD_DT_UINT8; }
// One PReLU node: nullptr when the device runs it, else the reason.  input_num: the node's inputs ([data, slope]); slope_data: the
// slope's payload where the caller has it (a support query may not), slope_elems values.
//  - 4-D only: ref_prelu_int8 reads dims[0..3] whatever the rank, and the uint8 3-D per-channel loop (`for (j = 0; j < c; c++)`)
//    never ends; 2-D stays out with them
//  - int8: the kernel indexes slope[c] unconditionally and reads past a one-element slope; uint8: one element is the shared slope
//  - the slope is widened by tamd_prelu_slope; a NaN would reach the reference's (int) conversion -- refused, and the kernels are free
//    of that case
inline const char* prelu_refusal(int dtype, int input_num, int in_dim_num, const int* in_dims, bool in_const, size_t in_quant, size_t out_quant, int slope_dtype,
                                 bool slope_const, size_t slope_elems, const void* slope_data)
{
    if (!prelu_on_device(dtype)) return "PReLU runs on the device in int8 and uint8 graphs only";
    if (input_num != 2) return "PReLU takes two inputs, the data and the slope";
    if (in_const) return "PReLU: the data tensor must not be a constant";
    if (in_dim_num != 4) return "PReLU runs on the device on a 4-D tensor only";
    if (in_quant != 1) return "PReLU needs per-tensor quant params on its input";
    if (out_quant != 1) return "PReLU needs per-tensor quant params on its output";
    if (!slope_const) return "PReLU: the slope must be a constant";
    if (slope_dtype != TAMD_DT_FP16) return "PReLU: the slope of a quantised graph must be fp16";
    if (dtype == TAMD_DT_INT8 && slope_elems != (size_t)in_dims[1]) return "an int8 PReLU needs one slope per channel";
    if (dtype == TAMD_DT_UINT8 && slope_elems != (size_t)in_dims[1] && slope_elems != 1) return "a uint8 PReLU needs one slope per channel, or one for all";
    if (slope_data && !prelu_slopes_finite((const unsigned short*)slope_data, slope_elems)) return "PReLU: a slope widens to inf or NaN";
    return nullptr;
}

// InstanceNorm: the uint8 kernel of the reference (instancenorm_ref.c:101-183; instnorm.hip).  run() has an fp32 and a uint8 branch and
// nothing for int8; fp32 graphs keep the node on the CPU device
inline bool instancenorm_on_device(int dtype) { return dtype == TAMD_DT_UINT8; }
// gamma or beta of an InstanceNorm node (inputs 1, 2); data: its payload where the caller has it
struct InStat { int dtype; bool is_const; size_t elems; const float* data; };
// One InstanceNorm node: nullptr when the device runs it, else the reason.  st[2]: gamma, beta.  in_scale / out_scale / out_zp: the
// quantisation values where the caller has them (have_q); without them, or without both payloads, the bound is not checked and prerun
// refuses by name what a support query let through.
//  - 4-D only: ref_instancenorm_uint8 reads dims[0 .. 3] whatever the rank
//  - eps <= 0 or not finite: a constant plane has var 0 and a = gamma / sqrt(eps)
//  - the bound (instnorm_tables.h): where (255 * in_scale * max|gamma| / sqrt(eps) + max|beta|) / out_scale + |out_zp| reaches 2^30 a
//    plane may exist whose value leaves int before the reference's conversion, which is undefined there.  (The device conversion
//    saturates whatever the bound says.)
inline const char* instancenorm_refusal(const tamd_instancenorm_param* p, int dtype, int input_num, int x_dim_num, const int* x_dims, bool x_const, size_t x_quant,
                                        size_t out_quant, const InStat* st, bool have_q, float in_scale, float out_scale, int out_zp)
{
    if (!p) return "InstanceNorm needs its parameter";
    if (dtype == TAMD_DT_INT8) return "InstanceNorm does not run on the device in int8 graphs: the reference has no int8 kernel";
    if (!instancenorm_on_device(dtype)) return "InstanceNorm runs on the device in uint8 graphs only";
    if (input_num != 3) return "InstanceNorm takes three inputs: the data, gamma and beta";
    if (x_dim_num != 4) return "InstanceNorm runs on the device on a 4-D tensor only";
    if (x_const) return "InstanceNorm: the data tensor must not be a constant";
    if (x_quant != 1 || out_quant != 1) return "InstanceNorm needs per-tensor quant params on both sides";
    if (x_dims[0] < 1 || x_dims[1] < 1) return "InstanceNorm: batch and channels must be at least 1";
    if (x_dims[2] < 1 || x_dims[3] < 1) return "InstanceNorm: a plane is empty";
    if ((double)x_dims[2] * x_dims[3] > (double)(0x7fffffffL - 64) || (double)x_dims[0] * x_dims[1] > (double)0x7fffffffL) return "InstanceNorm: a plane of more than 2^31 bytes";
    if (!(p->eps > 0.f) || !isfinite(p->eps)) return "InstanceNorm: eps must be finite and positive";
    const size_t C = (size_t)x_dims[1];
    for (int k = 0; k < 2; k++)
        if (st[k].dtype != TAMD_DT_FP32 || !st[k].is_const || st[k].elems != C) return "InstanceNorm: gamma and beta must be fp32 constants of C elements";
    if (!st[0].data || !st[1].data) return nullptr;
    for (int k = 0; k < 2; k++)
        for (size_t c = 0; c < C; c++) if (!isfinite(st[k].data[c])) return "InstanceNorm: gamma and beta must be finite";
    if (!have_q) return nullptr;
    if (!(instancenorm_bound(st[0].data, st[1].data, C, p->eps, in_scale, out_scale, out_zp) < 1073741824.0))
        return "InstanceNorm: a value could leave int before the reference's conversion (the bound on |y / out_scale + out_zp| reaches 2^30)";
    return nullptr;
}

}  // namespace tamd
