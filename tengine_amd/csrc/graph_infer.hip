// Shape inference and graph validation of the device graph IR (restating source/operator/prototype/*.c), the PriorBox evaluator
// (priorbox_ref.c:53-213) and the library's error string.  Split out of graph.hip in round 6 (one 157 KB translation
// unit held planner, executor, allocator, plan cache and profiler); the units are listed in graph_internal.h.
#include "graph.h"
#include "graph_internal.h"
#include "env.h"

#include <stdarg.h>
#include <stddef.h>
#include <stdio.h>
#include <string.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <cfloat>
#include <chrono>
#include <cmath>
#include <mutex>

#include "epilogue.h"

namespace tamd {

// prerun (plan + hipGraph capture) and the device-synchronous frees are serialised process-wide: HIP rejects legacy-
// stream / synchronous operations of one host thread while another one captures (seen as "operation would make the
// legacy stream depend on a capturing blocking stream" under tools/exp/stress_threads.py).  run/launch are not affected.
std::mutex g_capture_mutex;

static thread_local char g_err[512] = "";
void set_error(const char* fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    if (getenv("TAMD_VERBOSE")) fprintf(stderr, "tengine_amd: %s\n", g_err);
}


// ---------------------------------------------------------------------------------------------
// shape inference (restating the reference's infer_shape functions)
// ---------------------------------------------------------------------------------------------
// pooling_param.h:59-105
static int pool_out_size(int input, int kernel, int stride, int pad, int caffe)
{
    int output = 1;
    if (pad >= 0) {
        if (caffe == 1) {
            output = 2 + cdiv_c(input - kernel + 2 * pad - 1, stride);
            if (pad > 0 && ((output - 1) * stride >= input + pad)) output--;
        } else if (caffe == 2)
            output = 1 + cdiv_c(input - kernel + pad, stride);
        else
            output = 1 + cdiv_c(input - kernel + 2 * pad, stride);
    } else
        output = 1 + cdiv_c(input - 1, stride);
    return output;
}
static void pool_real_pads(int out, int in, int kernel, int stride, int pad_org, int* pad0, int* pad1)
{
    int total = (out - 1) * stride + kernel;
    int pad_num = total - in;
    if (pad_num < 0) pad_num = 0;
    if (pad_org < 0) { *pad0 = pad_num / 2; *pad1 = pad_num - pad_org; }
    else { *pad0 = pad_org; *pad1 = pad_num - pad_org; }
}

// pooling.c:36-100
PoolGeom pool_geom(const tamd_pool_param& p, int h, int w)
{
    PoolGeom g{};
    int glob = p.global;
    if (p.kernel_h == h && p.kernel_w == w && p.pad_w0 == 0 && p.pad_w1 == 0 && p.pad_h0 == 0 && p.pad_h1 == 0) glob = 1;
    if (glob) { g = {1, 1, h, w, 1, 1, 0, 0}; return g; }
    int caffe = p.caffe_flavor & ~0x100;
    g.oh = pool_out_size(h, p.kernel_h, p.stride_h, p.pad_h0, p.caffe_flavor);
    g.ow = pool_out_size(w, p.kernel_w, p.stride_w, p.pad_w0, p.caffe_flavor);
    g.kh = p.kernel_h; g.kw = p.kernel_w; g.sh = p.stride_h; g.sw = p.stride_w;
    int d;
    if (caffe != 2) {
        pool_real_pads(g.oh, h, p.kernel_h, p.stride_h, p.pad_h0, &g.ph0, &d);
        pool_real_pads(g.ow, w, p.kernel_w, p.stride_w, p.pad_w0, &g.pw0, &d);
    } else { g.ph0 = p.pad_h0 / 2; g.pw0 = p.pad_w0 / 2; }
    return g;
}

// ---------------------------------------------------------------------------------------------
// PriorBox: the SSD anchor boxes depend on tensor SHAPES and node parameters only, so the node is evaluated
// once at prerun and its output tensor is a device constant; the reference recomputes the same numbers at every run
// (priorbox_ref.c:53-175).  Arithmetic types follow that file: sizes are truncated to int (:110,:121); the (min, max)
// prior is the double sqrt of the int product; ratio priors are int * | / double sqrt(ratio), stored as float; corners are
// (centre -+ size * 0.5f) / extent in float; a flipped prior swaps the sizes AND the extents it divides by (:146-150).
// ---------------------------------------------------------------------------------------------
int priorbox_count(const tamd_priorbox_param& p)
{
    return (1 + (p.max_size_num > 0 ? 1 : 0) + p.aspect_ratio_num * (p.flip ? 2 : 1)) * p.min_size_num;       // priorbox.c:37-64
}

void priorbox_eval(const tamd_priorbox_param& p, int feat_h, int feat_w, int data_h, int data_w, std::vector<float>* out)
{
    struct Prior { float w, h; bool flipped; };
    std::vector<Prior> cell;                                     // the priors of one feature-map cell, in output order
    for (int s = 0; s < p.min_size_num; s++) {
        const int mn = (int)p.min_size[s];
        cell.push_back({(float)mn, (float)mn, false});
        if (p.max_size_num > 0) {
            const float q = (float)std::sqrt((double)(mn * (int)p.max_size[s]));
            cell.push_back({q, q, false});
        }
        for (int r = 0; r < p.aspect_ratio_num; r++) {
            const double root = std::sqrt((double)p.aspect_ratio[r]);
            const Prior pr{(float)(mn * root), (float)(mn / root), false};
            cell.push_back(pr);
            if (p.flip) cell.push_back({pr.w, pr.h, true});
        }
    }
    const bool own_image = p.image_h != 0 && p.image_w != 0, own_step = p.step_h != 0 && p.step_w != 0;
    const float iw = (float)(own_image ? p.image_w : data_w), ih = (float)(own_image ? p.image_h : data_h);
    const float step_w = own_step ? p.step_w : iw / (float)feat_w, step_h = own_step ? p.step_h : ih / (float)feat_h;
    const size_t dim = (size_t)feat_h * feat_w * cell.size() * 4;
    out->assign(2 * dim, 0.f);
    float* o = out->data();
    for (int y = 0; y < feat_h; y++)
        for (int x = 0; x < feat_w; x++) {
            const float cx = ((float)x + p.offset) * step_w, cy = ((float)y + p.offset) * step_h;
            for (const Prior& pr : cell) {
                const float hx = (pr.flipped ? pr.h : pr.w) * 0.5f, hy = (pr.flipped ? pr.w : pr.h) * 0.5f;
                const float ex = pr.flipped ? ih : iw, ey = pr.flipped ? iw : ih;
                o[0] = (cx - hx) / ex; o[1] = (cy - hy) / ey; o[2] = (cx + hx) / ex; o[3] = (cy + hy) / ey;
                o += 4;
            }
        }
    if (p.clip)
        for (size_t i = 0; i < dim; i++) (*out)[i] = std::min(std::max((*out)[i], 0.f), 1.f);
    for (size_t i = 0; i < dim; i++) (*out)[dim + i] = p.variance[i & 3];
}

// its quantisation (priorbox_ref.c:178-213): uint8 truncates (int)(f / scale + zp); int8 rounds
void priorbox_quant_u8(const std::vector<float>& f, float scale, int zp, std::vector<uint8_t>* q)
{
    q->resize(f.size());
    for (size_t i = 0; i < f.size(); i++) {
        const int u = (int)(f[i] / scale + (float)zp);
        (*q)[i] = (uint8_t)std::min(std::max(u, 0), 255);
    }
}

// priorbox_ref.c:195-210: round(f / scale) -- C `round` on the float quotient promoted to double -- clamped to +-127
void priorbox_quant_i8(const std::vector<float>& f, float scale, std::vector<int8_t>* q)
{
    q->resize(f.size());
    for (size_t i = 0; i < f.size(); i++) {
        const int v = (int)round((double)(f[i] / scale));
        (*q)[i] = (int8_t)std::min(std::max(v, -127), 127);
    }
}

int infer_shapes(tamd_graph* g)
{
    for (auto& n : g->nodes) {
        if (n.op == TAMD_OP_INPUT || n.op == TAMD_OP_CONST) continue;
        if (n.in.empty() || n.out.empty()) { set_error("node %s has no io", n.name.c_str()); return -1; }
        HTensor& x = g->tensors[n.in[0]];
        HTensor& y = g->tensors[n.out[0]];
        switch (n.op) {
        case TAMD_OP_CONV: {   // convolution.c:35-145
            if (n.in.size() < 2) { set_error("conv %s: no weight tensor", n.name.c_str()); return -1; }
            if (x.dims.size() != 4) { set_error("conv %s: input is not 4-D", n.name.c_str()); return -1; }
            if (g->tensors[n.in[1]].dims.size() != 4) { set_error("conv %s: weight is not 4-D", n.name.c_str()); return -1; }
            tamd_conv_param& p = n.p.conv;
            if (p.kernel_w == 0) { p.kernel_w = 1; p.pad_w0 = p.pad_w1 = 0; }
            if (p.kernel_h == 0) p.kernel_h = 1;
            if (p.stride_w == 0) p.stride_w = 1;
            if (p.stride_h == 0) p.stride_h = 1;
            if (p.dilation_h == 0) p.dilation_h = 1;
            if (p.dilation_w == 0) p.dilation_w = 1;
            p.input_channel = x.dims[1];
            const HTensor& w = g->tensors[n.in[1]];
            int h = x.dims[2], wd = x.dims[3];
            // SAME codes (-1 | -2): the reference's infer_shape resolves them into conv_param with a pad_num that holds no dilation and
            // sizes the axis (in - 1) / stride + 1; at every run its node's reshape (conv_hcl_x86.c:196-240, conv_ref.c:115-160) then finds
            // pads >= 0 and takes the explicit formula below -- the same size at dilation 1, a smaller map with dilation.  That is the
            // map the reference computes, so it is the one computed here.
            if (p.pad_h0 < 0) {
                const int pad_num = (h - 1) / p.stride_h * p.stride_h + p.kernel_h - h;
                if (p.pad_h0 == -1) { p.pad_h0 = pad_num / 2; p.pad_h1 = pad_num - pad_num / 2; }
                else { p.pad_h1 = pad_num / 2; p.pad_h0 = pad_num - pad_num / 2; }
            }
            if (p.pad_w0 < 0) {
                const int pad_num = (wd - 1) / p.stride_w * p.stride_w + p.kernel_w - wd;
                if (p.pad_w0 == -1) { p.pad_w0 = pad_num / 2; p.pad_w1 = pad_num - pad_num / 2; }
                else { p.pad_w1 = pad_num / 2; p.pad_w0 = pad_num - pad_num / 2; }
            }
            const int oh = (h - p.dilation_h * (p.kernel_h - 1) - 1 + p.pad_h0 + p.pad_h1) / p.stride_h + 1;
            const int ow = (wd - p.dilation_w * (p.kernel_w - 1) - 1 + p.pad_w0 + p.pad_w1) / p.stride_w + 1;
            y.dims = {x.dims[0], w.dims[0], oh ? oh : 1, ow ? ow : 1};
            break;
        }
        case TAMD_OP_FC: {
            if (n.in.size() < 2 || g->tensors[n.in[1]].dims.empty() || x.dims.empty()) { set_error("fc %s: no weight tensor", n.name.c_str()); return -1; }
            int nout = n.p.fc.num_output ? n.p.fc.num_output : g->tensors[n.in[1]].dims[0];
            y.dims = {x.dims[0], nout};
            break;
        }
        case TAMD_OP_POOL: {
            PoolGeom pg = pool_geom(n.p.pool, x.dims[2], x.dims[3]);
            y.dims = {x.dims[0], x.dims[1], pg.oh, pg.ow};
            break;
        }
        case TAMD_OP_ELTWISE: {           // eltwise.c infer_shape: the dims of the operand with more elements (a channel gate may be listed first)
            const HTensor& big = n.in.size() > 1 && g->tensors[n.in[1]].elems() > x.elems() ? g->tensors[n.in[1]] : x;
            y.dims = big.dims;
            break;
        }
        case TAMD_OP_RELU: case TAMD_OP_RELU6: case TAMD_OP_DROPOUT: case TAMD_OP_SOFTMAX:
        case TAMD_OP_SIGMOID: case TAMD_OP_CLIP: case TAMD_OP_HARDSWISH: case TAMD_OP_MISH:
            y.dims = x.dims;
            break;
        case TAMD_OP_CONCAT: {
            int ax = n.p.concat.axis < 0 ? n.p.concat.axis + (int)x.dims.size() : n.p.concat.axis;
            y.dims = x.dims;
            int s = 0;
            for (int i : n.in) s += g->tensors[i].dims[ax];
            y.dims[ax] = s;
            break;
        }
        case TAMD_OP_UPSAMPLE: {
            int sc = (int)n.p.ups.scale;
            y.dims = {x.dims[0], x.dims[1], x.dims[2] * sc, x.dims[3] * sc};
            break;
        }
        case TAMD_OP_INTERP: {            // interp.c:51-67: by the scales when both are set, else the sizes (interp_tables.cc)
            InterpGeom geom;
            if (x.dims.size() != 4) { set_error("interp %s: input is not 4-D", n.name.c_str()); return -1; }
            if (!interp_resolve(n.p.interp, x.dims[2], x.dims[3], &geom)) { set_error("interp %s: the reference does not keep this output size when it infers the shape again", n.name.c_str()); return -1; }
            y.dims = {x.dims[0], x.dims[1], geom.out_h, geom.out_w};
            break;
        }
        case TAMD_OP_SPLIT: {             // split.c:57-78, the split_sizes form: output i takes sizes[i] of the axis.  Every other form is
            const tamd_split_param& sp = n.p.split;                    // refused HERE, by name (split_refusal), before a shape is made up for it
            std::vector<size_t> oq;
            for (int o : n.out) oq.push_back(g->tensors[o].scales.size());
            const char* why = split_refusal(&sp, x.dtype, (int)x.dims.size(), x.dims.data(), x.ttype == TAMD_TT_CONST, x.scales.size(), (int)n.out.size(), oq.data());
            if (why) { set_error("split %s: %s", n.name.c_str(), why); return -1; }
            for (int i = 0; i < sp.num; i++) g->tensors[n.out[i]].dims = {x.dims[0], sp.sizes[i], x.dims[2], x.dims[3]};
            break;
        }
        case TAMD_OP_SHUFFLECHANNEL: y.dims = x.dims; break;
        case TAMD_OP_SLICE: {             // slice.c:116-156, the onnx form: end clipped to the dimension, end <= 0 counted from the back,
            SliceGeom sg;                 // (extent - 1) / step + 1.  Every other form is refused HERE, by name (slice_refusal)
            const char* why = slice_refusal_of(g, n, false, &sg, nullptr);
            if (why) { set_error("slice %s: %s", n.name.c_str(), why); return -1; }
            y.dims.assign(sg.out_dims, sg.out_dims + 4);
            break;
        }
        case TAMD_OP_TRANSPOSE: {         // transpose.c:35-54: out.dims[i] = in.dims[tr_shape[i]].  What the device does not run is refused HERE, by name
            TransposeGeom tg;
            const char* why = transpose_refusal_of(g, n, false, &tg, nullptr);
            if (why) { set_error("transpose %s: %s", n.name.c_str(), why); return -1; }
            y.dims.assign(tg.out_dims, tg.out_dims + tg.rank);
            break;
        }
        case TAMD_OP_CROP: {              // crop.c:34-78: N, C, H, W of INPUT 1.  What the device does not run is refused HERE, by name (crop_refusal)
            CropGeom cg;
            const char* why = crop_refusal_of(g, n, false, &cg);
            if (why) { set_error("crop %s: %s", n.name.c_str(), why); return -1; }
            y.dims.assign(cg.out_dims, cg.out_dims + 4);
            break;
        }
        case TAMD_OP_INSTANCENORM: y.dims = x.dims; y.dtype = x.dtype; break;   // instancenorm.c: the input's shape; gamma and beta are fp32, the data is not
        case TAMD_OP_BATCHNORM: y.dims = x.dims; y.dtype = x.dtype; break;      // batchnorm.c: the input's shape; the statistics are fp32, the data is not
        case TAMD_OP_DEPTHTOSPACE: {      // depthtospace.c infer_shape: (N, C / r^2, H * r, W * r).  What the device does not run is refused HERE, by name
            DepthToSpaceGeom dg;
            const char* why = depthtospace_refusal_of(g, n, false, &dg);
            if (why) { set_error("depthtospace %s: %s", n.name.c_str(), why); return -1; }
            y.dims.assign(dg.out_dims, dg.out_dims + 4);
            break;
        }
        case TAMD_OP_RESIZE: {            // resize.c infer_shape: (N, C, (int)(H * scale_h), (int)(W * scale_w)).  What the device does not run is refused HERE, by name
            ResizeGeom rg;
            const char* why = resize_refusal_of(g, n, false, &rg);
            if (why) { set_error("resize %s: %s", n.name.c_str(), why); return -1; }
            y.dims.assign(rg.out_dims, rg.out_dims + 4);
            break;
        }
        case TAMD_OP_PRELU: y.dims = x.dims; y.dtype = x.dtype; break;      // prelu.c: the input's shape; the type is the data's, not the fp16 slope's
        case TAMD_OP_PERMUTE: {           // permute.c infer_shape: out.dims[i] = in.dims[order[i]]
            if (x.dims.size() != 4) { set_error("permute %s: only 4-D tensors", n.name.c_str()); return -1; }
            y.dims.resize(4);
            for (int i = 0; i < 4; i++) {
                const int o = n.p.perm.order[i];
                if (o < 0 || o > 3) { set_error("permute %s: bad order", n.name.c_str()); return -1; }
                y.dims[i] = x.dims[o];
            }
            break;
        }
        case TAMD_OP_RESHAPE: {           // the resolved shape travels in the parameter; only the batch may have been re-set
            const tamd_reshape_param& rp = n.p.reshape;
            if (rp.dim_num < 1 || rp.dim_num > 8) { set_error("reshape %s: bad shape", n.name.c_str()); return -1; }
            y.dims.assign(rp.dims, rp.dims + rp.dim_num);
            size_t rest = 1;
            for (int i = 1; i < rp.dim_num; i++) rest *= (size_t)std::max(1, rp.dims[i]);
            if (y.elems() != x.elems() && rest && x.elems() % rest == 0) y.dims[0] = (int)(x.elems() / rest);
            if (y.elems() != x.elems()) { set_error("reshape %s: element count changes", n.name.c_str()); return -1; }
            break;
        }
        case TAMD_OP_FLATTEN: {
            int f = 1;
            for (size_t i = 1; i < x.dims.size(); i++) f *= x.dims[i];
            y.dims = {x.dims[0], f};
            break;
        }
        case TAMD_OP_PRIORBOX: {          // priorbox.c:33-75: [n][2][feat_h * feat_w * num_priors * 4][1]
            const tamd_priorbox_param& pb = n.p.priorbox;
            if (x.dims.size() != 4 || n.in.size() < 2 || g->tensors[n.in[1]].dims.size() != 4) { set_error("priorbox %s: needs a 4-D feature map and the 4-D image tensor", n.name.c_str()); return -1; }
            if (pb.min_size_num < 1 || pb.min_size_num > TAMD_PRIORBOX_MAX || pb.aspect_ratio_num < 0 || pb.aspect_ratio_num > TAMD_PRIORBOX_MAX
                || (pb.max_size_num != 0 && pb.max_size_num != pb.min_size_num)) { set_error("priorbox %s: bad size / ratio counts", n.name.c_str()); return -1; }
            y.dims = {x.dims[0], 2, x.dims[2] * x.dims[3] * priorbox_count(pb) * 4, 1};
            break;
        }
        default:
            set_error("infer_shape: unsupported op %d (%s)", n.op, n.name.c_str());
            return -1;
        }
    }
    return 0;
}


// ---------------------------------------------------------------------------------------------
// validation: the model bytes may come off the wire (RCCL broadcast, tm2_reader.cc checks the container); the planners
// index constant payloads by operator parameters, so parameters and payload sizes are reconciled ONCE here -- a
// malformed graph fails prerun with a message instead of over-reading the host heap
// ---------------------------------------------------------------------------------------------
int validate_graph(tamd_graph* g)
{
    auto bad = [&](const HNode& n, const char* what) { set_error("%s: %s", n.name.c_str(), what); return -1; };
    for (auto& n : g->nodes) {
        // priorbox_ref.c fills image 0 of its output only (:99-175); what a batch > 1 tensor holds behind it is undefined there
        if (n.op == TAMD_OP_PRIORBOX && g->tensors[n.out[0]].dims[0] != 1) return bad(n, "PriorBox is defined for batch 1 only");
        // the uint8 / fp32 planners and infer_shapes take the factor as an int: 1.5 would run as 1, 0.5 would give an empty tensor
        if (n.op == TAMD_OP_UPSAMPLE && !upsample_factor_on_device(n.p.ups.scale)) return bad(n, "Upsample takes an integer factor >= 1");
        if (is_lut_op(n.op)) {
            const HTensor& x = g->tensors[n.in[0]];
            if (!lut_op_on_device(n.op, x.dtype)) return bad(n, "Sigmoid / Clip run on the device in int8 and uint8 graphs, HardSwish / Mish in uint8 graphs only");
            if (!lut_rank_on_device(n.op, (int)x.dims.size())) return bad(n, "Mish is defined for a 4-D tensor only");
            if (x.scales.empty() || g->tensors[n.out[0]].scales.empty()) return bad(n, "missing quant params");
        }
        if (n.op == TAMD_OP_INTERP) {
            const HTensor& x = g->tensors[n.in[0]];
            InterpGeom geom;
            std::vector<int> iy, ix;
            const char* why = interp_refusal(&n.p.interp, x.dtype, (int)x.dims.size(), x.dims.data(), x.ttype == TAMD_TT_CONST, x.scales.size(),
                                             g->tensors[n.out[0]].scales.size(), &geom, &iy, &ix);
            if (why) return bad(n, why);
        }
        if (n.op == TAMD_OP_SPLIT) {
            const HTensor& x = g->tensors[n.in[0]];
            std::vector<size_t> oq;
            for (int o : n.out) oq.push_back(g->tensors[o].scales.size());
            const char* why = split_refusal(&n.p.split, x.dtype, (int)x.dims.size(), x.dims.data(), x.ttype == TAMD_TT_CONST, x.scales.size(), (int)n.out.size(), oq.data());
            if (why) return bad(n, why);
        }
        if (n.op == TAMD_OP_SHUFFLECHANNEL) {
            const HTensor& x = g->tensors[n.in[0]];
            const char* why = shuffle_refusal(&n.p.shuffle, x.dtype, (int)x.dims.size(), x.dims.data(), x.ttype == TAMD_TT_CONST, x.scales.size(),
                                              g->tensors[n.out[0]].scales.size());
            if (why) return bad(n, why);
        }
        if (n.op == TAMD_OP_SLICE) {
            const char* why = slice_refusal_of(g, n, true, nullptr, nullptr);
            if (why) return bad(n, why);
        }
        if (n.op == TAMD_OP_CROP) {
            const char* why = crop_refusal_of(g, n, true, nullptr);
            if (why) return bad(n, why);
        }
        if (n.op == TAMD_OP_DEPTHTOSPACE) {
            const char* why = depthtospace_refusal_of(g, n, true, nullptr);
            if (why) return bad(n, why);
        }
        if (n.op == TAMD_OP_RESIZE) {
            const char* why = resize_refusal_of(g, n, true, nullptr);
            if (why) return bad(n, why);
        }
        if (n.op == TAMD_OP_TRANSPOSE) {
            const char* why = transpose_refusal_of(g, n, true, nullptr, nullptr);
            if (why) return bad(n, why);
        }
        if (n.op == TAMD_OP_INSTANCENORM) {
            const char* why = instancenorm_refusal_of(g, n);
            if (why) return bad(n, why);
        }
        if (n.op == TAMD_OP_BATCHNORM) {
            const char* why = batchnorm_refusal_of(g, n, nullptr);
            if (why) return bad(n, why);
        }
        if (n.op == TAMD_OP_PRELU) {
            const char* why = prelu_refusal_of(g, n);
            if (why) return bad(n, why);
        }
        if (n.op == TAMD_OP_ELTWISE) {
            int gated = -1;
            const char* why = eltwise_refusal_of(g, n, &gated);
            if (why) return bad(n, why);
        }
        if (n.op != TAMD_OP_CONV && n.op != TAMD_OP_FC) continue;
        const HTensor& x = g->tensors[n.in[0]];
        HTensor& w = g->tensors[n.in[1]];
        const HTensor& y = g->tensors[n.out[0]];
        if (w.ttype != TAMD_TT_CONST) return bad(n, "weights must be a constant tensor");
        const size_t es = (size_t)esize(w.dtype);
        size_t want = 0;
        int cout = 0;
        if (n.op == TAMD_OP_CONV) {
            const tamd_conv_param& p = n.p.conv;
            cout = y.dims[1];
            if (p.group < 1 || p.kernel_h < 1 || p.kernel_w < 1 || p.stride_h < 1 || p.stride_w < 1 || p.dilation_h < 1 || p.dilation_w < 1)
                return bad(n, "kernel / stride / dilation / group must be positive");
            if (x.dims[1] % p.group || cout % p.group) return bad(n, "group does not divide the channel counts");
            if (y.dims[2] < 1 || y.dims[3] < 1) return bad(n, "empty output map");
            want = (size_t)cout * (x.dims[1] / p.group) * p.kernel_h * p.kernel_w;
            if (w.dims[0] != cout) return bad(n, "weight dims[0] != output channels");
        } else {
            cout = y.dims[1];
            const size_t hidden = x.elems() / (size_t)std::max(1, x.dims[0]);
            want = (size_t)cout * hidden;
            // fc_ref.c:351-356 switches to a transposed read (need_trans) when weight dims[0] != num_output, but the operator's own
            // infer_shape (operator/prototype/fc.c:43-97) sizes the output from weight dims[0] and insists on dims[1] == hidden,
            // so a consistent model never gets there; such a node is refused here (the plugin leaves it to the CPU device)
            if (w.dims.size() != 2 || w.dims[0] != cout || (size_t)w.dims[1] != hidden) return bad(n, "fc weight must be [num_output][hidden]");
        }
        if (w.elems() != want || w.data.size() != want * es) return bad(n, "weight size does not match the operator parameters");
        if (!w.scales.empty() && w.scales.size() != 1 && w.scales.size() != (size_t)cout) return bad(n, "weight scale count is neither 1 nor the output channel count");
        if (n.in.size() > 2) {
            const HTensor& b = g->tensors[n.in[2]];
            if (b.ttype != TAMD_TT_CONST || b.elems() < (size_t)cout || b.data.size() < (size_t)cout * esize(b.dtype) || esize(b.dtype) != 4)
                return bad(n, "bias must be a constant of at least one 32-bit value per output channel");
        }
    }
    return 0;
}


const char* last_error() { return g_err; }

}  // namespace tamd
