// Native tmfile-v2 loader: the SAME bytes the reference's serializer consumes
// (source/serializer/tmfile/tm2_serializer.c:157-466 load_graph_tensors, :468-760 load_graph_nodes,
// :915-936 load_mem) become a tamd_graph, so a model file -- or the RCCL-broadcast copy of it -- needs
// no Tengine host to run on the device.  Format restated from tm2_format.h:267-477 (little-endian,
// uint32 offsets from the buffer start, 0 == not set).  Only NCHW models (graph_layout 0) are accepted;
// every offset is bounds-checked because the bytes may come off the wire.
#include <stdint.h>
#include <string.h>

#include <string>
#include <vector>

#include "graph.h"

namespace {

struct Reader {
    const uint8_t* b;
    size_t n;
    bool ok = true;
    bool in(size_t off, size_t len) const { return off <= n && len <= n - off; }
    uint32_t u32(size_t off)
    {
        if (!in(off, 4)) { ok = false; return 0; }
        uint32_t v;
        memcpy(&v, b + off, 4);
        return v;
    }
    int32_t i32(size_t off) { return (int32_t)u32(off); }
    float f32(size_t off)
    {
        uint32_t v = u32(off);
        float f;
        memcpy(&f, &v, 4);
        return f;
    }
    std::vector<uint32_t> vec(size_t off)
    {
        std::vector<uint32_t> r;
        if (off == 0) return r;
        uint32_t cnt = u32(off);
        if (!ok || !in(off + 4, (size_t)cnt * 4)) { ok = false; return r; }
        r.resize(cnt);
        memcpy(r.data(), b + off + 4, (size_t)cnt * 4);
        return r;
    }
    std::string str(size_t off)
    {
        if (off == 0) return "";
        uint32_t size = u32(off), d = u32(off + 4);
        if (!ok || !in(d, size)) { ok = false; return ""; }
        std::string s((const char*)b + d, size);
        size_t z = s.find('\0');
        if (z != std::string::npos) s.resize(z);
        return s;
    }
};

// TM2_OPTYPE_* (tm2_format.h:157-264) -> TAMD_OP_*
int map_op(uint32_t t)
{
    switch (t) {
    case 1: return TAMD_OP_BATCHNORM;                 // TM2_OPTYPE_BATCHNORMALIZATION: TM2_BatchNormParam; inputs [x, gamma, beta, mean, var]
    case 3: return TAMD_OP_CONCAT;
    case 4: return TAMD_OP_CONST;
    case 5: return TAMD_OP_CONV;
    case 8: return TAMD_OP_DROPOUT;
    case 9: return TAMD_OP_ELTWISE;
    case 10: return TAMD_OP_FLATTEN;
    case 11: return TAMD_OP_FC;
    case 12: return TAMD_OP_INPUT;
    case 15: return TAMD_OP_PERMUTE;
    case 16: return TAMD_OP_POOL;
    case 17: return TAMD_OP_PRELU;                     // TM2_OPTYPE_PRELU: no parameter blob; inputs [data, slope]
    case 18: return TAMD_OP_PRIORBOX;
    case 20: return TAMD_OP_RELU;
    case 21: return TAMD_OP_RELU6;
    case 23: return TAMD_OP_RESHAPE;
    case 27: return TAMD_OP_SLICE;
    case 28: return TAMD_OP_SOFTMAX;
    case 29: return TAMD_OP_SPLIT;
    case 37: return TAMD_OP_SIGMOID;
    case 51: return TAMD_OP_UPSAMPLE;
    case 54: return TAMD_OP_RESIZE;
    case 55: return TAMD_OP_SHUFFLECHANNEL;
    case 56: return TAMD_OP_CROP;
    case 66: return TAMD_OP_INSTANCENORM;             // TM2_OPTYPE_INSTANCENORM: TM2_InstanceNormParam {eps}; inputs [x, gamma, beta]
    case 70: return TAMD_OP_HARDSWISH;
    case 71: return TAMD_OP_INTERP;
    case 77: return TAMD_OP_TRANSPOSE;
    case 80: return TAMD_OP_DEPTHTOSPACE;
    case 87: return TAMD_OP_CLIP;
    case 97: return TAMD_OP_MISH;
    default: return -1;
    }
}

}  // namespace

extern "C" tamd_graph* tamd_graph_load_tm2(const void* mem, size_t size)
{
    using namespace tamd;
    Reader r{(const uint8_t*)mem, size};
    if (!mem || size < 16) { set_error("tm2: buffer too small"); return nullptr; }
    uint16_t ver_main;
    memcpy(&ver_main, r.b, 2);
    if (ver_main != 2) { set_error("tm2: unsupported file version %u", ver_main); return nullptr; }
    const uint32_t root = r.u32(8);                           // TM2_Header.offset_root
    const uint32_t vo_subgraphs = r.u32(root + 8);             // TM2_Model.offset_vo_subgraphs
    std::vector<uint32_t> subs = r.vec(vo_subgraphs);
    if (!r.ok || subs.empty()) { set_error("tm2: no subgraph"); return nullptr; }
    const size_t sg = subs[0];                                 // only subgraph 0 is read (tm2_serializer.c:93-99)
    const int graph_layout = r.i32(sg + 4);
    if (graph_layout != 0) { set_error("tm2: only NCHW models are supported"); return nullptr; }
    std::vector<uint32_t> in_nodes = r.vec(r.u32(sg + 12)), out_nodes = r.vec(r.u32(sg + 16));
    std::vector<uint32_t> nodes = r.vec(r.u32(sg + 20)), tensors = r.vec(r.u32(sg + 24)), buffers = r.vec(r.u32(sg + 28));
    if (!r.ok) { set_error("tm2: corrupt subgraph table"); return nullptr; }

    tamd_graph* g = tamd_graph_create();
    auto fail = [&](const char* msg) { set_error("tm2: %s", msg); tamd_graph_destroy(g); return (tamd_graph*)nullptr; };

    for (uint32_t to : tensors) {                              // TM2_Tensor
        const uint32_t buffer_id = r.u32(to + 4), dims_o = r.u32(to + 8), name_o = r.u32(to + 12), q_o = r.u32(to + 16);
        const int ttype = r.i32(to + 24), dtype = r.i32(to + 28);
        std::vector<uint32_t> dv = r.vec(dims_o);
        std::vector<uint32_t> qv = r.vec(q_o);
        std::string name = r.str(name_o);
        if (!r.ok || dv.size() > 8) return fail("corrupt tensor");
        tamd_tensor_desc d{};
        d.dtype = dtype; d.ttype = ttype; d.dim_num = (int)dv.size();
        size_t elems = 1;
        for (size_t i = 0; i < dv.size(); i++) { d.dims[i] = (int)dv[i]; elems *= (size_t)dv[i]; }
        std::vector<float> scales;
        std::vector<int> zps;
        for (uint32_t qo : qv) { zps.push_back(r.i32(qo)); scales.push_back(r.f32(qo + 4)); }   // TM2_QuantParam{zp, scale, width}
        d.quant_num = (int)scales.size(); d.scales = scales.data(); d.zero_points = zps.data();
        d.name = name.c_str();
        if (ttype == TAMD_TT_CONST) {
            if (buffer_id >= buffers.size()) return fail("bad buffer id");
            const uint32_t bsize = r.u32(buffers[buffer_id]), boff = r.u32(buffers[buffer_id] + 4);   // TM2_Buffer
            const size_t es = (dtype == TAMD_DT_FP32 || dtype == TAMD_DT_INT32) ? 4 : (dtype == TAMD_DT_FP16 ? 2 : 1);
            if (boff) {
                if (!r.in(boff, bsize) || elems * es > bsize) return fail("const tensor size in model is too small");
                d.data = r.b + boff;
            }                                                   // else: structure-only model, zero filled
        }
        if (!r.ok) return fail("corrupt tensor record");
        if (tamd_graph_add_tensor(g, &d) < 0) return fail("add_tensor failed");
    }

    for (uint32_t no : nodes) {                                // TM2_Node
        std::vector<uint32_t> vi = r.vec(r.u32(no + 4)), vo = r.vec(r.u32(no + 8));
        const uint32_t op_o = r.u32(no + 12);
        std::string name = r.str(r.u32(no + 16));
        const uint32_t optype = r.u32(op_o + 4), po = r.u32(op_o + 8);   // TM2_Operator
        if (!r.ok) return fail("corrupt node");
        const int op = map_op(optype);
        if (op < 0) { set_error("tm2: operator type %u (%s) is not supported by the device backend", optype, name.c_str()); tamd_graph_destroy(g); return nullptr; }
        NodeParam p{};
        bool have_param = po != 0;
        if (op == TAMD_OP_RESHAPE) {        // TM2_ReshapeParam carries the recipe (re_shape, is_mxnet, is_onnx: reshape.c:37-160); the
            // serializer also stores the RESOLVED shape with the output tensor, which is what the device needs
            if (vo.empty() || vo[0] >= g->tensors.size()) return fail("reshape without output tensor");
            const HTensor& ot = g->tensors[vo[0]];
            if (ot.dims.empty() || ot.dims.size() > 8) return fail("reshape output without a shape");
            p.reshape.dim_num = (int)ot.dims.size();
            for (size_t i = 0; i < ot.dims.size(); i++) p.reshape.dims[i] = ot.dims[i];
            have_param = true;
        } else if (po) {
            switch (op) {
            case TAMD_OP_CONV: {                               // TM2_ConvParam tm2_format.h:419-435 (tm2_conv.c:50-73)
                tamd_conv_param& c = p.conv;
                c.kernel_h = r.i32(po); c.kernel_w = r.i32(po + 4); c.stride_h = r.i32(po + 8); c.stride_w = r.i32(po + 12);
                c.dilation_h = r.i32(po + 16); c.dilation_w = r.i32(po + 20); c.input_channel = r.i32(po + 24);
                c.output_channel = r.i32(po + 28); c.group = r.i32(po + 32); c.activation = r.i32(po + 36);
                c.pad_h0 = r.i32(po + 40); c.pad_w0 = r.i32(po + 44); c.pad_h1 = r.i32(po + 48); c.pad_w1 = r.i32(po + 52);
                break;
            }
            case TAMD_OP_POOL: {                               // TM2_PoolParam :510-524 (tm2_pool.c)
                tamd_pool_param& q = p.pool;
                q.pool_method = (int)r.u32(po); q.kernel_h = r.i32(po + 4); q.kernel_w = r.i32(po + 8);
                q.stride_h = r.i32(po + 12); q.stride_w = r.i32(po + 16); q.global = r.i32(po + 20);
                q.caffe_flavor = r.i32(po + 24); q.pad_h0 = r.i32(po + 28); q.pad_w0 = r.i32(po + 32);
                q.pad_h1 = r.i32(po + 36); q.pad_w1 = r.i32(po + 40);
                break;
            }
            case TAMD_OP_FC: p.fc.num_output = r.i32(po); break;
            case TAMD_OP_INSTANCENORM: p.inorm.eps = r.f32(po); break;      // TM2_InstanceNormParam: eps at offset 0
            case TAMD_OP_BATCHNORM: p.bn.rescale_factor = r.f32(po); p.bn.eps = r.f32(po + 4); p.bn.caffe_flavor = r.i32(po + 8); break;      // TM2_BatchNormParam :407-412
            case TAMD_OP_RELU: p.relu.negative_slope = r.f32(po); break;
            case TAMD_OP_ELTWISE:
                p.elt.type = (int)r.u32(po); p.elt.caffe_flavor = r.i32(po + 4); p.elt.shift = r.f32(po + 8);
                p.elt.power = r.f32(po + 12); p.elt.scale = r.f32(po + 16);
                break;
            case TAMD_OP_CONCAT: p.concat.axis = r.i32(po); break;
            case TAMD_OP_SOFTMAX: p.softmax.axis = r.i32(po); break;   // TM2_SoftmaxParam {axis}
            case TAMD_OP_UPSAMPLE: p.ups.scale = r.f32(po); break;
            case TAMD_OP_CLIP: p.clip.max = r.f32(po); p.clip.min = r.f32(po + 4); break;                 // TM2_ClipParam {max, min}
            case TAMD_OP_HARDSWISH: p.hardswish.alpha = r.f32(po); p.hardswish.beta = r.f32(po + 4); break;   // TM2_HardSwishParam {alpha, beta}
            case TAMD_OP_INTERP:                               // TM2_InterpParam {resize_type, width_scale, height_scale, output_width, output_height}
                p.interp.resize_type = r.i32(po); p.interp.width_scale = r.f32(po + 4); p.interp.height_scale = r.f32(po + 8);
                p.interp.output_width = r.i32(po + 12); p.interp.output_height = r.i32(po + 16);
                break;
            case TAMD_OP_SHUFFLECHANNEL: p.shuffle.group = r.i32(po); break;                              // TM2_ShuffleChannelParam {group}
            case TAMD_OP_SPLIT: {                              // TM2_SplitParam {axis, split_dim, u8 is_caffe, u8 is_onnx, offset_split_sizes} (tm2_split.c:48-78)
                const uint32_t flags = r.u32(po + 8), vs = r.u32(po + 12);
                const bool is_caffe = (flags & 0xffu) != 0, is_onnx = ((flags >> 8) & 0xffu) != 0;
                p.split.axis = is_onnx ? r.i32(po) : 0;        // the loader takes the file's axis only when is_onnx is set; split.c:134 defaults it to 0
                if (is_caffe) p.split.num = -1;
                else if (vs) {                                 // TM2_Vector_dims {v_num, dims[]}
                    const std::vector<uint32_t> sizes = r.vec(vs);
                    if (!r.ok || sizes.size() > TAMD_SPLIT_MAX) p.split.num = TAMD_SPLIT_MAX + 1;      // refused by count (split_refusal)
                    else { p.split.num = (int)sizes.size(); for (size_t i = 0; i < sizes.size(); i++) p.split.sizes[i] = (int)sizes[i]; }
                }
                break;
            }
            case TAMD_OP_SLICE: {                              // TM2_SliceParam :607-619 {axis, offset slice_points, offset begins, offset sizes,
                tamd_slice_param& q = p.slice;                 // iscaffe, ismxnet, isonnx, begin, end, step} (tm2_slice.c:48-92)
                q.axis = r.i32(po); q.iscaffe = r.i32(po + 16); q.ismxnet = r.i32(po + 20); q.isonnx = r.i32(po + 24);
                q.begin = r.i32(po + 28); q.end = r.i32(po + 32); q.step = r.i32(po + 36);
                auto count = [&](uint32_t vo_) { return vo_ ? (int)r.u32(vo_) : 0; };      // TM2_NOT_SET: no vector; the device carries the counts only
                q.slice_point_num = count(r.u32(po + 4)); q.begin_num = count(r.u32(po + 8)); q.size_num = count(r.u32(po + 12));
                // slice.c:52-53: a negative axis counts from the back of the input's rank.  Outside the rank the reference's infer_shape
                // fails; the value stays as it is and slice_refusal names it
                const int rank = !vi.empty() && vi[0] < g->tensors.size() ? (int)g->tensors[vi[0]].dims.size() : 0;
                if (rank > 0 && q.axis >= -rank && q.axis < rank) q.axis = (q.axis + rank) % rank;
                break;
            }
            case TAMD_OP_TRANSPOSE: {                          // TM2_TransposeParam :929-932 {offset_tr_shape -> TM2_Vector_dims} (tm2_transpose.c)
                const uint32_t vs = r.u32(po);
                if (!vs) return fail("transpose without its tr_shape vector");
                const std::vector<uint32_t> order = r.vec(vs);
                if (!r.ok) break;
                p.transpose.dim_num = (int)order.size();       // any length travels: transpose_refusal names the ones that do not run
                for (size_t i = 0; i < order.size() && i < 8; i++) p.transpose.order[i] = (int)order[i];
                break;
            }
            case TAMD_OP_RESIZE:                               // TM2_ResizeParam {scale_x, scale_y, type}: the reference's loader fills scale_h from
                p.resize.scale_h = r.f32(po); p.resize.scale_w = r.f32(po + 4); p.resize.type = 0;      // scale_x, scale_w from scale_y, and never reads type (tm2_resize.c:50-51)
                break;
            case TAMD_OP_DEPTHTOSPACE: p.d2s.block_size = r.i32(po); break;      // TM2_DepthToSpaceParam :942-945 {block_size} (tm2_depthtospace.c)
            case TAMD_OP_CROP: {                               // TM2_CropParam :812-823 {num_args, offset_c, offset_h, offset_w, crop_h, crop_w,
                tamd_crop_param& q = p.crop;                   // bool center_crop + 3 bytes of padding, axis, flag} (tm2_crop.c:42-61)
                q.num_args = r.i32(po); q.offset_c = r.i32(po + 4); q.offset_h = r.i32(po + 8); q.offset_w = r.i32(po + 12);
                q.crop_h = r.i32(po + 16); q.crop_w = r.i32(po + 20);
                q.center_crop = (r.u32(po + 24) & 0xffu) != 0;  // one byte; the three behind it are whatever the writer's compiler left there
                q.axis = r.i32(po + 28); q.flag = r.i32(po + 32);
                break;
            }
            case TAMD_OP_PRIORBOX: {                           // TM2_PriorBoxParam :526-542 (tm2_priorbox.c:43-84)
                tamd_priorbox_param& q = p.priorbox;
                auto floats = [&](uint32_t vo_, float* dst, int cap, int* num) {      // TM2_Vector_floats {v_num, data[]}
                    const uint32_t n = r.u32(vo_);
                    if (!r.ok || n > (uint32_t)cap) { r.ok = false; return; }
                    for (uint32_t i = 0; i < n; i++) dst[i] = r.f32(vo_ + 4 + 4 * i);
                    if (num) *num = (int)n;
                };
                int nvar = 0;
                floats(r.u32(po), q.min_size, TAMD_PRIORBOX_MAX, &q.min_size_num);
                floats(r.u32(po + 4), q.max_size, TAMD_PRIORBOX_MAX, &q.max_size_num);
                floats(r.u32(po + 8), q.variance, 4, &nvar);
                floats(r.u32(po + 12), q.aspect_ratio, TAMD_PRIORBOX_MAX, &q.aspect_ratio_num);
                if (nvar != 4) r.ok = false;
                q.flip = r.i32(po + 16); q.clip = r.i32(po + 20); q.image_h = r.i32(po + 28); q.image_w = r.i32(po + 32);
                q.step_w = r.f32(po + 36); q.step_h = r.f32(po + 40); q.offset = r.f32(po + 44);
                break;
            }
            case TAMD_OP_PERMUTE:                              // TM2_PermuteParam {flag, order0..3} (tm2_permute.c)
                for (int i = 0; i < 4; i++) p.perm.order[i] = r.i32(po + 4 + 4 * i);
                break;
            default: break;
            }
        }
        if (op == TAMD_OP_TRANSPOSE && !po) return fail("transpose without its tr_shape vector");
        if (!r.ok) return fail("corrupt operator params");
        std::vector<int> ins(vi.begin(), vi.end()), outs(vo.begin(), vo.end());
        tamd_node_desc d{};
        d.op = op; d.input_num = (int)ins.size(); d.inputs = ins.data(); d.output_num = (int)outs.size();
        d.outputs = outs.data(); d.param = have_param ? &p : nullptr; d.name = name.c_str();
        if (tamd_graph_add_node(g, &d) < 0) { tamd_graph_destroy(g); return nullptr; }
    }
    std::vector<int> gi, go;
    for (uint32_t ni : in_nodes) { if (ni >= g->nodes.size() || g->nodes[ni].out.empty()) return fail("bad input node"); gi.push_back(g->nodes[ni].out[0]); }
    for (uint32_t ni : out_nodes) { if (ni >= g->nodes.size() || g->nodes[ni].out.empty()) return fail("bad output node"); go.push_back(g->nodes[ni].out[0]); }
    tamd_graph_set_inputs(g, (int)gi.size(), gi.data());
    tamd_graph_set_outputs(g, (int)go.size(), go.data());
    return g;
}
