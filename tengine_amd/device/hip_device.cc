// Tengine device plugin "HIP": the drop-in boundary of SURVEY §8(b).
//
// Exports register_hip_device() / unregister_hip_device() -- the names cmake/registry.cmake:11-31
// derives from a file called hip_device.cc, so the same file works in-tree (one line in
// source/device/CMakeLists.txt) or as a plugin loaded with
//   load_tengine_plugin("hip", "libtengine_hip_device.so", "register_hip_device")   (source/api/plugin.c:88-159)
// against a Tengine built with all symbols visible.  Compiled against the reference's own headers
// (struct device / subgraph / tensor are plain C structs the backends read directly), it
// translates one `struct subgraph` into a tamd_graph (include/tengine_amd.h) at pre_run and moves
// bytes at run.  No kernel code lives here.
//
//   interface.init/pre_run/run/post_run/release_graph/release_device   device.h:40-65
//   allocator.describe                                                 device.h:71-84, cuda_device.cc:47-83 (pattern)
//   optimizer.split_graph                                              c_api.c:468-498 caller, split.c:140,314,536 helpers
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <stddef.h>
#include <string.h>

#include <dlfcn.h>

#include <atomic>
#include <map>
#include <mutex>
#include <string>
#include <vector>

extern "C" {
#include "api/c_api.h"
#include "device/device.h"
#include "executer/executer.h"
#include "graph/graph.h"
#include "graph/node.h"
#include "graph/subgraph.h"
#include "graph/tensor.h"
#include "module/module.h"
#include "operator/op.h"
#include "optimizer/split.h"
#include "scheduler/scheduler.h"
#include "utility/log.h"
#include "utility/sys_port.h"
#include "utility/vector.h"
// operator parameter structs (source/operator/prototype/)
#include "batchnorm_param.h"
#include "clip_param.h"
#include "concat_param.h"
#include "convolution_param.h"
#include "crop_param.h"
#include "depthtospace_param.h"
#include "eltwise_param.h"
#include "fc_param.h"
#include "flatten_param.h"
#include "hardswish_param.h"
#include "interp_param.h"
#include "permute_param.h"
#include "pooling_param.h"
#include "priorbox_param.h"
#include "instancenorm_param.h"
#include "resize_param.h"
#include "shuffle_channel_param.h"
#include "slice_param.h"
#include "relu_param.h"
#include "softmax_param.h"
#include "split_param.h"
#include "transpose_param.h"
#include "upsample_param.h"
}

#include "tengine_amd.h"

#define HIP_DEV_NAME "HIP"

namespace {

struct HipSubgraph {
    tamd_graph* g = nullptr;
    // (round 6: a batched subgraph of batch-wise independent operators is TWO device graphs of half the batch each behind this one handle,
    //  side by side on their own HSA queues -- tamd_options.split_batch, decided in hip_dev_prerun, done by the library: csrc/graph_pair.hip)
    std::vector<uint16_t> in_ir, out_ir;   // ir tensor indices of the subgraph inputs / outputs, in tamd order
};

// The operators the plugin hands to the device: OP_* (source/operator/op.h:38-145) -> TAMD_OP_*.  quantised_only: SSD head plumbing
// (Permute -> Flatten -> Concat, Reshape, PriorBox), on the device for the QUANTISED graphs (uint8 since round 3, int8 since round 6:
// csrc/graph_plan.hip "dense tensors") -- an fp32 graph keeps these on the CPU without dragging the convolutions around them back there
struct OpRow { int op; int tamd_op; bool quantised_only; };
const OpRow kOps[] = {
    {OP_INPUT, TAMD_OP_INPUT, false},       {OP_CONST, TAMD_OP_CONST, false},     {OP_CONV, TAMD_OP_CONV, false},
    {OP_FC, TAMD_OP_FC, false},             {OP_POOL, TAMD_OP_POOL, false},       {OP_RELU, TAMD_OP_RELU, false},
    {OP_ELTWISE, TAMD_OP_ELTWISE, false},   {OP_CONCAT, TAMD_OP_CONCAT, false},   {OP_DROPOUT, TAMD_OP_DROPOUT, false},
    {OP_UPSAMPLE, TAMD_OP_UPSAMPLE, false}, {OP_SOFTMAX, TAMD_OP_SOFTMAX, false}, {OP_RELU6, TAMD_OP_RELU6, false},
    {OP_PERMUTE, TAMD_OP_PERMUTE, true},    {OP_FLATTEN, TAMD_OP_FLATTEN, true},  {OP_RESHAPE, TAMD_OP_RESHAPE, true},
    {OP_PRIORBOX, TAMD_OP_PRIORBOX, true},
    // byte maps by table (csrc/lut_tables.cc): the quantised kernels of the reference alone; which of int8 / uint8: tamd_op_supported
    {OP_SIGMOID, TAMD_OP_SIGMOID, true},    {OP_CLIP, TAMD_OP_CLIP, true},        {OP_HARDSWISH, TAMD_OP_HARDSWISH, true},
    {OP_MISH, TAMD_OP_MISH, true},
    // every ONNX Resize; the device runs the nearest mode of the two quantised kernels (which nodes: tamd_node_supported)
    {OP_INTERP, TAMD_OP_INTERP, true},
    // the channel movers of a ShuffleNet unit: byte copies in the quantised kernels of the reference (csrc/chanmap.hip).  An fp32 graph
    // keeps both on the CPU device (which Split forms: tamd_node_supported; the caffe Slice of the benchmark file is another operator)
    {OP_SPLIT, TAMD_OP_SPLIT, true},        {OP_SHUFFLECHANNEL, TAMD_OP_SHUFFLECHANNEL, true},
    // the activation of the face models (csrc/prelu.hip): the two quantised kernels of the reference; its fp16 slope constant travels
    // like any constant.  An fp32 graph keeps the node on the CPU device (which ranks and slopes: tamd_node_supported)
    {OP_PRELU, TAMD_OP_PRELU, true},
    // the not-folded BatchNorm of an MXNet export (csrc/chan_lut.hip): the uint8 kernel of the reference, a byte map per channel; int8 (no
    // kernel in the reference) and fp32 graphs keep the node on the CPU device (which ranks and statistics: tamd_node_supported)
    {OP_BATCHNORM, TAMD_OP_BATCHNORM, true},
    // YOLOv4-tiny's routes and Focus's strided picks (csrc/slice.hip): the onnx form in uint8 graphs.  The reference has no int8 kernel, and
    // an fp32 graph keeps the node on the CPU device -- the caffe Slice of the ShuffleNet benchmark file too (which: tamd_node_supported)
    {OP_SLICE, TAMD_OP_SLICE, true},
    // every ONNX Transpose (csrc/transpose.hip): the Detect head of the YOLOv5 family, torch's channel shuffle, the ONNX form of the SSD
    // head permute -- the two quantised kernels of the reference, rank 2 .. 6.  An fp32 graph keeps the node on the CPU device (which
    // orders: tamd_node_supported)
    {OP_TRANSPOSE, TAMD_OP_TRANSPOSE, true},
    // the cut of RetinaFace's top-down pyramid (csrc/topdown.hip, csrc/slice.hip): a box of raw bytes in uint8 graphs.  The reference has no
    // int8 kernel, and an fp32 graph keeps the node on the CPU device (which forms and boxes: tamd_node_supported)
    {OP_CROP, TAMD_OP_CROP, true},
    // sub-pixel convolution's shuffle (csrc/d2s.hip): ESPCN / EDSR tails, torch's PixelShuffle -- the two quantised kernels of the
    // reference, raw bytes.  An fp32 graph keeps the node on the CPU device (which shapes: tamd_node_supported)
    {OP_DEPTHTOSPACE, TAMD_OP_DEPTHTOSPACE, true},
    // the nearest up-sampling of an ONNX Upsample and caffe's Resize layer (csrc/interp.hip, csrc/resize.hip): the nearest mode of the two
    // quantised kernels of the reference, batch 1.  An fp32 graph keeps the node on the CPU device (which nodes: tamd_node_supported)
    {OP_RESIZE, TAMD_OP_RESIZE, true},
    // the per-image normalisation of image-to-image generators (csrc/instnorm.hip): the uint8 kernel of the reference, a byte map per
    // plane computed on the device; int8 (no kernel in the reference) and fp32 graphs keep the node on the CPU device (which shapes and
    // values: tamd_node_supported)
    {OP_INSTANCENORM, TAMD_OP_INSTANCENORM, true},
};

const OpRow* find_op(int op)
{
    for (const OpRow& r : kOps)
        if (r.op == op) return &r;
    return nullptr;
}

int map_op(int op)
{
    const OpRow* r = find_op(op);
    return r ? r->tamd_op : -1;
}

// may a graph of activation type `dtype` (-1: unknown) hand this operator to the device at all?
bool op_supported(int op, int dtype)
{
    const OpRow* r = find_op(op);
    return r && (!r->quantised_only || dtype == TENGINE_DT_UINT8 || dtype == TENGINE_DT_INT8);
}


// struct priorbox_param (priorbox_param.h:28-52, float vectors on the heap) -> the inline-array form of the C ABI
bool translate_priorbox(const struct priorbox_param* p, tamd_priorbox_param* q)
{
    memset(q, 0, sizeof(*q));
    if (p->min_size_num < 1 || p->min_size_num > TAMD_PRIORBOX_MAX || p->max_size_num < 0 || p->max_size_num > TAMD_PRIORBOX_MAX
        || p->aspect_ratio_size < 0 || p->aspect_ratio_size > TAMD_PRIORBOX_MAX || !p->variance) return false;
    q->min_size_num = p->min_size_num; q->max_size_num = p->max_size_num; q->aspect_ratio_num = p->aspect_ratio_size;
    for (int i = 0; i < p->min_size_num; i++) q->min_size[i] = p->min_size[i];
    for (int i = 0; i < p->max_size_num; i++) q->max_size[i] = p->max_size[i];
    for (int i = 0; i < p->aspect_ratio_size; i++) q->aspect_ratio[i] = p->aspect_ratio[i];
    for (int i = 0; i < 4; i++) q->variance[i] = p->variance[i];
    q->flip = p->flip; q->clip = p->clip; q->image_h = p->image_h; q->image_w = p->image_w;
    q->step_h = p->step_h; q->step_w = p->step_w; q->offset = p->offset;
    return true;
}

// descriptor of an IR tensor.  with_payload: the constant's bytes and the quantisation values travel too (pre_run); without, shapes
// and the quantisation form alone (tamd_node_supported looks at nothing else, but for a PReLU's slope and the scales of a Slice or a Transpose).  The pointers stay the IR tensor's own.
tamd_tensor_desc describe_tensor(struct tensor* t, bool with_payload)
{
    tamd_tensor_desc d;
    memset(&d, 0, sizeof(d));
    d.dtype = t->data_type; d.ttype = t->tensor_type; d.dim_num = t->dim_num;
    for (int i = 0; i < t->dim_num && i < 8; i++) d.dims[i] = t->dims[i];
    d.quant_num = t->quant_param_num;
    d.name = t->name;
    if (!with_payload) return d;
    d.data = (t->tensor_type == TENSOR_TYPE_CONST) ? t->data : nullptr;
    if (t->quant_param_num == 1) { d.scales = &t->scale; d.zero_points = &t->zero_point; }      // (tensor.h:84-98: value and list share a union)
    else if (t->quant_param_num > 1) { d.scales = t->scale_list; d.zero_points = t->zp_list; }
    return d;
}

// IR node -> the parameter struct the C ABI takes for its operator: written into `s`, *param points at it (nullptr: the operator has
// none).  The one translation: pre_run and the support query of the splitter both come here.  false: a PriorBox the ABI cannot carry.
union NodeParams {
    tamd_conv_param conv; tamd_pool_param pool; tamd_fc_param fc; tamd_relu_param relu; tamd_eltwise_param elt; tamd_concat_param concat;
    tamd_upsample_param ups; tamd_permute_param perm; tamd_softmax_param softmax; tamd_reshape_param reshape; tamd_priorbox_param priorbox;
    tamd_clip_param clip; tamd_hardswish_param hardswish; tamd_interp_param interp; tamd_split_param split;
    tamd_shufflechannel_param shuffle; tamd_slice_param slice; tamd_crop_param crop; tamd_depthtospace_param d2s; tamd_resize_param resize; tamd_transpose_param transpose; tamd_batchnorm_param bn;
    tamd_instancenorm_param inorm;
};

bool translate_node(struct graph* ir, struct node* n, NodeParams* s, const void** param)
{
    *param = s;
    switch (map_op(n->op.type)) {
    case TAMD_OP_PRIORBOX: return translate_priorbox((const struct priorbox_param*)n->op.param_mem, &s->priorbox);
    case TAMD_OP_SOFTMAX: s->softmax.axis = ((const struct softmax_param*)n->op.param_mem)->axis; break;
    case TAMD_OP_RESHAPE: {          // the resolved shape (reshape.c infer_shape already ran)
        struct tensor* ot = get_ir_graph_tensor(ir, n->output_tensors[0]);
        s->reshape.dim_num = ot->dim_num;
        for (int k = 0; k < ot->dim_num && k < 8; k++) s->reshape.dims[k] = ot->dims[k];
        break;
    }
    case TAMD_OP_CONV: {
        const struct conv_param* p = (const struct conv_param*)n->op.param_mem;
        s->conv = {p->kernel_h, p->kernel_w, p->stride_h, p->stride_w, p->pad_h0, p->pad_h1, p->pad_w0, p->pad_w1,
                   p->dilation_h, p->dilation_w, p->input_channel, p->output_channel, p->group, p->activation};
        break;
    }
    case TAMD_OP_POOL: {
        const struct pool_param* p = (const struct pool_param*)n->op.param_mem;
        // hand over the ORIGINAL (model) pads: the backend re-resolves them like infer_shape does
        s->pool = {p->pool_method, p->kernel_h, p->kernel_w, p->stride_h, p->stride_w, p->pad_h0_org, p->pad_h1_org,
                   p->pad_w0_org, p->pad_w1_org, p->global, p->caffe_flavor};
        if (p->global) {   // infer_shape already rewrote kernel/stride for global pooling (pooling.c:52-66)
            s->pool.pad_h0 = s->pool.pad_h1 = s->pool.pad_w0 = s->pool.pad_w1 = 0;
        }
        break;
    }
    case TAMD_OP_FC: s->fc.num_output = ((const struct fc_param*)n->op.param_mem)->num_output; break;
    case TAMD_OP_RELU: s->relu.negative_slope = ((const struct relu_param*)n->op.param_mem)->negative_slope; break;
    case TAMD_OP_ELTWISE: {
        const struct eltwise_param* p = (const struct eltwise_param*)n->op.param_mem;
        s->elt = {p->type, p->caffe_flavor, p->shift, p->power, p->scale};
        break;
    }
    case TAMD_OP_CONCAT: s->concat.axis = ((const struct concat_param*)n->op.param_mem)->axis; break;
    case TAMD_OP_UPSAMPLE: s->ups.scale = ((const struct upsample_param*)n->op.param_mem)->scale; break;
    case TAMD_OP_CLIP: {
        const struct clip_param* p = (const struct clip_param*)n->op.param_mem;
        s->clip = {p->max, p->min};
        break;
    }
    case TAMD_OP_HARDSWISH: {
        const struct hardswish_param* p = (const struct hardswish_param*)n->op.param_mem;
        s->hardswish = {p->alpha, p->beta};
        break;
    }
    case TAMD_OP_INTERP: {           // all five fields (interp.c infer_shape already ran: both scales are set, the sizes are its result)
        const struct interp_param* p = (const struct interp_param*)n->op.param_mem;
        s->interp = {p->resize_type, p->width_scale, p->height_scale, p->output_width, p->output_height};
        break;
    }
    case TAMD_OP_SHUFFLECHANNEL: s->shuffle.group = ((const struct shuffle_channel_param*)n->op.param_mem)->group; break;
    case TAMD_OP_SLICE: {            // as infer_shape has left it (slice.c:52-53, 124-128: axis normalised, end clipped); the vectors as counts
        const struct slice_param* p = (const struct slice_param*)n->op.param_mem;
        s->slice = tamd_slice_param{};
        s->slice.axis = p->axis; s->slice.begin = p->begin; s->slice.end = p->end; s->slice.step = p->step;
        s->slice.iscaffe = p->iscaffe; s->slice.ismxnet = p->ismxnet; s->slice.isonnx = p->isonnx;
        s->slice.slice_point_num = p->slice_point_ ? get_vector_num(p->slice_point_) : 0;
        s->slice.begin_num = p->begin_ ? get_vector_num(p->begin_) : 0;
        s->slice.size_num = p->size_ ? get_vector_num(p->size_) : 0;
        break;
    }
    case TAMD_OP_BATCHNORM: {        // batchnorm_param.h, field for field
        const struct batchnorm_param* p = (const struct batchnorm_param*)n->op.param_mem;
        s->bn = {p->rescale_factor, p->eps, p->caffe_flavor};
        break;
    }
    case TAMD_OP_INSTANCENORM: {     // instancenorm_param.h, field for field
        const struct instancenorm_Param* p = (const struct instancenorm_Param*)n->op.param_mem;
        s->inorm = tamd_instancenorm_param{p->eps};
        break;
    }
    case TAMD_OP_RESIZE: {           // resize_param.h, field for field: the in-memory parameter, `type` included (a file never carries it)
        const struct resize_param* p = (const struct resize_param*)n->op.param_mem;
        s->resize = tamd_resize_param{p->scale_w, p->scale_h, p->type};
        break;
    }
    case TAMD_OP_DEPTHTOSPACE:       // depthtospace_param.h: the one field
        s->d2s = tamd_depthtospace_param{((const struct depthtospace_param*)n->op.param_mem)->block_size};
        break;
    case TAMD_OP_CROP: {             // crop_param.h, field for field
        const struct crop_param* p = (const struct crop_param*)n->op.param_mem;
        s->crop = tamd_crop_param{p->num_args, p->offset_c, p->offset_h, p->offset_w, p->crop_h, p->crop_w, p->center_crop, p->axis, p->flag};
        break;
    }
    case TAMD_OP_TRANSPOSE: {        // the tr_shape vector inline; its length as it is (the first 8 entries: transpose_refusal names the lengths that do not run)
        const struct transpose_param* p = (const struct transpose_param*)n->op.param_mem;
        s->transpose = tamd_transpose_param{};
        s->transpose.dim_num = p->tr_shape ? p->tr_shape_size : 0;
        for (int i = 0; i < s->transpose.dim_num && i < 8; i++) s->transpose.order[i] = p->tr_shape[i];
        break;
    }
    case TAMD_OP_SPLIT: {            // the split_sizes vector inline; num -1: is_caffe, 0: no sizes, above TAMD_SPLIT_MAX: too many (all refused by name)
        const struct split_param* p = (const struct split_param*)n->op.param_mem;
        s->split = tamd_split_param{};
        s->split.axis = p->axis;
        const int num = p->split_sizes_ ? get_vector_num(p->split_sizes_) : 0;
        if (p->is_caffe) s->split.num = -1;
        else if (num > TAMD_SPLIT_MAX) s->split.num = TAMD_SPLIT_MAX + 1;
        else {
            s->split.num = num;
            for (int k = 0; k < num; k++) s->split.sizes[k] = *(const int*)get_vector_data(p->split_sizes_, k);
        }
        break;
    }
    case TAMD_OP_PERMUTE: {
        const struct permute_param* p = (const struct permute_param*)n->op.param_mem;
        s->perm = {{p->order0, p->order1, p->order2, p->order3}};
        break;
    }
    default: *param = nullptr; break;
    }
    return true;
}

int hip_dev_init(struct device* dev)
{
    (void)dev;
    // registration must succeed on hosts without a GPU too (the CPU device keeps working); the
    // device is probed when a subgraph is actually assigned to it (pre_run fails loudly then).
    return 0;
}

int g_split_subgraphs = 0;       // subgraphs preran as two half-batch graphs since the plugin was loaded (hip_device_split_subgraphs: tests)

// Does this subgraph ask the library for two half-batch device graphs?  What only the plugin knows: its switch (TAMD_SPLIT_BATCH=0:
// never; =2: from batch 2 on (tests); default: from batch 8 on) and the batch, dimension 0 of the subgraph's non-constant inputs -- all
// of them, or there is no batch to speak of.  Whether the operators treat the images of a batch independently and every activation
// tensor carries the batch in front is the library's test (csrc/graph_pair.hip: pair_try_prerun keeps one launch list where it fails).
bool split_wanted(struct graph* ir, struct subgraph* subgraph)
{
    const char* e = getenv("TAMD_SPLIT_BATCH");
    const int mode = e ? atoi(e) : 1;
    if (mode == 0) return false;
    int B = 0;
    for (int i = 0; i < subgraph->input_num; i++) {
        struct tensor* t = get_ir_graph_tensor(ir, subgraph->input_tensor_list[i]);
        if (t->tensor_type == TENSOR_TYPE_CONST) continue;
        if (t->dim_num < 1 || (B != 0 && t->dims[0] != B)) return false;
        B = t->dims[0];
    }
    return B >= (mode == 2 ? 2 : 8) && B % 2 == 0;          // (profiles/r06_plugin_split_threshold.txt: batch 8 +1 .. +22 %, batch 4 0 .. +3 %, batch 2 -3 .. +2 %)
}

// the device graph of a subgraph; hs->in_ir / out_ir: its inputs / outputs as IR tensor indices, in tamd order
tamd_graph* build_device_graph(struct graph* ir, struct subgraph* subgraph, HipSubgraph* hs)
{
    tamd_graph* tg = tamd_graph_create();
    std::map<int, int> tmap;   // ir tensor index -> tamd tensor index

    auto is_sub_input = [&](uint16_t t) {
        for (int i = 0; i < subgraph->input_num; i++)
            if (subgraph->input_tensor_list[i] == t) return true;
        return false;
    };
    auto add_tensor = [&](uint16_t idx) -> int {
        auto it = tmap.find(idx);
        if (it != tmap.end()) return it->second;
        struct tensor* t = get_ir_graph_tensor(ir, idx);
        tamd_tensor_desc d = describe_tensor(t, true);
        if (t->tensor_type == TENSOR_TYPE_VAR && is_sub_input(idx)) d.ttype = TAMD_TT_INPUT;   // produced by another subgraph
        return tmap[idx] = tamd_graph_add_tensor(tg, &d);
    };

    for (int i = 0; i < subgraph->node_num; i++) {
        struct node* n = get_ir_graph_node(ir, subgraph->node_list[i]);
        NodeParams params;
        tamd_node_desc nd;
        memset(&nd, 0, sizeof(nd));
        nd.op = map_op(n->op.type);
        if (nd.op < 0 || !translate_node(ir, n, &params, &nd.param)) {
            TLOG_ERR("Tengine HIP: op %d (%s) is not supported on the device\n", n->op.type, n->name ? n->name : "?");
            tamd_graph_destroy(tg);
            return nullptr;
        }
        std::vector<int> ins, outs;
        for (int k = 0; k < n->input_num; k++) ins.push_back(add_tensor(n->input_tensors[k]));
        for (int k = 0; k < n->output_num; k++) outs.push_back(add_tensor(n->output_tensors[k]));
        nd.input_num = (int)ins.size(); nd.inputs = ins.data(); nd.output_num = (int)outs.size(); nd.outputs = outs.data(); nd.name = n->name;
        if (tamd_graph_add_node(tg, &nd) < 0) {
            TLOG_ERR("Tengine HIP: %s\n", tamd_last_error());
            tamd_graph_destroy(tg);
            return nullptr;
        }
    }
    std::vector<int> gi, go;
    for (int i = 0; i < subgraph->input_num; i++) {
        uint16_t t = subgraph->input_tensor_list[i];
        struct tensor* it = get_ir_graph_tensor(ir, t);
        if (it->tensor_type == TENSOR_TYPE_CONST) continue;
        if (!tmap.count(t)) continue;
        gi.push_back(tmap[t]);
        hs->in_ir.push_back(t);
    }
    for (int i = 0; i < subgraph->output_num; i++) {
        uint16_t t = subgraph->output_tensor_list[i];
        if (!tmap.count(t)) continue;
        go.push_back(tmap[t]);
        hs->out_ir.push_back(t);
    }
    tamd_graph_set_inputs(tg, (int)gi.size(), gi.data());
    tamd_graph_set_outputs(tg, (int)go.size(), go.data());
    return tg;
}

int hip_dev_prerun(struct device* dev, struct subgraph* subgraph, void* options)
{
    (void)dev;
    struct graph* ir = subgraph->graph;
    HipSubgraph* hs = new HipSubgraph();
    hs->g = build_device_graph(ir, subgraph, hs);
    if (!hs->g) { delete hs; return -1; }

    tamd_options opt;
    opt.dev_name = HIP_DEV_NAME; opt.size = (int)sizeof(opt); opt.gpu_index = 0; opt.use_hip_graph = 1; opt.profile = 0;
    opt.u8_integer = 0;           // byte-exact uint8 unless the application asks for the integer form
    opt.keep_tensors = 0;         // tensors of disjoint lifetimes share device memory (only subgraph outputs are visible to Tengine)
    opt.direct_dispatch = 1;      // the blocking host-to-host run as one AQL pass on the subgraph's own HSA queue (csrc/direct.cc:
                                  // MobileNet-v1 batch 1 81.6 -> 68.7 us per run); TAMD_DIRECT_DISPATCH=0 keeps the hipGraph
    if (options) {   // options may be NULL (scheduler.c:49-59); else the blob of set_context_device, whose byte count the core
                     // does not pass on (c_api.c:183-210): it carries its own `size`, and only the fields inside it are read
        const tamd_options* o = (const tamd_options*)options;
        if (o->dev_name && 0 == strcmp(o->dev_name, HIP_DEV_NAME)) {
            const int have = o->size;
            if (TAMD_OPTIONS_HAS(have, gpu_index)) opt.gpu_index = o->gpu_index;
            if (TAMD_OPTIONS_HAS(have, use_hip_graph)) opt.use_hip_graph = o->use_hip_graph;
            if (TAMD_OPTIONS_HAS(have, profile)) opt.profile = o->profile;
            if (TAMD_OPTIONS_HAS(have, direct_dispatch)) opt.direct_dispatch = o->direct_dispatch;
            if (TAMD_OPTIONS_HAS(have, keep_tensors)) opt.keep_tensors = o->keep_tensors;
            if (TAMD_OPTIONS_HAS(have, u8_integer)) opt.u8_integer = o->u8_integer;
        }
    }
    const char* env = getenv("TG_HIP_DEVICE");
    if (env) opt.gpu_index = atoi(env);
    // two half-batch device graphs instead of one: decided HERE per subgraph (split_wanted: from batch 8 on host to host), done by the library
    // behind the one tamd_graph (csrc/graph_pair.hip: it also keeps the reference's batch-dependent formulas on the WHOLE batch -- the
    // plugin's own pair of graphs, earlier this round, could not: halves of one image each took the batch-1 depthwise formula)
    opt.split_batch = (opt.direct_dispatch && split_wanted(ir, subgraph)) ? 2 : 1;
    if (tamd_graph_prerun(hs->g, &opt) != 0) {
        TLOG_ERR("Tengine HIP: prerun failed: %s\n", tamd_last_error());
        tamd_graph_destroy(hs->g);
        delete hs;
        return -1;
    }
    if (tamd_graph_halves(hs->g)) g_split_subgraphs++;
    // subgraph outputs must leave valid host bytes in ir_tensor->data (SURVEY §8b "Ownership")
    for (uint16_t t : hs->out_ir) {
        struct tensor* ot = get_ir_graph_tensor(ir, t);
        if (ot->data == nullptr) {
            ot->data = sys_malloc((size_t)ot->elem_num * ot->elem_size);
            ot->free_host_mem = 1;
        }
    }
    subgraph->device_graph = hs;
    return 0;
}

// host buffers of the subgraph's inputs / outputs -> the device graph (a graph compiled as two halves uses each buffer as two contiguous halves itself)
static int bind_io(HipSubgraph* hs, struct graph* ir)
{
    for (size_t i = 0; i < hs->in_ir.size(); i++) {
        struct tensor* t = get_ir_graph_tensor(ir, hs->in_ir[i]);
        if (!t->data) { TLOG_ERR("Tengine HIP: input tensor %s has no buffer\n", t->name); return -1; }
        if (tamd_graph_set_input(hs->g, (int)i, t->data, (size_t)t->elem_num * t->elem_size) != 0) return -1;
    }
    for (size_t i = 0; i < hs->out_ir.size(); i++) {
        struct tensor* t = get_ir_graph_tensor(ir, hs->out_ir[i]);
        if (tamd_graph_set_output(hs->g, (int)i, t->data, (size_t)t->elem_num * t->elem_size) != 0) return -1;
    }
    return 0;
}

int hip_dev_run(struct device* dev, struct subgraph* subgraph)
{
    (void)dev;
    HipSubgraph* hs = (HipSubgraph*)subgraph->device_graph;
    if (!hs) return -1;
    struct graph* ir = subgraph->graph;
    if (bind_io(hs, ir) != 0) {                         // pointers are re-read at every run (tm_benchmark.cc:95-102)
        TLOG_ERR("Tengine HIP: %s\n", tamd_last_error());
        return -1;
    }
    if (tamd_graph_run(hs->g) != 0) {
        TLOG_ERR("Tengine HIP: run failed: %s\n", tamd_last_error());
        return -1;
    }
    return 0;
}

// interface.async_run / async_wait (device.h:60-63).  The reference's scheduler never calls them (scheduler.c:75-79 rejects
// run_graph(graph, 0)); a pipelining scheduler can keep two runs of a subgraph in flight with this pair.
int hip_dev_async_run(struct device* dev, struct subgraph* subgraph)
{
    (void)dev;
    HipSubgraph* hs = (HipSubgraph*)subgraph->device_graph;
    if (!hs || bind_io(hs, subgraph->graph) != 0 || tamd_graph_run_async(hs->g) != 0) {
        TLOG_ERR("Tengine HIP: async_run failed: %s\n", tamd_last_error());
        return -1;
    }
    return 0;
}

int hip_dev_async_wait(struct device* dev, struct subgraph* subgraph, int try_wait)
{
    (void)dev;
    HipSubgraph* hs = (HipSubgraph*)subgraph->device_graph;
    if (!hs) return -1;
    if (try_wait && tamd_graph_inflight(hs->g) == 0) return 0;
    if (tamd_graph_wait(hs->g) != 0) {
        TLOG_ERR("Tengine HIP: async_wait failed: %s\n", tamd_last_error());
        return -1;
    }
    return 0;
}

int hip_release_graph(struct device* dev, void* device_graph)
{
    (void)dev;
    HipSubgraph* hs = (HipSubgraph*)device_graph;
    if (hs) {
        tamd_graph_destroy(hs->g);
        delete hs;
    }
    return 0;
}

int hip_dev_postrun(struct device* dev, struct subgraph* subgraph)
{
    hip_release_graph(dev, subgraph->device_graph);
    subgraph->device_graph = nullptr;
    return 0;
}

int hip_dev_release(struct device* dev)
{
    (void)dev;
    return tamd_shutdown();
}

// allowed / blocked operator lists for a graph of activation type `dtype` (-1: unknown), and the precisions of the device
void fill_op_lists(struct vector* allowed_ops, struct vector* blocked_ops, struct vector* precision, int dtype)
{
    for (int i = 0; i < OP_BUILTIN_LAST; i++) {
        if (op_supported(i, dtype)) push_vector_data(allowed_ops, &i);
        else push_vector_data(blocked_ops, &i);
    }
    for (int p : {TENGINE_DT_INT8, TENGINE_DT_UINT8, TENGINE_DT_FP32}) push_vector_data(precision, &p);
}

int hip_describe(struct device* device, struct vector* allowed_ops, struct vector* blocked_ops, struct vector* precision)
{
    (void)device;
    fill_op_lists(allowed_ops, blocked_ops, precision, -1);
    return 0;
}

int hip_evaluation(struct device* device, struct subgraph* sub_graph, struct vector* tensors, struct vector* nodes)
{
    (void)device; (void)sub_graph; (void)tensors; (void)nodes;
    return 0;
}

int hip_allocate(struct device* device, struct subgraph* sub_graph)
{
    if (nullptr == device) return -1;
    sub_graph->input_wait_count = 0;
    for (int i = 0; i < sub_graph->input_num; i++) {
        struct tensor* tensor = get_ir_graph_tensor(sub_graph->graph, sub_graph->input_tensor_list[i]);
        if (tensor->tensor_type == TENSOR_TYPE_VAR) sub_graph->input_wait_count++;
    }
    return 0;
}

int hip_release(struct device* device, struct subgraph* sub_graph)
{
    (void)sub_graph;
    return device ? 0 : -1;
}

// the node as the C ABI describes it (the same translation pre_run does), asked of the backend itself
static bool node_supported(struct graph* ir, struct node* n)
{
    const int op = map_op(n->op.type);
    if (op < 0) return false;
    if (op == TAMD_OP_INPUT || op == TAMD_OP_CONST) return true;
    std::vector<tamd_tensor_desc> in, out;
    // (descriptors alone, but for a PReLU's slope: its values decide -- one that widens to inf or NaN keeps the node on the CPU device --
    // and for the quantisation values on both sides of a Slice or a Transpose: a pair whose byte map the reference cannot compute does the same;
    // an Eltwise with a constant scalar or of a unary type is such a byte map too, of those values and the constant's)
    const bool values = op == TAMD_OP_SLICE || op == TAMD_OP_TRANSPOSE || op == TAMD_OP_ELTWISE || op == TAMD_OP_BATCHNORM || op == TAMD_OP_INSTANCENORM;      // (BatchNorm: the four statistics too; InstanceNorm: gamma and beta)
    for (int k = 0; k < n->input_num; k++) in.push_back(describe_tensor(get_ir_graph_tensor(ir, n->input_tensors[k]), values || (op == TAMD_OP_PRELU && k == 1)));
    for (int k = 0; k < n->output_num; k++) out.push_back(describe_tensor(get_ir_graph_tensor(ir, n->output_tensors[k]), values));
    NodeParams params;
    std::vector<int> ii(in.size()), oi(out.size());
    tamd_node_desc nd;
    memset(&nd, 0, sizeof(nd));
    if (!translate_node(ir, n, &params, &nd.param)) return false;
    nd.op = op; nd.input_num = (int)in.size(); nd.inputs = ii.data(); nd.output_num = (int)out.size(); nd.outputs = oi.data();
    nd.name = n->name;
    return tamd_node_supported(&nd, in.data(), (int)in.size(), out.data(), (int)out.size()) == 1;
}

// Can THIS node run on the device?  Op / dtype pair, quantisation form, and the node's own parameters and shapes -- the
// last asked of the backend itself (tamd_node_supported: the planners' conditions), so that the splitter and pre_run cannot
// disagree.  (Round 2 also kept two leftover guards here -- Concat axis != 1, Permute order -- from before the backend learnt
// them; the Concat one silently sent the whole of MobileNet-SSD-with-priors to the CPU device.  They are gone.)
// int8 graphs (round 6): what a Permute / Transpose / PriorBox produces -- and every Flatten / Reshape / Dropout / Concat / Softmax /
// Sigmoid / Clip result that is only a re-reading or a byte map of it -- lives in the reference's DENSE element order on the device (csrc/graph_plan.hip "dense tensors"), not in the NHWC
// layout the convolution stack reads.  Only those re-reading operators may consume such a tensor there; anything else (an FC behind
// Permute -> Flatten, say) is left to the CPU device here, so that the splitter and the planner cannot disagree (the planner would
// refuse the graph by name at pre_run otherwise).
bool int8_tensor_is_dense_on_device(struct graph* ir, struct tensor* t, int depth = 0)
{
    if (!t || t->producer < 0 || depth > 16) return false;
    struct node* pn = get_ir_graph_node(ir, t->producer);
    switch (pn->op.type) {
    case OP_PERMUTE: case OP_PRIORBOX: case OP_RESHAPE: case OP_TRANSPOSE: return true;
    case OP_FLATTEN: case OP_DROPOUT: case OP_SOFTMAX: case OP_SIGMOID: case OP_CLIP:      // (a byte map keeps the element order it finds)
        return pn->input_num >= 1 && int8_tensor_is_dense_on_device(ir, get_ir_graph_tensor(ir, pn->input_tensors[0]), depth + 1);
    case OP_CONCAT:
        for (int i = 0; i < pn->input_num; i++)
            if (int8_tensor_is_dense_on_device(ir, get_ir_graph_tensor(ir, pn->input_tensors[i]), depth + 1)) return true;
        return false;
    default: return false;
    }
}

bool node_runs_on_device(struct graph* ir, struct node* n)
{
    const int out_dt = n->output_num ? get_ir_graph_tensor(ir, n->output_tensors[0])->data_type : -1;
    if (!op_supported(n->op.type, out_dt)) return false;
    for (int k = 0; k < n->output_num; k++) {
        struct tensor* t = get_ir_graph_tensor(ir, n->output_tensors[k]);
        if (t->tensor_type == TENSOR_TYPE_CONST) continue;
        if (t->data_type != TENGINE_DT_INT8 && t->data_type != TENGINE_DT_UINT8 && t->data_type != TENGINE_DT_FP32) return false;
        if (!tamd_op_supported(map_op(n->op.type), t->data_type)) return false;
        if (t->data_type != TENGINE_DT_FP32 && t->quant_param_num != 1) return false;
    }
    if (n->op.type == OP_FLATTEN && ((const struct flatten_param*)n->op.param_mem)->axis != 1) return false;
    if (n->op.type == OP_SOFTMAX && out_dt == TENGINE_DT_INT8 && n->input_num >= 1) {
        // int8 tensors are NHWC on the device: a 2-D input that is the flattened view of an H x W > 1 map would be normalised per
        // pixel over C, the reference normalises over all C*H*W values (softmax_kernel_ref_int8.c) -- such a node stays on the CPU
        struct tensor* t = get_ir_graph_tensor(ir, n->input_tensors[0]);
        if (t->dim_num == 2) {
            while (t->producer >= 0) {
                struct node* pn = get_ir_graph_node(ir, t->producer);
                if ((pn->op.type != OP_FLATTEN && pn->op.type != OP_RESHAPE && pn->op.type != OP_DROPOUT) || pn->input_num < 1) break;
                t = get_ir_graph_tensor(ir, pn->input_tensors[0]);
            }
            if (t->dim_num == 4 && t->dims[2] * t->dims[3] != 1) return false;
        }
    }
    if (out_dt == TENGINE_DT_INT8 && n->op.type != OP_FLATTEN && n->op.type != OP_RESHAPE && n->op.type != OP_DROPOUT && n->op.type != OP_CONCAT
        && n->op.type != OP_SOFTMAX && n->op.type != OP_PRIORBOX && n->op.type != OP_TRANSPOSE && n->op.type != OP_SIGMOID && n->op.type != OP_CLIP)
        for (int i = 0; i < n->input_num; i++) {
            struct tensor* t = get_ir_graph_tensor(ir, n->input_tensors[i]);
            if (t->tensor_type != TENSOR_TYPE_CONST && int8_tensor_is_dense_on_device(ir, t)) return false;
        }
    return node_supported(ir, n);
}

// does a run of nodes contain anything worth a device subgraph?  (views and constants alone are not: the hand-over would cost
// more than the CPU device spends on them)
bool op_is_work(int op)
{
    return op != OP_INPUT && op != OP_CONST && op != OP_RESHAPE && op != OP_FLATTEN && op != OP_DROPOUT;
}

struct Piece { std::vector<uint16_t> nodes; struct device* dev; };

// Re-split every subgraph the reference's type-based splitter (split.c:140-312) gave to this device AROUND the nodes the
// device cannot run: maximal runs of supported nodes stay on "HIP", the unsupported nodes (and supported runs without any real
// work) go to the CPU device -- instead of surrendering the whole subgraph for one exotic node.  Node lists are contiguous
// ascending ranges (split.c builds them that way), the list itself runs from the graph's last nodes to its first.
void resplit_around_unsupported(struct graph* ir, struct device* hip)
{
    struct device* cpu = find_default_device();
    std::vector<Piece> pieces;                                   // in list order (descending node ranges)
    const int count = get_vector_num(ir->subgraph_list);
    bool changed = false;
    for (int i = 0; i < count; i++) {
        struct subgraph* sg = *(struct subgraph**)get_vector_data(ir->subgraph_list, i);
        if (sg->device != hip) { pieces.push_back({std::vector<uint16_t>(sg->node_list, sg->node_list + sg->node_num), sg->device}); continue; }
        std::vector<Piece> runs;                                 // ascending inside this subgraph
        for (int j = 0; j < sg->node_num; j++) {
            struct node* n = get_ir_graph_node(ir, sg->node_list[j]);
            struct device* d = node_runs_on_device(ir, n) ? hip : cpu;
            if (runs.empty() || runs.back().dev != d) runs.push_back({{}, d});
            runs.back().nodes.push_back(sg->node_list[j]);
        }
        for (Piece& r : runs) {
            if (r.dev != hip) continue;
            bool work = false;
            for (uint16_t id : r.nodes) work = work || op_is_work(get_ir_graph_node(ir, id)->op.type);
            if (!work) r.dev = cpu;
        }
        if (runs.size() != 1 || runs[0].dev != hip) changed = true;
        for (int r = (int)runs.size() - 1; r >= 0; r--) pieces.push_back(runs[r]);
    }
    if (!changed) return;
    // merge neighbours on the same device (list order is descending: the later piece holds the EARLIER nodes)
    std::vector<Piece> merged;
    for (Piece& p : pieces) {
        if (!merged.empty() && merged.back().dev == p.dev) merged.back().nodes.insert(merged.back().nodes.begin(), p.nodes.begin(), p.nodes.end());
        else merged.push_back(p);
    }
    for (int i = count - 1; i >= 0; i--) {
        struct subgraph* sg = *(struct subgraph**)get_vector_data(ir->subgraph_list, i);
        release_ir_subgraph(ir, sg);
        remove_vector_via_index(ir->subgraph_list, i);
    }
    for (Piece& p : merged) {
        struct subgraph* sg = (struct subgraph*)sys_malloc(sizeof(struct subgraph));
        init_ir_subgraph(ir, sg, 0);
        sg->node_num = (uint16_t)p.nodes.size();
        sg->node_list = (uint16_t*)sys_malloc(sizeof(uint16_t) * p.nodes.size());
        for (size_t j = 0; j < p.nodes.size(); j++) sg->node_list[j] = p.nodes[j];
        sg->device = p.dev;
        push_vector_data(ir->subgraph_list, &sg);
    }
}

// ---- the scheduler half of asynchronous runs -----------------------------------------------------------------
// The reference's only scheduler rejects run_graph(graph, 0) (scheduler.c:75-79) and has no wait (scheduler.c:186-189), so
// interface.async_run / async_wait (device.h:60-63) are unreachable through its API.  The plugin therefore ships a scheduler of the
// reference's own shape (struct scheduler, scheduler.h:34-43) and installs it on the context of every graph it splits:
//   prerun / postrun / run(block = 1): the reference's sync scheduler, unchanged (find_default_scheduler());
//   run(block = 0): a graph that is ONE subgraph on "HIP" is submitted with interface.async_run and the call returns -- up to two
//                   runs in flight (the device pipelines run k+1's upload behind run k's download, csrc/graph_exec.hip); any other
//                   graph (CPU pieces in between) runs to completion right here, which keeps the API's promise trivially;
//   wait:           interface.async_wait for the oldest run in flight; outputs land in the output tensors' buffers then.
// Reference defect to know about: wait_graph() itself can never reach a scheduler -- its status test
// `GRAPH_STAT_RUNNING != status || GRAPH_STAT_READY != status` (c_api.c:588) is always true, it returns -1.  The plugin exports
// hip_wait_graph(graph, try_wait) with the body wait_graph was meant to have; INTEGRATION.md shows the one-token fix.
// State per graph lives in attribute->scheduler_privacy, which the reference releases with sys_free when a graph is destroyed
// without postrun (executer.c:51-53): it is allocated with sys_malloc, a plain struct.
struct HipSchedState { int inflight; int attached; };      // attached: this graph's prerun succeeded and counts in g_sched_live

HipSchedState* sched_state(struct graph* ir_graph)
{
    if (!ir_graph->attribute->scheduler_privacy) {
        HipSchedState* st = (HipSchedState*)sys_malloc(sizeof(HipSchedState));
        if (!st) return nullptr;
        st->inflight = 0;
        st->attached = 0;
        ir_graph->attribute->scheduler_privacy = st;
    }
    return (HipSchedState*)ir_graph->attribute->scheduler_privacy;
}

// A context schedules through hip_scheduler only while graphs that the plugin split AND pre-ran are alive on it: the count per
// context is kept here, and the reference's own scheduler goes back onto the context when the last such graph is post-run.  A graph
// destroyed without postrun_graph (destroy_graph does not call it, c_api.c:662-671) leaves its count behind, and destroy_context has
// no hook, so the map may hold pointers to contexts that no longer exist: they are compared, never dereferenced, outside the calls
// that were handed the context by a live graph.  unregister_hip_device therefore does not walk the contexts; instead
// the library pins itself in memory at registration (RTLD_NODELETE) and hip_scheduler turns into a plain forwarder to the
// reference's scheduler -- a context that still points at it keeps working after the plugin is gone.
std::mutex g_sched_mu;
std::map<struct context*, int> g_sched_live;
std::atomic<bool> g_sched_forward{false};

void sched_attach(struct context* ctx)
{
    std::lock_guard<std::mutex> lk(g_sched_mu);
    g_sched_live[ctx]++;
}

void sched_detach(struct context* ctx);
extern struct scheduler hip_scheduler;

// The one subgraph asynchronous runs are built around: the graph's ONLY subgraph on "HIP", fed by graph inputs alone (nothing
// another subgraph produces).  Everything else of the graph -- the CPU pieces behind it: DetectionOutput of an SSD model, an
// unsupported tail -- runs on the host when the run is collected.  nullptr: the graph cannot be pipelined.
struct subgraph* pipelined_hip_subgraph(struct graph* ir_graph)
{
    struct subgraph* hip = nullptr;
    const int count = get_vector_num(ir_graph->subgraph_list);
    for (int i = 0; i < count; i++) {
        struct subgraph* sg = get_ir_graph_subgraph(ir_graph, i);
        if (sg->device && 0 == strcmp(sg->device->name, HIP_DEV_NAME)) {
            if (hip || !sg->device_graph) return nullptr;
            hip = sg;
        }
    }
    if (!hip) return nullptr;
    for (int i = 0; i < count; i++) {                     // the HIP piece must not wait for anybody
        struct subgraph* sg = get_ir_graph_subgraph(ir_graph, i);
        if (sg == hip) continue;
        for (int k = 0; k < sg->output_num; k++)
            for (int m = 0; m < hip->input_num; m++)
                if (sg->output_tensor_list[k] == hip->input_tensor_list[m]) return nullptr;
    }
    return hip;
}

// the subgraphs behind `done` (everything but the HIP piece), each once all of its producers have run: what the reference's
// scheduler does for the whole graph (scheduler.c:72-181), restated over tensor indices
int run_remaining_subgraphs(struct graph* ir_graph, struct subgraph* done)
{
    const int count = get_vector_num(ir_graph->subgraph_list);
    std::vector<char> ran(count, 0);
    int left = 0;
    for (int i = 0; i < count; i++) {
        if (get_ir_graph_subgraph(ir_graph, i) == done) ran[i] = 1;
        else left++;
    }
    while (left > 0) {
        bool progress = false;
        for (int i = 0; i < count; i++) {
            if (ran[i]) continue;
            struct subgraph* sg = get_ir_graph_subgraph(ir_graph, i);
            bool ready = true;
            for (int j = 0; j < count && ready; j++) {
                if (ran[j] || j == i) continue;
                struct subgraph* other = get_ir_graph_subgraph(ir_graph, j);
                for (int k = 0; k < other->output_num && ready; k++)
                    for (int m = 0; m < sg->input_num; m++)
                        if (other->output_tensor_list[k] == sg->input_tensor_list[m]) { ready = false; break; }
            }
            if (!ready) continue;
            sg->status = GRAPH_STAT_RUNNING;
            if (sg->device->interface->run(sg->device, sg) < 0) {
                TLOG_ERR("Tengine HIP scheduler: run subgraph %d error!\n", sg->index);
                sg->status = GRAPH_STAT_ERROR;
                return -1;
            }
            sg->status = GRAPH_STAT_READY;
            ran[i] = 1; left--; progress = true;
        }
        if (!progress) { TLOG_ERR("Tengine HIP scheduler: no subgraph is ready, %d still waiting\n", left); return -1; }
    }
    return 0;
}

int hip_sched_prerun(struct scheduler* s, struct graph* g)
{
    (void)s;
    struct scheduler* d = find_default_scheduler();
    const int rc = d->prerun(d, g);
    if (g_sched_forward.load()) return rc;
    struct context* ctx = g->attribute->context;
    HipSchedState* st = rc == 0 ? sched_state(g) : nullptr;
    if (st && !st->attached) { st->attached = 1; sched_attach(ctx); }
    if (rc != 0) {          // a failed prerun attaches nothing: with no other live graph the context goes back to the reference's scheduler
        std::lock_guard<std::mutex> lk(g_sched_mu);
        if (g_sched_live.find(ctx) == g_sched_live.end() && ctx->scheduler == &hip_scheduler) ctx->scheduler = d;
    }
    return rc;
}

int hip_sched_wait(struct scheduler* s, struct graph* ir_graph)
{
    (void)s;
    if (g_sched_forward.load()) { struct scheduler* d = find_default_scheduler(); return d->wait ? d->wait(d, ir_graph) : -1; }
    HipSchedState* st = sched_state(ir_graph);
    if (!st) return -1;
    if (st->inflight == 0) { ir_graph->status = GRAPH_STAT_READY; return 0; }
    struct subgraph* sg = pipelined_hip_subgraph(ir_graph);
    if (!sg || sg->device->interface->async_wait(sg->device, sg, 0) != 0) { ir_graph->status = GRAPH_STAT_ERROR; return -1; }
    // the device part of the OLDEST run is in the subgraph's output tensors now: the host pieces behind it consume them here,
    // before the next wait delivers the next run's
    if (run_remaining_subgraphs(ir_graph, sg) != 0) { ir_graph->status = GRAPH_STAT_ERROR; return -1; }
    if (--st->inflight == 0) { sg->status = GRAPH_STAT_READY; ir_graph->status = GRAPH_STAT_READY; }
    return 0;
}

int hip_sched_run(struct scheduler* s, struct graph* ir_graph, int block)
{
    struct scheduler* d = find_default_scheduler();
    if (g_sched_forward.load()) return d->run(d, ir_graph, block);
    HipSchedState* st = sched_state(ir_graph);
    if (!st) return -1;
    if (block) {
        while (st->inflight > 0)                         // a blocking run behind asynchronous ones: results stay in order
            if (hip_sched_wait(s, ir_graph) != 0) return -1;
        return d->run(d, ir_graph, 1);
    }
    struct subgraph* sg = pipelined_hip_subgraph(ir_graph);
    if (!sg) return d->run(d, ir_graph, 1);              // no single leading HIP piece: complete before returning (wait then has nothing to do)
    if (st->inflight >= 2) { TLOG_ERR("Tengine HIP: two asynchronous runs are already in flight: wait_graph first\n"); return -1; }
    sg->status = GRAPH_STAT_RUNNING;
    if (sg->device->interface->async_run(sg->device, sg) != 0) { sg->status = GRAPH_STAT_ERROR; return -1; }
    st->inflight++;
    return 0;
}

int hip_sched_postrun(struct scheduler* s, struct graph* ir_graph)
{
    const bool fwd = g_sched_forward.load();
    while (!fwd && ir_graph->attribute->scheduler_privacy && sched_state(ir_graph)->inflight > 0)
        if (hip_sched_wait(s, ir_graph) != 0) break;
    struct scheduler* d = find_default_scheduler();
    const int rc = d->postrun(d, ir_graph);
    bool attached = false;
    if (ir_graph->attribute->scheduler_privacy) {
        attached = ((HipSchedState*)ir_graph->attribute->scheduler_privacy)->attached != 0;
        sys_free(ir_graph->attribute->scheduler_privacy);
        ir_graph->attribute->scheduler_privacy = nullptr;
    }
    if (attached && !fwd) sched_detach(ir_graph->attribute->context);      // only a graph that attached detaches (a failed prerun never did)
    return rc;
}

struct scheduler hip_scheduler = {"hip_pipelined", hip_sched_prerun, hip_sched_run, hip_sched_wait, hip_sched_postrun, nullptr};

void sched_detach(struct context* ctx)
{
    std::lock_guard<std::mutex> lk(g_sched_mu);
    auto it = g_sched_live.find(ctx);
    if (it == g_sched_live.end()) return;
    if (--it->second <= 0) {
        g_sched_live.erase(it);
        if (ctx->scheduler == &hip_scheduler) ctx->scheduler = find_default_scheduler();
    }
}

int hip_split_graph(struct graph* ir_graph)
{
    struct device* cur_dev = ir_graph->attribute->context->device;
    if (0 != strcmp(HIP_DEV_NAME, cur_dev->name)) return -1;
    // split_graph runs inside prerun_graph, before the context's scheduler is asked to pre-run (c_api.c:468-530): from here on
    // this context schedules through the plugin's scheduler (TG_HIP_SCHEDULER=0 keeps the reference's)
    if (!(getenv("TG_HIP_SCHEDULER") && atoi(getenv("TG_HIP_SCHEDULER")) == 0))
        ir_graph->attribute->context->scheduler = &hip_scheduler;      // (the context is counted when this graph's prerun succeeds: hip_sched_prerun)

    int graph_dt = -1;
    if (ir_graph->input_num > 0) {
        struct node* in_node = get_ir_graph_node(ir_graph, ir_graph->input_nodes[0]);
        if (in_node->output_num > 0) graph_dt = get_ir_graph_tensor(ir_graph, in_node->output_tensors[0])->data_type;
    }
    struct vector* allowed_ops = create_vector(sizeof(int), nullptr);
    struct vector* blocked_ops = create_vector(sizeof(int), nullptr);
    struct vector* precision = create_vector(sizeof(int), nullptr);
    fill_op_lists(allowed_ops, blocked_ops, precision, graph_dt);      // (a quantised graph: the quantised-only operators are allowed too)
    split_graph_node_to_sub_graph(ir_graph, allowed_ops, blocked_ops, precision);
    release_vector(allowed_ops);
    release_vector(blocked_ops);
    release_vector(precision);

    // split.c decides by operator TYPE and lets every quantised tensor through its precision test (split.c:53-66): nodes whose
    // parameters / dtypes the kernels cannot express are cut out of the device subgraphs before IO generation
    resplit_around_unsupported(ir_graph, cur_dev);

    generate_sub_graph_io(ir_graph);
    add_sub_graph_to_ir_graph(ir_graph);

    for (int i = 0; i < (uint16_t)get_vector_num(ir_graph->subgraph_list); i++) {
        struct subgraph* sub_graph = *(struct subgraph**)get_vector_data(ir_graph->subgraph_list, i);
        sub_graph->index = i;
        for (uint16_t j = 0; j < sub_graph->node_num; j++) {
            struct node* ir_node = get_ir_graph_node(ir_graph, sub_graph->node_list[j]);
            ir_node->subgraph_idx = sub_graph->index;
        }
    }
    return 0;
}

struct interface hip_interface = {
    hip_dev_init, hip_dev_prerun, hip_dev_run, hip_dev_postrun, hip_dev_async_run, hip_dev_async_wait, hip_release_graph, hip_dev_release,
};
struct allocator hip_allocator = {hip_describe, hip_evaluation, hip_allocate, hip_release};
struct optimizer hip_optimizer = {hip_split_graph, nullptr};
struct device hip_device = {HIP_DEV_NAME, &hip_interface, &hip_allocator, &hip_optimizer, nullptr, nullptr};

}  // namespace

extern "C" {

__attribute__((visibility("default"))) int register_hip_device(void)
{
    int ret = register_device(&hip_device);
    if (0 != ret) {
        TLOG_INFO("Tengine plugin %s register failed.\n", hip_device.name);
        return -1;
    }
    // the plugin hands contexts a pointer into this library (hip_scheduler): keep the library mapped for the life of the process, so
    // that a context which outlives unload_tengine_plugin still points at valid (then forwarding) code -- see g_sched_live
    // (pinned ONCE: a second registration must not leak another handle -- ADVICE r5.  Between split_graph and the scheduler's prerun the
    //  reference has no failing step for a device without optimize_graph (c_api.c:476-527), and hip_split_graph fails only BEFORE it
    //  touches the context, so a context is never left on hip_scheduler by a failed split; graphs destroyed without postrun_graph and
    //  graphs attached before an unregister / re-register keep their HipSchedState with a stale `attached`: the counts of g_sched_live
    //  are a lower bound after that, which only means a context may go back to the reference's scheduler one graph early -- the forwarder
    //  path of hip_scheduler handles every graph either way)
    static std::atomic<bool> pinned{false};
    Dl_info me;
    if (!pinned.exchange(true) && dladdr((void*)&register_hip_device, &me) && me.dli_fname) (void)dlopen(me.dli_fname, RTLD_NOW | RTLD_NODELETE);
    g_sched_forward.store(false);
    TLOG_INFO("Tengine plugin device %s is registered.\n", hip_device.name);
    return 0;
}

// What the reference's wait_graph() was meant to do (its own status test makes it return -1 unconditionally, c_api.c:583-603):
// 0 when the OLDEST asynchronous run_graph(graph, 0) has completed and its outputs are in the output tensors' buffers.
__attribute__((visibility("default"))) int hip_wait_graph(void* graph, int try_wait)
{
    (void)try_wait;
    struct graph* ir = (struct graph*)graph;
    struct scheduler* sch = ir->attribute->context->scheduler;
    return sch->wait(sch, ir);
}

// how many subgraphs were compiled as two half-batch device graphs so far (tests: the split is asserted, not assumed)
__attribute__((visibility("default"))) int hip_device_split_subgraphs(void) { return g_split_subgraphs; }

// Introspection for tests and tools: where did the splitter put the nodes of a prerun graph?  One line per subgraph,
// "<index> <device name> <nodes> <nodes that are not Input/Const> <their operator names, comma separated>"; returns the number of
// subgraphs, or -1 when `cap` is too small.  (struct graph is the reference's own; this library is compiled against its headers.)
__attribute__((visibility("default"))) int hip_device_placement(void* graph, char* buf, int cap)
{
    struct graph* ir = (struct graph*)graph;
    int used = 0;
    const int count = get_vector_num(ir->subgraph_list);
    for (int i = 0; i < count; i++) {
        struct subgraph* sg = *(struct subgraph**)get_vector_data(ir->subgraph_list, i);
        int real = 0;
        std::string ops;
        for (int j = 0; j < sg->node_num; j++) {
            const int op = get_ir_graph_node(ir, sg->node_list[j])->op.type;
            if (op == OP_INPUT || op == OP_CONST) continue;
            const char* nm = find_op_name(op);
            ops += (real ? "," : "") + (nm ? std::string(nm) : std::to_string(op));
            real++;
        }
        const int n = snprintf(buf + used, cap > used ? (size_t)(cap - used) : 0, "%d %s %d %d %s\n", i, sg->device ? sg->device->name : "?", (int)sg->node_num, real, ops.c_str());
        if (n < 0 || used + n >= cap) return -1;
        used += n;
    }
    return count;
}

__attribute__((visibility("default"))) int unregister_hip_device(void)
{
    {   // contexts are not walked (they may have been destroyed: see g_sched_live): from now on hip_scheduler only forwards to the
        // reference's scheduler, and the library stays mapped (register_hip_device pinned it), so a context still pointing here is safe
        std::lock_guard<std::mutex> lk(g_sched_mu);
        g_sched_forward.store(true);
        g_sched_live.clear();
    }
    int ret = unregister_device(&hip_device);
    if (0 != ret) {
        TLOG_INFO("Tengine plugin %s unregister failed.\n", hip_device.name);
        return ret;
    }
    TLOG_INFO("Tengine plugin device %s is unregistered.\n", hip_device.name);
    return 0;
}
}
