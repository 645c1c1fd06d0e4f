// The byte-map node planners: nodes that move or map bytes without arithmetic between tensors -- Sigmoid / Clip / HardSwish / Mish by
// table (plan_lut), the scalar and the unary Eltwise by table (plan_eltwise_table), byte-pure chains of such nodes as ONE table (bytemap_chain_from, plan_bytemap_chain), the uint8 BatchNorm and InstanceNorm (a byte map per channel / per plane, the latter computed on the device), PReLU, nearest Interp, the uint8 Slice, the uint8 Crop (alone, inside the Interp's launch, or with both inside the Eltwise's), Transpose, Split, ShuffleChannel and Concat + ShuffleChannel.  plan_lut, plan_prelu,
// plan_interp and plan_transpose serve int8 (NHWC) and uint8 (NCHW) graphs alike; the channel maps have an int8 form (chan_map_i8, called by plan_i8, declared in
// graph_plan.h) and a uint8 form (chan_map_u8, called by plan_u8, declared in graph.h).  Each hands its launches back in `out`.
#include "graph.h"
#include "graph_internal.h"
#include "env.h"

#include <cstring>

#include "graph_plan.h"

namespace tamd {

// Sigmoid / Clip / HardSwish / Mish, int8 and uint8 graphs alike (graph_u8.hip calls this too): the node's 256-entry byte map is built
// on the host with the reference's arithmetic (lut_tables.cc), uploaded once here, and applied by one lut_u8 launch (misc_kernels.hip).
// An NHWC int8 tensor with padding lanes (cs > c) is mapped channel by channel and its padding is written as zero; everything else --
// uint8 tensors, dense int8 tensors, NHWC tensors without padding -- is a run of bytes.  A concat view is refused by name, as plan_relu
// does: neither planner makes one of these nodes' tensors a view (plan_concat_views: slice_capable; plan_u8: in_place), so the error
// guards a change to those lists.
static const char* lut_name(int op) { return op == TAMD_OP_SIGMOID ? "sigmoid" : op == TAMD_OP_CLIP ? "clip" : op == TAMD_OP_HARDSWISH ? "hardswish" : "mish"; }

// the byte table of one of these nodes between its two tensors, uploaded: what plan_lut applies with lut_u8 and plan_chan_gate inside
// the gate's launch
static int lut_table_upload(tamd_graph* g, const HNode& n, unsigned** dtable)
{
    const HTensor& x = g->tensors[n.in[0]];
    const HTensor& y = g->tensors[n.out[0]];
    const char* what = lut_name(n.op);
    if (x.scales.empty() || y.scales.empty()) { set_error("%s %s: missing quant params", what, n.name.c_str()); return -1; }
    if (x.dims != y.dims || x.dtype != y.dtype) { set_error("%s %s: output shape / type mismatch", what, n.name.c_str()); return -1; }
    if (!lut_rank_on_device(n.op, (int)x.dims.size())) { set_error("%s %s: only a 4-D tensor runs on the device", what, n.name.c_str()); return -1; }
    const void* param = n.op == TAMD_OP_CLIP ? (const void*)&n.p.clip : n.op == TAMD_OP_HARDSWISH ? (const void*)&n.p.hardswish : nullptr;
    std::vector<unsigned> table(64);
    if (tamd_lut_table(n.op, x.dtype, param, x.scales[0], x.zps.empty() ? 0 : x.zps[0], y.scales[0], y.zps.empty() ? 0 : y.zps[0], (unsigned char*)table.data())) {
        set_error("%s %s: not supported on the device for data type %d", what, n.name.c_str(), x.dtype);
        return -1;
    }
    return upload(g, table, dtable);
}

// one lut_u8 launch from x to y through an uploaded table: an NHWC int8 tensor with padding lanes channel by channel, else a run of bytes
static int lut_step(const std::string& node, const char* what, HTensor& x, HTensor& y, const unsigned* dtable, std::vector<Step>* out)
{
    if (x.is_view || y.is_view) { set_error("%s %s on a concat view is not supported", what, node.c_str()); return -1; }
    LutArgs a{};
    a.x = (const uint8_t*)x.dptr; a.y = (uint8_t*)y.dptr; a.table = dtable;
    const bool x_nhwc = !x.nchw_raw && x.cs > 0, y_nhwc = !y.nchw_raw && y.cs > 0;
    if (x_nhwc != y_nhwc || (x_nhwc && (x.cs != y.cs || x.cs % 16 || x.c_off || y.c_off))) { set_error("%s %s: input and output layouts differ", what, node.c_str()); return -1; }
    if (x_nhwc) {
        a.count = (size_t)x.n * x.h * x.w * x.cs;
        if (x.cs != x.c) { a.C = x.c; a.cs = x.cs; }
    } else {
        a.count = x.elems();
    }
    out->push_back(make_step(node, "lut_u8", 0, 2.0 * (double)x.elems(), [a](hipStream_t s) { return launch_lut(a, s); }, {access_of(x)}, {access_of(y)}, false));
    return 0;
}

int plan_lut(tamd_graph* g, HNode& n, std::vector<Step>* out)
{
    HTensor& x = g->tensors[n.in[0]];
    HTensor& y = g->tensors[n.out[0]];
    const char* what = lut_name(n.op);
    if (x.is_view || y.is_view) { set_error("%s %s on a concat view is not supported", what, n.name.c_str()); return -1; }
    unsigned* dtable = nullptr;
    if (lut_table_upload(g, n, &dtable)) return -1;
    return lut_step(n.name, what, x, y, dtable, out);
}

const char* eltwise_refusal_of(const tamd_graph* g, const HNode& n, int* gated, unsigned char* table)
{
    *gated = -1;
    if ((n.in.size() != 1 && n.in.size() != 2) || n.out.empty()) return "Eltwise runs on the device on two tensors";
    const HTensor& a = g->tensors[n.in[0]];
    const HTensor& b = g->tensors[n.in.back()];                    // (one input: unread)
    const HTensor& y = g->tensors[n.out[0]];
    EltwiseValues v{};
    const bool have_q = a.scales.size() == 1 && y.scales.size() == 1;
    if (have_q) {
        v.x_scale = a.scales[0]; v.x_zp = a.zps.empty() ? 0 : a.zps[0];
        v.out_scale = y.scales[0]; v.out_zp = y.zps.empty() ? 0 : y.zps[0];
        if (n.in.size() == 2 && b.ttype == TAMD_TT_CONST && b.data.size() >= (size_t)esize(b.dtype)) {
            v.c_data = b.data.data(); v.c_scale = b.scales.empty() ? 0.f : b.scales[0]; v.c_zp = b.zps.empty() ? 0 : b.zps[0];
        }
    }
    return eltwise_refusal(&n.p.elt, a.dtype, (int)n.in.size(), (int)a.dims.size(), a.dims.data(), a.ttype == TAMD_TT_CONST, a.scales.size(), (int)b.dims.size(), b.dims.data(),
                           b.ttype == TAMD_TT_CONST, b.scales.size(), y.scales.size(), gated, b.dtype, have_q ? &v : nullptr, table);
}

// The scalar and the unary Eltwise (eltwise_refusal: kEltScalar, kEltUnary), int8 and uint8 graphs alike: the node's byte map through
// one lut_u8 launch, exactly as plan_lut applies a Sigmoid's -- an NHWC int8 tensor with padding lanes channel by channel, its padding
// written as zero, everything else a run of bytes.  The constant is read here, at prerun, and never again
int plan_eltwise_table(tamd_graph* g, HNode& n, std::vector<Step>* out)
{
    int form = -1;
    std::vector<unsigned> table(64);
    const char* why = eltwise_refusal_of(g, n, &form, (unsigned char*)table.data());
    if (why) { set_error("eltwise %s: %s", n.name.c_str(), why); return -1; }
    HTensor& x = g->tensors[n.in[0]];
    HTensor& y = g->tensors[n.out[0]];
    if (form != kEltScalar && form != kEltUnary) { set_error("eltwise %s: not a scalar or unary form", n.name.c_str()); return -1; }
    if (form == kEltScalar && g->tensors[n.in[1]].data.size() < (size_t)esize(g->tensors[n.in[1]].dtype)) { set_error("eltwise %s: the constant has no value", n.name.c_str()); return -1; }
    if (x.dims != y.dims || x.dtype != y.dtype) { set_error("eltwise %s: output shape / type mismatch", n.name.c_str()); return -1; }
    unsigned* dtable = nullptr;
    if (upload(g, table, &dtable)) return -1;
    return lut_step(n.name, "eltwise", x, y, dtable, out);
}

// ---- uint8 BatchNorm: a byte map per channel ----
const char* batchnorm_refusal_of(const tamd_graph* g, const HNode& n, std::vector<unsigned>* tables)
{
    if (n.in.size() != 5 || n.out.empty()) return "BatchNorm takes five inputs: the data, gamma, beta, mean and var";
    const HTensor& x = g->tensors[n.in[0]];
    const HTensor& y = g->tensors[n.out[0]];
    BnStat st[4];
    for (int k = 0; k < 4; k++) {
        const HTensor& t = g->tensors[n.in[k + 1]];
        const bool whole = t.dtype == TAMD_DT_FP32 && t.data.size() >= t.elems() * 4;
        st[k] = BnStat{t.dtype, t.ttype == TAMD_TT_CONST, t.elems(), whole ? (const float*)t.data.data() : nullptr};
    }
    EltwiseValues v{};
    const bool have_q = x.scales.size() == 1 && y.scales.size() == 1;
    if (have_q) { v.x_scale = x.scales[0]; v.x_zp = x.zps.empty() ? 0 : x.zps[0]; v.out_scale = y.scales[0]; v.out_zp = y.zps.empty() ? 0 : y.zps[0]; }
    return batchnorm_refusal(&n.p.bn, x.dtype, (int)n.in.size(), (int)x.dims.size(), x.dims.data(), x.ttype == TAMD_TT_CONST, x.scales.size(), y.scales.size(), st,
                             have_q ? &v : nullptr, tables);
}

// batchnorm_kernel_ref_uint8.c:40-107 is a function of one byte and its channel: the C tables are built at prerun and uploaded once.
// Planes of at least kBnPlaneForm bytes go through prelu_u8's per-plane form (its arguments already are [C][64] tables), smaller ones --
// the [N,C] output of a FullyConnected, H * W = 1, included -- through chan_lut_u8 (chan_lut.hip); TAMD_PIN=bn_form=0 | 1 forces
// chan_lut_u8 | the per-plane form.  Measured (profiles/bytemap_chains.txt): chan_lut_u8 takes 3.0 us at every size up to 200 KB; the
// per-plane form is behind it with the ranges apart on [32,128] (3.79 us) and on planes of 49 and 196 bytes (3.61, 3.67 us), and level
// with it -- the ranges touch -- on planes of 784 and 3136 bytes and on [1,128]: it is ahead nowhere.  The threshold stands at the
// first power of two above the sizes where chan_lut_u8 wins; from there on the choice is free as far as it was measured
static const int kBnPlaneForm = 1024;
int plan_batchnorm_u8(tamd_graph* g, HNode& n, std::vector<Step>* out)
{
    std::vector<unsigned> tables;
    const char* why = batchnorm_refusal_of(g, n, &tables);
    if (why) { set_error("batchnorm %s: %s", n.name.c_str(), why); return -1; }
    HTensor& x = g->tensors[n.in[0]];
    HTensor& y = g->tensors[n.out[0]];
    if (x.is_view || y.is_view || !x.nchw_raw || !y.nchw_raw) { set_error("batchnorm %s on a concat view is not supported in a uint8 graph", n.name.c_str()); return -1; }
    if (x.dims != y.dims || x.dtype != y.dtype) { set_error("batchnorm %s: output shape / type mismatch", n.name.c_str()); return -1; }
    const int C = x.dims[1];
    if (tables.size() != (size_t)C * 64) { set_error("batchnorm %s: the statistics have no values", n.name.c_str()); return -1; }
    size_t hw = 1;
    for (size_t i = 2; i < x.dims.size(); i++) hw *= (size_t)x.dims[i];
    if (hw > 0x7fffffffu) { set_error("batchnorm %s: a plane of more than 2^31 bytes", n.name.c_str()); return -1; }
    unsigned* dtables = nullptr;
    if (upload(g, tables, &dtables)) return -1;
    const int form = tamd_pin_int("bn_form", hw >= (size_t)kBnPlaneForm ? 1 : 0);
    if (form == 1) {
        PreluU8Args a{};
        a.x = (const uint8_t*)x.dptr; a.y = (uint8_t*)y.dptr; a.planes = (long)x.dims[0] * C; a.C = C; a.HW = (int)hw; a.tables = dtables; a.shared = 0;
        out->push_back(make_step(n.name, "prelu_u8", 0, 2.0 * (double)x.elems(), [a](hipStream_t s) { return launch_prelu_u8(a, s); }, {access_of(x)}, {access_of(y)}, false));
    } else {
        ChanLutU8Args a{};
        a.x = (const uint8_t*)x.dptr; a.y = (uint8_t*)y.dptr; a.total = x.elems(); a.C = C; a.HW = (int)hw; a.tables = dtables;
        out->push_back(make_step(n.name, "chan_lut_u8", 0, 2.0 * (double)x.elems(), [a](hipStream_t s) { return launch_chan_lut_u8(a, s); }, {access_of(x)}, {access_of(y)}, false));
    }
    return 0;
}

// ---- uint8 InstanceNorm: a byte map per PLANE, computed on the device (instnorm.hip) ----
const char* instancenorm_refusal_of(const tamd_graph* g, const HNode& n)
{
    if (n.in.size() != 3 || n.out.empty()) return "InstanceNorm takes three inputs: the data, gamma and beta";
    const HTensor& x = g->tensors[n.in[0]];
    const HTensor& y = g->tensors[n.out[0]];
    InStat st[2];
    for (int k = 0; k < 2; k++) {
        const HTensor& t = g->tensors[n.in[k + 1]];
        const bool whole = t.dtype == TAMD_DT_FP32 && t.data.size() >= t.elems() * 4;
        st[k] = InStat{t.dtype, t.ttype == TAMD_TT_CONST, t.elems(), whole ? (const float*)t.data.data() : nullptr};
    }
    const bool have_q = x.scales.size() == 1 && y.scales.size() == 1;
    return instancenorm_refusal(&n.p.inorm, x.dtype, (int)n.in.size(), (int)x.dims.size(), x.dims.data(), x.ttype == TAMD_TT_CONST, x.scales.size(), y.scales.size(), st, have_q,
                                have_q ? x.scales[0] : 0.f, have_q ? y.scales[0] : 0.f, have_q && !y.zps.empty() ? y.zps[0] : 0);
}

// conv -> InstanceNorm -> ReLU is the universal generator block, and the uint8 ReLU is one byte to one byte (relu_kernel_ref_uint8.c):
// where a plain or leaky ReLU is the InstanceNorm output's only reader and that tensor is no graph output, the ReLU is composed into
// the plane's map on the device and the tensor between is never written.  The ReLU node's index, -1: none (TAMD_PIN=instnorm_relu=0)
int instancenorm_relu_next(const tamd_graph* g, size_t ni)
{
    const HNode& n = g->nodes[ni];
    if (n.op != TAMD_OP_INSTANCENORM || n.out.size() != 1 || !tamd_pin_int("instnorm_relu", 1) || count_consumers(g, n.out[0]) != 1) return -1;
    for (auto& o : g->outputs) if (o.tensor == n.out[0]) return -1;
    for (size_t nj = ni + 1; nj < g->nodes.size(); nj++) {
        const HNode& r = g->nodes[nj];
        if (r.op != TAMD_OP_RELU || r.in.size() != 1 || r.out.size() != 1 || r.in[0] != n.out[0]) continue;
        const HTensor& y = g->tensors[r.out[0]];
        if (y.scales.size() != 1 || y.dims != g->tensors[n.out[0]].dims || y.dtype != TAMD_DT_UINT8 || y.is_view) return -1;
        return (int)nj;
    }
    return -1;
}

// Which form runs where nothing is pinned, as measured (profiles/instnorm.txt, the committed kernels): as launches the one-launch form is
// ahead with the ranges apart on planes of 256, 1024 and 4096 bytes (6.31 against 8.30, 12.27 against 14.37, 41.85 against 43.52 us; at
// batch 8 x 128 planes of 1024 bytes 15.18 against 17.66 us) -- it saves the second launch and the round trip of the maps -- and BEHIND with
// the ranges apart on planes of 16384 bytes (163.1 against 161.3 us), where its apply step runs on 32 waves instead of the whole device.
// Through the plugin it is ahead with the ranges apart at (1,128,32,32) (72.0 - 73.8 against 74.7 - 74.9 us); at (1,64,64,64) and
// (1,32,128,128) the ranges overlap.  So one launch is the default up to the largest plane at which it was measured ahead, and two launches
// stay the default above it, where nothing between 4096 and 16384 bytes was measured
static const size_t kInstNormOneLaunchMaxPlane = 4096;
int instancenorm_form(size_t plane_bytes) { return tamd_pin_int("instnorm_form", plane_bytes <= kInstNormOneLaunchMaxPlane ? 1 : 0) == 1 ? 1 : 0; }

// form 0: instnorm_stats_u8 writes the planes' maps into a scratch buffer planned here, chan_lut_u8 (C := N * C) applies them;
// form 1: instnorm_u8 does both.  relu (may be null): the ReLU node composed into the map; the launch then writes ITS output
int plan_instancenorm_u8(tamd_graph* g, HNode& n, const HNode* relu, std::vector<Step>* out)
{
    const char* why = instancenorm_refusal_of(g, n);
    if (why) { set_error("instancenorm %s: %s", n.name.c_str(), why); return -1; }
    HTensor& x = g->tensors[n.in[0]];
    HTensor& mid = g->tensors[n.out[0]];
    HTensor& y = relu ? g->tensors[relu->out[0]] : mid;
    const HTensor& gm = g->tensors[n.in[1]];
    const HTensor& bt = g->tensors[n.in[2]];
    if (x.is_view || y.is_view || !x.nchw_raw || !y.nchw_raw) { set_error("instancenorm %s on a concat view is not supported in a uint8 graph", n.name.c_str()); return -1; }
    if (x.dims != y.dims || x.dims != mid.dims || x.dtype != y.dtype) { set_error("instancenorm %s: output shape / type mismatch", n.name.c_str()); return -1; }
    const size_t C = (size_t)x.dims[1];
    if (gm.data.size() < C * 4 || bt.data.size() < C * 4) { set_error("instancenorm %s: gamma / beta have no values", n.name.c_str()); return -1; }
    std::vector<float> hg((const float*)gm.data.data(), (const float*)gm.data.data() + C), hb((const float*)bt.data.data(), (const float*)bt.data.data() + C);
    float *dg = nullptr, *db = nullptr;
    if (upload(g, hg, &dg) || upload(g, hb, &db)) return -1;
    InstNormU8Args a{};
    a.x = (const uint8_t*)x.dptr; a.y = (uint8_t*)y.dptr;
    a.planes = (long)x.dims[0] * x.dims[1]; a.C = x.dims[1]; a.HW = x.dims[2] * x.dims[3];
    a.gamma = dg; a.beta = db; a.eps = n.p.inorm.eps;
    auto q_of = [](const HTensor& t) { return U8Q{t.scales[0], t.zps.empty() ? 0 : t.zps[0]}; };      // (one pair each: the refusal, instancenorm_relu_next)
    if (y.scales.size() != 1) { set_error("instancenorm %s: the ReLU's output needs per-tensor quant params", n.name.c_str()); return -1; }
    a.in = q_of(x); a.out = q_of(mid);
    if (relu) { a.relu.on = 1; a.relu.slope = relu->p.relu.negative_slope; a.relu.out = q_of(y); }
    const std::string node = relu ? n.name + "+" + relu->name : n.name;
    const double chain = 2.0 * (double)x.elems();
    if (instancenorm_form((size_t)a.HW) == 1) {
        out->push_back(make_step(node, "instnorm_u8", 0, 3.0 * (double)x.elems() + (double)y.elems(), [a](hipStream_t s) { return launch_instnorm_u8(a, s); }, {access_of(x)},
                                 {access_of(y)}, false));
    } else {
        const size_t dwords = (size_t)a.planes * 64;
        unsigned* dtables = nullptr;
        if (upload(g, std::vector<unsigned>(dwords, 0u), &dtables)) return -1;      // the scratch maps: written by every run before they are read
        a.tables = dtables;
        const Access scratch = access_of_bytes(dtables, dwords * 4);
        out->push_back(make_step(node, "instnorm_stats_u8", 0, chain + (double)dwords * 4, [a](hipStream_t s) { return launch_instnorm_stats_u8(a, s); }, {access_of(x)},
                                 {scratch}, false));
        ChanLutU8Args l{};
        l.x = a.x; l.y = a.y; l.total = x.elems(); l.C = (int)a.planes; l.HW = a.HW; l.tables = dtables;
        out->push_back(make_step(node, "chan_lut_u8", 0, 2.0 * (double)x.elems(), [l](hipStream_t s) { return launch_chan_lut_u8(l, s); }, {access_of(x), scratch},
                                 {access_of(y)}, false));
    }
    if (relu) {
        if (g->fused_away.size() != g->tensors.size()) g->fused_away.assign(g->tensors.size(), 0);
        g->fused_away[n.out[0]] = 1;                                                // never written
    }
    return 0;
}

// ---- byte-pure chains as ONE table ----
// A node whose output byte depends on ONE byte of a tensor S alone is byte-pure over S: a table node (Sigmoid / Clip / HardSwish / Mish,
// the scalar and the unary Eltwise) that reads S or a byte-pure tensor, and a same-shape PROD / SUM / SUB / MAX whose operands are both
// S or byte-pure over the same S -- x * sigmoid(x), x * clip(x + 3, 0, 6) / 6.  The value of every such tensor is known for each of the
// 256 bytes S can hold, so the chain is evaluated node by node on the host -- table2[table1[b]], tamd_eltwise_pair(val_a[b], val_b[b]):
// the reference's own arithmetic at every node -- and runs as one lut_u8 launch from S to the chain's last tensor; what lies between is
// never written.  The bytes are the node-by-node bytes by construction.

// the table of a table node between its two tensors; false: no table node, or one the device does not run alone either
static bool byte_node_table(const tamd_graph* g, const HNode& n, unsigned char table[256])
{
    if (n.in.empty() || n.out.size() != 1) return false;
    const HTensor& x = g->tensors[n.in[0]];
    const HTensor& y = g->tensors[n.out[0]];
    if (x.ttype == TAMD_TT_CONST || x.scales.size() != 1 || y.scales.size() != 1 || x.dims != y.dims || x.dtype != y.dtype) return false;
    if (is_lut_op(n.op)) {
        if (n.in.size() != 1 || !lut_op_on_device(n.op, x.dtype) || !lut_rank_on_device(n.op, (int)x.dims.size())) return false;
        const void* param = n.op == TAMD_OP_CLIP ? (const void*)&n.p.clip : n.op == TAMD_OP_HARDSWISH ? (const void*)&n.p.hardswish : nullptr;
        return tamd_lut_table(n.op, x.dtype, param, x.scales[0], x.zps.empty() ? 0 : x.zps[0], y.scales[0], y.zps.empty() ? 0 : y.zps[0], table) == 0;
    }
    if (n.op != TAMD_OP_ELTWISE) return false;
    int form = kEltSame;
    return eltwise_refusal_of(g, n, &form, table) == nullptr && (form == kEltScalar || form == kEltUnary);
}

bool bytemap_chain_from(const tamd_graph* g, size_t ni, const std::function<bool(int)>& node_free, const std::function<bool(int)>& tensor_plain, ByteChain* c)
{
    if (!tamd_pin_int("bytemap_chain", 1)) return false;
    const HNode& first = g->nodes[ni];
    unsigned char tab[256];
    if (!node_free((int)ni) || !byte_node_table(g, first, tab)) return false;
    const int src = first.in[0];
    if (!tensor_plain(src)) return false;
    const int dtype = g->tensors[src].dtype;
    if (dtype != TAMD_DT_INT8 && dtype != TAMD_DT_UINT8) return false;
    // val[t][b]: the byte tensor t holds where S holds b
    std::vector<std::vector<unsigned char>> val(g->tensors.size());
    val[src].resize(256);
    for (int b = 0; b < 256; b++) val[src][b] = (unsigned char)b;
    std::vector<int> members;
    auto q = [&](int t, float* s, int* z) { *s = g->tensors[t].scales[0]; *z = g->tensors[t].zps.empty() ? 0 : g->tensors[t].zps[0]; };
    for (size_t nj = ni; nj < g->nodes.size(); nj++) {
        const HNode& n = g->nodes[nj];
        if (n.op == TAMD_OP_INPUT || n.op == TAMD_OP_CONST || n.in.empty() || n.out.size() != 1 || !node_free((int)nj) || !tensor_plain(n.out[0])) continue;
        const int x = n.in[0], y = n.out[0];
        std::vector<unsigned char> v(256);
        if (!val[x].empty() && byte_node_table(g, n, tab)) {                                                   // a table node behind S or a member
            for (int b = 0; b < 256; b++) v[b] = tab[val[x][b]];
        } else if (n.op == TAMD_OP_ELTWISE && n.in.size() == 2 && !val[x].empty() && !val[n.in[1]].empty()) {
            int form = 0;                                                                                     // same shape: both operands S or members
            if (eltwise_refusal_of(g, n, &form) || form != kEltSame || g->tensors[x].dims != g->tensors[y].dims || g->tensors[y].scales.size() != 1) continue;
            float sa, sb, so; int za, zb, zo;
            q(x, &sa, &za); q(n.in[1], &sb, &zb); q(y, &so, &zo);
            bool defined = true;
            for (int b = 0; b < 256 && defined; b++) {
                const int r = tamd_eltwise_pair(n.p.elt.type, dtype, val[x][b], sa, za, val[n.in[1]][b], sb, zb, so, zo);
                defined = r >= 0;
                v[b] = (unsigned char)r;
            }
            if (!defined) continue;
        } else {
            continue;
        }
        val[y] = v;
        members.push_back((int)nj);
    }
    // The chain ends at ONE tensor, the last candidate's output if that works, else the one before, and so on: of the candidates it keeps
    // those that this tensor depends on (a table node on another branch of S stays a node of its own), and what lies between must be
    // the chain's alone -- an intermediate with a reader outside the set, or one that is a graph output, ends the set there
    for (size_t t = members.size(); t-- > 1;) {
        std::vector<char> in_set(g->nodes.size(), 0), needed(g->tensors.size(), 0);
        std::vector<int> set;
        needed[g->nodes[members[t]].out[0]] = 1;
        for (size_t k = t + 1; k-- > 0;) {
            const HNode& n = g->nodes[members[k]];
            if (!needed[n.out[0]]) continue;
            set.insert(set.begin(), members[k]);
            in_set[members[k]] = 1;
            for (int i : n.in) needed[i] = 1;
        }
        bool closed = set.size() >= 2 && set.front() == (int)ni;
        for (size_t k = 0; closed && k + 1 < set.size(); k++) {
            const int mid = g->nodes[set[k]].out[0];
            for (auto& o : g->outputs) closed = closed && o.tensor != mid;
            for (size_t nj = 0; closed && nj < g->nodes.size(); nj++)
                if (!in_set[nj]) for (int i : g->nodes[nj].in) closed = closed && i != mid;
        }
        if (!closed) continue;
        c->src = src; c->last = g->nodes[set.back()].out[0]; c->nodes = set;
        memcpy(c->table, val[c->last].data(), 256);
        return true;
    }
    return false;
}

int plan_bytemap_chain(tamd_graph* g, const ByteChain& c, std::vector<Step>* out)
{
    HTensor& x = g->tensors[c.src];
    HTensor& y = g->tensors[c.last];
    std::string node;
    for (int m : c.nodes) node += (node.empty() ? "" : "+") + g->nodes[m].name;
    if (x.dims != y.dims || x.dtype != y.dtype) { set_error("bytemap chain %s: output shape / type mismatch", node.c_str()); return -1; }
    std::vector<unsigned> table(64);
    memcpy(table.data(), c.table, 256);
    unsigned* dtable = nullptr;
    if (upload(g, table, &dtable)) return -1;
    if (lut_step(node, "bytemap chain", x, y, dtable, out)) return -1;
    if (g->fused_away.size() != g->tensors.size()) g->fused_away.assign(g->tensors.size(), 0);
    for (size_t k = 0; k + 1 < c.nodes.size(); k++) g->fused_away[g->nodes[c.nodes[k]].out[0]] = 1;      // never written
    return 0;
}

int gate_lut_producer(const tamd_graph* g, const HNode& e, int gated)
{
    if (gated < 0 || !tamd_pin_int("gate_lut", 1)) return -1;
    const int gate = e.in[1 - gated];
    if (g->tensors[gate].is_view || count_consumers(g, gate) != 1) return -1;      // (a graph output counts as a consumer)
    for (size_t pj = 0; pj < g->nodes.size(); pj++) {
        const HNode& p = g->nodes[pj];
        if (p.out.size() != 1 || p.out[0] != gate) continue;
        if (!is_lut_op(p.op) || p.in.size() != 1) return -1;
        const HTensor& pre = g->tensors[p.in[0]];
        if (!lut_op_on_device(p.op, pre.dtype) || pre.ttype == TAMD_TT_CONST || pre.is_view || pre.dims != g->tensors[gate].dims || pre.scales.size() != 1) return -1;
        return (int)pj;
    }
    return -1;
}

// The channel-gate Eltwise, int8 and uint8 graphs alike (graph_u8.hip calls this too): x is input `gated`, the gate the other one, and
// the launch computes x op gate whichever is listed first (eltwise_ref.c: run).  No view on any of the three tensors, as in plan_eltwise.
// lut_node >= 0 (gate_lut_producer; the planner has skipped that node): the launch reads that node's INPUT and maps it through the
// node's table itself, and the node's own output -- the gate tensor -- is never written.
int plan_chan_gate(tamd_graph* g, HNode& n, int gated, int lut_node, std::vector<Step>* out)
{
    HTensor& x = g->tensors[n.in[gated]];
    HTensor& gate = g->tensors[n.in[1 - gated]];
    HTensor& src = lut_node >= 0 ? g->tensors[g->nodes[lut_node].in[0]] : gate;      // the bytes the launch reads for the gate
    HTensor& y = g->tensors[n.out[0]];
    if (x.is_view || gate.is_view || src.is_view || y.is_view) { set_error("eltwise %s: views / broadcast not supported", n.name.c_str()); return -1; }
    if (y.dims != x.dims || y.dtype != x.dtype || gate.dtype != x.dtype || src.dtype != x.dtype) { set_error("eltwise %s: output shape / type mismatch", n.name.c_str()); return -1; }
    unsigned* dtable = nullptr;
    if (lut_node >= 0 && lut_table_upload(g, g->nodes[lut_node], &dtable)) return -1;
    const int type = n.p.elt.type, N = x.dims[0], C = x.dims[1], HW = x.dims[2] * x.dims[3];
    const std::string node = lut_node >= 0 ? g->nodes[lut_node].name + "+" + n.name : n.name;
    const double bytes = 2.0 * (double)x.elems() + (double)gate.elems();
    if (x.dtype == TAMD_DT_INT8) {
        if (x.nchw_raw || y.nchw_raw || src.nchw_raw || x.cs <= 0 || x.cs % 16 || x.cs != y.cs || src.cs != x.cs || x.c_off || y.c_off || src.c_off || x.c != C || C > x.cs
            || src.h * src.w != 1) {
            set_error("eltwise %s: the operands and the output are not NHWC tensors of one pixel stride", n.name.c_str());
            return -1;
        }
        ChanGateI8Args a{};
        a.x = (const int8_t*)x.dptr; a.gate = (const int8_t*)src.dptr; a.y = (int8_t*)y.dptr;
        a.N = N; a.HW = HW; a.C = C; a.cs = x.cs; a.type = type;
        a.sx = x.scales[0]; a.sg = gate.scales[0]; a.out_scale = y.scales[0]; a.table = dtable;
        a.iters = tamd_pin_int("gate_iters", 0);        // (tests: the walk of several pixels per lane on a small tensor)
        out->push_back(make_step(node, lut_node >= 0 ? "lut_chan_gate_i8" : "chan_gate_i8", 0, bytes, [a](hipStream_t s) { return launch_chan_gate_i8(a, s); },
                                 {access_of(x), access_of(src)}, {access_of(y)}, false));
    } else {
        if (!x.nchw_raw || !y.nchw_raw || !src.nchw_raw) { set_error("eltwise %s: the operands and the output are not dense NCHW tensors", n.name.c_str()); return -1; }
        ChanGateU8Args a{};
        a.x = (const uint8_t*)x.dptr; a.gate = (const uint8_t*)src.dptr; a.y = (uint8_t*)y.dptr;
        a.planes = (long)N * C; a.HW = HW; a.type = type;
        a.sx = x.scales[0]; a.sg = gate.scales[0]; a.out_scale = y.scales[0];
        a.zx = x.zps.empty() ? 0 : x.zps[0]; a.zg = gate.zps.empty() ? 0 : gate.zps[0]; a.out_zp = y.zps.empty() ? 0 : y.zps[0];
        a.table = dtable;
        out->push_back(make_step(node, lut_node >= 0 ? "lut_chan_gate_u8" : "chan_gate_u8", 0, bytes, [a](hipStream_t s) { return launch_chan_gate_u8(a, s); },
                                 {access_of(x), access_of(src)}, {access_of(y)}, false));
    }
    if (lut_node >= 0) {
        if (g->fused_away.size() != g->tensors.size()) g->fused_away.assign(g->tensors.size(), 0);
        g->fused_away[n.in[1 - gated]] = 1;              // the byte map's output only exists inside the launch
    }
    return 0;
}

const char* prelu_refusal_of(const tamd_graph* g, const HNode& n)
{
    if (n.in.size() != 2 || n.out.empty()) return "PReLU takes two inputs, the data and the slope";
    const HTensor& x = g->tensors[n.in[0]];
    const HTensor& sl = g->tensors[n.in[1]];
    const bool payload = sl.ttype == TAMD_TT_CONST && sl.dtype == TAMD_DT_FP16 && sl.data.size() == sl.elems() * 2;
    if (sl.ttype == TAMD_TT_CONST && sl.dtype == TAMD_DT_FP16 && !payload) return "PReLU: the slope's payload does not match its shape";
    return prelu_refusal(x.dtype, (int)n.in.size(), (int)x.dims.size(), x.dims.data(), x.ttype == TAMD_TT_CONST, x.scales.size(), g->tensors[n.out[0]].scales.size(),
                         sl.dtype, sl.ttype == TAMD_TT_CONST, sl.elems(), payload ? sl.data.data() : nullptr);
}

// PReLU, int8 and uint8 graphs alike (graph_u8.hip calls this too).  What the reference computes per channel is prepared HERE, once, on
// the host (prelu_tables.cc): int8 -- NHWC, 16 channels in a lane's 16 bytes -- gets the slopes widened to fp32 by tamd_prelu_slope and
// zero-padded to the pixel stride; uint8 -- dense NCHW, one slope per plane -- gets one 256-byte table per channel (one in all for a
// shared slope) from tamd_prelu_table.  Uploaded once; one launch of prelu.hip.  A concat view on either side is refused by name, as in
// plan_lut: neither planner makes a PReLU's tensors views (plan_concat_views: slice_capable; plan_u8: in_place)
int plan_prelu(tamd_graph* g, HNode& n, std::vector<Step>* out)
{
    const char* why = prelu_refusal_of(g, n);
    if (why) { set_error("prelu %s: %s", n.name.c_str(), why); return -1; }
    HTensor& x = g->tensors[n.in[0]];
    HTensor& y = g->tensors[n.out[0]];
    const HTensor& sl = g->tensors[n.in[1]];
    if (x.is_view || y.is_view) { set_error("prelu %s on a concat view is not supported", n.name.c_str()); return -1; }
    if (x.dims != y.dims || x.dtype != y.dtype) { set_error("prelu %s: output shape / type mismatch", n.name.c_str()); return -1; }
    const unsigned short* half = (const unsigned short*)sl.data.data();
    const size_t nslope = sl.elems();
    const int C = x.dims[1];
    if (x.dtype == TAMD_DT_INT8) {
        if (x.nchw_raw || y.nchw_raw || x.cs <= 0 || x.cs != y.cs || x.cs % 16 || x.c_off || y.c_off || x.c != C || C > x.cs) {
            set_error("prelu %s: input and output are not NHWC tensors of one pixel stride", n.name.c_str());
            return -1;
        }
        std::vector<float> slope((size_t)x.cs, 0.f);
        for (int c = 0; c < C; c++) slope[c] = tamd_prelu_slope(half[c]);
        float* dslope = nullptr;
        if (upload(g, slope, &dslope)) return -1;
        PreluI8Args a{};
        a.x = (const int8_t*)x.dptr; a.y = (int8_t*)y.dptr; a.count = (size_t)x.n * x.h * x.w * x.cs; a.C = C; a.cs = x.cs;
        a.slope = dslope; a.in_scale = x.scales[0]; a.out_scale = y.scales[0];
        out->push_back(make_step(n.name, "prelu_i8", 0, 2.0 * (double)x.elems(), [a](hipStream_t s) { return launch_prelu_i8(a, s); }, {access_of(x)}, {access_of(y)}, false));
    } else {
        if (!x.nchw_raw || !y.nchw_raw) { set_error("prelu %s: input and output are not dense NCHW tensors", n.name.c_str()); return -1; }
        const size_t ntab = nslope == 1 ? 1 : (size_t)C;
        std::vector<unsigned> tables(ntab * 64);
        for (size_t c = 0; c < ntab; c++)
            if (tamd_prelu_table(x.dtype, half[c], x.scales[0], x.zps.empty() ? 0 : x.zps[0], y.scales[0], y.zps.empty() ? 0 : y.zps[0], (unsigned char*)(tables.data() + c * 64))) {
                set_error("prelu %s: PReLU: a slope widens to inf or NaN", n.name.c_str());
                return -1;
            }
        unsigned* dtables = nullptr;
        if (upload(g, tables, &dtables)) return -1;
        PreluU8Args a{};
        a.x = (const uint8_t*)x.dptr; a.y = (uint8_t*)y.dptr; a.planes = (long)x.dims[0] * C; a.C = C; a.HW = x.dims[2] * x.dims[3];
        a.tables = dtables; a.shared = nslope == 1 ? 1 : 0;
        out->push_back(make_step(n.name, "prelu_u8", 0, 2.0 * (double)x.elems(), [a](hipStream_t s) { return launch_prelu_u8(a, s); }, {access_of(x)}, {access_of(y)}, false));
    }
    return 0;
}

// Nearest Interp, int8 and uint8 graphs alike (graph_u8.hip calls this too).  Everything the reference computes for the node is done
// HERE, once: the scales and the output size (interp_resolve), the source row of every output row and the source column of every
// output column (tamd_interp_indices), the byte map between the two tensors' quantisation parameters (tamd_interp_table) -- uploaded,
// and one launch of interp.hip looks them up.  int8: NHWC with padded channel stride, reads a channel slice, writes one (a concat
// view), like plan_upsample.  uint8: dense NCHW; writes a channel range of a concat buffer (out_img / out_c0), like plan_map_u8.
// With `crop` (uint8; crop_interp_producer) the launch writes the CROP's output: the Crop copies raw bytes, so it only shifts and cuts the
// two index vectors by its box; the byte map stays the Interp's own, between x and the Interp's own output tensor
int plan_interp(tamd_graph* g, HNode& n, std::vector<Step>* out, const HNode* crop)
{
    HTensor& x = g->tensors[n.in[0]];
    HTensor& mid = g->tensors[n.out[0]];
    HTensor& y = crop ? g->tensors[crop->out[0]] : mid;
    const std::string name = crop ? n.name + "+" + crop->name : n.name;
    InterpGeom geom;
    std::vector<int> iy, ix;
    const char* why = interp_refusal(&n.p.interp, x.dtype, (int)x.dims.size(), x.dims.data(), x.ttype == TAMD_TT_CONST, x.scales.size(), mid.scales.size(), &geom, &iy, &ix);
    if (why) { set_error("interp %s: %s", name.c_str(), why); return -1; }
    if (mid.dtype != x.dtype || mid.n != x.n || mid.c != x.c || mid.h != geom.out_h || mid.w != geom.out_w) { set_error("interp %s: output shape / type mismatch", name.c_str()); return -1; }
    if (crop) {
        CropGeom cg;
        why = crop_refusal_of(g, *crop, true, &cg);
        if (why) { set_error("interp %s: %s", name.c_str(), why); return -1; }
        if (x.dtype != TAMD_DT_UINT8 || crop->in[0] != n.out[0] || cg.start[1] != 0 || cg.out_dims[1] != x.c || y.is_view || y.dtype != x.dtype) {
            set_error("interp %s: this Crop does not run inside the Interp's launch", name.c_str());
            return -1;
        }
        iy = std::vector<int>(iy.begin() + cg.start[2], iy.begin() + cg.start[2] + cg.out_dims[2]);      // (inside the vectors: crop_refusal's box check)
        ix = std::vector<int>(ix.begin() + cg.start[3], ix.begin() + cg.start[3] + cg.out_dims[3]);
    }
    std::vector<unsigned> table(64);
    if (tamd_interp_table(x.dtype, x.scales[0], x.zps.empty() ? 0 : x.zps[0], mid.scales[0], mid.zps.empty() ? 0 : mid.zps[0], (unsigned char*)table.data())) {
        set_error("interp %s: not supported on the device for data type %d", name.c_str(), x.dtype);
        return -1;
    }
    int* diy = nullptr; int* dix = nullptr; unsigned* dtable = nullptr;
    if (upload(g, iy, &diy) || upload(g, ix, &dix) || upload(g, table, &dtable)) return -1;
    const double bytes = 2.0 * (double)y.elems();
    if (x.dtype == TAMD_DT_INT8) {
        // whole 16-byte vectors: up to the padding channels of its own buffers, never into a neighbour's slice (a view has c % 16 == 0)
        const int cv = rup(x.c, 16);
        if (x.nchw_raw || y.nchw_raw || x.cs <= 0 || y.cs <= 0 || x.cs % 16 || y.cs % 16 || x.c_off % 16 || y.c_off % 16 || x.c_off + cv > x.cs || y.c_off + cv > y.cs) {
            set_error("interp %s: channel slice not 16-byte aligned", n.name.c_str());
            return -1;
        }
        InterpI8Args a{};
        a.x = (const int8_t*)x.dptr + x.c_off; a.y = (int8_t*)y.dptr;
        a.N = x.n; a.H = x.h; a.W = x.w; a.C = x.c; a.cs_in = x.cs;
        a.OH = y.h; a.OW = y.w; a.ldc = y.cs; a.c_off = y.c_off;
        a.iy = diy; a.ix = dix; a.table = dtable;
        out->push_back(make_step(n.name, "interp_nearest_i8", 0, bytes, [a](hipStream_t s) { return launch_interp_i8(a, s); }, {access_of(x)}, {access_of(y)}, false));
    } else {
        if (x.is_view) { set_error("interp %s reads a concat view: not supported in a uint8 graph", n.name.c_str()); return -1; }
        InterpU8Args a{};
        a.x = (const uint8_t*)x.dptr; a.y = (uint8_t*)y.dptr;
        a.N = x.n; a.C = x.c; a.H = x.h; a.W = x.w; a.OH = y.h; a.OW = y.w;
        a.out_img = nchw_out_img(y); a.out_c0 = y.c_off;
        a.iy = diy; a.ix = dix; a.table = dtable;
        a.identity = 1;
        for (int b = 0; b < 256; b++) a.identity &= ((const unsigned char*)table.data())[b] == b;
        out->push_back(make_step(name, "interp_nearest_u8", 0, bytes, [a](hipStream_t s) { return launch_interp_u8(a, s); }, {access_of(x)}, {access_of(y)}, false));
    }
    if (crop) {
        if (g->fused_away.size() != g->tensors.size()) g->fused_away.assign(g->tensors.size(), 0);
        g->fused_away[n.out[0]] = 1;                         // the up-sampled map only exists inside the launch
    }
    return 0;
}

// ---- Split, ShuffleChannel and Concat + ShuffleChannel of an int8 graph: chan_map_i8 (chanmap.hip).  ONE launch writes tensor y from
// up to kChanMapMaxSrc source tensors; sel[o] = {source, channel of that source} for output channel o.  The table is built and checked
// here -- every entry inside its source's pixel -- and uploaded once; sources and output are addressed where they lie (whole tensors,
// concat views, Split views), the output's padding lanes are written as zero
static int plan_chan_map_i8(tamd_graph* g, const std::string& node, const std::vector<const HTensor*>& srcs, const std::vector<std::pair<int, int>>& sel, HTensor& y,
                            bool through_concat, Step* out)
{
    if (srcs.empty() || srcs.size() > (size_t)kChanMapMaxSrc || sel.size() != (size_t)y.c) { set_error("%s: at most %d sources, one entry per output channel", node.c_str(), kChanMapMaxSrc); return -1; }
    const int cv = rup(y.c, 16);
    if (y.dtype != TAMD_DT_INT8 || y.nchw_raw || y.cs <= 0 || y.cs % 16 || y.c_off % 16 || y.c_off + cv > y.cs) { set_error("%s: output channel slice not 16-byte aligned", node.c_str()); return -1; }
    ChanMapI8Args a{};
    a.nsrc = (int)srcs.size();
    for (size_t i = 0; i < srcs.size(); i++) {
        const HTensor& x = *srcs[i];
        if (x.dtype != TAMD_DT_INT8 || x.nchw_raw || x.cs <= 0 || !x.dptr || x.n != y.n || x.h != y.h || x.w != y.w || x.c_off + x.c > x.cs) {
            set_error("%s: source %s is not an NHWC int8 tensor of the output's map", node.c_str(), x.name.c_str());
            return -1;
        }
        a.src[i] = ChanMapI8Src{(const int8_t*)x.dptr, x.cs};
    }
    std::vector<unsigned> table((size_t)cv, kChanMapZero);
    for (int o = 0; o < y.c; o++) {
        const int s = sel[o].first, c = sel[o].second;
        if (s < 0 || s >= a.nsrc || c < 0 || c >= srcs[s]->c) { set_error("%s: a source channel leaves its tensor", node.c_str()); return -1; }
        table[o] = (unsigned)s << 28 | (unsigned)(srcs[s]->c_off + c);
    }
    unsigned* dtable = nullptr;
    if (upload(g, table, &dtable)) return -1;
    a.y = (int8_t*)y.dptr; a.pixels = (long)y.n * y.h * y.w; a.C = y.c; a.ldc = y.cs; a.c_off = y.c_off; a.table = dtable;
    a.fix128 = through_concat ? 1 : 0;                      // a Concat of several inputs: -128 -> 127 (chanmap.hip)
    std::vector<Access> reads;
    for (const HTensor* x : srcs) reads.push_back(access_of(*x));
    *out = make_step(node, "chan_map_i8", 0, 2.0 * (double)y.elems(), [a](hipStream_t s) { return launch_chan_map_i8(a, s); }, reads, {access_of(y)}, false);
    return 0;
}

// group 2 over two halves of equal width `half` -- channels [a0, a0 + half) of tensor a and [b0, b0 + half) of tensor b -- as the
// interleave launch (chanmap.hip: chan_map_i8_g2) where both halves can be read in aligned 8-byte words inside their own pixels.
// 1: *out is that launch, 0: the table form has to do it.  TAMD_PIN=chan_map_g2=0: always the table form (A/B runs, and the test that
// demands the same bytes of both)
static int try_chan_map_g2(tamd_graph* g, const std::string& node, const HTensor& a, int a0, const HTensor& b, int b0, int half, HTensor& y, bool through_concat,
                           Step* out)
{
    if (!tamd_pin_int("chan_map_g2", 1) || y.c != 2 * half || half < 1) return 0;
    if (y.dtype != TAMD_DT_INT8 || y.nchw_raw || y.cs <= 0 || y.cs % 16 || y.c_off % 16 || y.c_off + rup(y.c, 16) > y.cs) return 0;
    const int ra = a.c_off + a0, rb = b.c_off + b0, rv = rup(half, 8);
    for (const HTensor* x : {&a, &b})
        if (x->dtype != TAMD_DT_INT8 || x->nchw_raw || x->cs <= 0 || x->cs % 8 || !x->dptr || x->n != y.n || x->h != y.h || x->w != y.w) return 0;
    if (a0 < 0 || b0 < 0 || a0 + half > a.c || b0 + half > b.c || ra % 8 || rb % 8 || ra + rv > a.cs || rb + rv > b.cs) return 0;
    ChanMapG2Args k{};
    k.a = (const int8_t*)a.dptr + ra; k.b = (const int8_t*)b.dptr + rb; k.cs_a = a.cs; k.cs_b = b.cs;
    k.y = (int8_t*)y.dptr; k.pixels = (long)y.n * y.h * y.w; k.half = half; k.ldc = y.cs; k.c_off = y.c_off; k.fix128 = through_concat ? 1 : 0;
    *out = make_step(node, "chan_map_i8_g2", 0, 2.0 * (double)y.elems(), [k](hipStream_t s) { return launch_chan_map_g2(k, s); }, {access_of(a), access_of(b)}, {access_of(y)}, false);
    return 1;
}

// split_ref.c:109-135: output i is channels [first_i, first_i + sizes[i]) of the input, bytes as they are.  An output that
// plan_split_views made a view of the input has no launch; every other one is one chan_map_i8 launch with one source
int plan_split(tamd_graph* g, I8Layout& L, HNode& n, std::vector<Step>* out)
{
    HTensor& x = g->tensors[n.in[0]];
    std::vector<size_t> oq;
    for (int o : n.out) oq.push_back(g->tensors[o].scales.size());
    const char* why = split_refusal(&n.p.split, x.dtype, (int)x.dims.size(), x.dims.data(), x.ttype == TAMD_TT_CONST, x.scales.size(), (int)n.out.size(), oq.data());
    if (why) { set_error("split %s: %s", n.name.c_str(), why); return -1; }
    int first = 0;
    for (size_t i = 0; i < n.out.size(); i++) {
        HTensor& y = g->tensors[n.out[i]];
        if (y.dtype != x.dtype || y.dims.size() != 4 || y.n != x.n || y.c != n.p.split.sizes[i] || y.h != x.h || y.w != x.w) { set_error("split %s: output shape / type mismatch", n.name.c_str()); return -1; }
        if (!(L.view_of[n.out[i]] == n.in[0] && L.view_off[n.out[i]] == first)) {
            std::vector<std::pair<int, int>> sel((size_t)y.c);
            for (int c = 0; c < y.c; c++) sel[c] = {0, first + c};
            Step st;
            if (plan_chan_map_i8(g, n.name, {&x}, sel, y, false, &st)) return -1;
            out->push_back(st);
        }
        first += y.c;
    }
    return 0;
}

// shuffle_channel_ref.c: output channel group * j + i takes input channel (C / group) * i + j (tamd_shuffle_sources), bytes as they are
static int shuffle_sources(const HNode& n, const HTensor& x, const HTensor& y, std::vector<int>* src)
{
    const char* why = shuffle_refusal(&n.p.shuffle, x.dtype, (int)x.dims.size(), x.dims.data(), x.ttype == TAMD_TT_CONST, x.scales.size(), y.scales.size());
    if (why) { set_error("shufflechannel %s: %s", n.name.c_str(), why); return -1; }
    if (y.dtype != x.dtype || y.dims != x.dims) { set_error("shufflechannel %s: output shape / type mismatch", n.name.c_str()); return -1; }
    src->resize((size_t)x.dims[1]);
    if (tamd_shuffle_sources(x.dims[1], n.p.shuffle.group, src->data())) { set_error("shufflechannel %s: the group count must divide the channels", n.name.c_str()); return -1; }
    return 0;
}

int plan_shuffle(tamd_graph* g, HNode& n, std::vector<Step>* out)
{
    HTensor& x = g->tensors[n.in[0]];
    HTensor& y = g->tensors[n.out[0]];
    std::vector<int> src;
    if (shuffle_sources(n, x, y, &src)) return -1;
    std::vector<std::pair<int, int>> sel((size_t)y.c);
    for (int o = 0; o < y.c; o++) sel[o] = {0, src[o]};
    Step st;
    if (!(n.p.shuffle.group == 2 && try_chan_map_g2(g, n.name, x, 0, x, x.c / 2, x.c / 2, y, false, &st)) && plan_chan_map_i8(g, n.name, {&x}, sel, y, false, &st)) return -1;
    out->push_back(st);
    return 0;
}

// The pair match_cat_shuffle found, planned at the CONCAT's position: the launch reads the Concat's inputs and writes the
// ShuffleChannel's output.  That output's lifetime starts at the earliest producer within two hops above the ShuffleChannel
// (plan_buffers: shuffle <- concat <- the inputs' producers), so it never shares memory with an input; planned at the
// ShuffleChannel's position an input's buffer could have been reused before it is read.  plan_i8 checks it (step_writes_what_it_reads)
int plan_cat_shuffle(tamd_graph* g, I8Layout& L, HNode& cat, size_t sj, std::vector<Step>* out)
{
    HNode& sh = g->nodes[sj];
    HTensor& mid = g->tensors[cat.out[0]];
    HTensor& y = g->tensors[sh.out[0]];
    std::vector<int> src;
    if (shuffle_sources(sh, mid, y, &src)) return -1;
    std::vector<const HTensor*> srcs;
    std::vector<int> begin;                                  // first Concat channel of every input
    int total = 0;
    for (int i : cat.in) { srcs.push_back(&g->tensors[i]); begin.push_back(total); total += g->tensors[i].c; }
    if (total != mid.c) { set_error("concat %s: the inputs do not add up to the output", cat.name.c_str()); return -1; }
    std::vector<std::pair<int, int>> sel((size_t)y.c);
    for (int o = 0; o < y.c; o++) {
        int k = (int)cat.in.size() - 1;
        while (k > 0 && begin[k] > src[o]) k--;
        sel[o] = {k, src[o] - begin[k]};
    }
    Step st;
    const bool two_halves = sh.p.shuffle.group == 2 && srcs.size() == 2 && srcs[0]->c == srcs[1]->c;
    if (!(two_halves && try_chan_map_g2(g, cat.name + "+" + sh.name, *srcs[0], 0, *srcs[1], 0, srcs[0]->c, y, true, &st))
        && plan_chan_map_i8(g, cat.name + "+" + sh.name, srcs, sel, y, cat.in.size() > 1, &st))
        return -1;
    out->push_back(st);
    L.fused[sj] = 1;
    g->fused_away[cat.out[0]] = 1;
    return 0;
}

// ---- Slice of a uint8 graph (slice.hip).  Everything the reference decides for the node is decided by slice_refusal (node_rules.h):
// the form, the resolved box, the raw copy, the byte map
const char* slice_refusal_of(const tamd_graph* g, const HNode& n, bool check_out, SliceGeom* geom, unsigned char* table)
{
    if (n.in.empty() || n.out.empty()) return "Slice takes one input";
    const HTensor& x = g->tensors[n.in[0]];
    const HTensor& y = g->tensors[n.out[0]];
    return slice_refusal(&n.p.slice, x.dtype, (int)x.dims.size(), x.dims.data(), x.ttype == TAMD_TT_CONST, x.scales.size(), x.scales.empty() ? 0.f : x.scales[0],
                         x.zps.empty() ? 0 : x.zps[0], (int)n.out.size(), y.scales.size(), y.scales.empty() ? 0.f : y.scales[0], y.zps.empty() ? 0 : y.zps[0],
                         (int)y.dims.size(), check_out ? y.dims.data() : nullptr, geom, table);
}

int slice_chain_next(const tamd_graph* g, size_t ni)
{
    const HNode& n = g->nodes[ni];
    if (!tamd_pin_int("slice_chain", 1) || n.op != TAMD_OP_SLICE || n.out.size() != 1) return -1;
    const int mid = n.out[0];
    if (g->tensors[mid].is_view || count_consumers(g, mid) != 1) return -1;      // (a graph output counts as a consumer)
    for (size_t nj = ni + 1; nj < g->nodes.size(); nj++) {
        const HNode& m = g->nodes[nj];
        if (m.in.empty() || m.in[0] != mid) continue;
        if (m.op != TAMD_OP_SLICE || m.in.size() != 1 || slice_refusal_of(g, n, true, nullptr, nullptr) || slice_refusal_of(g, m, true, nullptr, nullptr)) return -1;
        return (int)nj;
    }
    return -1;
}

// One slice_u8 launch for the node, or for the node and the Slice `next` that alone reads it: output position o of the second is
// position start2 + o * step2 of the first's output, which is position start1 + (..) * step1 of x -- per axis start1 + start2 * step1
// and step1 * step2 -- and the byte map is table2[table1[b]], exact because both are byte maps (a raw-copy member is the identity).
// A concat view on either side is refused by name: plan_u8 makes neither tensor one (in_place), which the error guards
int plan_slice_u8(tamd_graph* g, HNode& n, int next, std::vector<Step>* out)
{
    HNode* m = next >= 0 ? &g->nodes[next] : nullptr;
    HTensor& x = g->tensors[n.in[0]];
    HTensor& y = g->tensors[(m ? *m : n).out[0]];
    const std::string node = m ? n.name + "+" + m->name : n.name;
    SliceGeom sg[2];
    unsigned char map[2][256];
    const char* why = slice_refusal_of(g, n, true, &sg[0], map[0]);
    if (!why && m) why = slice_refusal_of(g, *m, true, &sg[1], map[1]);
    if (why) { set_error("slice %s: %s", node.c_str(), why); return -1; }
    if (x.is_view || y.is_view || !x.nchw_raw || !y.nchw_raw) { set_error("slice %s on a concat view is not supported in a uint8 graph", node.c_str()); return -1; }
    const SliceGeom& last = sg[m ? 1 : 0];
    if (y.dtype != x.dtype || y.dims.size() != 4 || x.dims.size() != 4) { set_error("slice %s: output shape / type mismatch", node.c_str()); return -1; }
    SliceU8Args a{};
    for (int i = 0; i < 4; i++) {
        a.in_dims[i] = x.dims[i]; a.out_dims[i] = last.out_dims[i]; a.start[i] = 0; a.step[i] = 1;
        if (y.dims[i] != last.out_dims[i]) { set_error("slice %s: output shape / type mismatch", node.c_str()); return -1; }
    }
    a.start[sg[0].axis] = sg[0].start; a.step[sg[0].axis] = sg[0].step;
    if (m) {
        a.start[sg[1].axis] += sg[1].start * a.step[sg[1].axis];
        a.step[sg[1].axis] *= sg[1].step;
    }
    std::vector<unsigned> table(64, 0u);
    unsigned char* tb = (unsigned char*)table.data();
    a.identity = 1;
    for (int b = 0; b < 256; b++) {
        tb[b] = m ? map[1][map[0][b]] : map[0][b];
        a.identity &= tb[b] == b;
    }
    unsigned* dtable = nullptr;
    if (upload(g, table, &dtable)) return -1;
    a.x = (const uint8_t*)x.dptr; a.y = (uint8_t*)y.dptr; a.table = dtable;
    a.out_img = nchw_out_img(y); a.out_c0 = y.c_off;
    a.w2 = tamd_pin_int("slice_w2", 1) ? 1 : 0;             // 0: the byte-by-byte path at W step 2 too (A/B runs)
    out->push_back(make_step(node, "slice_u8", 0, 2.0 * (double)y.elems(), [a](hipStream_t s) { return launch_slice_u8(a, s); }, {access_of(x)}, {access_of(y)}, false));
    if (m) {
        if (g->fused_away.size() != g->tensors.size()) g->fused_away.assign(g->tensors.size(), 0);
        g->fused_away[n.out[0]] = 1;                        // the tensor between the two only exists inside the launch
    }
    return 0;
}

// ---- Transpose of a quantised graph (transpose.hip), both types.  Everything the reference decides for the node is decided by
// transpose_refusal (node_rules.h): the ranks, the order vector, the output's dims, the byte map
const char* transpose_refusal_of(const tamd_graph* g, const HNode& n, bool check_out, TransposeGeom* geom, unsigned char* table)
{
    if (n.in.empty() || n.out.empty()) return "Transpose takes one input";
    const HTensor& x = g->tensors[n.in[0]];
    const HTensor& y = g->tensors[n.out[0]];
    return transpose_refusal(&n.p.transpose, x.dtype, (int)x.dims.size(), x.dims.data(), x.ttype == TAMD_TT_CONST, x.scales.size(), x.scales.empty() ? 0.f : x.scales[0],
                             x.zps.empty() ? 0 : x.zps[0], y.scales.size(), y.scales.empty() ? 0.f : y.scales[0], y.zps.empty() ? 0 : y.zps[0], (int)y.dims.size(),
                             check_out ? y.dims.data() : nullptr, geom, table);
}

// The strides (bytes per step of every axis) under which `dims` index the convolution-stack NHWC buffer that s lives in -- element
// (n, c, p) of s lies at n * H * W * cs + p * cs + c behind its first channel --, where every axis of dims factors exactly ONE of the
// three index ranges N, C, H * W of s: (N, 255, H, W) seen as (N, 3, 85, H, W) does, C splits into 3 x 85, and so does s's own shape.
// false: an axis mixes two ranges (C with H, say), and no strides exist.  A size-1 axis factors anything (stride 0)
bool nhwc_view_strides(const HTensor& s, const std::vector<int>& dims, long* strides)
{
    size_t want = 1;
    for (int d : dims) want *= (size_t)d;
    if (dims.size() > 8 || want != (size_t)s.n * s.c * s.h * s.w) return false;
    const long range[3] = {s.n, s.c, (long)s.h * s.w}, unit[3] = {(long)s.h * s.w * s.cs, 1, s.cs};
    int gi = 0;
    long acc = 1;
    for (size_t d = 0; d < dims.size(); d++) {
        const long e = dims[d];
        if (e == 1) { strides[d] = 0; continue; }
        while (gi < 3 && acc == range[gi]) { gi++; acc = 1; }          // the range is used up: the next one
        if (gi >= 3 || range[gi] % (acc * e) != 0) return false;
        acc *= e;
        strides[d] = range[gi] / acc * unit[gi];
    }
    return true;
}

// One launch.  view_src >= 0 (int8 graphs): the node reads tensor view_src, a convolution-stack tensor, THROUGH the Reshape in front of
// it (nhwc_view_strides; plan_dense matched it and the Reshape has no launch); else its own input -- a dense tensor, or in an int8
// graph a convolution-stack tensor read where it lies, a concat or Split view included.  The form: TAMD_PIN=transpose_form where that
// form is legal for the geometry, else transpose_default_form
int plan_transpose(tamd_graph* g, HNode& n, int view_src, std::vector<Step>* out)
{
    HTensor& x = g->tensors[n.in[0]];
    HTensor& y = g->tensors[n.out[0]];
    TransposeGeom tg;
    std::vector<unsigned> table(64, 0u);
    unsigned char* tb = (unsigned char*)table.data();
    const char* why = transpose_refusal_of(g, n, true, &tg, tb);
    if (why) { set_error("transpose %s: %s", n.name.c_str(), why); return -1; }
    if (y.is_view || !(y.nchw_raw || y.cs <= 0) || y.dtype != x.dtype) { set_error("transpose %s: the output must be a dense tensor of the input's type", n.name.c_str()); return -1; }
    const HTensor& s = view_src >= 0 ? g->tensors[view_src] : x;
    std::string node = n.name;
    TransposeArgs a{};
    if (s.nchw_raw || s.cs <= 0) {                               // dense: the canonical geometry as transpose_refusal resolved it
        if (view_src >= 0 || s.is_view) { set_error("transpose %s on a concat view is not supported in a uint8 graph", n.name.c_str()); return -1; }
        a.x = (const uint8_t*)s.dptr; a.src_bytes = (unsigned)s.elems();
    } else {                                                     // a convolution-stack buffer: the same thing with other strides
        long strides[8];
        if (!nhwc_view_strides(s, x.dims, strides)) { set_error("transpose %s: the input's shape mixes the channel and the spatial axes of %s", n.name.c_str(), s.name.c_str()); return -1; }
        const size_t bytes = (size_t)s.n * s.h * s.w * s.cs;
        if (bytes > 0x7fffffffu) { set_error("transpose %s: the source buffer has more than 2^31 bytes", n.name.c_str()); return -1; }
        transpose_canon((int)x.dims.size(), x.dims.data(), strides, n.p.transpose.order, &tg);
        a.x = (const uint8_t*)s.dptr + s.c_off; a.src_bytes = (unsigned)(bytes - (size_t)s.c_off);
        if (view_src >= 0) {
            for (auto& m : g->nodes) if (!m.out.empty() && m.out[0] == n.in[0]) node = m.name + "+" + n.name;
            if (g->fused_away.size() != g->tensors.size()) g->fused_away.assign(g->tensors.size(), 0);
            g->fused_away[n.in[0]] = 1;                          // the reshaped tensor is never written
        }
    }
    a.y = (uint8_t*)y.dptr; a.nd = tg.nd; a.unit = tg.unit; a.total = (unsigned)y.elems();
    for (int d = 0; d < 6; d++) { a.extent[d] = tg.extent[d]; a.stride[d] = (int)tg.stride[d]; }
    a.identity = 1;
    for (int b = 0; b < 256; b++) a.identity &= tb[b] == b;
    if (!a.identity) {
        unsigned* dtable = nullptr;
        if (upload(g, table, &dtable)) return -1;
        a.table = dtable;
    }
    const int pin = tamd_pin_int("transpose_form", -1);
    a.form = pin >= 0 && transpose_form_legal(a, pin) ? pin : transpose_default_form(a);
    out->push_back(make_step(node, transpose_kernel_name(a.form), 0, 2.0 * (double)y.elems(), [a](hipStream_t st) { return launch_transpose(a, st); }, {access_of(s)},
                             {access_of(y)}, false));
    return 0;
}

// ---- Crop of a uint8 graph.  Everything the reference decides for the node is decided by crop_refusal (node_rules.h): the form and
// the box.  The output is a box of the data's RAW bytes (crop_ref.c:147-253 reads no quantisation parameter), so the node alone is the
// identity form of slice_u8; behind a nearest Interp it is a shift of that launch's index vectors (plan_interp); and in front of a
// same-shape Eltwise the three nodes are one topdown_u8 launch.  Input 1 gives its shape and nothing else: no launch reads it
const char* crop_refusal_of(const tamd_graph* g, const HNode& n, bool check_out, CropGeom* geom)
{
    if (n.in.size() != 2 || n.out.empty()) return "Crop takes two inputs: the data and the tensor whose shape it takes";
    const HTensor& x = g->tensors[n.in[0]];
    const HTensor& like = g->tensors[n.in[1]];
    const HTensor& y = g->tensors[n.out[0]];
    return crop_refusal(&n.p.crop, x.dtype, (int)n.in.size(), (int)x.dims.size(), x.dims.data(), x.ttype == TAMD_TT_CONST, x.scales.size(), (int)like.dims.size(),
                        like.dims.data(), y.scales.size(), (int)y.dims.size(), check_out ? y.dims.data() : nullptr, geom);
}

int crop_interp_producer(const tamd_graph* g, size_t ci)
{
    const HNode& c = g->nodes[ci];
    CropGeom cg;
    if (!tamd_pin_int("crop_chain", 1) || c.op != TAMD_OP_CROP || crop_refusal_of(g, c, true, &cg)) return -1;
    const int mid = c.in[0];
    const HTensor& t = g->tensors[mid];
    if (t.is_view || count_consumers(g, mid) != 1) return -1;      // (a graph output counts as a consumer)
    if (cg.start[1] != 0 || cg.out_dims[1] != t.dims[1] || g->tensors[c.out[0]].is_view) return -1;      // the box cuts no channels
    for (size_t pj = 0; pj < ci; pj++) {
        const HNode& p = g->nodes[pj];
        if (p.out.size() != 1 || p.out[0] != mid) continue;
        if (p.op != TAMD_OP_INTERP || p.in.empty()) return -1;
        const HTensor& x = g->tensors[p.in[0]];
        InterpGeom geom;
        std::vector<int> iy, ix;
        if (x.is_view || interp_refusal(&p.p.interp, x.dtype, (int)x.dims.size(), x.dims.data(), x.ttype == TAMD_TT_CONST, x.scales.size(), t.scales.size(), &geom, &iy, &ix)) return -1;
        if (t.dims.size() != 4 || t.dims[0] != x.dims[0] || t.dims[1] != x.dims[1] || t.dims[2] != geom.out_h || t.dims[3] != geom.out_w) return -1;
        return (int)pj;
    }
    return -1;
}

int crop_topdown_next(const tamd_graph* g, size_t ci)
{
    const HNode& c = g->nodes[ci];
    if (!tamd_pin_int("topdown", 0) || crop_interp_producer(g, ci) < 0) return -1;      // opt-in: it did not beat the chain + eltwise_u8 (profiles/crop_topdown.txt)
    const int cut = c.out[0];
    if (count_consumers(g, cut) != 1) return -1;                   // (a graph output counts as a consumer)
    for (size_t ej = ci + 1; ej < g->nodes.size(); ej++) {
        const HNode& e = g->nodes[ej];
        bool reads = false;
        for (int i : e.in) reads = reads || i == cut;
        if (!reads) continue;
        int gated = -1;
        if (e.op != TAMD_OP_ELTWISE || e.out.size() != 1 || eltwise_refusal_of(g, e, &gated) || gated != kEltSame) return -1;
        const HTensor& lat = g->tensors[e.in[e.in[0] == cut ? 1 : 0]];
        const HTensor& y = g->tensors[e.out[0]];
        if (lat.is_view || y.is_view || lat.dims != g->tensors[cut].dims || y.dims != lat.dims || lat.scales.size() != 1 || y.scales.size() != 1) return -1;
        return (int)ej;
    }
    return -1;
}

int plan_crop_u8(tamd_graph* g, HNode& n, std::vector<Step>* out)
{
    CropGeom cg;
    const char* why = crop_refusal_of(g, n, true, &cg);
    if (why) { set_error("crop %s: %s", n.name.c_str(), why); return -1; }
    HTensor& x = g->tensors[n.in[0]];
    HTensor& y = g->tensors[n.out[0]];
    if (x.is_view || y.is_view || !x.nchw_raw || !y.nchw_raw) { set_error("crop %s on a concat view is not supported in a uint8 graph", n.name.c_str()); return -1; }
    if (y.dtype != x.dtype) { set_error("crop %s: output shape / type mismatch", n.name.c_str()); return -1; }
    SliceU8Args a{};
    for (int i = 0; i < 4; i++) { a.in_dims[i] = x.dims[i]; a.out_dims[i] = cg.out_dims[i]; a.start[i] = cg.start[i]; a.step[i] = 1; }
    a.x = (const uint8_t*)x.dptr; a.y = (uint8_t*)y.dptr; a.table = nullptr;
    a.identity = 1;                                          // raw bytes, whatever the two tensors' parameters
    a.out_img = nchw_out_img(y); a.out_c0 = y.c_off;
    a.w2 = 0;
    out->push_back(make_step(n.name, "slice_u8", 0, 2.0 * (double)y.elems(), [a](hipStream_t s) { return launch_slice_u8(a, s); }, {access_of(x)}, {access_of(y)}, false));
    return 0;
}

// ---- DepthToSpace of a quantised graph (d2s.hip), both types.  Everything the reference decides for the node is decided by
// depthtospace_refusal (node_rules.h): the block size, the channel count, the output's dims.  The output is a shuffle of the input's RAW
// bytes (depthtospace_ref.c reads no quantisation parameter, -128 stays -128), so no table is made
const char* depthtospace_refusal_of(const tamd_graph* g, const HNode& n, bool check_out, DepthToSpaceGeom* geom)
{
    if (n.in.size() != 1 || n.out.empty()) return "DepthToSpace takes one input";
    const HTensor& x = g->tensors[n.in[0]];
    const HTensor& y = g->tensors[n.out[0]];
    return depthtospace_refusal(&n.p.d2s, x.dtype, (int)x.dims.size(), x.dims.data(), x.ttype == TAMD_TT_CONST, x.scales.size(), y.scales.size(), (int)y.dims.size(),
                                check_out ? y.dims.data() : nullptr, geom);
}

// One launch.  uint8 (NCHW): d2s_u8; the output may be a channel range of a Concat's buffer (out_img / out_c0).  int8 (NHWC): d2s_i8;
// the input is read where it lies (a concat or Split view: another base and pixel stride), the output may be a concat view.
// Block size 1 is a copy in the reference: the uint8 graph runs it as slice_u8 over the whole tensor in its identity form; d2s_i8 with
// r == 1 IS a 16-byte copy per lane.  Form 0 (TAMD_PIN=d2s_form=0, and the default below kD2sNewFormFromBytes output bytes: profiles/d2s.txt)
// is the baseline the new kernels are measured against -- the canonical gather of transpose.hip over the six-axis view with the identity
// map (raw bytes: no table, no clamp) -- where the output is ONE dense run, which is all that kernel writes: a uint8 output that is no
// slice of a Concat's buffer (or one of a single image), an int8 output without padding channels that is no concat view.  Elsewhere
// form 0 is not legal and the new kernel runs whatever the size or the pin
int plan_depthtospace(tamd_graph* g, HNode& n, bool fix128, std::vector<Step>* out)
{
    DepthToSpaceGeom dg;
    const char* why = depthtospace_refusal_of(g, n, true, &dg);
    if (why) { set_error("depthtospace %s: %s", n.name.c_str(), why); return -1; }
    HTensor& x = g->tensors[n.in[0]];
    HTensor& y = g->tensors[n.out[0]];
    if (y.dtype != x.dtype) { set_error("depthtospace %s: output shape / type mismatch", n.name.c_str()); return -1; }
    const int N = x.dims[0], C = dg.out_dims[1], H = x.dims[2], W = x.dims[3], r = dg.r;
    const double bytes = 2.0 * (double)y.elems();
    const bool want_gather = tamd_pin_int("d2s_form", (size_t)y.elems() >= kD2sNewFormFromBytes ? 1 : 0) == 0;
    TransposeArgs t{};
    t.identity = 1; t.form = kTransposeGather; t.total = (unsigned)y.elems();
    auto gather_step = [&](const long* strides, const int* order) {
        TransposeGeom tg;
        transpose_canon(6, dg.view_dims, strides, order, &tg);
        t.nd = tg.nd; t.unit = tg.unit;
        for (int d = 0; d < 6; d++) { t.extent[d] = tg.extent[d]; t.stride[d] = (int)tg.stride[d]; }
        const TransposeArgs a = t;
        out->push_back(make_step(n.name, transpose_kernel_name(a.form), 0, bytes, [a](hipStream_t st) { return launch_transpose(a, st); }, {access_of(x)}, {access_of(y)}, false));
    };
    if (x.dtype == TAMD_DT_UINT8) {
        if (x.is_view || fix128) { set_error("depthtospace %s reads a concat view: not supported in a uint8 graph", n.name.c_str()); return -1; }
        const long OHW = (long)H * r * W * r;
        if (want_gather && (!y.is_view || N == 1)) {
            const long strides[6] = {(long)C * r * r * H * W, (long)r * r * H * W, (long)r * H * W, (long)H * W, W, 1};
            t.x = (const uint8_t*)x.dptr; t.y = (uint8_t*)y.dptr + (size_t)y.c_off * OHW; t.src_bytes = (unsigned)x.elems();
            gather_step(strides, dg.order);
            return 0;
        }
        if (r == 1) {                                            // a copy: slice_u8 over the whole tensor, raw bytes, step 1
            SliceU8Args a{};
            for (int i = 0; i < 4; i++) { a.in_dims[i] = x.dims[i]; a.out_dims[i] = dg.out_dims[i]; a.start[i] = 0; a.step[i] = 1; }
            a.x = (const uint8_t*)x.dptr; a.y = (uint8_t*)y.dptr; a.table = nullptr; a.identity = 1;
            a.out_img = nchw_out_img(y); a.out_c0 = y.c_off; a.w2 = 0;
            out->push_back(make_step(n.name, "slice_u8", 0, bytes, [a](hipStream_t s) { return launch_slice_u8(a, s); }, {access_of(x)}, {access_of(y)}, false));
            return 0;
        }
        D2sU8Args a{};
        a.x = (const uint8_t*)x.dptr; a.y = (uint8_t*)y.dptr; a.N = N; a.C = C; a.H = H; a.W = W; a.r = r;
        a.out_img = nchw_out_img(y); a.out_c0 = y.c_off;
        out->push_back(make_step(n.name, "d2s_u8", 0, bytes, [a](hipStream_t s) { return launch_d2s_u8(a, s); }, {access_of(x)}, {access_of(y)}, false));
        return 0;
    }
    // int8: convolution-stack NHWC buffers on both sides
    if (x.nchw_raw || y.nchw_raw || x.cs <= 0 || y.cs <= 0) { set_error("depthtospace %s: a dense (permuted / flattened) tensor is not supported in an int8 graph", n.name.c_str()); return -1; }
    const int cv = rup(C, 16);
    if (x.cs % 16 || y.cs % 16 || x.c_off % 16 || y.c_off % 16 || x.c_off + x.dims[1] > x.cs || y.c_off + cv > y.cs) {
        set_error("depthtospace %s: channel slice not 16-byte aligned", n.name.c_str());
        return -1;
    }
    const size_t src_bytes = (size_t)N * H * W * x.cs - (size_t)x.c_off;
    if (want_gather && !y.is_view && y.cs == C && y.c_off == 0 && !fix128 && src_bytes < 0x7fffffffu) {
        // the NHWC output (n, h, w, s) = (n, hq, i, wq, j, s) reads the view's axes (0, 4, 2, 5, 3, 1) of a buffer with these strides
        const long strides[6] = {(long)H * W * x.cs, (long)r * r, r, 1, (long)W * x.cs, x.cs};
        const int order[6] = {0, 4, 2, 5, 3, 1};
        t.x = (const uint8_t*)x.dptr + x.c_off; t.y = (uint8_t*)y.dptr; t.src_bytes = (unsigned)src_bytes;
        gather_step(strides, order);
        return 0;
    }
    D2sI8Args a{};
    a.x = (const int8_t*)x.dptr + x.c_off; a.y = (int8_t*)y.dptr;
    a.N = N; a.C = C; a.H = H; a.W = W; a.r = r; a.cs_in = x.cs; a.ldc = y.cs; a.c_off = y.c_off; a.src_bytes = src_bytes;
    a.fix128 = fix128 ? 1 : 0;
    out->push_back(make_step(n.name, "d2s_i8", 0, bytes, [a](hipStream_t s) { return launch_d2s_i8(a, s); }, {access_of(x)}, {access_of(y)}, false));
    return 0;
}

// ---- nearest Resize of a quantised graph, both types.  Everything the reference decides for the node is decided by resize_refusal
// (node_rules.h): the output's dims, the two index vectors, the byte map, and whether the vectors are those of whole-number factors
const char* resize_refusal_of(const tamd_graph* g, const HNode& n, bool check_out, ResizeGeom* geom)
{
    if (n.in.size() != 1 || n.out.empty()) return "Resize takes one input";
    const HTensor& x = g->tensors[n.in[0]];
    const HTensor& y = g->tensors[n.out[0]];
    const bool have_q = x.scales.size() == 1 && y.scales.size() == 1;
    ResizeQuant q{};
    if (have_q) q = ResizeQuant{x.scales[0], x.zps.empty() ? 0 : x.zps[0], y.scales[0], y.zps.empty() ? 0 : y.zps[0]};
    return resize_refusal(&n.p.resize, x.dtype, (int)x.dims.size(), x.dims.data(), x.ttype == TAMD_TT_CONST, x.scales.size(), y.scales.size(), have_q ? &q : nullptr,
                          (int)y.dims.size(), check_out ? y.dims.data() : nullptr, geom);
}

// One launch, two forms (graph.h).  Both read and write what plan_interp's launches do: int8 (NHWC) reads a concat or Split view in place
// (another base and pixel stride) and writes a Concat's buffer in place through ldc / c_off -- the table saturates at +-127, so the byte
// -128 never comes out and the Concat's rule for it (plan_concat_views) does not arise --; uint8 (NCHW) writes a channel range of a
// Concat's buffer through out_img / out_c0.  Form 0 uploads the two index vectors; form 1 needs none
int plan_resize(tamd_graph* g, HNode& n, std::vector<Step>* out)
{
    ResizeGeom rg;
    const char* why = resize_refusal_of(g, n, true, &rg);
    if (why) { set_error("resize %s: %s", n.name.c_str(), why); return -1; }
    HTensor& x = g->tensors[n.in[0]];
    HTensor& y = g->tensors[n.out[0]];
    if (y.dtype != x.dtype || !rg.have_table) { set_error("resize %s: output shape / type mismatch", n.name.c_str()); return -1; }
    const int by_size = (size_t)y.elems() >= (x.dtype == TAMD_DT_INT8 ? kResizeRepFromBytesI8 : kResizeRepFromBytesU8) ? 1 : 0;      // (kernels.h: what was measured)
    const bool rep = rg.sh >= 1 && rg.sw >= 1 && tamd_pin_int("resize_form", by_size) == 1;
    std::vector<unsigned> table(64);
    memcpy(table.data(), rg.table, 256);
    int* diy = nullptr; int* dix = nullptr; unsigned* dtable = nullptr;
    if (upload(g, table, &dtable)) return -1;
    if (!rep && (upload(g, rg.iy, &diy) || upload(g, rg.ix, &dix))) return -1;
    const double bytes = (double)x.elems() + (double)y.elems();
    if (x.dtype == TAMD_DT_INT8) {
        // whole 16-byte vectors: up to the padding channels of its own buffers, never into a neighbour's slice (a view has c % 16 == 0)
        const int cv = rup(x.c, 16);
        if (x.nchw_raw || y.nchw_raw || x.cs <= 0 || y.cs <= 0 || x.cs % 16 || y.cs % 16 || x.c_off % 16 || y.c_off % 16 || x.c_off + cv > x.cs || y.c_off + cv > y.cs) {
            set_error("resize %s: channel slice not 16-byte aligned", n.name.c_str());
            return -1;
        }
        if (rep) {
            ResizeRepI8Args a{};
            a.x = (const int8_t*)x.dptr + x.c_off; a.y = (int8_t*)y.dptr;
            a.C = x.c; a.H = x.h; a.W = x.w; a.sh = rg.sh; a.sw = rg.sw; a.cs_in = x.cs; a.ldc = y.cs; a.c_off = y.c_off; a.table = dtable;
            out->push_back(make_step(n.name, "resize_rep_i8", 0, bytes, [a](hipStream_t s) { return launch_resize_rep_i8(a, s); }, {access_of(x)}, {access_of(y)}, false));
            return 0;
        }
        InterpI8Args a{};
        a.x = (const int8_t*)x.dptr + x.c_off; a.y = (int8_t*)y.dptr;
        a.N = 1; a.H = x.h; a.W = x.w; a.C = x.c; a.cs_in = x.cs;
        a.OH = y.h; a.OW = y.w; a.ldc = y.cs; a.c_off = y.c_off;
        a.iy = diy; a.ix = dix; a.table = dtable;
        out->push_back(make_step(n.name, "interp_nearest_i8", 0, bytes, [a](hipStream_t s) { return launch_interp_i8(a, s); }, {access_of(x)}, {access_of(y)}, false));
        return 0;
    }
    if (x.is_view) { set_error("resize %s reads a concat view: not supported in a uint8 graph", n.name.c_str()); return -1; }
    int identity = 1;
    for (int b = 0; b < 256; b++) identity &= rg.table[b] == b;
    if (rep) {
        ResizeRepU8Args a{};
        a.x = (const uint8_t*)x.dptr; a.y = (uint8_t*)y.dptr;
        a.C = x.c; a.H = x.h; a.W = x.w; a.sh = rg.sh; a.sw = rg.sw;
        a.out_img = nchw_out_img(y); a.out_c0 = y.c_off; a.table = dtable; a.identity = identity;
        out->push_back(make_step(n.name, "resize_rep_u8", 0, bytes, [a](hipStream_t s) { return launch_resize_rep_u8(a, s); }, {access_of(x)}, {access_of(y)}, false));
        return 0;
    }
    InterpU8Args a{};
    a.x = (const uint8_t*)x.dptr; a.y = (uint8_t*)y.dptr;
    a.N = 1; a.C = x.c; a.H = x.h; a.W = x.w; a.OH = y.h; a.OW = y.w;
    a.out_img = nchw_out_img(y); a.out_c0 = y.c_off;
    a.iy = diy; a.ix = dix; a.table = dtable; a.identity = identity;
    out->push_back(make_step(n.name, "interp_nearest_u8", 0, bytes, [a](hipStream_t s) { return launch_interp_u8(a, s); }, {access_of(x)}, {access_of(y)}, false));
    return 0;
}

int plan_topdown_u8(tamd_graph* g, HNode& in, HNode& cn, HNode& n, std::vector<Step>* out)
{
    const std::string node = in.name + "+" + cn.name + "+" + n.name;
    HTensor& x = g->tensors[in.in[0]];
    HTensor& mid = g->tensors[in.out[0]];
    HTensor& cut = g->tensors[cn.out[0]];
    const int u_first = n.in[0] == cn.out[0] ? 1 : 0;
    HTensor& lat = g->tensors[n.in[u_first ? 1 : 0]];
    HTensor& y = g->tensors[n.out[0]];
    InterpGeom geom;
    std::vector<int> iy, ix;
    CropGeom cg;
    int gated = -1;
    const char* why = interp_refusal(&in.p.interp, x.dtype, (int)x.dims.size(), x.dims.data(), x.ttype == TAMD_TT_CONST, x.scales.size(), mid.scales.size(), &geom, &iy, &ix);
    if (!why) why = crop_refusal_of(g, cn, true, &cg);
    if (!why) why = eltwise_refusal_of(g, n, &gated);
    if (why) { set_error("topdown %s: %s", node.c_str(), why); return -1; }
    if (x.dtype != TAMD_DT_UINT8 || gated != kEltSame || cn.in[0] != in.out[0] || mid.dims.size() != 4 || mid.dims[2] != geom.out_h || mid.dims[3] != geom.out_w || cg.start[1] != 0
        || cg.out_dims[1] != x.dims[1] || cg.out_dims[0] != x.dims[0] || lat.dims != cut.dims || y.dims != cut.dims || x.is_view || lat.is_view || y.is_view || !x.nchw_raw
        || !lat.nchw_raw || !y.nchw_raw || lat.dtype != x.dtype || y.dtype != x.dtype) {
        set_error("topdown %s: the three nodes do not run as one launch", node.c_str());
        return -1;
    }
    iy = std::vector<int>(iy.begin() + cg.start[2], iy.begin() + cg.start[2] + cg.out_dims[2]);          // (inside the vectors: crop_refusal's box check)
    ix = std::vector<int>(ix.begin() + cg.start[3], ix.begin() + cg.start[3] + cg.out_dims[3]);
    for (int v : iy) if (v < 0 || v >= x.dims[2]) { set_error("topdown %s: a source row leaves the input", node.c_str()); return -1; }
    for (int v : ix) if (v < 0 || v >= x.dims[3]) { set_error("topdown %s: a source column leaves the input", node.c_str()); return -1; }
    std::vector<unsigned> table(64);
    if (tamd_interp_table(x.dtype, x.scales[0], x.zps.empty() ? 0 : x.zps[0], mid.scales[0], mid.zps.empty() ? 0 : mid.zps[0], (unsigned char*)table.data())) {
        set_error("topdown %s: not supported on the device for data type %d", node.c_str(), x.dtype);
        return -1;
    }
    int* diy = nullptr; int* dix = nullptr; unsigned* dtable = nullptr;
    if (upload(g, iy, &diy) || upload(g, ix, &dix) || upload(g, table, &dtable)) return -1;
    TopdownU8Args a{};
    a.small = (const uint8_t*)x.dptr; a.lat = (const uint8_t*)lat.dptr; a.y = (uint8_t*)y.dptr;
    a.planes = (long)x.dims[0] * x.dims[1]; a.H = x.dims[2]; a.W = x.dims[3]; a.OH = cg.out_dims[2]; a.OW = cg.out_dims[3];
    a.iy = diy; a.ix = dix; a.table = dtable;
    a.identity = 1;
    for (int b = 0; b < 256; b++) a.identity &= ((const unsigned char*)table.data())[b] == b;
    a.type = n.p.elt.type; a.u_first = u_first;
    a.su = cut.scales[0]; a.zu = cut.zps.empty() ? 0 : cut.zps[0];                 // the Eltwise reads the Crop's output tensor: ITS parameters
    a.sl = lat.scales[0]; a.zl = lat.zps.empty() ? 0 : lat.zps[0];
    a.out_scale = y.scales[0]; a.out_zp = y.zps.empty() ? 0 : y.zps[0];
    out->push_back(make_step(node, "topdown_u8", 0, 2.0 * (double)y.elems() + (double)x.elems(), [a](hipStream_t s) { return launch_topdown_u8(a, s); },
                             {access_of(x), access_of(lat)}, {access_of(y)}, false));
    if (g->fused_away.size() != g->tensors.size()) g->fused_away.assign(g->tensors.size(), 0);
    g->fused_away[in.out[0]] = 1;                            // neither the up-sampled map nor its cut is ever written
    g->fused_away[cn.out[0]] = 1;
    return 0;
}

// The uint8 forms (graph_u8.hip calls these): dense NCHW, one chan_map_u8 launch per output tensor.  Neither planner makes these
// nodes' tensors concat views (plan_u8: in_place), which the errors below guard
static int plan_chan_map_u8(tamd_graph* g, const std::string& node, const HTensor& x, const HTensor& y, const std::vector<int>& planes, const unsigned char* map,
                            Step* out)
{
    if (x.is_view || y.is_view || !x.nchw_raw || !y.nchw_raw) { set_error("%s on a concat view is not supported in a uint8 graph", node.c_str()); return -1; }
    if (planes.size() != (size_t)y.c || y.n != x.n || y.h != x.h || y.w != x.w) { set_error("%s: output shape mismatch", node.c_str()); return -1; }
    for (int p : planes)
        if (p < 0 || p >= x.c) { set_error("%s: a source channel leaves its tensor", node.c_str()); return -1; }
    ChanMapU8Args a{};
    a.identity = 1;
    std::vector<unsigned> table(64, 0u);
    if (map) {
        memcpy(table.data(), map, 256);
        for (int b = 0; b < 256; b++) a.identity &= map[b] == b;
    }
    int* dplanes = nullptr; unsigned* dtable = nullptr;
    if (upload(g, planes, &dplanes) || upload(g, table, &dtable)) return -1;
    a.x = (const uint8_t*)x.dptr; a.y = (uint8_t*)y.dptr;
    a.N = y.n; a.C = y.c; a.HW = y.h * y.w; a.in_img = x.c * x.h * x.w; a.in_planes = x.c;
    a.out_img = nchw_out_img(y); a.out_c0 = y.c_off; a.src_plane = dplanes; a.table = dtable;
    *out = make_step(node, "chan_map_u8", 0, 2.0 * (double)y.elems(), [a](hipStream_t s) { return launch_chan_map_u8(a, s); }, {access_of(x)}, {access_of(y)}, false);
    return 0;
}

// split_ref.c:68-107: output i is channels [first_i, ..) of the input, every byte through tamd_split_table between the two tensors'
// parameters (the identity between equal ones: no lookups)
int plan_split_u8(tamd_graph* g, HNode& n, std::vector<Step>* out)
{
    HTensor& x = g->tensors[n.in[0]];
    std::vector<size_t> oq;
    for (int o : n.out) oq.push_back(g->tensors[o].scales.size());
    const char* why = split_refusal(&n.p.split, x.dtype, (int)x.dims.size(), x.dims.data(), x.ttype == TAMD_TT_CONST, x.scales.size(), (int)n.out.size(), oq.data());
    if (why) { set_error("split %s: %s", n.name.c_str(), why); return -1; }
    int first = 0;
    for (size_t i = 0; i < n.out.size(); i++) {
        HTensor& y = g->tensors[n.out[i]];
        if (y.dtype != x.dtype || y.dims.size() != 4 || y.c != n.p.split.sizes[i]) { set_error("split %s: output shape / type mismatch", n.name.c_str()); return -1; }
        std::vector<int> planes((size_t)y.c);
        for (int c = 0; c < y.c; c++) planes[c] = first + c;
        unsigned char map[256];
        if (tamd_split_table(x.scales[0], x.zps.empty() ? 0 : x.zps[0], y.scales[0], y.zps.empty() ? 0 : y.zps[0], map)) { set_error("split %s: no byte map", n.name.c_str()); return -1; }
        Step st;
        if (plan_chan_map_u8(g, n.name, x, y, planes, map, &st)) return -1;
        out->push_back(st);
        first += y.c;
    }
    return 0;
}

int plan_shuffle_u8(tamd_graph* g, HNode& n, std::vector<Step>* out)
{
    HTensor& x = g->tensors[n.in[0]];
    HTensor& y = g->tensors[n.out[0]];
    std::vector<int> src;
    if (shuffle_sources(n, x, y, &src)) return -1;
    Step st;
    if (plan_chan_map_u8(g, n.name, x, y, src, nullptr, &st)) return -1;
    out->push_back(st);
    return 0;
}

}  // namespace tamd

extern "C" int tamd_graph_bytemap_chain(const tamd_graph* g, int node, int* nodes, int cap, unsigned char table[256])
{
    using namespace tamd;
    if (!g || node < 0 || node >= (int)g->nodes.size() || !nodes || cap < 0 || !table) return -1;
    ByteChain c;
    if (!bytemap_chain_from(g, (size_t)node, [](int) { return true; }, [&](int t) { return g->tensors[t].ttype != TAMD_TT_CONST; }, &c)) return 0;
    for (size_t k = 0; k < c.nodes.size() && (int)k < cap; k++) nodes[k] = c.nodes[k];
    memcpy(table, c.table, 256);
    return (int)c.nodes.size();
}

extern "C" int tamd_graph_instancenorm_plan(const tamd_graph* g, int node, int* form, int* relu_node)
{
    using namespace tamd;
    if (!g || node < 0 || node >= (int)g->nodes.size() || !form || !relu_node) return -1;
    const HNode& n = g->nodes[(size_t)node];
    if (n.op != TAMD_OP_INSTANCENORM || instancenorm_refusal_of(g, n)) return -1;
    const HTensor& x = g->tensors[n.in[0]];
    *form = instancenorm_form((size_t)x.dims[2] * (size_t)x.dims[3]);
    *relu_node = instancenorm_relu_next(g, (size_t)node);
    return 0;
}
