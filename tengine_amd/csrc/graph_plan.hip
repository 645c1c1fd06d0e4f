// The int8 planner: I8Layout's passes (dense tensors, views, activation buffers), one function per node kind and plan_i8() itself --
// node list -> launch list (NHWC int8).  The convolution / FC / pooling launches are planned in graph_plan_conv.hip, the pair fusions
// (pointwise + depthwise, depthwise + pointwise) in graph_plan_pairs.hip, the byte-map nodes (tables, PReLU, Interp, Split,
// ShuffleChannel) in graph_plan_maps.hip; what all three planners share (dev_alloc, append_steps, ..) is graph_plan_common.hip.
#include "graph.h"
#include "graph_internal.h"
#include "env.h"

#include <stdio.h>

#include <algorithm>

#include "graph_plan.h"

namespace tamd {

// ---- DENSE tensors (the SSD head plumbing of an int8 graph).  The convolution stack lives in NHWC buffers
// with padded channels; what Permute(0,2,3,1) / PriorBox produce, and everything that is only a re-reading of it (Flatten, Reshape,
// Concat on any axis, Softmax on any axis), lives in the reference's own dense element order (HTensor::nchw_raw, cs = 0): those ops
// are byte copies / views there (permute_ref.c:305-343, flatten_ref.c:74-80, reshape_ref.c:76-90), and a graph output needs no
// layout pass.  L.perm_src[t] >= 0: t is NHWC tensor L.perm_src[t] seen through Permute(0,2,3,1) (+ views) -- a Concat reads the NHWC
// buffer itself (flatcat_i8, kind 1) and the permuted copy is never written unless something else reads it too.
static int plan_dense(tamd_graph* g, I8Layout& L)
{
    const size_t NT = g->tensors.size();
    std::vector<char> need_buf(NT, 0);
    auto root = [&](int t) { for (int hop = 0; hop < 16 && L.alias_of[t] >= 0; hop++) t = L.alias_of[t]; return t; };
    for (size_t ni = 0; ni < g->nodes.size(); ni++) {
        HNode& n = g->nodes[ni];
        if (n.op == TAMD_OP_INPUT || n.op == TAMD_OP_CONST || n.in.empty() || n.out.empty()) continue;
        HTensor& x = g->tensors[n.in[0]];
        const int yo = n.out[0];
        switch (n.op) {
        case TAMD_OP_PERMUTE: {
            if (x.dims.size() != 4 || L.dense[n.in[0]] || !permute_order_on_device(n.p.perm.order)) {
                set_error("permute %s: only order (0, 2, 3, 1) of a 4-D convolution-stack tensor runs on the device", n.name.c_str());
                return -1;
            }
            L.dense[yo] = 1; L.perm_src[yo] = n.in[0];
            break;
        }
        case TAMD_OP_PRIORBOX: L.dense[yo] = 1; break;
        case TAMD_OP_RESHAPE: L.dense[yo] = 1; if (L.dense[n.in[0]]) { L.alias_of[yo] = n.in[0]; L.perm_src[yo] = L.perm_src[n.in[0]]; } break;
        case TAMD_OP_DROPOUT: case TAMD_OP_FLATTEN:
            if (L.dense[n.in[0]]) { L.dense[yo] = 1; L.alias_of[yo] = n.in[0]; L.perm_src[yo] = L.perm_src[n.in[0]]; }
            else {
                // Flatten of an H x W map: the [N, C*H*W] result is the SAME NCHW element order; on the device it stays the NHWC
                // buffer and keeps the 4-D geometry, so a following FC (== conv whose kernel covers the map), the NCHW output
                // conversion and a flat Concat (kind 2) all see (c, h, w).  Set HERE, in node order: the Concat case below looks
                // at the geometry of its inputs (a 2-D tensor that is a flattened MAP must not take the channel-concat path --
                // it did until round 6 and wrote N*H*W rows into an N-row output)
                L.alias_of[yo] = n.in[0];
                HTensor& yy = g->tensors[yo];
                yy.n = x.n; yy.c = x.c; yy.h = x.h; yy.w = x.w;
            }
            break;
        case TAMD_OP_SOFTMAX: if (L.dense[n.in[0]]) L.dense[yo] = 1; break;
        // the result of a Transpose is dense, whatever it reads: a dense tensor, or a convolution-stack tensor where it lies (plan_transpose)
        case TAMD_OP_TRANSPOSE: L.dense[yo] = 1; break;
        case TAMD_OP_SIGMOID: case TAMD_OP_CLIP: if (L.dense[n.in[0]]) L.dense[yo] = 1; break;       // a byte map keeps the element order it finds
        case TAMD_OP_CONCAT: {
            HTensor& y = g->tensors[yo];
            const int ax = n.p.concat.axis < 0 ? n.p.concat.axis + (int)y.dims.size() : n.p.concat.axis;
            bool any_dense = false, any_map = false;
            for (int i : n.in) { any_dense |= L.dense[i] != 0; any_map |= g->tensors[i].h * g->tensors[i].w > 1; }
            if (any_dense || ax != 1 || (y.dims.size() != 4 && any_map)) {
                L.flat_concat[ni] = 1; L.dense[yo] = 1;
            }
            break;
        }
        default:
            for (int i : n.in)
                if (g->tensors[i].ttype != TAMD_TT_CONST && L.dense[i]) {
                    set_error("%s reads %s, a tensor in dense (permuted / flattened) order: only Flatten, Reshape, Concat and Softmax do on the device", n.name.c_str(), g->tensors[i].name.c_str());
                    return -1;
                }
        }
    }
    // Reshape -> Transpose of a convolution-stack tensor as ONE launch and no reshape_i8 copy: the Reshape's only reader is the Transpose,
    // it is no graph output, and every axis of the reshaped tensor factors exactly one of the source's N, C, H * W index ranges
    // (nhwc_view_strides) -- the Transpose then reads the source's buffer under the strides that follow from (H * W * cs, 1, cs).  A
    // Reshape that mixes C with H or W keeps its copy.  TAMD_PIN=transpose_view=0: the copy always (A/B runs; the bytes are the same)
    std::vector<char> viewed(NT, 0);
    for (size_t ti = 0; ti < g->nodes.size() && tamd_pin_int("transpose_view", 1); ti++) {
        const HNode& t = g->nodes[ti];
        if (t.op != TAMD_OP_TRANSPOSE || t.in.empty()) continue;
        const int mid = t.in[0];
        if (count_consumers(g, mid) != 1 || L.alias_of[mid] >= 0) continue;                 // (a graph output counts as a consumer)
        for (size_t ri = 0; ri < ti; ri++) {
            const HNode& r = g->nodes[ri];
            if (r.op != TAMD_OP_RESHAPE || r.out.empty() || r.out[0] != mid || L.dense[r.in[0]] || g->tensors[r.in[0]].ttype == TAMD_TT_CONST) continue;
            HTensor s = g->tensors[r.in[0]];
            long strides[8];
            s.cs = rup(s.c, 16);                                                            // (any padding: only the factoring is asked here)
            if (!nhwc_view_strides(s, g->tensors[mid].dims, strides)) continue;
            L.tview[ti] = (int)ri + 1; L.fused[ri] = 1; viewed[mid] = 1;
        }
    }
    // who needs the bytes of a dense tensor in memory: everything but the flat Concat of a lazily permuted tensor (and its views)
    for (size_t ni = 0; ni < g->nodes.size(); ni++) {
        const HNode& n = g->nodes[ni];
        for (int i : n.in) {
            if (g->tensors[i].ttype == TAMD_TT_CONST || !L.dense[i] || viewed[i]) continue;
            const bool is_alias_op = !n.out.empty() && L.alias_of[n.out[0]] == i;
            if (is_alias_op) continue;
            if (!(L.flat_concat[ni] && L.perm_src[i] >= 0)) need_buf[root(i)] = 1;
        }
    }
    for (auto& io : g->outputs) if (L.dense[io.tensor]) need_buf[root(io.tensor)] = 1;
    for (size_t t = 0; t < NT; t++) {
        if (!L.dense[t]) continue;
        if (need_buf[root((int)t)]) L.perm_src[t] = -1;              // materialised: its readers take the dense bytes
        HTensor& d = g->tensors[t];
        d.nchw_raw = true; d.cs = 0; d.c_off = 0;
    }
    for (size_t t = 0; t < NT; t++) {
        HTensor& d = g->tensors[t];
        if (!L.dense[t] || L.alias_of[t] >= 0) continue;
        if (d.dtype != TAMD_DT_INT8) { set_error("tensor %s: dtype %d not supported on the device yet", d.name.c_str(), d.dtype); return -1; }
        if (L.perm_src[t] >= 0 || viewed[t]) continue;                // never written: read through its NHWC source
        if (dev_alloc(g, &d.dptr, d.elems(), true)) return -1;
    }
    return 0;
}

// concat outputs own a buffer; their inputs become views when layouts allow (concat-by-offset:
// concat/concat_kernel_ref_int8.c with in_scale == out_scale is a pure copy)
// An input that cannot be written in place (its scale differs -> the reference rescales, concat_kernel_ref_int8.c:70-80;
// channel count / offset not a multiple of 16; produced or also consumed by a kernel that does not address channel
// slices; a graph input) keeps its own buffer and is copied by concat_copy_i8 at the concat's position.
// the operators whose launches address a channel slice of a wider buffer, on the side they read and on the side they write
static bool slice_capable(int op) { return op == TAMD_OP_CONV || op == TAMD_OP_FC || op == TAMD_OP_POOL || op == TAMD_OP_UPSAMPLE || op == TAMD_OP_INTERP || op == TAMD_OP_DEPTHTOSPACE || op == TAMD_OP_RESIZE; }
// .. and on the side they read alone.  Split and ShuffleChannel are NOT written in place into a Concat's buffer: they hand on the byte
// -128 where their input holds it, and the reference's Concat of several inputs turns that byte into 127 even between equal scales
// (concat_kernel_ref_int8.c:83-84) -- concat_copy_i8 does that, a view would not.  Upsample holds that byte too and IS written in
// place: its launch stores 127 for it, where the Concat is its only reader (plan_concat_views, plan_upsample).  DepthToSpace moves raw
// bytes, -128 among them, and follows the Upsample's rule (plan_depthtospace: D2sI8Args::fix128)
// A Transpose reads its source through strides (plan_transpose): a channel slice is the same read from another base
static bool reads_slices(int op) { return slice_capable(op) || op == TAMD_OP_SPLIT || op == TAMD_OP_SHUFFLECHANNEL || op == TAMD_OP_TRANSPOSE; }

static int plan_concat_views(tamd_graph* g, I8Layout& L)
{
    auto producer_op = [&](int t) { for (auto& n : g->nodes) for (int o : n.out) if (o == t) return n.op; return -1; };     // (a Split has several outputs)
    for (auto& n : g->nodes) {
        // (a Concat that runs inside its ShuffleChannel's launch writes no buffer: its inputs must not become slices of one)
        if (n.op != TAMD_OP_CONCAT || L.flat_concat[&n - g->nodes.data()] || L.cat_shuffle[&n - g->nodes.data()]) continue;
        HTensor& y = g->tensors[n.out[0]];
        int ax = n.p.concat.axis < 0 ? n.p.concat.axis + (int)y.dims.size() : n.p.concat.axis;
        if (ax != 1 || y.dims.size() < 2) { set_error("concat %s: only the channel axis is supported on the device", n.name.c_str()); return -1; }
        if (y.scales.empty()) { set_error("concat %s: missing quant params", n.name.c_str()); return -1; }
        int off = 0;
        for (int i : n.in) {
            HTensor& x = g->tensors[i];
            if (x.dtype != y.dtype || x.scales.empty()) { set_error("concat %s: input %s: dtype / quant params", n.name.c_str(), x.name.c_str()); return -1; }
            bool ok = (x.c % 16 == 0) && (off % 16 == 0) && (x.scales[0] == y.scales[0] || n.in.size() == 1) && x.ttype == TAMD_TT_VAR
                      && L.view_of[i] < 0 && slice_capable(producer_op(i));
            for (auto& c : g->nodes)            // every other reader must cope with a channel slice too
                for (int ci : c.in)
                    if (ci == i && &c != &n && !(reads_slices(c.op) || c.op == TAMD_OP_CONCAT)) ok = false;
            int readers = 0;
            for (int ci : n.in) readers += (ci == i);
            if (readers > 1) ok = false;        // the same tensor twice: one copy per position
            // an Upsample hands on the byte -128 and can emit it (misc_kernels.hip: upsample_i8 runs the reference's uint8 routine on the
            // bytes), and a Concat of several inputs stores 127 for it.  In place, the Upsample's launch stores 127 itself
            // (UpsampleI8Args::fix128) -- which is what the Concat's readers must see and NOT what another reader of the Upsample's own
            // tensor must see: with a second reader it keeps its buffer and concat_copy_i8 copies.  (Conv, FC, Pool and Interp
            // saturate at +-127 and never hold the byte.)
            if ((producer_op(i) == TAMD_OP_UPSAMPLE || producer_op(i) == TAMD_OP_DEPTHTOSPACE) && n.in.size() > 1 && count_consumers(g, i) > 1) ok = false;      // (DepthToSpace: raw bytes, the same rule)
            if (ok) { L.view_of[i] = n.out[0]; L.view_off[i] = off; L.in_multi_cat[i] = n.in.size() > 1; }
            off += x.c;
        }
    }
    return 0;
}

// Concat -> ShuffleChannel as ONE launch (ShuffleNet-v2: every unit ends in this pair).  A channel Concat whose every input carries the
// Concat's scale is a copy in the reference but for one byte (concat_kernel_ref_int8.c:70-84 rescales otherwise; -128 comes out as 127
// from a Concat of several inputs: ChanMapI8Args::fix128), the ShuffleChannel behind it is a copy always: together they are one
// channel map from the Concat's inputs to the ShuffleChannel's output, and the Concat's own tensor is never written.  Matched BEFORE plan_concat_views, so that the inputs are not turned into slices of a buffer nobody writes.
// TAMD_PIN=cat_shuffle=0: two steps (A/B runs and the fused == unfused tests)
static void match_cat_shuffle(tamd_graph* g, I8Layout& L)
{
    if (!tamd_pin_int("cat_shuffle", 1)) return;
    for (size_t ni = 0; ni < g->nodes.size(); ni++) {
        const HNode& n = g->nodes[ni];
        if (n.op != TAMD_OP_CONCAT || L.flat_concat[ni] || n.in.empty() || n.in.size() > (size_t)kChanMapMaxSrc) continue;
        const HTensor& y = g->tensors[n.out[0]];
        const int ax = n.p.concat.axis < 0 ? n.p.concat.axis + (int)y.dims.size() : n.p.concat.axis;
        if (ax != 1 || y.dims.size() != 4 || y.dtype != TAMD_DT_INT8 || y.scales.size() != 1) continue;
        bool copy = true;
        for (int i : n.in) {
            const HTensor& x = g->tensors[i];
            copy &= x.ttype != TAMD_TT_CONST && x.dtype == y.dtype && x.dims.size() == 4 && x.scales.size() == 1 && (x.scales[0] == y.scales[0] || n.in.size() == 1);
        }
        const int sj = copy ? sole_reader(g, n.out[0]) : -1;            // (a graph output counts as a consumer)
        if (sj < 0 || g->nodes[sj].op != TAMD_OP_SHUFFLECHANNEL || sj < (int)ni) continue;
        L.cat_shuffle[ni] = sj + 1;
    }
}

// Split outputs as VIEWS of the Split's input: an output whose first channel and width are multiples of 16 is a channel slice of the
// input's pixels as they lie, so it needs no launch where every reader addresses channel slices.  Neither tensor may be a graph input
// or output (those keep their own staging).  view_of / view_off carry it like a concat view: root_of (plan_buffers) keeps the input's
// buffer alive until the last reader of the view.  At ShuffleNet's own widths (58, 116, 232) nothing aligns and plan_split copies
static void plan_split_views(tamd_graph* g, I8Layout& L)
{
    auto is_io = [&](int t) {
        for (auto& io : g->inputs) if (io.tensor == t) return true;
        for (auto& io : g->outputs) if (io.tensor == t) return true;
        return false;
    };
    for (auto& n : g->nodes) {
        if (n.op != TAMD_OP_SPLIT || n.in.empty()) continue;
        const HTensor& x = g->tensors[n.in[0]];
        if (x.ttype != TAMD_TT_VAR || x.dims.size() != 4 || L.dense[n.in[0]] || is_io(n.in[0])) continue;
        int first = 0;
        for (int t : n.out) {
            const int width = g->tensors[t].c;
            bool ok = first % 16 == 0 && width % 16 == 0 && width > 0 && !is_io(t) && L.view_of[t] < 0;
            for (size_t ci = 0; ci < g->nodes.size(); ci++)
                for (int i : g->nodes[ci].in)
                    if (i == t && !(reads_slices(g->nodes[ci].op) || (g->nodes[ci].op == TAMD_OP_CONCAT && !L.flat_concat[ci]))) ok = false;
            if (ok) { L.view_of[t] = n.in[0]; L.view_off[t] = first; }
            first += width;
        }
    }
}

// Byte map -> channel-gate Eltwise as ONE launch (the tail of a Squeeze-and-Excitation block: Sigmoid -> Eltwise PROD(x, gate)): the
// Eltwise's launch reads the byte map's INPUT and maps the N * C gate bytes through the node's table itself (chan_gate.hip), the byte map
// has no launch and its output is never written.  Matched BEFORE plan_buffers: the launch runs at the Eltwise's position and reads the
// byte map's input there, past that tensor's last reader in node order, and plan_buffers keeps it alive until then.  Neither tensor of
// the byte map may be a concat view, an alias or dense (permuted / flattened) here.  TAMD_PIN=gate_lut=0: two launches
static void match_gate_lut(tamd_graph* g, I8Layout& L)
{
    for (size_t ei = 0; ei < g->nodes.size(); ei++) {
        const HNode& e = g->nodes[ei];
        int gated = -1;
        if (e.op != TAMD_OP_ELTWISE || eltwise_refusal_of(g, e, &gated) || gated < 0) continue;
        const int pj = gate_lut_producer(g, e, gated);
        if (pj < 0 || pj >= (int)ei || L.fused[pj]) continue;
        bool plain = true;
        for (int t : {g->nodes[pj].in[0], g->nodes[pj].out[0], e.in[gated], e.out[0]}) plain &= L.view_of[t] < 0 && L.alias_of[t] < 0 && !L.dense[t];
        if (!plain) continue;
        L.gate_lut[ei] = pj + 1; L.fused[pj] = 1;
    }
}

// graph inputs: NCHW staging; first conv with <=4 channels reads NCHW directly
static int plan_input_staging(tamd_graph* g)
{
    for (auto& io : g->inputs) {
        HTensor& t = g->tensors[io.tensor];
        io.bytes = t.elems() * esize(t.dtype);
        if (dev_alloc(g, &io.stage, io.bytes + 64, true)) return -1;     // slack: the first-layer kernel over-reads the last row by < 8 bytes
        bool direct = (t.dims.size() == 4 && t.c <= 4 && count_consumers(g, io.tensor) == 1);
        if (direct) {
            for (auto& n : g->nodes)
                if (n.op == TAMD_OP_CONV && n.in[0] == io.tensor && n.p.conv.group != 1) direct = false;
                else if (n.op != TAMD_OP_CONV && !n.in.empty() && n.in[0] == io.tensor) direct = false;
        }
        if (direct) { t.nchw_raw = true; t.dptr = io.stage; t.cs = 0; }
    }
    return 0;
}

// byte-pure chains (bytemap_chain_from, graph_plan_maps.hip) as one lut_u8 launch each, at the LAST member's position: no member is
// planned inside another launch already, and the source, the tensors between and the result are convolution-stack tensors with
// buffers of their own.  In front of plan_buffers: the source is read at the last member's position
static void match_bytemap_chains(tamd_graph* g, I8Layout& L)
{
    auto node_free = [&](int k) { return !L.fused[k] && !L.gate_lut[k] && !L.tview[k] && !L.cat_shuffle[k] && !L.chain_at[k]; };
    auto tensor_plain = [&](int t) { return g->tensors[t].ttype != TAMD_TT_CONST && L.view_of[t] < 0 && L.alias_of[t] < 0 && !L.dense[t] && !L.in_multi_cat[t]; };
    for (size_t ni = 0; ni < g->nodes.size(); ni++) {
        ByteChain c;
        if (!bytemap_chain_from(g, ni, node_free, tensor_plain, &c)) continue;      // (a byte map inside its gate's launch is fused[]: no member)
        for (size_t k = 0; k + 1 < c.nodes.size(); k++) L.fused[c.nodes[k]] = 1;
        L.chains.push_back(c);
        L.chain_at[c.nodes.back()] = (int)L.chains.size();
    }
}

// ---- activation buffers.  Tensors whose lifetimes cannot overlap share device memory (tamd_options.keep_tensors = 0, the
// default): a pass then touches a fraction of the bytes -- ResNet-50 at batch 32 owns 345 MB of activations one by one, more
// than the 256 MB last-level cache, but never has more than ~65 MB of them alive.  Lifetime of a buffer, in node positions
// (the launch list follows the node order, except that a fused tail runs at ITS PRODUCER's position and a fused
// eltwise / ReLU at the position of the convolution that absorbs it): written from `birth` = the earliest producer within two
// hops above the node that produces it (covers both exceptions, conservatively) -- THREE hops for the output of a depthwise conv
// behind a pointwise conv behind a depthwise conv: chain4.hip runs those three at the position of the conv in front of them, so its
// launch writes that output while it reads that conv's input, and the two must never share memory -- read until `death` = the last
// node that names it (or a view / alias of it) as an input.  A launch reads and writes in one go, so buffers with birth == death of
// another never share.  Graph inputs / outputs and tensors with padding channels (cs != c: their padding bytes are zero from
// the allocation on and stay zero) keep their own buffers.
static int plan_buffers(tamd_graph* g, I8Layout& L)
{
    std::vector<size_t> own;                     // tensors that own a buffer (not a constant, a raw input, a view or an alias)
    for (size_t i = 0; i < g->tensors.size(); i++) {
        HTensor& t = g->tensors[i];
        if (t.ttype == TAMD_TT_CONST || t.nchw_raw) continue;
        if (L.view_of[i] >= 0 || L.alias_of[i] >= 0) continue;
        if (t.dtype != TAMD_DT_INT8) { set_error("tensor %s: dtype %d not supported on the device yet", t.name.c_str(), t.dtype); return -1; }
        t.cs = rup(t.c, 16);
        // a 1x1-map graph output written by conv/fc/pool (dword stores) keeps its channels dense, so the
        // NHWC buffer IS the reference's NCHW order and no output layout pass is needed
        if (t.h * t.w == 1 && t.c % 4 == 0 && count_consumers(g, (int)i) == 1) {
            bool is_out = false, dword_producer = false;
            for (auto& o : g->outputs) is_out |= (o.tensor == (int)i);
            for (auto& n : g->nodes)
                if (n.out.size() == 1 && n.out[0] == (int)i)      // (a node with several outputs -- Split -- stores bytes)
                    dword_producer = (n.op == TAMD_OP_CONV || n.op == TAMD_OP_FC || n.op == TAMD_OP_POOL || n.op == TAMD_OP_SOFTMAX);   // (softmax: byte stores, any stride)
            if (is_out && dword_producer) t.cs = t.c;
        }
        own.push_back(i);
    }
    g->pooled.assign(g->tensors.size(), 0);
    const char* pe = getenv("TAMD_POOL");
    const bool pool = pe ? atoi(pe) != 0 : !g->opt.keep_tensors;
    const int NN = (int)g->nodes.size();
    auto root_of = [&](int t) { for (int hop = 0; hop < 8; hop++) { if (L.view_of[t] >= 0) t = L.view_of[t]; else if (L.alias_of[t] >= 0) t = L.alias_of[t]; else break; } return t; };
    std::vector<int> prod(g->tensors.size(), -1), birth(g->tensors.size(), NN), death(g->tensors.size(), -1);
    for (int ni = 0; ni < NN; ni++)
        for (int o : g->nodes[ni].out) prod[o] = ni;
    auto up = [&](int ni) { int e = ni; for (int i : g->nodes[ni].in) if (g->tensors[i].ttype != TAMD_TT_CONST && prod[i] >= 0) e = std::min(e, prod[i]); return e; };
    for (int ni = 0; ni < NN; ni++) {
        const HNode& n = g->nodes[ni];
        if (n.op == TAMD_OP_INPUT || n.op == TAMD_OP_CONST) continue;
        int e = ni;
        for (int i : n.in) if (g->tensors[i].ttype != TAMD_TT_CONST && prod[i] >= 0) e = std::min(e, up(prod[i]));
        // the chain of four (find_chain4's node shape, whether or not the chain is taken later): dw <- 1x1 conv <- dw <- its producer
        auto conv_in = [&](int k) { const HNode& c = g->nodes[k]; return c.op == TAMD_OP_CONV && !c.in.empty() ? prod[c.in[0]] : -1; };
        if (n.op == TAMD_OP_CONV && n.p.conv.group > 1) {
            const int p2 = conv_in(ni), d1 = p2 >= 0 && g->nodes[p2].op == TAMD_OP_CONV && g->nodes[p2].p.conv.group == 1 ? conv_in(p2) : -1;
            if (d1 >= 0 && g->nodes[d1].op == TAMD_OP_CONV && g->nodes[d1].p.conv.group > 1) e = std::min(e, up(d1));
        }
        for (int o : n.out) { const int r = root_of(o); birth[r] = std::min(birth[r], e); death[r] = std::max(death[r], ni); }
        for (int i : n.in) if (g->tensors[i].ttype != TAMD_TT_CONST) { const int r = root_of(i); death[r] = std::max(death[r], ni); }
    }
    // an NHWC tensor that a flat Concat reads THROUGH its Permute (perm_src) is read at the Concat's position, not at the Permute's
    for (int ni = 0; ni < NN; ni++)
        if (L.flat_concat[ni])
            for (int i : g->nodes[ni].in)
                if (L.perm_src[i] >= 0) { const int r = root_of(L.perm_src[i]); death[r] = std::max(death[r], ni); }
    // the input of a byte map that runs inside its channel-gate Eltwise's launch (match_gate_lut) is read at the ELTWISE's position
    for (int ni = 0; ni < NN; ni++)
        if (L.gate_lut[ni]) { const int r = root_of(g->nodes[L.gate_lut[ni] - 1].in[0]); death[r] = std::max(death[r], ni); }
    // the source of a byte-pure chain (match_bytemap_chains) is read at the LAST member's position
    for (int ni = 0; ni < NN; ni++)
        if (L.chain_at[ni]) { const int r = root_of(L.chains[L.chain_at[ni] - 1].src); death[r] = std::max(death[r], ni); }
    // the source of a Reshape that its Transpose reads through (plan_dense: tview) is read at the TRANSPOSE's position
    for (int ni = 0; ni < NN; ni++)
        if (L.tview[ni]) { const int r = root_of(g->nodes[L.tview[ni] - 1].in[0]); death[r] = std::max(death[r], ni); }
    std::vector<char> pinned(g->tensors.size(), 0);
    for (auto& io : g->inputs) pinned[root_of(io.tensor)] = 1;
    for (auto& io : g->outputs) pinned[root_of(io.tensor)] = 1;
    struct Blk { size_t t, bytes, off; int b, d; };
    std::vector<Blk> blks;
    auto bytes_of = [&](const HTensor& t) { return ((size_t)t.n * t.h * t.w * t.cs + 1024 + 255) & ~(size_t)255; };
    for (size_t i : own) {
        HTensor& t = g->tensors[i];
        g->unpooled_bytes += bytes_of(t);
        if (pool && !pinned[i] && t.cs == t.c && death[i] >= 0 && birth[i] <= death[i]) blks.push_back({i, bytes_of(t), 0, birth[i], death[i]});
        else if (dev_alloc(g, &t.dptr, (size_t)t.n * t.h * t.w * t.cs, true)) return -1;
    }
    // greedy by size: the largest buffers first, each at the lowest offset that is free over its whole lifetime
    std::sort(blks.begin(), blks.end(), [](const Blk& a, const Blk& b) { return a.bytes != b.bytes ? a.bytes > b.bytes : a.t < b.t; });
    size_t total = 0;
    for (size_t k = 0; k < blks.size(); k++) {
        std::vector<std::pair<size_t, size_t>> busy;           // [offset, end) of placed buffers alive at the same time
        for (size_t j = 0; j < k; j++)
            if (blks[j].b <= blks[k].d && blks[k].b <= blks[j].d) busy.push_back({blks[j].off, blks[j].off + blks[j].bytes});
        std::sort(busy.begin(), busy.end());
        size_t off = 0;
        for (auto& r : busy) { if (off + blks[k].bytes <= r.first) break; off = std::max(off, r.second); }
        blks[k].off = off;
        total = std::max(total, off + blks[k].bytes);
    }
    if (!blks.empty()) {
        void* base = nullptr;
        if (dev_alloc(g, &base, total, true)) return -1;
        for (const Blk& b : blks) { g->tensors[b.t].dptr = (char*)base + b.off; g->pooled[b.t] = 1; }
        g->pool_bytes = total;
    }
    for (size_t i = 0; i < g->tensors.size(); i++)                 // views / aliases of a shared buffer are shared too
        if (g->tensors[i].ttype != TAMD_TT_CONST && (L.view_of[i] >= 0 || L.alias_of[i] >= 0) && g->pooled[root_of((int)i)]) g->pooled[i] = 1;
    if (getenv("TAMD_DEBUG"))
        fprintf(stderr, "[tamd] activations: %.1f MB one buffer per tensor, %zu of %zu buffers share %.1f MB\n", g->unpooled_bytes / 1048576.0, blks.size(),
                own.size(), g->pool_bytes / 1048576.0);
    return 0;
}

// Resolve views / aliases (nodes are in topological order; resolve chains iteratively); then the input layout steps
static int resolve_views(tamd_graph* g, I8Layout& L)
{
    for (int pass = 0; pass < 4; pass++)
        for (size_t i = 0; i < g->tensors.size(); i++) {
            HTensor& t = g->tensors[i];
            if (L.view_of[i] >= 0) {
                HTensor& o = g->tensors[L.view_of[i]];
                t.dptr = o.dptr; t.cs = o.cs; t.c_off = o.c_off + L.view_off[i]; t.is_view = true;
            } else if (L.alias_of[i] >= 0) {
                HTensor& o = g->tensors[L.alias_of[i]];
                t.dptr = o.dptr; t.cs = o.cs; t.c_off = o.c_off; t.is_view = o.is_view;
            }
        }
    // input layout steps.  in_steps / out_steps state no accesses and are outside append_steps' check: they move a graph input / output
    // between its staging buffer and its own NHWC buffer, and neither is ever shared (plan_buffers: pinned)
    for (auto& io : g->inputs) {
        HTensor& t = g->tensors[io.tensor];
        if (t.nchw_raw) continue;
        LayoutArgs a{io.stage, t.dptr, t.n, t.c, t.h, t.w, t.cs, esize(t.dtype)};
        g->in_steps.push_back(make_step(t.name, "nchw_to_nhwc", 0, 0, [a](hipStream_t s) { return launch_nchw_to_nhwc(a, s); }, {}, {}, false));
    }
    return 0;
}

// conv -> eltwise (-> relu) fusion (ResNet: branch2c / branch1 + residual add + relu): the eltwise is
// folded into the LATER of its two producers when that one is a group-1 GEMM conv whose output feeds nothing else
static void scan_eltwise_fusion(tamd_graph* g, I8Layout& L)
{
    g->fused_away.assign(g->tensors.size(), 0);
    const char* fuse_env = getenv("TAMD_FUSE_ELTWISE");
    auto producer = [&](int t) { for (size_t i = 0; i < g->nodes.size(); i++) for (int o : g->nodes[i].out) if (o == t) return (int)i; return -1; };
    for (size_t ei = 0; ei < g->nodes.size() && !(fuse_env && atoi(fuse_env) == 0); ei++) {
        HNode& e = g->nodes[ei];
        if (e.op != TAMD_OP_ELTWISE || e.in.size() != 2 || L.fused[ei] || L.chain_at[ei]) continue;      // (a member of a byte-pure chain is taken)
        const int ty = e.p.elt.type;
        if (!eltwise_type_on_device(ty)) continue;
        HTensor& ta = g->tensors[e.in[0]];
        HTensor& tb = g->tensors[e.in[1]];
        HTensor& te = g->tensors[e.out[0]];
        if (ta.dims != tb.dims || ta.is_view || tb.is_view || te.is_view || ta.ttype == TAMD_TT_CONST || tb.ttype == TAMD_TT_CONST) continue;
        const int pa = producer(e.in[0]), pb = producer(e.in[1]);
        const int later = std::max(pa, pb), conv_in = later == pa ? 0 : 1;
        if (later < 0 || later >= (int)ei) continue;
        HNode& c = g->nodes[later];
        if (c.op != TAMD_OP_CONV || c.p.conv.group != 1 || g->tensors[c.in[0]].nchw_raw || L.has_fuse[later]) continue;
        if (!conv_i8_gemm_taps_fit(c.p.conv.kernel_h, c.p.conv.kernel_w) || count_consumers(g, e.in[conv_in]) != 1) continue;
        FusedElt fz{};
        fz.res_tensor = e.in[1 - conv_in]; fz.elt_tensor = e.out[0]; fz.out_tensor = e.out[0]; fz.type = ty;
        fz.conv_is_first = conv_in == 0; fz.relu = false;
        const int relu_node = sole_reader(g, e.out[0]);
        if (relu_node >= 0) {
            const HNode& r = g->nodes[relu_node];
            if (r.op == TAMD_OP_RELU && r.p.relu.negative_slope == 0.f && !g->tensors[r.out[0]].is_view) { fz.relu = true; fz.out_tensor = r.out[0]; }
        }
        L.fuse_at[later] = fz; L.has_fuse[later] = 1; L.fused[ei] = 1;
        g->fused_away[e.in[conv_in]] = 1;        // the conv's own int8 result only exists in registers
        if (fz.relu) { L.fused[relu_node] = 1; g->fused_away[e.out[0]] = 1; }
    }
}

// Permute(0, 2, 3, 1) and Reshape of a convolution-stack tensor: one copy into the reference's dense element order, the source read
// as flatcat_i8 kind 1 (permuted) | 2 (NCHW)
static Step dense_copy(tamd_graph* g, HNode& n, int kind, const char* kernel)
{
    HTensor& x = g->tensors[n.in[0]];
    HTensor& y = g->tensors[n.out[0]];
    FlatCatI8Args a{};
    a.nsrc = 1; a.y = (int8_t*)y.dptr; a.outer = x.n; a.out_row = x.c * x.h * x.w; a.row_begin = 0; a.row_len = a.out_row;
    a.src[0] = FlatCatI8Src{(const int8_t*)x.dptr + x.c_off, kind, a.out_row, x.c, x.h * x.w, x.cs, 0, 1.f, 1};
    return make_step(n.name, kernel, 0, 2.0 * x.elems(), [a](hipStream_t s) { return launch_flatcat_i8(a, s); }, {access_of(x)}, {access_of(y)}, false);
}

// permute_ref.c:305-343, order (0, 2, 3, 1): a byte permutation -- written only when somebody reads it
static int plan_permute(tamd_graph* g, I8Layout& L, HNode& n, std::vector<Step>* out)
{
    if (L.perm_src[n.out[0]] >= 0) g->fused_away[n.out[0]] = 1;         // its Concat reads the NHWC buffer itself
    else out->push_back(dense_copy(g, n, 1, "permute_i8"));
    return 0;
}

// reshape_ref.c:76-90 (NCHW): the same bytes under another shape
static int plan_reshape(tamd_graph* g, I8Layout& L, HNode& n, std::vector<Step>* out)
{
    if (L.alias_of[n.out[0]] >= 0) { if (L.perm_src[n.out[0]] >= 0) g->fused_away[n.out[0]] = 1; }     // dense input: a view
    else out->push_back(dense_copy(g, n, 2, "reshape_i8"));      // convolution-stack input: its NCHW element order, written once
    return 0;
}

// shapes only: evaluated here, once (graph_infer.hip priorbox_eval), quantised as priorbox_ref.c:195-210
static int plan_priorbox(tamd_graph* g, HNode& n)
{
    HTensor& x = g->tensors[n.in[0]];
    HTensor& y = g->tensors[n.out[0]];
    const HTensor& img = g->tensors[n.in[1]];
    if (y.scales.empty()) { set_error("priorbox %s: missing quant params", n.name.c_str()); return -1; }
    std::vector<float> boxes;
    std::vector<int8_t> q;
    priorbox_eval(n.p.priorbox, x.dims[2], x.dims[3], img.dims[2], img.dims[3], &boxes);
    if (boxes.size() != y.elems()) { set_error("priorbox %s: output shape mismatch", n.name.c_str()); return -1; }
    priorbox_quant_i8(boxes, y.scales[0], &q);
    HIPCHK(hipMemcpyAsync(y.dptr, q.data(), q.size(), hipMemcpyHostToDevice, g->stream));
    HIPCHK(hipStreamSynchronize(g->stream));
    y.prerun_const = true;
    return 0;
}

static int plan_flat_concat(tamd_graph* g, I8Layout& L, HNode& n, std::vector<Step>* out)
{
    HTensor& y = g->tensors[n.out[0]];
    // dense output: for every index in front of the axis each input is one contiguous run of the output's run; up to
    // kFlatCatMax inputs per launch (the six SSD heads of a Concat: one launch), each read in the reference's element order
    const int ax = n.p.concat.axis < 0 ? n.p.concat.axis + (int)y.dims.size() : n.p.concat.axis;
    if (y.scales.empty()) { set_error("concat %s: missing quant params", n.name.c_str()); return -1; }
    long outer = 1, inner = 1;
    for (int d = 0; d < ax; d++) outer *= y.dims[d];
    for (size_t d = ax + 1; d < y.dims.size(); d++) inner *= y.dims[d];
    const int out_row = (int)(y.dims[ax] * inner);
    bool all_const = true;
    for (int i : n.in) all_const &= g->tensors[i].prerun_const;
    int begin = 0;
    for (size_t k0 = 0; k0 < n.in.size(); k0 += kFlatCatMax) {
        FlatCatI8Args a{};
        a.y = (int8_t*)y.dptr; a.outer = outer; a.out_row = out_row; a.row_begin = begin;
        const char* kernel = "flatcat_i8";
        double bytes = 0;
        std::vector<Access> reads;                                     // every source as the launch actually reads it
        for (size_t k = k0; k < std::min(n.in.size(), k0 + (size_t)kFlatCatMax); k++) {
            HTensor& x = g->tensors[n.in[k]];
            if (x.dtype != y.dtype || x.scales.empty()) { set_error("concat %s: input %s: dtype / quant params", n.name.c_str(), x.name.c_str()); return -1; }
            FlatCatI8Src s{};
            s.begin = begin; s.identity = n.in.size() == 1;            // concat_kernel_ref_int8.c:47-57: a single input is copied as it is
            volatile float rs = x.scales[0] / y.scales[0];             // :70 rescale = in_scale / out_scale
            s.rescale = rs;
            if (L.perm_src[n.in[k]] >= 0) {                              // Permute(0,2,3,1) (-> Flatten) of an NHWC tensor, read in place
                HTensor& p = g->tensors[L.perm_src[n.in[k]]];
                s.x = (const int8_t*)p.dptr + p.c_off; s.kind = 1; s.C = p.c; s.HW = p.h * p.w; s.cs = p.cs; s.chunk = p.c * p.h * p.w;
                if (p.n != outer) { set_error("concat %s: a permuted input on axis %d", n.name.c_str(), ax); return -1; }
                kernel = "permute_concat_i8";
                reads.push_back(access_of(p));                          // (the NHWC tensor, not its never-written permuted form)
            } else if (L.dense[n.in[k]]) {
                s.x = (const int8_t*)x.dptr; s.kind = 0; s.chunk = (int)(x.dims[ax] * inner);
                reads.push_back(access_of(x));
            } else {                                                   // a convolution-stack tensor, read in NCHW element order
                s.x = (const int8_t*)x.dptr + x.c_off; s.kind = 2; s.C = x.c; s.HW = x.h * x.w; s.cs = x.cs;
                s.chunk = (int)((size_t)x.n * x.c * x.h * x.w / (size_t)outer);
                reads.push_back(access_of(x));
            }
            a.src[a.nsrc++] = s;
            begin += s.chunk;
            bytes += 2.0 * outer * s.chunk;
        }
        a.row_len = begin - a.row_begin;
        out->push_back(make_step(n.name, kernel, 0, bytes, [a](hipStream_t s) { return launch_flatcat_i8(a, s); }, reads, {access_of(y)}, false));
        out->back().once = all_const;
    }
    if (begin != out_row) { set_error("concat %s: the inputs do not add up to the output", n.name.c_str()); return -1; }
    y.prerun_const = all_const;
    return 0;
}

static int plan_channel_concat(tamd_graph* g, I8Layout& L, HNode& n, std::vector<Step>* out)
{
    HTensor& y = g->tensors[n.out[0]];
    int off = 0;
    for (int i : n.in) {
        HTensor& x = g->tensors[i];
        if (!(L.view_of[i] == n.out[0] && L.view_off[i] == off && x.is_view)) {
            CatCopyArgs a{};
            a.x = (const int8_t*)x.dptr + x.c_off; a.y = (int8_t*)y.dptr;
            a.pixels = (long)x.n * x.h * x.w; a.C = x.c; a.cs_in = x.cs; a.ldc = y.cs; a.c_off = y.c_off + off;
            volatile float rs = x.scales[0] / y.scales[0];      // concat_kernel_ref_int8.c:70: rescale = in_scale / out_scale
            a.rescale = rs;
            a.identity = n.in.size() == 1;                      // :47-57: a single input is copied as it is
            // writes this input's slot of the output's pixels alone: the slots beside it may be views that are read here
            out->push_back(make_step(n.name, "concat_copy_i8", 0, 2.0 * a.pixels * x.c, [a](hipStream_t s) { return launch_concat_copy_i8(a, s); }, {access_of(x)},
                                     {access_of_channels(y, off, x.c)}, false));
        }
        off += x.c;
    }
    return 0;
}

// stem: first-layer convolution whose only consumer is a MAX pool 3x3 / 2 -> one launch, the conv map stays in LDS
// (conv_first_pool.hip).  1: *fused is that launch, 0: the pair stays two launches
static int fuse_stem(tamd_graph* g, HNode& conv, HNode& pool, const Planned& c, const Planned& p, Step* fused)
{
    if (c.kind != Planned::FIRST || !conv_first_pool_applicable(c.first, p.pool)) return 0;
    const FirstPoolArgs fa = conv_first_pool_args(c.first, p.pool);
    *fused = fused_step({&c, &p}, "conv_first_pool_i8", [fa](hipStream_t s) { return launch_conv_first_pool(fa, s); }, g->tensors[conv.in[0]], g->tensors[pool.out[0]], true);
    g->fused_away[conv.out[0]] = 1;
    return 1;
}

// depthwise 3x3 whose only consumer is a pointwise conv (large batches): one launch, the depthwise map stays in LDS (dwpw.hip).
// The node dwi has just been planned as `pd`; where that is a depthwise 3x3 launch this plans its pointwise consumer as a trial and
// lets plan_dwpw turn the two into one.  1: *fused is that launch (the consumer is marked), 0: the depthwise launch stands alone, the
// trial is dropped and the consumer goes through the ordinary path at its own node (its weights are uploaded again there: known, and
// kept, because keeping the trial would move every later buffer), -1: error
static int try_dwpw(tamd_graph* g, I8Layout& L, size_t dwi, const Planned& pd, Step* fused)
{
    HNode& d = g->nodes[dwi];
    const HTensor& dy = g->tensors[d.out[0]];
    const char* dp_env = getenv("TAMD_FUSE_DWPW");
    if ((dp_env && atoi(dp_env) == 0) || pd.kind != Planned::DW3X3 || d.p.conv.stride_h != 1 || dy.is_view) return 0;
    if ((long)dy.n * dy.h * dy.w < 4096 && !(dp_env && atoi(dp_env) == 2)) return 0;
    const int pw_node = sole_reader(g, d.out[0]);
    if (pw_node < 0 || g->nodes[pw_node].op != TAMD_OP_CONV || g->nodes[pw_node].in.size() < 2 || L.fused[pw_node] || L.has_fuse[pw_node]) return 0;
    // what dwpw_applicable will ask of the shapes, before the consumer is planned (and its weights uploaded) for nothing
    const tamd_conv_param& q = g->nodes[pw_node].p.conv;
    if (q.group != 1 || q.kernel_h != 1 || q.kernel_w != 1) return 0;
    if (!dwpw_pw_shape_ok(g->tensors[g->nodes[pw_node].out[0]].c, dy.w, q.kernel_h, q.kernel_w, q.stride_h, q.stride_w, q.pad_h0 || q.pad_w0 || q.pad_h1 || q.pad_w1)) return 0;
    Planned pc;
    if (plan_conv(g, g->nodes[pw_node], false, nullptr, &pc)) return -1;
    const int r = plan_dwpw(g, d, g->nodes[pw_node], pd, pc, fused);
    if (r == 1) L.fused[pw_node] = 1;
    return r;
}

// identity bottleneck block (opt-in, TAMD_FUSE_BLOCK=1): node ni is a convolution whose output feeds exactly one convolution, whose
// output feeds exactly one convolution that carries an eltwise SUM tail (scan_eltwise_fusion) with ni's INPUT as the other operand;
// neither intermediate is a view or a graph output (count_consumers counts those).  The three are planned here, the later two ahead
// of their node order (each reads only what is written by then), and either become one launch (plan_block) or are pushed as
// planned.  1: handed back in *out, 0: not such a block (nothing planned), -1: error.
// Where the block fuses, plan_conv has uploaded each convolution's GEMM-family weight panel and run its plan-time race although only
// its bias and requantisation vectors are read by the fused launch: dead device memory (res2: 3 x 68 KB), prerun time, and possibly
// plan-cache entries for launches that never run -- try_dwpw's known waste, kept for the same reason (one plan_conv, no second path
// that folds a requantisation).  The switch and the match on the eltwise tail are tested here only; plan_block takes what it is given.
static int try_block(tamd_graph* g, I8Layout& L, size_t ni, std::vector<Step>* out)
{
    if (!fuse_block_enabled()) return 0;
    HNode& na = g->nodes[ni];
    if (L.has_fuse[ni] || na.in.size() < 2 || g->tensors[na.in[0]].nchw_raw) return 0;
    auto sole_conv_behind = [&](int tensor) {
        const int nj = g->tensors[tensor].is_view ? -1 : sole_reader(g, tensor);
        return nj >= 0 && g->nodes[nj].op == TAMD_OP_CONV && g->nodes[nj].in.size() >= 2 && !L.fused[nj] ? nj : -1;
    };
    const int ib = sole_conv_behind(na.out[0]);
    if (ib < 0 || L.has_fuse[ib]) return 0;
    const int ic = sole_conv_behind(g->nodes[ib].out[0]);
    if (ic < 0 || !L.has_fuse[ic] || L.fuse_at[ic].res_tensor != na.in[0] || L.fuse_at[ic].type != 2) return 0;
    // what block_applicable will ask of the nodes' own shapes, before three convolutions are planned ahead of their order for nothing
    auto shape_ok = [](const tamd_conv_param& q, int k) {
        return q.group == 1 && block_conv_shape_ok(k, q.kernel_h, q.kernel_w, q.stride_h, q.stride_w, q.dilation_h, q.dilation_w, q.pad_h0, q.pad_h1, q.pad_w0, q.pad_w1);
    };
    if (!shape_ok(na.p.conv, 1) || !shape_ok(g->nodes[ib].p.conv, 3) || !shape_ok(g->nodes[ic].p.conv, 1)) return 0;      // (the pairings below keep the rest)
    if (!block_channels_ok(g->tensors[na.in[0]].c, g->tensors[na.out[0]].c, g->tensors[g->nodes[ic].out[0]].c)) return 0;
    Planned a, b, c;
    if (plan_conv(g, na, false, nullptr, &a) || plan_conv(g, g->nodes[ib], false, nullptr, &b) || plan_conv(g, g->nodes[ic], false, &L.fuse_at[ic], &c)) return -1;
    L.fused[ib] = 1; L.fused[ic] = 1;
    Step st;
    const int took = plan_block(g, na, g->nodes[ib], g->nodes[ic], L.fuse_at[ic], a, b, c, &st);
    if (took < 0) return -1;
    if (took) out->push_back(st);
    else out->insert(out->end(), {a.step, b.step, c.step});
    return 1;
}

// A convolution node and its fusions: the bottleneck block (opt-in), then the three pairings conv + pool (stem), pointwise + its tail
// (pwdw; two adjacent ones as a chain of four: chain4), depthwise + pointwise (dwpw).  Each plans the launches involved as values and hands back either the fused launch or the
// planned ones.
static int plan_conv_node(tamd_graph* g, I8Layout& L, size_t ni, std::vector<Step>* out)
{
    HNode& n = g->nodes[ni];
    Step st;
    const int blk = try_block(g, L, ni, out);
    if (blk) return blk < 0 ? -1 : 0;
    // stem (TAMD_FIRST_POOL=0: two launches, for A/B runs and the fused == unfused tests)
    if (!L.has_fuse[ni] && g->tensors[n.in[0]].nchw_raw) {
        const int pool_node = sole_reader(g, n.out[0]);
        const char* fp_env = tamd_pin("first_pool");
        if (pool_node >= 0 && g->nodes[pool_node].op == TAMD_OP_POOL && !L.fused[pool_node] && !(fp_env && atoi(fp_env) == 0)) {
            Planned c, p;
            if (plan_conv(g, n, false, nullptr, &c)) return -1;
            if (plan_pool(g, g->nodes[pool_node], &p)) return -1;
            L.fused[pool_node] = 1;
            if (fuse_stem(g, n, g->nodes[pool_node], c, p, &st)) out->push_back(st);
            else out->insert(out->end(), {c.step, p.step});
            return 0;
        }
    }
    int tmode = -1, prod = 0;
    const int tail = L.has_fuse[ni] ? -1 : find_pwdw_tail(g, ni, &tmode, &prod);
    if (tail >= 0 && !L.fused[tail]) {
        // the pair is planned here, the tail ahead of its node order (its only input is this conv's output), then
        // possibly replaced by ONE fused launch
        Planned a, b;
        if (plan_conv(g, n, false, nullptr, &a)) return -1;
        if (tmode == 0 ? plan_pool(g, g->nodes[tail], &b) : plan_conv(g, g->nodes[tail], false, nullptr, &b)) return -1;
        L.fused[tail] = 1;
        // Two adjacent pairs -- this one and the pointwise + depthwise behind it -- as ONE launch where the four nodes fit chain4.hip and
        // the switches / the default rule (batch 1) want it: the second pair is planned here as well, ahead of its node order.  Where
        // no tile configuration fits, this pair goes on as before and the second pair is planned again at its own node (try_dwpw's known
        // waste).  The chain's launch runs HERE and writes the second depthwise's output while it reads this conv's input: safe only
        // because plan_buffers starts that output's lifetime three hops up for this node shape (dw <- 1x1 <- dw <- this conv); a change to
        // that rule or to this look-ahead that lets the two share memory fails prerun (plan_i8: step_writes_what_it_reads)
        int pw2 = -1, dw2 = -1;
        if (tmode == 1 && find_chain4(g, ni, tail, prod, L.fused, L.has_fuse, &pw2, &dw2)) {
            Planned c, d;
            if (plan_conv(g, g->nodes[pw2], false, nullptr, &c) || plan_conv(g, g->nodes[dw2], false, nullptr, &d)) return -1;
            const int chained = plan_chain4(g, n, g->nodes[tail], g->nodes[pw2], g->nodes[dw2], prod, a, b, c, d, &st);
            if (chained < 0) return -1;
            if (chained) { L.fused[pw2] = 1; L.fused[dw2] = 1; out->push_back(st); return 0; }
        }
        // Where the depthwise tail can go together with ITS consumer (dwpw.hip: batched 14x14-class maps, stride 1), that pairing is
        // tried FIRST.  In a chain pw, dw, pw, dw, .. either pairing covers every layer once per period, and in a pass dwpw is the
        // cheaper period (MobileNet-v1 b64: 16.4 us against 22.9 us for the pwdw pair with two slices per block) -- but the
        // plan-time race, which times a launch back to back with itself, saw the pwdw pair at < 18.8 us and took it
        // (profiles/r05_layers_mobilenet_v1_int8_b64.txt, the evidence plan: the 14x14 block 120 us; with this order 95 us)
        int took = tmode == 1 ? try_dwpw(g, L, (size_t)tail, b, &st) : 0;
        if (took < 0) return -1;
        if (took) { out->insert(out->end(), {a.step, st}); return 0; }
        took = plan_pwdw(g, n, g->nodes[tail], tmode, prod, a, b, &st);
        if (took < 0) return -1;
        if (took) out->push_back(st);
        else out->insert(out->end(), {a.step, b.step});
        return 0;
    }
    Planned c;
    if (plan_conv(g, n, false, L.has_fuse[ni] ? &L.fuse_at[ni] : nullptr, &c)) return -1;
    const int took = try_dwpw(g, L, ni, c, &st);        // (anything but a depthwise 3x3 launch: 0)
    if (took < 0) return -1;
    out->push_back(took ? st : c.step);
    return 0;
}

// ResNet-50's prob; softmax_kernel_ref_int8.c over the channel axis
static int plan_softmax(tamd_graph* g, I8Layout& L, HNode& n, std::vector<Step>* out)
{
    HTensor& x = g->tensors[n.in[0]];
    HTensor& y = g->tensors[n.out[0]];
    int ax = n.p.softmax.axis < 0 ? n.p.softmax.axis + (int)x.dims.size() : n.p.softmax.axis;
    if (x.scales.empty() || y.scales.empty()) { set_error("softmax %s: missing quant params", n.name.c_str()); return -1; }
    const bool general = L.dense[n.in[0]] || (x.dims.size() == 4 && (ax == 2 || ax == 3));
    if (general) {
        // any axis of a dense tensor (the SSD tail: Reshape -> Softmax(axis 2) on [N, priors, classes]) and the spatial
        // axes of an NHWC tensor -- the same kernel with strided addressing (kernels.h: SoftmaxI8Args)
        if (ax < 0 || ax >= (int)x.dims.size() || !softmax_i8_axis_fits(x.dims[ax])) {
            set_error("softmax %s: axis %d of at most %d values", n.name.c_str(), ax, kSoftmaxI8MaxC);
            return -1;
        }
        SoftmaxI8Args a{};
        a.x = (const int8_t*)x.dptr + x.c_off; a.y = (int8_t*)y.dptr + y.c_off;
        a.C = x.dims[ax]; a.in_scale = x.scales[0]; a.out_scale = y.scales[0];
        if (L.dense[n.in[0]]) {
            long outer = 1, inner = 1;
            for (int d = 0; d < ax; d++) outer *= x.dims[d];
            for (size_t d = ax + 1; d < x.dims.size(); d++) inner *= x.dims[d];
            a.positions = outer * inner; a.d1 = a.d2 = inner; a.is1 = a.os1 = (long)a.C * inner; a.is2 = a.os2 = 0; a.istride = a.ostride = inner;
        } else if (ax == 3) {
            a.positions = (long)x.n * x.h * x.c; a.d1 = a.d2 = x.c;
            a.is1 = (long)x.w * x.cs; a.os1 = (long)y.w * y.cs; a.is2 = a.os2 = 0; a.istride = x.cs; a.ostride = y.cs;
        } else {
            a.positions = (long)x.n * x.w * x.c; a.d1 = (long)x.w * x.c; a.d2 = x.c;
            a.is1 = (long)x.h * x.w * x.cs; a.os1 = (long)y.h * y.w * y.cs; a.is2 = x.cs; a.os2 = y.cs;
            a.istride = (long)x.w * x.cs; a.ostride = (long)y.w * y.cs;
        }
        out->push_back(make_step(n.name, "softmax_i8", 0, 2.0 * (double)x.elems(), [a](hipStream_t s) { return launch_softmax_i8(a, s); }, {access_of(x)}, {access_of(y)}, false));
        return 0;
    }
    if (ax != 1 || (x.dims.size() != 2 && x.dims.size() != 4) || !softmax_i8_axis_fits(x.c)) {
        set_error("softmax %s is not supported on the device: int8 softmax runs over the channel axis of a 2-D / 4-D tensor of at most %d channels",
                  n.name.c_str(), kSoftmaxI8MaxC);
        return -1;
    }
    if (x.dims.size() == 2 && x.h * x.w != 1) {
        // a 2-D tensor that is the flattened view of an H x W > 1 map keeps the map's NHWC geometry on the device: its "channel
        // axis" is C, the reference normalises over all C*H*W values in NCHW order.  The plugin leaves such a node to
        // the CPU device (hip_device.cc: node_runs_on_device); through the C ABI it is refused here
        set_error("softmax %s is not supported on the device: its 2-D input is the flattened view of a %d x %d map", n.name.c_str(), x.h, x.w);
        return -1;
    }
    SoftmaxI8Args a{};
    a.x = (const int8_t*)x.dptr + x.c_off; a.y = (int8_t*)y.dptr + y.c_off;
    a.positions = (long)x.n * x.h * x.w; a.C = x.c; a.cs_in = x.cs; a.cs_out = y.cs;
    a.in_scale = x.scales[0]; a.out_scale = y.scales[0];
    out->push_back(make_step(n.name, "softmax_i8", 0, 2.0 * a.positions * x.c, [a](hipStream_t s) { return launch_softmax_i8(a, s); }, {access_of(x)}, {access_of(y)}, false));
    return 0;
}

// ReLU (slope >= 0) whose only consumer is a MAX pool (YOLOv3-tiny: five of its eleven leaky ReLUs; leaky4 has a second reader): one launch, relu_pool_i8
// (misc_kernels.hip: the ReLU's byte map is non-decreasing, so it commutes with the max).  The pool is planned here, ahead of its
// node, and its launch reads the ReLU's input; the ReLU's own output is never written.  A negative slope is not monotone, an average
// pool does not commute, the global form has its own kernel: those stay two launches.  TAMD_PIN=relu_pool=0: two launches (A/B runs
// and the fused == unfused tests).  1: handed back in *out, 0: not such a pair, -1: error
// The pool may sit anywhere behind the ReLU in node order: its output is then written at the RELU's position, while the ReLU's input is
// still being read.  That is safe only because plan_buffers starts a buffer's lifetime at the earliest producer within TWO hops above the
// node that produces it (pool <- relu <- the ReLU's producer), so the pool's output can never share memory with the ReLU's input; a change
// to that rule or to this look-ahead that lets the two share memory fails prerun: the step carries what it reads and writes, and plan_i8
// checks it (step_writes_what_it_reads).  The ReLU's never-written output still owns its (shared) buffer.
static int try_relu_pool(tamd_graph* g, I8Layout& L, size_t ni, std::vector<Step>* out)
{
    HNode& n = g->nodes[ni];
    HTensor& x = g->tensors[n.in[0]];
    HTensor& y = g->tensors[n.out[0]];
    if (!tamd_pin_int("relu_pool", 1) || !(n.p.relu.negative_slope >= 0.f) || x.is_view || y.is_view || x.nchw_raw) return 0;
    const int pool_node = sole_reader(g, n.out[0]);              // (a graph output counts as a consumer)
    if (pool_node < 0 || g->nodes[pool_node].op != TAMD_OP_POOL || L.fused[pool_node] || g->nodes[pool_node].p.pool.pool_method != 0) return 0;
    Planned p;
    if (plan_pool(g, g->nodes[pool_node], &p)) return -1;
    if (pool_is_global(p.pool)) return 0;                        // (plan_pool uploads nothing: the trial costs nothing)
    ReluPoolArgs a{};
    a.p = p.pool;
    a.p.x = (const int8_t*)x.dptr; a.p.cs_in = x.cs;
    a.slope = n.p.relu.negative_slope; a.relu_in_scale = x.scales[0];
    out->push_back(make_step(n.name + "+" + g->nodes[pool_node].name, "relu_pool_i8", 0, p.step.bytes, [a](hipStream_t s) { return launch_relu_pool(a, s); }, {access_of(x)},
                             {access_of(g->tensors[g->nodes[pool_node].out[0]])}, false));
    L.fused[pool_node] = 1;
    g->fused_away[n.out[0]] = 1;
    return 1;
}

static int plan_relu(tamd_graph* g, I8Layout& L, size_t ni, std::vector<Step>* out)
{
    HNode& n = g->nodes[ni];
    HTensor& x = g->tensors[n.in[0]];
    HTensor& y = g->tensors[n.out[0]];
    const int took = try_relu_pool(g, L, ni, out);
    if (took) return took < 0 ? -1 : 0;
    if (x.is_view || y.is_view) { set_error("relu %s on a concat view is not supported", n.name.c_str()); return -1; }
    ReluArgs a{(const int8_t*)x.dptr, (int8_t*)y.dptr, (size_t)x.n * x.h * x.w * x.cs, n.p.relu.negative_slope, x.scales[0], y.scales[0]};
    out->push_back(make_step(n.name, "relu_i8", 0, 2.0 * x.n * x.h * x.w * x.c, [a](hipStream_t s) { return launch_relu(a, s); }, {access_of(x)}, {access_of(y)}, false));
    return 0;
}

// upsample_ref.c:74-130 on the int8 bytes (misc_kernels.hip: upsample_i8); reads a channel slice, writes one (a concat view)
static int plan_upsample(tamd_graph* g, I8Layout& L, HNode& n, std::vector<Step>* out)
{
    HTensor& x = g->tensors[n.in[0]];
    HTensor& y = g->tensors[n.out[0]];
    const int sc = (int)n.p.ups.scale;
    if (x.dims.size() != 4 || !upsample_factor_on_device(n.p.ups.scale)) { set_error("upsample %s: only an integer factor of a 4-D tensor runs on the device", n.name.c_str()); return -1; }
    if (x.scales.empty() || y.scales.empty()) { set_error("upsample %s: missing quant params", n.name.c_str()); return -1; }
    if (y.n != x.n || y.c != x.c || y.h != x.h * sc || y.w != x.w * sc) { set_error("upsample %s: output shape mismatch", n.name.c_str()); return -1; }
    // whole 16-byte vectors: up to the padding channels of its own buffers, never into a neighbour's slice (a view has c % 16 == 0)
    const int cv = rup(x.c, 16);
    if (x.cs % 16 || y.cs % 16 || x.c_off % 16 || y.c_off % 16 || x.c_off + cv > x.cs || y.c_off + cv > y.cs) {
        set_error("upsample %s: channel slice not 16-byte aligned", n.name.c_str());
        return -1;
    }
    UpsampleI8Args a{};
    a.x = (const int8_t*)x.dptr + x.c_off; a.y = (int8_t*)y.dptr;
    a.N = x.n; a.H = x.h; a.W = x.w; a.C = x.c; a.cs_in = x.cs; a.scale = sc; a.ldc = y.cs; a.c_off = y.c_off;
    a.in_scale = x.scales[0]; a.out_scale = y.scales[0];
    a.in_zp = x.zps.empty() ? 0 : x.zps[0]; a.out_zp = y.zps.empty() ? 0 : y.zps[0];
    a.copy = a.in_scale == a.out_scale && a.in_zp == a.out_zp;
    // written in place of a Concat's copy: that copy turns -128 into 127 when the Concat has several inputs (a single input is copied
    // byte for byte, concat_kernel_ref_int8.c:47-57), so the launch does.  plan_concat_views makes such an output a view only where the
    // Concat is its one reader: anyone else reads the Upsample's own bytes, -128 included.
    a.fix128 = L.in_multi_cat[n.out[0]] ? 1 : 0;
    out->push_back(make_step(n.name, "upsample_i8", 0, (double)x.n * x.h * x.w * x.c + (double)y.n * y.h * y.w * y.c, [a](hipStream_t s) { return launch_upsample_i8(a, s); },
                             {access_of(x)}, {access_of(y)}, false));
    return 0;
}

// the scalar and unary forms: one lut_u8 launch by table (plan_eltwise_table); the same-shape form: eltwise_i8 (+ the ReLU behind it); the channel-gate form x (N, C, H, W) op gate (N, C, 1, 1): plan_chan_gate, with the
// byte map in front of the gate where match_gate_lut took it.  The ReLU-behind-Eltwise fusion is not extended to the gate form
static int plan_eltwise(tamd_graph* g, I8Layout& L, size_t ni, std::vector<Step>* out)
{
    HNode& n = g->nodes[ni];
    int gated = -1;
    const char* why = eltwise_refusal_of(g, n, &gated);
    if (why) { set_error("eltwise %s: %s", n.name.c_str(), why); return -1; }
    if (gated == kEltScalar || gated == kEltUnary) return plan_eltwise_table(g, n, out);
    if (gated >= 0) return plan_chan_gate(g, n, gated, L.gate_lut[ni] - 1, out);
    HTensor& xa = g->tensors[n.in[0]];
    HTensor& xb = g->tensors[n.in[1]];
    HTensor* y = &g->tensors[n.out[0]];
    if (xa.is_view || xb.is_view || y->is_view || xa.dims != xb.dims) { set_error("eltwise %s: views / broadcast not supported", n.name.c_str()); return -1; }
    EltArgs a{};
    a.a = (const int8_t*)xa.dptr; a.b = (const int8_t*)xb.dptr; a.count = (size_t)xa.n * xa.h * xa.w * xa.cs;
    a.type = n.p.elt.type; a.sa = xa.scales[0]; a.sb = xb.scales[0]; a.out_scale = y->scales[0];
    if (!eltwise_type_on_device(a.type)) { set_error("eltwise %s: type %d unsupported", n.name.c_str(), a.type); return -1; }
    std::string kname = "eltwise_i8";
    double bytes = 3.0 * xa.n * xa.h * xa.w * xa.c;
    // fuse the standalone ReLU that follows (ResNet: 16 x eltwise -> relu), SURVEY §8f-1
    const int nj = sole_reader(g, n.out[0]);
    if (nj >= 0 && g->nodes[nj].op == TAMD_OP_RELU && g->nodes[nj].p.relu.negative_slope == 0.f && !g->tensors[g->nodes[nj].out[0]].is_view) {
        HTensor& ry = g->tensors[g->nodes[nj].out[0]];
        a.fuse_relu = ry.scales[0] == a.out_scale ? 2 : 1; a.relu_out_scale = ry.scales[0];
        y = &ry; L.fused[nj] = 1; kname = "eltwise_relu_i8";
        g->fused_away[n.out[0]] = 1;
    }
    a.y = (int8_t*)y->dptr;
    out->push_back(make_step(n.name, kname, 0, bytes, [a](hipStream_t s) { return launch_eltwise(a, s); }, {access_of(xa), access_of(xb)}, {access_of(*y)}, false));
    return 0;
}

// outputs: NHWC -> the reference's NCHW order
static int plan_outputs(tamd_graph* g)
{
    for (auto& io : g->outputs) {
        HTensor& t = g->tensors[io.tensor];
        io.bytes = t.elems() * esize(t.dtype);
        if (t.nchw_raw) { io.stage = t.dptr; continue; }                 // dense tensors are the reference's element order already
        if (t.h * t.w == 1 && t.cs == t.c && t.c_off == 0) { io.stage = t.dptr; continue; }
        if (dev_alloc(g, &io.stage, io.bytes, true)) return -1;
        LayoutArgs a{(const int8_t*)t.dptr + t.c_off, io.stage, t.n, t.c, t.h, t.w, t.cs, esize(t.dtype)};
        g->out_steps.push_back(make_step(t.name, "nhwc_to_nchw", 0, 0, [a](hipStream_t s) { return launch_nhwc_to_nchw(a, s); }, {}, {}, false));     // (no accesses: resolve_views)
    }
    return 0;
}

// node list -> launch list: the layout passes in order, then one planner per node.  A node function hands its launches back in `out`
// (none for a node that is a view, runs inside another node's launch or -- PriorBox -- is evaluated here) and pushes nothing itself;
// append_steps (graph_plan_common.hip) checks what each says it reads and writes
int plan_i8(tamd_graph* g)
{
    for (auto& t : g->tensors) if (t.ttype != TAMD_TT_CONST) nhwc_geom(t);
    I8Layout L(g->tensors.size(), g->nodes.size());
    if (plan_dense(g, L)) return -1;
    match_cat_shuffle(g, L);
    plan_split_views(g, L);
    if (plan_concat_views(g, L)) return -1;
    match_gate_lut(g, L);                    // (behind every pass that makes a tensor a view, in front of the one that shares buffers)
    match_bytemap_chains(g, L);              // (the same place, and behind match_gate_lut: a byte map inside its gate's launch is no member)
    if (plan_input_staging(g) || plan_buffers(g, L) || resolve_views(g, L)) return -1;
    scan_eltwise_fusion(g, L);
    for (size_t ni = 0; ni < g->nodes.size(); ni++) {
        HNode& n = g->nodes[ni];
        if (L.fused[ni]) continue;
        std::vector<Step> out;
        if (L.chain_at[ni]) {                // a byte-pure chain that ends here: one lut_u8 launch
            if (plan_bytemap_chain(g, L.chains[L.chain_at[ni] - 1], &out) || append_steps(g, out)) return -1;
            continue;
        }
        Planned one;                 // FC / pooling: a single launch as plan_conv / plan_pool hand it to the fusers
        int r = 0;
        switch (n.op) {
        case TAMD_OP_INPUT: case TAMD_OP_CONST: case TAMD_OP_DROPOUT: case TAMD_OP_FLATTEN: break;
        case TAMD_OP_PERMUTE: r = plan_permute(g, L, n, &out); break;
        case TAMD_OP_RESHAPE: r = plan_reshape(g, L, n, &out); break;
        case TAMD_OP_PRIORBOX: r = plan_priorbox(g, n); break;
        case TAMD_OP_CONCAT:
            r = L.flat_concat[ni] ? plan_flat_concat(g, L, n, &out)
                : L.cat_shuffle[ni] ? plan_cat_shuffle(g, L, n, (size_t)L.cat_shuffle[ni] - 1, &out) : plan_channel_concat(g, L, n, &out);
            break;
        case TAMD_OP_CONV: r = plan_conv_node(g, L, ni, &out); break;
        case TAMD_OP_FC: if (!(r = plan_conv(g, n, true, nullptr, &one))) out.push_back(one.step); break;
        case TAMD_OP_POOL: if (!(r = plan_pool(g, n, &one))) out.push_back(one.step); break;
        case TAMD_OP_SOFTMAX: r = plan_softmax(g, L, n, &out); break;
        case TAMD_OP_RELU: r = plan_relu(g, L, ni, &out); break;
        case TAMD_OP_UPSAMPLE: r = plan_upsample(g, L, n, &out); break;
        case TAMD_OP_DEPTHTOSPACE: r = plan_depthtospace(g, n, L.in_multi_cat[n.out[0]] != 0, &out); break;      // one d2s_i8 launch (d2s.hip)
        case TAMD_OP_ELTWISE: r = plan_eltwise(g, L, ni, &out); break;
        case TAMD_OP_SIGMOID: case TAMD_OP_CLIP: case TAMD_OP_HARDSWISH: case TAMD_OP_MISH: r = plan_lut(g, n, &out); break;
        case TAMD_OP_INTERP: r = plan_interp(g, n, &out); break;
        case TAMD_OP_RESIZE: r = plan_resize(g, n, &out); break;      // one launch: interp_nearest_i8 with Resize's operands, or resize_rep_i8 (resize.hip)
        case TAMD_OP_SPLIT: r = plan_split(g, L, n, &out); break;
        case TAMD_OP_SHUFFLECHANNEL: r = plan_shuffle(g, n, &out); break;
        case TAMD_OP_PRELU: r = plan_prelu(g, n, &out); break;
        case TAMD_OP_TRANSPOSE: r = plan_transpose(g, n, L.tview[ni] ? g->nodes[L.tview[ni] - 1].in[0] : -1, &out); break;
        default:
            set_error("op %d (%s) is not supported on the device", n.op, n.name.c_str());
            return -1;
        }
        if (r || append_steps(g, out)) return -1;
    }
    return plan_outputs(g);
}

}  // namespace tamd
