// What the units of the int8 planner share (graph_plan.hip, graph_plan_conv.hip, graph_plan_pairs.hip, and the int8 side of
// graph_plan_maps.hip); private.
// Planned launches are values (Planned): a fuser is handed the launches of the nodes it covers, reads the constants they folded and
// uploaded out of their kernel arguments, and builds its one launch with fused_step.  The rules every fuser shares are stated once
// here: sole_reader (the one node behind a tensor), fused_step (the step of a launch that covers several nodes).  Every step says what
// its launch reads and writes (graph.h: make_step); node functions hand their launches back and plan_i8 alone appends them (append_steps).
#pragma once
#include <initializer_list>

#include "graph_internal.h"
#include "epilogue.h"

namespace tamd {

// a1: which reference formula a convolution node's result follows (conv_mode), and its requantisation folded for the device
enum { RQ_CONV_HCL = 0, RQ_CONV_REF = 1, RQ_FC = 2 };   // A1 / A2 / A5 of SURVEY Appendix A (epilogue.h)
int conv_mode(const tamd_conv_param& p, int batch, int cin, int cout);
struct RqFold { float m1, lo, hi, out_scale; std::vector<float> m2; };
RqFold fold_requant(int mode, int act, float in_s, float out_s, const HTensor& w, int cout);
int upload_rq(tamd_graph* g, const RqFold& r, int cpad, const float** wscale, RqArgs* rq);
int upload_rq_m2(tamd_graph* g, const RqFold& r, int cpad, std::vector<float>* mf, RqArgs* rq);
bool exp_plain_kernels();
std::vector<int8_t> pack_pw_panel(const int8_t* wd, int C, int K, int nsteps);

std::vector<int8_t> pack_dw3x3(const int8_t* wd, int cin, int cw);
std::vector<int32_t> padded_bias(const int32_t* bd, int n, int padded);
// a depthwise 3x3, stride 1 or 2, no dilation: what the depthwise kernels take (dwconv.hip; pwdw.hip asks for more on top)
bool is_dw3x3(const tamd_conv_param& p, int cin, int cout);
// channels [0, limit) a launch of `cout` channels may store into y: the padding channels of its own buffer, nothing of a neighbour's slice
inline int store_limit(const HTensor& y, int cout) { return y.is_view ? cout : std::min(rup(cout, 16), y.cs - y.c_off); }

struct FusedElt {            // an eltwise (+ReLU) node folded into the epilogue of the conv that produces its later operand
    int res_tensor;          // the other eltwise operand
    int elt_tensor;          // the eltwise node's own output (its scale)
    int out_tensor;          // where the result is stored: elt_tensor, or the ReLU's output when one follows
    int type;
    bool conv_is_first, relu;
};

// What the passes of plan_i8 hand on to each other, per tensor (layout) and per node (fusion).
struct I8Layout {
    // view_of / view_off: a concat input that lives in its concat's buffer at a channel offset; alias_of: an identity op's output
    // (Dropout, Flatten, Reshape of a dense tensor); dense / perm_src / flat_concat: see plan_dense
    std::vector<int> view_of, view_off, alias_of, perm_src;
    std::vector<char> dense, flat_concat;
    // fused[node]: planned inside another node's launch (skipped at its own position); has_fuse / fuse_at[node]: the convolution
    // that takes an eltwise (+ReLU) into its epilogue
    // cat_shuffle[node]: a channel Concat that runs together with the ShuffleChannel behind it, node index cat_shuffle[node] - 1
    std::vector<char> fused, has_fuse;
    std::vector<FusedElt> fuse_at;
    std::vector<int> cat_shuffle;
    // in_multi_cat[tensor]: written in place into the buffer of a Concat with SEVERAL inputs (plan_concat_views; plan_upsample: fix128)
    std::vector<char> in_multi_cat;
    // gate_lut[node]: a channel-gate Eltwise that applies the byte map in front of its gate itself, node index gate_lut[node] - 1
    std::vector<int> gate_lut;
    // tview[node]: a Transpose that reads a convolution-stack tensor THROUGH the Reshape in front of it (plan_dense: match_transpose_view),
    // node index of that Reshape tview[node] - 1; the Reshape has no launch and its output no buffer
    std::vector<int> tview;
    // chain_at[node]: the last member of a byte-pure chain (match_bytemap_chains), which runs as one lut_u8 launch at this node's
    // position: chains[chain_at[node] - 1]; the other members are fused[]
    std::vector<int> chain_at;
    std::vector<ByteChain> chains;
    I8Layout(size_t nt, size_t nn)
        : view_of(nt, -1), view_off(nt, 0), alias_of(nt, -1), perm_src(nt, -1), dense(nt, 0), flat_concat(nn, 0), fused(nn, 0), has_fuse(nn, 0), fuse_at(nn),
          cat_shuffle(nn, 0), in_multi_cat(nt, 0), gate_lut(nn, 0), tview(nn, 0), chain_at(nn, 0) {}
};

// One planned launch, as plan_conv / plan_pool hand it out: the step, which form it took, and that form's kernel arguments for a
// fuser that folds this launch and its neighbour into one.  The caller pushes either the fused step or the planned ones.
struct Planned {
    enum Kind { FIRST, DW3X3, DIRECT, GEMM, POOL } kind = DIRECT;   // first-layer MFMA conv, depthwise 3x3, generic direct, GEMM family, pooling
    bool elt_tail = false;      // GEMM: an eltwise (+ReLU) tail is folded into the launch
    Step step;
    FirstArgs first{};          // the member of `kind` is set; DIRECT has none
    DwArgs dw{};
    ConvArgs gemm{};
    ConvArgs gemm_tail{};       // GEMM with elt_tail: the arguments as launched, tail included (`gemm` stays the bare convolution).  A second
                                // ConvArgs in every Planned for ONE reader, plan_block, which needs the tail's folded constants
    PoolArgs pool{};
};

// The node that reads `tensor` as its FIRST input, where that node is the tensor's only consumer of any kind (a second operand of another
// node and a graph output count as consumers: count_consumers); -1 otherwise.  What else a fusion asks of that node or of the tensor
// (is_view, I8Layout::fused / has_fuse) stays with the caller
inline int sole_reader(const tamd_graph* g, int tensor)
{
    if (count_consumers(g, tensor) != 1) return -1;
    for (size_t nj = 0; nj < g->nodes.size(); nj++)
        if (!g->nodes[nj].in.empty() && g->nodes[nj].in[0] == tensor) return (int)nj;
    return -1;
}

// the one launch for the planned launches `parts`: their node names joined by '+', their macs and bytes summed (SURVEY 8(d) accounting,
// per layer: the intermediate tensors still count as algorithmic bytes).  It reads x and writes y, nothing else besides constants;
// deps: as make_step
inline Step fused_step(std::initializer_list<const Planned*> parts, const std::string& kernel, std::function<hipError_t(hipStream_t)> fn, const HTensor& x,
                       const HTensor& y, bool deps)
{
    Step st = make_step("", kernel, 0, 0, std::move(fn), {access_of(x)}, {access_of(y)}, deps);
    for (const Planned* p : parts) {
        st.node += (p == *parts.begin() ? "" : "+") + p->step.node;
        st.macs += p->step.macs; st.bytes += p->step.bytes;
    }
    return st;
}

// graph_plan_conv.hip.  One convolution / FC (as_fc) / pooling node as ONE launch, handed out in *out; fz: the eltwise tail it takes
int plan_conv(tamd_graph* g, HNode& n, bool as_fc, const FusedElt* fz, Planned* out);
int plan_pool(tamd_graph* g, HNode& n, Planned* out);

// graph_plan_maps.hip.  Split, ShuffleChannel and Concat + ShuffleChannel (node sj) of an int8 graph: chan_map_i8 launches
int plan_split(tamd_graph* g, I8Layout& L, HNode& n, std::vector<Step>* out);
int plan_shuffle(tamd_graph* g, HNode& n, std::vector<Step>* out);
int plan_cat_shuffle(tamd_graph* g, I8Layout& L, HNode& cat, size_t sj, std::vector<Step>* out);

// graph_plan_pairs.hip.  The fusers: 1 = *fused is the one launch for both, 0 = not fused, -1 = error
int find_pwdw_tail(tamd_graph* g, size_t ni, int* tmode, int* prod);
int plan_pwdw(tamd_graph* g, HNode& pw, HNode& tl, int tmode, int prod, const Planned& a, const Planned& b, Step* fused);
int plan_dwpw(tamd_graph* g, HNode& dw, HNode& pw, const Planned& d, const Planned& c, Step* fused);
// two adjacent pwdw pairs -- producer conv, depthwise (stride 1), pointwise conv, depthwise -- in one launch: chain4.hip.  find_chain4: the
// pointwise conv and the depthwise behind the pair (ni, its tail `tail`) where the four nodes fit the kernel AND the switches / default rule
// want the chain; fused[nj] / has_fuse[nj]: node nj already belongs to another launch / takes an eltwise tail (I8Layout).  The chain runs
// at ni's position and writes the last depthwise's output while it reads ni's input: plan_buffers' birth rule keeps the two apart (plan_i8
// checks every step for it)
bool find_chain4(tamd_graph* g, size_t ni, int tail, int prod, const std::vector<char>& fused, const std::vector<char>& has_fuse, int* pw2, int* dw2);
int plan_chain4(tamd_graph* g, HNode& n0, HNode& d1, HNode& p2, HNode& d2, int prod, const Planned& a, const Planned& b, const Planned& c, const Planned& d, Step* fused);
// an identity bottleneck block (1x1 -> 3x3 -> 1x1 + residual [+ ReLU]) in one launch: block_i8.hip.  c carries the eltwise tail fz
bool fuse_block_enabled();
int plan_block(tamd_graph* g, HNode& na, HNode& nb, HNode& nc, const FusedElt& fz, const Planned& a, const Planned& b, const Planned& c, Step* fused);

}  // namespace tamd
