// Planner for fp32 device graphs (config #1 plumbing, parity bar 1e-4, order-free).
// Dense NCHW fp32 tensors -- the reference's own order, no layout pass at the graph edges.  group == 1 convolutions
// and FC run on the matrix cores (conv_f32_mfma.hip, LDS-DMA operand ring).  3x3 / stride 1 convolutions also have a
// Winograd F(2,3) form (winograd_f32.hip; the reference's CPU backend uses F(4,3), wino_conv_kernel_x86.c -- the same
// mathematical result): the planner times both and keeps the faster (TAMD_F32_WINOGRAD=0 never, 1 always).
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <cstring>

#include <algorithm>

#include "graph.h"

namespace tamd {

// conv (group 1) or FC (as_fc: the kernel covers the whole flattened input, no activation) as [cout] x [pixels] x [K] GEMM on the
// matrix cores: *direct is the launch
static int plan_gemm_f32(tamd_graph* g, HNode& n, const HTensor& x, const HTensor& y, bool as_fc, Step* direct)
{
    const tamd_conv_param& p = n.p.conv;                          // (read for a convolution only)
    const int N = as_fc ? x.dims[0] : x.n, C = as_fc ? (int)(x.elems() / N) : x.c, H = as_fc ? 1 : x.h, W = as_fc ? 1 : x.w;
    const int OH = as_fc ? 1 : y.h, OW = as_fc ? 1 : y.w, cout = y.c;
    const int KH = as_fc ? 1 : p.kernel_h, KW = as_fc ? 1 : p.kernel_w, SH = as_fc ? 1 : p.stride_h, SW = as_fc ? 1 : p.stride_w;
    const int PH = as_fc ? 0 : p.pad_h0, PW = as_fc ? 0 : p.pad_w0, DH = as_fc ? 1 : p.dilation_h, DW = as_fc ? 1 : p.dilation_w;
    const int act = as_fc ? -1 : p.activation, oimg = as_fc ? y.c : nchw_out_img(y), oc0 = as_fc ? 0 : y.c_off;
    HTensor& w = g->tensors[n.in[1]];
    HTensor* b = n.in.size() > 2 ? &g->tensors[n.in[2]] : nullptr;
    const int K = C * KH * KW, Kpad = rup(K, 32);
    if (w.dtype != TAMD_DT_FP32 || (size_t)cout * K * 4 != w.data.size()) { set_error("%s: fp32 weight size mismatch", n.name.c_str()); return -1; }
    if ((KH - 1) * DH > 15 || (KW - 1) * DW > 15 || (size_t)C * H * W >= (1u << 24)) { set_error("%s: kernel extent / image size outside the packed tap table", n.name.c_str()); return -1; }
    F32ConvArgs a{};
    a.N = N; a.C = C; a.H = H; a.W = W; a.OH = OH; a.OW = OW; a.cout = cout; a.K = K; a.Kpad = Kpad;
    a.SH = SH; a.SW = SW; a.PH = PH; a.PW = PW;
    a.tail_split = 0;
    const float* wsrc = (const float*)w.data.data();
    if (conv_f32_mfma_operands(g, a, KH, KW, DH, DW, [&](int co, int k) { return wsrc[(size_t)co * K + k]; })) return -1;
    if (b && b->dtype != TAMD_DT_FP32) { set_error("%s: fp32 bias expected", n.name.c_str()); return -1; }
    if (upload_bias(g, b, cout, &a.bias_f32)) return -1;
    if (!g->zero_page) { if (dev_alloc(g, &g->zero_page, 256, true)) return -1; }
    a.x = (const float*)x.dptr; a.zeros = (const float*)g->zero_page; a.out_f32 = (float*)y.dptr;
    a.out_img = oimg; a.out_c0 = oc0; a.act = act; a.out_scale = 1.f;
    *direct = make_step(n.name, conv_f32_mfma_kernel_name(a), (double)N * OH * OW * cout * K,
                        4.0 * ((double)N * C * H * W + (double)N * cout * OH * OW + (double)cout * K),
                        [a](hipStream_t s) { return launch_conv_f32_mfma(a, s); }, {access_of(x)}, {access_of(y)}, false);
    return 0;
}

// Winograd F(2,3) form of the 3x3 / stride 1 convolution whose direct form is `direct`: hands back the three Winograd launches when
// they are faster (or when TAMD_F32_WINOGRAD=1), `direct` otherwise.  U = G g G^T with G = [1 0 0; .5 .5 .5; .5 -.5 .5; 0 0 1],
// evaluated in double and rounded once.
static int plan_winograd_f32(tamd_graph* g, HNode& n, const HTensor& x, const HTensor& y, const Step& direct, std::vector<Step>* out)
{
    auto keep = [&]() { out->push_back(direct); return 0; };
    const char* env = getenv("TAMD_F32_WINOGRAD");                // read at every prerun (tests switch it)
    const int mode = env ? atoi(env) : -1;
    const tamd_conv_param& p = n.p.conv;
    if (mode == 0 || p.group != 1 || p.kernel_h != 3 || p.kernel_w != 3 || p.stride_h != 1 || p.stride_w != 1 || p.dilation_h != 1
        || p.dilation_w != 1) return keep();
    HTensor& w = g->tensors[n.in[1]];
    HTensor* b = n.in.size() > 2 ? &g->tensors[n.in[2]] : nullptr;
    F32WinoArgs a{};
    a.N = x.n; a.C = x.c; a.H = x.h; a.W = x.w; a.OH = y.h; a.OW = y.w; a.cout = y.c; a.PH = p.pad_h0; a.PW = p.pad_w0;
    a.TH = (y.h + 1) / 2; a.TW = (y.w + 1) / 2; a.T = x.n * a.TH * a.TW; a.Tpad = rup(a.T, 64);
    a.Cpad = rup(x.c, 16); a.Mpad = rup(y.c, 64);
    a.out_img = nchw_out_img(y); a.out_c0 = y.c_off; a.act = p.activation;
    const size_t ws_bytes = 16ull * ((size_t)a.Cpad + a.Mpad) * a.Tpad * 4;
    if (ws_bytes > (1ull << 30)) return keep();                        // transformed tensors of this layer would not be "small"
    // only worth timing when the multiplications matter at all (the plan-time decision is by measurement anyway)
    if (mode != 1 && (double)a.T * y.c * x.c < 2e6) return keep();
    static const double G[4][3] = {{1, 0, 0}, {0.5, 0.5, 0.5}, {0.5, -0.5, 0.5}, {0, 0, 1}};
    const float* wsrc = (const float*)w.data.data();
    std::vector<float> U((size_t)16 * a.Mpad * a.Cpad, 0.f);
    for (int co = 0; co < y.c; co++)
        for (int c = 0; c < x.c; c++) {
            const float* gk = wsrc + ((size_t)co * x.c + c) * 9;
            double t[4][3];
            for (int i = 0; i < 4; i++)
                for (int j = 0; j < 3; j++) t[i][j] = G[i][0] * gk[j] + G[i][1] * gk[3 + j] + G[i][2] * gk[6 + j];
            for (int i = 0; i < 4; i++)
                for (int j = 0; j < 4; j++)
                    U[((size_t)(4 * i + j) * a.Mpad + co) * a.Cpad + c] = (float)(t[i][0] * G[j][0] + t[i][1] * G[j][1] + t[i][2] * G[j][2]);
        }
    // transformed weights, bias and the V / M workspaces (up to 1 GiB per layer) belong to the graph only if Winograd WINS the
    // timing below: plain allocations until then, freed when the direct convolution is kept (they used to stay in dev_allocs --
    // hundreds of MB of dead HBM per batched fp32 network)
    float* dU = nullptr; float* db = nullptr;
    void* dV = nullptr; void* dM = nullptr;
    std::vector<void*> mine;
    auto drop = [&]() { for (void* q : mine) (void)hipFree(q); mine.clear(); };
    auto grab = [&](void** q, size_t bytes) -> int {
        if (hipMalloc(q, bytes + 1024) != hipSuccess) { (void)hipGetLastError(); set_error("winograd workspace: out of device memory"); drop(); return -1; }
        mine.push_back(*q);
        return 0;
    };
    if (grab((void**)&dU, U.size() * 4)) return -1;
    if (hipMemcpy(dU, U.data(), U.size() * 4, hipMemcpyHostToDevice) != hipSuccess) { drop(); set_error("winograd weight upload failed"); return -1; }
    if (b) {
        if (grab((void**)&db, (size_t)y.c * 4) || hipMemcpy(db, b->data.data(), (size_t)y.c * 4, hipMemcpyHostToDevice) != hipSuccess) { drop(); return -1; }
    }
    const size_t v_bytes = 16ull * a.Cpad * a.Tpad * 4, m_bytes = 16ull * a.Mpad * a.Tpad * 4;
    if (grab(&dV, v_bytes) || grab(&dM, m_bytes)) return -1;
    a.x = (const float*)x.dptr; a.U = dU; a.bias = db; a.V = (float*)dV; a.M = (float*)dM; a.y = (float*)y.dptr;
    std::vector<std::function<hipError_t(hipStream_t)>> wino = {[a](hipStream_t s) { return launch_wino_in_f32(a, s); },
                                                                 [a](hipStream_t s) { return launch_wino_gemm_f32(a, s); },
                                                                 [a](hipStream_t s) { return launch_wino_out_f32(a, s); }};
    // tw = the three Winograd launches together, td = the direct launch: Winograd when 3 tw < 0.97 td.  Not cached; timed even under
    // TAMD_AUTOTUNE=0 (TAMD_F32_WINOGRAD alone governs this site)
    const RaceCand direct_c{"direct", direct.fn, direct.kernel};
    const RaceCand wino_c{"winograd", [wino](hipStream_t s) {
                              for (auto& f : wino) { const hipError_t e = f(s); if (e != hipSuccess) return e; }
                              return hipSuccess;
                          }, "winograd F(2,3)"};
    const int win = mode == 1 ? 1 : plan_race(g, n.name, {direct_c, wino_c}, "", 0.97f / 3.f, true);
    if (win < 0) { drop(); return -1; }
    const bool use = win == 1;
    if (!use) { HIPCHK(hipStreamSynchronize(g->stream)); drop(); return keep(); }
    for (void* q : mine) g->dev_allocs.push_back(q);           // from here on the graph owns them (freed by tamd_graph_destroy)
    const Access V = access_of_bytes(dV, v_bytes), M = access_of_bytes(dM, m_bytes);
    out->push_back(make_step(n.name, "wino_in_f32", 0, 0, wino[0], {access_of(x)}, {V}, false));
    out->push_back(make_step(n.name, "wino_gemm_f32<F(2,3)>", 16.0 * a.T * y.c * x.c, direct.bytes, wino[1], {V}, {M}, false));     // SURVEY 8(d) bytes of the node, once
    out->push_back(make_step(n.name, "wino_out_f32", 0, 0, wino[2], {M}, {access_of(y)}, false));
    return 0;
}

static int plan_conv_f32(tamd_graph* g, HNode& n, HTensor& x, HTensor& y, std::vector<Step>* out)
{
    Step direct;
    return plan_gemm_f32(g, n, x, y, false, &direct) || plan_winograd_f32(g, n, x, y, direct, out) ? -1 : 0;
}

static int plan_conv_grouped_f32(tamd_graph* g, HNode& n, HTensor& x, HTensor& y, std::vector<Step>* out)
{
    const tamd_conv_param& p = n.p.conv;
    HTensor& w = g->tensors[n.in[1]];
    HTensor* b = n.in.size() > 2 ? &g->tensors[n.in[2]] : nullptr;
    std::vector<float> hw((const float*)w.data.data(), (const float*)w.data.data() + w.data.size() / 4);
    float* dw = nullptr; const float* db = nullptr;
    if (upload(g, hw, &dw) || upload_bias(g, b, y.c, &db)) return -1;
    F32DirectArgs a{};
    a.x = (const float*)x.dptr; a.w = dw; a.bias = db; a.y = (float*)y.dptr;
    a.N = x.n; a.C = x.c; a.H = x.h; a.W = x.w; a.OH = y.h; a.OW = y.w; a.cout = y.c;
    a.KH = p.kernel_h; a.KW = p.kernel_w; a.SH = p.stride_h; a.SW = p.stride_w; a.PH = p.pad_h0; a.PW = p.pad_w0;
    a.DH = p.dilation_h; a.DW = p.dilation_w; a.group = p.group;
    a.out_img = nchw_out_img(y); a.out_c0 = y.c_off; a.act = p.activation;
    out->push_back(make_step(n.name, "conv_f32_direct", (double)y.elems() * (x.c / p.group) * p.kernel_h * p.kernel_w,
                             4.0 * ((double)x.elems() + (double)y.elems()), [a](hipStream_t s) { return launch_conv_f32_direct(a, s); },
                             {access_of(x)}, {access_of(y)}, false));
    return 0;
}

static int plan_fc_f32(tamd_graph* g, HNode& n, HTensor& x, HTensor& y, std::vector<Step>* out)
{
    Step st;
    if (plan_gemm_f32(g, n, x, y, true, &st)) return -1;
    out->push_back(st);
    return 0;
}

static int plan_pool_f32(HNode& n, HTensor& x, HTensor& y, std::vector<Step>* out)
{
    PoolGeom pg = pool_geom(n.p.pool, x.h, x.w);
    F32PoolArgs a{};
    a.x = (const float*)x.dptr; a.y = (float*)y.dptr;
    a.N = x.n; a.C = x.c; a.H = x.h; a.W = x.w; a.OH = y.h; a.OW = y.w;
    a.KH = pg.kh; a.KW = pg.kw; a.SH = pg.sh; a.SW = pg.sw; a.PH = pg.ph0; a.PW = pg.pw0;
    a.method = n.p.pool.pool_method; a.caffe_flavor = n.p.pool.caffe_flavor;
    out->push_back(make_step(n.name, "pool_f32", 0, 4.0 * ((double)x.elems() + (double)y.elems()), [a](hipStream_t s) { return launch_pool_f32(a, s); },
                             {access_of(x)}, {access_of(y)}, false));
    return 0;
}

static int plan_map_f32(HNode& n, HTensor& x, HTensor& y, std::vector<Step>* out)          // ReLU / leaky ReLU / ReLU6, nearest upsample
{
    F32MapArgs a{};
    a.x = (const float*)x.dptr; a.y = (float*)y.dptr;
    a.N = x.n; a.C = x.c; a.H = x.h; a.W = x.w;
    a.scale = n.op == TAMD_OP_UPSAMPLE ? (int)n.p.ups.scale : 1;
    a.out_img = nchw_out_img(y); a.out_c0 = y.c_off;
    a.slope = n.op == TAMD_OP_RELU ? n.p.relu.negative_slope : 0.f;
    const int mode = n.op == TAMD_OP_RELU ? 0 : (n.op == TAMD_OP_UPSAMPLE ? 2 : 3);
    out->push_back(make_step(n.name, mode == 2 ? "upsample_f32" : "relu_f32", 0, 4.0 * ((double)x.elems() + (double)y.elems()),
                             [a, mode](hipStream_t s) { return launch_map_f32(a, mode, s); }, {access_of(x)}, {access_of(y)}, false));
    return 0;
}

// shapes-only node: evaluated here, once (graph_infer.hip priorbox_eval); no launch at run
static int plan_priorbox_f32(tamd_graph* g, HNode& n, HTensor& x, HTensor& y)
{
    const HTensor& img = g->tensors[n.in[1]];
    std::vector<float> boxes;
    priorbox_eval(n.p.priorbox, x.dims[2], x.dims[3], img.dims[2], img.dims[3], &boxes);
    if (boxes.size() != y.elems()) { set_error("priorbox %s: output shape mismatch", n.name.c_str()); return -1; }
    HIPCHK(hipMemcpyAsync(y.dptr, boxes.data(), boxes.size() * 4, hipMemcpyHostToDevice, g->stream));
    HIPCHK(hipStreamSynchronize(g->stream));
    y.prerun_const = true;
    return 0;
}

// dense tensors: any axis is a channel concat of the [outer][dims[ax]][1][inner] view
static int plan_concat_f32(tamd_graph* g, HNode& n, HTensor& y, std::vector<Step>* out)
{
    AxisSplit sp;
    if (axis_split(y.dims, n.p.concat.axis, "concat", n.name, &sp)) return -1;
    const int ax = sp.axis, outer = sp.outer, inner = sp.inner;
    bool all_const = true;
    for (int i : n.in) all_const &= g->tensors[i].prerun_const;
    int off = 0;
    for (int i : n.in) {
        HTensor& xi = g->tensors[i];
        if (xi.is_view && xi.dptr == y.dptr) { off += xi.dims[ax]; continue; }      // written in place by its producer
        F32MapArgs a{};
        a.x = (const float*)xi.dptr; a.y = (float*)y.dptr;
        a.N = outer; a.C = xi.dims[ax]; a.H = 1; a.W = inner; a.scale = 1;
        a.out_img = y.dims[ax] * inner; a.out_c0 = off;
        // reads its source, writes ITS slot of every outer slice
        out->push_back(make_step(n.name, "concat_f32", 0, 8.0 * xi.elems(), [a](hipStream_t s) { return launch_map_f32(a, 1, s); }, {access_of(xi)},
                                 {access_of_slot(y, (size_t)y.dims[ax] * inner, (size_t)off * inner, (size_t)xi.dims[ax] * inner, 4)}, false));
        out->back().once = all_const;
        off += xi.dims[ax];
    }
    y.prerun_const = all_const;
    return 0;
}

static int plan_eltwise_f32(tamd_graph* g, HNode& n, HTensor& x, HTensor& y, std::vector<Step>* out)
{
    HTensor& xb = g->tensors[n.in[1]];
    const int type = n.p.elt.type;
    if (x.dims != xb.dims || !eltwise_type_on_device(type)) { set_error("eltwise %s: broadcast / type %d unsupported", n.name.c_str(), type); return -1; }
    const float* pa = (const float*)x.dptr; const float* pb = (const float*)xb.dptr; float* py = (float*)y.dptr;
    const size_t cnt = x.elems();
    out->push_back(make_step(n.name, "eltwise_f32", 0, 12.0 * cnt, [pa, pb, py, cnt, type](hipStream_t s) { return launch_eltwise_f32(pa, pb, py, cnt, type, s); },
                             {access_of(x), access_of(xb)}, {access_of(y)}, false));
    return 0;
}

static int plan_softmax_f32(HNode& n, HTensor& x, HTensor& y, std::vector<Step>* out)
{
    const float* px = (const float*)x.dptr; float* py = (float*)y.dptr;
    AxisSplit sp;
    if (axis_split(x.dims, n.p.softmax.axis, "softmax", n.name, &sp)) return -1;
    const int N = sp.outer, C = sp.on, inner = sp.inner;
    out->push_back(make_step(n.name, "softmax_f32", 0, 8.0 * x.elems(), [px, py, N, C, inner](hipStream_t s) { return launch_softmax_f32(px, py, N, C, inner, s); },
                             {access_of(x)}, {access_of(y)}, false));
    return 0;
}

// node list -> launch list, laid out as plan_u8: the buffer front, one function per node kind that hands back its launches, append_steps
// (every launch states what it reads and writes; none carries deps), the output tail
int plan_f32(tamd_graph* g)
{
    // concat-by-offset: a conv / relu / upsample whose only consumer is a channel concat writes in place (kernel arguments
    // out_img / out_c0)
    if (plan_nchw_buffers(g, 4, [](const HNode& pn, const HTensor&, const HTensor&) {
            return pn.op == TAMD_OP_CONV || pn.op == TAMD_OP_RELU || pn.op == TAMD_OP_RELU6 || pn.op == TAMD_OP_UPSAMPLE;
        }))
        return -1;

    for (auto& n : g->nodes) {
        if (n.op == TAMD_OP_INPUT || n.op == TAMD_OP_CONST || n.op == TAMD_OP_DROPOUT || n.op == TAMD_OP_FLATTEN || n.op == TAMD_OP_RESHAPE) continue;
        HTensor& x = g->tensors[n.in[0]];
        HTensor& y = g->tensors[n.out[0]];
        std::vector<Step> out;                             // the node's launches: the only thing that goes onto g->steps (append_steps)
        int rc = 0;
        switch (n.op) {
        case TAMD_OP_CONV: rc = n.p.conv.group == 1 ? plan_conv_f32(g, n, x, y, &out) : plan_conv_grouped_f32(g, n, x, y, &out); break;
        case TAMD_OP_FC: rc = plan_fc_f32(g, n, x, y, &out); break;
        case TAMD_OP_POOL: rc = plan_pool_f32(n, x, y, &out); break;
        case TAMD_OP_RELU: case TAMD_OP_RELU6: case TAMD_OP_UPSAMPLE: rc = plan_map_f32(n, x, y, &out); break;
        case TAMD_OP_PRIORBOX: rc = plan_priorbox_f32(g, n, x, y); break;
        case TAMD_OP_CONCAT: rc = plan_concat_f32(g, n, y, &out); break;
        case TAMD_OP_ELTWISE: rc = plan_eltwise_f32(g, n, x, y, &out); break;
        case TAMD_OP_SOFTMAX: rc = plan_softmax_f32(n, x, y, &out); break;
        default:
            set_error("op %d (%s) is not supported on the device for fp32", n.op, n.name.c_str());
            rc = -1;
        }
        if (rc || append_steps(g, out)) return -1;
    }
    return plan_nchw_outputs(g, 4);
}

}  // namespace tamd
