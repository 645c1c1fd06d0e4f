// int8 planner, the convolution / FC / pooling launches: requantisation folds, weight packers, and one function per form a
// convolution node can take (first-layer MFMA conv, depthwise 3x3, generic direct, GEMM family).  plan_conv opens a ConvI8,
// picks the form and calls it; every form hands back ONE Planned and pushes nothing onto g->steps.  The order of the uploads
// inside a form is behaviour: it fixes every later device address.
#include "graph_plan.h"
#include "env.h"

#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <cfloat>
#include <cmath>

namespace tamd {

// which formula the reference's score() selection lands on (conv_hcl_x86.c:351-371,
// conv_dw_hcl_x86.c:508-543, conv_ref.c:197-200)
int conv_mode(const tamd_conv_param& p, int batch, int cin, int cout)
{
    if (p.group == 1) return RQ_CONV_HCL;
    int cin_g = cin / p.group, cout_g = cout / p.group;
    if (p.kernel_h == p.kernel_w && batch == 1 && p.group > 1 && cin_g == 1 && cout_g == 1 && p.pad_h0 == p.pad_h1
        && p.pad_w0 == p.pad_w1 && p.dilation_h == 1 && p.dilation_w == 1 && p.kernel_h == 3
        && ((p.stride_h == 1 && p.stride_w == 1) || (p.stride_h == 2 && p.stride_w == 2)))
        return RQ_CONV_HCL;
    return RQ_CONV_REF;
}


// the reference's three requantisation formulas folded into (m1, m2[c], lo, hi, out_scale) -- epilogue.h.
// Host float arithmetic here is binary32, unfused (-ffp-contract=off), exactly the reference's expressions.
RqFold fold_requant(int mode, int act, float in_s, float out_s, const HTensor& w, int cout)
{
    RqFold r;
    r.m2.resize(cout);
    for (int i = 0; i < cout; i++) r.m2[i] = w.scales.size() == (size_t)cout ? w.scales[i] : w.scales[0];
    r.m1 = in_s; r.out_scale = out_s; r.lo = -FLT_MAX; r.hi = FLT_MAX;
    if (mode == RQ_CONV_HCL) {
        if (act == 0) r.lo = 0.f;
        if (act > 0) { r.lo = 0.f; r.hi = 6.f; }
    } else if (mode == RQ_CONV_REF) {
        r.m1 = 1.0f;
        for (int i = 0; i < cout; i++) { volatile float d = in_s * r.m2[i]; r.m2[i] = d; }
        if (act == 1) { r.lo = -1.f; r.hi = 1.f; }
        else if (act >= 0) { r.lo = 0.f; if (act == 6) r.hi = 6.f; }
    } else {   // RQ_FC
        r.m1 = 1.0f;
        for (int i = 0; i < cout; i++) { volatile float d = in_s * r.m2[i]; volatile float q = d / out_s; r.m2[i] = q; }
        r.out_scale = 1.0f;
    }
    return r;
}

// RqArgs of epilogue.h for one node: the reference chain's constants (the +-127.49 * out_scale saturation folded into lo / hi)
// and the fast path's window / multipliers.  Host float arithmetic here is binary32, unfused: q(lo) / q(hi) are the
// reference's own sat127(round(x / out_scale)) on the clamp bounds.  The fold is used only when every factor is an ordinary
// normal number (the error bound of epilogue.h assumes no underflow in the chain); otherwise thr = 2 hands every value to the chain.
static int host_q(float x, float s)
{
    volatile float d = x / s;
    const float r = roundf(d);
    return r > 127.f ? 127 : (r < -127.f ? -127 : (int)r);
}
static RqArgs host_rq(const RqFold& r, int cpad, std::vector<float>* mf, std::vector<float>* m2)
{
    RqArgs q{};
    volatile float lim = 127.49f * r.out_scale;
    q.m1 = r.m1; q.out_scale = r.out_scale;
    q.lo = std::max(r.lo, -(float)lim);
    q.hi = std::min(r.hi, (float)lim);
    auto ordinary = [](double v) { return std::isfinite(v) && std::fabs(v) >= 1e-30 && std::fabs(v) <= 1e30; };
    bool ok = ordinary(r.m1) && ordinary(r.out_scale) && r.out_scale > 0.f && r.m1 > 0.f && q.lo <= q.hi;
    for (float v : r.m2) ok = ok && (v == 0.f || (ordinary(v) && ordinary((double)r.m1 * v) && ordinary((double)r.m1 * v / r.out_scale)));
    mf->assign(cpad, 0.f);
    m2->assign(cpad, 1.f);
    for (size_t c = 0; c < r.m2.size() && c < (size_t)cpad; c++) {
        (*m2)[c] = r.m2[c];
        if (ok) (*mf)[c] = (float)((double)r.m1 * (double)r.m2[c] / (double)r.out_scale);
    }
    q.thr = ok ? 0x1p-13f : 2.0f;
    q.ylo = ok ? 128.f + (float)host_q(q.lo, r.out_scale) + 0.25f : 1.25f;
    q.yhi = ok ? 128.f + (float)host_q(q.hi, r.out_scale) + 0.75f : 255.75f;
    return q;
}
// The fused eltwise tail's SUM (+ scale-keeping ReLU) as the two-fma tail of epilogue.h: its constants from e's scales, when the
// tail is of that kind, `allowed`, and the error bound holds (S = mc + mr <= 2, ordinary scales); otherwise thr = 0: not applicable
static void host_elt_fold(EltFuse& e, bool allowed)
{
    const double sc = e.s_conv, sr = e.s_res, so = e.out_scale;
    auto ordinary = [](double v) { return std::isfinite(v) && v >= 1e-30 && v <= 1e30; };
    const bool ok = e.type == 2 && e.relu != 1 && ordinary(sc) && ordinary(sr) && ordinary(so) && (sc + sr) / so <= 2.0;
    e.thr = 0.f;
    if (!ok || !allowed) return;
    const float eps = 0x1p-13f;
    e.mc = (float)(sc / so); e.mr = (float)(sr / so);
    e.k0 = (float)(128.5 + (double)eps - 128.0 * ((double)e.mc + (double)e.mr));
    e.ylo = e.relu ? 128.25f : 1.25f; e.yhi = 255.75f; e.thr = 2.f * eps;
}
// timing experiments only (tools/exp/xcd_local.sh): TAMD_EXP_PLAIN_KERNELS=1 plans the ordinary (non-coherent) kernel
// instances under direct dispatch; TAMD_EXP_NOFENCE=1 strips the fences of ordinary launches AND skips the self-check -- the bytes
// of such a graph are NOT trustworthy (stale L1 lines), only its clock is looked at
bool exp_plain_kernels() { const char* e = exp_env("TAMD_EXP_PLAIN_KERNELS"); return e && atoi(e) == 1; }

// uploads both per-channel vectors; *wscale = the fast-path multipliers, rq->m2 = the chain's factors
int upload_rq(tamd_graph* g, const RqFold& r, int cpad, const float** wscale, RqArgs* rq)
{
    std::vector<float> mf, m2;
    *rq = host_rq(r, cpad, &mf, &m2);
    float *d0, *d1;
    if (upload(g, mf, &d0) || upload(g, m2, &d1)) return -1;
    *wscale = d0; rq->m2 = d1;
    return 0;
}

// as upload_rq, but the fast-path multipliers stay on the host in *mf (chain4.hip stages them into LDS together with its weights)
int upload_rq_m2(tamd_graph* g, const RqFold& r, int cpad, std::vector<float>* mf, RqArgs* rq)
{
    std::vector<float> m2;
    *rq = host_rq(r, cpad, mf, &m2);
    float* d1;
    if (upload(g, m2, &d1)) return -1;
    rq->m2 = d1;
    return 0;
}

// pointwise weight panel in MFMA fragment order: [16-channel slice][64-deep K step][lane = (k block of 16) * 16 + channel][16 B];
// `wd` = [C][K] int8 rows (1x1 conv: K = cin; first conv: K = cin*KH*KW in OIHW order), zero padded to nsteps * 64
std::vector<int8_t> pack_pw_panel(const int8_t* wd, int C, int K, int nsteps)
{
    const int slices = (C + 15) / 16;
    std::vector<int8_t> wf((size_t)slices * nsteps * 1024, 0);
    for (int c = 0; c < C; c++)
        for (int k = 0; k < K; k++)
            wf[((size_t)((c >> 4) * nsteps + (k >> 6)) * 64 + ((k >> 4) & 3) * 16 + (c & 15)) * 16 + (k & 15)] = wd[(size_t)c * K + k];
    return wf;
}

// depthwise 3x3 weights as [3 rows][cw] dwords {w[r][0], w[r][1], w[r][2], 0}: one v_dot4 operand per (row, channel)
std::vector<int8_t> pack_dw3x3(const int8_t* wd, int cin, int cw)
{
    std::vector<int8_t> wp((size_t)3 * cw * 4, 0);
    for (int c = 0; c < cin; c++)
        for (int r = 0; r < 3; r++)
            for (int kx = 0; kx < 3; kx++) wp[((size_t)r * cw + c) * 4 + kx] = wd[(size_t)c * 9 + r * 3 + kx];
    return wp;
}

// a node's int32 bias, zeros where it has none, in a vector of `padded` entries
std::vector<int32_t> padded_bias(const int32_t* bd, int n, int padded)
{
    std::vector<int32_t> bp(padded, 0);
    for (int c = 0; c < n; c++) bp[c] = bd ? bd[c] : 0;
    return bp;
}

bool is_dw3x3(const tamd_conv_param& p, int cin, int cout)
{
    return p.group > 1 && p.group == cin && cout == cin && p.kernel_h == 3 && p.kernel_w == 3 && p.dilation_h == 1 && p.dilation_w == 1
           && p.stride_h == p.stride_w && (p.stride_h == 1 || p.stride_h == 2);
}

// One convolution / FC node, built once (conv_i8_open): what the four forms below share
struct ConvI8 {
    tamd_graph* g;
    HNode& n;
    HTensor& x; HTensor& w; HTensor* b; HTensor& y;
    tamd_conv_param p{};       // the node's, or the "valid" convolution an FC is
    RqFold rq;                 // the requantisation of the node's formula (conv_mode | RQ_FC), folded
    const int8_t* wd = nullptr;
    const int32_t* bd = nullptr;       // null: no bias
    int cin = 0, cout = 0, group = 1, KH = 0, KW = 0;
    double macs = 0, bytes = 0;
};

// the checks and the constants of the node; uploads nothing
static int conv_i8_open(ConvI8& c, bool as_fc)
{
    const HNode& n = c.n;
    const HTensor &x = c.x, &w = c.w, &y = c.y;
    if (x.dtype != TAMD_DT_INT8 || w.dtype != TAMD_DT_INT8 || y.dtype != TAMD_DT_INT8) {
        set_error("conv/fc %s: only int8 is implemented on the device in this round (dtype %d)", n.name.c_str(), x.dtype);
        return -1;
    }
    if (x.scales.empty() || y.scales.empty() || w.scales.empty()) { set_error("%s: missing quant params", n.name.c_str()); return -1; }
    tamd_conv_param& p = c.p;
    int mode;
    if (as_fc) {   // FC == "valid" convolution whose kernel covers the whole input map; weight [out][c*h*w]
        p.kernel_h = x.h; p.kernel_w = x.w; p.stride_h = p.stride_w = 1; p.dilation_h = p.dilation_w = 1;
        p.group = 1; p.activation = -1; p.input_channel = x.c; p.output_channel = y.c;
        mode = RQ_FC;
        if ((size_t)w.elems() != (size_t)y.c * x.c * x.h * x.w) { set_error("fc %s: weight size mismatch", n.name.c_str()); return -1; }
    } else {
        p = n.p.conv;
        mode = conv_mode(p, c.g->formula_batch ? c.g->formula_batch : x.n, x.c, y.c);      // (a half of a pair: the whole graph's batch decides, graph.h)
    }
    c.cout = y.c; c.cin = x.c; c.group = p.group; c.KH = p.kernel_h; c.KW = p.kernel_w;
    const int cin_g = c.cin / c.group;
    c.rq = fold_requant(mode, p.activation, x.scales[0], y.scales[0], w, c.cout);
    c.wd = (const int8_t*)w.data.data(); c.bd = c.b ? (const int32_t*)c.b->data.data() : nullptr;
    c.macs = (double)y.n * y.h * y.w * c.cout * cin_g * c.KH * c.KW;
    c.bytes = (double)x.n * x.h * x.w * c.cin + (double)y.n * y.h * y.w * c.cout + (double)c.cout * cin_g * c.KH * c.KW + 4.0 * c.cout;
    return 0;
}

// which form the node takes: from the context alone, before anything is uploaded
static Planned::Kind conv_i8_form(const ConvI8& c)
{
    const tamd_conv_param& p = c.p;
    if (c.x.nchw_raw && c.group == 1 && c.cin <= 4 && c.cin * c.KH * c.KW <= 224 && c.cout <= 128
        && p.dilation_h * (c.KH - 1) < 256 && p.dilation_w * (c.KW - 1) < 256)
        return Planned::FIRST;         // from the NCHW graph input on MFMA
    if (!c.x.nchw_raw && c.group == 1) return Planned::GEMM;
    if (!c.x.nchw_raw && is_dw3x3(p, c.cin, c.cout)) return Planned::DW3X3;
    return Planned::DIRECT;            // first layer from NCHW with more channels, grouped, non-3x3 depthwise
}

// ---- first layer from the NCHW graph input on MFMA ----
static int conv_i8_first(ConvI8& c, Planned* out)
{
    const HTensor &x = c.x, &y = c.y;
    const tamd_conv_param& p = c.p;
    const int cin = c.cin, cout = c.cout, KH = c.KH, KW = c.KW;
    const char* rows_env = tamd_pin("first_rows");                   // 0: always the generic gather kernel (tests; read at every prerun)
    const int kwp = (rows_env && atoi(rows_env) == 0) ? 0 : conv_first_kwp(cin, KH, KW, p.dilation_w);
    const int kreal = cin * KH * KW, kp = kwp ? rup(cin * KH * kwp, 32) : rup(kreal, 32), cpad = rup(cout, 32);
    std::vector<int8_t> wp((size_t)cpad * kp, 0);
    for (int co = 0; co < cout; co++) {
        if (!kwp) { memcpy(&wp[(size_t)co * kp], c.wd + (size_t)co * kreal, kreal); continue; }   // OIHW row as stored
        for (int r = 0; r < cin * KH; r++)                              // kx padded to kwp: a patch row is kwp consecutive bytes
            memcpy(&wp[(size_t)co * kp + (size_t)r * kwp], c.wd + (size_t)co * kreal + (size_t)r * KW, KW);
    }
    const std::vector<int32_t> bp = padded_bias(c.bd, cout, cpad);
    FirstArgs a{};
    int8_t* dw_; int32_t* db_;
    if (upload(c.g, wp, &dw_) || upload(c.g, bp, &db_) || upload_rq(c.g, c.rq, cpad, &a.wscale, &a.rq)) return -1;
    a.x = (const int8_t*)x.dptr; a.w = dw_; a.bias = db_; a.y = (int8_t*)y.dptr;
    a.N = x.n; a.C = cin; a.H = x.h; a.W = x.w; a.OH = y.h; a.OW = y.w; a.cout = cout; a.ldc = y.cs; a.c_off = y.c_off;
    a.c_limit = store_limit(y, cout);
    a.KH = KH; a.KW = KW; a.SH = p.stride_h; a.SW = p.stride_w; a.PH = p.pad_h0; a.PW = p.pad_w0;
    a.DH = p.dilation_h; a.DW = p.dilation_w; a.kp = kp; a.kwp = kwp;
    out->step.kernel = "conv_first_i8";
    out->step.fn = [a](hipStream_t s) { return launch_conv_first(a, s); };
    out->kind = Planned::FIRST; out->first = a;
    return 0;
}

// ---- depthwise 3x3 ----
static int conv_i8_dw3x3(ConvI8& c, Planned* out)
{
    const HTensor &x = c.x, &y = c.y;
    const int cw = rup(c.cin, 16);
    const std::vector<int8_t> wp = pack_dw3x3(c.wd, c.cin, cw);
    const std::vector<int32_t> bp = padded_bias(c.bd, c.cin, cw);
    DwArgs a{};
    int8_t* dw_; int32_t* db_;
    if (upload(c.g, wp, &dw_) || upload(c.g, bp, &db_) || upload_rq(c.g, c.rq, cw, &a.wscale, &a.rq)) return -1;
    a.x = (const int8_t*)x.dptr + x.c_off; a.w = dw_; a.bias = db_;
    a.y = (int8_t*)y.dptr;
    a.N = x.n; a.H = x.h; a.W = x.w; a.C = c.cin; a.cs_in = x.cs; a.cw = cw; a.OH = y.h; a.OW = y.w;
    a.ldc = y.cs; a.c_off = y.c_off; a.S = c.p.stride_h; a.PH = c.p.pad_h0; a.PW = c.p.pad_w0;
    out->step.kernel = dwconv3x3_kernel_name(a);
    out->step.fn = [a](hipStream_t s) { return launch_dwconv3x3(a, s); };
    out->kind = Planned::DW3X3; out->dw = a;
    return 0;
}

// ---- generic direct (first layer from NCHW, grouped, non-3x3 depthwise) ----
static int conv_i8_direct(ConvI8& c, Planned* out)
{
    const HTensor &x = c.x, &y = c.y;
    const tamd_conv_param& p = c.p;
    std::vector<int8_t> wv(c.wd, c.wd + c.w.elems());
    DirectArgs a{};
    int8_t* dw_; int32_t* db_ = nullptr;
    if (upload(c.g, wv, &dw_) || upload_rq(c.g, c.rq, rup(c.cout, 4), &a.wscale, &a.rq)) return -1;
    if (c.bd) { std::vector<int32_t> bv(c.bd, c.bd + c.cout); if (upload(c.g, bv, &db_)) return -1; }
    a.x = (const int8_t*)x.dptr + (x.nchw_raw ? 0 : x.c_off); a.w = dw_; a.bias = db_;
    a.y = (int8_t*)y.dptr;
    a.N = x.n; a.C = c.cin; a.H = x.h; a.W = x.w; a.cs_in = x.nchw_raw ? 0 : x.cs;
    a.OH = y.h; a.OW = y.w; a.cout = c.cout; a.ldc = y.cs; a.c_off = y.c_off;
    a.KH = c.KH; a.KW = c.KW; a.SH = p.stride_h; a.SW = p.stride_w; a.PH = p.pad_h0; a.PW = p.pad_w0;
    a.DH = p.dilation_h; a.DW = p.dilation_w; a.group = c.group;
    out->step.kernel = "conv_direct_i8";
    out->step.fn = [a](hipStream_t s) { return launch_conv_direct(a, s); };
    out->kind = Planned::DIRECT;
    return 0;
}

// ---- implicit GEMM on MFMA: the family ----
// The node's ConvArgs and the family's weights, [cout_pad][kpad] rows of (tap, channel); *wp keeps the host copy (the conv_pgemm
// variants repack it)
static int conv_i8_gemm_args(ConvI8& c, ConvArgs* args, std::vector<int8_t>* wp)
{
    tamd_graph* g = c.g;
    const HTensor &x = c.x, &y = c.y;
    const tamd_conv_param& p = c.p;
    const int cin = c.cin, cout = c.cout, KH = c.KH, KW = c.KW;
    const int ckp = rup(cin, 16);
    const int ktot = KH * KW * ckp;
    const int kpad = rup(ktot, 64);
    const int cout_pad = rup(cout, 128);
    if (!conv_i8_gemm_taps_fit(KH, KW)) { set_error("conv %s: kernel %dx%d too large", c.n.name.c_str(), KH, KW); return -1; }
    wp->assign((size_t)cout_pad * kpad + 256, 0);      // + tail: deep-K stages may read past the last row
    for (int co = 0; co < cout; co++)
        for (int ci = 0; ci < cin; ci++)
            for (int ky = 0; ky < KH; ky++)
                for (int kx = 0; kx < KW; kx++)
                    (*wp)[(size_t)co * kpad + (size_t)(ky * KW + kx) * ckp + ci] = c.wd[(((size_t)co * cin + ci) * KH + ky) * KW + kx];
    const std::vector<int32_t> bp = padded_bias(c.bd, cout, cout_pad);
    ConvArgs& a = *args;
    int8_t* dw_; int32_t* db_;
    if (upload(g, *wp, &dw_) || upload(g, bp, &db_) || upload_rq(g, c.rq, cout_pad, &a.wscale, &a.rq)) return -1;
    a.x = (const int8_t*)x.dptr + x.c_off; a.w = dw_; a.bias = db_; a.y = (int8_t*)y.dptr;
    a.N = x.n; a.H = x.h; a.W = x.w; a.cs_in = x.cs; a.ckp = ckp; a.OH = y.h; a.OW = y.w; a.cout = cout;
    a.ldc = y.cs; a.c_off = y.c_off; a.c_limit = store_limit(y, cout);
    a.KH = KH; a.KW = KW; a.SH = p.stride_h; a.SW = p.stride_w; a.PH = p.pad_h0; a.PW = p.pad_w0;
    a.DH = p.dilation_h; a.DW = p.dilation_w; a.cin = cin; a.ktot = ktot; a.kpad = kpad;
    if (!g->zero_page) { if (dev_alloc(g, &g->zero_page, 256, true)) return -1; }
    a.zeros = (const int8_t*)g->zero_page;
    a.mg_ohw = ((1ull << 40) + (unsigned)(y.h * y.w) - 1) / (unsigned)(y.h * y.w);
    a.mg_ow = ((1ull << 40) + (unsigned)y.w - 1) / (unsigned)y.w;
    a.M = y.n * y.h * y.w;
    a.cfg = -1;
    return 0;
}

// conv -> eltwise (-> relu) in one launch: the conv's own int8 rounding is kept, see epilogue.h.  `a` then stores the TAIL's output
static void conv_i8_elt_tail(const ConvI8& c, const FusedElt& fz, ConvArgs& a, Step& st)
{
    const HTensor& r = c.g->tensors[fz.res_tensor];
    const HTensor& o = c.g->tensors[fz.out_tensor];
    a.elt.res = (const int8_t*)r.dptr; a.elt.res_ldc = r.cs; a.elt.res_c_off = r.c_off;
    a.elt.type = fz.type; a.elt.conv_is_first = fz.conv_is_first ? 1 : 0;
    a.elt.s_conv = c.y.scales[0]; a.elt.s_res = r.scales[0];
    a.elt.out_scale = c.g->tensors[fz.elt_tensor].scales[0];
    a.elt.relu = fz.relu ? (o.scales[0] == a.elt.out_scale ? 2 : 1) : 0; a.elt.relu_out_scale = o.scales[0];
    host_elt_fold(a.elt, !(tamd_pin("elt_fold") && atoi(tamd_pin("elt_fold")) == 0));
    a.y = (int8_t*)o.dptr; a.ldc = o.cs; a.c_off = o.c_off;
    a.c_limit = store_limit(o, c.cout);
    st.bytes += (double)r.n * r.h * r.w * r.c;
}

static RaceCand igemm_cand(const ConvArgs& a, int cfg)      // cfg -1: the launcher's heuristic
{
    ConvArgs ac = a;
    ac.cfg = cfg;
    return {conv_igemm_kernel_name(ac), [ac](hipStream_t s) { return launch_conv_igemm(ac, s); }};
}

// (the fused eltwise tail lives in the conv_igemm / conv_igemm2 / pw_stream epilogues)
static void gemm_fixed_cands(const ConvArgs& a, bool tail, std::vector<RaceCand>& cands)
{
    if (!tail && gemm_direct_applicable(a)) cands.push_back({"gemm_direct_i8", [a](hipStream_t s) { return launch_gemm_direct(a, s); }});
    if (pw_stream_applicable(a)) cands.push_back({"pw_stream_i8", [a](hipStream_t s) { return launch_pw_stream(a, s); }});
    if (pw_rows_applicable(a)) cands.push_back({"pw_rows_i8", [a](hipStream_t s) { return launch_pw_rows(a, s); }});
    if (conv_igemm2_applicable(a)) cands.push_back({conv_igemm2_kernel_name(a), [a](hipStream_t s) { return launch_conv_igemm2(a, s); }});
}

// lean-loop kernels (conv_pgemm.hip): fragment-ordered weights, k x k activations as an LDS-resident patch
static int gemm_pgemm_cands(ConvI8& c, const ConvArgs& a, const std::vector<int8_t>& wp, std::vector<RaceCand>& cands)
{
    int8_t* packed[2] = {nullptr, nullptr};       // per cout-tile width (64 / 128), packed on first use
    int* geom[2] = {nullptr, nullptr};            // conv_pgemm_w.hip: the per-tile geometry table, per pixel-tile height (128 / 64)
    for (int v = 0; v < conv_pgemm_num_variants(); v++) {
        if (!conv_pgemm_applicable(a, v)) continue;
        if ((v & 2) && a.M >= 65536) continue;    // 64-pixel tiles: only where 128-pixel tiles leave CUs idle
        ConvArgs ap = a;
        conv_pgemm_prepare(ap, v);
        const int bn = conv_pgemm_bn(v), slot = bn == 128;
        if (!packed[slot]) {
            std::vector<int8_t> wf(conv_pgemm_packed_bytes(ap, bn), 0);
            conv_pgemm_pack(ap, wp.data(), rup(c.cout, 128), bn, wf.data());
            if (upload(c.g, wf, &packed[slot])) return -1;
        }
        ap.wfrag = packed[slot];
        if (v & 16) {
            const int gs = (v & 2) ? 1 : 0;
            if (!geom[gs]) {
                std::vector<int> tab;
                conv_pgemm_w_table(ap, tab);
                if (upload(c.g, tab, &geom[gs])) return -1;
            }
            ap.pg_tab = geom[gs];
        }
        cands.push_back({conv_pgemm_kernel_name(ap), [ap](hipStream_t s) { return launch_conv_pgemm(ap, s); }});
    }
    return 0;
}

// small maps (batch-1 tails, 1x1-map FC): the lean 16-channel-slice kernel of pwdw.hip without a tail
static int gemm_pw_small_cands(ConvI8& c, const ConvArgs& a, std::vector<RaceCand>& cands)
{
    const HTensor& x = c.x;
    const tamd_conv_param& p = c.p;
    const int cin = c.cin, cout = c.cout, ckp = a.ckp;
    const bool is1x1 = c.KH == 1 && c.KW == 1 && p.stride_h == 1 && p.stride_w == 1 && !p.pad_h0 && !p.pad_h1 && !p.pad_w0 && !p.pad_w1;
    if (!is1x1 || a.M > 4096 || (exp_env("TAMD_PW_SMALL") && atoi(exp_env("TAMD_PW_SMALL")) == 0)) return 0;
    PwDwArgs v{};
    const int slices = (cout + 15) / 16, cws = slices * 16;
    const int steps = pwdw_steps((ckp + 63) / 64), nsteps = rup((ckp + 63) / 64, steps);
    const std::vector<int8_t> wf = pack_pw_panel(c.wd, cout, cin, nsteps);
    const std::vector<int32_t> b2 = padded_bias(c.bd, cout, cws);
    int8_t* d0; int32_t* d1;
    if (upload(c.g, wf, &d0) || upload(c.g, b2, &d1) || upload_rq(c.g, c.rq, cws, &v.wscale, &v.rq)) return -1;
    v.wf = d0; v.bias = d1;
    v.x = a.x; v.N = x.n; v.H = x.h; v.W = x.w; v.cs_in = x.cs; v.ktot = ckp; v.nsteps = nsteps; v.steps = steps;
    v.mode = 2; v.prod = 0; v.slices = slices; v.cw = cws;
    v.coherent = (c.g->opt.direct_dispatch && !exp_plain_kernels()) ? 1 : 0;
    v.tile_major = (double)x.h * x.w * x.cs > (double)cout * ckp && slices <= 65535 ? 1 : 0;
    v.y = a.y; v.ldc = a.ldc; v.c_off = a.c_off; v.c_limit = a.c_limit;
    v.S = 1; v.OH = x.h; v.OW = x.w; v.TW = x.w; v.tiles_x = 1; v.RH = 1; v.RW = x.w;
    for (int px : {64, 128, 256}) {          // pixels per block: 1, 2, 4 tiles of 16 per wave at 256 threads
        int th = std::max(1, std::min(x.h, px / std::max(1, x.w)));
        v.TH = th; v.tiles_y = (x.h + th - 1) / th;
        bool dup = false;
        for (auto& k : cands) dup |= k.tag == "pw_small_i8<" + std::to_string(th) + ">";
        if (dup || !pwdw_config_ok(v, 256)) continue;
        const PwDwArgs vc = v;
        cands.push_back({"pw_small_i8<" + std::to_string(th) + ">", [vc](hipStream_t s) { return launch_pwdw(vc, 256, s); }});
    }
    return 0;
}

// conv_igemm: one candidate per tile configuration when the race is on, else the launcher's heuristic -- where nothing above applied
static void gemm_igemm_cands(const ConvArgs& a, bool autotune, std::vector<RaceCand>& cands)
{
    if (!cands.empty() && !autotune) return;
    if (!autotune) { cands.push_back(igemm_cand(a, -1)); return; }
    for (int k = 0; k < conv_igemm_num_cfgs(); k++) {
        if ((k == 1 || k == 3) && a.cout > 256 && a.M > 4096) continue;       // slivers: never competitive there
        if (conv_igemm_cfg_ok(a, k)) cands.push_back(igemm_cand(a, k));
    }
}

// TAMD_FORCE_GEMM (tests; read at every prerun): pin one member of the family -- "igemm<k>", or the prefix of a candidate's tag
static void force_gemm_filter(const ConvArgs& a, std::vector<RaceCand>& cands)
{
    const char* force = getenv("TAMD_FORCE_GEMM");
    if (!force) return;
    const std::string want = force;
    std::vector<RaceCand> only;
    for (int k = 0; k < conv_igemm_num_cfgs(); k++)
        if (want == "igemm" + std::to_string(k) && conv_igemm_cfg_ok(a, k)) only.push_back(igemm_cand(a, k));
    for (auto& k : cands)
        if (k.tag.find(want) == 0) only.push_back(k);
    if (!only.empty()) cands = only;
}

// Every kernel of the family computes the same bytes (exact integer GEMM + the same epilogue), so the choice is purely a matter
// of speed.  The heuristic candidates come first: a later one has to win by more than the timing noise; the heuristics remain
// the fallback (TAMD_AUTOTUNE=0)
static int conv_i8_gemm(ConvI8& c, const FusedElt* fz, Planned* out)
{
    Step& st = out->step;
    ConvArgs a{};
    std::vector<int8_t> wp;
    if (conv_i8_gemm_args(c, &a, &wp)) return -1;
    out->kind = Planned::GEMM; out->gemm = a;       // (as it is without the eltwise tail: what a fuser reads)
    if (fz) { conv_i8_elt_tail(c, *fz, a, st); out->gemm_tail = a; }
    std::vector<RaceCand> cands;        // tag = kernel name
    gemm_fixed_cands(a, fz != nullptr, cands);
    if (gemm_pgemm_cands(c, a, wp, cands)) return -1;
    if (!fz && gemm_pw_small_cands(c, a, cands)) return -1;
    const bool autotune = autotune_enabled() && st.macs >= 5e5;
    gemm_igemm_cands(a, autotune, cands);
    force_gemm_filter(a, cands);
    char ckey[256];
    snprintf(ckey, sizeof(ckey), "gemm|%s|%dx%dx%dx%d>%d k%dx%d s%d%s", c.n.name.c_str(), c.x.n, c.x.c, c.x.h, c.x.w, c.cout, c.KH, c.KW, c.p.stride_h, fz ? "+elt" : "");
    const int best = plan_race(c.g, c.n.name, cands, ckey, 0.96f, autotune && cands.size() > 1);
    if (best < 0) return -1;
    st.kernel = cands[best].tag + (fz ? (fz->relu ? "+eltwise+relu" : "+eltwise") : "");
    st.fn = cands[best].fn;
    return 0;
}

// Plans one convolution / FC node as ONE launch and hands it out in *out; nothing is pushed onto g->steps here.
int plan_conv(tamd_graph* g, HNode& n, bool as_fc, const FusedElt* fz, Planned* out)
{
    ConvI8 c{g, n, g->tensors[n.in[0]], g->tensors[n.in[1]], n.in.size() > 2 ? &g->tensors[n.in[2]] : nullptr, g->tensors[n.out[0]]};
    if (conv_i8_open(c, as_fc)) return -1;
    // the step without kernel and launch, which the form fills in.  Constants aside, all a convolution / FC launch touches is its input
    // and its output; with an eltwise tail (a GEMM form always: scan_eltwise_fusion) it also reads the other operand and stores the
    // tail's output instead of its own, and stays ordered
    if (fz) out->step = make_step(n.name, "", c.macs, c.bytes, nullptr, {access_of(c.x), access_of(g->tensors[fz->res_tensor])}, {access_of(g->tensors[fz->out_tensor])}, false);
    else out->step = make_step(n.name, "", c.macs, c.bytes, nullptr, {access_of(c.x)}, {access_of(c.y)}, true);
    out->elt_tail = fz != nullptr;
    switch (conv_i8_form(c)) {
    case Planned::FIRST: return conv_i8_first(c, out);
    case Planned::DW3X3: return conv_i8_dw3x3(c, out);
    case Planned::GEMM: return conv_i8_gemm(c, fz, out);
    default: return conv_i8_direct(c, out);
    }
}


int plan_pool(tamd_graph* g, HNode& n, Planned* out)
{
    HTensor& x = g->tensors[n.in[0]];
    HTensor& y = g->tensors[n.out[0]];
    PoolGeom pg = pool_geom(n.p.pool, x.h, x.w);
    PoolArgs a{};
    a.x = (const int8_t*)x.dptr + x.c_off; a.y = (int8_t*)y.dptr;
    a.N = x.n; a.H = x.h; a.W = x.w; a.C = x.c; a.cs_in = x.cs; a.OH = y.h; a.OW = y.w; a.ldc = y.cs; a.c_off = y.c_off;
    a.KH = pg.kh; a.KW = pg.kw; a.SH = pg.sh; a.SW = pg.sw; a.PH = pg.ph0; a.PW = pg.pw0;
    a.method = n.p.pool.pool_method; a.caffe_flavor = n.p.pool.caffe_flavor;
    a.in_scale = x.scales[0]; a.out_scale = y.scales[0];
    out->kind = Planned::POOL; out->pool = a;
    // (x and y may be channel slices of ONE concat buffer -- concat(x, pool(x), ..) -- which access_overlap tells apart)
    out->step = make_step(n.name, "pool_i8", 0, (double)x.n * x.h * x.w * x.c + (double)y.n * y.h * y.w * y.c, [a](hipStream_t s) { return launch_pool(a, s); },
                          {access_of(x)}, {access_of(y)}, false);
    return 0;
}

}  // namespace tamd
