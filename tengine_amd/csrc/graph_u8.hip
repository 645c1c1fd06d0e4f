// Planner for uint8 (per-tensor asymmetric) device graphs.
//
// The reference simulates uint8 in fp32 (see u8_kernels.hip); the device keeps every activation as a dense
// NCHW byte tensor -- the reference's own order, so graph inputs/outputs need no layout pass -- and prepares, once
// at prerun, exactly the fp32 operands the reference prepares:
//   conv (group 1)  weights -> fp32 as conv_kernel_x86.c:68-80 (interleave_uint8), transposed to [K][cout_pad];
//                   k -> (c,ky,kx) offsets of im2col_uint8 (:126-185) as a lookup table
//   conv (grouped)  weights -> fp32 as conv_kernel_ref_uint8.c:82-86, OIHW kept
//   fc              weights -> fp32 as fc_ref.c:150-160, transposed to [hidden][nout_pad]
//
// Structure: plan_u8 walks the nodes and calls one function per node kind; each hands back the launches it planned, every one stating
// what it reads and writes (graph.h: make_step), and plan_u8 alone appends them through append_steps.  A convolution is a ConvU8 (the node's tensors, quantisation, fused tail, bias, step skeleton)
// that one of four forms turns into a launch: conv_u8_dma, conv_u8_int, conv_u8_exact, conv_u8_direct.
#include <hip/hip_runtime.h>
#include "env.h"

#include <cstdlib>
#include <cstring>

#include <functional>
#include <map>
#include <mutex>

#include "graph.h"

namespace tamd {

static int q_of(const HTensor& t, U8Q* q, const char* what)
{
    if (t.scales.empty()) { set_error("%s %s has no quantisation parameters", what, t.name.c_str()); return -1; }
    q->scale = t.scales[0];
    q->zp = t.zps.empty() ? 0 : t.zps[0];
    return 0;
}

// the TAMD_PIN keys of the conv planner, read once per node (at every prerun: tests switch them); null: not pinned
struct U8Pins {
    const char* patch;         // u8_patch: 0 never the patch kernel (conv_u8_patch_prepare), 1 whenever it applies, otherwise it has to win the timing
    const char* patch_cfg;     // u8_patch_cfg: with u8_patch=1, the patch configuration that competes alone / is tried first
    const char* c3;            // u8_c3, u8_pw: 0 never, 1 wherever it applies (tests)
    const char* pw;
    const char* rgb;           // u8_rgb3x3: 0 never, 1 always (tests)
    const char* cfg;           // u8_cfg: one GEMM tile shape (conv_u8_gemm_pick reads the value); no race
    const char* i_pw;          // u8i_pw: 0 never the integer pointwise kernel (tests), 1 only it where it applies
    const char* i_cfg;         // u8i_cfg: one integer tile shape where it applies (tests / fuzzing)
};
static bool pin_is(const char* v, int k) { return v && atoi(v) == k; }

// One convolution node, built once (conv_u8_open): what the four forms below share
struct ConvU8 {
    tamd_graph* g;
    HNode& n;
    HTensor& x; HTensor& w; HTensor* b;
    HTensor& yc;               // the conv's own output: its quantisation parameters
    HTensor& y;                // where the bytes go (the fused ReLU's output)
    const tamd_conv_param& p;
    const HNode* relu;         // ReLU / 2x2 stride-2 max-pool node applied in the conv epilogue (U8Relu / U8PoolFuse); null: none
    const HNode* pool;
    U8Pins pin;
    int K = 0, cout = 0;
    U8Q qx{}, qw{}, qy{};
    U8Relu fr{};
    const int32_t* dbias = nullptr;
    Step st;                   // node, macs, bytes, what the launch touches: every form starts from it
    // device copies of the weights, each made when a candidate that reads it is first launched or chosen
    std::map<int, uint8_t*> wgemm;     // (BM, KC) -> raw bytes packed for that GEMM tile shape
    float* wfrag = nullptr;            // dequantised, in MFMA fragment order: one copy serves every patch configuration, conv_u8_pw and conv_u8_c3
    float* wrgb = nullptr;             // dequantised, [cout][rup(K, 4)]: conv_u8_rgb3x3
};

static int conv_u8_open(ConvU8& c)
{
    if (c.w.dtype != TAMD_DT_UINT8 || (c.b && c.b->dtype != TAMD_DT_INT32)) { set_error("conv %s: uint8 weights / int32 bias expected", c.n.name.c_str()); return -1; }
    if (q_of(c.x, &c.qx, "tensor") || q_of(c.w, &c.qw, "weight") || q_of(c.yc, &c.qy, "tensor")) return -1;
    if (c.relu) { c.fr.on = 1; c.fr.slope = c.relu->p.relu.negative_slope; if (q_of(c.y, &c.fr.out, "tensor")) return -1; }
    c.K = c.x.c / c.p.group * c.p.kernel_h * c.p.kernel_w; c.cout = c.y.c;
    if ((size_t)c.cout * c.K != c.w.data.size()) { set_error("conv %s: weight size mismatch", c.n.name.c_str()); return -1; }
    if (upload_bias(c.g, c.b, c.cout, &c.dbias)) return -1;
    // everything a form's launch touches besides constants: the input, the output (a concat slice when it is a view), the pooled output
    std::vector<Access> wr{access_of(c.y)};
    if (c.pool) wr.push_back(access_of(c.g->tensors[c.pool->out[0]]));
    c.st = make_step(c.n.name, "", (double)c.y.n * c.y.h * c.y.w * c.cout * c.K,
                     (double)c.x.n * c.x.c * c.x.h * c.x.w + (double)c.y.n * c.cout * c.y.h * c.y.w + 1.0 * c.cout * c.K, nullptr, {access_of(c.x)}, wr, false);
    return 0;
}

// the launch of a form: the skeleton and the kernel's name with the fused tail's suffixes.  deps: as make_step
static Step conv_u8_step(const ConvU8& c, const char* kernel, bool deps, std::function<hipError_t(hipStream_t)> fn)
{
    Step st = c.st;
    st.kernel = std::string(kernel) + (c.relu ? "+relu" : "") + (c.pool ? "+maxpool" : "");
    st.deps = deps;
    st.fn = std::move(fn);
    return st;
}

// the plan-cache key of a conv's race at `site` ("u8conv": the byte-exact family, "u8iconv": the integer path's tiles)
static std::string conv_u8_race_key(const ConvU8& c, const char* site)
{
    char key[256];
    snprintf(key, sizeof(key), "%s|%s|%dx%dx%dx%d>%d k%dx%d s%d d%d%s%s", site, c.n.name.c_str(), c.x.n, c.x.c, c.x.h, c.x.w, c.cout, c.p.kernel_h,
             c.p.kernel_w, c.p.stride_h, c.p.dilation_h, c.relu ? "+relu" : "", c.pool ? "+pool" : "");
    return key;
}

// w_fp32 = ((float)w - (float)zp) * scale (conv_kernel_x86.c:68-80)
static float conv_u8_wf(const ConvU8& c, int co, int k) { return ((float)c.w.data[(size_t)co * c.K + k] - (float)c.qw.zp) * c.qw.scale; }

// ---- the fp32 LDS-DMA form (conv_f32_mfma.hip): fp32 copy of the input + fp32 packed weights ----

static bool u8_dma_wanted(const tamd_conv_param& p, int K)
{
    static const char* dma_env = exp_env("TAMD_U8_DMA");
    bool use_dma = dma_env && atoi(dma_env) != 0;            // measured no faster than the register-staged kernel
    // the register-staged kernel keeps the whole k -> tap table in LDS: beyond ~28k taps it does not fit next to the
    // operand tiles (160 KB per CU) and the DMA kernel (table read with scalar loads) takes over
    if (p.group == 1 && (size_t)(rup(K, 64) + 2 * (64 + 64) * 36) * 4 > 150 * 1024) use_dma = true;
    return use_dma;
}

// Which fused tail the form this node gets can carry, asked before anything is planned or uploaded: the pooled epilogue lives in the
// group-1 byte kernels (conv_u8_gemm / _patch / _c3 / _rgb3x3 and the integer path), and the DMA kernel has no fused ReLU tail either
struct U8Tail { bool pool, relu; };
static U8Tail conv_u8_tail(const tamd_graph* g, const HNode& n)
{
    const tamd_conv_param& p = n.p.conv;
    const bool dma = u8_dma_wanted(p, g->tensors[n.in[0]].c / p.group * p.kernel_h * p.kernel_w);
    return {p.group == 1 && !dma, !(p.group == 1 && dma)};
}

// `dq`: the launch that refreshes the fp32 copy of the input, where this conv is the first to read it (kernel empty: none)
static int conv_u8_dma(ConvU8& c, Step* dq, Step* out)
{
    tamd_graph* g = c.g;
    const HTensor &x = c.x, &y = c.y;
    const tamd_conv_param& p = c.p;
    const int K = c.K, cout = c.cout, Kpad = rup(K, 32);
    F32ConvArgs a{};
    a.N = x.n; a.C = x.c; a.H = x.h; a.W = x.w; a.OH = y.h; a.OW = y.w; a.cout = cout;
    a.K = K; a.Kpad = Kpad; a.SH = p.stride_h; a.SW = p.stride_w; a.PH = p.pad_h0; a.PW = p.pad_w0;
    a.tail_split = 1;
    if (conv_f32_mfma_operands(g, a, p.kernel_h, p.kernel_w, p.dilation_h, p.dilation_w, [&](int co, int k) { return conv_u8_wf(c, co, k); })) return -1;
    // the fp32 copy of the input tensor (shared by every conv that reads it; refreshed once per run)
    float* xf = nullptr;
    auto it = g->f32_copy.find(c.n.in[0]);
    if (it == g->f32_copy.end()) {
        void* pxf = nullptr;
        if (dev_alloc(g, &pxf, x.elems() * sizeof(float), true)) return -1;
        xf = (float*)pxf;
        g->f32_copy[c.n.in[0]] = xf;
        const uint8_t* src = (const uint8_t*)x.dptr;
        const size_t cnt = x.elems();
        const float zp = (float)c.qx.zp, sc = c.qx.scale;
        *dq = make_step(x.name, "dequant_u8_f32", 0, 5.0 * cnt,
                        [src, xf, cnt, zp, sc](hipStream_t s) { return launch_dequant_u8_f32(src, xf, cnt, zp, sc, s); },
                        {access_of(x)}, {access_of_bytes(xf, cnt * sizeof(float))}, false);
    } else
        xf = it->second;
    if (!g->zero_page) { if (dev_alloc(g, &g->zero_page, 256, true)) return -1; }
    a.x = xf; a.zeros = (const float*)g->zero_page; a.bias = c.dbias; a.y = (uint8_t*)y.dptr;
    a.out_img = nchw_out_img(y); a.out_c0 = y.c_off;
    a.m_blocked = (cout >> 3 << 3) + (((cout - (cout >> 3 << 3)) >> 2) << 2);
    a.bias_scale = c.qx.scale * c.qw.scale;           // conv_kernel_x86.c:1723
    a.act = p.activation; a.out_scale = c.qy.scale; a.out_zp = c.qy.zp;
    *out = conv_u8_step(c, conv_f32_mfma_kernel_name(a), false, [a](hipStream_t s) { return launch_conv_f32_mfma(a, s); });
    out->rd = {access_of_bytes(xf, x.elems() * sizeof(float))};      // the launch reads the fp32 copy, not x
    out->bytes = 4.0 * x.elems() + (double)y.elems() + 4.0 * cout * K;
    return 0;
}

// ---- group 1 on the byte kernels: the arguments the integer path and the byte-exact family share ----

static int conv_u8_args(ConvU8& c, U8ConvArgs* args)
{
    tamd_graph* g = c.g;
    const HTensor &x = c.x, &y = c.y;
    const tamd_conv_param& p = c.p;
    const int K = c.K, cout = c.cout, Kpad = rup(K, 64), cout_pad = rup(cout, 64);     // 64: the deepest K stage of the kernel family
    U8ConvArgs a{};
    a.N = x.n; a.C = x.c; a.H = x.h; a.W = x.w; a.OH = y.h; a.OW = y.w; a.cout = cout; a.cout_pad = cout_pad;
    a.K = K; a.Kpad = Kpad; a.SH = p.stride_h; a.SW = p.stride_w; a.PH = p.pad_h0; a.PW = p.pad_w0;
    a.cfg = conv_u8_gemm_pick(a);
    if ((p.kernel_h - 1) * p.dilation_h > 15 || (p.kernel_w - 1) * p.dilation_w > 15 || (size_t)x.c * x.h * x.w >= (1u << 24)
        || conv_u8_gemm_lds(a) > 150 * 1024) {
        set_error("conv %s: kernel extent / image size / K = %d outside the packed tap table of the uint8 GEMM kernel", c.n.name.c_str(), K);
        return -1;
    }
    unsigned* dlut = nullptr;
    if (upload(g, conv_tap_table(K, Kpad, x.h, x.w, p.kernel_h, p.kernel_w, p.dilation_h, p.dilation_w), &dlut)) return -1;
    a.x = (const uint8_t*)x.dptr; a.klut = dlut; a.w_scale = c.qw.scale; a.w_zp = (float)c.qw.zp; a.bias = c.dbias; a.y = (uint8_t*)y.dptr;
    a.out_img = nchw_out_img(y); a.out_c0 = y.c_off;
    a.m_blocked = (cout >> 3 << 3) + (((cout - (cout >> 3 << 3)) >> 2) << 2);
    a.in_scale = c.qx.scale; a.in_zp = (float)c.qx.zp;
    a.bias_scale = c.qx.scale * c.qw.scale;           // conv_kernel_x86.c:1723
    a.act = p.activation; a.out_scale = c.qy.scale; a.out_zp = c.qy.zp; a.relu = c.fr;
    {   // the integer path's requantisation constants (u8_epilogue.h: u8i_requant), binary32 like everything around them
        const float bs = c.qx.scale * c.qw.scale;
        a.i_m = bs / c.qy.scale;
        a.i_qlo = 0; a.i_qhi = 255;
        if (p.activation >= 0) a.i_qlo = std::min(std::max(c.qy.zp, 0), 255);
        if (p.activation > 0) a.i_qhi = std::min(255, std::max(a.i_qlo, (int)roundf(6.0f / c.qy.scale) + c.qy.zp));
    }
    if (c.pool) {
        HTensor& yp = g->tensors[c.pool->out[0]];
        a.pool.on = 1;
        a.pool.y = (uint8_t*)yp.dptr;
        a.pool.out_img = nchw_out_img(yp); a.pool.out_c0 = yp.c_off;
        if (q_of(y, &a.pool.in, "tensor") || q_of(yp, &a.pool.out, "tensor")) return -1;
        a.pool.write_full = count_consumers(g, c.pool->in[0]) > 1;
        for (auto& io : g->outputs) a.pool.write_full |= (io.tensor == c.pool->in[0]);
        c.st.bytes += (double)yp.elems() - (a.pool.write_full ? 0.0 : (double)y.elems());
    }
    *args = a;
    return 0;
}

// ---- the opt-in INTEGER path (tamd_options.u8_integer; u8i_kernels.hip): exact int32 sums on the int8 MFMA, one rounding,
// then the reference's own requantisation -- within one quantisation step of the reference's bytes, not identical.
// Everything of this node that is not the convolution proper (fused ReLU / max-pool tails, concat-by-offset placement)
// is shared with the byte-exact kernels.  Layers the kernel does not take (maps narrower than 4 columns, patches beyond
// 512 pixels) fall through to the byte-exact family, whose bytes are inside the bar by definition.
// Both functions: 1 = *out is the launch, 0 = not taken, -1 = error.

// first layers (3x3 on <= 4 input channels against the general kernel's 32-channel K step); the others stay on conv_u8_rgb3x3 / the staging GEMM
static int conv_u8_int_first(ConvU8& c, U8ConvArgs& a, Step* out)
{
    const tamd_conv_param& p = c.p;
    if (!(c.x.c <= 4 && !(exp_env("TAMD_U8I_RGB") && atoi(exp_env("TAMD_U8I_RGB")) == 0))) return 0;
    a.i_alpha = c.qx.zp - 128; a.i_beta = c.qw.zp - 128;
    if (!conv_u8i_rgb_applicable(a, p.kernel_h, p.kernel_w, p.dilation_h, p.dilation_w)) return 0;
    conv_u8i_rgb_prepare(a);
    std::vector<int8_t> wp(conv_u8i_rgb_packed_bytes(a));
    std::vector<int32_t> cv((size_t)rup(c.cout, 16) + 4);
    conv_u8i_rgb_pack(a, c.w.data.data(), c.qw.zp, c.qx.zp, c.b ? (const int32_t*)c.b->data.data() : nullptr, wp.data(), cv.data());
    int8_t* dw = nullptr; int32_t* dc = nullptr;
    if (upload(c.g, wp, &dw) || upload(c.g, cv, &dc)) return -1;
    a.iw = dw; a.icv = dc;
    *out = conv_u8_step(c, "conv_u8i_rgb3x3", true, [a](hipStream_t s) { return launch_conv_u8i_rgb(a, s); });
    return 1;
}

// candidates: the general kernel's tile shapes (ids 0..5) and, for 1x1 / stride 1 / unpadded layers, the register-only
// pointwise kernel's (ids 6..11).  Every one computes the same bytes (exact integer sums, one epilogue)
static int conv_u8_int_tiles(ConvU8& c, U8ConvArgs& a, Step* out)
{
    const HTensor &x = c.x, &y = c.y;
    const tamd_conv_param& p = c.p;
    const int cout = c.cout;
    const char* imc = exp_env("TAMD_U8_INT_MIN_C");
    if (x.c < (imc ? atoi(imc) : 8)) return 0;
    a.i_alpha = c.qx.zp - 128; a.i_beta = c.qw.zp - 128;
    const int NG = conv_u8i_num_cfgs(), NP = conv_u8i_pw_num_cfgs();
    auto iprepare = [&](U8ConvArgs& ac, int cf) -> bool {
        return cf < NG ? conv_u8i_prepare(ac, cf, p.kernel_h, p.kernel_w, p.dilation_h, p.dilation_w) : conv_u8i_pw_prepare(ac, cf - NG, p.kernel_h, p.kernel_w);
    };
    std::vector<int> cands;
    for (int cf = 0; cf < NG + NP; cf++) {
        if (cf >= NG && pin_is(c.pin.i_pw, 0)) continue;
        U8ConvArgs ac = a;
        if (iprepare(ac, cf)) cands.push_back(cf);
    }
    if (pin_is(c.pin.i_pw, 1)) {
        std::vector<int> only;
        for (int cf : cands) if (cf >= NG) only.push_back(cf);
        if (!only.empty()) cands.swap(only);
    }
    if (c.pin.i_cfg && *c.pin.i_cfg) {
        const int want = atoi(c.pin.i_cfg) % (NG + NP);
        if (std::find(cands.begin(), cands.end(), want) != cands.end()) cands.assign(1, want);
    }
    if (cands.empty()) return 0;
    std::map<int, std::pair<int8_t*, int32_t*>> ipacked;      // cout tile height -> packed weights + per-channel constants
    auto bm_of = [&](int cf) { return cf < NG ? conv_u8i_bm(cf) : conv_u8i_pw_bm(cf - NG); };
    auto iready = [&](U8ConvArgs& ac, int cf) -> int {
        if (!iprepare(ac, cf)) return -1;
        const int bm = bm_of(cf);
        auto it = ipacked.find(bm);
        if (it == ipacked.end()) {
            std::vector<int8_t> wp(conv_u8i_packed_bytes(ac, bm));
            std::vector<int32_t> cv((size_t)rup(cout, bm) + 4);
            conv_u8i_pack(ac, bm, c.w.data.data(), c.qw.zp, c.qx.zp, c.b ? (const int32_t*)c.b->data.data() : nullptr, wp.data(), cv.data());
            int8_t* dw = nullptr; int32_t* dc = nullptr;
            if (upload(c.g, wp, &dw) || upload(c.g, cv, &dc)) return -1;
            it = ipacked.emplace(bm, std::make_pair(dw, dc)).first;
        }
        ac.iw = it->second.first; ac.icv = it->second.second;
        return 0;
    };
    auto ilaunch = [NG](const U8ConvArgs& ac, int cf, hipStream_t s) { return cf < NG ? launch_conv_u8i(ac, s) : launch_conv_u8i_pw(ac, s); };
    auto iname = [NG](const U8ConvArgs& ac, int cf) { return cf < NG ? conv_u8i_kernel_name(ac) : conv_u8i_pw_kernel_name(ac); };
    // geometry heuristic: the largest tile that still gives every CU a block; the plan-time timing then decides
    auto blocks_of = [&](int cf) {
        U8ConvArgs ac = a;
        iprepare(ac, cf);
        static const int bns[] = {64, 64, 128, 128, 128, 256};
        const int bm = bm_of(cf), bn = cf < NG ? bns[cf] : conv_u8i_pw_bn(cf - NG);
        const long tiles = ac.i_tw ? (long)((y.w + ac.i_tw - 1) / ac.i_tw) * ((y.h + bn / ac.i_tw - 1) / (bn / ac.i_tw)) : (y.h * y.w + bn - 1) / bn;
        return tiles * x.n * ((cout + bm - 1) / bm);
    };
    int pick = cands[0];
    {
        static const int pref[] = {6, 7, 9, 8, 10, 11, 3, 1, 2, 0, 5, 4};
        long most = -1;
        bool done = false;
        for (int cf : pref) {
            if (std::find(cands.begin(), cands.end(), cf) == cands.end()) continue;
            const long bl = blocks_of(cf);
            if (!done && bl >= 256) { pick = cf; done = true; }
            if (!done && bl > most) { most = bl; pick = cf; }
        }
    }
    // the heuristic pick is timed first; another shape has to beat it by more than the timing noise.  The candidates run inside
    // plan_race below: what they capture by reference (a, iready and its cache) lives in this frame
    std::vector<int> order{pick};
    for (int cf : cands) if (cf != pick) order.push_back(cf);
    std::vector<RaceCand> race;
    for (int cf : order) {
        U8ConvArgs ac = a;
        iprepare(ac, cf);
        race.push_back({"i" + std::to_string(cf), [&, cf](hipStream_t s) {
                            U8ConvArgs ar = a;
                            return iready(ar, cf) ? hipErrorOutOfMemory : ilaunch(ar, cf, s);
                        }, iname(ac, cf)});
    }
    const int w = plan_race(c.g, c.n.name, race, conv_u8_race_key(c, "u8iconv"), 0.96f, autotune_enabled() && c.st.macs >= 4e6 && cands.size() > 1);
    if (w < 0) return -1;
    const int picked = order[w];
    if (iready(a, picked)) return -1;
    *out = conv_u8_step(c, iname(a, picked), true, [a, picked, ilaunch](hipStream_t s) { return ilaunch(a, picked, s); });
    return 1;
}

// ---- the byte-exact family: conv_u8_gemm's tile shapes, conv_u8_patch's configurations, conv_u8_pw, conv_u8_c3, conv_u8_rgb3x3.
// Every member produces the same bytes (the chain order of an output does not depend on the tiling; the patch kernel -- 3x3 / 1x1
// with whole super-steps of channels -- is one more candidate of the same bytes), so which one runs is a plan-time choice: pins
// first, then the race, then the heuristics

struct U8Choice {
    enum Form { GEMM, PATCH, PW, C3, RGB } form;
    int cfg;                   // GEMM: tile shape; PATCH: patch configuration
    int gemm_cfg;              // PATCH: the GEMM tile shape whose weights are packed all the same (see conv_u8_exact)
};
struct U8Applies { bool pw, c3, rgb; };

// raw bytes, [cout tile][stage][row][32 slots], slot (k%4)*8 + (k%32)/4; padding = weight zero point
static uint8_t* gemm_weights(ConvU8& c, int cfg)
{
    const int K = c.K, cout = c.cout;
    const int BM = conv_u8_gemm_bm(cfg), KC = conv_u8_gemm_kc(cfg), NPOS = KC / 4, nstage = rup(K, KC) / KC;
    auto it = c.wgemm.find(BM * 1000 + KC);
    if (it != c.wgemm.end()) return it->second;
    const int ntile = (cout + BM - 1) / BM;
    std::vector<uint8_t> wq((size_t)ntile * nstage * BM * KC, (uint8_t)c.qw.zp);
    for (int co = 0; co < cout; co++)
        for (int k = 0; k < K; k++) {
            const int kl = k % KC;
            wq[(((size_t)(co / BM) * nstage + k / KC) * BM + co % BM) * KC + (kl & 3) * NPOS + (kl >> 2)] = c.w.data[(size_t)co * K + k];
        }
    uint8_t* d = nullptr;
    if (upload(c.g, wq, &d)) return nullptr;
    c.wgemm[BM * 1000 + KC] = d;
    return d;
}

// the fragment-order weights of `ac` (its pk_k* name the filter shape), made once
static int frag_weights(ConvU8& c, U8ConvArgs& ac)
{
    if (!c.wfrag) {
        std::vector<float> wp(conv_u8_patch_packed_bytes(ac) / 4);
        conv_u8_patch_pack(ac, c.w.data.data(), (uint8_t)c.qw.zp, c.qw.scale, wp.data());
        if (upload(c.g, wp, &c.wfrag)) return -1;
    }
    ac.wpk = reinterpret_cast<const uint8_t*>(c.wfrag);
    return 0;
}
static bool patch_applies(const ConvU8& c, U8ConvArgs ac, int cfg, U8ConvArgs* prepared = nullptr)      // *prepared: a copy of ac with its pk_* filled
{
    const bool ok = conv_u8_patch_prepare(ac, cfg, c.p.kernel_h, c.p.kernel_w, c.p.dilation_h, c.p.dilation_w);
    if (prepared) *prepared = ac;
    return ok;
}
static int patch_ready(ConvU8& c, U8ConvArgs& ac, int cfg)          // 1: ready, 0: not applicable, -1: error
{
    if (!patch_applies(c, ac, cfg, &ac)) return 0;
    return frag_weights(c, ac) ? -1 : 1;
}
// conv_u8_pw shares the 1x1 fragment-order weights and the tail blocks with the patch kernel, not its switches
static int pw_ready(ConvU8& c, U8ConvArgs& ac)
{
    ac.pk_kh = ac.pk_kw = 1; ac.pk_dh = ac.pk_dw = 1; ac.pk_wp = 0; ac.pk_cfg = 0; ac.pk_npad = 64;
    return frag_weights(c, ac);
}
// conv_u8_c3 (shallow 3x3 layers of large maps) shares the 3x3 fragment-order weights and the tail blocks with the patch kernel
static int c3_ready(ConvU8& c, U8ConvArgs& ac)
{
    ac.pk_kh = ac.pk_kw = 3; ac.pk_dh = ac.pk_dw = 1; ac.pk_wp = 0; ac.pk_cfg = 0; ac.pk_npad = 256; ac.pk_tw = 0;
    return frag_weights(c, ac);
}
static int rgb_ready(ConvU8& c, U8ConvArgs& ac)
{
    ac.wf_ld = rup(c.K, 4);
    if (!c.wrgb) {
        std::vector<float> wf((size_t)c.cout * ac.wf_ld, 0.f);
        for (int co = 0; co < c.cout; co++)
            for (int k = 0; k < c.K; k++) wf[(size_t)co * ac.wf_ld + k] = conv_u8_wf(c, co, k);
        if (upload(c.g, wf, &c.wrgb)) return -1;
    }
    ac.wf = c.wrgb;
    return 0;
}

// The race, one ordered list: the GEMM family's tile shapes (the heuristic one first), the patch kernel's configurations,
// conv_u8_pw, conv_u8_c3, conv_u8_rgb3x3 -- the last to beat the best so far by more than the timing noise wins.  Per-launch
// times as the candidates run inside a pass (plan_race's cold timing: back-to-back launches of one layer flatter the
// latency-bound members by 30-60 %, profiles/r03_insitu_*).  The plan cache records "g<cfg>" GEMM family, "p<cfg>" patch
// kernel, "pw", "c3" or "rgb"; a pinned race (u8_patch, u8_rgb3x3, u8_pw, u8_c3) never reads the file, it still writes it.
// *tag: the winner's.  The candidates run inside this call and copy `a` when they do; `c` and `a` are the caller's
static int conv_u8_exact_race(ConvU8& c, const U8ConvArgs& a, const U8Applies& ok, std::string* tag)
{
    const tamd_conv_param& p = c.p;
    const U8Pins& pin = c.pin;
    const bool pk_force = pin_is(pin.patch, 1);
    const bool pinned = pin.patch || pin.rgb || pin.pw || pin.c3;
    const std::function<bool()> unpinned = [pinned]() { return !pinned; };
    std::vector<RaceCand> race, patches;
    std::vector<int> order{a.cfg};
    for (int cf = 0; cf < conv_u8_gemm_num_cfgs(); cf++)
        if (cf != a.cfg) order.push_back(cf);
    for (int cf : order) {
        U8ConvArgs ac = a; ac.cfg = cf; ac.Kpad = rup(c.K, conv_u8_gemm_kc(cf));
        if (conv_u8_gemm_lds(ac) > 150 * 1024) continue;
        race.push_back({"g" + std::to_string(cf), [&c, ac, cf](hipStream_t s) {
                            U8ConvArgs ar = ac;
                            return (ar.wq = gemm_weights(c, cf)) ? launch_conv_u8_gemm(ar, s) : hipErrorOutOfMemory;
                        }, conv_u8_gemm_kernel_name(ac), unpinned});
    }
    int named = pk_force && pin.patch_cfg ? atoi(pin.patch_cfg) % conv_u8_patch_num_cfgs() : -1;
    if (named >= 0 && !patch_applies(c, a, named)) named = -1;
    for (int cf = 0; cf < conv_u8_patch_num_cfgs(); cf++) {
        // u8_patch=1 + u8_patch_cfg=<c>: that configuration alone competes where it applies (tests pin forms with it);
        // without a name the lanes configuration stays out of the forced race (it pins the MFMA patch kernel)
        if (pk_force && named >= 0 && cf != named) continue;
        if (pk_force && named < 0 && cf == conv_u8_patch_lanes_cfg()) continue;
        U8ConvArgs ac;
        if (!patch_applies(c, a, cf, &ac)) continue;
        patches.push_back({"p" + std::to_string(cf), [&c, &a, cf](hipStream_t s) {
                               U8ConvArgs ar = a;
                               return patch_ready(c, ar, cf) == 1 ? launch_conv_u8_patch(ar, s) : hipErrorOutOfMemory;
                           }, conv_u8_patch_kernel_name(ac), [&c, &a, pinned, cf]() { U8ConvArgs ar = a; return !pinned && patch_ready(c, ar, cf) == 1; }});
    }
    if (pk_force) {
        // u8_patch=1 pins the patch kernel: its configurations race each other alone, the GEMM family only sets the bar
        // conv_u8_pw / _c3 / _rgb3x3 have to beat and stands for the patch kernel in the file
        if (!patches.empty()) {
            const int w = plan_race(c.g, c.n.name, patches, "", 1.0f, true);
            if (w < 0) return -1;
            for (auto& r : race) r.tag = patches[w].tag;
        }
    } else
        race.insert(race.end(), patches.begin(), patches.end());
    if (ok.pw)
        race.push_back({"pw", [&c, &a](hipStream_t s) { U8ConvArgs ar = a; return pw_ready(c, ar) ? hipErrorOutOfMemory : launch_conv_u8_pw(ar, s); },
                        conv_u8_pw_kernel_name(a), unpinned});
    if (ok.c3)
        race.push_back({"c3", [&c, &a](hipStream_t s) { U8ConvArgs ar = a; return c3_ready(c, ar) ? hipErrorOutOfMemory : launch_conv_u8_c3(ar, s); },
                        conv_u8_c3_kernel_name(a), unpinned});
    if (ok.rgb)
        race.push_back({"rgb", [&c, &a](hipStream_t s) { U8ConvArgs ar = a; return rgb_ready(c, ar) ? hipErrorOutOfMemory : launch_conv_u8_rgb3x3(ar, s); },
                        conv_u8_rgb3x3_kernel_name(a), unpinned});
    const int w = plan_race(c.g, c.n.name, race, conv_u8_race_key(c, "u8conv"), 0.96f, true);
    if (w < 0) return -1;
    *tag = race[w].tag;
    return 0;
}

// (pins, what applies, the race winner's tag or "" when the site was not raced) -> the kernel that runs.  Precedence
// rgb > pw > c3 > patch > GEMM; a pin of 1 takes its kernel wherever it applies, whatever the race said.  Under u8_patch=1 the GEMM
// candidates carry the winning patch tag, so a "p<c>" winner is the patch kernel either way
static U8Choice conv_u8_choose(const ConvU8& c, const U8ConvArgs& a, const U8Applies& ok, const std::string& tag)
{
    const U8Pins& pin = c.pin;
    if (tag == "rgb" || (ok.rgb && pin_is(pin.rgb, 1))) return {U8Choice::RGB, 0, 0};
    if (tag == "pw" || (ok.pw && pin_is(pin.pw, 1))) return {U8Choice::PW, 0, 0};
    if (tag == "c3" || (ok.c3 && pin_is(pin.c3, 1))) return {U8Choice::C3, 0, 0};
    int gemm = a.cfg, patch = -1;
    if (tag[0] == 'g') gemm = atoi(tag.c_str() + 1);
    if (tag[0] == 'p') patch = atoi(tag.c_str() + 1);
    if (tag.empty() && !pin.patch && !pin.cfg && patch_applies(c, a, conv_u8_patch_lanes_cfg())) {
        // layers too small to be worth timing (< 4 MMAC): lane-level chains wherever they apply -- a GEMM launch there is 8-19 us
        // of set-up around a handful of live MFMA columns (profiles/r04_layers_mssd_uint8_b16_lanes.txt)
        patch = conv_u8_patch_lanes_cfg();
    }
    if (pin_is(pin.patch, 1) && patch < 0) {
        const int first = pin.patch_cfg ? atoi(pin.patch_cfg) % conv_u8_patch_num_cfgs() : 0;      // tests / fuzzing: the configuration to try first
        for (int k = 0; k < conv_u8_patch_num_cfgs() && patch < 0; k++)
            if (patch_applies(c, a, (first + k) % conv_u8_patch_num_cfgs())) patch = (first + k) % conv_u8_patch_num_cfgs();
    }
    if (patch >= 0) return {U8Choice::PATCH, patch, gemm};
    return {U8Choice::GEMM, gemm, gemm};
}

static int conv_u8_exact(ConvU8& c, U8ConvArgs a, Step* out)
{
    const tamd_conv_param& p = c.p;
    // conv_u8_pw: shallow pointwise layers of large maps; conv_u8_c3: shallow 3x3 layers of large maps; conv_u8_rgb3x3: first layers
    // (3x3 on <= 4 channels), the per-pixel VALU kernel competes with the MFMA family (same bytes)
    const U8Applies ok{conv_u8_pw_applicable(a, p.kernel_h, p.kernel_w), conv_u8_c3_applicable(a, p.kernel_h, p.kernel_w, p.dilation_h, p.dilation_w),
                       conv_u8_rgb3x3_applicable(c.x.c, p.kernel_h, p.kernel_w, p.dilation_h, p.dilation_w, p.group) && c.cout <= 128 && !pin_is(c.pin.rgb, 0)};
    // plan-time autotune over the family; TAMD_AUTOTUNE=0 keeps the heuristic choice
    std::string tag;
    if (autotune_enabled() && c.st.macs >= 4e6 && !c.pin.cfg && conv_u8_exact_race(c, a, ok, &tag)) return -1;
    const U8Choice ch = conv_u8_choose(c, a, ok, tag);
    switch (ch.form) {
    case U8Choice::PW:
        if (pw_ready(c, a)) return -1;
        *out = conv_u8_step(c, conv_u8_pw_kernel_name(a), false, [a](hipStream_t s) { return launch_conv_u8_pw(a, s); });
        break;
    case U8Choice::C3:
        if (c3_ready(c, a)) return -1;
        *out = conv_u8_step(c, conv_u8_c3_kernel_name(a), true, [a](hipStream_t s) { return launch_conv_u8_c3(a, s); });
        break;
    case U8Choice::RGB:
        if (rgb_ready(c, a)) return -1;
        *out = conv_u8_step(c, conv_u8_rgb3x3_kernel_name(a), true, [a](hipStream_t s) { return launch_conv_u8_rgb3x3(a, s); });
        break;
    case U8Choice::GEMM: case U8Choice::PATCH:
        a.cfg = ch.gemm_cfg;
        a.Kpad = rup(c.K, conv_u8_gemm_kc(a.cfg));      // stages of the chosen depth only (the tap table stays padded to 64)
        // (also in front of the patch kernel, which never reads wq: a dead upload, kept so that the allocation order stays what it was)
        if ((a.wq = gemm_weights(c, a.cfg)) == nullptr) return -1;
        if (ch.form == U8Choice::PATCH) {
            if (patch_ready(c, a, ch.cfg) != 1) return -1;
            *out = conv_u8_step(c, conv_u8_patch_kernel_name(a), true, [a](hipStream_t s) { return launch_conv_u8_patch(a, s); });
        } else
            *out = conv_u8_step(c, conv_u8_gemm_kernel_name(a), true, [a](hipStream_t s) { return launch_conv_u8_gemm(a, s); });
        break;
    }
    return 0;
}

// ---- grouped / depthwise: the direct form ----

static int conv_u8_direct(ConvU8& c, Step* out)
{
    const HTensor &x = c.x, &y = c.y;
    const tamd_conv_param& p = c.p;
    std::vector<float> wf((size_t)c.cout * c.K);
    for (size_t i = 0; i < wf.size(); i++) wf[i] = ((float)c.w.data[i] - (float)c.qw.zp) * c.qw.scale;
    float* dwf = nullptr;
    if (upload(c.g, wf, &dwf)) return -1;
    U8DirectArgs a{};
    a.x = (const uint8_t*)x.dptr; a.wf = dwf; a.bias = c.dbias; a.y = (uint8_t*)y.dptr;
    a.N = x.n; a.C = x.c; a.H = x.h; a.W = x.w; a.OH = y.h; a.OW = y.w; a.cout = c.cout;
    a.KH = p.kernel_h; a.KW = p.kernel_w; a.SH = p.stride_h; a.SW = p.stride_w; a.PH = p.pad_h0; a.PW = p.pad_w0;
    a.DH = p.dilation_h; a.DW = p.dilation_w; a.group = p.group;
    a.out_img = nchw_out_img(y); a.out_c0 = y.c_off;
    a.in_scale = c.qx.scale; a.in_zp = (float)c.qx.zp; a.w_scale = c.qw.scale;
    a.act = p.activation; a.out_scale = c.qy.scale; a.out_zp = c.qy.zp; a.relu = c.fr;
    *out = conv_u8_step(c, "conv_u8_direct", false, [a](hipStream_t s) { return launch_conv_u8_direct(a, s); });
    return 0;
}

// one conv node with the fused tail the caller settled (conv_u8_tail): its launch, behind the dequantising step where the DMA form needs one
static int plan_conv_u8(tamd_graph* g, HNode& n, const HNode* relu, const HNode* pool, std::vector<Step>* out)
{
    HTensor& yc = g->tensors[n.out[0]];
    ConvU8 c{g, n, g->tensors[n.in[0]], g->tensors[n.in[1]], n.in.size() > 2 ? &g->tensors[n.in[2]] : nullptr, yc,
             relu ? g->tensors[relu->out[0]] : yc, n.p.conv, relu, pool,
             {tamd_pin("u8_patch"), tamd_pin("u8_patch_cfg"), tamd_pin("u8_c3"), tamd_pin("u8_pw"), tamd_pin("u8_rgb3x3"), tamd_pin("u8_cfg"),
              tamd_pin("u8i_pw"), tamd_pin("u8i_cfg")}};
    if (conv_u8_open(c)) return -1;
    const tamd_conv_param& p = c.p;
    Step dq, st;
    if (p.group != 1) {
        if (conv_u8_direct(c, &st)) return -1;
    } else if (u8_dma_wanted(p, c.K) && (p.kernel_h - 1) * p.dilation_h <= 15 && (p.kernel_w - 1) * p.dilation_w <= 15
               && (size_t)c.x.c * c.x.h * c.x.w < (1u << 24)) {
        if (conv_u8_dma(c, &dq, &st)) return -1;
    } else {
        U8ConvArgs a;
        if (conv_u8_args(c, &a)) return -1;
        int taken = g->opt.u8_integer ? conv_u8_int_first(c, a, &st) : 0;
        if (!taken && g->opt.u8_integer) taken = conv_u8_int_tiles(c, a, &st);
        if (taken < 0 || (!taken && conv_u8_exact(c, a, &st))) return -1;
    }
    if (!dq.kernel.empty()) out->push_back(dq);
    out->push_back(st);
    return 0;
}

static int plan_fc_u8(tamd_graph* g, HNode& n, std::vector<Step>* out)
{
    HTensor& x = g->tensors[n.in[0]];
    HTensor& w = g->tensors[n.in[1]];
    HTensor* b = n.in.size() > 2 ? &g->tensors[n.in[2]] : nullptr;
    HTensor& y = g->tensors[n.out[0]];
    U8Q qx, qw, qy;
    if (q_of(x, &qx, "tensor") || q_of(w, &qw, "weight") || q_of(y, &qy, "tensor")) return -1;
    const int batch = x.dims[0], hidden = (int)(x.elems() / batch), nout = y.c, nout_pad = rup(nout, 64);
    if (w.dtype != TAMD_DT_UINT8 || (size_t)hidden * nout != w.data.size()) { set_error("fc %s: weight mismatch", n.name.c_str()); return -1; }
    if (!fc_u8_row_fits_lds((size_t)hidden)) { set_error("fc %s: hidden %d too large for the LDS row", n.name.c_str(), hidden); return -1; }
    std::vector<float> wf((size_t)hidden * nout_pad, 0.f);
    for (int o = 0; o < nout; o++)
        for (int j = 0; j < hidden; j++)
            wf[(size_t)j * nout_pad + o] = ((float)w.data[(size_t)o * hidden + j] - (float)qw.zp) * qw.scale;
    float* dwf = nullptr;
    if (upload(g, wf, &dwf)) return -1;
    U8FcArgs a{};
    a.x = (const uint8_t*)x.dptr; a.wf = dwf; a.y = (uint8_t*)y.dptr;
    if (upload_bias(g, b, nout, &a.bias)) return -1;
    if (b) a.bias_scale = b->scales.empty() ? 0.f : b->scales[0];      // fc_ref.c:146 bias_tensor->scale
    a.batch = batch; a.hidden = hidden; a.nout = nout; a.nout_pad = nout_pad;
    a.in_scale = qx.scale; a.in_zp = (float)qx.zp; a.out_scale = qy.scale; a.out_zp = qy.zp;
    out->push_back(make_step(n.name, "fc_u8", (double)batch * hidden * nout, 4.0 * hidden * nout + batch * (hidden + nout),
                             [a](hipStream_t s) { return launch_fc_u8(a, s); }, {access_of(x)}, {access_of(y)}, false));
    return 0;
}

// the quantised part of the SSD tail: Reshape -> Softmax(axis 2) -> Flatten on mbox_conf
static int plan_softmax_u8(HNode& n, HTensor& x, HTensor& y, std::vector<Step>* out)
{
    if (x.is_view || y.is_view) { set_error("softmax %s on a concat view is not supported", n.name.c_str()); return -1; }
    AxisSplit sp;
    if (axis_split(x.dims, n.p.softmax.axis, "softmax", n.name, &sp)) return -1;
    U8SoftmaxArgs a{};
    a.x = (const uint8_t*)x.dptr; a.y = (uint8_t*)y.dptr;
    a.outer = sp.outer; a.inner = sp.inner; a.on = sp.on;
    if (q_of(x, &a.in, "tensor") || q_of(y, &a.out, "tensor")) return -1;
    out->push_back(make_step(n.name, "softmax_u8", 0, 2.0 * x.elems(), [a](hipStream_t s) { return launch_softmax_u8(a, s); }, {access_of(x)},
                             {access_of(y)}, false));
    return 0;
}

static int plan_pool_u8(HNode& n, HTensor& x, HTensor& y, std::vector<Step>* out)
{
    PoolGeom pg = pool_geom(n.p.pool, x.h, x.w);
    U8PoolArgs a{};
    a.x = (const uint8_t*)x.dptr; a.y = (uint8_t*)y.dptr;
    a.N = x.n; a.C = x.c; a.H = x.h; a.W = x.w; a.OH = y.h; a.OW = y.w;
    a.KH = pg.kh; a.KW = pg.kw; a.SH = pg.sh; a.SW = pg.sw; a.PH = pg.ph0; a.PW = pg.pw0;
    a.method = n.p.pool.pool_method; a.caffe_flavor = n.p.pool.caffe_flavor;
    if (q_of(x, &a.in, "tensor") || q_of(y, &a.out, "tensor")) return -1;
    out->push_back(make_step(n.name, "pool_u8", 0, (double)x.elems() + (double)y.elems(), [a](hipStream_t s) { return launch_pool_u8(a, s); }, {access_of(x)},
                             {access_of(y)}, false));
    return 0;
}

static int plan_map_u8(HNode& n, HTensor& x, HTensor& y, std::vector<Step>* out)          // ReLU / leaky ReLU, nearest upsample
{
    U8MapArgs a{};
    a.x = (const uint8_t*)x.dptr; a.y = (uint8_t*)y.dptr;
    a.N = x.n; a.C = x.c; a.H = x.h; a.W = x.w;
    a.scale = n.op == TAMD_OP_UPSAMPLE ? (int)n.p.ups.scale : 1;
    a.out_img = nchw_out_img(y); a.out_c0 = y.c_off;
    a.slope = n.op == TAMD_OP_RELU ? n.p.relu.negative_slope : 0.f;
    if (q_of(x, &a.in, "tensor") || q_of(y, &a.out, "tensor")) return -1;
    const bool up = n.op == TAMD_OP_UPSAMPLE;
    out->push_back(make_step(n.name, up ? "upsample_u8" : "relu_u8", 0, (double)x.elems() + (double)y.elems(),
                             [a, up](hipStream_t s) { return up ? launch_upsample_u8(a, s) : launch_relu_u8(a, s); }, {access_of(x)}, {access_of(y)}, false));
    return 0;
}

static int plan_permute_u8(HNode& n, HTensor& x, HTensor& y, std::vector<Step>* out)
{
    if (!permute_order_on_device(n.p.perm.order)) { set_error("permute %s: only order (0,2,3,1) is supported on the device", n.name.c_str()); return -1; }
    U8CatArgs a{};
    a.x = (const uint8_t*)x.dptr; a.y = (uint8_t*)y.dptr;
    a.N = x.dims[0]; a.in_img = (int)(x.elems() / x.dims[0]);
    a.perm_c = x.dims[1]; a.perm_p = x.dims[2] * x.dims[3];
    a.out_img = a.in_img; a.out_off = 0; a.identity = 1;
    a.in.scale = a.out.scale = 1.f;
    out->push_back(make_step(n.name, "permute_u8", 0, 2.0 * x.elems(), [a](hipStream_t s) { return launch_flatcat_u8(a, s); }, {access_of(x)}, {access_of(y)},
                             false));
    return 0;
}

// shapes-only node: evaluated here, once (graph_infer.hip priorbox_eval); no launch at run
static int plan_priorbox_u8(tamd_graph* g, HNode& n, HTensor& x, HTensor& y)
{
    const HTensor& img = g->tensors[n.in[1]];
    U8Q qy;
    if (q_of(y, &qy, "tensor")) return -1;
    std::vector<float> boxes;
    std::vector<uint8_t> q;
    priorbox_eval(n.p.priorbox, x.dims[2], x.dims[3], img.dims[2], img.dims[3], &boxes);
    if (boxes.size() != y.elems()) { set_error("priorbox %s: output shape mismatch", n.name.c_str()); return -1; }
    priorbox_quant_u8(boxes, qy.scale, qy.zp, &q);
    HIPCHK(hipMemcpyAsync(y.dptr, q.data(), q.size(), hipMemcpyHostToDevice, g->stream));
    HIPCHK(hipStreamSynchronize(g->stream));
    y.prerun_const = true;
    return 0;
}

// perm_src[t] >= 0: input t reaches this concat through Permute(0,2,3,1) -> Flatten and is read from perm_src[t] in permuted order
static int plan_concat_u8(tamd_graph* g, HNode& n, const std::vector<int>& perm_src, std::vector<Step>* out)
{
    HTensor& y = g->tensors[n.out[0]];
    // dense tensors: for every index in front of the axis, each input is one contiguous slice of the output's slice
    // (axis 1 of [n][c][...]: one slice per image)
    AxisSplit sp;
    if (axis_split(y.dims, n.p.concat.axis, "concat", n.name, &sp)) return -1;
    const int out_img = sp.on * sp.inner;
    bool all_const = true;
    for (int i : n.in) all_const &= g->tensors[i].prerun_const;
    int off = 0;
    U8CatMulti multi{};
    std::vector<Step> each;                // one launch per copied input
    for (int i : n.in) {
        HTensor& x = g->tensors[i];
        const int in_img = x.dims[sp.axis] * sp.inner;
        if (x.is_view && x.dptr == y.dptr) { off += in_img; continue; }       // written in place by its producer
        U8CatArgs a{};
        a.x = (const uint8_t*)x.dptr; a.y = (uint8_t*)y.dptr;
        a.N = sp.outer; a.in_img = in_img; a.out_img = out_img; a.out_off = off;
        if (q_of(x, &a.in, "tensor") || q_of(y, &a.out, "tensor")) return -1;
        // roundf((u - zp) * 1 + zp) == u: equal parameters make the rescale a copy
        // (.. and a SINGLE input is copied byte for byte whatever the quantisation says: concat_kernel_ref_uint8.c:47-58 --
        //  round 6, found by tools/fuzz_heads.py on the int8 twin of this rule)
        a.identity = (a.in.scale == a.out.scale && a.in.zp == a.out.zp) || n.in.size() == 1;
        const char* kname = "concat_u8";
        if (perm_src[i] >= 0) {                                  // Permute(0,2,3,1) -> Flatten -> this concat
            HTensor& s = g->tensors[perm_src[i]];
            a.x = (const uint8_t*)s.dptr; a.perm_c = s.dims[1]; a.perm_p = s.dims[2] * s.dims[3];
            kname = "permute_concat_u8";
        }
        // reads its source, writes ITS slot of every outer slice
        Step st = make_step(n.name, kname, 0, 2.0 * x.elems(), [a](hipStream_t s) { return launch_flatcat_u8(a, s); },
                            {access_of(perm_src[i] >= 0 ? g->tensors[perm_src[i]] : x)}, {access_of_slot(y, out_img, off, in_img, 1)}, !y.is_view);
        st.once = all_const;                                     // e.g. mbox_priorbox: PriorBox outputs only
        each.push_back(st);
        if (multi.count < 8) { multi.src[multi.count] = a; multi.rescale[multi.count] = a.in.scale / a.out.scale; }
        multi.count++;
        off += in_img;
    }
    y.prerun_const = all_const;
    // two to eight copied inputs (the SSD heads: six per concat): one launch for all of them (TAMD_FUSE_CONCAT=0: one each)
    const char* fc_env = getenv("TAMD_FUSE_CONCAT");
    if (!(multi.count >= 2 && multi.count <= 8 && !all_const && !y.is_view && !(fc_env && atoi(fc_env) == 0))) {
        out->insert(out->end(), each.begin(), each.end());
        return 0;
    }
    Step st = each[0];
    st.kernel = each[0].kernel + "<x" + std::to_string(multi.count) + ">";
    st.bytes = 0; st.rd.clear(); st.wr.clear();
    for (const Step& e : each) {
        st.bytes += e.bytes;
        st.rd.insert(st.rd.end(), e.rd.begin(), e.rd.end());
        st.wr.insert(st.wr.end(), e.wr.begin(), e.wr.end());
        if (e.kernel != each[0].kernel) st.kernel = "concat_u8<x" + std::to_string(multi.count) + ">";
    }
    st.fn = [multi](hipStream_t s) { return launch_flatcat_multi_u8(multi, s); };
    out->push_back(st);
    return 0;
}

// the scalar and unary forms: one lut_u8 launch by table (plan_eltwise_table); the same-shape form: eltwise_u8; the channel-gate form x (N, C, H, W) op gate (N, C, 1, 1): plan_chan_gate (graph_plan_maps.hip), with the
// byte map in front of the gate (node lut_node, -1: none) inside the launch
static int plan_eltwise_u8(tamd_graph* g, HNode& n, int lut_node, std::vector<Step>* out)
{
    int gated = -1;
    const char* why = eltwise_refusal_of(g, n, &gated);
    if (why) { set_error("eltwise %s: %s", n.name.c_str(), why); return -1; }
    if (gated == kEltScalar || gated == kEltUnary) return plan_eltwise_table(g, n, out);
    if (gated >= 0) return plan_chan_gate(g, n, gated, lut_node, out);
    HTensor& xa = g->tensors[n.in[0]];
    HTensor& xb = g->tensors[n.in[1]];
    HTensor& y = g->tensors[n.out[0]];
    if (xa.dims != xb.dims) { set_error("eltwise %s: broadcast not supported", n.name.c_str()); return -1; }
    U8EltArgs a{};
    a.a = (const uint8_t*)xa.dptr; a.b = (const uint8_t*)xb.dptr; a.y = (uint8_t*)y.dptr;
    a.count = xa.elems(); a.type = n.p.elt.type;
    if (!eltwise_type_on_device(a.type)) { set_error("eltwise %s: type %d unsupported", n.name.c_str(), a.type); return -1; }
    if (q_of(xa, &a.qa, "tensor") || q_of(xb, &a.qb, "tensor") || q_of(y, &a.out, "tensor")) return -1;
    out->push_back(make_step(n.name, "eltwise_u8", 0, 3.0 * xa.elems(), [a](hipStream_t s) { return launch_eltwise_u8(a, s); }, {access_of(xa), access_of(xb)},
                             {access_of(y)}, false));
    return 0;
}

// ---- the fusion scans: each returns what it found ----

// SSD heads (MobileNet-SSD: 12 of them): conv -> Permute(0,2,3,1) -> Flatten -> Concat.  The permute and the
// flatten only re-index bytes, so the concat reads the conv result in permuted order itself: perm_src[flatten
// output] = the permute's input, and the permute launch disappears -- skip_perm[its node] (TAMD_FUSE_PERMUTE=0 keeps it)
static std::vector<int> find_permute_concats(const tamd_graph* g, std::vector<char>* skip_perm)
{
    std::vector<int> perm_src(g->tensors.size(), -1);
    skip_perm->assign(g->nodes.size(), 0);
    const char* pe = getenv("TAMD_FUSE_PERMUTE");
    if (pe && atoi(pe) == 0) return perm_src;
    for (size_t pi = 0; pi < g->nodes.size(); pi++) {
        const HNode& pn = g->nodes[pi];
        if (pn.op != TAMD_OP_PERMUTE || !permute_order_on_device(pn.p.perm.order)) continue;
        if (count_consumers(g, pn.out[0]) != 1) continue;
        const HNode* fl = nullptr;
        for (auto& m : g->nodes)
            if (m.op == TAMD_OP_FLATTEN && m.in[0] == pn.out[0]) fl = &m;
        if (!fl || count_consumers(g, fl->out[0]) != 1) continue;
        bool to_concat = false;
        for (auto& m : g->nodes)
            if (m.op == TAMD_OP_CONCAT)
                for (int i : m.in) to_concat |= (i == fl->out[0]);
        if (!to_concat) continue;
        perm_src[fl->out[0]] = pn.in[0];
        (*skip_perm)[pi] = 1;
    }
    return perm_src;
}

// conv -> ReLU / leaky ReLU fusion (YOLOv3-tiny: 11 of them): the ReLU node is applied to the conv's own uint8
// result in the conv epilogue when nothing else reads that result.  The ReLU node's index, -1: none
static int find_fused_relu(const tamd_graph* g, size_t ni)
{
    const char* fuse_env = getenv("TAMD_FUSE_RELU");          // read at every prerun (tests switch it)
    const HNode& n = g->nodes[ni];
    if (!(fuse_env && atoi(fuse_env) == 0) && count_consumers(g, n.out[0]) == 1)
        for (size_t nj = ni + 1; nj < g->nodes.size(); nj++)
            if (g->nodes[nj].op == TAMD_OP_RELU && g->nodes[nj].in[0] == n.out[0]) return (int)nj;
    return -1;
}

// conv (-> ReLU) -> 2x2 stride-2 max-pool (YOLOv3-tiny: conv0..conv3): the pool is applied to the final
// bytes in the conv epilogue -- the window's four pixels are computed by four neighbouring lanes -- when the map is
// even-sized and has no reference "tail" pixels (OH*OW % 8 == 0); TAMD_FUSE_POOL=0 keeps the pool_u8 launch.
// `full`: the tensor the pool reads (the conv's or its fused ReLU's output).  The pool node's index, -1: none
static int find_fused_pool(const tamd_graph* g, size_t ni, int full, const std::vector<char>& fused)
{
    const char* pool_env = getenv("TAMD_FUSE_POOL");         // read at every prerun (tests switch it)
    const HTensor& yf = g->tensors[full];
    if (!(pool_env && atoi(pool_env) == 0) && yf.dims.size() == 4
        && yf.h % 2 == 0 && yf.w % 2 == 0 && (yf.h * yf.w) % 8 == 0 && !yf.is_view)
        for (size_t nj = ni + 1; nj < g->nodes.size(); nj++) {
            const HNode& m = g->nodes[nj];
            if (m.op != TAMD_OP_POOL || m.in[0] != full || fused[nj]) continue;
            const PoolGeom pg = pool_geom(m.p.pool, yf.h, yf.w);
            if (m.p.pool.pool_method == 0 && pg.kh == 2 && pg.kw == 2 && pg.sh == 2 && pg.sw == 2 && pg.ph0 == 0 && pg.pw0 == 0
                && pg.oh == yf.h / 2 && pg.ow == yf.w / 2) return (int)nj;
        }
    return -1;
}

// a conv node and the ReLU / max-pool nodes behind it that its launch carries: those are marked in `fused`
static int plan_conv_node_u8(tamd_graph* g, size_t ni, std::vector<char>* fused, std::vector<Step>* out)
{
    HNode& n = g->nodes[ni];
    int rj = find_fused_relu(g, ni);
    int pj = find_fused_pool(g, ni, rj >= 0 ? g->nodes[rj].out[0] : n.out[0], *fused);
    // what the kernel this conv gets cannot carry stays a launch of its own: the pool first, then the ReLU
    const U8Tail can = conv_u8_tail(g, n);
    if (!can.pool) pj = -1;
    if (!can.relu) rj = -1;
    const HNode* relu = rj >= 0 ? &g->nodes[rj] : nullptr;
    const HNode* pool = pj >= 0 ? &g->nodes[pj] : nullptr;
    if (plan_conv_u8(g, n, relu, pool, out)) return -1;
    // tensors that now only exist inside the fused launch: tamd_graph_read_tensor must refuse them instead of returning the
    // zeros of a buffer nobody writes (layer-by-layer parity tooling would be misled)
    if (g->fused_away.size() != g->tensors.size()) g->fused_away.assign(g->tensors.size(), 0);
    if (relu) { (*fused)[rj] = 1; g->fused_away[n.out[0]] = 1; }
    if (pool) {
        (*fused)[pj] = 1;
        const int full = relu ? relu->out[0] : n.out[0];
        bool written = count_consumers(g, full) > 1;           // == U8PoolFuse::write_full
        for (auto& io : g->outputs) written = written || io.tensor == full;
        if (!written) g->fused_away[full] = 1;
    }
    return 0;
}

int plan_u8(tamd_graph* g)
{
    // concat-by-offset: when an input carries the concat output's (scale, zero point) the reference's per-element rescale
    // roundf((u - zp) * 1 + zp) is the identity (concat_kernel_ref_uint8.c:309-352), so a conv / relu / upsample / interp / depthtospace / resize whose only
    // consumer is that concat writes in place
    if (plan_nchw_buffers(g, 1, [](const HNode& pn, const HTensor& xi, const HTensor& y) {
            return (pn.op == TAMD_OP_CONV || pn.op == TAMD_OP_RELU || pn.op == TAMD_OP_UPSAMPLE || pn.op == TAMD_OP_INTERP || pn.op == TAMD_OP_DEPTHTOSPACE || pn.op == TAMD_OP_RESIZE) && !xi.scales.empty() && !y.scales.empty()
                   && xi.scales[0] == y.scales[0] && (xi.zps.empty() ? 0 : xi.zps[0]) == (y.zps.empty() ? 0 : y.zps[0]);
        }))
        return -1;
    std::vector<char> skip_perm;
    const std::vector<int> perm_src = find_permute_concats(g, &skip_perm);
    std::vector<char> fused(g->nodes.size(), 0);          // ReLU / pool nodes that the conv in front of them carries
    // byte map -> channel-gate Eltwise as one launch (gate_lut_producer): gate_lut[eltwise node] = the byte map's node + 1, which is skipped
    std::vector<int> gate_lut(g->nodes.size(), 0);
    for (size_t ei = 0; ei < g->nodes.size(); ei++) {
        int gated = -1;
        if (g->nodes[ei].op != TAMD_OP_ELTWISE || eltwise_refusal_of(g, g->nodes[ei], &gated) || gated < 0) continue;
        const int pj = gate_lut_producer(g, g->nodes[ei], gated);
        if (pj >= 0 && pj < (int)ei) { gate_lut[ei] = pj + 1; fused[pj] = 1; }
    }
    // Slice -> Slice as one launch (slice_chain_next): slice_next[first] = the second's node + 1, which is skipped
    std::vector<int> slice_next(g->nodes.size(), 0);
    for (size_t si = 0; si < g->nodes.size(); si++) {
        if (g->nodes[si].op != TAMD_OP_SLICE || fused[si]) continue;
        const int nj = slice_chain_next(g, si);
        if (nj > (int)si && !fused[nj]) { slice_next[si] = nj + 1; fused[nj] = 1; }
    }
    // Interp -> Crop as one launch at the Crop's position (crop_interp_producer): crop_interp[crop] = the Interp's node + 1, which is skipped;
    // and, with TAMD_PIN=topdown=1, that chain -> Eltwise as one launch at the ELTWISE's position, where its other operand is made (crop_topdown_next):
    // topdown[eltwise] = the Crop's node + 1, which is skipped too
    std::vector<int> crop_interp(g->nodes.size(), 0), topdown(g->nodes.size(), 0);
    for (size_t ci = 0; ci < g->nodes.size(); ci++) {
        if (g->nodes[ci].op != TAMD_OP_CROP || fused[ci]) continue;
        const int pj = crop_interp_producer(g, ci);
        if (pj < 0 || fused[pj]) continue;
        crop_interp[ci] = pj + 1; fused[pj] = 1;
        const int ej = crop_topdown_next(g, ci);
        if (ej > (int)ci && !fused[ej] && !gate_lut[ej] && !topdown[ej]) { topdown[ej] = (int)ci + 1; fused[ci] = 1; }
    }
    // InstanceNorm -> ReLU as the InstanceNorm's launches (instancenorm_relu_next): in_relu[instancenorm node] = the ReLU's node + 1, which is skipped
    std::vector<int> in_relu(g->nodes.size(), 0);
    for (size_t ni = 0; ni < g->nodes.size(); ni++) {
        const int rj = instancenorm_relu_next(g, ni);
        if (rj > (int)ni && !fused[rj]) { in_relu[ni] = rj + 1; fused[rj] = 1; }
    }
    // byte-pure chains (bytemap_chain_from, graph_plan_maps.hip) as one lut_u8 launch each at the LAST member's position:
    // chain_at[last member] = the chain's index + 1, the other members are skipped.  Every tensor owns its buffer here: only views are out
    std::vector<ByteChain> chains;
    std::vector<int> chain_at(g->nodes.size(), 0);
    for (size_t ni = 0; ni < g->nodes.size(); ni++) {
        ByteChain c;
        if (!bytemap_chain_from(g, ni, [&](int k) { return !fused[k] && !gate_lut[k] && !slice_next[k] && !crop_interp[k] && !topdown[k] && !chain_at[k]; },
                                [&](int t) { return g->tensors[t].ttype != TAMD_TT_CONST && !g->tensors[t].is_view; }, &c))
            continue;
        for (size_t k = 0; k + 1 < c.nodes.size(); k++) fused[c.nodes[k]] = 1;
        chains.push_back(c);
        chain_at[c.nodes.back()] = (int)chains.size();
    }
    for (size_t ni = 0; ni < g->nodes.size(); ni++) {
        HNode& n = g->nodes[ni];
        if (fused[ni]) continue;
        if (chain_at[ni]) {
            std::vector<Step> one;
            if (plan_bytemap_chain(g, chains[chain_at[ni] - 1], &one) || append_steps(g, one)) return -1;
            continue;
        }
        if (n.op == TAMD_OP_INPUT || n.op == TAMD_OP_CONST || n.op == TAMD_OP_DROPOUT || n.op == TAMD_OP_FLATTEN || n.op == TAMD_OP_RESHAPE) continue;
        HTensor& x = g->tensors[n.in[0]];
        HTensor& y = g->tensors[n.out[0]];
        std::vector<Step> out;                             // the node's launches: the only thing that goes onto g->steps (append_steps)
        int rc = 0;
        switch (n.op) {
        case TAMD_OP_SOFTMAX: rc = plan_softmax_u8(n, x, y, &out); break;
        case TAMD_OP_CONV: rc = plan_conv_node_u8(g, ni, &fused, &out); break;
        case TAMD_OP_FC: rc = plan_fc_u8(g, n, &out); break;
        case TAMD_OP_POOL: rc = plan_pool_u8(n, x, y, &out); break;
        case TAMD_OP_RELU: case TAMD_OP_UPSAMPLE: rc = plan_map_u8(n, x, y, &out); break;
        // the byte-map planners both quantised graphs share (graph_plan_maps.hip): tables, index vectors and plane maps at prerun
        case TAMD_OP_SIGMOID: case TAMD_OP_CLIP: case TAMD_OP_HARDSWISH: case TAMD_OP_MISH: rc = plan_lut(g, n, &out); break;
        case TAMD_OP_INTERP: rc = plan_interp(g, n, &out); break;
        case TAMD_OP_RESIZE: rc = plan_resize(g, n, &out); break;      // one launch: interp_nearest_u8 with Resize's operands, or resize_rep_u8 (resize.hip)
        case TAMD_OP_SPLIT: rc = plan_split_u8(g, n, &out); break;      // one chan_map_u8 launch per output
        case TAMD_OP_SHUFFLECHANNEL: rc = plan_shuffle_u8(g, n, &out); break;
        case TAMD_OP_SLICE: rc = plan_slice_u8(g, n, slice_next[ni] - 1, &out); break;      // one slice_u8 launch, the Slice behind it inside
        case TAMD_OP_TRANSPOSE: rc = plan_transpose(g, n, -1, &out); break;      // one launch; the Reshapes around it are views
        case TAMD_OP_DEPTHTOSPACE: rc = plan_depthtospace(g, n, false, &out); break;      // one d2s_u8 launch (d2s.hip)
        case TAMD_OP_CROP:                                      // alone: slice_u8 over the box; behind a nearest Interp: that launch, shifted
            rc = crop_interp[ni] ? plan_interp(g, g->nodes[crop_interp[ni] - 1], &out, &n) : plan_crop_u8(g, n, &out);
            break;
        case TAMD_OP_PRELU: rc = plan_prelu(g, n, &out); break;
        case TAMD_OP_INSTANCENORM: rc = plan_instancenorm_u8(g, n, in_relu[ni] ? &g->nodes[in_relu[ni] - 1] : nullptr, &out); break;      // instnorm.hip: two launches, or one
        case TAMD_OP_BATCHNORM: rc = plan_batchnorm_u8(g, n, &out); break;      // chan_lut_u8, or prelu_u8's per-plane form on large planes
        case TAMD_OP_PERMUTE:
            if (!skip_perm[ni]) rc = plan_permute_u8(n, x, y, &out);      // else folded into the concat that reads it
            break;
        case TAMD_OP_PRIORBOX: rc = plan_priorbox_u8(g, n, x, y); break;
        case TAMD_OP_CONCAT: rc = plan_concat_u8(g, n, perm_src, &out); break;
        case TAMD_OP_ELTWISE:
            if (topdown[ni]) {                                  // Interp -> Crop -> this node: one topdown_u8 launch
                HNode& cn = g->nodes[topdown[ni] - 1];
                rc = plan_topdown_u8(g, g->nodes[crop_interp[topdown[ni] - 1] - 1], cn, n, &out);
            } else {
                rc = plan_eltwise_u8(g, n, gate_lut[ni] - 1, &out);
            }
            break;
        default:
            set_error("op %d (%s) is not supported on the device for uint8", n.op, n.name.c_str());
            rc = -1;
        }
        if (rc || append_steps(g, out)) return -1;
    }
    return plan_nchw_outputs(g, 1);
}

}  // namespace tamd
