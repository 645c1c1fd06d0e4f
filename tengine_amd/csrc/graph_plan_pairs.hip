// int8 planner, the pair fusions: pointwise conv + its single consumer (depthwise 3x3 | global pooling) in one launch (pwdw.hip), and
// depthwise 3x3 + the pointwise conv behind it (dwpw.hip); two adjacent pwdw pairs as one launch (chain4.hip); and the one triple: an
// identity bottleneck block (block_i8.hip).
#include "graph.h"
#include "graph_internal.h"
#include "env.h"

#include <stdio.h>

#include <algorithm>
#include <cmath>

#include "block_pack.h"
#include "epilogue.h"
#include "graph_plan.h"

namespace tamd {

// ---- pointwise conv + its single consumer (depthwise 3x3 | global pooling) in one launch: pwdw.hip ---------------------
// Which node, if any, can ride in pointwise conv `ni`'s launch.  *tmode: 1 depthwise 3x3, 0 global pooling.
int find_pwdw_tail(tamd_graph* g, size_t ni, int* tmode, int* prod)
{
    const HNode& n = g->nodes[ni];
    if (n.op != TAMD_OP_CONV || n.in.size() < 2) return -1;
    const tamd_conv_param& p = n.p.conv;
    const HTensor& x = g->tensors[n.in[0]];
    const HTensor& y = g->tensors[n.out[0]];
    if (p.group != 1 || y.is_view || x.dtype != TAMD_DT_INT8) return -1;
    if (x.nchw_raw) {
        // the network's first conv, gathered from the NCHW graph input: patch rows of 4 consecutive bytes (KW <= 4, no
        // x dilation), at most 16 rows (c, ky) = one 64-deep K step; row offsets of 24 bits, ky*DH of 4
        if (x.c > 4 || p.kernel_w > 4 || p.dilation_w != 1 || x.c * p.kernel_h > 16 || p.dilation_h * (p.kernel_h - 1) > 15
            || (long)x.c * x.h * x.w >= (1L << 24) || p.pad_h0 < 0 || p.pad_w0 < 0)
            return -1;
        *prod = 1;
    } else {
        if (p.kernel_h != 1 || p.kernel_w != 1 || p.stride_h != 1 || p.stride_w != 1 || p.pad_h0 || p.pad_h1 || p.pad_w0 || p.pad_w1) return -1;
        *prod = 0;
    }
    const int nj = sole_reader(g, n.out[0]);
    if (nj < 0) return -1;
    const HNode& c = g->nodes[nj];
    const HTensor& o = g->tensors[c.out[0]];
    if (c.op == TAMD_OP_CONV && c.in.size() >= 2) {
        const tamd_conv_param& q = c.p.conv;
        const bool dw3 = is_dw3x3(q, y.c, o.c) && q.pad_h0 >= 0 && q.pad_w0 >= 0 && q.pad_h0 <= 2 && q.pad_w0 <= 2;
        if (!dw3 || o.scales.empty() || g->tensors[c.in[1]].scales.empty()) return -1;
        *tmode = 1;
        return nj;
    }
    if (c.op == TAMD_OP_POOL && *prod == 0) {
        const PoolGeom pg = pool_geom(c.p.pool, y.h, y.w);
        const int m = c.p.pool.pool_method;
        if (pg.oh != 1 || pg.ow != 1 || pg.kh != y.h || pg.kw != y.w || pg.ph0 || pg.pw0 || (m != 0 && m != 1) || y.h * y.w > 1024 || o.scales.empty())
            return -1;
        *tmode = 0;
        return nj;
    }
    return -1;
}

// the incumbent of a fusion race: the pair's two planned steps, launched back to back
static RaceCand two_launches(const std::string& tag, const Step& sa, const Step& sb)
{
    const std::function<hipError_t(hipStream_t)> fa = sa.fn, fb = sb.fn;
    return {tag, [fa, fb](hipStream_t s) { const hipError_t e = fa(s); return e != hipSuccess ? e : fb(s); }, sa.kernel + " + " + sb.kernel};
}

// ---- what plan_pwdw and plan_chain4 share ------------------------------------------------------------------------------------------
// The depthwise 3x3 launch `p` planned for node `dn` of C channels: its kernel arguments hold the taps, the bias and the requantisation
// that plan_conv folded (conv_mode at the graph's batch) and uploaded -- DwArgs::w / bias / wscale / rq, rows of rup(C, 16) channels --
// and a fused launch reads those.  null: not planned in that form, or a weight / bias tensor of the wrong size (plan_conv does not look)
static const DwArgs* planned_dw(tamd_graph* g, const HNode& dn, const Planned& p, int C)
{
    const HTensor& w = g->tensors[dn.in[1]];
    const HTensor* b = dn.in.size() > 2 ? &g->tensors[dn.in[2]] : nullptr;
    if (p.kind != Planned::DW3X3 || w.elems() != (size_t)C * 9 || (b && b->elems() < (size_t)C)) return nullptr;
    return &p.dw;
}

// The producer that is the network's first convolution (prod 1; find_pwdw_tail checked its limits), for PwDwArgs | Chain4Args: the
// weight rows as the kernels walk them in *wrows -- [C][cin*KH*4], k = (c*KH + ky)*4 + kx, a patch row padded to 4 taps -- the 16-entry
// row table (c, ky) -> (c*H*W + ky*DH*W) | ky*DH << 28 uploaded (a->taps), and the geometry of the NCHW input
template <typename Args>
static int first_conv_producer(tamd_graph* g, const HTensor& x, const HTensor& w, const tamd_conv_param& pp, int C, std::vector<int8_t>* wrows, Args* a)
{
    const int nrows = x.c * pp.kernel_h, Kw = nrows * pp.kernel_w, K = nrows * 4;
    const int8_t* wd = (const int8_t*)w.data.data();
    wrows->assign((size_t)C * K, 0);
    for (int c = 0; c < C; c++)
        for (int r = 0; r < nrows; r++)
            for (int kx = 0; kx < pp.kernel_w; kx++) (*wrows)[(size_t)c * K + r * 4 + kx] = wd[(size_t)c * Kw + r * pp.kernel_w + kx];
    std::vector<unsigned> rows(16, 0u);
    for (int r = 0; r < nrows; r++) {
        const int ky = r % pp.kernel_h, ci = r / pp.kernel_h;
        rows[r] = (unsigned)(ci * x.h * x.w + ky * pp.dilation_h * x.w) | ((unsigned)(ky * pp.dilation_h) << 28);
    }
    unsigned* dt;
    if (upload(g, rows, &dt)) return -1;
    a->taps = dt; a->in_C = x.c; a->in_H = x.h; a->in_W = x.w;
    a->fSH = pp.stride_h; a->fSW = pp.stride_w; a->fPH = pp.pad_h0; a->fPW = pp.pad_w0;
    return 0;
}

// TAMD_PIN=<key>=THxTWxthreads[xSL] (tests): the pinned tile, clamped to the OH x OW map; *sl = 1 where none is given.  false: no such pin
static bool pinned_tile(const char* key, int OH, int OW, int* th, int* tw, int* threads, int* sl)
{
    const char* pin = tamd_pin(key);
    *sl = 1;
    if (!pin || sscanf(pin, "%dx%dx%dx%d", th, tw, threads, sl) < 3) return false;
    *th = std::min(*th, OH); *tw = std::min(*tw, OW);
    return *th >= 1 && *tw >= 1;
}

// The two nodes were just planned as `pa` (the pointwise conv) and `pb` (its tail); build the fused launch, and keep whichever is
// faster (plan-time measurement; without autotune: fuse the small-map cases where launches, not bytes, are the cost).  The producer's
// constants are folded here (a first conv of more than 128 outputs is planned as a generic direct launch and keeps none), the
// depthwise tail's are the ones `pb` uploaded.
// TAMD_FUSE_PWDW=0 never fuses, =2 always fuses; TAMD_PWDW_CFG="TH,TW,threads" pins the tile configuration (tests).
int plan_pwdw(tamd_graph* g, HNode& pw, HNode& tl, int tmode, int prod, const Planned& pa, const Planned& pb, Step* fused)
{
    const char* fenv = getenv("TAMD_FUSE_PWDW");                 // read at every prerun
    const int fmode = fenv ? atoi(fenv) : 1;
    if (fmode == 0) return 0;
    HTensor& x = g->tensors[pw.in[0]];
    HTensor& w = g->tensors[pw.in[1]];
    HTensor* b = pw.in.size() > 2 ? &g->tensors[pw.in[2]] : nullptr;
    HTensor& mid = g->tensors[pw.out[0]];
    HTensor& y = g->tensors[tl.out[0]];
    const tamd_conv_param& pp = pw.p.conv;
    const int cin = x.c, C = mid.c, slices = (C + 15) / 16, cw = slices * 16;
    const int Kw = prod == 1 ? cin * pp.kernel_h * pp.kernel_w : cin;           // weight row length in the model
    const int K = prod == 1 ? cin * pp.kernel_h * 4 : cin;                      // reduction length as the kernel walks it
    const int ktot = prod == 1 ? K : rup(cin, 16), steps = pwdw_steps((ktot + 63) / 64), nsteps = rup((ktot + 63) / 64, steps);
    if (w.elems() != (size_t)C * Kw || (b && b->elems() < (size_t)C)) return 0;
    const DwArgs* dwp = tmode == 1 ? planned_dw(g, tl, pb, C) : nullptr;
    if (tmode == 1 && !dwp) return 0;
    PwDwArgs a{};
    {
        const RqFold rq = fold_requant(RQ_CONV_HCL, pp.activation, x.scales[0], mid.scales[0], w, C);
        const int8_t* wd = (const int8_t*)w.data.data();
        std::vector<int8_t> wrows;
        if (prod == 1) {
            if (first_conv_producer(g, x, w, pp, C, &wrows, &a)) return -1;
            wd = wrows.data();
        }
        const std::vector<int8_t> wf = pack_pw_panel(wd, C, K, nsteps);
        const std::vector<int32_t> bp = padded_bias(b ? (const int32_t*)b->data.data() : nullptr, C, cw);
        int8_t* d0; int32_t* d1;
        if (upload(g, wf, &d0) || upload(g, bp, &d1) || upload_rq(g, rq, cw, &a.wscale, &a.rq)) return -1;
        a.wf = d0; a.bias = d1;
    }
    a.prod = prod;
    a.coherent = (g->opt.direct_dispatch && !exp_plain_kernels()) ? 1 : 0;
    // the larger operand is the one every XCD should fetch only its share of (pwdw.hip: block -> XCD mapping)
    a.tile_major = (double)x.h * x.w * (prod == 1 ? x.c : x.cs) * (slices >= 8 ? 8 : slices) > (double)C * ktot * 8.0 ? 1 : 0;
    if (slices > 65535) a.tile_major = 0;
    a.x = (const int8_t*)x.dptr + (prod == 1 ? 0 : x.c_off);
    a.N = x.n; a.H = mid.h; a.W = mid.w; a.cs_in = x.cs; a.ktot = ktot; a.nsteps = nsteps; a.steps = steps;
    a.mode = tmode; a.cw = cw; a.slices = slices;
    a.y = (int8_t*)y.dptr; a.ldc = y.cs; a.c_off = y.c_off;
    a.c_limit = store_limit(y, C);
    a.S = 1; a.OH = a.OW = 1; a.TH = a.TW = 1; a.tiles_x = a.tiles_y = 1; a.RH = mid.h; a.RW = mid.w;
    if (tmode == 1) {
        a.dw_w = dwp->w; a.dw_bias = dwp->bias; a.dw_wscale = dwp->wscale; a.d_rq = dwp->rq;
        a.S = dwp->S; a.PH = dwp->PH; a.PW = dwp->PW; a.OH = dwp->OH; a.OW = dwp->OW;
    } else {
        a.pool_method = tl.p.pool.pool_method; a.p_in_scale = mid.scales[0]; a.p_out_scale = y.scales[0];
    }

    // ---- tile configurations: (TH, TW, threads) ranked by a small cost model, the best few timed on the device ---------
    struct Cfg { int th, tw, threads; double cost; int sl; };      // sl: 16-channel slices per block (pwdw.hip)
    std::vector<Cfg> cfgs;
    auto with_tiles = [&](PwDwArgs v, int th, int tw, int sl = 1) {
        v.TH = th; v.TW = tw; v.tiles_y = (v.OH + th - 1) / th; v.tiles_x = (v.OW + tw - 1) / tw;
        v.RH = (th - 1) * v.S + 3; v.RW = (tw - 1) * v.S + 3;
        v.sl = sl; v.slices = (slices + sl - 1) / sl;
        return v;
    };
    if (tmode == 0) {
        cfgs.push_back({1, 1, 256, 0.0, 1});
        cfgs.push_back({1, 1, 512, 1.0, 1});
    } else {
        std::vector<int> ths, tws;
        for (int v : {1, 2, 3, 4, 5, 6, 7, 8, 10, 12, 14, 16, 28, a.OH}) if (v <= a.OH && std::find(ths.begin(), ths.end(), v) == ths.end()) ths.push_back(v);
        for (int v : {4, 6, 7, 8, 14, 16, 28, 56, a.OW}) if (v <= a.OW && std::find(tws.begin(), tws.end(), v) == tws.end()) tws.push_back(v);
        for (int th : ths)
            for (int tw : tws)
                for (int threads : {256, 512})
                  for (int sl : {1, 2, 4}) {
                    if (sl > 1 && (slices % sl != 0 || nsteps > steps)) continue;
                    const PwDwArgs v = with_tiles(a, th, tw, sl);
                    if (!pwdw_config_ok(v, threads)) continue;
                    // two slices per block halve the grid: offered where two blocks per CU remain (the batched early layers it is for;
                    // a batch-1 launch is a latency chain, its blocks must stay many and short)
                    if (sl > 1 && (double)a.N * v.tiles_y * v.tiles_x * v.slices < 512.0) continue;
                    // instruction slots of the busiest wave (a lone wave issues one instruction per 4 cycles): pointwise tiles
                    // (address + K steps + requantisation) and depthwise tasks, on top of a fixed prologue
                    const int nw = threads / 64;
                    const double vp = (double)std::min(v.RH, a.H) * std::min(v.RW, a.W);
                    const double tiles_w = std::ceil(std::ceil(vp / 16.0) / nw);
                    const int twl = a.S == 1 ? 2 : 1;
                    const double tasks_t = std::ceil((double)th * ((tw + twl - 1) / twl) * 4.0 * sl / threads);
                    // (a second slice repeats the K steps and the requantisation of a tile, not its address arithmetic, load and loop control)
                    const double block = 250.0 + tiles_w * (45.0 + sl * (25.0 + 3.0 * nsteps)) + tasks_t * (a.S == 1 ? 150.0 : 100.0) + vp * ktot / 400.0;
                    const double blocks = (double)a.N * v.tiles_y * v.tiles_x * v.slices;
                    const double rounds = std::ceil(blocks / (256.0 * (threads == 256 ? 2 : 1)));
                    cfgs.push_back({th, tw, threads, rounds * block * (threads == 256 && blocks > 256 ? 1.3 : 1.0), sl});
                }
        std::sort(cfgs.begin(), cfgs.end(), [](const Cfg& l, const Cfg& r) { return l.cost < r.cost; });
        // the best few of EACH block width go to the device: the model ranks within a width, the race decides between them
        std::vector<Cfg> keep;
        for (int sl : {1, 2, 4}) {
            int n = 0;
            for (auto& c : cfgs)
                if (c.sl == sl && n < (sl == 1 ? 8 : 6)) { keep.push_back(c); n++; }
        }
        cfgs = keep;
    }
    int pth = 0, ptw = 0, pthreads = 0, psl = 1;      // "THxTWxthreads" or "THxTWxthreadsx2" / "..x4" (two / four slices per block)
    if (tmode == 1 && pinned_tile("pwdw_cfg", a.OH, a.OW, &pth, &ptw, &pthreads, &psl)) {
        if ((psl != 2 && psl != 4) || slices % psl != 0 || nsteps > steps) psl = 1;
        if (pwdw_config_ok(with_tiles(a, pth, ptw, psl), pthreads)) { cfgs.clear(); cfgs.push_back({pth, ptw, pthreads, 0.0, psl}); }
    } else if (tmode == 0 && pinned_tile("pwdw_cfg", a.OH, a.OW, &pth, &ptw, &pthreads, &psl) && pwdw_config_ok(a, pthreads)) {
        cfgs.clear(); cfgs.push_back({1, 1, pthreads, 0.0, 1});      // a pooling tail has no tile: the pin picks the block width (tests)
    }
    if (cfgs.empty()) return 0;
    const Step& sa = pa.step;
    const Step& sb = pb.step;
    const bool autotune = autotune_enabled() && sa.macs >= 4e6;
    // fused by construction (no race): a link of a LATENCY chain only -- batch 1.  Everything batched keeps the race against the two-launch
    // plan below (batch 8 at 56x56 or batch 16 at 19x19 are throughput launches; round 6's first evidence pass showed what the
    // wider rule costs where the race is skipped: MobileNet-v1 b64's 7x7 tail fused by construction ran conv6/sep + pool6 in 34.9 us
    // against 9.9 + 3.5 us as two launches, and conv5_6/sep + conv6/dw in 18.5 against 7.5 + 5.8 -- 287 instead of 265 us per step)
    bool fuse = fmode == 2 || (a.N == 1 && (double)a.N * a.H * a.W <= 32768.0);
    // cost model inputs below use the map the tail reads (a.H x a.W) and the reduction depth
    char ckey[256];
    snprintf(ckey, sizeof(ckey), "pwdw|%s|n%d %dx%d k%d m%d f%d c%zu", sa.node.c_str(), a.N, a.H, a.W, a.ktot, tmode, fmode, cfgs.size());
    // one entry "<fuse>,<cfg>" answers both races below: "1,<c>" the fused launch in tile configuration c, which must still launch
    // here (a cached index is only as good as the file it came from), "0,<c>" two launches
    std::vector<RaceCand> tiles, answers;
    for (size_t c = 0; c < cfgs.size(); c++) {
        const PwDwArgs v = tmode == 1 ? with_tiles(a, cfgs[c].th, cfgs[c].tw, cfgs[c].sl) : a;
        const int threads = cfgs[c].threads;
        hipStream_t stream = g->stream;
        tiles.push_back({"1," + std::to_string(c), [v, threads](hipStream_t s) { return launch_pwdw(v, threads, s); }, "pwdw cfg " + std::to_string(c),
                         [v, threads, stream]() {
                             if (launch_pwdw(v, threads, stream) == hipSuccess) return true;
                             (void)hipGetLastError();
                             return false;
                         }});
    }
    answers = tiles;
    for (size_t c = 0; c < cfgs.size(); c++) answers.push_back({"0," + std::to_string(c), nullptr});
    int best = 0;
    const int hit = autotune ? plan_cached(ckey, answers) : -1;
    if (hit >= 0) {
        fuse = hit < (int)cfgs.size();
        best = hit % (int)cfgs.size();
    } else if (autotune) {
        // the fastest tile configuration.  A small pair is a link of a latency chain (batch 1: 3.4 us per dependent launch whatever it
        // does): one launch instead of two is right by construction there, and the race -- which times a launch back to back with
        // ITSELF, i.e. its throughput -- gets exactly these wrong now and then (conv6/sep + pool6 left as two launches: 54.9 instead of
        // 51.4 us per MobileNet-v1 pass, profiles/r05_ab_b1_call12_vs_now_v2.txt, r05_ab_firstdw_pingpong_mobilenet_v1_b1.txt).
        // Timed against two launches: the batched pairs only.
        const bool batched = fmode != 2 && !fuse;
        if ((best = plan_race(g, sa.node, tiles, batched ? "" : ckey, 1.0f, true)) < 0) return -1;
        if (batched) {
            const int w = plan_race(g, sa.node, {two_launches("0," + std::to_string(best), sa, sb), tiles[best]}, ckey, 0.97f, true);
            if (w < 0) return -1;
            fuse = w == 1;
        }
    }
    if (!fuse) return 0;
    const PwDwArgs v = tmode == 1 ? with_tiles(a, cfgs[best].th, cfgs[best].tw, cfgs[best].sl) : a;
    const int threads = cfgs[best].threads;
    char nm[48];
    if (tmode == 1) snprintf(nm, sizeof(nm), "%s_i8<s%d,%dx%d,%d%s>", prod == 1 ? "firstdw" : "pwdw", a.S, v.TH, v.TW, threads, v.sl == 4 ? ",c64" : v.sl == 2 ? ",c32" : "");
    else snprintf(nm, sizeof(nm), "pwpool_i8<%d>", threads);
    // reads the pointwise input, writes the tail's output, nothing else; the first layer pair may run beside its predecessors (run_steps: wrap)
    *fused = fused_step({&pa, &pb}, nm, [v, threads](hipStream_t s) { return launch_pwdw(v, threads, s); }, x, y, prod == 1 && tmode == 1);
    g->fused_away[pw.out[0]] = 1;
    return 1;
}

// ---- two adjacent pwdw pairs in one launch: producer conv -> depthwise 3x3 (stride 1) -> pointwise conv -> depthwise 3x3: chain4.hip --------
// Which chains run by DEFAULT (batch 1 only): bit 0 the chain behind the network's first convolution (MobileNet-v1: conv1 .. conv2_2/dw),
// bit 1 a chain behind a pointwise conv (conv2_2/sep .. conv3_2/dw).  Set per kind from the interleaved A/B of profiles/chain4_ab.txt
// (parent build against a build with ONE kind on): the first-conv chain took the MobileNet-v1 batch-1 step from 51.62 to 50.38 us
// (median of 7, spreads 0.35 / 0.14 us) and is on; the pointwise chain left it where it was (51.59 against 51.62 us: its launch takes
// 7.1 us against 3.7 + 3.7 for the two it replaces) and stays reachable through TAMD_PIN=chain4=2 only.
#ifndef TAMD_CHAIN4_DEFAULT
#define TAMD_CHAIN4_DEFAULT 1
#endif

// The pair (ni, tail) was found by find_pwdw_tail (tmode 1).  Looks one pair further: the tail's sole consumer must be a 1x1 / stride-1 /
// unpadded conv whose own find_pwdw_tail is again a depthwise 3x3.  Limits of the kernel: dw1 stride 1, every depthwise pad 0 | 1,
// C1, C2 <= 128, a pointwise producer of K <= 128; each of the three intermediates has one consumer and is neither a graph output nor a
// view (find_pwdw_tail asks that of a pair's intermediate; the middle one is checked here).  TAMD_FUSE_PWDW=0 disables the chain with the
// pairs it is made of; TAMD_PIN=chain4=0 never, =2 always where applicable (also at batch > 1: tests); default: batch 1, a link of a
// latency chain, fused by construction (plan_pwdw: why not by a race).
bool find_chain4(tamd_graph* g, size_t ni, int tail, int prod, const std::vector<char>& fused, const std::vector<char>& has_fuse, int* pw2, int* dw2)
{
    auto taken = [&](int nj) { return fused[nj] || has_fuse[nj]; };
    const char* fenv = getenv("TAMD_FUSE_PWDW");
    const int pin = tamd_pin_int("chain4", 1);
    if ((fenv && atoi(fenv) == 0) || pin == 0) return false;
    const HNode& n0 = g->nodes[ni];
    const HNode& d1 = g->nodes[tail];
    const HTensor& x = g->tensors[n0.in[0]];
    const HTensor& y1 = g->tensors[d1.out[0]];
    if (pin != 2 && !(x.n == 1 && (TAMD_CHAIN4_DEFAULT & (prod == 1 ? 1 : 2)))) return false;
    auto pads01 = [](const tamd_conv_param& q) { return q.pad_h0 >= 0 && q.pad_h0 <= 1 && q.pad_w0 >= 0 && q.pad_w0 <= 1 && q.pad_h1 >= 0 && q.pad_h1 <= 1 && q.pad_w1 >= 0 && q.pad_w1 <= 1; };
    if (d1.p.conv.stride_h != 1 || !pads01(d1.p.conv) || y1.is_view) return false;
    if (g->tensors[n0.out[0]].c > 128 || (prod == 0 && x.c > 128)) return false;
    const int pj = sole_reader(g, d1.out[0]);
    if (pj < 0 || taken(pj) || g->nodes[pj].op != TAMD_OP_CONV) return false;
    int tmode = -1, prod2 = 0;
    const int dj = find_pwdw_tail(g, (size_t)pj, &tmode, &prod2);
    if (dj < 0 || tmode != 1 || prod2 != 0 || taken(dj) || g->tensors[g->nodes[pj].out[0]].c > 128 || !pads01(g->nodes[dj].p.conv)) return false;
    *pw2 = pj; *dw2 = dj;
    return true;
}

// The four nodes were just planned as pa .. pd.  The two GEMM nodes' constants are folded here (the multipliers go into the blob the
// kernel stages into LDS, and a first conv may have been planned in a form that keeps none); the two depthwise nodes' are the ones pb
// and pd uploaded.  TAMD_PIN=chain4_cfg=THxTWxthreads pins the tile.  0: no tile configuration fits -- the pairs stay as they are.
int plan_chain4(tamd_graph* g, HNode& n0, HNode& d1, HNode& p2, HNode& d2, int prod, const Planned& pa, const Planned& pb, const Planned& pc, const Planned& pd, Step* fused)
{
    HTensor& x = g->tensors[n0.in[0]];
    HTensor& w0 = g->tensors[n0.in[1]];
    HTensor* b0 = n0.in.size() > 2 ? &g->tensors[n0.in[2]] : nullptr;
    HTensor& m0 = g->tensors[n0.out[0]];
    HTensor& m1 = g->tensors[d1.out[0]];
    HTensor& w2 = g->tensors[p2.in[1]];
    HTensor* b2 = p2.in.size() > 2 ? &g->tensors[p2.in[2]] : nullptr;
    HTensor& m2 = g->tensors[p2.out[0]];
    HTensor& y = g->tensors[d2.out[0]];
    const tamd_conv_param& pp = n0.p.conv;
    const int cin = x.c, C1 = m0.c, C2 = m2.c, ns1 = (C1 + 15) / 16, ns2 = (C2 + 15) / 16;
    const int Kw = prod == 1 ? cin * pp.kernel_h * pp.kernel_w : cin;           // weight row length in the model
    const int K = prod == 1 ? cin * pp.kernel_h * 4 : cin;                      // reduction length as the kernel walks it (plan_pwdw)
    const int ks0 = ((prod == 1 ? K : rup(cin, 16)) + 63) / 64, ks2 = (ns1 * 16 + 63) / 64;
    if (w0.elems() != (size_t)C1 * Kw || (b0 && b0->elems() < (size_t)C1) || w2.elems() != (size_t)C2 * C1 || (b2 && b2->elems() < (size_t)C2)) return 0;
    if (m1.c != C1 || y.c != C2 || m1.h != m2.h || m1.w != m2.w || ks0 > 2 || ks2 > 2 || (prod == 1 && ks0 != 1)) return 0;
    // the two depthwise nodes: taps, bias and multipliers per thread from memory (DwArgs layout), as planned.  (The reference picks the
    // depthwise formula by batch == 1: conv_mode)
    const DwArgs *dw1 = planned_dw(g, d1, pb, C1), *dw2 = planned_dw(g, d2, pd, C2);
    if (!dw1 || !dw2) return 0;
    Chain4Args a{};
    RqArgs rq[4];
    rq[1] = dw1->rq; rq[3] = dw2->rq;
    a.dw1_w = dw1->w; a.dw1_bias = dw1->bias; a.dw1_wscale = dw1->wscale;
    a.dw2_w = dw2->w; a.dw2_bias = dw2->bias; a.dw2_wscale = dw2->wscale;
    std::vector<float> mf0, mf2;
    // the two GEMM nodes: panels, bias and multiplier vectors go into the blob the kernel stages into LDS
    std::vector<int8_t> wf0, wf2;
    {
        const int8_t* wd = (const int8_t*)w0.data.data();
        std::vector<int8_t> wrows;
        if (prod == 1) {
            if (first_conv_producer(g, x, w0, pp, C1, &wrows, &a)) return -1;
            wd = wrows.data();
        }
        wf0 = pack_pw_panel(wd, C1, K, ks0);
        // pw2's K is C1 rounded up to 16 and padded to 64-deep steps with zero weights: the slack channels of a slice meet zeros
        wf2 = pack_pw_panel((const int8_t*)w2.data.data(), C2, C1, ks2);
        if (upload_rq_m2(g, fold_requant(RQ_CONV_HCL, pp.activation, x.scales[0], m0.scales[0], w0, C1), ns1 * 16, &mf0, &rq[0])) return -1;
        if (upload_rq_m2(g, fold_requant(RQ_CONV_HCL, p2.p.conv.activation, m1.scales[0], m2.scales[0], w2, C2), ns2 * 16, &mf2, &rq[2])) return -1;
    }
    {
        std::vector<int8_t> blob;
        auto put = [&](const void* p, size_t bytes) { const int off = (int)blob.size(); blob.insert(blob.end(), (const int8_t*)p, (const int8_t*)p + bytes); return off; };
        const std::vector<int32_t> bp0 = padded_bias(b0 ? (const int32_t*)b0->data.data() : nullptr, C1, ns1 * 16);
        const std::vector<int32_t> bp2 = padded_bias(b2 ? (const int32_t*)b2->data.data() : nullptr, C2, ns2 * 16);
        put(wf0.data(), wf0.size());
        a.off_wf2 = put(wf2.data(), wf2.size());
        a.off_b0 = put(bp0.data(), bp0.size() * 4);
        a.off_s0 = put(mf0.data(), mf0.size() * 4);
        a.off_b2 = put(bp2.data(), bp2.size() * 4);
        a.off_s2 = put(mf2.data(), mf2.size() * 4);
        a.off_rq = put(rq, sizeof(rq));
        blob.resize(rup((int)blob.size(), 16), 0);
        a.blob_q = (int)(blob.size() / 16);
        int8_t* d0;
        if (upload(g, blob, &d0)) return -1;
        a.blob = d0;
    }
    a.win = rq_win(rq[0]) && rq_win(rq[1]) && rq_win(rq[2]) && rq_win(rq[3]) ? 1 : 0;
    a.prod = prod;
    a.coherent = (g->opt.direct_dispatch && !exp_plain_kernels()) ? 1 : 0;
    a.x = (const int8_t*)x.dptr + (prod == 1 ? 0 : x.c_off);
    a.N = x.n; a.cs_in = x.cs; a.H0 = m0.h; a.W0 = m0.w; a.H1 = m1.h; a.W1 = m1.w; a.OH = y.h; a.OW = y.w;
    a.P1H = d1.p.conv.pad_h0; a.P1W = d1.p.conv.pad_w0; a.S2 = d2.p.conv.stride_h; a.P2H = d2.p.conv.pad_h0; a.P2W = d2.p.conv.pad_w0;
    a.ns1 = ns1; a.ns2 = ns2; a.ks0 = ks0; a.ks2 = ks2;
    while ((1 << a.qsh1) < ns1 * 4) a.qsh1++;
    while ((1 << a.qsh2) < ns2 * 4) a.qsh2++;
    a.y = (int8_t*)y.dptr; a.ldc = y.cs; a.c_off = y.c_off; a.c_limit = store_limit(y, C2);

    // ---- tile configurations: a short list, ranked by the instruction slots of the busiest wave, the fastest by plan_race ---------
    struct Cfg { int th, tw, threads; double cost; };
    std::vector<Cfg> cfgs;
    auto with_tiles = [&](Chain4Args v, int th, int tw) {
        v.TH = th; v.TW = tw; v.tiles_y = (v.OH + th - 1) / th; v.tiles_x = (v.OW + tw - 1) / tw;
        v.RCH = (th - 1) * v.S2 + 3; v.RCW = (tw - 1) * v.S2 + 3;
        return v;
    };
    const int shapes[5][2] = {{2, 2}, {2, 4}, {4, 4}, {4, 7}, {7, 7}};
    for (auto& sh : shapes)
        for (int threads : {256, 512}) {
            const int th = std::min(sh[0], a.OH), tw = std::min(sh[1], a.OW);
            bool dup = false;
            for (auto& c : cfgs) dup |= c.th == th && c.tw == tw && c.threads == threads;
            const Chain4Args v = with_tiles(a, th, tw);
            if (dup || !chain4_config_ok(v, threads)) continue;
            const double nw = threads / 64, ap = (double)std::min(v.RCH + 2, a.H0) * std::min(v.RCW + 2, a.W0), cp = (double)std::min(v.RCH, a.H1) * std::min(v.RCW, a.W1);
            const double block = 300.0 + std::ceil(std::ceil(ap / 16.0) / nw) * (45.0 + 30.0 * ns1) + std::ceil(cp * ns1 * 4.0 / threads) * 90.0
                                 + std::ceil(std::ceil(cp / 16.0) * ns2 / nw) * (40.0 + 4.0 * ks2) + std::ceil((double)th * tw * ns2 * 4.0 / threads) * 90.0;
            const double blocks = (double)a.N * v.tiles_y * v.tiles_x;
            cfgs.push_back({th, tw, threads, std::ceil(blocks / (256.0 * (threads == 256 ? 2 : 1))) * block});
        }
    std::sort(cfgs.begin(), cfgs.end(), [](const Cfg& l, const Cfg& r) { return l.cost < r.cost; });
    int pth = 0, ptw = 0, pthreads = 0, psl = 1;
    if (pinned_tile("chain4_cfg", a.OH, a.OW, &pth, &ptw, &pthreads, &psl) && chain4_config_ok(with_tiles(a, pth, ptw), pthreads)) {
        cfgs.clear(); cfgs.push_back({pth, ptw, pthreads, 0.0});
    }
    if (cfgs.empty()) return 0;
    std::vector<RaceCand> tiles;
    for (size_t c = 0; c < cfgs.size(); c++) {
        const Chain4Args v = with_tiles(a, cfgs[c].th, cfgs[c].tw);
        const int threads = cfgs[c].threads;
        char tag[32];
        snprintf(tag, sizeof(tag), "%dx%dx%d", cfgs[c].th, cfgs[c].tw, threads);
        tiles.push_back({tag, [v, threads](hipStream_t s) { return launch_chain4(v, threads, s); }, std::string("chain4 ") + tag});
    }
    char ckey[256];
    snprintf(ckey, sizeof(ckey), "chain4|%s|n%d %dx%d c%d>%d s%d p%d c%zu", pa.step.node.c_str(), a.N, a.H0, a.W0, C1, C2, a.S2, prod, cfgs.size());
    const int best = tiles.size() > 1 ? plan_race(g, pa.step.node, tiles, ckey, 1.0f, autotune_enabled()) : 0;
    if (best < 0) return -1;
    const Chain4Args v = with_tiles(a, cfgs[best].th, cfgs[best].tw);
    const int threads = cfgs[best].threads;
    char nm[64];
    snprintf(nm, sizeof(nm), "%s_i8<s%d,%dx%d,%d>", prod == 1 ? "firstchain4" : "chain4", a.S2, v.TH, v.TW, threads);
    // reads the producer's input, writes the last depthwise's output, nothing else (deps: as plan_pwdw)
    *fused = fused_step({&pa, &pb, &pc, &pd}, nm, [v, threads](hipStream_t s) { return launch_chain4(v, threads, s); }, x, y, prod == 1);
    g->fused_away[n0.out[0]] = 1;
    g->fused_away[d1.out[0]] = 1;
    g->fused_away[p2.out[0]] = 1;
    return 1;
}

// ---- depthwise 3x3 (stride 1) + the pointwise conv that consumes it in one launch: dwpw.hip ------------------------------------
// Called with the pair planned as `pd` (the depthwise launch) and `pc` (whichever GEMM-family member the pointwise race chose).
// Large batches only: at batch 1 the pointwise conv pairs with the depthwise BEHIND it instead (pwdw.hip), which this
// fusion would take away.  TAMD_FUSE_DWPW=0 never, =2 always (tests); default: the faster of the two by plan-time timing.
int plan_dwpw(tamd_graph* g, HNode& dw, HNode& pw, const Planned& pd, const Planned& pc, Step* fused)
{
    const char* env = getenv("TAMD_FUSE_DWPW");
    const int fmode = env ? atoi(env) : 1;
    if (!fmode || pd.kind != Planned::DW3X3 || pc.kind != Planned::GEMM || pc.elt_tail || !dwpw_applicable(pd.dw, pc.gemm)) return 0;
    const DwArgs& d = pd.dw;
    const ConvArgs& c = pc.gemm;
    if (fmode != 2 && (long)d.N * d.OH * d.OW < 4096) return 0;
    const HTensor& w = g->tensors[pw.in[1]];
    std::vector<int8_t> wp(dwpw_packed_bytes(c.cout, c.cin));
    dwpw_pack((const int8_t*)w.data.data(), c.cout, c.cin, wp.data());
    int8_t* dwf = nullptr;
    if (upload(g, wp, &dwf)) return -1;
    DwPwArgs a{};
    a.x = d.x; a.dw_w = d.w; a.dw_bias = d.bias; a.dw_wscale = d.wscale; a.dw_rq = d.rq;
    a.pw_wfrag = dwf; a.pw_bias = c.bias; a.pw_wscale = c.wscale; a.pw_rq = c.rq;
    a.y = c.y;
    a.N = d.N; a.H = d.H; a.W = d.W; a.C = d.C; a.cs_in = d.cs_in; a.cw = d.cw; a.OH = d.OH; a.OW = d.OW; a.PH = d.PH; a.PW = d.PW;
    a.cout = c.cout; a.ldc = c.ldc; a.c_off = c.c_off; a.c_limit = c.c_limit;
    bool fuse = fmode == 2;
    if (fmode != 2) {
        char ckey[256];
        snprintf(ckey, sizeof(ckey), "dwpw|%s|n%d %dx%d c%d>%d", pd.step.node.c_str(), d.N, d.OH, d.OW, d.C, c.cout);
        const RaceCand one{"1", [a](hipStream_t s) { return launch_dwpw(a, s); }, "dwpw_i8"};
        const int w = plan_race(g, pd.step.node, {two_launches("0", pd.step, pc.step), one}, ckey, 0.97f, autotune_enabled());
        if (w < 0) return -1;
        fuse = w == 1;
    }
    if (!fuse) return 0;
    *fused = fused_step({&pd, &pc}, "dwpw_i8", [a](hipStream_t s) { return launch_dwpw(a, s); }, g->tensors[dw.in[0]], g->tensors[pw.out[0]], true);
    g->fused_away[dw.out[0]] = 1;
    return 1;
}

// ---- an identity bottleneck block -- 1x1 -> 3x3 -> 1x1 + residual (+ ReLU) -- in one launch: block_i8.hip --------------------------
// TAMD_FUSE_BLOCK=1 fuses wherever block_applicable holds; unset or 0: never (opt-in: no plan-time race, no plan-cache entry).
bool fuse_block_enabled()
{
    const char* env = getenv("TAMD_FUSE_BLOCK");                 // read at every prerun
    return env && atoi(env) == 1;
}

// Called with the three convolutions planned as `pa`, `pb` (as they stand) and `pc` (with the eltwise tail fz that scan_eltwise_fusion
// gave it); every one keeps the requantisation plan_conv folded for it (conv_mode at the graph's batch), the fused launch reads the
// same device vectors.  The caller (try_block) has read the switch and matched the graph shape.
int plan_block(tamd_graph* g, HNode& na, HNode& nb, HNode& nc, const FusedElt& fz, const Planned& pa, const Planned& pb, const Planned& pc, Step* fused)
{
    if (pa.kind != Planned::GEMM || pb.kind != Planned::GEMM || pc.kind != Planned::GEMM) return 0;
    if (pa.elt_tail || pb.elt_tail || !pc.elt_tail || !block_applicable(pa.gemm, pb.gemm, pc.gemm_tail)) return 0;      // (the residual IS na's input: block_applicable compares the pointers)
    const ConvArgs& a = pa.gemm;
    const HTensor &wa = g->tensors[na.in[1]], &wb = g->tensors[nb.in[1]], &wc = g->tensors[nc.in[1]];
    const int C = a.cin, mid = a.cout;
    if (wa.elems() != (size_t)mid * C || wb.elems() != (size_t)mid * mid * 9 || wc.elems() != (size_t)C * mid) return 0;
    std::vector<int8_t> wp(block_packed_bytes(C, block_mid_pad(mid)));
    block_pack((const int8_t*)wa.data.data(), (const int8_t*)wb.data.data(), (const int8_t*)wc.data.data(), C, mid, wp.data());
    int8_t* dwp = nullptr;
    if (upload(g, wp, &dwp)) return -1;
    const BlockArgs v = block_args(a, pb.gemm, pc.gemm_tail, dwp);
    *fused = fused_step({&pa, &pb, &pc}, "block_i8", [v](hipStream_t s) { return launch_block(v, s); }, g->tensors[na.in[0]], g->tensors[fz.out_tensor], true);
    g->fused_away[na.out[0]] = 1;
    g->fused_away[nb.out[0]] = 1;
    return 1;
}

}  // namespace tamd
