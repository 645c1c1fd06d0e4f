// Device-kernel argument blocks and host launchers (private to the backend).
// Device layout: activations are NHWC int8 with a channel stride `cs` that is a multiple of 16 bytes
// (so every pixel row is 16-B aligned and K-contiguous for MFMA operand loads); conv weights are
// repacked once at prerun to [cout_pad][kpad] with k = (ky*KW+kx)*cin_pad + ci, zero padded.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

namespace tamd {

struct EltFuse {              // eltwise (+ReLU) node applied in the conv epilogue (epilogue.h: fuse_elt4)
    const int8_t* res;        // the other eltwise operand (NHWC, same pixels); nullptr: no fusion
    int res_ldc, res_c_off;   // its channel stride / offset
    int type;                 // ELT_* (0 prod, 2 sum, 4 sub, 6 max)
    int conv_is_first;        // the conv output is eltwise input 0 (matters for sub)
    float s_conv, s_res;      // scales of the conv output tensor and of the residual tensor
    float out_scale;          // eltwise output scale
    int relu;                 // a ReLU (slope 0) node follows
    float relu_out_scale;
    // SUM (+ ReLU that keeps the eltwise scale) in two fused multiply-adds per value (epilogue.h: elt_sum16_fold), folded by the
    // planner: mc = RN32(s_conv / out_scale), mr = RN32(s_res / out_scale), k0 = RN32(128.5 + e - 128 * (mc + mr)), window
    // [ylo, yhi] = [128 + (relu ? 0 : -127) + 0.25, 255.75], hand-over threshold thr = 2e; thr = 0: not applicable
    float mc, mr, k0, ylo, yhi, thr;
};

// Requantisation constants of one conv / FC node, folded by the planner (graph_plan_conv.hip: fold_requant + host_rq; the arithmetic and
// its exactness argument are in epilogue.h).  The kernels' per-channel vector `wscale[]` holds the FAST-path multiplier
// M[c] = RN32(m1 * m2[c] / out_scale); the reference chain's own factors stay here for the values the fast path hands over.
struct RqArgs {
    float m1, lo, hi, out_scale;   // reference chain: f = clamp(fl(fl((float)acc * m1) * m2[c]), lo, hi), q = sat127(round(f / out_scale));
                                   // lo / hi already fold the +-127.49 * out_scale saturation
    float ylo, yhi;                // fast path: clamp of the biased value, 128 + q(lo) + 0.25 / 128 + q(hi) + 0.75
    float thr;                     // fast path: hand over when fract(y) < thr (2^-13; 2.0 = always, when the constants are out of range)
    const float* m2;               // [as wscale] m2[c] of the reference chain, read on the hand-over path only
};

struct ConvArgs {
    const int8_t* x;       // NHWC input, channel stride cs_in
    const int8_t* w;       // packed weights [cout_pad][kpad]
    const int32_t* bias;   // [cout_pad] (zeros when the node has no bias)
    const float* wscale;   // [cout_pad] fast-path multipliers M[c] (see RqArgs)
    int8_t* y;             // NHWC output base
    int N, H, W, cs_in;    // cs_in: bytes between consecutive input pixels
    int ckp;               // K bytes per tap = roundup(cin,16) (== cs_in unless x is a concat view)
    int OH, OW;
    int cout;              // logical output channels
    int ldc;               // output channel stride (bytes per pixel)
    int c_off;             // channel offset inside the output pixel (concat-by-offset)
    int c_limit;           // channels [0,c_limit) of this conv may be stored (multiple of 4)
    int KH, KW, SH, SW, PH, PW, DH, DW;
    int cin;               // logical input channels per group
    int ktot;              // KH*KW*ckp
    int kpad;              // weight row stride (multiple of the K tile)
    int M;                 // N*OH*OW
    RqArgs rq;             // requantisation constants, see epilogue.h (wscale[] holds M[c])
    const int8_t* zeros;   // >= 16 zero bytes (source of out-of-image taps for the LDS-DMA kernel)
    unsigned long long mg_ohw, mg_ow;   // ceil(2^40 / (OH*OW)), ceil(2^40 / OW): pixel index -> (n, oy, ox) by multiply-high (conv_igemm_fast.h)
    int cfg;               // tile configuration of the chosen GEMM kernel (-1: the launcher's heuristic), set by the planner
    // conv_pgemm.hip only (conv_pgemm_prepare / the planner fill these; other kernels ignore them)
    const int8_t* wfrag;   // weights in MFMA fragment order: [cout tile of BN][stage][BN/32 x 2 fragments][64 lanes][16 B]
    int pg_ns;             // 64-deep K stages; stage = (64-channel chunk) * KH*KW + tap
    int pg_variant;        // tile shape, see conv_pgemm_bn()
    int pg_npad;           // patch pixels of the worst pixel tile, rounded up to 64 (k x k convolutions)
    int pg_hp, pg_wp;      // rows per image / columns of the virtual padded input the patch is cut from
    unsigned long long mg_hp, mg_wp;     // ceil(2^40 / pg_hp), ceil(2^40 / pg_wp)
    // conv_pgemm_w.hip only (conv_pgemm_w_prepare / conv_pgemm_w_table)
    const int* pg_tab;     // per pixel tile: [pg_npad] NHWC pixel index of each patch unit (-1: zeros), [BM] patch origin | edge bits << 16 of each output pixel
    int pg_ts;             // dwords per tile of pg_tab
    int pg_tiles_m, pg_tiles_n;
    int pg_zarea;          // bytes of the zero area behind each patch buffer (edge taps)
    unsigned mg_tn;        // ceil(2^32 / pg_tiles_n) (pg_tiles_n > 1)
#ifdef TAMD_IGEMM_STAMPS
    long long* dbg_stamps; // tools/exp/igemm_anatomy.hip only: s_memtime at the stage boundaries of wave 0 of block 0
    int dbg_flags;         // .. ablation: 1 no MFMA, 2 no LDS traffic, 4 no global loads
#endif
    EltFuse elt;           // fused eltwise(+relu) tail (conv_igemm / conv_igemm2 only); y/ldc/c_off then describe ITS output
};

// The pointwise form of the GEMM family: output pixel m reads input pixel m.  ConvArgs carries the leading pads only; a trailing pad
// (pad_h1 / pad_w1 of a TF-converted 1x1 layer) shows as an output map larger than the input -- its extra row / column holds the
// requantised bias, which only the tap-addressed form computes.
inline bool conv_is_pointwise(const ConvArgs& a)
{
    return a.KH == 1 && a.KW == 1 && a.SH == 1 && a.SW == 1 && a.PH == 0 && a.PW == 0 && a.OH == a.H && a.OW == a.W;
}

struct DwArgs {
    const int8_t* x;       // NHWC
    const int8_t* w;       // [3 rows][cw] dwords {w[r][0],w[r][1],w[r][2],0}, cw = roundup(C,16)
    const int32_t* bias;   // [cw]
    const float* wscale;   // [cw]
    int8_t* y;
    int N, H, W, C, cs_in, cw, OH, OW, ldc, c_off;
    int S, PH, PW;
    RqArgs rq;             // requantisation constants, see epilogue.h (wscale[] holds M[c])
};

struct DwPwArgs {          // depthwise 3x3 (stride 1) -> pointwise 1x1 in one launch (dwpw.hip): the depthwise result only exists in LDS
    const int8_t* x;       // NHWC input of the depthwise conv (channel offset applied)
    const int8_t* dw_w;    // DwArgs::w
    const int32_t* dw_bias; const float* dw_wscale; RqArgs dw_rq;
    const int8_t* pw_wfrag;        // pointwise weights in A-fragment order (dwpw_pack)
    const int32_t* pw_bias; const float* pw_wscale; RqArgs pw_rq;
    int8_t* y;             // NHWC output of the pointwise conv
    int N, H, W, C, cs_in, cw, OH, OW, PH, PW;     // depthwise geometry (C channels in and out, cw = roundup(C, 16))
    int cout, ldc, c_off, c_limit;                 // pointwise output
#ifdef TAMD_DWPW_STAMPS
    unsigned long long* stamps;                    // tools/exp/dwpw_anatomy.hip only: 16 per block
    int ablate;                                    // .. 1: no MFMAs, 2: no depthwise arithmetic, 4: no epilogue requantisation, 8: no A-fragment loads after stage 0, 16: no tap loads, 32: no B-fragment reads
#endif
};

struct BlockArgs {         // identity bottleneck block in one launch (block_i8.hip): 1x1 -> 3x3 -> 1x1 + residual [+ ReLU]; both intermediate
                           // maps only exist in LDS
    const int8_t* x;       // NHWC input of branch2a == the residual (channel offset applied)
    const int8_t* wpk;     // the three weight sets in A-fragment order (block_pack.h)
    const int32_t* bias_a; const float* wscale_a; RqArgs rq_a;     // branch2a (1x1, C -> mid), padded to >= roundup(mid, 32) channels
    const int32_t* bias_b; const float* wscale_b; RqArgs rq_b;     // branch2b (3x3 stride 1 pad 1, mid -> mid)
    const int32_t* bias_c; const float* wscale_c; RqArgs rq_c;     // branch2c (1x1, mid -> C)
    EltFuse elt;           // the eltwise (+ReLU) tail of branch2c; elt.res is not read: the residual comes from the staged input tile
    int8_t* y;             // NHWC output of the tail
    int N, H, W, C, mid, cs_in, ldc, c_off, c_limit;
    int tiles_x, tiles_y, tiles;           // 8 x 8 output tiles per image row / column, in all (N * tiles_y * tiles_x)
    int grid;              // blocks; each loops over tiles blockIdx.x, blockIdx.x + grid, ..
#ifdef TAMD_BLOCK_STAMPS
    unsigned long long* stamps;            // tools/exp/block_anatomy.hip only: 8 per block (100 MHz wall clock)
#endif
};

struct PwDwArgs {          // pointwise conv + its consumer in one launch (pwdw.hip)
    const int8_t* x;       // NHWC input of the pointwise conv (channel offset applied)
    const int8_t* wf;      // pointwise weights in MFMA fragment order: [16-channel slice][64-deep K step][64 lanes][16 B]
    const int32_t* bias;   // [slices * 16]
    const float* wscale;   // [slices * 16] (M[c] of epilogue.h)
    RqArgs rq;             // pointwise requantisation constants
    int N, H, W, cs_in, ktot;          // H x W: the pointwise map == the tail's input map
    int nsteps, steps;                 // 64-deep K steps of the (zero padded) weight panel, a multiple of `steps` = pwdw_steps()
#ifdef TAMD_PWDW_STAMPS
    unsigned long long* stamps;        // tools/exp/pwdw_anatomy.hip only
#endif
    int coherent;          // 1: the coherent instance (agent-scope loads of x, write-through stores of y): its launch needs no cache
                           // maintenance at its boundaries (pwdw.hip: pwdw_i8_coh_kernel; set when the graph dispatches directly)
    int mode;              // tail: 0 global pooling, 1 depthwise 3x3, 2 none (the tile results are stored)
    int prod;              // producer: 0 pointwise conv of an NHWC tensor, 1 first-layer conv gathered from the NCHW graph input
    const unsigned* taps;  // prod 1: [16] patch row (c, ky) -> (c*in_H*in_W + ky*DH*in_W) | ky*DH << 28, zero padded; k = row*4 + kx
    int in_C, in_H, in_W;  // prod 1: the NCHW input;  H x W above is then the first conv's OUTPUT map
    int fSH, fSW, fPH, fPW;            // prod 1: stride, leading pads
    int sl;                // 16-channel slices per block: 2 | 4 (depthwise tails with a register-resident K; slices = cout / (16 sl)), else one.
                           // HERE, in what was a 4-byte alignment hole: the struct must not grow -- its size decides which 64-byte line of the
                           // argument segment holds the hidden block size the kernels read late, and 8 bytes more cost every batch-1 launch
                           // with a depthwise tail 0.15-0.2 us (a cold scalar-cache line on the critical path;
                           // profiles/r05_ab_b1_call12_vs_now.txt: identical instructions, +3-6 % per launch)
    const int8_t* dw_w;    // as DwArgs::w
    const int32_t* dw_bias;
    const float* dw_wscale;
    RqArgs d_rq;
    int cw;                // depthwise weight row length (channels rounded up to 16)
    int S, PH, PW, OH, OW; // depthwise stride / leading pads / output map
    int8_t* y;             // NHWC output of the tail
    int ldc, c_off, c_limit;
    int TH, TW, tiles_y, tiles_x, slices;      // depthwise output tile per block, grid (slices: blocks along the channels)
    int tile_major;        // 1: grid = (tile_x, tile_y * N, slice) instead of (slice, tile_x, tile_y * N): which operand an XCD's L2 shares
    int RH, RW;            // input region of a tile: (TH-1)*S+3, (TW-1)*S+3
    int pool_method;       // mode 0: 0 max, 1 avg
    float p_in_scale, p_out_scale;
};

struct Chain4Args {        // producer conv -> depthwise 3x3 (stride 1) -> pointwise conv -> depthwise 3x3 (stride 1 | 2) in one launch (chain4.hip):
                           // a block owns a spatial tile with all channels; the three intermediate maps only exist in LDS
    const int8_t* x;       // prod 0: NHWC input of the producer (channel offset applied); prod 1: the NCHW graph input
    const int8_t* blob;    // [producer panel | pw2 panel | producer bias | producer M[c] | pw2 bias | pw2 M[c] | RqArgs of producer, dw1, pw2, dw2]:
                           // both pointwise weight sets in MFMA fragment order (pack_pw_panel) with their vectors and the four nodes'
                           // requantisation constants, staged into LDS once per block; blob_q 16-byte pieces
    const unsigned* taps;  // prod 1: PwDwArgs::taps
    const int8_t* dw1_w; const int32_t* dw1_bias; const float* dw1_wscale;     // as DwArgs::w / bias / wscale, rows of ns1 * 16 channels
    const int8_t* dw2_w; const int32_t* dw2_bias; const float* dw2_wscale;     // .. of ns2 * 16
    int8_t* y;             // NHWC output of the last depthwise
    int prod, coherent;    // as PwDwArgs
    int win;               // 1: all four requantisation windows are in the one-binade form (epilogue.h: rq_win)
    int N;
    int in_C, in_H, in_W, fSH, fSW, fPH, fPW;      // prod 1: the NCHW input, the first conv's stride / leading pads
    int cs_in;             // prod 0: bytes between consecutive input pixels
    int H0, W0;            // the producer's output map (= its input map for prod 0)
    int H1, W1;            // dw1's output map = pw2's map
    int OH, OW;            // dw2's output map
    int P1H, P1W, S2, P2H, P2W;        // leading pads of dw1; stride and leading pads of dw2
    int ns1, ns2;          // 16-channel slices of C1 (producer / dw1) and C2 (pw2 / dw2), <= 8 each
    int ks0, ks2;          // 64-deep K steps of the producer's and pw2's panel (1 | 2)
    int qsh1, qsh2;        // log2 of the threads per pixel in the depthwise phases (channel quads rounded up to a power of two)
    int blob_q, off_b0, off_s0, off_wf2, off_b2, off_s2, off_rq;       // blob: size in 16-byte pieces, byte offsets of its parts (the producer panel is at 0)
    int ldc, c_off, c_limit;
    int TH, TW, tiles_x, tiles_y;      // dw2 output tile per block, grid (tiles_x, tiles_y, N)
    int RCH, RCW;          // dw2's input region of a tile: (TH-1)*S2+3, (TW-1)*S2+3; dw1's is two more each way
};

#ifdef TAMD_PWDW_CHAIN_EXPERIMENT      // tools/exp/chain_anatomy.hip only (why the chained launch is not in the product)
struct PwChainArgs {       // several PwDwArgs layers as ONE launch, ordered by counters (pwdw.hip: pwdw_chain_kernel)
    const PwDwArgs* layers;    // device array [nlayers]
    int nlayers;
    int first_block[17];       // blocks of layer l: [first_block[l], first_block[l + 1])
    short variant[16];         // kernel variant of layer l: MODE | PROD << 3 | steps << 4 (pwdw_chain_variant)
    short gx[16], gy[16];      // its grid (x, y; z follows from the block count)
    int* flags;                // [32 * nlayers] finished-block counter of layer l at [32 * l] (a cache line each); never reset
    int* sync;                 // [0] epoch, [1] finished blocks of the last layer, [2] a bounded wait gave up
};
#endif

struct DirectArgs {        // generic direct conv (any group / cin), also NCHW-input first layers
    const int8_t* x;
    const int8_t* w;       // OIHW as in the model
    const int32_t* bias;   // may be null
    const float* wscale;
    int8_t* y;             // NHWC
    int N, C, H, W, cs_in; // cs_in == 0 => x is NCHW (graph input), else NHWC with that stride
    int OH, OW, cout, ldc, c_off;
    int KH, KW, SH, SW, PH, PW, DH, DW, group;
    RqArgs rq;             // requantisation constants, see epilogue.h (wscale[] holds M[c])
};

struct FirstArgs {         // first layer from the NCHW graph input (C <= 4) on MFMA
    const int8_t* x;       // NCHW
    const int8_t* w;       // [cout_pad32][kp], k = (c*KH+ky)*KW+kx (OIHW order), zero padded
    const int32_t* bias;   // [cout_pad32]
    const float* wscale;   // [cout_pad32]
    int8_t* y;             // NHWC
    int N, C, H, W, OH, OW, cout, ldc, c_off, c_limit;
    int KH, KW, SH, SW, PH, PW, DH, DW;
    int kp;                // roundup(C*KH*KW, 32) <= 256
    int kwp;               // 0: k = OIHW order (gather kernel); 4 / 8: k = (c*KH+ky)*kwp + kx, kp = roundup(C*KH*kwp, 32) <= 192
    RqArgs rq;             // requantisation constants, see epilogue.h (wscale[] holds M[c])
};

struct PoolArgs {
    const int8_t* x; int8_t* y;
    int N, H, W, C, cs_in, OH, OW, ldc, c_off;
    int KH, KW, SH, SW, PH, PW;
    int method, caffe_flavor;
    float in_scale, out_scale;
};

// the global form (window == whole map, no padding): launch_pool takes its own kernel for it
inline bool pool_is_global(const PoolArgs& a) { return a.OH == 1 && a.OW == 1 && a.KH == a.H && a.KW == a.W && a.PH == 0 && a.PW == 0; }

struct ReluPoolArgs {      // ReLU (slope >= 0) -> MAX pool in one launch: max of the raw bytes, the ReLU's byte map once, the pool's requant
    PoolArgs p;            // the pool as planned, except x / cs_in: the ReLU's INPUT; in_scale is the ReLU's output scale
    float slope, relu_in_scale;
};

struct UpsampleI8Args {    // nearest upsample by an integer factor, NHWC int8: upsample_ref.c:74-130 run on the int8 BYTES (0 .. 255)
    const int8_t* x;       // first channel of the input (a view's channel offset applied)
    int8_t* y;             // base of the output buffer
    int N, H, W, C, cs_in; // input map; the output map is H * scale x W * scale
    int scale, ldc, c_off; // output pixel stride and channel offset (a concat view)
    float in_scale, out_scale;
    int in_zp, out_zp;
    int copy;              // equal scales and zero points: the byte map is the identity
    int fix128;            // 1: the output is a view of a Concat of several inputs, whose copy stores 127 for the byte -128 (epilogue.h: fix128_4)
};

struct FirstPoolArgs {     // the stem in one launch: FirstArgs' convolution (7 x KW, stride 2, C = 3) + MAX pool 3x3 / 2 / pad 0 (conv_first_pool.hip)
    const int8_t* x;       // NCHW graph input
    const int8_t* w;       // FirstArgs::w with kwp == 8
    const int32_t* bias; const float* wscale;
    int8_t* y;             // NHWC pooled map
    int N, C, H, W, OH, OW, cout;      // OH x OW: the conv map (never stored)
    int KH, KW, PH, PW, kp;
    int POH, POW, ldc, c_off;          // pooled map and its destination
    float pool_in_scale, pool_out_scale;
    RqArgs rq;
};

struct EltArgs {
    const int8_t* a; const int8_t* b; int8_t* y;
    size_t count;          // bytes (padded NHWC buffers, identical geometry)
    int type;
    float sa, sb, out_scale;
    int fuse_relu;         // 1: apply the following standalone ReLU node (slope 0) in the same pass
    float relu_out_scale;
};

struct ReluArgs {
    const int8_t* x; int8_t* y; size_t count; float slope, in_scale, out_scale;
};

struct LutArgs {           // y[i] = table[x[i]] over `count` bytes, x and y 16-byte aligned (Sigmoid / Clip / HardSwish / Mish, int8 and uint8)
    const uint8_t* x; uint8_t* y;
    size_t count;          // cs == 0: the bytes of a dense tensor, any number.  cs > 0: an NHWC int8 buffer, N * H * W * cs bytes
    int C, cs;             // cs > 0 (a multiple of 16): only channels [0, C) of every pixel are mapped, the padding lanes [C, cs) are written 0
    const unsigned* table; // [64]: entries 4i .. 4i + 3 in the bytes of dword i, lowest first (tamd_lut_table's 256 bytes as they lie)
};

struct InterpI8Args {      // nearest Interp, NHWC int8 (interp.hip): y[n][oy][ox][c] = table[x[n][iy[oy]][ix[ox]][c]], padding lanes written 0
    const int8_t* x;       // first channel of the input (a view's channel offset applied)
    int8_t* y;             // base of the output buffer
    int N, H, W, C, cs_in; // input map and its pixel stride
    int OH, OW, ldc, c_off;// output map, its pixel stride and channel offset (a concat view)
    const int* iy;         // [OH] source row of every output row, [OW] source column of every output column (tamd_interp_indices)
    const int* ix;
    const unsigned* table; // [64]: tamd_interp_table's 256 bytes as they lie
};

struct InterpU8Args {      // nearest Interp, dense NCHW uint8 (interp.hip)
    const uint8_t* x; uint8_t* y;
    int N, C, H, W, OH, OW;
    int out_img, out_c0;   // output image stride (bytes) / channel offset (concat), as in U8MapArgs
    const int* iy; const int* ix;
    const unsigned* table;
    int identity;          // the table maps every byte to itself: no lookups
};

// Split / ShuffleChannel / Concat + ShuffleChannel of an int8 graph (chanmap.hip): y[pixel][c_off + o] = src[s][pixel][off] for every
// output channel o, where table[o] = s << 28 | off names the source and the byte offset inside ITS pixel (a view's channel offset
// included), or kChanMapZero: written as zero.  The table has one entry per channel of the whole 16-byte vectors, rup(C, 16)
constexpr int kChanMapMaxSrc = 4;
constexpr unsigned kChanMapZero = 0xffffffffu;
struct ChanMapI8Src { const int8_t* x; int cs; };      // base of the source's buffer, its bytes per pixel
struct ChanMapI8Args {
    ChanMapI8Src src[kChanMapMaxSrc];
    int nsrc;
    int8_t* y;             // base of the output buffer
    long pixels;           // N * H * W, the same in every source
    int C, ldc, c_off;     // output channels, pixel stride and channel offset (a concat view)
    const unsigned* table; // [rup(C, 16)]
    int fix128;            // 1: the byte -128 is written as 127 (the reference's Concat between equal scales, see chanmap.hip)
};

// group 2 over two sources of equal width `half` (ShuffleNet-v2's own pair: Concat of two halves -> ShuffleChannel(2), or a
// ShuffleChannel(2) of one tensor): output channel 2j is a[j], 2j + 1 is b[j] -- output vector v is the byte interleave of 8 bytes of each
struct ChanMapG2Args {
    const int8_t* a; const int8_t* b;   // first channel of either half (a view's channel offset applied), 8-byte aligned
    int cs_a, cs_b;        // their bytes per pixel
    int8_t* y; long pixels;
    int half, ldc, c_off;
    int fix128;
};

// the same operators in a uint8 graph (dense NCHW): output plane o of image n = plane src_plane[o] of image n of x, every byte through
// `table` unless it is the identity (a uint8 Split's requantisation: tamd_split_table)
struct ChanMapU8Args {
    const uint8_t* x; uint8_t* y;
    int N, C, HW;          // images, OUTPUT planes per image, bytes per plane
    int in_img;            // bytes per input image
    int in_planes;         // planes per input image (every src_plane entry is below it: checked where the table is built)
    int out_img, out_c0;   // output image stride (bytes) / channel offset (concat), as in U8MapArgs
    const int* src_plane;  // [C]
    const unsigned* table; // [64]: tamd_split_table's 256 bytes as they lie
    int identity;
};

// Slice of a uint8 graph (slice.hip; the host truth of the byte map: slice_tables.cc), dense NCHW: a strided box of x,
// y[n][c][h][w] = table[x[start0 + n * step0][start1 + c * step1][start2 + h * step2][start3 + w * step3]].  One Slice node cuts one
// axis; two in a row compose into one box over two axes
struct SliceU8Args {
    const uint8_t* x; uint8_t* y;
    int in_dims[4], out_dims[4];   // N, C, H, W of either tensor; start[i] + (out_dims[i] - 1) * step[i] < in_dims[i]: launch_slice_u8 checks it
    int start[4], step[4];         // every step >= 1
    int out_img, out_c0;           // output image stride (bytes) / channel offset, as in ChanMapU8Args
    const unsigned* table;         // [64]: the 256 bytes of the map as they lie
    int identity;                  // the map is the identity (equal parameters, or the reference's raw copy): no table, no LDS
    int w2;                        // 1: an output row's 16 bytes at W step 2 come from two 16-byte loads and byte permutes; 0: byte by byte
    int contig;                    // (set by launch_slice_u8) how far consecutive output bytes are consecutive source bytes: 0 nowhere (W
                                   // step > 1), 1 inside a row, 2 inside a plane (W not cut, H step 1), 3 inside an image (H not cut, C step 1)
};

// Transpose of a quantised graph (transpose.hip; the host truth of the byte map: transpose_tables.cc), both types:
// y[o] = table[x[sum_d i_d * stride[d]]] with o decomposed over extent[] as a dense row-major index, axis nd - 1 innermost.  The pairs are
// the canonical geometry of transpose_canon (node_rules.h), LEFT-aligned as it makes them (axes nd .. 5: extent 1, stride 0).  x is a
// dense tensor or a convolution-stack NHWC buffer (the same thing with other strides, base + c_off); y is dense
struct TransposeArgs {
    const uint8_t* x; uint8_t* y;
    int nd;                        // 1 .. 6
    int extent[6], stride[6];      // every extent >= 1; the largest source offset stays below src_bytes: launch_transpose checks it
    int unit;                      // which axis has stride 1 (-1: none)
    unsigned total;                // output bytes, the product of the extents
    unsigned src_bytes;            // bytes of the buffer x points into, from x on
    const unsigned* table;         // [64]: the 256 bytes of the map as they lie
    int identity;                  // the map is the identity: no table, no LDS map
    int form;                      // kTransposeGather | kTransposeRows | kTransposeTile
};
enum { kTransposeGather = 0, kTransposeRows = 1, kTransposeTile = 2 };

// DepthToSpace of a quantised graph (d2s.hip), the CRD order of depthtospace_ref.c: raw bytes, no map --
//   out[n, s, h, w] = in[n, s * r * r + (h % r) * r + (w % r), h / r, w / r]
// uint8: x dense NCHW (N, C * r * r, H, W); y dense NCHW (N, C, H * r, W * r), or a channel range of a Concat's NCHW buffer (out_img /
// out_c0: planes at any byte offset)
// which of the two forms a DepthToSpace node takes when TAMD_PIN=d2s_form does not say: 1, the kernels of d2s.hip, from this many output
// bytes on; below, 0: the canonical gather of transpose.hip (where the output is one dense run, which is all that kernel writes).  What
// was measured decides it (profiles/d2s.txt): from 1 MiB to 14 MB d2s_u8 and d2s_i8 are ahead of the gather with the ranges apart
// (2.67 against 4.72 us at 1 MiB, 4.58 against 30.3 us at 11 MB); at 256 KB and 389 KB the gather is ahead in uint8 (3.05 against 3.39 us,
// 3.03 against 4.57 us) and level in int8 (2.63 against 2.64 us).  Between 389 KB and 1 MiB nothing was measured: the threshold stands at
// the smallest size measured as a win
constexpr size_t kD2sNewFormFromBytes = (size_t)1 << 20;
struct D2sU8Args {
    const uint8_t* x; uint8_t* y;
    int N, C, H, W;                // C: OUTPUT channels; H, W: the INPUT map
    int r;
    long out_img; int out_c0;      // bytes per image of the buffer y lies in, first channel of y in it
};
// int8: NHWC with padded pixel strides.  x: first channel of the input (a view's channel offset applied), pixel stride cs_in, read where
// it lies; y: base of the output buffer, pixel stride ldc, channel offset c_off (a concat view).  Whole 16-byte channel vectors are
// stored, the lanes from C on as ZERO: c_off, ldc multiples of 16, c_off + rup(C, 16) <= ldc (launch_d2s_i8 checks)
struct D2sI8Args {
    const int8_t* x; int8_t* y;
    int N, C, H, W;                // C: OUTPUT channels; H, W: the INPUT map
    int r, cs_in, ldc, c_off;
    size_t src_bytes;              // bytes of the buffer x points into, from x on: every read stays below (launch_d2s_i8 checks)
    int fix128;                    // 1: the output is a view of a Concat of several inputs, whose copy stores 127 for the byte -128 (epilogue.h: fix128_4)
};

// Nearest Resize at whole-number factors, the replicate form (resize.hip): output pixel (h, w) = table[input pixel (h / sh, w / sw)],
// OH = H * sh, OW = W * sw, ONE image (the reference defines the operator for batch 1 only).  A lane owns SOURCE data, maps it once and
// stores its copies; no index vectors, no divisions by the output's extents.  Form 0 of a Resize node is interp.hip's kernel fed with
// Resize's index vectors and table (InterpI8Args / InterpU8Args), legal for every node; this form is legal where node_rules.h:
// ResizeGeom::sh / sw are set.
// which form a Resize node takes when TAMD_PIN=resize_form does not say: 1 from this many OUTPUT bytes on, where it is legal; 0 below.
// What was measured decides it (profiles/resize.txt, x2, us per launch, ranges of seven alternating rounds).  uint8: resize_rep_u8 is
// ahead with the ranges apart at 1.6 MB (3.23 against 5.51), 4 MiB (3.69 against 11.69) and 6.5 MB (4.55 against 17.12), and behind at
// 205 KB (4.06 against 3.65, ranges touching).  int8: resize_rep_i8 is ahead with the ranges apart at 6.5 MB alone (3.70 against 4.78);
// at 205 KB, 1.6 MB and 4 MiB its median is lower (3.02 / 3.22 / 3.38 against 3.22 / 3.43 / 3.82) but the ranges overlap.  Each
// threshold stands at the smallest size measured as a win; between the measured sizes nothing is known
constexpr size_t kResizeRepFromBytesU8 = 1638400, kResizeRepFromBytesI8 = 6553600;
// int8: NHWC with padded pixel strides.  x: first channel of the input (a view's channel offset applied), pixel stride cs_in, read where
// it lies; y: base of the output buffer, pixel stride ldc, channel offset c_off (a concat view).  Whole 16-byte channel vectors are
// stored, the lanes from C on as ZERO: c_off, ldc multiples of 16, c_off + rup(C, 16) <= ldc (launch_resize_rep_i8 checks)
struct ResizeRepI8Args {
    const int8_t* x; int8_t* y;
    int C, H, W;                   // the INPUT map
    int sh, sw, cs_in, ldc, c_off;
    const unsigned* table;         // [64]: tamd_resize_table's 256 bytes as they lie
};
// uint8: x dense NCHW (1, C, H, W); y dense NCHW (1, C, H * sh, W * sw), or a channel range of a Concat's NCHW buffer (out_c0: planes at
// any byte offset; out_img: the bytes of the image y lies in)
struct ResizeRepU8Args {
    const uint8_t* x; uint8_t* y;
    int C, H, W;                   // the INPUT map
    int sh, sw;
    long out_img; int out_c0;
    const unsigned* table;
    int identity;                  // the table maps every byte to itself: no lookups
};

// The top-down merge of a feature pyramid in a uint8 graph, nearest Interp -> Crop -> same-shape Eltwise, as one launch (topdown.hip).
// All three tensors dense NCHW; lat and y have the output's dims (N, C, OH, OW) and are 16-byte aligned.  Per output byte
//   u = table[small[n][c][iy[h]][ix[w]]]          (the Interp's byte map; iy / ix: its index vectors, shifted and cut by the Crop's box)
//   y = requant(deq(u; su, zu) op deq(lat; sl, zl))  with the operands in the node's order (u_first), the chain of eltwise_u8_k
struct TopdownU8Args {
    const uint8_t* small; const uint8_t* lat; uint8_t* y;
    long planes;                   // N * C
    int H, W, OH, OW;              // the small map, the output map; every iy[h] < H, ix[w] < W (the planner checks the tables it uploads)
    const int* iy; const int* ix;  // [OH], [OW]
    const unsigned* table;         // [64]: the Interp's 256-byte map as it lies
    int identity;                  // the map is the identity: no lookups
    int type, u_first;             // ELT_PROD 0, SUM 2, SUB 4, MAX 6; 1: the cropped operand is the Eltwise's input 0
    float su, sl, out_scale;       // u is dequantised with the CROP OUTPUT's parameters (the Eltwise reads that tensor), lat with its own
    int zu, zl, out_zp;
};

// PReLU of a quantised graph (prelu.hip; the host truth: prelu_tables.cc)
struct PreluI8Args {       // NHWC int8, x and y of one pixel stride: y = requant(x < 0 ? x * slope[c] : x), the chain of relu_i8 per channel
    const int8_t* x; int8_t* y;
    size_t count;          // N * H * W * cs bytes
    int C, cs;             // cs (a multiple of 16) bytes per pixel, C of them channels; the padding lanes [C, cs) are written 0
    const float* slope;    // [cs]: tamd_prelu_slope of every channel's fp16 slope, zeros behind C; 16-byte aligned
    float in_scale, out_scale;
};

struct PreluU8Args {       // dense NCHW uint8: plane p = n * C + c of HW bytes is mapped through the byte table of channel c
    const uint8_t* x; uint8_t* y;      // both 16-byte aligned, so a plane starts at the same offset in its 16 bytes on either side
    long planes;           // N * C
    int C, HW;
    const unsigned* tables;// [C][64] (shared: [1][64]): tamd_prelu_table's 256 bytes of every channel as they lie
    int shared;            // one slope, one table, for every channel
};

// The channel gate of a Squeeze-and-Excitation block (chan_gate.hip): y = requant(x op gate), x (N, C, H, W), gate (N, C, 1, 1), op PROD 0 |
// SUM 2 | SUB 4 as x op gate (eltwise_ref.c: the operand with more elements comes first whichever input it is).  table != nullptr: the
// gate bytes are the INPUT of the byte-map node in front of the gate (Sigmoid, Clip, ..) and go through that node's table first
struct ChanGateI8Args {    // NHWC int8: x and y N * HW pixels of cs bytes, the gate N pixels of cs bytes; all three 16-byte aligned
    const int8_t* x; const int8_t* gate; int8_t* y;
    int N, HW, C, cs;      // cs (a multiple of 16) bytes per pixel, C of them channels; the padding lanes [C, cs) of y are written 0
    int type;
    float sx, sg, out_scale;
    const unsigned* table; // [64]: tamd_lut_table's 256 bytes as they lie, or nullptr
    int iters;             // pixels a lane walks in turn; 0: the launcher's rule (by the size of the tensor)
};

struct ChanGateU8Args {    // dense NCHW uint8: plane p = n * C + c of HW bytes has the one gate byte gate[p]
    const uint8_t* x; const uint8_t* gate; uint8_t* y;      // x and y 16-byte aligned and laid out alike
    long planes;           // N * C
    int HW;
    int type;
    float sx, sg, out_scale;
    int zx, zg, out_zp;
    const unsigned* table; // as above
};

struct SoftmaxI8Args {     // softmax over ONE axis of an int8 tensor: the channels of an NHWC tensor (a view's channel slice included), or --
                           // round 6 -- any axis of a dense (reference-order) or NHWC tensor
    const int8_t* x; int8_t* y;
    long positions;        // the (outer, inner) index pairs: N * H * W for the channel axis
    int C, cs_in, cs_out;  // C = length of the axis.  Position p starts at p * cs_in / p * cs_out ...
    float in_scale, out_scale;
    // ... unless d1 > 0 (the general form): start = (p / d1) * s1 + ((p % d1) / d2) * s2 + (p % d2), element j of the axis `stride`
    // bytes further on; i-fields for the input, o-fields for the output.  Dense [outer][A][inner]: d1 = d2 = inner, s1 = A * inner, s2 = 0,
    // stride = inner.  NHWC over W: d1 = d2 = C, s1 = W * cs, stride = cs.  NHWC over H: d1 = W * C, d2 = C, s1 = H * W * cs, s2 = cs,
    // stride = W * cs.
    long d1, d2;
    long is1, is2, os1, os2;
    long istride, ostride;
};
constexpr int kSoftmaxI8MaxC = 16000;      // the axis' exponentials live in LDS as floats (<= 64 KB with the chain's padding)

struct CatCopyArgs {       // one concat input that cannot be written in place: (re-scaling) copy into its channel slice
    const int8_t* x; int8_t* y;
    long pixels;
    int C, cs_in, ldc, c_off;
    float rescale;         // in_scale / out_scale
    int identity;          // plain byte copy (single-input concat)
};

// ---- int8 tensors in the reference's DENSE element order (round 6: the SSD head plumbing of an int8 graph -- Permute(0,2,3,1), Flatten,
// Reshape, Concat on any axis, PriorBox).  One launch copies up to kFlatCatMax inputs of a Concat into their slots of every outer slice
// of the dense output, each read in the element order the reference sees and re-scaled as concat_kernel_ref_int8.c does.
struct FlatCatI8Src {
    const int8_t* x;
    int kind;              // 0: dense, element e of outer slice o at o * chunk + e
                           // 1: NHWC tensor seen through Permute(0,2,3,1) (+ Flatten): e = p * C + c   -> (o * HW + p) * cs + c
                           // 2: NHWC tensor in NCHW element order: L = o * chunk + e = (n * C + c) * HW + p   -> (n * HW + p) * cs + c
    int chunk;             // elements per outer slice
    int C, HW, cs;
    int begin;             // first element of this input inside an output slice
    float rescale;         // in_scale / out_scale
    int identity;          // plain byte copy (single-input concat, a lone Permute / layout copy)
};
constexpr int kFlatCatMax = 8;
struct FlatCatI8Args {
    FlatCatI8Src src[kFlatCatMax];
    int nsrc;
    int8_t* y;
    long outer;
    int out_row;           // elements of one outer slice of the output
    int row_begin, row_len;   // this launch covers [row_begin, row_begin + row_len) of every slice
};

struct LayoutArgs {        // NCHW <-> NHWC(cs) int8 / generic element size
    const void* src; void* dst; int N, C, H, W, cs; int elem;
};

// launchers (return hipError_t of the launch)
hipError_t launch_conv_igemm(const ConvArgs& a, hipStream_t s);
const char* conv_igemm_kernel_name(const ConvArgs& a);   // tile shape the launcher will pick
int conv_igemm_num_cfgs();                               // ConvArgs::cfg values the autotuner may try
bool conv_igemm_cfg_ok(const ConvArgs& a, int cfg);
hipError_t launch_gemm_direct(const ConvArgs& a, hipStream_t s);   // 1x1, small-M / latency-bound shapes
bool gemm_direct_applicable(const ConvArgs& a);
hipError_t launch_conv_igemm2(const ConvArgs& a, hipStream_t s);  // LDS-DMA 3-stage ring, large problems
bool conv_igemm2_applicable(const ConvArgs& a);
const char* conv_igemm2_kernel_name(const ConvArgs& a);
// lean-loop implicit GEMM: fragment-ordered weights by LDS-DMA, k x k activations as an LDS-resident input patch (conv_pgemm.hip)
int conv_pgemm_num_variants();
int conv_pgemm_bn(int variant);                                    // cout tile of a variant (the weight packing unit)
bool conv_pgemm_applicable(const ConvArgs& a, int variant);
void conv_pgemm_prepare(ConvArgs& a, int variant);                 // fills pg_* / mg_hp / mg_wp
size_t conv_pgemm_packed_bytes(const ConvArgs& a, int bn);
void conv_pgemm_pack(const ConvArgs& a, const int8_t* w, int cout_pad, int bn, int8_t* out);   // w: [cout_pad][kpad] family layout
const char* conv_pgemm_kernel_name(const ConvArgs& a);
hipError_t launch_conv_pgemm(const ConvArgs& a, hipStream_t s);
// wave-grid form for 3x3 (conv_pgemm_w.hip): variants 16 .. 31 of the family above; the same packed weights, plus a geometry table
bool conv_pgemm_w_applicable(const ConvArgs& a, int variant);
void conv_pgemm_w_prepare(ConvArgs& a, int variant);               // fills pg_* except pg_tab
void conv_pgemm_w_table(const ConvArgs& a, std::vector<int>& out); // after prepare: the table the planner uploads (pg_tab)
const char* conv_pgemm_w_kernel_name(const ConvArgs& a);
hipError_t launch_conv_pgemm_w(const ConvArgs& a, hipStream_t s);
hipError_t launch_pw_stream(const ConvArgs& a, hipStream_t s);     // 1x1, shallow K, many pixels
bool pw_stream_applicable(const ConvArgs& a);
hipError_t launch_pw_rows(const ConvArgs& a, hipStream_t s);       // 1x1, shallow K, many pixels: row-major epilogue, persistent pipelined waves
bool pw_rows_applicable(const ConvArgs& a);
hipError_t launch_conv_first(const FirstArgs& a, hipStream_t s);
bool dwpw_pw_shape_ok(int cout, int map_w, int KH, int KW, int SH, int SW, bool pads);   // the pointwise consumer's shape alone: what the planner can ask before it plans it
bool dwpw_applicable(const DwArgs& d, const ConvArgs& p);
size_t dwpw_packed_bytes(int cout, int cin);
void dwpw_pack(const int8_t* w, int cout, int cin, int8_t* out);        // w: [cout][cin] (OIHW, 1x1)
hipError_t launch_dwpw(const DwPwArgs& a, hipStream_t s);
// identity bottleneck block in one launch (block_i8.hip).  a / b: branch2a / branch2b as planned; c: branch2c WITH its eltwise tail
bool block_applicable(const ConvArgs& a, const ConvArgs& b, const ConvArgs& c);
bool block_conv_shape_ok(int k, int KH, int KW, int SH, int SW, int DH, int DW, int p_h0, int p_h1, int p_w0, int p_w1);   // k = 1 (branch2a / 2c) or 3 (branch2b): a node's shape alone ..
bool block_channels_ok(int C, int mid, int cout);                                                                        // .. and the channel counts: what the planner can ask before it plans the three
BlockArgs block_args(const ConvArgs& a, const ConvArgs& b, const ConvArgs& c, const int8_t* wpk);     // (after block_applicable)
hipError_t launch_block(const BlockArgs& a, hipStream_t s);
bool conv_first_pool_applicable(const FirstArgs& c, const PoolArgs& p);
FirstPoolArgs conv_first_pool_args(const FirstArgs& c, const PoolArgs& p);
hipError_t launch_conv_first_pool(const FirstPoolArgs& a, hipStream_t s);
int conv_first_kwp(int C, int KH, int KW, int DW);
hipError_t launch_dwconv3x3(const DwArgs& a, hipStream_t s);
const char* dwconv3x3_kernel_name(const DwArgs& a);   // variant <stride, fragments per row> the launcher will pick
hipError_t launch_conv_direct(const DirectArgs& a, hipStream_t s);
hipError_t launch_pwdw(const PwDwArgs& a, int threads, hipStream_t s);
size_t pwdw_lds_bytes(const PwDwArgs& a, int threads);
#ifdef TAMD_PWDW_CHAIN_EXPERIMENT
int pwdw_chain_variant(const PwDwArgs& a, int threads, int* gx, int* gy, int* gz);
hipError_t launch_pwdw_chain(const PwChainArgs& c, int threads, size_t lds, hipStream_t s);
#endif
bool pwdw_config_ok(const PwDwArgs& a, int threads);
hipError_t launch_chain4(const Chain4Args& a, int threads, hipStream_t s);
size_t chain4_lds_bytes(const Chain4Args& a);
bool chain4_config_ok(const Chain4Args& a, int threads);
int pwdw_steps(int nsteps);
hipError_t launch_pool(const PoolArgs& a, hipStream_t s);
hipError_t launch_relu_pool(const ReluPoolArgs& a, hipStream_t s);   // (never the global form)
hipError_t launch_upsample_i8(const UpsampleI8Args& a, hipStream_t s);
hipError_t launch_eltwise(const EltArgs& a, hipStream_t s);
hipError_t launch_relu(const ReluArgs& a, hipStream_t s);
hipError_t launch_lut(const LutArgs& a, hipStream_t s);
hipError_t launch_interp_i8(const InterpI8Args& a, hipStream_t s);
hipError_t launch_interp_u8(const InterpU8Args& a, hipStream_t s);
hipError_t launch_chan_map_i8(const ChanMapI8Args& a, hipStream_t s);
hipError_t launch_chan_map_g2(const ChanMapG2Args& a, hipStream_t s);
hipError_t launch_chan_map_u8(const ChanMapU8Args& a, hipStream_t s);
hipError_t launch_slice_u8(const SliceU8Args& a, hipStream_t s);
hipError_t launch_topdown_u8(const TopdownU8Args& a, hipStream_t s);
hipError_t launch_d2s_u8(const D2sU8Args& a, hipStream_t s);
hipError_t launch_d2s_i8(const D2sI8Args& a, hipStream_t s);
hipError_t launch_resize_rep_i8(const ResizeRepI8Args& a, hipStream_t s);
hipError_t launch_resize_rep_u8(const ResizeRepU8Args& a, hipStream_t s);
// which forms a geometry is legal in, and the default among them (transpose.hip: the one place it is decided)
bool transpose_form_legal(const TransposeArgs& a, int form);
int transpose_default_form(const TransposeArgs& a);
const char* transpose_kernel_name(int form);
hipError_t launch_transpose(const TransposeArgs& a, hipStream_t s);
hipError_t launch_prelu_i8(const PreluI8Args& a, hipStream_t s);
hipError_t launch_prelu_u8(const PreluU8Args& a, hipStream_t s);
// A byte map per channel over a dense uint8 tensor [N][C][HW] (chan_lut.hip): y[i] = tables[c(i)][x[i]], c(i) = (i / HW) % C
struct ChanLutU8Args {
    const uint8_t* x; uint8_t* y;      // both 16-byte aligned: chunk k is bytes [16k, 16k + 16) of either
    size_t total;          // N * C * HW bytes
    int C, HW;
    const unsigned* tables;// [C][64]: the 256 bytes of every channel's map as they lie
};
hipError_t launch_chan_lut_u8(const ChanLutU8Args& a, hipStream_t s);
hipError_t launch_chan_gate_i8(const ChanGateI8Args& a, hipStream_t s);
hipError_t launch_chan_gate_u8(const ChanGateU8Args& a, hipStream_t s);
hipError_t launch_softmax_i8(const SoftmaxI8Args& a, hipStream_t s);
hipError_t launch_concat_copy_i8(const CatCopyArgs& a, hipStream_t s);
hipError_t launch_flatcat_i8(const FlatCatI8Args& a, hipStream_t s);
hipError_t launch_copy_bytes(void* dst, const void* src, size_t bytes, hipStream_t s);   // 16-byte aligned buffers
hipError_t launch_nchw_to_nhwc(const LayoutArgs& a, hipStream_t s);
hipError_t launch_nhwc_to_nchw(const LayoutArgs& a, hipStream_t s);

// ---- uint8 (per-tensor asymmetric) ---------------------------------------------------------------------------
// The reference SIMULATES uint8 in fp32: operands are dequantised, the convolution is an fp32 GEMM
// whose per-element summation order is fixed by the reference's register tiling, and only the result is
// requantised.  Byte-identical outputs therefore need the same fp32 operations in the same order: one fused
// multiply-add chain per output element -- which is exactly how v_mfma_f32_16x16x4f32 accumulates (measured,
// profiles/r01_mfma_f32_is_sequential_fma_chain.txt), so the path runs on the matrix cores (u8_conv_*.hip, u8_kernels.hip).
// uint8 activations stay in the reference's dense NCHW order on the device.
struct U8Q { float scale; int zp; };
// a ReLU node folded into the producing conv: applied to the conv's own uint8 result in registers
// (relu_kernel_ref_uint8.c:48-95 on that byte), so the bytes equal the two-launch sequence
struct U8Relu { int on; float slope; U8Q out; };

// uint8 InstanceNorm over a dense NCHW tensor (instnorm.hip): a wave per plane p = n * C + c of HW bytes computes the plane's two
// sequential fp32 sums, a and b, and the plane's 256-entry byte map (tamd_instancenorm_plane is the specification).
// instnorm_stats_u8 stores the map as tables[p][64] dwords for a chan_lut_u8 launch with C := planes; instnorm_u8 keeps it in a
// register per lane and maps its own plane to y.  relu.on: the ReLU node behind, composed into the map (fused_relu on the map's byte)
struct InstNormU8Args {
    const uint8_t* x; uint8_t* y;      // both 16-byte aligned (y: instnorm_u8 only)
    long planes;                       // N * C
    int C, HW;
    const float* gamma; const float* beta;      // [C] each
    float eps;
    U8Q in, out;
    U8Relu relu;
    unsigned* tables;                  // [planes][64] (instnorm_stats_u8 only)
};
hipError_t launch_instnorm_stats_u8(const InstNormU8Args& a, hipStream_t s);
hipError_t launch_instnorm_u8(const InstNormU8Args& a, hipStream_t s);

struct U8PoolFuse {            // a 2x2 / stride 2 / unpadded MAX-pool node applied to the conv's final bytes in the conv epilogue
    int on;                    // the kernel then enumerates output pixels window-major: j = 4 * window + 2 * dy + dx (so the four
                               // pixels of a window sit in four neighbouring lanes); needs OH, OW even and OH*OW % 8 == 0
    int write_full;            // the unpooled tensor has other readers (or is a graph output): store it as well
    uint8_t* y;                // pooled output, NCHW, image stride out_img bytes, first channel at out_c0
    int out_img, out_c0;
    U8Q in, out;               // quantisation of the pool node's input (== what the conv epilogue produced) and output
};

struct U8ConvArgs {            // group == 1: conv_kernel_x86.c sgemm_fp order (u8_conv_gemm.hip: conv_u8_gemm)
    const uint8_t* x;          // NCHW
    const uint8_t* wq;         // raw uint8 weights, [cout tile of BM][stage of 32 k][BM rows][32 slots]; BM =
                               // conv_u8_gemm_bm(cfg); slot of k inside its stage: (k%4)*8 + (k%32)/4 (class-major);
                               // padding holds the weight zero point (dequantises to exactly 0)
    const unsigned* klut;      // [Kpad] packed tap table: (c*H*W + ky*DH*W + kx*DW) | kx*DW << 24 | ky*DH << 28
                               // (padding rows: 0 -- their weights are 0 and fma(x, 0, s) == s for finite x)
    const int32_t* bias;       // may be null
    uint8_t* y;                // NCHW, image stride out_img bytes, first channel at out_c0
    int N, C, H, W, OH, OW, cout, cout_pad, K, Kpad;
    int SH, SW, PH, PW;
    int out_img, out_c0;       // bytes per output image / channel offset (concat outputs are written in place)
    int cfg;                   // conv_u8_gemm_pick(): block tile (channels x pixels)
    int m_blocked;             // rows below this sit in an 8- or 4-row block of the reference's sgemm_fp
    float in_scale, in_zp;     // zero point as float (exact)
    float w_scale, w_zp;
    float bias_scale;          // in_scale * w_scale
    int act;
    float out_scale; int out_zp;
    U8Relu relu;               // fused ReLU / leaky ReLU node (y, out_img, out_c0 then describe ITS output)
    const float* wf;           // conv_u8_rgb3x3 only: dequantised weights, [cout][wf_ld] rows in OIHW k order
    int wf_ld;
    U8PoolFuse pool;           // fused max-pool node (conv_u8_gemm main tiles and conv_u8_rgb3x3)
    // conv_u8_patch (u8_conv_patch.hip): the main pixels (j < (OH*OW)&~7) from an LDS-resident fp32 input patch
    const uint8_t* wpk;        // DEQUANTISED weights (floats) in MFMA A-fragment order, [16-row tile][super-step of 4*SS k][float4 group][lane]
    int pk_cfg;                // -1: not used; else tile configuration of launch_conv_u8_patch
    int pk_npad, pk_wp;        // floats per channel plane of the patch (3x3: 256 | 512, 1x1: the pixel tile) / patch row pitch (input columns incl. halo)
    int pk_kh, pk_kw, pk_dh, pk_dw;    // filter shape / dilation (the GEMM kernel gets them through klut)
    int pk_tw;                 // 0: a pixel tile is a run of consecutive pixels (rows of the whole map width in the patch); > 0 (round 4): 2-D pixel
                               // tiles of 8 rows x pk_tw columns (= the configuration's pixel-tile size / 8), the patch is the tile + its halo
    // conv_u8i (u8i_kernels.hip): the opt-in INTEGER path -- exact int32 sums on the int8 MFMA, results within one step of the reference
    const int8_t* iw;          // (w ^ 0x80) in MFMA A-fragment order [cout tile][step = (32-channel chunk, tap)][32-row fragment][lane][16 B]
    const int32_t* icv;        // per output channel: bias - alpha * sum_k w'_k + Kp * alpha * beta, padded to the cout tile
    int i_cfg, i_npad, i_nchunks;      // tile configuration / pixels per patch granule plane (128 | 256 | 512) / 32-channel chunks
    int i_cgs;                 // log2 of the 32-channel groups a chunk (= one barrier) holds: 0 | 1 | 2
    int i_dbg;                 // anatomy runs only (TAMD_U8I_ABLATE): 1 no stores, 2 no requantisation, 4 no input loads -- wrong bytes by design
    int i_tw;                  // 0: linear pixel tiles; 8 | 16: 2-D tiles of this width (maps too wide for a linear tile's bounding box)
    int i_alpha, i_beta;       // in_zp - 128, w_zp - 128
    float i_m;                 // requantisation multiplier fl(fl(in_scale * w_scale) / out_scale) (u8_epilogue.h: u8i_requant)
    int i_qlo, i_qhi;          // clamp window of the result: [0, 255] narrowed by the conv's own activation
};

struct U8DirectArgs {          // grouped / depthwise: conv_kernel_ref_uint8.c order (conv_u8_direct), also FC
    const uint8_t* x; const float* wf;   // wf: [cout][cin_g*KH*KW] dequantised weights, OIHW order
    const int32_t* bias; uint8_t* y;
    int N, C, H, W, OH, OW, cout, KH, KW, SH, SW, PH, PW, DH, DW, group;
    int out_img, out_c0;
    float in_scale, in_zp, w_scale;
    int act;
    float out_scale; int out_zp;
    U8Relu relu;
};

struct U8FcArgs {              // fc_ref.c:121-207
    const uint8_t* x; const float* wf;   // wf: [hidden][nout_pad] dequantised, zero padded
    const int32_t* bias; uint8_t* y;
    int batch, hidden, nout, nout_pad;
    float in_scale, in_zp, bias_scale, out_scale; int out_zp;
};

struct U8PoolArgs {
    const uint8_t* x; uint8_t* y;
    int N, C, H, W, OH, OW, KH, KW, SH, SW, PH, PW, method, caffe_flavor;
    U8Q in, out;
};

struct U8MapArgs {             // relu / leaky, concat slice copy, nearest upsample: one output byte per input byte
    const uint8_t* x; uint8_t* y;
    int N, C, H, W;            // INPUT geometry
    int out_img, out_c0;       // output image stride (bytes) / channel offset (concat)
    int scale;                 // upsample factor (1 otherwise)
    float slope;               // relu
    U8Q in, out;
};

struct U8CatArgs {             // flat per-image slice copy: concat on axis 1 of any rank, Permute(0,2,3,1), or both at once
    const uint8_t* x; uint8_t* y;
    int N, in_img;             // images, bytes per input image
    int perm_c, perm_p;        // 0: source index == j; else source = (j % perm_c) * perm_p + j / perm_c  (NCHW read in NHWC order)
    int out_img, out_off;      // output image stride / byte offset of this slice inside the output image
    int identity;              // 1: plain byte copy (permute, or concat input carrying the output's scale and zero point)
    U8Q in, out;
};

struct U8CatMulti {            // every input of one concat node in ONE launch (blockIdx.z = input): MobileNet-SSD's mbox_loc / mbox_conf
    U8CatArgs src[8];
    float rescale[8];
    int count;
};
hipError_t launch_flatcat_multi_u8(const U8CatMulti& m, hipStream_t s);

struct U8SoftmaxArgs {         // softmax over the middle axis of [outer][on][inner]
    const uint8_t* x; uint8_t* y;
    int outer, on, inner;
    U8Q in, out;
};

struct U8EltArgs {
    const uint8_t* a; const uint8_t* b; uint8_t* y; size_t count; int type;
    U8Q qa, qb, out;
};

int conv_u8_gemm_pick(const U8ConvArgs& a);        // geometry fields only
int conv_u8_gemm_bm(int cfg);                      // channel rows per block tile (weight packing unit)
int conv_u8_gemm_kc(int cfg);                      // K stage depth (weight packing unit)
int conv_u8_gemm_num_cfgs();
size_t conv_u8_gemm_lds(const U8ConvArgs& a);      // dynamic LDS bytes of the chosen configuration
hipError_t launch_conv_u8_gemm(const U8ConvArgs& a, hipStream_t s);
// main pixels from an LDS-resident fp32 patch (3x3 and 1x1, group 1); tail pixels, if any, on the VALU by extra blocks of the same launch
int conv_u8_patch_num_cfgs();
int conv_u8_patch_lanes_cfg();                                      // the configuration index of the lane-level chain kernel (conv_u8_lanes)
int conv_u8_patch_bm(int cfg);
int conv_u8_patch_ss(const U8ConvArgs& a);                         // MFMA steps per super-step (9: 3x3, 4: 1x1); 0: shape not supported
bool conv_u8_patch_prepare(U8ConvArgs& a, int cfg, int KH, int KW, int DH, int DW);     // fills pk_*; false: not applicable
const char* conv_u8_patch_kernel_name(const U8ConvArgs& a);
size_t conv_u8_patch_packed_bytes(const U8ConvArgs& a);
void conv_u8_patch_pack(const U8ConvArgs& a, const uint8_t* w, uint8_t w_zp, float w_scale, float* out);       // w: [cout][K] as in the model
hipError_t launch_conv_u8_patch(const U8ConvArgs& a, hipStream_t s);
// shallow pointwise layers of large maps (K = 32 | 64): weights resident in registers, B straight from the NCHW input, one wave per tile
bool conv_u8_pw_applicable(const U8ConvArgs& a, int KH, int KW);
const char* conv_u8_pw_kernel_name(const U8ConvArgs& a);
// shallow 3x3 layers of large maps (C = 16 | 32): weights resident in registers, the 3x3 gather straight from the NCHW input, one wave per tile
bool conv_u8_c3_applicable(const U8ConvArgs& a, int KH, int KW, int DH, int DW);
const char* conv_u8_c3_kernel_name(const U8ConvArgs& a);
hipError_t launch_conv_u8_c3(const U8ConvArgs& a, hipStream_t s);
hipError_t launch_conv_u8_pw(const U8ConvArgs& a, hipStream_t s);
// the integer path (u8i_kernels.hip); shares U8ConvArgs (geometry, fused ReLU / max-pool tails) with the byte-exact kernels
int conv_u8i_num_cfgs();
int conv_u8i_bm(int cfg);
bool conv_u8i_prepare(U8ConvArgs& a, int cfg, int KH, int KW, int DH, int DW);          // fills i_cfg / i_npad / i_nchunks / pk_k*; false: not applicable
size_t conv_u8i_packed_bytes(const U8ConvArgs& a, int bm);                          // bm: channel rows of a block tile (conv_u8i_bm / conv_u8i_pw_bm)
void conv_u8i_pack(const U8ConvArgs& a, int bm, const uint8_t* w, int w_zp, int in_zp, const int32_t* bias, int8_t* out, int32_t* cvec);    // w: [cout][K] as in the model
// pointwise layers (1x1, stride 1, no padding): register-only transposes, no LDS, dword stores
int conv_u8i_pw_num_cfgs();
int conv_u8i_pw_bm(int cfg);
int conv_u8i_pw_bn(int cfg);
bool conv_u8i_pw_prepare(U8ConvArgs& a, int cfg, int KH, int KW);
const char* conv_u8i_pw_kernel_name(const U8ConvArgs& a);
hipError_t launch_conv_u8i_pw(const U8ConvArgs& a, hipStream_t s);
const char* conv_u8i_kernel_name(const U8ConvArgs& a);
hipError_t launch_conv_u8i(const U8ConvArgs& a, hipStream_t s);
// first layers of the integer path (3x3, <= 4 input channels): the whole K in one v_mfma_i32_16x16x64_i8
bool conv_u8i_rgb_applicable(const U8ConvArgs& a, int KH, int KW, int DH, int DW);
void conv_u8i_rgb_prepare(U8ConvArgs& a);          // fills i_npad (patch pixels of a full 16x16 window)
size_t conv_u8i_rgb_packed_bytes(const U8ConvArgs& a);
void conv_u8i_rgb_pack(const U8ConvArgs& a, const uint8_t* w, int w_zp, int in_zp, const int32_t* bias, int8_t* out, int32_t* cvec);
hipError_t launch_conv_u8i_rgb(const U8ConvArgs& a, hipStream_t s);
bool conv_u8_rgb3x3_applicable(int cin, int kh, int kw, int dh, int dw, int group);
hipError_t launch_conv_u8_rgb3x3(const U8ConvArgs& a, hipStream_t s);
const char* conv_u8_rgb3x3_kernel_name(const U8ConvArgs& a);      // "conv_u8_rgb3x3_mfma" (main pixels on the matrix cores) | "conv_u8_rgb3x3"
const char* conv_u8_gemm_kernel_name(const U8ConvArgs& a);
hipError_t launch_conv_u8_direct(const U8DirectArgs& a, hipStream_t s);

// group == 1 convolution as an fp32 GEMM on the matrix cores, operands streamed with LDS-DMA (conv_f32_mfma.hip).
// Serves uint8 models (x = dequantised copy of the byte tensor, uint8 epilogue) and fp32 models (fp32 epilogue).
struct F32ConvArgs {
    const float* x;            // NCHW fp32
    const float* w;            // packed fp32 weights: [cout tile of BM][stage of 32 k][row group][64], see graph_u8.hip
    const unsigned* klut;      // [Kpad] packed tap table (as U8ConvArgs::klut)
    const float* zeros;        // >= 4 zero bytes: source of out-of-image taps
    const int32_t* bias;       // uint8 models (may be null)
    const float* bias_f32;     // fp32 models (may be null)
    uint8_t* y;                // uint8 output (NCHW) ...
    float* out_f32;            // ... or fp32 output when non-null
    int N, C, H, W, OH, OW, cout, K, Kpad;
    int SH, SW, PH, PW;
    int out_img, out_c0;       // elements per output image / channel offset
    int cfg, m_blocked;
    int tail_split;            // 1: uint8 models (the reference's tail-pixel summation order); 0: fp32 models (order-free)
    float bias_scale;
    int act;
    float out_scale; int out_zp;
};
int conv_f32_mfma_pick(const F32ConvArgs& a);      // geometry fields only
int conv_f32_mfma_bm(int cfg);
size_t conv_f32_mfma_lds(int cfg);
const char* conv_f32_mfma_kernel_name(const F32ConvArgs& a);
hipError_t launch_conv_f32_mfma(const F32ConvArgs& a, hipStream_t s);
hipError_t launch_dequant_u8_f32(const uint8_t* x, float* y, size_t n, float zp, float scale, hipStream_t s);

// Winograd F(2x2, 3x3) for fp32 3x3 / stride 1 / dilation 1 / group 1 convolutions (winograd_f32.hip): three launches
struct F32WinoArgs {
    const float* x;            // NCHW input
    const float* U;            // transformed weights [16][Mpad][Cpad] (host: G g G^T), zero padded
    const float* bias;         // may be null
    float* V;                  // workspace [16][Cpad][Tpad]: transformed input tiles
    float* M;                  // workspace [16][Mpad][Tpad]: products
    float* y;                  // NCHW output, image stride out_img elements, first channel out_c0
    int N, C, H, W, OH, OW, cout, PH, PW;
    int TH, TW, T, Tpad;       // tiles per image (rows, columns), tiles in total, padded to 64
    int Cpad, Mpad;            // cin padded to 16, cout padded to 64
    int out_img, out_c0, act;
};
hipError_t launch_wino_in_f32(const F32WinoArgs& a, hipStream_t s);
hipError_t launch_wino_gemm_f32(const F32WinoArgs& a, hipStream_t s);
hipError_t launch_wino_out_f32(const F32WinoArgs& a, hipStream_t s);

// ---- fp32 models (f32_kernels.hip): dense NCHW fp32 ------------------------------------------------------------------
struct F32DirectArgs {         // grouped / depthwise convolution
    const float* x; const float* w; const float* bias; float* y;
    int N, C, H, W, OH, OW, cout, KH, KW, SH, SW, PH, PW, DH, DW, group;
    int out_img, out_c0, act;
};
struct F32PoolArgs {
    const float* x; float* y;
    int N, C, H, W, OH, OW, KH, KW, SH, SW, PH, PW, method, caffe_flavor;
};
struct F32MapArgs {            // relu / leaky / relu6, concat slice copy, nearest upsample
    const float* x; float* y;
    int N, C, H, W;            // INPUT geometry
    int out_img, out_c0, scale;
    float slope;
};
hipError_t launch_conv_f32_direct(const F32DirectArgs& a, hipStream_t s);
hipError_t launch_pool_f32(const F32PoolArgs& a, hipStream_t s);
hipError_t launch_map_f32(const F32MapArgs& a, int mode, hipStream_t s);   // 0 relu/leaky, 1 concat copy, 2 upsample, 3 relu6
hipError_t launch_eltwise_f32(const float* a, const float* b, float* y, size_t count, int type, hipStream_t s);
hipError_t launch_softmax_f32(const float* x, float* y, int N, int C, int inner, hipStream_t s);
hipError_t launch_fc_u8(const U8FcArgs& a, hipStream_t s);
hipError_t launch_pool_u8(const U8PoolArgs& a, hipStream_t s);
hipError_t launch_relu_u8(const U8MapArgs& a, hipStream_t s);
hipError_t launch_requant_copy_u8(const U8MapArgs& a, hipStream_t s);
hipError_t launch_upsample_u8(const U8MapArgs& a, hipStream_t s);
hipError_t launch_flatcat_u8(const U8CatArgs& a, hipStream_t s);
hipError_t launch_eltwise_u8(const U8EltArgs& a, hipStream_t s);
hipError_t launch_softmax_u8(const U8SoftmaxArgs& a, hipStream_t s);

}  // namespace tamd

// every launch of the backend goes through the launch recorder (launch_rec.h): a plain launch, plus -- while prerun records
// the launch list for direct dispatch -- a copy of what was launched
#include "launch_rec.h"
#undef hipLaunchKernelGGL
#define hipLaunchKernelGGL(kernel, grid, block, shmem, stream, ...) ::tamd::launch_rec(kernel, grid, block, shmem, stream, __VA_ARGS__)
