// FOUR int8 nodes in one launch: producer conv -> depthwise 3x3 (stride 1) -> pointwise conv -> depthwise 3x3 (stride 1 | 2).
// The producer is the network's first convolution, gathered from the NCHW graph input (PROD 1, pwdw.hip's patch-row gather), or a
// pointwise conv of an NHWC tensor (PROD 0).  MobileNet-v1 batch 1: conv1 + conv2_1/dw + conv2_1/sep + conv2_2/dw, and
// conv2_2/sep + conv3_1/dw + conv3_1/sep + conv3_2/dw -- each two pwdw.hip launches before, one here.
//
// Why: the batch-1 pass is a chain of dependent packets at ~3.4 us each whatever they compute, so the lever is the
// packet count.  pwdw.hip gives a block a CHANNEL slice, which makes every layer boundary an all-to-all dependency.  Here a block owns
// a SPATIAL tile with ALL channels: a pointwise conv is per pixel, a depthwise 3x3 needs a one-pixel halo, and in the early layers the
// channel counts are small enough (C1, C2 <= 128) that both weight panels sit in LDS.  The halo is recomputed, nothing is handed from
// block to block, there are no atomics.
//
// Block = one image x one TH x TW tile of the LAST depthwise's outputs x all channels.  Regions are derived OUTWARD from that tile and
// clipped to the map at every level (a position outside its map is the depthwise zero padding: it stays zero in LDS, no GEMM ever
// runs on it -- with a bias it would come out nonzero):
//   C (dw2's input = pw2's output, map H1 x W1): rows oy0*S2 - P2 .. + (th-1)*S2 + 2, clipped -> [cvy0, cvy1)
//   B (pw2's input = dw1's output, same map):    the same clipped rectangle (a pointwise conv is per pixel)
//   A (dw1's input = the producer's output, map H0 x W0): rows cvy0 - P1 .. cvy1 - 1 - P1 + 2, clipped -> [avy0, avy1)
// Phases, a barrier between each:
//   0. everything that depends on the block index only goes out: the weight blob (both pointwise panels in A-fragment order, their
//      bias and multiplier vectors, the four nodes' requantisation constants -- staged ONCE into LDS, <= 27 KB; fragments are then
//      ds_read_b128, and the constants of a phase are read when it starts instead of sitting in 32 scalar registers from the top), this thread's depthwise taps / bias / multipliers of BOTH depthwise nodes (registers), the first activation loads;
//      LDS regions A and C are zeroed
//   1. producer over the clipped A rectangle: v_mfma_i32_16x16x64_i8, accumulator starts at the bias, the producer's own
//      requantisation (epilogue.h) -> int8 -> LDS A [slice][region pixel][16 ch].  A wave takes a 16-pixel tile and ALL slices: the
//      activation operand (the only global load of the phase) is fetched once per tile
//   2. dw1 over the clipped B rectangle from A (dw_common.h: 4x4 byte transposes + one v_dot4 per filter row), its own
//      requantisation -> LDS B [slice][region pixel][16 ch] -- which IS the B-operand layout of the next GEMM: lane (pixel, kb) reads
//      its 16 K bytes of step u with one ds_read_b128 at slice kb + 4u
//   3. pw2 over the same rectangle, work items (16-pixel tile x 16-channel slice) dealt round-robin to the waves -> LDS C
//   4. dw2 from C, its own requantisation, dword stores to the NHWC output
// Same integers, same float operations as the four stand-alone launches: bit-exact with them and with the reference.
#include "dw_common.h"
#include "epilogue.h"
#include "kernels.h"

namespace tamd {

typedef int v4i __attribute__((ext_vector_type(4)));

constexpr int kChain4Stage = 8;       // 16-byte pieces of the weight blob a thread stages at most

// One depthwise 3x3 position of a channel quad from an LDS region [pixel][16 ch] of `pitch` pixels per row: `row` = this thread's dword of
// the window's top-left pixel, `w` its taps, acc = the bias on entry (the dot chain starts there).  The 4th column meets a zero tap; it
// may lie past the region row (the buffer has 4 pixels of slack)
__device__ __forceinline__ void dw3x3_from_lds(const unsigned* row, int pitch, const unsigned (&w)[3][4], int (&acc)[4])
{
#pragma unroll
    for (int r = 0; r < 3; r++) {
        const unsigned d[4] = {row[(r * pitch + 0) * 4], row[(r * pitch + 1) * 4], row[(r * pitch + 2) * 4], row[(r * pitch + 3) * 4]};
        unsigned frag[4];
        transpose4x4(d, frag);
#pragma unroll
        for (int c = 0; c < 4; c++) acc[c] = __builtin_amdgcn_sdot4((int)frag[c], (int)w[r][c], acc[c], false);
    }
}

template <int PROD, bool COH, int WIN>
__device__ __forceinline__ void chain4_block(const Chain4Args& a, unsigned* __restrict__ lds)
{
    const int t = threadIdx.x, nthreads = blockDim.x, lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6), nwaves = nthreads >> 6;
    const int l15 = lane & 15, kb = lane >> 4;
    const int tx = blockIdx.x, ty = blockIdx.y, n = blockIdx.z;
    const int ns1 = a.ns1, ns2 = a.ns2;

    // ---- phase 0: loads that depend on nothing but the block index ---------------------------------------------------------
    uint4 wst[kChain4Stage];
#pragma unroll
    for (int k = 0; k < kChain4Stage; k++) {
        // (pieces past the end re-read the last one instead of branching around the load; they are not stored)
        wst[k] = reinterpret_cast<const uint4*>(a.blob)[min(t + k * nthreads, a.blob_q - 1)];
    }
    // depthwise phases: thread = (pixel, channel quad); quads rounded up to a power of two, the excess threads sit those phases out
    const int cq1 = t & ((1 << a.qsh1) - 1), cq2 = t & ((1 << a.qsh2) - 1);
    const bool on1 = cq1 < ns1 * 4, on2 = cq2 < ns2 * 4;
    const int c1 = (on1 ? cq1 : 0) * 4, c2 = (on2 ? cq2 : 0) * 4;
    unsigned w1[3][4], w2[3][4];
#pragma unroll
    for (int r = 0; r < 3; r++) {
        const uint4 v = *reinterpret_cast<const uint4*>(a.dw1_w + ((size_t)r * ns1 * 16 + c1) * 4);
        w1[r][0] = v.x; w1[r][1] = v.y; w1[r][2] = v.z; w1[r][3] = v.w;
        const uint4 u = *reinterpret_cast<const uint4*>(a.dw2_w + ((size_t)r * ns2 * 16 + c2) * 4);
        w2[r][0] = u.x; w2[r][1] = u.y; w2[r][2] = u.z; w2[r][3] = u.w;
    }
    const int4 db1 = *reinterpret_cast<const int4*>(a.dw1_bias + c1), db2 = *reinterpret_cast<const int4*>(a.dw2_bias + c2);
    const float4 ds1 = *reinterpret_cast<const float4*>(a.dw1_wscale + c1), ds2 = *reinterpret_cast<const float4*>(a.dw2_wscale + c2);

    // ---- geometry of this block (uniform): outward from the output tile, clipped at every level ---------------------------------
    const int S2 = a.S2, RCW = a.RCW, RAW = a.RCW + 2;
    const int oy0 = ty * a.TH, ox0 = tx * a.TW;
    const int th = min(a.TH, a.OH - oy0), tw = min(a.TW, a.OW - ox0);
    const int cy0 = oy0 * S2 - a.P2H, cx0 = ox0 * S2 - a.P2W;                     // origin of regions C and B (may be -1: padding)
    const int cvy0 = max(cy0, 0), cvx0 = max(cx0, 0);
    const int cvy1 = min(cy0 + (th - 1) * S2 + 3, a.H1), cvx1 = min(cx0 + (tw - 1) * S2 + 3, a.W1);
    const int ay0 = cy0 - a.P1H, ax0 = cx0 - a.P1W;                               // origin of region A
    const int avy0 = max(cvy0 - a.P1H, 0), avx0 = max(cvx0 - a.P1W, 0);
    const int avy1 = min(cvy1 + 2 - a.P1H, a.H0), avx1 = min(cvx1 + 2 - a.P1W, a.W0);
    const int AVW = avx1 - avx0, AVP = (avy1 - avy0) * AVW;
    const int CVW = cvx1 - cvx0, CVP = (cvy1 - cvy0) * CVW;
    const float inv_avw = __builtin_amdgcn_rcpf((float)AVW), inv_cvw = __builtin_amdgcn_rcpf((float)CVW);
    const int soffA = ((a.RCH + 2) * RAW + 4) * 4, soffC = (a.RCH * RCW + 4) * 4;   // dwords between the slices' copies of a region (4 pixels of slack)
    unsigned* const ldsA = lds + a.blob_q * 4;
    unsigned* const ldsC = ldsA + ns1 * soffA;
    unsigned* const ldsB = ldsC + ns2 * soffC;
    const int8_t* const wl = reinterpret_cast<const int8_t*>(lds);                // the staged blob

    // producer tile i: lane l15's pixel of the clipped A rectangle -> its slot in region A (lanes past the last pixel re-read the
    // last one instead of branching around their loads; `live` says whether the result is stored)
    int piy = 0, pix = 0;
    auto locate_a = [&](int i, bool& live) -> int {
        const int v = i * 16 + l15, vc = min(v, AVP - 1);
        // v / AVW without an integer division (pwdw.hip: locate)
        const int vy = (int)(((float)vc + 0.5f) * inv_avw), vx = vc - vy * AVW;
        piy = avy0 + vy; pix = avx0 + vx;
        live = v < AVP;
        return (piy - ay0) * RAW + (pix - ax0);
    };
    const int8_t* xn = PROD == 0 ? a.x + (size_t)n * a.H0 * a.W0 * a.cs_in + kb * 16 : a.x + (size_t)n * a.in_C * a.in_H * a.in_W;
    unsigned rows[4];
    if (PROD == 1) {
        const uint4 v = *reinterpret_cast<const uint4*>(a.taps + kb * 4);
        rows[0] = v.x; rows[1] = v.y; rows[2] = v.z; rows[3] = v.w;
    }
    const __amdgpu_buffer_rsrc_t xrsrc = __builtin_amdgcn_make_buffer_rsrc((void*)a.x, 0, 0x7fffffff, 0x00020000);
    auto load_b = [&](v4i (&bf)[2]) {
        if (PROD == 0) {
            const int8_t* xp = xn + (unsigned)((piy * a.W0 + pix) * a.cs_in);
            if (COH) {                 // agent-scope (sc1) loads of the previous launch's write-through output
                const int voff = (int)(xp - a.x);
                bf[0] = __builtin_amdgcn_raw_buffer_load_b128(xrsrc, voff, 0, 16 /* sc1 */);
                if (a.ks0 > 1) bf[1] = __builtin_amdgcn_raw_buffer_load_b128(xrsrc, voff, 64, 16);
            } else {
                bf[0] = *reinterpret_cast<const v4i*>(xp);
                if (a.ks0 > 1) bf[1] = *reinterpret_cast<const v4i*>(xp + 64);
            }
        } else {
            gather_patch_rows(a, xn, rows, piy, pix, bf[0]);       // (dw_common.h; the graph input: ordinary loads in both instances)
        }
    };
    const int ntilesA = (AVP + 15) >> 4;
    v4i b0[2] = {v4i{0, 0, 0, 0}, v4i{0, 0, 0, 0}};
    bool live0;
    int slot0 = locate_a(wave, live0);
    load_b(b0);                                            // the first tile's activations fly while the LDS is prepared

    // zero padding of both depthwise nodes: everything phases 1 and 3 do not overwrite; then the staged blob
    {
        const uint4 z = {0u, 0u, 0u, 0u};
        const int nz = ns1 * (soffA >> 2) + ns2 * (soffC >> 2);
        for (int i = t; i < nz; i += nthreads) reinterpret_cast<uint4*>(ldsA)[i] = z;
#pragma unroll
        for (int k = 0; k < kChain4Stage; k++) {
            const int i = t + k * nthreads;
            if (i < a.blob_q) reinterpret_cast<uint4*>(lds)[i] = wst[k];
        }
    }
    __syncthreads();

    // ---- phase 1: producer over the clipped A rectangle -> LDS A -------------------------------------------------------------------
    {
        const Rq rq = *reinterpret_cast<const Rq*>(wl + a.off_rq + 0 * (int)sizeof(Rq));
        for (int i = wave; i < ntilesA; i += nwaves) {
            if (i != wave) { slot0 = locate_a(i, live0); load_b(b0); }
            for (int s = 0; s < ns1; s++) {
                const int4 pb = *reinterpret_cast<const int4*>(wl + a.off_b0 + (s * 16 + 4 * kb) * 4);
                const float4 ps = *reinterpret_cast<const float4*>(wl + a.off_s0 + (s * 16 + 4 * kb) * 4);
                v4i acc = v4i{pb.x, pb.y, pb.z, pb.w};      // the MFMA chain starts at the bias
                acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(*reinterpret_cast<const v4i*>(wl + ((s * a.ks0) * 64 + lane) * 16), b0[0], acc, 0, 0, 0);
                if (PROD == 0 && a.ks0 > 1)
                    acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(*reinterpret_cast<const v4i*>(wl + ((s * a.ks0 + 1) * 64 + lane) * 16), b0[1], acc, 0, 0, 0);
                const unsigned p = requant4<WIN>(acc[0], acc[1], acc[2], acc[3], ps, s * 16 + 4 * kb, rq);
                if (live0) ldsA[s * soffA + slot0 * 4 + kb] = p;
            }
        }
    }
    __syncthreads();

    // ---- phase 2: dw1 (stride 1) over the clipped B rectangle, A -> LDS B ---------------------------------------------------------
    if (on1) {
        const Rq rq = *reinterpret_cast<const Rq*>(wl + a.off_rq + 1 * (int)sizeof(Rq));
        const unsigned* const src = ldsA + (cq1 >> 2) * soffA + (cq1 & 3);
        unsigned* const dst = ldsB + (cq1 >> 2) * soffC + (cq1 & 3);
        for (int q = t >> a.qsh1; q < CVP; q += nthreads >> a.qsh1) {
            const int vy = (int)(((float)q + 0.5f) * inv_cvw), vx = q - vy * CVW;
            const int ly = cvy0 + vy - cy0, lx = cvx0 + vx - cx0;        // B / C region coordinates; A's are the same + the tap
            const unsigned* row = src + (ly * RAW + lx) * 4;
            int acc[4] = {db1.x, db1.y, db1.z, db1.w};                   // the dot chain starts at the bias
            dw3x3_from_lds(row, RAW, w1, acc);
            dst[(ly * RCW + lx) * 4] = requant4<WIN>(acc[0], acc[1], acc[2], acc[3], ds1, c1, rq);
        }
    }
    __syncthreads();

    // ---- phase 3: pw2 over the same rectangle, B -> LDS C; items (pixel tile, slice) round-robin over the waves ------------------
    {
        const Rq rq = *reinterpret_cast<const Rq*>(wl + a.off_rq + 2 * (int)sizeof(Rq));
        const int ntilesC = (CVP + 15) >> 4;
        int tile = 0, s = wave;
        while (s >= ns2) { s -= ns2; tile++; }
        while (tile < ntilesC) {
            const int v = tile * 16 + l15, vc = min(v, CVP - 1);
            const int vy = (int)(((float)vc + 0.5f) * inv_cvw), vx = vc - vy * CVW;
            const int slot = (cvy0 + vy - cy0) * RCW + (cvx0 + vx - cx0);
            // K byte 16 * (kb + 4u) + j of the pixel = channel j of slice kb + 4u; slices past the last one meet zero weights
            const v4i bq0 = *reinterpret_cast<const v4i*>(ldsB + min(kb, ns1 - 1) * soffC + slot * 4);
            const int4 pb = *reinterpret_cast<const int4*>(wl + a.off_b2 + (s * 16 + 4 * kb) * 4);
            const float4 ps = *reinterpret_cast<const float4*>(wl + a.off_s2 + (s * 16 + 4 * kb) * 4);
            v4i acc = v4i{pb.x, pb.y, pb.z, pb.w};
            acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(*reinterpret_cast<const v4i*>(wl + a.off_wf2 + ((s * a.ks2) * 64 + lane) * 16), bq0, acc, 0, 0, 0);
            if (a.ks2 > 1) {
                const v4i bq1 = *reinterpret_cast<const v4i*>(ldsB + min(kb + 4, ns1 - 1) * soffC + slot * 4);
                acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(*reinterpret_cast<const v4i*>(wl + a.off_wf2 + ((s * a.ks2 + 1) * 64 + lane) * 16), bq1, acc, 0, 0, 0);
            }
            const unsigned p = requant4<WIN>(acc[0], acc[1], acc[2], acc[3], ps, s * 16 + 4 * kb, rq);
            if (v < CVP) ldsC[s * soffC + slot * 4 + kb] = p;
            s += nwaves;
            while (s >= ns2) { s -= ns2; tile++; }
        }
    }
    __syncthreads();

    // ---- phase 4: dw2 (stride S2) from C -> NHWC output ---------------------------------------------------------------------------
    if (on2) {
        const Rq rq = *reinterpret_cast<const Rq*>(wl + a.off_rq + 3 * (int)sizeof(Rq));
        const unsigned* const src = ldsC + (cq2 >> 2) * soffC + (cq2 & 3);
        const float inv_tw = __builtin_amdgcn_rcpf((float)tw);
        int8_t* yn = a.y + ((size_t)(n * a.OH + oy0) * a.OW + ox0) * a.ldc + a.c_off + c2;
        for (int q = t >> a.qsh2; q < th * tw; q += nthreads >> a.qsh2) {
            const int oyl = (int)(((float)q + 0.5f) * inv_tw), oxl = q - oyl * tw;
            const unsigned* row = src + ((oyl * S2) * RCW + oxl * S2) * 4;
            int acc[4] = {db2.x, db2.y, db2.z, db2.w};
            dw3x3_from_lds(row, RCW, w2, acc);
            const unsigned p = requant4<WIN>(acc[0], acc[1], acc[2], acc[3], ds2, c2, rq);
            if (c2 < a.c_limit) {
                unsigned* dstp = reinterpret_cast<unsigned*>(yn + ((size_t)oyl * a.OW + oxl) * a.ldc);
                // coherent instance: write-through (agent-scope) stores; S_ENDPGM waits for them (pwdw.hip: chain_signal)
                if (COH) __hip_atomic_store(dstp, p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); else *dstp = p;
            }
        }
    }
}

// plain instance: hipGraph replay.  (symbols must not match bench.py's pwdw_i8(_coh)?_kernel< family pattern)
template <int PROD, int WIN>
__global__ __launch_bounds__(512) void chain4_i8_kernel(Chain4Args a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned chain4_lds[];
    chain4_block<PROD, false, WIN>(a, chain4_lds);
}

// coherent instance: direct dispatch (pwdw.hip: pwdw_i8_coh_kernel) -- the PROD 0 input by sc1 buffer loads, results by write-through
// stores, so its packet needs no cache maintenance at its boundaries; the PROD 1 graph input is read with ordinary loads
template <int PROD, int WIN>
__global__ __launch_bounds__(512) void chain4_i8_coh_kernel(Chain4Args a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned chain4_lds[];
    chain4_block<PROD, true, WIN>(a, chain4_lds);
}

size_t chain4_lds_bytes(const Chain4Args& a)
{
    const size_t soffA = (size_t)((a.RCH + 2) * (a.RCW + 2) + 4) * 16, soffC = (size_t)(a.RCH * a.RCW + 4) * 16;
    return (size_t)a.blob_q * 16 + a.ns1 * soffA + (size_t)(a.ns2 + a.ns1) * soffC;
}

bool chain4_config_ok(const Chain4Args& a, int threads)
{
    if (threads != 256 && threads != 512) return false;
    if (a.TH < 1 || a.TW < 1 || a.ns1 < 1 || a.ns1 > 8 || a.ns2 < 1 || a.ns2 > 8 || a.ks0 < 1 || a.ks0 > 2 || a.ks2 < 1 || a.ks2 > 2) return false;
    if (a.prod == 1 && a.ks0 != 1) return false;
    if (a.blob_q > kChain4Stage * threads) return false;
    if ((1 << a.qsh1) < a.ns1 * 4 || (1 << a.qsh2) < a.ns2 * 4 || (1 << a.qsh1) > threads || (1 << a.qsh2) > threads) return false;
    if ((a.RCH + 2) * (a.RCW + 2) >= 16384) return false;              // (locate: pixel indices exact in float)
    return chain4_lds_bytes(a) <= 64 * 1024;
}

template <int PROD>
static hipError_t launch_chain4_p(const Chain4Args& a, int threads, hipStream_t s)
{
    const dim3 grid(a.tiles_x, a.tiles_y, a.N);
    const size_t lds = chain4_lds_bytes(a);
    const bool win = a.win != 0;          // all four windows in the one-binade form (epilogue.h: rq_win; the planner checked)
    if (a.coherent) {
        launch_rec_coherent();
        if (win) hipLaunchKernelGGL((chain4_i8_coh_kernel<PROD, 1>), grid, dim3(threads), lds, s, a);
        else hipLaunchKernelGGL((chain4_i8_coh_kernel<PROD, 0>), grid, dim3(threads), lds, s, a);
    } else {
        if (win) hipLaunchKernelGGL((chain4_i8_kernel<PROD, 1>), grid, dim3(threads), lds, s, a);
        else hipLaunchKernelGGL((chain4_i8_kernel<PROD, 0>), grid, dim3(threads), lds, s, a);
    }
    return hipGetLastError();
}

hipError_t launch_chain4(const Chain4Args& a, int threads, hipStream_t s)
{
    if (!chain4_config_ok(a, threads) || a.tiles_y > 65535 || a.N > 65535) return hipErrorInvalidValue;
    return a.prod == 1 ? launch_chain4_p<1>(a, threads, s) : launch_chain4_p<0>(a, threads, s);
}

}  // namespace tamd
