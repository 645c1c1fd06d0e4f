// The channel gate of a Squeeze-and-Excitation block: Eltwise PROD | SUM | SUB of x (N, C, H, W) with a gate (N, C, 1, 1), int8 and uint8
// graphs (eltwise_ref.c: the branch input_chan == input1_count4 of ref_eltwise_int8 / ref_eltwise_uint8, out[i] = in0[i] op in1[i / input_hw];
// in0 is the operand with more elements whichever input it is, so it is always x op gate).  The arithmetic per value is that of the
// same-shape kernels -- eltwise_i8_kernel (misc_kernels.hip), eltwise_u8_k (u8_kernels.hip) -- with the second operand one value per
// plane, read and dequantised ONCE by the lane that walks the plane's bytes: the launch reads x and N * C gate bytes where the
// same-shape form reads two tensors.  The two kernels differ because the two layouts do, as in prelu.hip:
//  - int8 tensors are NHWC: a lane's 16 bytes are 16 channels of one pixel, so a lane keeps the 16 gate values of its channel group and
//    walks pixels of one image;
//  - uint8 tensors are dense NCHW: a plane has ONE gate byte, and a lane's 16 bytes lie in one plane or in two neighbouring ones.
// LUT: the gate bytes are the input of the byte-map node in front of the gate (Sigmoid, Clip, HardSwish, Mish) and are mapped through
// that node's 256-byte table first (tamd_lut_table: what lut_u8 would have stored), staged in LDS once per block -- the byte map and
// the gate are one launch, the same bytes by construction.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "epilogue.h"
#include "u8_epilogue.h"
#include "kernels.h"

namespace tamd {

__device__ __forceinline__ int gate_sxb(unsigned v, int b) { return (int)(signed char)((v >> (8 * b)) & 0xff); }

// the 256-byte table of a block: 64 dwords by the first wave, one barrier; every lane of the block arrives (nobody has left yet)
template <bool LUT>
__device__ __forceinline__ void gate_table_stage(unsigned* tab, const unsigned* table)
{
    if (LUT) {
        if (threadIdx.x < 64) tab[threadIdx.x] = table[threadIdx.x];
        __syncthreads();
    }
}
template <bool LUT>
__device__ __forceinline__ unsigned gate_byte(const unsigned* tab, unsigned b)
{
    return LUT ? (unsigned)reinterpret_cast<const uint8_t*>(tab)[b] : b;
}

// ---- int8, NHWC with a padded channel stride.  A block of 256 lanes is `ppi` pixels of `gpb` 16-channel groups (gpb = the groups of a
// pixel, at most 256; ppi = 256 / gpb whole pixels, the lanes behind them idle): one iteration of a block is one contiguous run of
// ppi * cs bytes, and a lane meets the SAME channel group in every iteration, `iters` of them, ppi pixels apart.  So it loads and
// dequantises its 16 gate values once (16 registers), then per pixel one 16-byte load, the chain of eltwise_i8_kernel on 16 values --
// fa = (float)q * sx, f = fa op g, round(f / out_scale) saturated to +-127 through round_div_sat (epilogue.h: exact) -- and one 16-byte
// store.  blockIdx.y is the image: the gate is indexed with n; blockIdx.z is the chunk of 256 groups of a pixel of more than 256
// (C > 4096).  The padding lanes [C, cs) are WRITTEN AS ZERO whatever x and the gate hold there: the next convolution's K loop reads
// them (graph_plan.hip: plan_buffers).  -128 is a legal byte of either operand and never comes out (sat127).
// iters is the launcher's: a pixel's 16 values are ~250 VALU instructions behind one load, so pixels walked in turn by one lane are
// latency in a row, and a tensor that does not fill the chip several times over is faster with one pixel per lane (measured:
// profiles/se_gate.txt); only from kChanGateBlocksPerIter blocks on does a lane take 2, then 4.
constexpr long kChanGateBlocksPerIter = 4096;

template <bool LUT>
__global__ __launch_bounds__(256) void chan_gate_i8_kernel(ChanGateI8Args a, int gpb, int ppi, int iters)
{
    __shared__ unsigned tab[64];
    gate_table_stage<LUT>(tab, a.table);
    const int nv = a.cs / 16;
    const int pl = (int)threadIdx.x / gpb;
    const int g = (int)blockIdx.z * 256 + ((int)threadIdx.x - pl * gpb);
    const int n = blockIdx.y;
    if (pl >= ppi || g >= nv) return;
    const uint4 gv = *reinterpret_cast<const uint4*>(a.gate + (size_t)n * a.cs + (size_t)g * 16);
    const unsigned gp[4] = {gv.x, gv.y, gv.z, gv.w};
    float gf[16];
#pragma unroll
    for (int k = 0; k < 16; k++) {
        const unsigned b = gate_byte<LUT>(tab, (gp[k >> 2] >> (8 * (k & 3))) & 0xffu);
        gf[k] = __fmul_rn((float)(int)(signed char)b, a.sg);
    }
    const float inv_out = __fdiv_rn(1.0f, a.out_scale);
    int p = (int)blockIdx.x * (iters * ppi) + pl;
    for (int it = 0; it < iters && p < a.HW; it++, p += ppi) {
        const size_t off = ((size_t)n * a.HW + p) * a.cs + (size_t)g * 16;
        const uint4 v = *reinterpret_cast<const uint4*>(a.x + off);
        const unsigned pv[4] = {v.x, v.y, v.z, v.w};
        unsigned out[4];
#pragma unroll
        for (int d = 0; d < 4; d++) {
            int q[4];
#pragma unroll
            for (int b = 0; b < 4; b++) {
                const float fa = __fmul_rn((float)gate_sxb(pv[d], b), a.sx), fb = gf[d * 4 + b];
                float f;
                switch (a.type) {
                case 0: f = __fmul_rn(fa, fb); break;
                case 2: f = __fadd_rn(fa, fb); break;
                default: f = __fsub_rn(fa, fb); break;
                }
                q[b] = g * 16 + d * 4 + b < a.C ? round_div_sat(f, a.out_scale, inv_out) : 0;
            }
            out[d] = pack4(q[0], q[1], q[2], q[3]);
        }
        *reinterpret_cast<uint4*>(a.y + off) = make_uint4(out[0], out[1], out[2], out[3]);
    }
}

hipError_t launch_chan_gate_i8(const ChanGateI8Args& a, hipStream_t s)
{
    if (!a.x || !a.gate || !a.y || a.cs < 16 || a.cs % 16 || a.C < 1 || a.C > a.cs || a.N < 1 || a.N > 65535 || a.HW < 1) return hipErrorInvalidValue;
    if (a.type != 0 && a.type != 2 && a.type != 4) return hipErrorInvalidValue;
    if (((uintptr_t)a.x | (uintptr_t)a.gate | (uintptr_t)a.y | (uintptr_t)a.table) & 15) return hipErrorInvalidValue;
    const int nv = a.cs / 16, gpb = nv < 256 ? nv : 256, ppi = 256 / gpb, gchunks = (nv + 255) / 256;
    if (gchunks > 65535) return hipErrorInvalidValue;
    const long blocks1 = ((long)a.HW + ppi - 1) / ppi * gchunks * a.N;                 // with one pixel per lane
    const int iters = a.iters > 0 ? (a.iters < 64 ? a.iters : 64) : blocks1 >= 4 * kChanGateBlocksPerIter ? 4 : blocks1 >= 2 * kChanGateBlocksPerIter ? 2 : 1;
    const long per_block = (long)iters * ppi;
    const long gx = ((long)a.HW + per_block - 1) / per_block;
    if (gx > 0x7fffffffL) return hipErrorInvalidValue;
    const dim3 grid((unsigned)gx, (unsigned)a.N, (unsigned)gchunks);
    if (a.table) hipLaunchKernelGGL(chan_gate_i8_kernel<true>, grid, dim3(256), 0, s, a, gpb, ppi, iters);
    else hipLaunchKernelGGL(chan_gate_i8_kernel<false>, grid, dim3(256), 0, s, a, gpb, ppi, iters);
    return hipGetLastError();
}

// ---- uint8, dense NCHW.  Plane p = n * C + c (HW bytes) has the one gate byte gate[p]; the planes lie back to back and start at any
// byte address (7 x 7 = 49 bytes).  The tensor is cut at the 16-byte boundaries of its ADDRESSES, as prelu_u8 and chan_map_u8 cut
// theirs, but a lane owns an aligned 16-byte chunk of the TENSOR, not of a plane: with HW >= 16 a chunk lies in one plane or in two
// neighbouring ones, so the lane reads the gate bytes of both (the second one where it exists), dequantises both, and picks per byte --
// bytes [0, split) of the chunk belong to plane p0, bytes [split, 16) to p0 + 1 -- with a select, not a branch.  Every chunk is ONE
// aligned 16-byte load and ONE 16-byte store, every lane of every wave has a chunk (a plane of 196 bytes does not cost a wave of
// which 13 lanes work), and no byte is written by two lanes.  x and y are both 16-byte aligned and laid out alike.  Only the LAST
// chunk of the tensor can be ragged (planes * HW % 16 bytes): it goes byte by byte and touches nothing past the tensor's last byte.
// Per value the chain of eltwise_u8_k: fa = (float)(u - zx) * sx, fb = (float)(gate - zg) * sg, r = fa op fb, quant_round_sat_u8
// (u8_epilogue.h: round(r / out_scale) + out_zp saturated to 0 .. 255, exact).
template <bool LUT>
__global__ __launch_bounds__(256) void chan_gate_u8_kernel(ChanGateU8Args a)
{
    __shared__ unsigned tab[64];
    gate_table_stage<LUT>(tab, a.table);
    const size_t total = (size_t)a.planes * a.HW;
    const size_t first = ((size_t)blockIdx.x * 256 + threadIdx.x) * 16;          // tensor index of this chunk's byte 0
    if (first >= total) return;
    const int hi = total - first >= 16 ? 16 : (int)(total - first);
    const long p0 = (long)(first / (size_t)a.HW);
    const int split = a.HW - (int)(first - (size_t)p0 * a.HW);                    // >= 1; >= 16: the chunk lies in plane p0 alone
    const long p1 = p0 + 1 < a.planes ? p0 + 1 : p0;                              // (never read past the gate's last byte)
    const float fb0 = (float)((int)gate_byte<LUT>(tab, a.gate[p0]) - a.zg) * a.sg;
    const float fb1 = (float)((int)gate_byte<LUT>(tab, a.gate[p1]) - a.zg) * a.sg;
    unsigned pv[4] = {0u, 0u, 0u, 0u};
    if (hi == 16) {
        const uint4 v = *reinterpret_cast<const uint4*>(a.x + first);
        pv[0] = v.x; pv[1] = v.y; pv[2] = v.z; pv[3] = v.w;
    } else {
#pragma unroll
        for (int j = 0; j < 16; j++)                     // (unrolled: registers indexed by constants, no scratch memory)
            if (j < hi) pv[j >> 2] |= (unsigned)a.x[first + j] << (8 * (j & 3));
    }
    unsigned out[4];
#pragma unroll
    for (int d = 0; d < 4; d++) {
        unsigned o = 0;
#pragma unroll
        for (int b = 0; b < 4; b++) {
            const float fa = (float)((int)((pv[d] >> (8 * b)) & 0xffu) - a.zx) * a.sx;
            const float fb = d * 4 + b < split ? fb0 : fb1;
            float r;
            switch (a.type) {
            case 0: r = fa * fb; break;
            case 2: r = fa + fb; break;
            default: r = fa - fb; break;
            }
            o |= (unsigned)quant_round_sat_u8(r, a.out_scale, a.out_zp) << (8 * b);
        }
        out[d] = o;
    }
    if (hi == 16) {
        *reinterpret_cast<uint4*>(a.y + first) = make_uint4(out[0], out[1], out[2], out[3]);
    } else {
#pragma unroll
        for (int j = 0; j < 16; j++)
            if (j < hi) a.y[first + j] = (uint8_t)(out[j >> 2] >> (8 * (j & 3)));
    }
}

// planes of fewer than 16 bytes (a chunk would span three of them or more): a byte per lane, its plane by division
template <bool LUT>
__global__ __launch_bounds__(256) void chan_gate_u8_small_kernel(ChanGateU8Args a)
{
    __shared__ unsigned tab[64];
    gate_table_stage<LUT>(tab, a.table);
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)a.planes * a.HW) return;
    const float fa = (float)((int)a.x[i] - a.zx) * a.sx;
    const float fb = (float)((int)gate_byte<LUT>(tab, a.gate[i / (size_t)a.HW]) - a.zg) * a.sg;
    float r;
    switch (a.type) {
    case 0: r = fa * fb; break;
    case 2: r = fa + fb; break;
    default: r = fa - fb; break;
    }
    a.y[i] = quant_round_sat_u8(r, a.out_scale, a.out_zp);
}

hipError_t launch_chan_gate_u8(const ChanGateU8Args& a, hipStream_t s)
{
    if (!a.x || !a.gate || !a.y || a.HW < 1 || a.planes < 1 || a.planes > 0x7fffffffL) return hipErrorInvalidValue;
    if (a.type != 0 && a.type != 2 && a.type != 4) return hipErrorInvalidValue;
    if (((uintptr_t)a.x | (uintptr_t)a.y | (uintptr_t)a.table) & 15) return hipErrorInvalidValue;
    const size_t total = (size_t)a.planes * a.HW;
    const size_t lanes = a.HW >= 16 ? (total + 15) / 16 : total;
    const size_t blocks = (lanes + 255) / 256;
    if (blocks > 0x7fffffffUL) return hipErrorInvalidValue;
    const dim3 grid((unsigned)blocks);
    if (a.HW >= 16) {
        if (a.table) hipLaunchKernelGGL(chan_gate_u8_kernel<true>, grid, dim3(256), 0, s, a);
        else hipLaunchKernelGGL(chan_gate_u8_kernel<false>, grid, dim3(256), 0, s, a);
    } else {
        if (a.table) hipLaunchKernelGGL(chan_gate_u8_small_kernel<true>, grid, dim3(256), 0, s, a);
        else hipLaunchKernelGGL(chan_gate_u8_small_kernel<false>, grid, dim3(256), 0, s, a);
    }
    return hipGetLastError();
}

}  // namespace tamd
