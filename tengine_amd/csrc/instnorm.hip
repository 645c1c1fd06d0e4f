// uint8 InstanceNorm (instancenorm_ref.c:101-183), dense NCHW: per plane p = n * C + c the reference dequantises, sums the plane and the
// squared deviations from the mean in two strictly SEQUENTIAL fp32 chains, derives a = gamma / sqrt(var + eps) and b = fma(-mean, a, beta)
// and requantises fma(v, a, b).  The order of the two chains shows in the bytes, and this project's bar in uint8 is byte equality, so a
// chain cannot be split: the parallelism is across planes, and inside a plane between the chain and everything that is not the chain.
// What the built reference computes, operation by operation, is restated on the host in instnorm_tables.cc (tamd_instancenorm_plane) from
// its object code -- which products are rounded, which are fused, where double is kept; the kernels here perform the same operations and
// tests/test_gpu_instnorm.py holds them to the reference's bytes.
//
// A WAVE PER PLANE (one wave per block, so the waves spread over as many SIMDs as there are planes):
//  - all 64 lanes load a tile of the plane, 16 bytes each.  A plane starts at any byte address (H * W % 16 != 0), so it is cut at the
//    16-byte boundaries OF ITS ADDRESS as prelu_u8 / slice_u8 cut theirs: chunk t is the aligned 16 bytes number t counted from the
//    boundary at or below the plane's first byte, and bytes [lo, hi) of it belong to the plane.  A whole chunk is one 16-byte load;
//    the ragged head and tail go byte by byte; nothing outside the plane is read
//  - they dequantise ((float)u - (float)zp, then * scale: two rounded operations) and stage the floats in LDS in plane order.  In the
//    second pass they also subtract the mean and -- for the elements whose product the reference ROUNDS (all but the last H * W % 4)
//    -- square: the rounded product is not part of the chain, only its addition is
//  - lane 0 walks the staged tile in order: eight ds_read_b128, then 32 dependent v_add_f32 (instnorm_walk), and for the last H * W % 4 elements of the
//    second pass v_fma_f32(t, t, sqsum), as the reference's scalar remainder loop does
//  - the wave then computes mean, var (fp32 divisions), a in double (sqrt and quotient, one rounding to float) and b, and the 256-entry
//    byte map, four entries per lane: fma(v(u), a, b), roundf(y / out_scale + out_zp) by quant_round_in_exact, whose conversion
//    saturates (and makes 0 of a NaN) whatever instancenorm_refusal's bound let through.  A ReLU node behind is composed into the map
//    by fused_relu, the device function the convolution epilogues use
// The dword of a lane IS the lane's row of prelu_u8's / chan_lut_u8's [64]-dword table.  instnorm_stats_u8 stores it (form 0: one
// chan_lut_u8 launch with C := N * C applies the maps with the whole device; the default above 4096 bytes a plane); instnorm_u8 keeps it and
// maps its own plane through ds_bpermute_b32 exactly as prelu_u8 does (form 1: one launch, the apply step on one wave per plane; the default
// up to 4096 bytes a plane, where it measured ahead: graph_plan_maps.hip).
// Every arithmetic operation is an explicit _rn intrinsic: nothing is fused that the restatement does not fuse (the file is built with
// contraction off as well).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"
#include "u8_epilogue.h"

namespace tamd {

static constexpr int kInTile = 1024;       // floats of a staged tile: 64 lanes x 16 bytes

// chunk t = k * 64 + lane of the plane at xp (mis = its address & 15): first = the plane index of the chunk's byte 0; bytes [lo, hi) of
// the chunk belong to the plane.  pv: the chunk's bytes (zero outside [lo, hi))
__device__ __forceinline__ void instnorm_load_chunk(const uint8_t* xp, long first, int HW, unsigned (&pv)[4], int* lo_, int* hi_)
{
    const int lo = first < 0 ? (int)-first : 0;
    const int hi = first >= HW ? 0 : (HW - first >= 16 ? 16 : (int)(HW - first));
    pv[0] = pv[1] = pv[2] = pv[3] = 0u;
    if (lo == 0 && hi == 16) {
        const uint4 v = *reinterpret_cast<const uint4*>(xp + first);
        pv[0] = v.x; pv[1] = v.y; pv[2] = v.z; pv[3] = v.w;
    } else if (lo < hi) {
#pragma unroll
        for (int j = 0; j < 16; j++)                     // (unrolled: registers indexed by constants, no scratch memory)
            if (j >= lo && j < hi) pv[j >> 2] |= (unsigned)xp[first + j] << (8 * (j & 3));
    }
    *lo_ = lo; *hi_ = hi;
}

// stage tile k: lds[16 * lane + j] = the value of plane element first + j.  SECOND: t = v - mean, squared (rounded) below `body`
template <bool SECOND>
__device__ __forceinline__ void instnorm_stage(float* lds, const uint8_t* xp, int HW, int mis, int k, int lane, float zp, float scale, float mean, int body)
{
    const long first = ((long)k * 64 + lane) * 16 - mis;
    unsigned pv[4];
    int lo, hi;
    instnorm_load_chunk(xp, first, HW, pv, &lo, &hi);
    float f[16];
#pragma unroll
    for (int j = 0; j < 16; j++) {
        const unsigned u = (pv[j >> 2] >> (8 * (j & 3))) & 0xffu;
        float v = __fmul_rn(__fsub_rn((float)u, zp), scale);
        if (SECOND) {
            const float t = __fsub_rn(v, mean);
            v = first + j < (long)body ? __fmul_rn(t, t) : t;
        }
        f[j] = v;
    }
    float* dst = lds + 16 * lane;
    if (lo == 0 && hi == 16) {
#pragma unroll
        for (int d = 0; d < 4; d++) *reinterpret_cast<float4*>(dst + 4 * d) = make_float4(f[4 * d], f[4 * d + 1], f[4 * d + 2], f[4 * d + 3]);
    } else if (lo < hi) {
#pragma unroll
        for (int j = 0; j < 16; j++)
            if (j >= lo && j < hi) dst[j] = f[j];
    }
}

// acc + lds[i0] + lds[i0 + 1] + ... + lds[i1 - 1], strictly in that order.  The adds are one dependent chain; the LDS reads are not part
// of it.  With one ds_read_b128 in front of every four adds the walk measured 12.4 ns (about 30 cycles) per element and pass; this form,
// which issues EIGHT reads (32 floats) and then adds, measures 4.6 - 4.7 ns, about 11 cycles (profiles/instnorm.txt, both runs).  The
// compiler waits for the reads one by one (s_waitcnt lgkmcnt(7) .. (0)), so the first read's latency still stands in front of every 32
// adds; how much of the 11 cycles that is was not measured.  (A loop written to read the next batch before adding the current one is
// folded back into this form by the compiler, and volatile reads become flat loads: neither is kept.)
__device__ __forceinline__ float instnorm_walk(const float* lds, int i0, int i1, float acc)
{
    int i = i0;
    for (; i < i1 && (i & 3); i++) acc = __fadd_rn(acc, lds[i]);
    for (; i + 32 <= i1; i += 32) {
        float4 v[8];
#pragma unroll
        for (int d = 0; d < 8; d++) v[d] = *reinterpret_cast<const float4*>(lds + i + 4 * d);
#pragma unroll
        for (int d = 0; d < 8; d++) {
            acc = __fadd_rn(acc, v[d].x); acc = __fadd_rn(acc, v[d].y); acc = __fadd_rn(acc, v[d].z); acc = __fadd_rn(acc, v[d].w);
        }
    }
    for (; i + 4 <= i1; i += 4) {
        const float4 v = *reinterpret_cast<const float4*>(lds + i);
        acc = __fadd_rn(acc, v.x); acc = __fadd_rn(acc, v.y); acc = __fadd_rn(acc, v.z); acc = __fadd_rn(acc, v.w);
    }
    for (; i < i1; i++) acc = __fadd_rn(acc, lds[i]);
    return acc;
}

// the plane's byte map: the dword of this lane holds entries 4 * lane .. 4 * lane + 3
__device__ __forceinline__ unsigned instnorm_plane_map(const InstNormU8Args& a, float* lds, const uint8_t* xp, int mis, int c, int lane)
{
    const int HW = a.HW;
    const float zp = (float)a.in.zp, scale = a.in.scale, size = (float)HW;
    const int tiles = (int)(((long)HW + mis + kInTile - 1) / kInTile);
    const int body = HW - HW % 4;
    float sum = 0.f, sq = 0.f;
    for (int k = 0; k < tiles; k++) {
        instnorm_stage<false>(lds, xp, HW, mis, k, lane, zp, scale, 0.f, 0);
        __syncthreads();
        if (lane == 0) {
            const long base = (long)k * kInTile - mis;                   // the plane index of lds[0]
            const int w0 = k == 0 ? mis : 0, w1 = HW - base >= kInTile ? kInTile : (int)(HW - base);
            sum = instnorm_walk(lds, w0, w1, sum);
        }
        __syncthreads();
    }
    sum = __shfl(sum, 0);
    const float mean = __fdiv_rn(sum, size);
    for (int k = 0; k < tiles; k++) {
        instnorm_stage<true>(lds, xp, HW, mis, k, lane, zp, scale, mean, body);
        __syncthreads();
        if (lane == 0) {
            const long base = (long)k * kInTile - mis;
            const int w0 = k == 0 ? mis : 0, w1 = HW - base >= kInTile ? kInTile : (int)(HW - base);
            long wbl = (long)body - base;                                // where the fused remainder begins in this tile
            const int wb = wbl < w0 ? w0 : (wbl > w1 ? w1 : (int)wbl);
            sq = instnorm_walk(lds, w0, wb, sq);
            for (int i = wb; i < w1; i++) sq = __fmaf_rn(lds[i], lds[i], sq);
        }
        __syncthreads();
    }
    sq = __shfl(sq, 0);
    const float var = __fdiv_rn(sq, size);
    const float ve = __fadd_rn(var, a.eps);
    const float ca = __double2float_rn(__ddiv_rn((double)a.gamma[c], __dsqrt_rn((double)ve)));
    const float cb = __fmaf_rn(-mean, ca, a.beta[c]);
    unsigned tab = 0;
#pragma unroll
    for (int e = 0; e < 4; e++) {
        const float v = __fmul_rn(__fsub_rn((float)(4 * lane + e), zp), scale);
        uint8_t q = quant_round_in_exact(__fmaf_rn(v, ca, cb), a.out);
        if (a.relu.on) q = fused_relu(q, a.out.scale, a.out.zp, a.relu);
        tab |= (unsigned)q << (8 * e);
    }
    return tab;
}

__global__ __launch_bounds__(64) void instnorm_stats_u8_kernel(InstNormU8Args a)
{
    __shared__ __attribute__((aligned(16))) float lds[kInTile];
    const long plane = blockIdx.x;
    const uint8_t* xp = a.x + (size_t)plane * a.HW;
    const unsigned tab = instnorm_plane_map(a, lds, xp, (int)((uintptr_t)xp & 15), (int)(plane % a.C), (int)threadIdx.x);
    a.tables[(size_t)plane * 64 + threadIdx.x] = tab;
}

// the map applied to the wave's own plane: prelu_u8's loop.  The bpermute takes its data from every lane, so ALL 64 lanes stay active up
// to the stores and the lookups stand outside every branch
__global__ __launch_bounds__(64) void instnorm_u8_kernel(InstNormU8Args a)
{
    __shared__ __attribute__((aligned(16))) float lds[kInTile];
    const long plane = blockIdx.x;
    const int lane = (int)threadIdx.x;
    const uint8_t* xp = a.x + (size_t)plane * a.HW;
    uint8_t* yp = a.y + (size_t)plane * a.HW;
    const int mis = (int)((uintptr_t)xp & 15);                           // (== that of yp: both tensors are aligned and laid out alike)
    const unsigned tab = instnorm_plane_map(a, lds, xp, mis, (int)(plane % a.C), lane);
    const int tiles = (int)(((long)a.HW + mis + kInTile - 1) / kInTile);
    for (int k = 0; k < tiles; k++) {
        const long first = ((long)k * 64 + lane) * 16 - mis;
        unsigned pv[4];
        int lo, hi;
        instnorm_load_chunk(xp, first, a.HW, pv, &lo, &hi);
        unsigned out[4];
#pragma unroll
        for (int d = 0; d < 4; d++) {
            unsigned o = 0;
#pragma unroll
            for (int b = 0; b < 4; b++) {
                const unsigned q = (pv[d] >> (8 * b)) & 0xffu;
                const unsigned t = (unsigned)__builtin_amdgcn_ds_bpermute((int)(q & 0xfcu), (int)tab);      // byte address of lane q >> 2
                o |= ((t >> (8 * (q & 3u))) & 0xffu) << (8 * b);
            }
            out[d] = o;
        }
        if (lo == 0 && hi == 16) {
            *reinterpret_cast<uint4*>(yp + first) = make_uint4(out[0], out[1], out[2], out[3]);
        } else if (lo < hi) {
#pragma unroll
            for (int j = 0; j < 16; j++)
                if (j >= lo && j < hi) yp[first + j] = (uint8_t)(out[j >> 2] >> (8 * (j & 3)));
        }
    }
}

static bool instnorm_args_ok(const InstNormU8Args& a)
{
    if (!a.x || !a.gamma || !a.beta || a.C < 1 || a.HW < 1 || a.HW > 0x7fffffff - 64 || a.planes < 1 || a.planes % a.C || a.planes > 0x7fffffffL) return false;
    return (((uintptr_t)a.x) & 15) == 0;
}

hipError_t launch_instnorm_stats_u8(const InstNormU8Args& a, hipStream_t s)
{
    if (!instnorm_args_ok(a) || !a.tables || ((uintptr_t)a.tables & 15)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(instnorm_stats_u8_kernel, dim3((unsigned)a.planes), dim3(64), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_instnorm_u8(const InstNormU8Args& a, hipStream_t s)
{
    if (!instnorm_args_ok(a) || !a.y || ((uintptr_t)a.y & 15)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(instnorm_u8_kernel, dim3((unsigned)a.planes), dim3(64), 0, s, a);
    return hipGetLastError();
}

}  // namespace tamd
