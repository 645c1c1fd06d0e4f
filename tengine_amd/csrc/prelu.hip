// PReLU of quantised graphs (prelu_ref.c: ref_prelu_int8, ref_prelu_uint8).  What the reference computes for one byte of one channel
// is stated once, on the host: tamd_prelu_slope widens the fp16 slopes the way the reference does (not IEEE), tamd_prelu_table gives
// the output byte of every input byte (prelu_tables.cc).  The two kernels differ because the two layouts do:
//  - uint8 tensors are dense NCHW: a plane has ONE slope, so it is a byte map, and the kernel looks bytes up in its channel's table;
//  - int8 tensors are NHWC: the 16 bytes of a lane are 16 channels, a per-wave table does not fit, and the kernel computes the chain
//    relu_i8 computes (misc_kernels.hip), with a slope per channel.  It is correct when it equals tamd_prelu_table on every byte of
//    every channel: tests/test_gpu_prelu.py asks exactly that.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "epilogue.h"
#include "kernels.h"

namespace tamd {

__device__ __forceinline__ int prelu_sxb(unsigned v, int b) { return (int)(signed char)((v >> (8 * b)) & 0xff); }

// ---- int8, NHWC with a padded channel stride.  One lane per 16 bytes of one pixel, i.e. 16 neighbouring channels: one 16-byte load,
// the 16 slopes of those channels as four 16-byte loads of an fp32 array every pixel shares (the host widened and zero-padded it to cs),
// one 16-byte store.  Per value the reference's operations in its order: f = (float)q * in_scale; f < 0: f = slope[c] * f (the other
// addend of MAX(x, 0) + slope * MIN(x, 0) is a zero, so the sum rounds nothing: prelu_tables.cc); round(f / out_scale) saturated to
// +-127 through round_div_sat (epilogue.h: exact, the division itself only where the fast form cannot decide).  The padding lanes
// [C, cs) are WRITTEN AS ZERO whatever they held: the next convolution's K loop reads them (graph_plan.hip: plan_buffers).
__global__ __launch_bounds__(256) void prelu_i8_kernel(PreluI8Args a)
{
    const unsigned nv = (unsigned)a.cs / 16;
    const unsigned idx = blockIdx.x * blockDim.x + threadIdx.x;          // (fits 32 bits: launch_prelu_i8)
    const size_t i = (size_t)idx * 16;
    if (i >= a.count) return;
    const int c0 = (int)(idx % nv) * 16;
    const uint4 v = *reinterpret_cast<const uint4*>(a.x + i);
    const unsigned pv[4] = {v.x, v.y, v.z, v.w};
    const float4* sp = reinterpret_cast<const float4*>(a.slope + c0);
    const float inv_out = __fdiv_rn(1.0f, a.out_scale);
    unsigned out[4];
#pragma unroll
    for (int d = 0; d < 4; d++) {
        const float4 s4 = sp[d];
        const float sl[4] = {s4.x, s4.y, s4.z, s4.w};
        int q[4];
#pragma unroll
        for (int b = 0; b < 4; b++) {
            float f = __fmul_rn((float)prelu_sxb(pv[d], b), a.in_scale);
            if (f < 0.f) f = __fmul_rn(f, sl[b]);
            q[b] = c0 + d * 4 + b < a.C ? round_div_sat(f, a.out_scale, inv_out) : 0;
        }
        out[d] = pack4(q[0], q[1], q[2], q[3]);
    }
    *reinterpret_cast<uint4*>(a.y + i) = make_uint4(out[0], out[1], out[2], out[3]);
}

hipError_t launch_prelu_i8(const PreluI8Args& a, hipStream_t s)
{
    if (!a.x || !a.y || !a.slope || a.cs < 16 || a.cs % 16 || a.C < 1 || a.C > a.cs || a.count % (size_t)a.cs) return hipErrorInvalidValue;
    if (((uintptr_t)a.x | (uintptr_t)a.y | (uintptr_t)a.slope) & 15) return hipErrorInvalidValue;
    const size_t n16 = a.count / 16;
    if (n16 == 0) return hipSuccess;
    if (n16 > 0x7fffff00u) return hipErrorInvalidValue;                  // the kernel counts lanes in 32 bits
    hipLaunchKernelGGL(prelu_i8_kernel, dim3((unsigned)((n16 + 255) / 256)), dim3(256), 0, s, a);
    return hipGetLastError();
}

// ---- uint8, dense NCHW.  Plane p = n * C + c (HW bytes) has one slope, hence one 256-byte table: tables[c] (tables[0] when the slope
// is shared).  One wave per block, every block inside ONE plane, so the wave stages its plane's table the way lut_u8 does
// (misc_kernels.hip, where the argument about where a byte table lives is made): 64 dwords, one per lane, one coalesced 256-byte load;
// a lookup is a ds_bpermute_b32 of that register from lane b >> 2 and a shift by b & 3.  No LDS array, no barrier.  The bpermute takes
// its data from every lane, so ALL 64 lanes stay active up to the stores: a lane with nothing to do loads nothing, looks up zeros and
// stores nothing -- nobody leaves early, and the lookups stand outside every branch.
// A plane of HW bytes (7 x 7 = 49) starts at any byte address.  It is cut at the 16-byte boundaries OF ITS ADDRESS, as chan_map_u8 and
// interp_nearest_u8 cut theirs: lane t of the plane owns the aligned 16 bytes number t counted from the boundary at or below the
// plane's first byte, and the bytes [lo, hi) of them belong to the plane.  x and y are both 16-byte aligned and laid out alike, so the
// input chunk is aligned where the output chunk is: a whole chunk is one 16-byte load and one 16-byte store; the ragged head and tail
// chunks go byte by byte and touch nothing outside [lo, hi) -- the neighbouring planes' lanes write the other bytes of those 16, and
// nothing before the tensor's first byte or past its last one is read or written.
__global__ __launch_bounds__(64) void prelu_u8_kernel(PreluU8Args a)
{
    const long plane = blockIdx.x;
    const int c = a.shared ? 0 : (int)(plane % a.C);
    const unsigned tab = a.tables[(size_t)c * 64 + threadIdx.x];
    const uint8_t* xp = a.x + (size_t)plane * a.HW;
    uint8_t* yp = a.y + (size_t)plane * a.HW;
    const int mis = (int)((uintptr_t)yp & 15);
    const long first = ((long)blockIdx.y * 64 + threadIdx.x) * 16 - mis;        // plane index of this chunk's byte 0
    const int lo = first < 0 ? (int)-first : 0;
    const int hi = first >= a.HW ? 0 : (a.HW - first >= 16 ? 16 : (int)(a.HW - first));
    const bool any = lo < hi, whole = lo == 0 && hi == 16;
    unsigned pv[4] = {0u, 0u, 0u, 0u};
    if (whole) {
        const uint4 v = *reinterpret_cast<const uint4*>(xp + first);
        pv[0] = v.x; pv[1] = v.y; pv[2] = v.z; pv[3] = v.w;
    } else if (any) {
#pragma unroll
        for (int j = 0; j < 16; j++)                     // (unrolled: registers indexed by constants, no scratch memory)
            if (j >= lo && j < hi) pv[j >> 2] |= (unsigned)xp[first + j] << (8 * (j & 3));
    }
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
    if (whole) {
        *reinterpret_cast<uint4*>(yp + first) = make_uint4(out[0], out[1], out[2], out[3]);
    } else if (any) {
#pragma unroll
        for (int j = 0; j < 16; j++)
            if (j >= lo && j < hi) yp[first + j] = (uint8_t)(out[j >> 2] >> (8 * (j & 3)));
    }
}

hipError_t launch_prelu_u8(const PreluU8Args& a, hipStream_t s)
{
    if (!a.x || !a.y || !a.tables || a.C < 1 || a.HW < 1 || a.planes < 1 || a.planes % a.C || a.planes > 0x7fffffffL) return hipErrorInvalidValue;
    if (((uintptr_t)a.x | (uintptr_t)a.y | (uintptr_t)a.tables) & 15) return hipErrorInvalidValue;
    const long chunks = ((long)a.HW + 15) / 16 + 1;      // + 1: a plane that starts mid-chunk ends one chunk later
    const long by = (chunks + 63) / 64;
    if (by > 65535) return hipErrorInvalidValue;
    hipLaunchKernelGGL(prelu_u8_kernel, dim3((unsigned)a.planes, (unsigned)by), dim3(64), 0, s, a);
    return hipGetLastError();
}

}  // namespace tamd
