// The channel-moving operators of quantised graphs: Split (split_ref.c), ShuffleChannel (shuffle_channel_ref.c) and a channel Concat
// whose only reader is a ShuffleChannel.  In the reference they are memcpys -- no quantisation parameter is read, -128 stays -128 --
// except the uint8 Split, which requantises one byte to one byte.  Nothing is computed here either: which source channel an output
// channel takes, and the uint8 byte map, come from the host, built at prerun (chanmap_tables.cc, graph_plan_maps.hip), so every one of
// these nodes is the same kernel and its bytes are the reference's by construction.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "epilogue.h"       // fix128_4
#include "kernels.h"

namespace tamd {

// ---- int8, NHWC with a padded channel stride.  One lane per pixel and 16-byte OUTPUT vector: sixteen table entries (four 16-byte
// loads of a table that every pixel shares), sixteen byte loads from wherever the sources lie -- a whole tensor, a concat view, a
// Split view -- and one 16-byte store.  An entry of kChanMapZero is WRITTEN AS ZERO: the lanes behind channel C are the padding the
// next convolution's K loop reads (graph_plan.hip: plan_buffers).  The output is addressed by pixel stride ldc and channel offset
// c_off (a concat view).  fix128: the map runs THROUGH a Concat of several inputs, whose copy between equal scales is the identity
// on every byte but one -- concat_kernel_ref_int8.c clamps below -127 to PLUS 127 (:83-84), so -128 comes out as 127.
__global__ __launch_bounds__(256) void chan_map_i8_kernel(ChanMapI8Args a)
{
    const unsigned nv = (unsigned)(a.C + 15) / 16;
    const unsigned total = (unsigned)a.pixels * nv;                  // (fits: launch_chan_map_i8) -- the position in 32-bit divisions
    const unsigned idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    const unsigned v = idx % nv;
    const size_t pix = idx / nv;
    const uint4* te = reinterpret_cast<const uint4*>(a.table + v * 16);
    unsigned e[16];
#pragma unroll
    for (int q = 0; q < 4; q++) { const uint4 t = te[q]; e[4 * q] = t.x; e[4 * q + 1] = t.y; e[4 * q + 2] = t.z; e[4 * q + 3] = t.w; }
    unsigned p[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int k = 0; k < 16; k++) {
        const unsigned t = e[k];
        if (t == kChanMapZero) continue;
        const unsigned s = t >> 28, off = t & 0x0fffffffu;
        const int8_t* base = s == 0 ? a.src[0].x : s == 1 ? a.src[1].x : s == 2 ? a.src[2].x : a.src[3].x;
        const int cs = s == 0 ? a.src[0].cs : s == 1 ? a.src[1].cs : s == 2 ? a.src[2].cs : a.src[3].cs;
        unsigned b = (unsigned)(uint8_t)base[pix * (size_t)cs + off];
        if (a.fix128 && b == 0x80u) b = 0x7fu;
        p[k >> 2] |= b << (8 * (k & 3));
    }
    *reinterpret_cast<uint4*>(a.y + pix * (size_t)a.ldc + a.c_off + v * 16) = make_uint4(p[0], p[1], p[2], p[3]);
}

hipError_t launch_chan_map_i8(const ChanMapI8Args& a, hipStream_t s)
{
    if (a.nsrc < 1 || a.nsrc > kChanMapMaxSrc || a.pixels < 1 || a.C < 1 || !a.y || !a.table) return hipErrorInvalidValue;
    for (int i = 0; i < a.nsrc; i++)
        if (!a.src[i].x || a.src[i].cs < 1) return hipErrorInvalidValue;
    const int cv = (a.C + 15) / 16 * 16;                 // whole vectors: inside the output's slice
    if (a.ldc % 16 || a.c_off % 16 || a.c_off < 0 || a.c_off + cv > a.ldc) return hipErrorInvalidValue;
    if (((uintptr_t)a.y | (uintptr_t)a.table) & 15) return hipErrorInvalidValue;
    const long total = a.pixels * (cv / 16);
    if (total > 0x7fffff00L) return hipErrorInvalidValue;           // the kernel counts lanes in 32 bits
    hipLaunchKernelGGL(chan_map_i8_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, a);
    return hipGetLastError();
}

// ---- the one shape of the real network: group 2 over two sources of equal width (every ShuffleNet-v2 unit: Concat(x1, branch) ->
// ShuffleChannel(2)).  Output channel 2j is a[j], 2j + 1 is b[j], so output vector v is the byte interleave of a[8v .. 8v + 7] and
// b[8v .. 8v + 7]: two 8-byte loads, four byte permutes, one 16-byte store -- no table.  Bytes behind channel `half` are zero (the
// padding lanes).  Its results are chan_map_i8's (tests/test_gpu_shuffle.py runs both forms on the same graphs).
__global__ __launch_bounds__(256) void chan_map_i8_g2_kernel(ChanMapG2Args a)
{
    const unsigned nv = (unsigned)(2 * a.half + 15) / 16;
    const unsigned total = (unsigned)a.pixels * nv;                  // (fits: launch_chan_map_g2)
    const unsigned idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    const unsigned v = idx % nv;
    const size_t pix = idx / nv;
    uint2 xa = *reinterpret_cast<const uint2*>(a.a + pix * (size_t)a.cs_a + v * 8);
    uint2 xb = *reinterpret_cast<const uint2*>(a.b + pix * (size_t)a.cs_b + v * 8);
    const int valid = a.half - (int)v * 8;               // channels of either half in this vector (>= 8: all of them)
    if (valid < 8) {
        const unsigned lo = valid >= 4 ? 0xffffffffu : 0xffffffffu >> (8 * (4 - valid));
        const unsigned hi = valid <= 4 ? 0u : 0xffffffffu >> (8 * (8 - valid));
        xa.x &= lo; xb.x &= lo; xa.y &= hi; xb.y &= hi;
    }
    // v_perm_b32: selector bytes 0 .. 3 take the bytes of the SECOND operand, 4 .. 7 those of the first
    uint4 o;
    o.x = __builtin_amdgcn_perm(xb.x, xa.x, 0x05010400u);
    o.y = __builtin_amdgcn_perm(xb.x, xa.x, 0x07030602u);
    o.z = __builtin_amdgcn_perm(xb.y, xa.y, 0x05010400u);
    o.w = __builtin_amdgcn_perm(xb.y, xa.y, 0x07030602u);
    if (a.fix128) { o.x = fix128_4(o.x); o.y = fix128_4(o.y); o.z = fix128_4(o.z); o.w = fix128_4(o.w); }
    *reinterpret_cast<uint4*>(a.y + pix * (size_t)a.ldc + a.c_off + v * 16) = o;
}

hipError_t launch_chan_map_g2(const ChanMapG2Args& a, hipStream_t s)
{
    if (!a.a || !a.b || !a.y || a.pixels < 1 || a.half < 1) return hipErrorInvalidValue;
    const int cv = (2 * a.half + 15) / 16 * 16, rv = (a.half + 7) / 8 * 8;     // whole output vectors; whole 8-byte reads of either half
    if (a.ldc % 16 || a.c_off % 16 || a.c_off < 0 || a.c_off + cv > a.ldc || a.cs_a % 8 || a.cs_b % 8 || rv > a.cs_a || rv > a.cs_b) return hipErrorInvalidValue;
    if (((uintptr_t)a.y & 15) || (((uintptr_t)a.a | (uintptr_t)a.b) & 7)) return hipErrorInvalidValue;
    const long total = a.pixels * (cv / 16);
    if (total > 0x7fffff00L) return hipErrorInvalidValue;
    hipLaunchKernelGGL(chan_map_i8_g2_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, a);
    return hipGetLastError();
}

// ---- uint8, dense NCHW.  The C output planes of one image are ONE run of L = C * HW bytes (at channel out_c0 of an image of out_img
// bytes), and a plane of HW bytes may be odd-sized, so neither a plane nor the run starts aligned in general: the run is cut at the
// 16-byte boundaries OF ITS ADDRESS, as interp_nearest_u8 cuts its rows.  Thread t of an image owns the aligned 16 bytes number t counted
// from the boundary at or below the run's first byte; the bytes [lo, hi) of them belong to the run.  A whole chunk inside one plane takes
// its sixteen source bytes as they lie (one plane of the input, at any alignment) and is stored with one 16-byte store; a chunk that
// crosses planes, and the ragged head and tail chunks, step from byte to byte and touch nothing outside the run.  The byte map (a uint8
// Split between tensors of different quantisation parameters) is staged in LDS, 256 bytes; IDENT: no map, no LDS.
template <bool IDENT>
__global__ __launch_bounds__(64) void chan_map_u8_kernel(ChanMapU8Args a)
{
    __shared__ unsigned tab_s[64];
    if (!IDENT) {
        tab_s[threadIdx.x] = a.table[threadIdx.x];
        __syncthreads();
    }
    const uint8_t* tab = reinterpret_cast<const uint8_t*>(tab_s);
    const int n = blockIdx.y;
    const int L = a.C * a.HW;
    uint8_t* run = a.y + (size_t)n * a.out_img + (size_t)a.out_c0 * a.HW;
    const int mis = (int)((uintptr_t)run & 15);
    const long first = ((long)blockIdx.x * blockDim.x + threadIdx.x) * 16 - mis;       // run index of this chunk's byte 0
    const int lo = first < 0 ? (int)-first : 0;
    const int hi = first >= L ? 0 : (L - first >= 16 ? 16 : (int)(L - first));
    if (lo >= hi) return;                                // (behind the barrier)
    const uint8_t* xs = a.x + (size_t)n * a.in_img;
    const int j0 = (int)(first + lo);
    int ch = j0 / a.HW, r = j0 - ch * a.HW;
    const uint8_t* sp = xs + (size_t)a.src_plane[ch] * a.HW;
    unsigned p[4] = {0u, 0u, 0u, 0u};
    const bool whole = lo == 0 && hi == 16;
    if (whole && r + 16 <= a.HW) {
        __builtin_memcpy(p, sp + r, 16);
    } else {
#pragma unroll
        for (int j = 0; j < 16; j++)                     // (unrolled: registers indexed by constants, no scratch memory)
            if (j >= lo && j < hi) {
                p[j >> 2] |= (unsigned)sp[r] << (8 * (j & 3));
                if (++r == a.HW) {
                    r = 0;
                    if (++ch < a.C) sp = xs + (size_t)a.src_plane[ch] * a.HW;       // (behind the last plane: nothing more is read)
                }
            }
    }
    if (!IDENT) {
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const unsigned q = p[k];
            p[k] = (unsigned)tab[q & 0xffu] | (unsigned)tab[(q >> 8) & 0xffu] << 8 | (unsigned)tab[(q >> 16) & 0xffu] << 16 | (unsigned)tab[q >> 24] << 24;
        }
    }
    if (whole) {
        *reinterpret_cast<uint4*>(run + first) = make_uint4(p[0], p[1], p[2], p[3]);
    } else {
#pragma unroll
        for (int j = 0; j < 16; j++)
            if (j >= lo && j < hi) run[first + j] = (uint8_t)(p[j >> 2] >> (8 * (j & 3)));
    }
}

hipError_t launch_chan_map_u8(const ChanMapU8Args& a, hipStream_t s)
{
    if (a.N < 1 || a.N > 65535 || a.C < 1 || a.HW < 1 || !a.x || !a.y || !a.src_plane || (!a.identity && !a.table)) return hipErrorInvalidValue;
    const long L = (long)a.C * a.HW;
    if (L > 0x7fffffffL - 64 || a.in_planes < 1 || (long)a.in_planes * a.HW > (long)a.in_img || a.out_c0 < 0
        || (long)a.out_img < ((long)a.out_c0 + a.C) * a.HW)
        return hipErrorInvalidValue;
    const long chunks = (L + 15) / 16 + 1;               // + 1: a run that starts mid-chunk ends one chunk later
    const dim3 grid((unsigned)((chunks + 63) / 64), (unsigned)a.N);
    if (a.identity) hipLaunchKernelGGL(chan_map_u8_kernel<true>, grid, dim3(64), 0, s, a);
    else hipLaunchKernelGGL(chan_map_u8_kernel<false>, grid, dim3(64), 0, s, a);
    return hipGetLastError();
}

}  // namespace tamd
