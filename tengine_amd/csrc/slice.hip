// Slice of a uint8 graph (slice_ref.c: the onnx form on a 4-D tensor): YOLOv4-tiny's "second half of the channels" routes and the
// x[..., ::2, ::2] picks of YOLOv5's Focus.  The reference dequantises the input, copies floats and requantises the output, so a byte
// of the output is a function of one byte of the input: the map comes from the host (slice_tables.cc, built at prerun), and this
// kernel only moves bytes out of a strided box of x.  Two Slices in a row are one box and one composed map (graph_plan_maps.hip).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"

namespace tamd {

// Dense NCHW.  The C * H * W output bytes of one image are ONE run (at channel out_c0 of an image of out_img bytes) whose address is
// in general not aligned, so the run is cut at the 16-byte boundaries OF ITS ADDRESS, as chan_map_u8 and interp_nearest_u8 cut theirs:
// thread t of an image owns the aligned 16 bytes number t counted from the boundary at or below the run's first byte, and the bytes
// [lo, hi) of them belong to the run.  It decomposes its first byte into (c, h, w) once.  A whole chunk takes one of three paths:
//  (a) its sixteen source bytes lie side by side (a.contig says how far they do: inside a row, a plane or the whole image): one
//      16-byte load at any alignment;
//  (b) W step 2 inside one output row: the sixteen bytes are every other one of 31 source bytes -- two 16-byte loads, at the first
//      byte and at the sixteenth (the second ends ON the last byte needed: nothing behind it is read), and four byte permutes;
//  (c) anything else -- other steps, a chunk that crosses rows or planes: byte by byte, walking (w, h) as the reference's loops do.
// The ragged head and tail chunks take (c) for their bytes [lo, hi) and store byte by byte: nothing outside the run is touched.  The
// byte map is staged in LDS, 256 bytes; IDENT: no map, no LDS.
template <bool IDENT>
__global__ __launch_bounds__(64) void slice_u8(SliceU8Args a)
{
    __shared__ unsigned tab_s[64];
    if (!IDENT) {
        tab_s[threadIdx.x] = a.table[threadIdx.x];
        __syncthreads();
    }
    const uint8_t* tab = reinterpret_cast<const uint8_t*>(tab_s);
    const int n = blockIdx.y;
    const int IH = a.in_dims[2], IW = a.in_dims[3], OH = a.out_dims[2], OW = a.out_dims[3];
    const int OHW = OH * OW, L = a.out_dims[1] * OHW;
    uint8_t* run = a.y + (size_t)n * a.out_img + (size_t)a.out_c0 * OHW;
    const int mis = (int)((uintptr_t)run & 15);
    const long first = ((long)blockIdx.x * blockDim.x + threadIdx.x) * 16 - mis;       // run index of this chunk's byte 0
    const int lo = first < 0 ? (int)-first : 0;
    const int hi = first >= L ? 0 : (L - first >= 16 ? 16 : (int)(L - first));
    if (lo >= hi) return;                                // (behind the barrier)
    const uint8_t* xs = a.x + (size_t)(a.start[0] + n * a.step[0]) * ((size_t)a.in_dims[1] * IH * IW);
    const int j0 = (int)(first + lo);
    const int c = j0 / OHW, rem = j0 - c * OHW;
    int h = rem / OW, w = rem - h * OW;
    const int sw = a.step[3], row = a.step[2] * IW, plane = a.step[1] * IH * IW;       // source bytes per step in w, h, c
    int src = (a.start[1] * IH + a.start[2]) * IW + a.start[3] + c * plane + h * row + w * sw;
    const bool whole = lo == 0 && hi == 16;
    const int left = a.contig == 3 ? L - j0 : a.contig == 2 ? OHW - rem : a.contig == 1 ? OW - w : 0;      // .. bytes that lie side by side from here
    unsigned p[4] = {0u, 0u, 0u, 0u};
    if (whole && left >= 16) {
        __builtin_memcpy(p, xs + src, 16);
    } else if (whole && a.w2 && OW - w >= 16) {
        unsigned e[4], o[4];
        __builtin_memcpy(e, xs + src, 16);               // source bytes 0 .. 15: the even ones are output bytes 0 .. 7
        __builtin_memcpy(o, xs + src + 15, 16);          // source bytes 15 .. 30: the odd ones of THESE are source 16, 18 .. 30
        p[0] = __builtin_amdgcn_perm(e[1], e[0], 0x06040200u);
        p[1] = __builtin_amdgcn_perm(e[3], e[2], 0x06040200u);
        p[2] = __builtin_amdgcn_perm(o[1], o[0], 0x07050301u);
        p[3] = __builtin_amdgcn_perm(o[3], o[2], 0x07050301u);
    } else {
#pragma unroll
        for (int j = 0; j < 16; j++)                     // (unrolled: registers indexed by constants, no scratch memory)
            if (j >= lo && j < hi) {
                p[j >> 2] |= (unsigned)xs[src] << (8 * (j & 3));
                src += sw;
                if (++w == OW) {                         // (behind the run's last byte src is not read any more)
                    w = 0;
                    src += row - OW * sw;
                    if (++h == OH) { h = 0; src += plane - OH * row; }
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

hipError_t launch_slice_u8(const SliceU8Args& a0, hipStream_t s)
{
    SliceU8Args a = a0;
    if (!a.x || !a.y || (!a.identity && !a.table)) return hipErrorInvalidValue;
    long in_img = 1, L = 1;
    for (int i = 0; i < 4; i++) {
        if (a.in_dims[i] < 1 || a.out_dims[i] < 1 || a.start[i] < 0 || a.step[i] < 1) return hipErrorInvalidValue;
        if ((long)a.start[i] + (long)(a.out_dims[i] - 1) * a.step[i] >= (long)a.in_dims[i]) return hipErrorInvalidValue;      // the box stays inside x
        if (a.out_dims[i] == 1) a.step[i] = 1;           // one position: the step is never taken, and no product below is made of it
        if (i > 0) { in_img *= a.in_dims[i]; L *= a.out_dims[i]; }
        if (in_img > 0x7fffffffL - 64 || L > 0x7fffffffL - 64) return hipErrorInvalidValue;                                   // 32-bit positions inside an image
    }
    if (a.out_dims[0] > 65535 || a.out_c0 < 0 || (long)a.out_img < ((long)a.out_c0 + a.out_dims[1]) * a.out_dims[2] * a.out_dims[3]) return hipErrorInvalidValue;
    const bool rows_adjoin = a.step[3] == 1 && a.out_dims[3] == a.in_dims[3] && a.step[2] == 1;
    a.contig = a.step[3] != 1 ? 0 : !rows_adjoin ? 1 : (a.out_dims[2] == a.in_dims[2] && a.step[1] == 1) ? 3 : 2;
    a.w2 = a.w2 && a.step[3] == 2 ? 1 : 0;
    const long chunks = (L + 15) / 16 + 1;               // + 1: a run that starts mid-chunk ends one chunk later
    const dim3 grid((unsigned)((chunks + 63) / 64), (unsigned)a.out_dims[0]);
    if (a.identity) hipLaunchKernelGGL(slice_u8<true>, grid, dim3(64), 0, s, a);
    else hipLaunchKernelGGL(slice_u8<false>, grid, dim3(64), 0, s, a);
    return hipGetLastError();
}

}  // namespace tamd
