// Nearest Interp (every ONNX Resize) of quantised graphs: interp_ref.c:275-301 (int8) and :384-410 (uint8).  The reference dequantises
// the input, moves values -- output pixel (h, w) takes input pixel ((int)(h / height_scale), (int)(w / width_scale)) -- and requantises
// the output.  Neither step is computed here: the two index vectors and the 256-entry byte map come from the host, built at prerun with
// the reference's own arithmetic (interp_tables.cc), so non-integer scales, scales below 1 and scales that differ per axis are all the
// same kernel, and its bytes are the reference's by construction.
//
// The byte map lives in registers, as in lut_u8 (misc_kernels.hip, where the choice is argued): 256 bytes are one dword per lane of a
// wave, staged with one coalesced load; a lookup is a ds_bpermute_b32 from lane b >> 2 and a shift by b & 3 -- no LDS allocation, no
// barrier.  bpermute reads 0 from a disabled lane, so NO THREAD LEAVES EARLY in either kernel: a thread with nothing to do loads
// nothing, looks up zeros and stores nothing.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"

namespace tamd {

// four packed bytes through the table held in `tab` (lane l: entries 4l .. 4l + 3)
__device__ __forceinline__ unsigned interp_map4(unsigned p, unsigned tab)
{
    unsigned o = 0;
#pragma unroll
    for (int b = 0; b < 4; b++) {
        const unsigned q = (p >> (8 * b)) & 0xffu;
        const unsigned t = (unsigned)__builtin_amdgcn_ds_bpermute((int)(q & 0xfcu), (int)tab);      // byte address of lane q >> 2
        o |= ((t >> (8 * (q & 3u))) & 0xffu) << (8 * b);
    }
    return o;
}

// ---- int8, NHWC with a padded channel stride.  One lane per OUTPUT pixel and 16-byte channel vector: one 16-byte load from the source
// pixel, sixteen lookups, one 16-byte store.  Lanes of the last vector behind channel C are WRITTEN AS ZERO whatever table[0] is: they
// are the padding the next convolution's K loop reads (graph_plan.hip: plan_buffers).  x: the input's first channel (a view's offset
// applied); the output is addressed by pixel stride ldc and channel offset c_off (a concat view).
__global__ __launch_bounds__(256) void interp_nearest_i8_kernel(InterpI8Args a)
{
    const unsigned tab = a.table[threadIdx.x & 63];
    const int nv = (a.C + 15) / 16;
    const unsigned total = (unsigned)a.N * a.OH * a.OW * nv;         // (fits: launch_interp_i8) -- the position in 32-bit divisions
    unsigned idx = blockIdx.x * blockDim.x + threadIdx.x;
    const bool inside = idx < total;
    if (!inside) idx = 0;
    const int v = (int)(idx % (unsigned)nv); idx /= (unsigned)nv;
    const int ox = (int)(idx % (unsigned)a.OW); idx /= (unsigned)a.OW;
    const int oy = (int)(idx % (unsigned)a.OH);
    const int n = (int)(idx / (unsigned)a.OH);
    uint4 d = make_uint4(0u, 0u, 0u, 0u);
    if (inside) d = *reinterpret_cast<const uint4*>(a.x + (((size_t)n * a.H + a.iy[oy]) * a.W + a.ix[ox]) * a.cs_in + v * 16);
    const int valid = a.C - v * 16;                  // channels of this vector (>= 16: all of it)
    unsigned p[4] = {d.x, d.y, d.z, d.w};
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const unsigned m = interp_map4(p[k], tab);
        const int left = valid - 4 * k;              // mapped bytes of this dword
        p[k] = left >= 4 ? m : (left <= 0 ? 0u : m & (0xffffffffu >> (8 * (4 - left))));
    }
    if (inside)
        *reinterpret_cast<uint4*>(a.y + (((size_t)n * a.OH + oy) * a.OW + ox) * a.ldc + a.c_off + v * 16) = make_uint4(p[0], p[1], p[2], p[3]);
}

hipError_t launch_interp_i8(const InterpI8Args& a, hipStream_t s)
{
    if (a.N < 1 || a.C < 1 || a.H < 1 || a.W < 1 || a.OH < 1 || a.OW < 1 || !a.iy || !a.ix || !a.table) return hipErrorInvalidValue;
    const int cv = (a.C + 15) / 16 * 16;             // whole vectors: inside the input's pixel, inside the output's slice
    if (a.cs_in % 16 || a.ldc % 16 || a.c_off % 16 || cv > a.cs_in || a.c_off + cv > a.ldc) return hipErrorInvalidValue;
    if (((uintptr_t)a.x | (uintptr_t)a.y) & 15) return hipErrorInvalidValue;
    const long total = (long)a.N * a.OH * a.OW * (cv / 16);
    if (total > 0x7fffff00L) return hipErrorInvalidValue;           // the kernel counts lanes in 32 bits
    hipLaunchKernelGGL(interp_nearest_i8_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, a);
    return hipGetLastError();
}

// ---- uint8, dense NCHW.  The C output planes of one image are ONE run of L = C * OH * OW bytes (at channel out_c0 of an image of
// out_img bytes: the tensor itself, or its slice of a concat buffer), rows contiguous along x.  A plane may be odd-sized, so neither a
// row nor a plane starts aligned in general: the run is cut at the 16-byte boundaries OF ITS ADDRESS.  Thread t of an image owns the
// aligned 16 bytes number t counted from the boundary at or below the run's first byte; the bytes [lo, hi) of them belong to the run.
// A whole chunk is gathered byte by byte (source bytes of neighbouring output bytes are up to 1 / scale apart), mapped, and stored with
// one 16-byte store; the ragged head and tail chunks store their bytes one by one and touch nothing outside the run.  The position
// (channel, row, column) is divided out once per thread; the ragged chunks (and every chunk of a map narrower than 16) step it from
// byte to byte.  IDENT: equal quantisation on both sides makes the uint8 map the identity on all 256 bytes -- no lookups.
// Blocks of ONE wave: a thread carries 16 output bytes, so a neck-sized tensor (1 x 128 x 40 x 40) is 12 800 threads -- 50 blocks of
// 256 would leave four fifths of the CUs idle.
template <bool IDENT>
__global__ __launch_bounds__(64) void interp_nearest_u8_kernel(InterpU8Args a)
{
    const unsigned tab = IDENT ? 0u : a.table[threadIdx.x & 63];
    const int n = blockIdx.y;
    const int OHW = a.OH * a.OW, L = a.C * OHW;
    uint8_t* run = a.y + (size_t)n * a.out_img + (size_t)a.out_c0 * OHW;
    const int mis = (int)((uintptr_t)run & 15);
    const long first = ((long)blockIdx.x * blockDim.x + threadIdx.x) * 16 - mis;       // run index of this chunk's byte 0
    const int lo = first < 0 ? (int)-first : 0;
    const int hi = first >= L ? 0 : (L - first >= 16 ? 16 : (int)(L - first));
    unsigned p[4] = {0u, 0u, 0u, 0u};
    const uint8_t* xs = a.x + (size_t)n * a.C * a.H * a.W;
    if (lo == 0 && hi == 16 && a.OW >= 16) {
        // a whole chunk with at most ONE row boundary inside it -- nearly every chunk of a tensor of any size: the two source rows are
        // found first, then the sixteen gathers depend on nothing but their own index load and are all in flight together (the stepping
        // loop below chains every load behind the position of the byte before it)
        const int j0 = (int)first;
        const int ch = j0 / OHW, r = j0 - ch * OHW, oy = r / a.OW, ox = r - oy * a.OW;
        const bool last = oy + 1 == a.OH;                // the next row opens the next channel (behind the last one: computed, never read)
        const uint8_t* row0 = xs + ((size_t)ch * a.H + a.iy[oy]) * a.W;
        const uint8_t* row1 = xs + ((size_t)(ch + (last ? 1 : 0)) * a.H + a.iy[last ? 0 : oy + 1]) * a.W;
#pragma unroll
        for (int j = 0; j < 16; j++) {
            const int o = ox + j;
            const bool wrap = o >= a.OW;
            p[j >> 2] |= (unsigned)(wrap ? row1 : row0)[a.ix[wrap ? o - a.OW : o]] << (8 * (j & 3));
        }
    } else if (lo < hi) {
        const int j0 = (int)(first + lo);
        int ch = j0 / OHW, r = j0 - ch * OHW, oy = r / a.OW, ox = r - oy * a.OW;
        const uint8_t* row = xs + ((size_t)ch * a.H + a.iy[oy]) * a.W;
#pragma unroll
        for (int j = 0; j < 16; j++)                     // (unrolled: registers indexed by constants, no scratch memory)
            if (j >= lo && j < hi) {
                p[j >> 2] |= (unsigned)row[a.ix[ox]] << (8 * (j & 3));
                if (++ox == a.OW) {
                    ox = 0;
                    if (++oy == a.OH) { oy = 0; ch++; }
                    row = xs + ((size_t)ch * a.H + a.iy[oy]) * a.W;      // (behind the run's last byte: computed, never read)
                }
            }
    }
    if (!IDENT) {
#pragma unroll
        for (int k = 0; k < 4; k++) p[k] = interp_map4(p[k], tab);
    }
    if (lo == 0 && hi == 16) {
        *reinterpret_cast<uint4*>(run + first) = make_uint4(p[0], p[1], p[2], p[3]);
    } else if (lo < hi) {
#pragma unroll
        for (int j = 0; j < 16; j++)
            if (j >= lo && j < hi) run[first + j] = (uint8_t)(p[j >> 2] >> (8 * (j & 3)));
    }
}

hipError_t launch_interp_u8(const InterpU8Args& a, hipStream_t s)
{
    if (a.N < 1 || a.N > 65535 || a.C < 1 || a.H < 1 || a.W < 1 || a.OH < 1 || a.OW < 1 || !a.iy || !a.ix || !a.table) return hipErrorInvalidValue;
    const long L = (long)a.C * a.OH * a.OW;
    if (L > 0x7fffffffL - 64 || (long)a.C * a.H * a.W > 0x7fffffffL || a.out_c0 < 0 || (long)a.out_img < ((long)a.out_c0 + a.C) * a.OH * a.OW) return hipErrorInvalidValue;
    const long chunks = (L + 15) / 16 + 1;           // + 1: a run that starts mid-chunk ends one chunk later
    const dim3 grid((unsigned)((chunks + 63) / 64), (unsigned)a.N);
    if (a.identity) hipLaunchKernelGGL(interp_nearest_u8_kernel<true>, grid, dim3(64), 0, s, a);
    else hipLaunchKernelGGL(interp_nearest_u8_kernel<false>, grid, dim3(64), 0, s, a);
    return hipGetLastError();
}

}  // namespace tamd
