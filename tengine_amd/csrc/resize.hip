// Nearest Resize of a quantised graph at WHOLE-NUMBER factors, the replicate form (resize_ref.c:261-381): output pixel (h, w) takes input
// pixel (h / sh, w / sw) through the byte map between the two tensors' quantisation parameters (tamd_resize_table).  x2 is what nearly
// every Resize node is (the up-sampling of a YOLOv3 / YOLOv4 neck).  interp.hip's kernels serve the node at any scale -- a lane per
// OUTPUT vector, two index loads and three divisions per lane, every source value mapped sh * sw times -- and are form 0 of the node
// (TAMD_PIN=resize_form=0); here a lane owns SOURCE data, maps it once and stores its copies, with no index vector at all.  The planner
// (plan_resize) takes this form only where the host-built index vectors ARE i / sh and j / sw (node_rules.h: ResizeGeom::sh / sw).
// One image: the reference defines the operator for batch 1 only.
//
// The byte map lives in registers, as in lut_u8 and interp.hip: 256 bytes are one dword per lane of a wave; a lookup is a
// ds_bpermute_b32 from lane b >> 2 and a shift by b & 3.  bpermute reads 0 from a disabled lane, so NO THREAD LEAVES EARLY and every
// lookup stands in code that the whole wave runs: a thread with nothing to do loads nothing, looks up zeros and stores nothing.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"

namespace tamd {

// four packed bytes through the table held in `tab` (lane l: entries 4l .. 4l + 3)
__device__ __forceinline__ unsigned resize_map4(unsigned p, unsigned tab)
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

// ---- int8, NHWC with a padded channel stride.  A lane owns one 16-channel vector of one SOURCE pixel: one 16-byte load, sixteen
// lookups, sh * sw 16-byte stores.  Lanes of the last vector behind channel C are WRITTEN AS ZERO whatever table[0] is: they are the
// padding the next convolution's K loop reads.  x: the input's first channel (a view's offset applied), read where it lies; the output
// is addressed by pixel stride ldc and channel offset c_off (a concat view).
__global__ __launch_bounds__(256) void resize_rep_i8(ResizeRepI8Args a)
{
    const unsigned tab = a.table[threadIdx.x & 63];
    const int nv = (a.C + 15) / 16;
    const unsigned total = (unsigned)a.H * a.W * nv;                 // (fits: launch_resize_rep_i8)
    unsigned idx = blockIdx.x * blockDim.x + threadIdx.x;
    const bool inside = idx < total;
    if (!inside) idx = 0;
    const int v = (int)(idx % (unsigned)nv); idx /= (unsigned)nv;    // idx: the source pixel
    const int sx = (int)(idx % (unsigned)a.W);
    const int sy = (int)(idx / (unsigned)a.W);
    uint4 d = make_uint4(0u, 0u, 0u, 0u);
    if (inside) d = *reinterpret_cast<const uint4*>(a.x + (size_t)idx * a.cs_in + v * 16);
    const int valid = a.C - v * 16;                  // channels of this vector (>= 16: all of it)
    unsigned p[4] = {d.x, d.y, d.z, d.w};
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const unsigned m = resize_map4(p[k], tab);
        const int left = valid - 4 * k;              // mapped bytes of this dword
        p[k] = left >= 4 ? m : (left <= 0 ? 0u : m & (0xffffffffu >> (8 * (4 - left))));
    }
    if (inside) {
        const uint4 o = make_uint4(p[0], p[1], p[2], p[3]);
        const size_t OW = (size_t)a.W * a.sw;
        int8_t* y0 = a.y + ((size_t)sy * a.sh * OW + (size_t)sx * a.sw) * a.ldc + a.c_off + v * 16;
        for (int i = 0; i < a.sh; i++)
            for (int j = 0; j < a.sw; j++) *reinterpret_cast<uint4*>(y0 + ((size_t)i * OW + j) * a.ldc) = o;
    }
}

hipError_t launch_resize_rep_i8(const ResizeRepI8Args& a, hipStream_t s)
{
    if (!a.x || !a.y || !a.table || a.C < 1 || a.H < 1 || a.W < 1 || a.sh < 1 || a.sw < 1) return hipErrorInvalidValue;
    const int cv = (a.C + 15) / 16 * 16;             // whole vectors: inside the input's pixel, inside the output's slice
    if (a.cs_in % 16 || a.ldc % 16 || a.c_off % 16 || a.c_off < 0 || cv > a.cs_in || a.c_off + cv > a.ldc) return hipErrorInvalidValue;
    if (((uintptr_t)a.x | (uintptr_t)a.y) & 15) return hipErrorInvalidValue;
    const long total = (long)a.H * a.W * (cv / 16);
    if (total > 0x7fffff00L) return hipErrorInvalidValue;           // the kernel counts lanes in 32 bits
    if ((double)a.H * a.sh > 2147483000.0 || (double)a.W * a.sw > 2147483000.0 || (double)a.H * a.sh * (double)a.W * a.sw * (double)a.ldc > 9.0e18) return hipErrorInvalidValue;
    hipLaunchKernelGGL(resize_rep_i8, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, a);
    return hipGetLastError();
}

// ---- uint8, dense NCHW.  The C output planes are ONE run of L = C * OH * OW bytes (at channel out_c0 of the image y lies in: the
// tensor itself, or its slice of a Concat's buffer), cut at the 16-byte boundaries OF ITS ADDRESS as interp_nearest_u8 cuts it: thread t
// owns the aligned 16 bytes number t counted from the boundary at or below the run's first byte; the bytes [lo, hi) of them belong to
// the run.  It divides its first byte's position into (channel, row, column) once.
//  (a) sw == 2 and a whole chunk inside one output row that starts at an even column: its sixteen bytes are the 8 source bytes from
//      column ox / 2 on, each twice -- one 8-byte load at any alignment, mapped ONCE, doubled by four v_perm_b32, one 16-byte store.
//      (With sw == 2 every row and every plane has an even byte count, so in a 16-byte-aligned buffer EVERY whole chunk starts at an
//      even column, inside a Concat's buffer too: a nine-byte form for odd columns would never run, and is not built.  An odd column
//      takes (b).);
//  (b) anything else -- another sw, a chunk that crosses a row or a plane, the ragged head and tail: byte by byte with carried
//      positions (row = sy * sh + ry, column = sx * sw + rx), then mapped.
// The lookups stand behind the branch, in code every lane runs; whether the upper two dwords hold anything to look up is asked of the
// whole wave (a ballot: the same answer in every lane, so the branch is the wave's and no lane is disabled at a bpermute).  The ragged
// chunks store byte by byte: nothing outside the run is touched (the neighbours of a Concat's slice stay as they are).
// IDENT: equal quantisation on both sides makes the uint8 map the identity on all 256 bytes -- no lookups.
// Blocks of ONE wave, for the reason given at interp_nearest_u8: a neck-sized tensor is a few thousand threads.
template <bool IDENT>
__global__ __launch_bounds__(64) void resize_rep_u8(ResizeRepU8Args a)
{
    const unsigned tab = IDENT ? 0u : a.table[threadIdx.x & 63];
    const int sh = a.sh, sw = a.sw, OH = a.H * sh, OW = a.W * sw;
    const int OHW = OH * OW, L = a.C * OHW;          // (fit: launch_resize_rep_u8)
    uint8_t* run = a.y + (size_t)a.out_c0 * OHW;
    const int mis = (int)((uintptr_t)run & 15);
    const long first = ((long)blockIdx.x * blockDim.x + threadIdx.x) * 16 - mis;       // run index of this chunk's byte 0
    const int lo = first < 0 ? (int)-first : 0;
    const int hi = first >= L ? 0 : (L - first >= 16 ? 16 : (int)(L - first));
    const bool whole = lo == 0 && hi == 16;
    unsigned r[4] = {0u, 0u, 0u, 0u};
    bool doubled = false, walked = false;            // path (a): r[0 .. 1] hold 8 source bytes; path (b): r[] holds the 16 output bytes' sources
    if (lo < hi) {
        const int j0 = (int)(first + lo);
        int ch = j0 / OHW;
        const int rem = j0 - ch * OHW;
        int oy = rem / OW, ox = rem - oy * OW;
        int sy = oy / sh;
        if (whole && sw == 2 && OW - ox >= 16 && (ox & 1) == 0) {
            __builtin_memcpy(r, a.x + ((size_t)ch * a.H + sy) * a.W + (ox >> 1), 8);      // columns ox / 2 .. ox / 2 + 7 <= W - 1
            doubled = true;
        } else {
            walked = true;
            int ry = oy - sy * sh, sx = ox / sw;
            int rx = ox - sx * sw;
            const uint8_t* row = a.x + ((size_t)ch * a.H + sy) * a.W;
#pragma unroll
            for (int j = 0; j < 16; j++)                 // (unrolled: registers indexed by constants, no scratch memory)
                if (j >= lo && j < hi) {
                    r[j >> 2] |= (unsigned)row[sx] << (8 * (j & 3));
                    if (++rx == sw) { rx = 0; sx++; }
                    if (++ox == OW) {
                        ox = 0; sx = 0; rx = 0;
                        if (++ry == sh) { ry = 0; sy++; }
                        if (++oy == OH) { oy = 0; sy = 0; ry = 0; ch++; }
                        row = a.x + ((size_t)ch * a.H + sy) * a.W;       // (behind the run's last byte: computed, never read)
                    }
                }
        }
    }
    if (!IDENT) {
        r[0] = resize_map4(r[0], tab);
        r[1] = resize_map4(r[1], tab);
        if (__ballot(walked) != 0ull) { r[2] = resize_map4(r[2], tab); r[3] = resize_map4(r[3], tab); }
    }
    unsigned p[4] = {r[0], r[1], r[2], r[3]};
    if (doubled) {                                       // source bytes 0 0 1 1 | 2 2 3 3 | 4 4 5 5 | 6 6 7 7
        p[0] = __builtin_amdgcn_perm(r[0], r[0], 0x01010000u); p[1] = __builtin_amdgcn_perm(r[0], r[0], 0x03030202u);
        p[2] = __builtin_amdgcn_perm(r[1], r[1], 0x01010000u); p[3] = __builtin_amdgcn_perm(r[1], r[1], 0x03030202u);
    }
    if (whole) {
        *reinterpret_cast<uint4*>(run + first) = make_uint4(p[0], p[1], p[2], p[3]);
    } else if (lo < hi) {
#pragma unroll
        for (int j = 0; j < 16; j++)
            if (j >= lo && j < hi) run[first + j] = (uint8_t)(p[j >> 2] >> (8 * (j & 3)));
    }
}

hipError_t launch_resize_rep_u8(const ResizeRepU8Args& a, hipStream_t s)
{
    if (!a.x || !a.y || !a.table || a.C < 1 || a.H < 1 || a.W < 1 || a.sh < 1 || a.sw < 1 || a.out_c0 < 0) return hipErrorInvalidValue;
    const double OH = (double)a.H * a.sh, OW = (double)a.W * a.sw;
    if ((double)a.C * OH * OW > (double)(0x7fffffffL - 64) || (double)a.C * a.H * a.W > (double)0x7fffffffL) return hipErrorInvalidValue;      // 32-bit positions
    const long L = (long)a.C * (long)OH * (long)OW;
    if (a.out_img < ((long)a.out_c0 + a.C) * (long)OH * (long)OW) return hipErrorInvalidValue;      // the run stays inside its image
    const long chunks = (L + 15) / 16 + 1;           // + 1: a run that starts mid-chunk ends one chunk later
    const dim3 grid((unsigned)((chunks + 63) / 64));
    if (a.identity) hipLaunchKernelGGL(resize_rep_u8<true>, grid, dim3(64), 0, s, a);
    else hipLaunchKernelGGL(resize_rep_u8<false>, grid, dim3(64), 0, s, a);
    return hipGetLastError();
}

}  // namespace tamd
