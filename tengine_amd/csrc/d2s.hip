// DepthToSpace of a quantised graph (depthtospace_ref.c: ref_depthtospace_uint8 / _int8), the shuffle behind a sub-pixel convolution:
//   out[n, s, h, w] = in[n, s * r * r + (h % r) * r + (w % r), h / r, w / r]          (the CRD order, torch's PixelShuffle)
// The reference moves RAW bytes and reads no quantisation parameter of either tensor, so there is no byte map here and the int8 byte
// -128 stays -128 (but for fix128, below).  Two kernels, one per layout of the device's quantised graphs; the canonical gather of
// transpose.hip over (N, C, r, r, H, W) in the order (0, 1, 4, 2, 5, 3) is the baseline they are measured against (TAMD_PIN=d2s_form=0).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "epilogue.h"       // fix128_4
#include "kernels.h"

namespace tamd {

// uint8, dense NCHW.  An output row is the byte interleave of r input rows out of r different planes.  The C * OH * OW output bytes of
// one image are ONE run (at channel out_c0 of an image of out_img bytes) cut at the 16-byte boundaries OF ITS ADDRESS, as slice_u8 cuts
// its run: thread t of an image owns the aligned 16 bytes number t counted from the boundary at or below the run's first byte, and the
// bytes [lo, hi) of them belong to the run.  It decomposes its first byte into (s, h, w) once.
//  (a) r == 2, a whole chunk inside one output row that starts at an even w: its sixteen bytes are eight bytes of plane
//      s * 4 + 2 * (h % 2) and eight of the plane behind it, both from row h / 2, column w / 2 on -- two 8-byte loads at any alignment,
//      four byte interleaves (v_perm_b32), one 16-byte store;
//  (b) anything else -- another r, a chunk that crosses a row or a plane or starts at an odd w, the ragged head and tail: byte by byte
//      with carried indices (s; h = hq * r + hr; w = wq * r + wr), as the reference's loops walk.
// The ragged chunks store byte by byte: nothing outside the run is touched (the neighbours of a Concat's slice stay as they are).
__global__ __launch_bounds__(256) void d2s_u8(D2sU8Args a)
{
    const int n = blockIdx.y;
    const int r = a.r, H = a.H, W = a.W, OH = H * r, OW = W * r;
    const int OHW = OH * OW;
    const long L = (long)a.C * OHW;
    uint8_t* run = a.y + (size_t)n * a.out_img + (size_t)a.out_c0 * OHW;
    const int mis = (int)((uintptr_t)run & 15);
    const long first = ((long)blockIdx.x * blockDim.x + threadIdx.x) * 16 - mis;       // run index of this chunk's byte 0
    const int lo = first < 0 ? (int)-first : 0;
    const int hi = first >= L ? 0 : (L - first >= 16 ? 16 : (int)(L - first));
    if (lo >= hi) return;
    const int HW = H * W;
    const uint8_t* xs = a.x + (size_t)n * ((size_t)a.C * r * r * HW);
    const int j0 = (int)(first + lo);
    int s = j0 / OHW;
    const int rem = j0 - s * OHW;
    int h = rem / OW, w = rem - h * OW;
    const bool whole = lo == 0 && hi == 16;
    unsigned p[4] = {0u, 0u, 0u, 0u};
    if (whole && r == 2 && OW - w >= 16 && (w & 1) == 0) {
        const uint8_t* s0 = xs + ((size_t)(s * 4 + 2 * (h & 1)) * H + (h >> 1)) * W + (w >> 1);
        unsigned e[2], o[2];
        __builtin_memcpy(e, s0, 8);                      // the even output columns: offset_w 0
        __builtin_memcpy(o, s0 + HW, 8);                 // the odd ones: the next plane
        p[0] = __builtin_amdgcn_perm(o[0], e[0], 0x05010400u); p[1] = __builtin_amdgcn_perm(o[0], e[0], 0x07030602u);
        p[2] = __builtin_amdgcn_perm(o[1], e[1], 0x05010400u); p[3] = __builtin_amdgcn_perm(o[1], e[1], 0x07030602u);
    } else {
        int hq = h / r, wq = w / r;
        int hr = h - hq * r, wr = w - wq * r;
#pragma unroll
        for (int j = 0; j < 16; j++)                     // (unrolled: registers indexed by constants, no scratch memory)
            if (j >= lo && j < hi) {
                const size_t src = ((size_t)((s * r + hr) * r + wr) * H + hq) * W + wq;
                p[j >> 2] |= (unsigned)xs[src] << (8 * (j & 3));
                if (++wr == r) { wr = 0; wq++; }
                if (++w == OW) {                         // (behind the run's last byte nothing is read any more)
                    w = 0; wq = 0; wr = 0;
                    if (++hr == r) { hr = 0; hq++; }
                    if (++h == OH) { h = 0; hq = 0; hr = 0; s++; }
                }
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

// int8, NHWC.  A lane owns the 16 output channels g * 16 .. + 15 of one output pixel (n, h, w): they are the channels
// (g * 16 + k) * r * r + (h % r) * r + (w % r) of input pixel (h / r, w / r), a stride-r*r gather out of that pixel's vector, read
// where the pixel lies (any pixel stride: a concat view or a Split view is read in place).
//  (a) r == 2 and all 16 channels exist: they are byte (h % 2) * 2 + (w % 2) of the sixteen dwords at g * 64 -- four 16-byte loads,
//      and per output dword three v_perm_b32 with a selector the lane makes of its (h, w);
//  (b) anything else: one byte load per existing channel.
// One 16-byte store; the lanes from C on are written as zero.  fix128: 0x80 -> 0x7f (the Concat of several inputs the output lies in).
__global__ __launch_bounds__(256) void d2s_i8(D2sI8Args a)
{
    const int G = (a.C + 15) / 16;
    const int r = a.r, OH = a.H * r, OW = a.W * r;
    const long total = (long)a.N * OH * OW * G;
    long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    const int g = (int)(idx % G); idx /= G;              // idx: the output pixel
    const long pix = idx;
    const int w = (int)(idx % OW); idx /= OW;
    const int h = (int)(idx % OH);
    const int n = (int)(idx / OH);
    const int hq = h / r, wq = w / r;
    const int off = (h - hq * r) * r + (w - wq * r);
    const int8_t* xs = a.x + (((size_t)n * a.H + hq) * a.W + wq) * a.cs_in;
    unsigned p[4] = {0u, 0u, 0u, 0u};
    const int have = a.C - g * 16;                       // channels of this group that exist (>= 1)
    if (r == 2 && have >= 16) {
        const uint4* v = reinterpret_cast<const uint4*>(xs + g * 64);      // (16-byte aligned: x, cs_in and g * 64 are)
        const unsigned s01 = (unsigned)off | (unsigned)(4 + off) << 8;     // byte `off` of the low operand, then of the high one
        const unsigned sel = s01 | 0x0c0c0000u;                            // (0x0c: a zero byte)
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const uint4 d = v[k];
            const unsigned t0 = __builtin_amdgcn_perm(d.y, d.x, sel), t1 = __builtin_amdgcn_perm(d.w, d.z, sel);
            p[k] = __builtin_amdgcn_perm(t1, t0, 0x05040100u);
        }
    } else {
        const int r2 = r * r;
#pragma unroll
        for (int k = 0; k < 16; k++)
            if (k < have) p[k >> 2] |= (unsigned)(uint8_t)xs[(size_t)(g * 16 + k) * r2 + off] << (8 * (k & 3));
    }
    if (a.fix128) {
#pragma unroll
        for (int k = 0; k < 4; k++) p[k] = fix128_4(p[k]);
    }
    *reinterpret_cast<uint4*>(a.y + (size_t)pix * a.ldc + a.c_off + g * 16) = make_uint4(p[0], p[1], p[2], p[3]);
}

hipError_t launch_d2s_u8(const D2sU8Args& a, hipStream_t s)
{
    if (!a.x || !a.y || a.N < 1 || a.C < 1 || a.H < 1 || a.W < 1 || a.r < 1 || a.r > 0x7fff || a.N > 65535 || a.out_c0 < 0) return hipErrorInvalidValue;
    const long r = a.r, OH = a.H * r, OW = a.W * r;
    if (OH > 0x7fffffffL - 64 || OW > 0x7fffffffL - 64 || (long)a.C * r * r > 0x7fffffffL - 64) return hipErrorInvalidValue;
    const long L = (long)a.C * OH * OW;                  // == the input image's bytes
    if ((double)a.C * (double)OH * (double)OW > (double)(0x7fffffffL - 64)) return hipErrorInvalidValue;      // 32-bit positions inside an image
    if (a.out_img < ((long)a.out_c0 + a.C) * OH * OW) return hipErrorInvalidValue;      // the run stays inside its image
    const long chunks = (L + 15) / 16 + 1;               // + 1: a run that starts mid-chunk ends one chunk later
    const dim3 grid((unsigned)((chunks + 255) / 256), (unsigned)a.N);
    hipLaunchKernelGGL(d2s_u8, grid, dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_d2s_i8(const D2sI8Args& a, hipStream_t s)
{
    if (!a.x || !a.y || a.N < 1 || a.C < 1 || a.H < 1 || a.W < 1 || a.r < 1 || a.r > 0x7fff) return hipErrorInvalidValue;
    const long r = a.r, G = (a.C + 15) / 16;
    if ((long)a.C * r * r > (long)a.cs_in) return hipErrorInvalidValue;                  // the input's channels fit its pixel stride
    if (a.cs_in % 16 || ((uintptr_t)a.x & 15) || ((uintptr_t)a.y & 15) || a.ldc % 16 || a.c_off % 16 || a.c_off < 0 || a.c_off + G * 16 > (long)a.ldc) return hipErrorInvalidValue;
    // the last byte read: the last pixel's last channel
    const double pixels_in = (double)a.N * a.H * a.W, pixels_out = pixels_in * (double)r * (double)r;
    if (pixels_out * (double)G > 1.75e12 || pixels_out * (double)a.ldc > 9.0e18) return hipErrorInvalidValue;
    if ((size_t)((long)a.N * a.H * a.W - 1) * (size_t)a.cs_in + (size_t)((long)a.C * r * r) > a.src_bytes) return hipErrorInvalidValue;
    const long total = (long)a.N * a.H * r * a.W * r * G;
    const long blocks = (total + 255) / 256;
    if (blocks > 0x7fffffffL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(d2s_i8, dim3((unsigned)blocks), dim3(256), 0, s, a);
    return hipGetLastError();
}

}  // namespace tamd
