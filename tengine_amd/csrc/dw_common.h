// Shared by the depthwise kernels (dwconv.hip, pwdw.hip, chain4.hip): the 4x4 byte transpose in front of the v_dot4 rows, and the patch gather of
// the two launches whose producer is the network's first convolution (pwdw.hip and chain4.hip, PROD 1).
#pragma once
#include <hip/hip_runtime.h>

namespace tamd {

// 4x4 byte transpose: d[p] = pixel p's channels {c0,c1,c2,c3}  ->  x[c] = channel c at pixels {p0,p1,p2,p3}
// v_perm_b32 D = bytes of {S0(hi):S1(lo)} picked by the selector (0-3 -> S1, 4-7 -> S0)
__device__ __forceinline__ void transpose4x4(const unsigned (&d)[4], unsigned (&x)[4])
{
    const unsigned t0 = __builtin_amdgcn_perm(d[1], d[0], 0x05010400u);   // {d0.c0, d1.c0, d0.c1, d1.c1}
    const unsigned t1 = __builtin_amdgcn_perm(d[1], d[0], 0x07030602u);   // {d0.c2, d1.c2, d0.c3, d1.c3}
    const unsigned t2 = __builtin_amdgcn_perm(d[3], d[2], 0x05010400u);   // {d2.c0, d3.c0, d2.c1, d3.c1}
    const unsigned t3 = __builtin_amdgcn_perm(d[3], d[2], 0x07030602u);
    x[0] = __builtin_amdgcn_perm(t2, t0, 0x05040100u);                    // {t0.b0, t0.b1, t2.b0, t2.b1}
    x[1] = __builtin_amdgcn_perm(t2, t0, 0x07060302u);
    x[2] = __builtin_amdgcn_perm(t3, t1, 0x05040100u);
    x[3] = __builtin_amdgcn_perm(t3, t1, 0x07060302u);
}

// PROD 1 of pwdw.hip / chain4.hip: this lane's 16 K bytes of first-conv output pixel (piy, pix) -- the four patch rows (c, ky) of `rows`
// (PwDwArgs::taps), each FOUR consecutive bytes of the NCHW image `xn` -- into the four dwords of `bf`.  Column handling is the same for
// every row: bytes left of the image are shifted in as zeros, bytes right of it masked; rows above / below the image are zero.  All four
// loads are unconditional (clamped addresses) so they fly together.  Args: PwDwArgs | Chain4Args (in_H, in_W, fSH, fSW, fPH, fPW)
template <typename Args, typename V4>
__device__ __forceinline__ void gather_patch_rows(const Args& a, const int8_t* xn, const unsigned (&rows)[4], int piy, int pix, V4& bf)
{
    const int iyb = piy * a.fSH - a.fPH, ixb = pix * a.fSW - a.fPW;
    const int sft = max(-ixb, 0), xs = max(ixb, 0), nvalid = a.in_W - ixb;
    const bool colok = nvalid > 0 && sft < 4;
    const unsigned cmask = nvalid < 4 ? (1u << (8 * max(nvalid, 0))) - 1u : ~0u;
    const int base = iyb * a.in_W + xs;
    unsigned raw[4];
    bool ok[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int iy = iyb + (int)(rows[j] >> 28);
        ok[j] = colok && (unsigned)iy < (unsigned)a.in_H;
        __builtin_memcpy(&raw[j], xn + (ok[j] ? base + (int)(rows[j] & 0xffffffu) : 0), 4);
    }
#pragma unroll
    for (int j = 0; j < 4; j++) bf[j] = ok[j] ? (int)((raw[j] << (8 * sft)) & cmask) : 0;
}

}  // namespace tamd
