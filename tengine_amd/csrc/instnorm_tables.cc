// One plane of the uint8 InstanceNorm, restated from the built reference: the specification of the kernels in instnorm.hip and what the
// CPU tests pin to the real reference library (tests/test_instnorm_cpu.py).  Plain C++, compiled with contraction off; every fused
// operation of the reference's object code is an fmaf here and nothing else is fused.
//
// instancenorm_ref.c:101-183 (ref_instancenorm_uint8; run() calls it at :222 with the literal 0 as `layout`, and TENGINE_LAYOUT_NCHW is 0:
// in the object code run() ends in a jump to the routine with that argument zeroed) as gcc -O3 -mfma -std=gnu99 compiled it -- read
// from the disassembly of the reference's own object file, function ref_instancenorm_uint8, NCHW branch (the strided NHWC branch is
// never taken):
//  - dequantisation :125-126  vcvtdq2ps / vsubps zero / vmulps scale (tail: vcvtsi2ss, vsubss, vmulss): ((float)x - (float)zp) * scale,
//    two rounded operations
//  - sum :135-142             eight vaddss per iteration on the elements in ascending order (the vector load only feeds the scalar
//    adds; shuffles pick element 1, 2, 3, ...), then up to seven vaddss: ONE sequential chain, as the C text says
//  - mean :143                vdivss by (float)size
//  - sqsum :145-153           vsubps mean, vmulps t * t -- the product is ROUNDED --, then eight (main loop) or four (one xmm step for
//    a remainder of at least four) vaddss in ascending order; the last size % 4 elements go through the scalar loop, and THAT one is
//    vsubss + vfmadd231ss: sqsum = fma(t, t, sqsum).  So the elements below size - size % 4 are added unfused and the last size % 4
//    fused, still one chain in ascending order
//  - var :154                 vdivss by (float)size
//  - a :156                   vaddss eps + var in float; vcvtss2sd of that and of gamma; vsqrtsd; vdivsd; vcvtsd2ss: the sqrt and the
//    quotient stay double, one rounding to float at the end
//  - b :157                   vfnmadd213ss: fma(-mean, a, beta)
//  - y :158-165               vfmadd132ps in the vector loop and vfmadd132ss / vfmadd231ss in both scalar forms: fma(v, a, b) everywhere,
//    so the vectorised loop and its tails agree
//  - requantisation :170-178  vdivss out_scale; vaddss (float)out_zp; roundf; vcvttss2si; vpmaxsd 0; vpminsd 255
#include <math.h>
#include <stdint.h>

#include "instnorm_tables.h"

namespace {

inline float in_dequant(unsigned char u, float in_scale, int in_zp) { return ((float)u - (float)in_zp) * in_scale; }

}  // namespace

extern "C" int tamd_instancenorm_plane(const unsigned char* x, int size, float gamma, float beta, float eps, float in_scale, int in_zp, float out_scale,
                                       int out_zp, unsigned char table[256], float stats[4])
{
    if (!x || size < 1 || !table) return -1;
    float sum = 0.f, sqsum = 0.f, mean;
    const int body = size - size % 4;
    for (int j = 0; j < size; j++) sum = sum + in_dequant(x[j], in_scale, in_zp);
    mean = sum / (float)size;
    for (int j = 0; j < body; j++) {
        const float t = in_dequant(x[j], in_scale, in_zp) - mean;
        const float p = t * t;
        sqsum = sqsum + p;
    }
    for (int j = body; j < size; j++) {
        const float t = in_dequant(x[j], in_scale, in_zp) - mean;
        sqsum = fmaf(t, t, sqsum);
    }
    const float var = sqsum / (float)size;
    const float ve = var + eps;
    const float a = (float)((double)gamma / sqrt((double)ve));
    const float b = fmaf(-mean, a, beta);
    if (stats) { stats[0] = sum; stats[1] = sqsum; stats[2] = a; stats[3] = b; }
    unsigned char t[256];
    for (int u = 0; u < 256; u++) {
        const float y = fmaf(in_dequant((unsigned char)u, in_scale, in_zp), a, b);
        const float r = roundf(y / out_scale + (float)out_zp);
        if (!(r >= -2147483648.f && r < 2147483648.f)) return -2;
        int q = (int)r;
        if (q > 255) q = 255;
        else if (q < 0) q = 0;
        t[u] = (unsigned char)q;
    }
    for (int u = 0; u < 256; u++) table[u] = t[u];
    return 0;
}
