// The arithmetic of the uint8 InstanceNorm that needs no device: tamd_instancenorm_plane (instnorm_tables.cc, declared in tengine_amd.h)
// and the bound instancenorm_refusal (node_rules.h) holds a node to.
#pragma once
#include <math.h>
#include <stddef.h>

#include "../../include/tengine_amd.h"

namespace tamd {

// An upper bound of |y / out_scale + out_zp| over every plane a node can meet: |v| <= 255 * in_scale (zero points lie in 0 .. 255),
// |v - mean| <= 255 * in_scale, |a| <= max|gamma| / sqrt(eps) (var >= 0), so |fma(v, a, b)| = |(v - mean) * a + beta| up to rounding
// <= 255 * in_scale * max|gamma| / sqrt(eps) + max|beta|.  In double; the reference's (int) conversion is defined below 2^31, and the
// rule asks for 2^30: a factor of two above every rounding of the float chain
inline double instancenorm_bound(const float* gamma, const float* beta, size_t C, float eps, float in_scale, float out_scale, int out_zp)
{
    double g = 0, b = 0;
    for (size_t c = 0; c < C; c++) {
        g = fmax(g, fabs((double)gamma[c]));
        b = fmax(b, fabs((double)beta[c]));
    }
    return (255.0 * fabs((double)in_scale) * g / sqrt((double)eps) + b) / fabs((double)out_scale) + fabs((double)out_zp);
}

}  // namespace tamd
