// The host-built operands of a nearest Interp node (interp_tables.cc; private).  Plain C++: no HIP in it.
#pragma once
#include "../../include/tengine_amd.h"

namespace tamd {

// what interp.c:51-67 makes of a node's parameter on an input of in_h x in_w: the scales the kernel divides by and the output size
struct InterpGeom { float height_scale, width_scale; int out_h, out_w; };

// false: no size the reference would keep.  Both scales non-zero: they stand, and the size is (int)(in * scale), a float product
// truncated.  Otherwise the scales are (float)out / (float)in, rounded to float as the reference stores them -- and the reference's rule
// applied to THOSE scales must give the sizes back: once the scales are filled in, every later inference takes the first branch, and for
// some pairs (11 -> 13 gives 12, 7 -> 31 gives 30) it then shrinks the tensor under a kernel that was planned for the other size
bool interp_resolve(const tamd_interp_param& p, int in_h, int in_w, InterpGeom* g);

// the value of one element before its conversion to int: round(((float)q - (float)in_zp) * in_scale / out_scale + (float)out_zp), the
// division and the addition in float, the rounding the double round().  tamd_interp_table converts and clamps it; resize_ref.c has the
// same two lines (:288 / :349, :310 / :371), so tamd_resize_table (resize_tables.cc) is built from it too
double interp_rounded(int q, float in_scale, int in_zp, float out_scale, int out_zp);

}  // namespace tamd
