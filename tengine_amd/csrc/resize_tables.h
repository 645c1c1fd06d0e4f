// The host-built operands of a nearest Resize node (resize_tables.cc; private).  Plain C++: no HIP in it.  The two builders themselves
// are part of the C ABI (tamd_resize_table, tamd_resize_indices: include/tengine_amd.h).
#pragma once
#include "../../include/tengine_amd.h"

namespace tamd {

// resize.c:47-48: (int)(in_extent * scale), the product int * float in float, truncated by the assignment.  false: the scale is not
// finite and positive, or the product leaves int (the reference's conversion is undefined there); *out may be 0 (an empty output)
bool resize_out_extent(int in_extent, float scale, int* out);

}  // namespace tamd
