// The host-built byte map of the quantised Transpose (transpose_tables.cc; private).  Plain C++: no HIP in it.  The builder itself is
// part of the C ABI (tamd_transpose_table: include/tengine_amd.h).
#pragma once
#include "../../include/tengine_amd.h"
