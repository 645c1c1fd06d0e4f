// The host-built operands of Split and ShuffleChannel (chanmap_tables.cc; private).  Plain C++: no HIP in it.  The two builders
// themselves are part of the C ABI (tamd_shuffle_sources, tamd_split_table: include/tengine_amd.h).
#pragma once
#include "../../include/tengine_amd.h"
