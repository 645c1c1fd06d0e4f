// The host truth of the quantised PReLU nodes (prelu_tables.cc; the two entry points are public: include/tengine_amd.h).  Plain C++:
// no HIP in it.
#pragma once
#include <stddef.h>

#include "../../include/tengine_amd.h"

namespace tamd {

// true when none of the `count` slopes (fp16 bit patterns) widens to inf or NaN through tamd_prelu_slope
bool prelu_slopes_finite(const unsigned short* half_bits, size_t count);

}  // namespace tamd
