// The byte maps of the quantised Sigmoid / Clip / HardSwish / Mish nodes (lut_tables.cc; private).  Plain C++: no HIP in it.
#pragma once
#include "../../include/tengine_amd.h"

namespace tamd {

// does the device run this operator on tensors of this type?  The table of include/tengine_amd.h, read off the one list of builders
// in lut_tables.cc: Sigmoid and Clip in int8 and uint8, HardSwish and Mish in uint8 (the reference has no int8 kernel for them)
bool lut_op_on_device(int op, int dtype);

}  // namespace tamd
