// The byte maps of the quantised Sigmoid / Clip / HardSwish / Mish nodes (lut_tables.cc; private).  Plain C++: no HIP in it.
#pragma once
#include "../../include/tengine_amd.h"

namespace tamd {

// does the device run this operator on tensors of this type?  The table of include/tengine_amd.h, read off the one list of builders
// in lut_tables.cc: Sigmoid and Clip in int8 and uint8, HardSwish and Mish in uint8 (the reference has no int8 kernel for them)
bool lut_op_on_device(int op, int dtype);

// the Eltwise types (eltwise_param.h) that both quantised kernels of the reference have a line for with a one-element second operand
// (PROD 0, PROD_SCALAR 1, SUM 2, SUB 4, SUB_SCALAR 5, MIN_SCALAR 8, DIV 10), and with no second operand at all (RSQRT 7, LOG 11, EXP 12,
// SQRT 13, FLOOR 14, SQUARE 15, POWER 17): the lists tamd_eltwise_table builds a byte map for.  The int8 and the uint8 kernel have the
// same cases
bool eltwise_scalar_type(int type);
bool eltwise_unary_type(int type);

}  // namespace tamd
