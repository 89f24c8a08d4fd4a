// A slot's page-locked result buffer (the last kernel of a chain writes there through the buffer's device view):
//   [PIN_AFF ..)     this proof's commitments after sync_results(), affine
//   [PIN_XYZZ ..)    MSM sums as they leave the device, XYZZ: up to MSM_ARGS_MAX points - a gang's merged batch lands in its LEAD's
//   [PIN_FR ..)      evaluations / the grand product's total / an opening's values (kzg_run.h)
//   PIN_TAIL, PIN_DENSITY   the quotient's tail flag, the wires' digit count
#pragma once
#include <stddef.h>

namespace apk {
constexpr size_t PIN_AFF = 0, PIN_XYZZ = 1024, PIN_FR = 4096, PIN_TAIL = 6144, PIN_DENSITY = 6208, PIN_BYTES = 8192;
}  // namespace apk
