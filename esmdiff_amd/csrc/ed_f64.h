// ed_f64.h — the float64 primitives that more than one analysis unit uses.  Device only.
// sq3 and dist are written as (dx dx + dy dy) + dz dz, the order of the numpy restatements under tests/.  Whether the products are
// contracted into FMAs, and so the bits, follows the INCLUDING unit's flags: every present user (lddt, dssp, contacts, shape, sasa)
// is compiled with -ffp-contract=off (build.py) and gets numpy's bits.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

namespace ed {

__device__ __forceinline__ double quiet_nan() { return __longlong_as_double(0x7ff8000000000000ll); }
__device__ __forceinline__ double sq3(double dx, double dy, double dz) { return (dx * dx + dy * dy) + dz * dz; }
__device__ __forceinline__ double dist(double dx, double dy, double dz) { return sqrt((dx * dx + dy * dy) + dz * dz); }

}  // namespace ed
