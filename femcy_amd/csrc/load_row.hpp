// Device-only: the row load shared by the gather kernels of kernels_assembly.hip and kernels_explicit.hip.
#pragma once
#include <hip/hip_runtime.h>

namespace femcy {

// a gradient row / force row / coordinate triple is dm contiguous doubles at 8-byte alignment: one 16-byte load (+ one
// 8-byte load for dm = 3) instead of dm 8-byte loads.  The gather kernels are bound by the texture-address path
// (24-byte gathers: DESIGN.md section 3); a third fewer load instructions is a third fewer address cycles.
typedef double femcy_d2u __attribute__((ext_vector_type(2), aligned(8)));
template <int DM>
__device__ __forceinline__ void load_row(const double* __restrict__ p, double (&v)[DM]) {
    const femcy_d2u t = *reinterpret_cast<const femcy_d2u*>(p);
    v[0] = t.x;
    v[1] = t.y;
    if (DM == 3) v[DM - 1] = p[2];
}

}  // namespace femcy
