// The element families the library is instantiated for, and the step from the run-time (npe, dm) of a mesh to the
// compile-time <NPE, DM> of an element pass, for both backends (kernels_assembly.hip, csrc_cpu/femcy_cpu.cpp).  Host-only:
// no HIP header.  A new family is registered HERE, in dispatch_element, and nowhere else.
#pragma once
#include <type_traits>

namespace femcy {

template <int NPE, int DM, class F>
bool dispatch_family(int npe, int dm, F& f) {
    if (npe != NPE || dm != DM) return false;
    f(std::integral_constant<int, NPE>{}, std::integral_constant<int, DM>{});
    return true;
}

// calls f(std::integral_constant<int, NPE>{}, std::integral_constant<int, DM>{}) for the family of the mesh; false, and f
// not called, when (npe, dm) is none of the instantiated families (the caller answers FEMCY_ENOKERNEL):
// (3, 2) CPS3, (4, 2) CPS4, (6, 2) CPS6, (8, 2) CPS8, (4, 3) C3D4, (10, 3) C3D10, (8, 3) C3D8, (6, 3) C3D6
template <class F>
bool dispatch_element(int npe, int dm, F&& f) {
    return dispatch_family<3, 2>(npe, dm, f) || dispatch_family<4, 2>(npe, dm, f) || dispatch_family<6, 2>(npe, dm, f) ||
           dispatch_family<8, 2>(npe, dm, f) || dispatch_family<4, 3>(npe, dm, f) || dispatch_family<10, 3>(npe, dm, f) ||
           dispatch_family<8, 3>(npe, dm, f) || dispatch_family<6, 3>(npe, dm, f);
}

// calls f(std::integral_constant<int, DM>{}) for dm = 3, else for 2 (femcy_set_mesh admits nothing else), and returns
// what f returns
template <class F>
decltype(auto) dispatch_dm(int dm, F&& f) {
    if (dm == 3) return f(std::integral_constant<int, 3>{});
    return f(std::integral_constant<int, 2>{});
}

}  // namespace femcy
