// What an entry point of include/femcy.h refuses, and with which words: stated once for the device library (csrc/) and the
// host library (csrc_cpu/).  Host-only, no HIP types.  Every check_* is a function template over the context type (femcy::
// Ctx there, femcy_ctx here; the fields a check reads carry the same name in both), holds an entry's argument and state
// conditions in the order they are tested, and returns FEMCY_OK or the status after set_error.  A check that reads a
// library's own storage stays with that library; where both word it alike, the text is a constant below.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <cmath>
#include <vector>
#include "../../include/femcy.h"

// Nothing here leaves its library: set_error and the inline checks exist in both, and a process may hold both (the device
// library is loaded with RTLD_GLOBAL), so none of them may be bound to the other library's copy.
#pragma GCC visibility push(hidden)
namespace femcy {

// each library defines it over its own thread-local buffer, next to its femcy_last_error
void set_error(const char* fmt, ...);

#define FEMCY_REQUIRE(cond, ...)                    \
    do {                                            \
        if (!(cond)) {                              \
            femcy::set_error(__VA_ARGS__);          \
            return FEMCY_EINVAL;                    \
        }                                           \
    } while (0)

// return the status of a check_* unless it is FEMCY_OK
#define FEMCY_TRY(call)                \
    do {                               \
        const int _rc = (call);        \
        if (_rc) return _rc;           \
    } while (0)

// texts of one-line checks that stand in the entry points themselves, and of checks that read a library's own storage
constexpr const char* TEXT_NULL_CONTEXT = "null context";
constexpr const char* TEXT_NULL_OUTPUT = "null output";
constexpr const char* TEXT_CTX_OUT_NULL = "out is null";
constexpr const char* TEXT_PATTERN_NOT_BUILT = "pattern not built";
constexpr const char* TEXT_NOT_DEFINED = "context not fully defined";
constexpr const char* TEXT_GET_K = "pattern not built or null outputs";
constexpr const char* TEXT_UNKNOWN_OPTION = "unknown option %d";
constexpr const char* TEXT_NULL_VALUES = "null values";
constexpr const char* TEXT_ASSEMBLE_FIRST = "femcy_explicit_stable_dt bounds the matrix of the last femcy_assemble_K: assemble first";

inline bool positive_finite(double x) { return std::isfinite(x) && x > 0.0; }

// what an element pass answers for a mesh whose family dispatch_element (element_dispatch.hpp) does not list
template <class C>
int no_kernel(const C* c, const char* what) {
    set_error("no %s kernel instantiated for npe=%d dm=%d", what, c->npe, c->dm);
    return FEMCY_ENOKERNEL;
}

// ---------------------------------------------------------------------------------- the checks most entries share
// The one question a shared check asks of a library's storage: does vector v exist (femcy_set_mesh allocates all of them)?
// Specialised next to each context.
template <class C>
bool vec_allocated(const C* c, int v);

template <class C>
int check_vec(const C* c, int v) {
    FEMCY_REQUIRE(v >= 0 && v < FEMCY_VEC_COUNT, "vector id %d out of range", v);
    FEMCY_REQUIRE(vec_allocated(c, v), "vectors are allocated by femcy_set_mesh; call it first");
    return FEMCY_OK;
}
#define VEC_OR_FAIL(v) FEMCY_TRY(femcy::check_vec(c, (v)))

template <class C>
int check_ready(const C* c) {
    FEMCY_REQUIRE(c->have_mesh && c->have_element && c->have_material && c->have_pattern,
                  "context not fully defined (mesh=%d element=%d material=%d pattern=%d)", (int)c->have_mesh,
                  (int)c->have_element, (int)c->have_material, (int)c->have_pattern);
    return FEMCY_OK;
}
#define READY_OR_FAIL() FEMCY_TRY(femcy::check_ready(c))

// id names an object of one of the context's lists; what: "body load", "mass object" ...
template <class V>
int check_object(const V& objects, int32_t id, const char* what) {
    FEMCY_REQUIRE(id >= 0 && (size_t)id < objects.size(), "unknown %s %d", what, (int)id);
    return FEMCY_OK;
}
#define FEMCY_OBJECT_OR_FAIL(var, objects, id, what)            \
    FEMCY_TRY(femcy::check_object((objects), (id), (what)));    \
    const auto& var = (objects)[(id)]

template <class C>
int check_have_mesh(const C* c) {
    FEMCY_REQUIRE(c->have_mesh, "femcy_set_mesh must come first");
    return FEMCY_OK;
}

inline int check_rhs_not_scratch(int rhs_vec) {
    FEMCY_REQUIRE(rhs_vec != FEMCY_VEC_TMP0 && rhs_vec != FEMCY_VEC_TMP1, "rhs may not alias the scratch vectors");
    return FEMCY_OK;
}

// ------------------------------------------------------------------------------------------ options
// femcy_set_option: the value ranges of the options that act on both libraries; each keeps its own switch for what the
// option then does (and the device library the ranges of its own knobs)
template <class C>
int check_option(const C* c, int option, int64_t value) {
    switch (option) {
        case FEMCY_OPT_TANGENT:
            FEMCY_REQUIRE(value == 0 || value == 1, "tangent: 0 (reference) or 1 (consistent)");
            break;
        case FEMCY_OPT_DIRECT_MAX_BYTES:
            FEMCY_REQUIRE(value >= (int64_t)1 << 20, "direct solve: the band limit must be at least 1 MiB");
            break;
        case FEMCY_OPT_SELL_SIGMA:
            FEMCY_REQUIRE(value >= 64 && value <= (1 << 24), "sorting window must be in [64, 2^24] nodes");
            FEMCY_REQUIRE(!c->have_pattern, "set the sorting window before femcy_build_pattern");
            break;
        case FEMCY_OPT_NODE_ORDER:
            FEMCY_REQUIRE(value >= 0 && value <= 7, "node order: 0 (caller's numbering), 1 (measured choice), 2..7 (coordinate order k - 2)");
            FEMCY_REQUIRE(!c->have_pattern, "set the node order before femcy_build_pattern");
            break;
        default:
            break;
    }
    return FEMCY_OK;
}

// ------------------------------------------------------------------------------------------ problem definition
inline int check_set_mesh(int32_t nn, int32_t dm, const double* nodes, int32_t ne, int32_t npe, const int32_t* elems) {
    FEMCY_REQUIRE(nodes && elems, "null mesh arrays");
    FEMCY_REQUIRE(nn > 0 && ne > 0, "empty mesh (nn=%d, ne=%d)", nn, ne);
    FEMCY_REQUIRE(dm == 2 || dm == 3, "dm must be 2 or 3, got %d", dm);
    FEMCY_REQUIRE(npe >= 2 && npe <= 27, "npe out of range: %d", npe);
    for (int64_t k = 0; k < (int64_t)ne * npe; ++k)
        FEMCY_REQUIRE(elems[k] >= 0 && elems[k] < nn, "element %lld references node %d outside [0,%d)",
                      (long long)(k / npe), elems[k], nn);
    return FEMCY_OK;
}

template <class C>
int check_set_element(const C* c, int32_t nGP, const double* dN, const double* w, int32_t voigt_kind) {
    FEMCY_TRY(check_have_mesh(c));
    FEMCY_REQUIRE(dN && w && nGP >= 1 && nGP <= 64, "bad element tables (nGP=%d)", nGP);
    FEMCY_REQUIRE((voigt_kind == FEMCY_VOIGT_2D && c->dm == 2) || (voigt_kind == FEMCY_VOIGT_3D && c->dm == 3),
                  "voigt kind %d does not match dm=%d", voigt_kind, c->dm);
    return FEMCY_OK;
}

template <class C>
int check_set_material(const C* c, int32_t kind, const double* Cm, const double* params, int32_t nparams) {
    FEMCY_TRY(check_have_mesh(c));
    FEMCY_REQUIRE(Cm, "null C");
    FEMCY_REQUIRE(kind >= FEMCY_MAT_LIN3D && kind <= FEMCY_MAT_NEOHOOKE, "unknown material kind %d", kind);
    // neo-Hookean exists for dm = 3 (the reference's) and, as an extension, for dm = 2 (plane strain)
    const bool ok_dm = kind == FEMCY_MAT_NEOHOOKE || ((kind == FEMCY_MAT_LIN3D) == (c->dm == 3));
    FEMCY_REQUIRE(ok_dm, "material kind %d does not match dm=%d", kind, c->dm);
    FEMCY_REQUIRE(nparams >= 2 && params, "material needs 2 parameters");
    return FEMCY_OK;
}

template <class C>
int check_get_assembly_used(const C* c, const int32_t* mode) {
    FEMCY_REQUIRE(mode && c->asm_used >= 0, "no assembly has run on this context");
    return FEMCY_OK;
}

// ------------------------------------------------------------------------------------------ vectors
// femcy_vec_upload / femcy_vec_download; what: "upload" / "download"
template <class C>
int check_vec_transfer(const C* c, const char* what, int vec, const double* host, int64_t n) {
    FEMCY_TRY(check_vec(c, vec));
    FEMCY_REQUIRE(host && n == c->n, "%s length %lld != n = %lld", what, (long long)n, (long long)c->n);
    return FEMCY_OK;
}

// femcy_vec_scatter with k != 0 (k = 0 is a valid no-op)
template <class C>
int check_vec_scatter(const C* c, const int32_t* idx, const double* vals, int32_t k) {
    FEMCY_REQUIRE(idx && vals && k > 0, "bad scatter arguments");
    for (int32_t i = 0; i < k; ++i) FEMCY_REQUIRE(idx[i] >= 0 && idx[i] < c->n, "scatter index %d out of range", idx[i]);
    return FEMCY_OK;
}

// ------------------------------------------------------------------------------------------ Dirichlet, DOF sets
template <class C>
int check_constrained_dofs(const C* c, const int32_t* dofs, int32_t k) {
    for (int32_t i = 0; i < k; ++i) FEMCY_REQUIRE(dofs[i] >= 0 && dofs[i] < c->n, "constrained DOF %d out of range", dofs[i]);
    return FEMCY_OK;
}

// femcy_apply_dirichlet_linear after the vector check (k = 0 is valid: on several ranks the elimination is collective)
template <class C>
int check_dirichlet_linear(const C* c, const int32_t* dofs, const double* vals, int32_t k, int rhs_vec) {
    FEMCY_REQUIRE(k >= 0 && (k == 0 || (dofs && vals)), "bad Dirichlet arguments");
    FEMCY_TRY(check_rhs_not_scratch(rhs_vec));
    return check_constrained_dofs(c, dofs, k);
}

// femcy_apply_dirichlet_newton with k != 0
template <class C>
int check_dirichlet_newton(const C* c, const int32_t* dofs, int32_t k) {
    FEMCY_REQUIRE(dofs && k > 0, "bad Dirichlet arguments");
    return check_constrained_dofs(c, dofs, k);
}

template <class C>
int check_dofset_create(const C* c, const int32_t* dofs, int32_t k, const int32_t* id_out) {
    FEMCY_REQUIRE(c->have_mesh && id_out && k >= 0 && (k == 0 || dofs), "bad dofset arguments");
    for (int32_t i = 0; i < k; ++i) FEMCY_REQUIRE(dofs[i] >= 0 && dofs[i] < c->n, "DOF %d out of range", dofs[i]);
    return FEMCY_OK;
}

// ------------------------------------------------------------------------------------------ loads
template <class C>
int check_loadset_create(const C* c, int32_t nft, int32_t nfn, int32_t nip, const int32_t* ft_nodes, const double* ft_N,
                         const double* ft_dN, const double* ft_normal, const double* ft_weight, int32_t nload,
                         const int32_t* load_elem, const int32_t* load_ft, const int32_t* id_out) {
    FEMCY_REQUIRE(c->have_mesh && id_out, "mesh not set or null id_out");
    FEMCY_REQUIRE(nft > 0 && nip > 0 && nfn >= c->dm && nfn <= c->npe, "bad facet table sizes (nft %d, nfn %d, nip %d)", nft, nfn, nip);
    FEMCY_REQUIRE(ft_nodes && ft_N && ft_dN && ft_normal && ft_weight, "null facet tables");
    FEMCY_REQUIRE(nload >= 0 && (nload == 0 || (load_elem && load_ft)), "bad load facet lists");
    for (int32_t i = 0; i < nft * nfn; ++i)
        FEMCY_REQUIRE(ft_nodes[i] >= 0 && ft_nodes[i] < c->npe, "facet table: local node %d out of range", ft_nodes[i]);
    for (int32_t l = 0; l < nload; ++l) {
        FEMCY_REQUIRE(load_elem[l] >= 0 && load_elem[l] < c->ne, "load facet %d: element %d out of range", l, load_elem[l]);
        FEMCY_REQUIRE(load_ft[l] >= 0 && load_ft[l] < nft, "load facet %d: facet type %d out of range", l, load_ft[l]);
    }
    return FEMCY_OK;
}

// the state femcy_bodyload_create, femcy_mass_create and femcy_lumped_mass_create need; entry: the caller's name
template <class C>
int check_mesh_element_pattern(const C* c, const char* entry) {
    FEMCY_REQUIRE(c->have_mesh && c->have_element && c->have_pattern,
                  "%s needs the mesh, the element tables and the pattern (mesh=%d element=%d pattern=%d)", entry,
                  (int)c->have_mesh, (int)c->have_element, (int)c->have_pattern);
    return FEMCY_OK;
}

// ... and mask [ne] = 1 on the selected elements (left empty when sel_elems is null: every element)
template <class C>
int check_bodyload_create(const C* c, const double* N, int32_t nsel, const int32_t* sel_elems, const int32_t* id_out,
                          std::vector<uint8_t>& mask) {
    FEMCY_TRY(check_mesh_element_pattern(c, "femcy_bodyload_create"));
    FEMCY_REQUIRE(N && id_out, "null shape-function table or id_out");
    FEMCY_REQUIRE(sel_elems ? nsel >= 0 : true, "negative selection size %d", nsel);
    if (!sel_elems) return FEMCY_OK;
    mask.assign((size_t)c->ne, 0);
    for (int32_t i = 0; i < nsel; ++i) {
        FEMCY_REQUIRE(sel_elems[i] >= 0 && sel_elems[i] < c->ne, "body load: element %d out of range", sel_elems[i]);
        FEMCY_REQUIRE(!mask[sel_elems[i]], "body load: element %d selected twice", sel_elems[i]);
        mask[sel_elems[i]] = 1;
    }
    return FEMCY_OK;
}

template <class C>
int check_bodyload_apply(const C* c, int32_t id, const double* b, int rhs_vec) {
    FEMCY_TRY(check_vec(c, rhs_vec));
    FEMCY_TRY(check_object(c->bodyloads, id, "body load"));
    FEMCY_REQUIRE(b, "null force");
    return FEMCY_OK;
}

template <class C>
int check_thermal_create(const C* c, const double* N, double alpha, const double* dT, const int32_t* id_out) {
    FEMCY_REQUIRE(c->have_mesh && c->have_element && c->have_material && c->have_pattern,
                  "femcy_thermal_create needs the mesh, the element tables, the material and the pattern (mesh=%d element=%d "
                  "material=%d pattern=%d)", (int)c->have_mesh, (int)c->have_element, (int)c->have_material,
                  (int)c->have_pattern);
    FEMCY_REQUIRE(N && dT && id_out, "null shape-function table, temperature field or id_out");
    FEMCY_REQUIRE(std::isfinite(alpha), "thermal load: the expansion coefficient is not finite");
    FEMCY_REQUIRE(c->mat_kind != FEMCY_MAT_NEOHOOKE, "thermal load: a neo-Hookean material has no small-strain thermal "
                  "stress (linear materials only)");
    return FEMCY_OK;
}

template <class C>
int check_thermal_stress(const C* c, int32_t id) {
    FEMCY_TRY(check_object(c->thermals, id, "thermal load"));
    FEMCY_REQUIRE(c->mat_kind != FEMCY_MAT_NEOHOOKE, "thermal stress: a neo-Hookean material has no small-strain thermal "
                  "stress (linear materials only)");
    FEMCY_REQUIRE(c->post_small, "femcy_thermal_stress corrects the stress of femcy_compute_strain_stress(large = 0): call "
                  "that first (the Gauss-point stress does not exist, is the nlgeom one, or has been corrected already)");
    return FEMCY_OK;
}

// ------------------------------------------------------------------------------------------ implicit dynamics
// femcy_mass_create and femcy_lumped_mass_create; entry: the caller's name
template <class C>
int check_mass_rule(const C* c, const char* entry, int32_t nq, const double* Nq, const double* dNq, const double* wq,
                    double rho, const int32_t* id_out) {
    FEMCY_TRY(check_mesh_element_pattern(c, entry));
    FEMCY_REQUIRE(Nq && dNq && wq && id_out, "null mass-rule table or id_out");
    FEMCY_REQUIRE(nq >= 1 && nq <= 64, "mass rule: %d points (1 .. 64 are supported)", nq);
    FEMCY_REQUIRE(std::isfinite(rho) && rho > 0.0, "mass: the density must be finite and positive");
    return FEMCY_OK;
}

template <class C>
int check_mass_apply(const C* c, int32_t id, int x_vec, int y_vec) {
    FEMCY_TRY(check_vec(c, x_vec));
    FEMCY_TRY(check_vec(c, y_vec));
    FEMCY_TRY(check_object(c->masses, id, "mass object"));
    FEMCY_REQUIRE(x_vec != y_vec, "the mass product cannot run in place");
    return FEMCY_OK;
}

template <class C>
int check_mass_add_to_K(const C* c, int32_t id, double cc) {
    FEMCY_TRY(check_object(c->masses, id, "mass object"));
    FEMCY_REQUIRE(std::isfinite(cc), "femcy_mass_add_to_K: the factor is not finite");
    return FEMCY_OK;
}

template <class C>
int check_newmark_predict(const C* c, int u_vec, int v_vec, int a_vec, int out_vec) {
    FEMCY_TRY(check_vec(c, u_vec));
    FEMCY_TRY(check_vec(c, v_vec));
    FEMCY_TRY(check_vec(c, a_vec));
    FEMCY_TRY(check_vec(c, out_vec));
    FEMCY_REQUIRE(out_vec != u_vec && out_vec != v_vec && out_vec != a_vec,
                  "femcy_newmark_predict: the output may not be one of the inputs");
    return FEMCY_OK;
}

template <class C>
int check_newmark_update(const C* c, int u_new_vec, int u_vec, int v_vec, int a_vec, double beta, double gamma, double dt) {
    FEMCY_TRY(check_vec(c, u_new_vec));
    FEMCY_TRY(check_vec(c, u_vec));
    FEMCY_TRY(check_vec(c, v_vec));
    FEMCY_TRY(check_vec(c, a_vec));
    FEMCY_REQUIRE(std::isfinite(beta) && beta > 0.0 && std::isfinite(gamma) && std::isfinite(dt) && dt > 0.0,
                  "femcy_newmark_update: beta and dt must be positive, gamma finite");
    FEMCY_REQUIRE(v_vec != a_vec && v_vec != u_vec && v_vec != u_new_vec && a_vec != u_vec && a_vec != u_new_vec,
                  "femcy_newmark_update: velocity and acceleration are written in place and may alias nothing");
    return FEMCY_OK;
}

// ------------------------------------------------------------------------------------------ explicit dynamics
template <class C>
int check_explicit_create(const C* c, int32_t lumped_id, int32_t ndofsets, const int32_t* dofset_ids, const int32_t* id_out) {
    FEMCY_TRY(check_object(c->lumped_masses, lumped_id, "lumped mass"));
    FEMCY_REQUIRE(id_out && ndofsets >= 0 && (ndofsets == 0 || dofset_ids), "femcy_explicit_create: null id_out or DOF-set list");
    for (int32_t k = 0; k < ndofsets; ++k) FEMCY_TRY(check_object(c->dofsets, dofset_ids[k], "DOF set"));
    return FEMCY_OK;
}

// femcy_lumped_mass_scale, after the state check (the estimate reads the element tables and the material)
template <class C>
int check_lumped_mass_scale(const C* c, int32_t lumped_id, double s_C, double factor, double dt, int32_t type,
                            const double* mass_before, const double* mass_after, const int64_t* n_scaled,
                            const double* factor_max) {
    FEMCY_TRY(check_object(c->lumped_masses, lumped_id, "lumped mass"));
    FEMCY_REQUIRE(mass_before && mass_after && n_scaled && factor_max, TEXT_NULL_OUTPUT);
    FEMCY_REQUIRE(std::isfinite(factor) && factor >= 0.0 && std::isfinite(dt) && dt >= 0.0,
                  "femcy_lumped_mass_scale: factor and dt must be finite and not negative");
    FEMCY_REQUIRE(factor != 0.0 || dt != 0.0, "femcy_lumped_mass_scale: give a factor, a target increment dt or both");
    FEMCY_REQUIRE(type == FEMCY_MS_BELOW_MIN || type == FEMCY_MS_SET_EQUAL_DT || type == FEMCY_MS_UNIFORM,
                  "femcy_lumped_mass_scale: unknown type %d", (int)type);
    FEMCY_REQUIRE(dt == 0.0 || positive_finite(s_C),
                  "femcy_lumped_mass_scale: the material stiffness s_C must be finite and positive");
    for (size_t k = 0; k < c->explicits.size(); ++k)
        FEMCY_REQUIRE(c->explicits[k].lumped != lumped_id, "femcy_lumped_mass_scale: explicit integrator %d refers to lumped "
                      "mass %d; scale before femcy_explicit_create (its inverse mass is derived once)", (int)k, (int)lumped_id);
    return FEMCY_OK;
}

// the checks the stepping calls share: the integrator, and a load vector that is none of the three state vectors
template <class C>
int check_explicit_rhs(const C* c, const char* entry, int32_t id, int rhs_vec) {
    FEMCY_TRY(check_object(c->explicits, id, "explicit integrator"));
    FEMCY_TRY(check_vec(c, rhs_vec));
    FEMCY_REQUIRE(rhs_vec != FEMCY_VEC_DOF && rhs_vec != FEMCY_VEC_VEL && rhs_vec != FEMCY_VEC_ACC,
                  "%s: the load vector may not be one of the state vectors DOF, VEL, ACC", entry);
    return FEMCY_OK;
}

template <class C>
int check_explicit_set_damping(const C* c, int32_t id, double alpha, double b1, double b2, double M_d) {
    FEMCY_TRY(check_object(c->explicits, id, "explicit integrator"));
    auto ok = [](double x) { return std::isfinite(x) && x >= 0.0; };
    FEMCY_REQUIRE(ok(alpha) && ok(b1) && ok(b2) && ok(M_d),
                  "femcy_explicit_set_damping: alpha, b1, b2 and M_d must be finite and not negative");
    FEMCY_REQUIRE(M_d > 0.0 || (b1 == 0.0 && b2 == 0.0),
                  "femcy_explicit_set_damping: bulk viscosity needs a positive dilatational modulus M_d");
    return FEMCY_OK;
}

// femcy_amplitude_create: a known kind, 2 .. FEMCY_AMP_MAX_POINTS finite points, t strictly increasing
inline int check_amplitude_create(int32_t kind, int32_t npts, const double* t, const double* A, const int32_t* id_out) {
    FEMCY_REQUIRE(id_out && t && A, "femcy_amplitude_create: null id_out, t or A");
    FEMCY_REQUIRE(kind == FEMCY_AMP_TABULAR || kind == FEMCY_AMP_SMOOTH_STEP, "femcy_amplitude_create: unknown kind %d", (int)kind);
    FEMCY_REQUIRE(npts >= 2 && npts <= FEMCY_AMP_MAX_POINTS, "femcy_amplitude_create: %d points, 2 .. %d are taken", (int)npts,
                  FEMCY_AMP_MAX_POINTS);
    for (int32_t k = 0; k < npts; ++k)
        FEMCY_REQUIRE(std::isfinite(t[k]) && std::isfinite(A[k]), "femcy_amplitude_create: point %d is not finite", (int)k);
    for (int32_t k = 1; k < npts; ++k)
        FEMCY_REQUIRE(t[k] > t[k - 1], "femcy_amplitude_create: the times must be strictly increasing (point %d)", (int)k);
    return FEMCY_OK;
}

// femcy_explicit_set_motion: known objects, finite values, only sets the integrator holds (explicits[id].held: the DOF-set
// ids it was created with), at most FEMCY_MOTION_MAX_CURVES distinct curves
template <class C>
int check_explicit_set_motion(const C* c, int32_t id, int32_t nsets, const int32_t* dofset_ids, const double* values,
                              const int32_t* amplitude_ids) {
    FEMCY_TRY(check_object(c->explicits, id, "explicit integrator"));
    FEMCY_REQUIRE(nsets >= 0 && (nsets == 0 || (dofset_ids && values && amplitude_ids)),
                  "femcy_explicit_set_motion: null DOF-set, value or amplitude list");
    int32_t curves[FEMCY_MOTION_MAX_CURVES], ncurves = 0;
    for (int32_t k = 0; k < nsets; ++k) {
        FEMCY_TRY(check_object(c->dofsets, dofset_ids[k], "DOF set"));
        FEMCY_TRY(check_object(c->amplitudes, amplitude_ids[k], "amplitude"));
        FEMCY_REQUIRE(std::isfinite(values[k]), "femcy_explicit_set_motion: value %d is not finite", (int)k);
        bool held = false;
        for (int32_t h : c->explicits[id].held) held = held || h == dofset_ids[k];
        FEMCY_REQUIRE(held, "femcy_explicit_set_motion: DOF set %d is not one of the sets integrator %d holds "
                      "(femcy_explicit_create); only held DOFs can be moved", (int)dofset_ids[k], (int)id);
        int32_t j = 0;
        while (j < ncurves && curves[j] != amplitude_ids[k]) ++j;
        if (j == ncurves) {
            FEMCY_REQUIRE(ncurves < FEMCY_MOTION_MAX_CURVES, "femcy_explicit_set_motion: more than %d distinct amplitudes",
                          FEMCY_MOTION_MAX_CURVES);
            curves[ncurves++] = amplitude_ids[k];
        }
    }
    return FEMCY_OK;
}

// femcy_explicit_energy_get: a known integrator whose balance has been running since a start (energy_on: set by
// femcy_explicit_start / _auto_begin of an integrator with femcy_explicit_energy_enable(on != 0), cleared by on = 0)
template <class C>
int check_explicit_energy_get(const C* c, int32_t id, const double* out) {
    FEMCY_TRY(check_object(c->explicits, id, "explicit integrator"));
    FEMCY_REQUIRE(out, TEXT_NULL_OUTPUT);
    FEMCY_REQUIRE(c->explicits[id].energy_on, "femcy_explicit_energy_get: the energy balance of integrator %d is not running "
                  "(femcy_explicit_energy_enable, then femcy_explicit_start or femcy_explicit_auto_begin)", (int)id);
    return FEMCY_OK;
}

// femcy_explicit_set_wall: a known integrator, 0 .. FEMCY_WALL_MAX walls of finite entries, a normal that has a length, a
// positive penalty.  What both libraries then run on: the unit normal, d = n . point and kappa of every wall in `out` (W:
// ExplicitWalls of element_math.hpp), with the fused multiply-adds written out so that both round alike.  out is written
// only when everything holds.
template <class C, class W>
int check_explicit_set_wall(const C* c, int32_t id, int32_t nwalls, const double* point, const double* normal,
                            const double* kappa, W& out) {
    FEMCY_TRY(check_object(c->explicits, id, "explicit integrator"));
    FEMCY_REQUIRE(nwalls >= 0 && nwalls <= FEMCY_WALL_MAX, "femcy_explicit_set_wall: %d walls, 0 .. %d are taken", (int)nwalls,
                  FEMCY_WALL_MAX);
    FEMCY_REQUIRE(nwalls == 0 || (point && normal && kappa), "femcy_explicit_set_wall: null point, normal or kappa");
    W w{};
    w.n = nwalls;
    for (int32_t k = 0; k < nwalls; ++k) {
        double len2 = 0.0;
        for (int j = 0; j < c->dm; ++j) {
            const double pj = point[k * c->dm + j], nj = normal[k * c->dm + j];
            FEMCY_REQUIRE(std::isfinite(pj) && std::isfinite(nj), "femcy_explicit_set_wall: wall %d has an entry that is not finite",
                          (int)k);
            len2 = std::fma(nj, nj, len2);
        }
        const double len = std::sqrt(len2);
        FEMCY_REQUIRE(positive_finite(len), "femcy_explicit_set_wall: the normal of wall %d has no length", (int)k);
        FEMCY_REQUIRE(positive_finite(kappa[k]), "femcy_explicit_set_wall: the penalty of wall %d must be finite and positive",
                      (int)k);
        double d = 0.0;
        for (int j = 0; j < c->dm; ++j) {
            w.nrm[k][j] = normal[k * c->dm + j] / len;
            d = std::fma(w.nrm[k][j], point[k * c->dm + j], d);
        }
        w.d[k] = d;
        w.kappa[k] = kappa[k];
    }
    out = w;
    return FEMCY_OK;
}

// femcy_explicit_wall_get: a known integrator, one of the walls it has
template <class C>
int check_explicit_wall_get(const C* c, int32_t id, int32_t wall, const double* out) {
    FEMCY_TRY(check_object(c->explicits, id, "explicit integrator"));
    FEMCY_REQUIRE(out, TEXT_NULL_OUTPUT);
    FEMCY_REQUIRE(wall >= 0 && wall < c->explicits[id].walls.n, "femcy_explicit_wall_get: wall %d of integrator %d, which has %d "
                  "(femcy_explicit_set_wall)", (int)wall, (int)id, (int)c->explicits[id].walls.n);
    return FEMCY_OK;
}

template <class C>
int check_explicit_start(const C* c, int32_t id, int rhs_vec, double scale) {
    FEMCY_TRY(check_explicit_rhs(c, "femcy_explicit_start", id, rhs_vec));
    FEMCY_REQUIRE(std::isfinite(scale), "femcy_explicit_start: the load scale is not finite");
    return FEMCY_OK;
}

template <class C>
int check_explicit_advance(const C* c, int32_t id, int rhs_vec, int32_t nsteps, double dt, double scale0, double dscale) {
    FEMCY_TRY(check_explicit_rhs(c, "femcy_explicit_advance", id, rhs_vec));
    FEMCY_REQUIRE(nsteps >= 0, "femcy_explicit_advance: %d steps", nsteps);
    FEMCY_REQUIRE(std::isfinite(dt) && dt > 0.0, "femcy_explicit_advance: the increment must be finite and positive");
    FEMCY_REQUIRE(std::isfinite(scale0) && std::isfinite(dscale), "femcy_explicit_advance: the load scale is not finite");
    return FEMCY_OK;
}

template <class C>
int check_explicit_element_bound(const C* c, int32_t id, int u_vec, double s_C, const double* omega) {
    FEMCY_TRY(check_object(c->explicits, id, "explicit integrator"));
    FEMCY_TRY(check_vec(c, u_vec));
    FEMCY_REQUIRE(omega, TEXT_NULL_OUTPUT);
    FEMCY_REQUIRE(positive_finite(s_C), "femcy_explicit_element_bound: the material stiffness s_C must be finite and positive");
    return FEMCY_OK;
}

template <class C>
int check_explicit_auto_begin(const C* c, int32_t id, int rhs_vec, double s_C, double scale_factor, double T) {
    FEMCY_TRY(check_explicit_rhs(c, "femcy_explicit_auto_begin", id, rhs_vec));
    FEMCY_REQUIRE(positive_finite(s_C) && positive_finite(scale_factor) && positive_finite(T),
                  "femcy_explicit_auto_begin: s_C, the scale factor and T must be finite and positive");
    return FEMCY_OK;
}

template <class C>
int check_explicit_auto_advance(const C* c, int32_t id, int rhs_vec, int32_t nsteps) {
    FEMCY_TRY(check_explicit_rhs(c, "femcy_explicit_auto_advance", id, rhs_vec));
    FEMCY_REQUIRE(nsteps >= 0, "femcy_explicit_auto_advance: %d steps", nsteps);
    FEMCY_REQUIRE(c->explicits[id].auto_begun, "femcy_explicit_auto_advance before femcy_explicit_auto_begin");
    return FEMCY_OK;
}

template <class C>
int check_explicit_auto_state(const C* c, int32_t id, const double* t, const double* h_last, const double* h_min,
                              const int64_t* steps_done) {
    FEMCY_TRY(check_object(c->explicits, id, "explicit integrator"));
    FEMCY_REQUIRE(t && h_last && h_min && steps_done, TEXT_NULL_OUTPUT);
    FEMCY_REQUIRE(c->explicits[id].auto_begun, "femcy_explicit_auto_state before femcy_explicit_auto_begin");
    return FEMCY_OK;
}

// ------------------------------------------------------------------------------------------ solvers
// femcy_spmv, femcy_pcg, femcy_direct_solve: a pattern and two different vectors; in_place: what the entry says to x = y
template <class C>
int check_two_vectors(const C* c, int a_vec, int b_vec, const char* in_place) {
    FEMCY_REQUIRE(c->have_pattern, TEXT_PATTERN_NOT_BUILT);
    FEMCY_TRY(check_vec(c, a_vec));
    FEMCY_TRY(check_vec(c, b_vec));
    FEMCY_REQUIRE(a_vec != b_vec, "%s", in_place);
    return FEMCY_OK;
}
constexpr const char* TEXT_SPMV_IN_PLACE = "spmv cannot run in place";
constexpr const char* TEXT_PCG_IN_PLACE = "pcg: b and x must be different vectors";
constexpr const char* TEXT_DIRECT_IN_PLACE = "direct solve: b and x must be different vectors";

template <class C>
int check_direct_plan(const C* c, const femcy_direct_info* info) {
    FEMCY_REQUIRE(c->have_pattern, TEXT_PATTERN_NOT_BUILT);
    FEMCY_REQUIRE(info != nullptr, "femcy_direct_plan: info must not be null");
    return FEMCY_OK;
}

// ------------------------------------------------------------------------------------------ post-processing, inspection
template <class C>
int check_elastic_energy_small(const C* c, int u_vec, const double* total) {
    FEMCY_REQUIRE(c->have_mesh && c->have_element && c->have_material && total, TEXT_NOT_DEFINED);
    FEMCY_TRY(check_vec(c, u_vec));
    FEMCY_REQUIRE(c->mat_kind != FEMCY_MAT_NEOHOOKE, "femcy_elastic_energy_small: a neo-Hookean material has no small-strain "
                  "energy (linear materials only)");
    return FEMCY_OK;
}

// ... and *width = components per Gauss point of the field
template <class C>
int check_extrapolate(const C* c, int gp_field, int comp, const double* E, const double* out, int* width) {
    FEMCY_REQUIRE(c->have_element && E && out, "element tables not set or null arguments");
    switch (gp_field) {
        case FEMCY_GP_VOL: case FEMCY_GP_MISES: case FEMCY_GP_ENERGY: *width = 1; break;
        case FEMCY_GP_F: case FEMCY_GP_SIGMA: case FEMCY_GP_STRAIN: *width = c->dm * c->dm; break;
        default: set_error("field %d cannot be extrapolated", gp_field); return FEMCY_EINVAL;
    }
    FEMCY_REQUIRE(comp >= 0 && comp < *width, "component %d out of range for field %d", comp, gp_field);
    return FEMCY_OK;
}

template <class C>
int check_get_gp_field(const C* c, int which, const double* out) {
    FEMCY_REQUIRE(c->have_element && out, "element tables not set or null output");
    FEMCY_REQUIRE(which >= FEMCY_GP_DSDX && which <= FEMCY_GP_ENERGY, "unknown Gauss-point field %d", which);
    return FEMCY_OK;
}

}  // namespace femcy
#pragma GCC visibility pop
