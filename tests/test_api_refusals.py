"""What every entry point of include/femcy.h refuses, and with which words: one table of rows (name, prepare, call, status,
exact text), run on the host library and on the device library.  The rows go through the raw C ABI (ctx._call / ctx.lib
with ctypes arguments): the Context wrappers validate some arguments themselves and would hide the library's own check.
Every row is a call that returns before anything is allocated or launched; each group ends in valid calls on the context
the refusals left behind.  The meshes are single elements (loads_reference.single): the C3D4, and the CPS3 where dm = 2
matters; the state rows start from no mesh at all.

GROUPS is the table both libraries answered alike before the checks were shared (it passes on either library of the commit
before).  ADOPTED is apart from it: the two value ranges of femcy_set_option the host library took over from the device
library, which had them alone until then."""
import ctypes as C
import math
import subprocess
import sys

import numpy as np
import pytest

import loads_reference as lr
from femcy_amd import backend as be
from femcy_amd.material_zoo import LinearIsotropic, LinearIsotropicPlaneStress

EINVAL = -1
NAN, INF = math.nan, math.inf
P = be._ptr
NOT_READY = "context not fully defined (mesh=%d element=%d material=%d pattern=%d)"
NEEDS3 = "%s needs the mesh, the element tables and the pattern (mesh=%d element=%d pattern=%d)"
THERMAL_NEEDS = ("femcy_thermal_create needs the mesh, the element tables, the material and the pattern (mesh=%d "
                 "element=%d material=%d pattern=%d)")
NEO = "a neo-Hookean material has no small-strain"
STATE_VECS = "the load vector may not be one of the state vectors DOF, VEL, ACC"


def _i32(*v):
    return np.array(v, dtype=np.int32)


class Env:
    """the arrays a group's rows point into (kept alive here) and the ids of the objects its prepare steps made"""

    def __init__(self, etype):
        self.nodes, self.el, self.ELE, _ = lr.single(etype)
        self.nodes = be._f64(self.nodes)
        t = self.ELE.tables()
        self.nn, self.dm = self.nodes.shape
        self.npe, self.nGP, self.voigt = self.el.shape[1], int(t["nGP"]), int(t["voigt_kind"])
        self.n = self.nn * self.dm
        self.N, self.dN, self.w = be._f64(t["N"]), be._f64(t["dN"]), be._f64(t["w"])
        m = self.ELE.mass_tables()
        self.nq, self.Nq, self.dNq, self.wq = int(m["nq"]), m["Nq"], m["dNq"], m["wq"]
        self.ft = self.ELE.facet_tables()
        self.C6, self.par = np.eye(6).ravel().copy(), np.array([1.0, 0.01])
        self.buf = np.zeros(64)                    # an output nobody reads
        self.ibuf = np.zeros(64, dtype=np.int32)
        self.dT = np.ones(self.nn)
        self.out_i32, self.out_f64, self.out_i64 = C.c_int32(-7), C.c_double(), C.c_int64()
        self.ids = {}

    def id_out(self):
        return C.byref(self.out_i32)

    def f64_out(self):
        return C.byref(self.out_f64)


def _mesh(ctx, e):
    ctx.set_mesh(e.nodes, e.el)


def _element(ctx, e):
    ctx.set_element(e.ELE)


def _material(ctx, e):
    ctx.set_material(LinearIsotropic(2.0e5, 0.3) if e.dm == 3 else LinearIsotropicPlaneStress(2.0e5, 0.3))


def _pattern(ctx, e):
    ctx.build_pattern()


def _ready(ctx, e):
    for step in (_mesh, _element, _material, _pattern):
        step(ctx, e)


def _objects(ctx, e):
    """one object of every kind, id 0 each: the rows below ask for id 5 (or -1) and misuse id 0"""
    _ready(ctx, e)
    assert ctx.dofset([0, 1, 2]) == 0
    assert ctx.loadset(e.ELE, [0], [0]) == 0
    assert ctx.bodyload(e.ELE) == 0
    assert ctx.thermal(e.ELE, 1.2e-5, e.dT) == 0
    assert ctx.mass(e.ELE, 7.85e-3) == 0
    assert ctx.lumped_mass(e.ELE, 7.85e-3) == 0
    assert ctx.explicit(0, [0]) == 0


def _neo(ctx, e):
    ctx._call("femcy_set_material", 3, P(e.C6), P(e.par), 2)


def _null_ctx(name, *args):
    def call(ctx, e):
        rc = getattr(ctx.lib, name)(None, *args)
        if rc != 0:
            raise be.FemcyError(f"{name} -> {rc}: {ctx.lib.femcy_last_error().decode()}", status=rc)
    return call


def _c(name, args):
    """a row's call: args(e) -> the raw argument tuple"""
    return lambda ctx, e: ctx._call(name, *args(e))


def _loadset_args(e, **over):
    t = e.ft
    a = dict(nft=t["nft"], nfn=t["nfn"], nip=t["nip"], ft_nodes=P(t["ft_nodes"]), N=P(t["N"]), dN=P(t["dN"]),
             normal=P(t["normal"]), weight=P(t["weight"]), nload=1, elem=P(e.ids.setdefault("le", _i32(0))),
             lft=P(e.ids.setdefault("lf", _i32(0))), out=e.id_out())
    a.update(over)
    return tuple(a[k] for k in ("nft", "nfn", "nip", "ft_nodes", "N", "dN", "normal", "weight", "nload", "elem", "lft", "out"))


def _mass_rows(entry):
    """the argument checks femcy_mass_create and femcy_lumped_mass_create share"""
    def args(**over):
        def f(e):
            a = dict(nq=e.nq, Nq=P(e.Nq), dNq=P(e.dNq), wq=P(e.wq), rho=7.85e-3, out=e.id_out())
            a.update(over)
            return tuple(a[k] for k in ("nq", "Nq", "dNq", "wq", "rho", "out"))
        return f
    rows = [(f"{entry} null {k}", None, _c(entry, args(**{k: None})), EINVAL, "null mass-rule table or id_out")
            for k in ("Nq", "dNq", "wq", "out")]
    rows += [(f"{entry} nq={nq}", None, _c(entry, args(nq=nq)), EINVAL, f"mass rule: {nq} points (1 .. 64 are supported)")
             for nq in (0, 65)]
    rows += [(f"{entry} rho={rho}", None, _c(entry, args(rho=rho)), EINVAL, "mass: the density must be finite and positive")
             for rho in (NAN, INF, 0.0, -1.0)]
    return rows


def _group_null_context():
    z = C.c_void_p()
    calls = [("femcy_set_option", 7, 0), ("femcy_sync",), ("femcy_set_mesh", 1, 3, z, 1, 4, z),
             ("femcy_set_element", 1, z, z, 1), ("femcy_set_material", 0, z, z, 2), ("femcy_build_pattern",),
             ("femcy_vec_fill", 0, 0.0), ("femcy_vec_norm", 0, None), ("femcy_assemble_K", 0),
             ("femcy_dofset_create", z, 0, None), ("femcy_bodyload_weights", 0, z), ("femcy_thermal_apply", 0, 1.0, 1, 0),
             ("femcy_mass_apply", 0, 9, 1, 1.0, 0), ("femcy_newmark_predict", 0, 9, 10, 1, 1.0, 1.0, 1.0),
             ("femcy_lumped_mass_get", 0, z), ("femcy_explicit_advance", 0, 1, 1, 1.0, 1.0, 0.0),
             ("femcy_explicit_auto_state", 0, None, None, None, None), ("femcy_spmv", 0, 1),
             ("femcy_pcg", 1, 6, 1e-3, 0, None, None, None), ("femcy_direct_plan", None),
             ("femcy_compute_strain_stress", 0, 0), ("femcy_get_gp_field", 1, z), ("femcy_timing", None),
             ("femcy_comm_info", z, z, z)]
    rows = [(f"{c[0]} null context", None, _null_ctx(*c), EINVAL, "null context") for c in calls]

    def create_without_out(ctx, e):                         # returns before the library looks for a device
        rc = ctx.lib.femcy_ctx_create(0, None)
        raise be.FemcyError(f"femcy_ctx_create -> {rc}: {ctx.lib.femcy_last_error().decode()}", status=rc)
    rows.append(("femcy_ctx_create null out", None, create_without_out, EINVAL, "out is null"))
    return "null context", None, None, rows, lambda ctx, e: ctx.sync()


def _group_state():
    """from an empty context up to a complete one: what each entry says about the state it needs"""
    e = Env("C3D4")
    set_mesh = lambda **o: _c("femcy_set_mesh", lambda e: tuple(dict(dict(nn=e.nn, dm=3, nodes=P(e.nodes), ne=1, npe=4,
                                                                          el=P(e.el)), **o).values()))
    three = lambda name, m, el, p: NEEDS3 % (name, m, el, p)
    mass_args = lambda e: (e.nq, P(e.Nq), P(e.dNq), P(e.wq), 7.85e-3, e.id_out())
    rows = [
        ("set_element before the mesh", None, _c("femcy_set_element", lambda e: (e.nGP, P(e.dN), P(e.w), 1)), EINVAL,
         "femcy_set_mesh must come first"),
        ("set_material before the mesh", None, _c("femcy_set_material", lambda e: (0, P(e.C6), P(e.par), 2)), EINVAL,
         "femcy_set_mesh must come first"),
        ("build_pattern before the mesh", None, _c("femcy_build_pattern", lambda e: ()), EINVAL,
         "femcy_set_mesh must come first"),
        ("vector before the mesh", None, _c("femcy_vec_fill", lambda e: (0, 1.0)), EINVAL,
         "vectors are allocated by femcy_set_mesh; call it first"),
        ("vector id 11", None, _c("femcy_vec_fill", lambda e: (11, 1.0)), EINVAL, "vector id 11 out of range"),
        ("vector id -1", None, _c("femcy_vec_scale", lambda e: (-1, 1.0)), EINVAL, "vector id -1 out of range"),
        ("assemble_K on nothing", None, _c("femcy_assemble_K", lambda e: (0,)), EINVAL, NOT_READY % (0, 0, 0, 0)),
        ("dofset_create before the mesh", None, _c("femcy_dofset_create", lambda e: (P(e.ibuf), 1, e.id_out())), EINVAL,
         "bad dofset arguments"),
        ("loadset_create before the mesh", None, _c("femcy_loadset_create", _loadset_args), EINVAL,
         "mesh not set or null id_out"),
        ("bodyload_create on nothing", None, _c("femcy_bodyload_create", lambda e: (P(e.N), 0, None, e.id_out())), EINVAL,
         three("femcy_bodyload_create", 0, 0, 0)),
        ("thermal_create on nothing", None, _c("femcy_thermal_create", lambda e: (P(e.N), 1e-5, P(e.dT), e.id_out())),
         EINVAL, THERMAL_NEEDS % (0, 0, 0, 0)),
        ("mass_create on nothing", None, _c("femcy_mass_create", mass_args), EINVAL, three("femcy_mass_create", 0, 0, 0)),
        ("lumped_mass_create on nothing", None, _c("femcy_lumped_mass_create", mass_args), EINVAL,
         three("femcy_lumped_mass_create", 0, 0, 0)),
        ("spmv without a pattern", None, _c("femcy_spmv", lambda e: (0, 1)), EINVAL, "pattern not built"),
        ("pcg without a pattern", None, _c("femcy_pcg", lambda e: (1, 6, 1e-3, 0, None, None, None)), EINVAL,
         "pattern not built"),
        ("direct_solve without a pattern", None, _c("femcy_direct_solve", lambda e: (1, 6, None)), EINVAL, "pattern not built"),
        ("direct_plan without a pattern", None, _c("femcy_direct_plan", lambda e: (None,)), EINVAL, "pattern not built"),
        ("pattern_info without a pattern", None, _c("femcy_get_pattern_info", lambda e: (C.byref(be.PatternInfo()),)), EINVAL,
         "pattern not built"),
        ("node_order without a pattern", None, _c("femcy_get_node_order", lambda e: (None, None)), EINVAL, "pattern not built"),
        ("K_ell without a pattern", None, _c("femcy_get_K_ell", lambda e: (P(e.ibuf), P(e.buf))), EINVAL,
         "pattern not built or null outputs"),
        ("K_bsr without a pattern", None, _c("femcy_get_K_bsr", lambda e: (P(e.ibuf), P(e.ibuf), P(e.buf))), EINVAL,
         "pattern not built or null outputs"),
        ("strain_stress on nothing", None, _c("femcy_compute_strain_stress", lambda e: (0, 0)), EINVAL,
         "context not fully defined"),
        ("elastic_energy on nothing", None, _c("femcy_elastic_energy", lambda e: (0, e.f64_out())), EINVAL,
         "context not fully defined"),
        ("elastic_energy_small on nothing", None, _c("femcy_elastic_energy_small", lambda e: (0, e.f64_out())), EINVAL,
         "context not fully defined"),
        ("gp_field without element tables", None, _c("femcy_get_gp_field", lambda e: (1, P(e.buf))), EINVAL,
         "element tables not set or null output"),
        ("extrapolate without element tables", None, _c("femcy_extrapolate", lambda e: (1, 0, P(e.buf), P(e.buf))), EINVAL,
         "element tables not set or null arguments"),
        ("assembly_used before an assembly", None, _c("femcy_get_assembly_used", lambda e: (e.id_out(),)), EINVAL,
         "no assembly has run on this context"),
        ("assembly_used null", None, _c("femcy_get_assembly_used", lambda e: (None,)), EINVAL,
         "no assembly has run on this context"),
        # femcy_set_option: the range texts both libraries have, at the first value outside each end
        ("tangent 2", None, _c("femcy_set_option", lambda e: (be.OPT_TANGENT, 2)), EINVAL,
         "tangent: 0 (reference) or 1 (consistent)"),
        ("tangent -1", None, _c("femcy_set_option", lambda e: (be.OPT_TANGENT, -1)), EINVAL,
         "tangent: 0 (reference) or 1 (consistent)"),
        ("band limit below 1 MiB", None, _c("femcy_set_option", lambda e: (be.OPT_DIRECT_MAX_BYTES, (1 << 20) - 1)), EINVAL,
         "direct solve: the band limit must be at least 1 MiB"),
        ("unknown option", None, _c("femcy_set_option", lambda e: (9999, 0)), EINVAL, "unknown option 9999"),
        # femcy_set_mesh
        ("mesh null nodes", None, set_mesh(nodes=None), EINVAL, "null mesh arrays"),
        ("mesh null elements", None, set_mesh(el=None), EINVAL, "null mesh arrays"),
        ("mesh nn=0", None, set_mesh(nn=0), EINVAL, "empty mesh (nn=0, ne=1)"),
        ("mesh ne=0", None, set_mesh(ne=0), EINVAL, "empty mesh (nn=4, ne=0)"),
        ("mesh dm=1", None, set_mesh(dm=1), EINVAL, "dm must be 2 or 3, got 1"),
        ("mesh dm=4", None, set_mesh(dm=4), EINVAL, "dm must be 2 or 3, got 4"),
        ("mesh npe=1", None, set_mesh(npe=1), EINVAL, "npe out of range: 1"),
        ("mesh npe=28", None, set_mesh(npe=28), EINVAL, "npe out of range: 28"),
        ("mesh node out of range", None, set_mesh(nn=3), EINVAL, "element 0 references node 3 outside [0,3)"),
        # with the mesh
        ("element nGP=0", _mesh, _c("femcy_set_element", lambda e: (0, P(e.dN), P(e.w), 1)), EINVAL,
         "bad element tables (nGP=0)"),
        ("element nGP=65", None, _c("femcy_set_element", lambda e: (65, P(e.dN), P(e.w), 1)), EINVAL,
         "bad element tables (nGP=65)"),
        ("element null dN", None, _c("femcy_set_element", lambda e: (1, None, P(e.w), 1)), EINVAL, "bad element tables (nGP=1)"),
        ("element null w", None, _c("femcy_set_element", lambda e: (1, P(e.dN), None, 1)), EINVAL, "bad element tables (nGP=1)"),
        ("element voigt 2-D on dm=3", None, _c("femcy_set_element", lambda e: (1, P(e.dN), P(e.w), 0)), EINVAL,
         "voigt kind 0 does not match dm=3"),
        ("material null C", None, _c("femcy_set_material", lambda e: (0, None, P(e.par), 2)), EINVAL, "null C"),
        ("material kind 4", None, _c("femcy_set_material", lambda e: (4, P(e.C6), P(e.par), 2)), EINVAL,
         "unknown material kind 4"),
        ("material kind -1", None, _c("femcy_set_material", lambda e: (-1, P(e.C6), P(e.par), 2)), EINVAL,
         "unknown material kind -1"),
        ("material plane strain on dm=3", None, _c("femcy_set_material", lambda e: (1, P(e.C6), P(e.par), 2)), EINVAL,
         "material kind 1 does not match dm=3"),
        ("material one parameter", None, _c("femcy_set_material", lambda e: (0, P(e.C6), P(e.par), 1)), EINVAL,
         "material needs 2 parameters"),
        ("material null parameters", None, _c("femcy_set_material", lambda e: (0, P(e.C6), None, 2)), EINVAL,
         "material needs 2 parameters"),
        ("assemble_K with the mesh", None, _c("femcy_assemble_K", lambda e: (0,)), EINVAL, NOT_READY % (1, 0, 0, 0)),
        ("bodyload_create with the mesh", None, _c("femcy_bodyload_create", lambda e: (P(e.N), 0, None, e.id_out())), EINVAL,
         three("femcy_bodyload_create", 1, 0, 0)),
        ("internal_force with the element", _element, _c("femcy_internal_force", lambda e: (0, 3)), EINVAL,
         NOT_READY % (1, 1, 0, 0)),
        ("mass_create with the element", None, _c("femcy_mass_create", mass_args), EINVAL, three("femcy_mass_create", 1, 1, 0)),
        ("strain_stress without a material", None, _c("femcy_compute_strain_stress", lambda e: (0, 0)), EINVAL,
         "context not fully defined"),
        ("thermal_create without a material", _pattern,
         _c("femcy_thermal_create", lambda e: (P(e.N), 1e-5, P(e.dT), e.id_out())), EINVAL, THERMAL_NEEDS % (1, 1, 0, 1)),
        ("residual_and_K without a material", None, _c("femcy_residual_and_K", lambda e: (0, 3)), EINVAL,
         NOT_READY % (1, 1, 0, 1)),
        ("explicit_advance without a material", None, _c("femcy_explicit_advance", lambda e: (0, 1, 1, 1.0, 1.0, 0.0)), EINVAL,
         NOT_READY % (1, 1, 0, 1)),
        ("sorting window after the pattern", None, _c("femcy_set_option", lambda e: (be.OPT_SELL_SIGMA, 128)), EINVAL,
         "set the sorting window before femcy_build_pattern"),
        ("node order after the pattern", None, _c("femcy_set_option", lambda e: (be.OPT_NODE_ORDER, 0)), EINVAL,
         "set the node order before femcy_build_pattern"),
    ]

    def valid(ctx, e):
        assert e.out_i32.value == -7                        # no refusal wrote an id
        _material(ctx, e)
        ctx.assemble_K(be.VEC_DOF)
        assert ctx.bodyload(e.ELE) == 0

    return "state", e, None, rows, valid


def _group_arguments():
    """a complete C3D4 context with one object of every kind"""
    e = Env("C3D4")
    n = e.n
    big = _i32(n)
    twice, beyond = _i32(0, 0), _i32(1)
    rows = [
        ("upload null", None, _c("femcy_vec_upload", lambda e: (0, None, n)), EINVAL, f"upload length {n} != n = {n}"),
        ("upload short", None, _c("femcy_vec_upload", lambda e: (0, P(e.buf), n - 1)), EINVAL,
         f"upload length {n - 1} != n = {n}"),
        ("download null", None, _c("femcy_vec_download", lambda e: (0, None, n)), EINVAL, f"download length {n} != n = {n}"),
        ("download long", None, _c("femcy_vec_download", lambda e: (0, P(e.buf), n + 1)), EINVAL,
         f"download length {n + 1} != n = {n}"),
        ("upload vector id", None, _c("femcy_vec_upload", lambda e: (11, P(e.buf), n)), EINVAL, "vector id 11 out of range"),
        ("scatter k=-1", None, _c("femcy_vec_scatter", lambda e: (0, P(e.ibuf), P(e.buf), -1)), EINVAL, "bad scatter arguments"),
        ("scatter null idx", None, _c("femcy_vec_scatter", lambda e: (0, None, P(e.buf), 1)), EINVAL, "bad scatter arguments"),
        ("scatter null values", None, _c("femcy_vec_scatter", lambda e: (0, P(e.ibuf), None, 1)), EINVAL, "bad scatter arguments"),
        ("scatter index n", None, _c("femcy_vec_scatter", lambda e: (0, P(big), P(e.buf), 1)), EINVAL,
         f"scatter index {n} out of range"),
        ("vec_norm null", None, _c("femcy_vec_norm", lambda e: (0, None)), EINVAL, "null output"),
        ("vec_absmax null", None, _c("femcy_vec_absmax", lambda e: (0, None)), EINVAL, "null output"),
        ("vec_sub vector id", None, _c("femcy_vec_sub", lambda e: (0, 1, 11)), EINVAL, "vector id 11 out of range"),
        ("vec_axpy vector id", None, _c("femcy_vec_axpy", lambda e: (0, -1, 1.0, 1)), EINVAL, "vector id -1 out of range"),
        ("assemble_K vector id", None, _c("femcy_assemble_K", lambda e: (11,)), EINVAL, "vector id 11 out of range"),
        ("internal_force vector id", None, _c("femcy_internal_force", lambda e: (0, 11)), EINVAL, "vector id 11 out of range"),
        # Dirichlet
        ("dirichlet_linear null dofs", None, _c("femcy_apply_dirichlet_linear", lambda e: (None, P(e.buf), 1, 1)), EINVAL,
         "bad Dirichlet arguments"),
        ("dirichlet_linear null values", None, _c("femcy_apply_dirichlet_linear", lambda e: (P(e.ibuf), None, 1, 1)), EINVAL,
         "bad Dirichlet arguments"),
        ("dirichlet_linear k=-1", None, _c("femcy_apply_dirichlet_linear", lambda e: (P(e.ibuf), P(e.buf), -1, 1)), EINVAL,
         "bad Dirichlet arguments"),
        ("dirichlet_linear rhs TMP0", None, _c("femcy_apply_dirichlet_linear", lambda e: (P(e.ibuf), P(e.buf), 1, 7)), EINVAL,
         "rhs may not alias the scratch vectors"),
        ("dirichlet_linear dof n", None, _c("femcy_apply_dirichlet_linear", lambda e: (P(big), P(e.buf), 1, 1)), EINVAL,
         f"constrained DOF {n} out of range"),
        ("dirichlet_newton null dofs", None, _c("femcy_apply_dirichlet_newton", lambda e: (None, 1, 2)), EINVAL,
         "bad Dirichlet arguments"),
        ("dirichlet_newton k=-1", None, _c("femcy_apply_dirichlet_newton", lambda e: (P(e.ibuf), -1, 2)), EINVAL,
         "bad Dirichlet arguments"),
        ("dirichlet_newton dof n", None, _c("femcy_apply_dirichlet_newton", lambda e: (P(big), 1, 2)), EINVAL,
         f"constrained DOF {n} out of range"),
        ("dofset_create null id_out", None, _c("femcy_dofset_create", lambda e: (P(e.ibuf), 1, None)), EINVAL,
         "bad dofset arguments"),
        ("dofset_create k=-1", None, _c("femcy_dofset_create", lambda e: (P(e.ibuf), -1, e.id_out())), EINVAL,
         "bad dofset arguments"),
        ("dofset_create null dofs", None, _c("femcy_dofset_create", lambda e: (None, 1, e.id_out())), EINVAL,
         "bad dofset arguments"),
        ("dofset_create dof n", None, _c("femcy_dofset_create", lambda e: (P(big), 1, e.id_out())), EINVAL,
         f"DOF {n} out of range"),
        ("dofset_fill unknown", None, _c("femcy_dofset_fill", lambda e: (5, 0, 1.0)), EINVAL, "unknown dofset 5"),
        ("dofset_add unknown", None, _c("femcy_dofset_add", lambda e: (-1, 0, 1.0)), EINVAL, "unknown dofset -1"),
        ("dofset_newton unknown", None, _c("femcy_dofset_dirichlet_newton", lambda e: (5, 2)), EINVAL, "unknown dofset 5"),
        ("dofset_linear unknown", None, _c("femcy_dofset_dirichlet_linear", lambda e: (5, 0.0, 1)), EINVAL, "unknown dofset 5"),
        ("dofset_linear rhs TMP1", None, _c("femcy_dofset_dirichlet_linear", lambda e: (0, 0.0, 8)), EINVAL,
         "rhs may not alias the scratch vectors"),
        ("dofset_scatter null values", None, _c("femcy_dofset_scatter", lambda e: (0, 0, None)), EINVAL, "null values"),
        ("dofset_scatter vector id", None, _c("femcy_dofset_scatter", lambda e: (0, 11, P(e.buf))), EINVAL,
         "vector id 11 out of range"),
        # load sets
        ("loadset null id_out", None, _c("femcy_loadset_create", lambda e: _loadset_args(e, out=None)), EINVAL,
         "mesh not set or null id_out"),
        ("loadset nft=0", None, _c("femcy_loadset_create", lambda e: _loadset_args(e, nft=0)), EINVAL,
         "bad facet table sizes (nft 0, nfn 3, nip %d)" % e.ft["nip"]),
        ("loadset nip=0", None, _c("femcy_loadset_create", lambda e: _loadset_args(e, nip=0)), EINVAL,
         "bad facet table sizes (nft 4, nfn 3, nip 0)"),
        ("loadset nfn below dm", None, _c("femcy_loadset_create", lambda e: _loadset_args(e, nfn=2)), EINVAL,
         "bad facet table sizes (nft 4, nfn 2, nip %d)" % e.ft["nip"]),
        ("loadset nfn above npe", None, _c("femcy_loadset_create", lambda e: _loadset_args(e, nfn=5)), EINVAL,
         "bad facet table sizes (nft 4, nfn 5, nip %d)" % e.ft["nip"]),
        *[(f"loadset null {k}", None, _c("femcy_loadset_create", lambda e, k=k: _loadset_args(e, **{k: None})), EINVAL,
           "null facet tables") for k in ("ft_nodes", "N", "dN", "normal", "weight")],
        ("loadset nload=-1", None, _c("femcy_loadset_create", lambda e: _loadset_args(e, nload=-1)), EINVAL,
         "bad load facet lists"),
        ("loadset null element list", None, _c("femcy_loadset_create", lambda e: _loadset_args(e, elem=None)), EINVAL,
         "bad load facet lists"),
        ("loadset null facet list", None, _c("femcy_loadset_create", lambda e: _loadset_args(e, lft=None)), EINVAL,
         "bad load facet lists"),
        ("loadset local node 4", None,
         _c("femcy_loadset_create", lambda e: _loadset_args(e, nft=1, ft_nodes=P(e.ids.setdefault("bad_ft", _i32(0, 1, 4))))),
         EINVAL, "facet table: local node 4 out of range"),
        ("loadset element 1", None, _c("femcy_loadset_create", lambda e: _loadset_args(e, elem=P(beyond))), EINVAL,
         "load facet 0: element 1 out of range"),
        ("loadset facet type 4", None, _c("femcy_loadset_create", lambda e: _loadset_args(e, lft=P(e.ids.setdefault("f4", _i32(4))))),
         EINVAL, "load facet 0: facet type 4 out of range"),
        ("neumann unknown", None, _c("femcy_loadset_neumann", lambda e: (5, 1.0, None, 1)), EINVAL, "unknown load set 5"),
        ("neumann_add unknown", None, _c("femcy_loadset_neumann_add", lambda e: (-1, 1.0, None, 1)), EINVAL,
         "unknown load set -1"),
        ("neumann vector id", None, _c("femcy_loadset_neumann", lambda e: (0, 1.0, None, 11)), EINVAL,
         "vector id 11 out of range"),
        # body loads
        ("bodyload null N", None, _c("femcy_bodyload_create", lambda e: (None, 0, None, e.id_out())), EINVAL,
         "null shape-function table or id_out"),
        ("bodyload null id_out", None, _c("femcy_bodyload_create", lambda e: (P(e.N), 0, None, None)), EINVAL,
         "null shape-function table or id_out"),
        ("bodyload nsel=-1", None, _c("femcy_bodyload_create", lambda e: (P(e.N), -1, P(twice), e.id_out())), EINVAL,
         "negative selection size -1"),
        ("bodyload element 1", None, _c("femcy_bodyload_create", lambda e: (P(e.N), 1, P(beyond), e.id_out())), EINVAL,
         "body load: element 1 out of range"),
        ("bodyload element -1", None,
         _c("femcy_bodyload_create", lambda e: (P(e.N), 1, P(e.ids.setdefault("m1", _i32(-1))), e.id_out())), EINVAL,
         "body load: element -1 out of range"),
        ("bodyload element twice", None, _c("femcy_bodyload_create", lambda e: (P(e.N), 2, P(twice), e.id_out())), EINVAL,
         "body load: element 0 selected twice"),
        ("bodyload_weights unknown", None, _c("femcy_bodyload_weights", lambda e: (5, P(e.buf))), EINVAL, "unknown body load 5"),
        ("bodyload_weights null", None, _c("femcy_bodyload_weights", lambda e: (0, None)), EINVAL, "null output"),
        ("bodyload_apply unknown", None, _c("femcy_bodyload_apply", lambda e: (-1, P(e.buf), 1, 0)), EINVAL,
         "unknown body load -1"),
        ("bodyload_apply null force", None, _c("femcy_bodyload_apply", lambda e: (0, None, 1, 0)), EINVAL, "null force"),
        ("bodyload_apply vector id", None, _c("femcy_bodyload_apply", lambda e: (0, P(e.buf), 11, 0)), EINVAL,
         "vector id 11 out of range"),
        # thermal loads
        *[(f"thermal null {k}", None, _c("femcy_thermal_create", lambda e, k=k: tuple(
            dict(dict(N=P(e.N), alpha=1e-5, dT=P(e.dT), out=e.id_out()), **{k: None}).values())), EINVAL,
           "null shape-function table, temperature field or id_out") for k in ("N", "dT", "out")],
        *[(f"thermal alpha={a}", None, _c("femcy_thermal_create", lambda e, a=a: (P(e.N), a, P(e.dT), e.id_out())), EINVAL,
           "thermal load: the expansion coefficient is not finite") for a in (NAN, INF, -INF)],
        ("thermal_force unknown", None, _c("femcy_thermal_force", lambda e: (5, P(e.buf))), EINVAL, "unknown thermal load 5"),
        ("thermal_force null", None, _c("femcy_thermal_force", lambda e: (0, None)), EINVAL, "null output"),
        ("thermal_apply unknown", None, _c("femcy_thermal_apply", lambda e: (5, 1.0, 1, 0)), EINVAL, "unknown thermal load 5"),
        ("thermal_apply vector id", None, _c("femcy_thermal_apply", lambda e: (0, 1.0, 11, 0)), EINVAL,
         "vector id 11 out of range"),
        ("thermal_stress unknown", None, _c("femcy_thermal_stress", lambda e: (5, 1.0)), EINVAL, "unknown thermal load 5"),
        ("thermal_stress without the small-strain stress", None, _c("femcy_thermal_stress", lambda e: (0, 1.0)), EINVAL,
         "femcy_thermal_stress corrects the stress of femcy_compute_strain_stress(large = 0): call that first (the "
         "Gauss-point stress does not exist, is the nlgeom one, or has been corrected already)"),
        # consistent mass, Newmark
        *_mass_rows("femcy_mass_create"),
        ("mass_get unknown", None, _c("femcy_mass_get", lambda e: (5, P(e.buf))), EINVAL, "unknown mass object 5"),
        ("mass_get null", None, _c("femcy_mass_get", lambda e: (0, None)), EINVAL, "null output"),
        ("mass_apply unknown", None, _c("femcy_mass_apply", lambda e: (5, 9, 1, 1.0, 0)), EINVAL, "unknown mass object 5"),
        ("mass_apply in place", None, _c("femcy_mass_apply", lambda e: (0, 9, 9, 1.0, 0)), EINVAL,
         "the mass product cannot run in place"),
        ("mass_apply vector id", None, _c("femcy_mass_apply", lambda e: (0, 9, 11, 1.0, 0)), EINVAL, "vector id 11 out of range"),
        ("mass_add_to_K unknown", None, _c("femcy_mass_add_to_K", lambda e: (5, 1.0, 0)), EINVAL, "unknown mass object 5"),
        ("mass_add_to_K nan", None, _c("femcy_mass_add_to_K", lambda e: (0, NAN, 0)), EINVAL,
         "femcy_mass_add_to_K: the factor is not finite"),
        ("mass_add_to_K inf", None, _c("femcy_mass_add_to_K", lambda e: (0, INF, 0)), EINVAL,
         "femcy_mass_add_to_K: the factor is not finite"),
        ("mass_kinetic_energy unknown", None, _c("femcy_mass_kinetic_energy", lambda e: (5, 9, e.f64_out())), EINVAL,
         "unknown mass object 5"),
        ("mass_kinetic_energy null", None, _c("femcy_mass_kinetic_energy", lambda e: (0, 9, None)), EINVAL, "null output"),
        *[(f"newmark_predict out = input {k}", None,
           _c("femcy_newmark_predict", lambda e, k=k: (0, 9, 10, (0, 9, 10)[k], 1.0, 1.0, 1.0)), EINVAL,
           "femcy_newmark_predict: the output may not be one of the inputs") for k in range(3)],
        ("newmark_predict vector id", None, _c("femcy_newmark_predict", lambda e: (0, 9, 10, 11, 1.0, 1.0, 1.0)), EINVAL,
         "vector id 11 out of range"),
        *[(f"newmark_update {name}", None, _c("femcy_newmark_update", lambda e, a=a: (6, 0, 9, 10) + a), EINVAL,
           "femcy_newmark_update: beta and dt must be positive, gamma finite")
          for name, a in (("beta=0", (0.0, 0.5, 1.0)), ("beta=nan", (NAN, 0.5, 1.0)), ("gamma=inf", (0.25, INF, 1.0)),
                          ("dt=0", (0.25, 0.5, 0.0)), ("dt=nan", (0.25, 0.5, NAN)))],
        *[(f"newmark_update aliases {v}", None, _c("femcy_newmark_update", lambda e, v=v: v + (0.25, 0.5, 1.0)), EINVAL,
           "femcy_newmark_update: velocity and acceleration are written in place and may alias nothing")
          for v in ((6, 0, 9, 9), (6, 9, 9, 10), (9, 0, 9, 10), (6, 10, 9, 10), (10, 0, 9, 10))],
        # explicit dynamics
        *_mass_rows("femcy_lumped_mass_create"),
        ("lumped_mass_get unknown", None, _c("femcy_lumped_mass_get", lambda e: (5, P(e.buf))), EINVAL, "unknown lumped mass 5"),
        ("lumped_mass_get null", None, _c("femcy_lumped_mass_get", lambda e: (0, None)), EINVAL, "null output"),
        ("explicit_create unknown lumped mass", None, _c("femcy_explicit_create", lambda e: (5, 0, None, e.id_out())), EINVAL,
         "unknown lumped mass 5"),
        ("explicit_create null id_out", None, _c("femcy_explicit_create", lambda e: (0, 0, None, None)), EINVAL,
         "femcy_explicit_create: null id_out or DOF-set list"),
        ("explicit_create null list", None, _c("femcy_explicit_create", lambda e: (0, 1, None, e.id_out())), EINVAL,
         "femcy_explicit_create: null id_out or DOF-set list"),
        ("explicit_create ndofsets=-1", None, _c("femcy_explicit_create", lambda e: (0, -1, P(e.ibuf), e.id_out())), EINVAL,
         "femcy_explicit_create: null id_out or DOF-set list"),
        ("explicit_create unknown DOF set", None,
         _c("femcy_explicit_create", lambda e: (0, 1, P(e.ids.setdefault("d7", _i32(7))), e.id_out())), EINVAL,
         "unknown DOF set 7"),
        ("explicit_start unknown", None, _c("femcy_explicit_start", lambda e: (5, 1, 1.0)), EINVAL,
         "unknown explicit integrator 5"),
        ("explicit_start vector id", None, _c("femcy_explicit_start", lambda e: (0, 11, 1.0)), EINVAL, "vector id 11 out of range"),
        *[(f"explicit_start load in vector {v}", None, _c("femcy_explicit_start", lambda e, v=v: (0, v, 1.0)), EINVAL,
           "femcy_explicit_start: " + STATE_VECS) for v in (0, 9, 10)],
        ("explicit_start scale=nan", None, _c("femcy_explicit_start", lambda e: (0, 1, NAN)), EINVAL,
         "femcy_explicit_start: the load scale is not finite"),
        ("explicit_advance unknown", None, _c("femcy_explicit_advance", lambda e: (-1, 1, 1, 1.0, 1.0, 0.0)), EINVAL,
         "unknown explicit integrator -1"),
        ("explicit_advance load in DOF", None, _c("femcy_explicit_advance", lambda e: (0, 0, 1, 1.0, 1.0, 0.0)), EINVAL,
         "femcy_explicit_advance: " + STATE_VECS),
        ("explicit_advance nsteps=-1", None, _c("femcy_explicit_advance", lambda e: (0, 1, -1, 1.0, 1.0, 0.0)), EINVAL,
         "femcy_explicit_advance: -1 steps"),
        *[(f"explicit_advance dt={dt}", None, _c("femcy_explicit_advance", lambda e, dt=dt: (0, 1, 1, dt, 1.0, 0.0)), EINVAL,
           "femcy_explicit_advance: the increment must be finite and positive") for dt in (0.0, -1.0, NAN, INF)],
        ("explicit_advance scale0=nan", None, _c("femcy_explicit_advance", lambda e: (0, 1, 1, 1.0, NAN, 0.0)), EINVAL,
         "femcy_explicit_advance: the load scale is not finite"),
        ("explicit_advance dscale=inf", None, _c("femcy_explicit_advance", lambda e: (0, 1, 1, 1.0, 1.0, INF)), EINVAL,
         "femcy_explicit_advance: the load scale is not finite"),
        ("explicit_kinetic_energy unknown", None, _c("femcy_explicit_kinetic_energy", lambda e: (5, 9, e.f64_out())), EINVAL,
         "unknown explicit integrator 5"),
        ("explicit_kinetic_energy vector id", None, _c("femcy_explicit_kinetic_energy", lambda e: (0, 11, e.f64_out())),
         EINVAL, "vector id 11 out of range"),
        ("explicit_kinetic_energy null", None, _c("femcy_explicit_kinetic_energy", lambda e: (0, 9, None)), EINVAL,
         "null output"),
        ("stable_dt unknown", None, _c("femcy_explicit_stable_dt", lambda e: (5, e.f64_out(), e.f64_out())), EINVAL,
         "unknown explicit integrator 5"),
        ("stable_dt null dt", None, _c("femcy_explicit_stable_dt", lambda e: (0, None, e.f64_out())), EINVAL, "null output"),
        ("stable_dt null bound", None, _c("femcy_explicit_stable_dt", lambda e: (0, e.f64_out(), None)), EINVAL, "null output"),
        ("stable_dt before an assembly", None, _c("femcy_explicit_stable_dt", lambda e: (0, e.f64_out(), e.f64_out())), EINVAL,
         "femcy_explicit_stable_dt bounds the matrix of the last femcy_assemble_K: assemble first"),
        ("element_bound unknown", None, _c("femcy_explicit_element_bound", lambda e: (5, 0, 1.0, e.f64_out())), EINVAL,
         "unknown explicit integrator 5"),
        ("element_bound vector id", None, _c("femcy_explicit_element_bound", lambda e: (0, 11, 1.0, e.f64_out())), EINVAL,
         "vector id 11 out of range"),
        ("element_bound null", None, _c("femcy_explicit_element_bound", lambda e: (0, 0, 1.0, None)), EINVAL, "null output"),
        *[(f"element_bound s_C={s}", None, _c("femcy_explicit_element_bound", lambda e, s=s: (0, 0, s, e.f64_out())), EINVAL,
           "femcy_explicit_element_bound: the material stiffness s_C must be finite and positive")
          for s in (0.0, -1.0, NAN, INF)],
        ("auto_begin unknown", None, _c("femcy_explicit_auto_begin", lambda e: (5, 1, 1.0, 0.9, 1.0, 0)), EINVAL,
         "unknown explicit integrator 5"),
        ("auto_begin load in VEL", None, _c("femcy_explicit_auto_begin", lambda e: (0, 9, 1.0, 0.9, 1.0, 0)), EINVAL,
         "femcy_explicit_auto_begin: " + STATE_VECS),
        *[(f"auto_begin {name}", None, _c("femcy_explicit_auto_begin", lambda e, a=a: (0, 1) + a + (0,)), EINVAL,
           "femcy_explicit_auto_begin: s_C, the scale factor and T must be finite and positive")
          for name, a in (("s_C=0", (0.0, 0.9, 1.0)), ("s_C=nan", (NAN, 0.9, 1.0)), ("factor=0", (1.0, 0.0, 1.0)),
                          ("factor=inf", (1.0, INF, 1.0)), ("T=0", (1.0, 0.9, 0.0)), ("T=nan", (1.0, 0.9, NAN)))],
        ("auto_advance unknown", None, _c("femcy_explicit_auto_advance", lambda e: (5, 1, 1)), EINVAL,
         "unknown explicit integrator 5"),
        ("auto_advance load in ACC", None, _c("femcy_explicit_auto_advance", lambda e: (0, 10, 1)), EINVAL,
         "femcy_explicit_auto_advance: " + STATE_VECS),
        ("auto_advance nsteps=-1", None, _c("femcy_explicit_auto_advance", lambda e: (0, 1, -1)), EINVAL,
         "femcy_explicit_auto_advance: -1 steps"),
        ("auto_advance before auto_begin", None, _c("femcy_explicit_auto_advance", lambda e: (0, 1, 1)), EINVAL,
         "femcy_explicit_auto_advance before femcy_explicit_auto_begin"),
        ("auto_state unknown", None,
         _c("femcy_explicit_auto_state", lambda e: (5, e.f64_out(), e.f64_out(), e.f64_out(), C.byref(e.out_i64))), EINVAL,
         "unknown explicit integrator 5"),
        *[(f"auto_state null output {k}", None, _c("femcy_explicit_auto_state", lambda e, k=k: (0,) + tuple(
            None if j == k else (C.byref(e.out_i64) if j == 3 else e.f64_out()) for j in range(4))), EINVAL, "null output")
          for k in range(4)],
        ("auto_state before auto_begin", None,
         _c("femcy_explicit_auto_state", lambda e: (0, e.f64_out(), e.f64_out(), e.f64_out(), C.byref(e.out_i64))), EINVAL,
         "femcy_explicit_auto_state before femcy_explicit_auto_begin"),
        # solvers, post-processing, inspection
        ("spmv in place", None, _c("femcy_spmv", lambda e: (1, 1)), EINVAL, "spmv cannot run in place"),
        ("spmv vector id", None, _c("femcy_spmv", lambda e: (1, 11)), EINVAL, "vector id 11 out of range"),
        ("pcg b = x", None, _c("femcy_pcg", lambda e: (1, 1, 1e-3, 0, None, None, None)), EINVAL,
         "pcg: b and x must be different vectors"),
        ("direct_solve b = x", None, _c("femcy_direct_solve", lambda e: (1, 1, None)), EINVAL,
         "direct solve: b and x must be different vectors"),
        ("direct_plan null info", None, _c("femcy_direct_plan", lambda e: (None,)), EINVAL,
         "femcy_direct_plan: info must not be null"),
        ("pattern_info null", None, _c("femcy_get_pattern_info", lambda e: (None,)), EINVAL, "pattern not built"),
        ("elastic_energy null", None, _c("femcy_elastic_energy", lambda e: (0, None)), EINVAL, "context not fully defined"),
        ("elastic_energy_small null", None, _c("femcy_elastic_energy_small", lambda e: (0, None)), EINVAL,
         "context not fully defined"),
        ("strain_stress vector id", None, _c("femcy_compute_strain_stress", lambda e: (11, 0)), EINVAL,
         "vector id 11 out of range"),
        ("extrapolate null E", None, _c("femcy_extrapolate", lambda e: (1, 0, None, P(e.buf))), EINVAL,
         "element tables not set or null arguments"),
        ("extrapolate null out", None, _c("femcy_extrapolate", lambda e: (1, 0, P(e.buf), None)), EINVAL,
         "element tables not set or null arguments"),
        ("extrapolate the gradients", None, _c("femcy_extrapolate", lambda e: (0, 0, P(e.buf), P(e.buf))), EINVAL,
         "field 0 cannot be extrapolated"),
        ("extrapolate field 7", None, _c("femcy_extrapolate", lambda e: (7, 0, P(e.buf), P(e.buf))), EINVAL,
         "field 7 cannot be extrapolated"),
        ("extrapolate component 9 of F", None, _c("femcy_extrapolate", lambda e: (2, 9, P(e.buf), P(e.buf))), EINVAL,
         "component 9 out of range for field 2"),
        ("extrapolate component 1 of vol", None, _c("femcy_extrapolate", lambda e: (1, 1, P(e.buf), P(e.buf))), EINVAL,
         "component 1 out of range for field 1"),
        ("extrapolate component -1", None, _c("femcy_extrapolate", lambda e: (5, -1, P(e.buf), P(e.buf))), EINVAL,
         "component -1 out of range for field 5"),
        ("gp_field 7", None, _c("femcy_get_gp_field", lambda e: (7, P(e.buf))), EINVAL, "unknown Gauss-point field 7"),
        ("gp_field -1", None, _c("femcy_get_gp_field", lambda e: (-1, P(e.buf))), EINVAL, "unknown Gauss-point field -1"),
        ("gp_field null", None, _c("femcy_get_gp_field", lambda e: (1, None)), EINVAL, "element tables not set or null output"),
        ("K_ell null", None, _c("femcy_get_K_ell", lambda e: (None, P(e.buf))), EINVAL, "pattern not built or null outputs"),
        ("K_bsr null", None, _c("femcy_get_K_bsr", lambda e: (P(e.ibuf), None, P(e.buf))), EINVAL,
         "pattern not built or null outputs"),
        ("timing null", None, _c("femcy_timing", lambda e: (None,)), EINVAL, "null output"),
        ("persist_streamed_bytes null", None, _c("femcy_persist_streamed_bytes", lambda e: (None,)), EINVAL, "null output"),
    ]
    rows[0] = rows[0][:1] + (_objects,) + rows[0][2:]

    def valid(ctx, e):
        assert e.out_i32.value == -7                        # no refusal wrote an id
        assert ctx.dofset([3]) == 1 and ctx.bodyload(e.ELE, [0]) == 1 and ctx.mass(e.ELE, 1.0) == 1
        assert ctx.lumped_mass(e.ELE, 1.0) == 1 and ctx.explicit(1) == 1
        ctx.bodyload_apply(0, [0.0, 0.0, -9.81])
        ctx.thermal_apply(0, 1.0, be.VEC_FORCE)
        ctx.mass_apply(0, be.VEC_VEL, be.VEC_TMP0)
        ctx.loadset_neumann(0, 1.0, None, be.VEC_RESIDUAL)
        ctx.dofset_fill(0, be.VEC_DOF, 0.0)
        ctx.explicit_start(0, be.VEC_RHS, 1.0)
        assert np.all(np.isfinite(ctx.download(be.VEC_ACC)))
        ctx.compute_strain_stress(be.VEC_DOF, large=False)
        ctx.thermal_stress(0, 1.0)                          # ... which the refusal above did not use up

    return "arguments", e, None, rows, valid


def _group_neo_hookean():
    """a thermal load made with a linear material, then the material becomes neo-Hookean"""
    e = Env("C3D4")

    def prepare(ctx, e):
        _ready(ctx, e)
        assert ctx.thermal(e.ELE, 1.2e-5, e.dT) == 0
        ctx.compute_strain_stress(be.VEC_DOF, large=False)
        _neo(ctx, e)

    rows = [
        ("thermal_create", prepare, _c("femcy_thermal_create", lambda e: (P(e.N), 1e-5, P(e.dT), e.id_out())), EINVAL,
         f"thermal load: {NEO} thermal stress (linear materials only)"),
        ("thermal_stress", None, _c("femcy_thermal_stress", lambda e: (0, 1.0)), EINVAL,
         f"thermal stress: {NEO} thermal stress (linear materials only)"),
        ("elastic_energy_small", None, _c("femcy_elastic_energy_small", lambda e: (0, e.f64_out())), EINVAL,
         f"femcy_elastic_energy_small: {NEO} energy (linear materials only)"),
    ]

    def valid(ctx, e):
        assert np.isfinite(ctx.elastic_energy(be.VEC_DOF))
        _material(ctx, e)
        ctx.thermal_apply(0, 1.0)
        assert ctx.thermal(e.ELE, 1.2e-5, e.dT) == 1

    return "neo-Hookean", e, None, rows, valid


def _group_plane():
    """a single CPS3: the checks that read dm"""
    e = Env("CPS3")
    rows = [
        ("element voigt 3-D on dm=2", _mesh, _c("femcy_set_element", lambda e: (e.nGP, P(e.dN), P(e.w), 1)), EINVAL,
         "voigt kind 1 does not match dm=2"),
        ("material 3-D on dm=2", None, _c("femcy_set_material", lambda e: (0, P(e.C6), P(e.par), 2)), EINVAL,
         "material kind 0 does not match dm=2"),
        ("loadset nfn below dm", _ready, _c("femcy_loadset_create", lambda e: _loadset_args(e, nfn=1)), EINVAL,
         "bad facet table sizes (nft 3, nfn 1, nip %d)" % e.ft["nip"]),
        ("extrapolate component 4 of F", None, _c("femcy_extrapolate", lambda e: (2, 4, P(e.buf), P(e.buf))), EINVAL,
         "component 4 out of range for field 2"),
        ("dofset dof n", None, _c("femcy_dofset_create", lambda e: (P(e.ids.setdefault("n", _i32(e.n))), 1, e.id_out())), EINVAL,
         "DOF 6 out of range"),
    ]

    def valid(ctx, e):
        assert ctx.loadset(e.ELE, [0], [0]) == 0
        ctx.loadset_neumann(0, 1.0, [1.0, 0.0], be.VEC_RHS)
        ctx.assemble_K(be.VEC_DOF)

    return "plane", e, None, rows, valid


def _group_adopted_ranges():
    """femcy_set_option: the sorting window and the node order at the first value outside each end, before a pattern"""
    window, order = "sorting window must be in [64, 2^24] nodes", ("node order: 0 (caller's numbering), 1 (measured "
                                                                    "choice), 2..7 (coordinate order k - 2)")
    rows = [(f"option {opt} = {v}", None, _c("femcy_set_option", lambda e, opt=opt, v=v: (opt, v)), EINVAL, text)
            for opt, v, text in ((be.OPT_SELL_SIGMA, 63, window), (be.OPT_SELL_SIGMA, (1 << 24) + 1, window),
                                 (be.OPT_NODE_ORDER, -1, order), (be.OPT_NODE_ORDER, 8, order))]

    def valid(ctx, e):
        for opt, v in ((be.OPT_SELL_SIGMA, 64), (be.OPT_SELL_SIGMA, 1 << 24), (be.OPT_NODE_ORDER, 0), (be.OPT_NODE_ORDER, 7)):
            ctx.set_option(opt, v)

    return "adopted ranges", None, None, rows, valid


GROUPS = (_group_null_context, _group_state, _group_arguments, _group_neo_hookean, _group_plane)
ADOPTED = (_group_adopted_ranges,)


def _run_table(make, groups=GROUPS):
    for group in groups:
        gname, e, _, rows, valid = group()
        ctx = make()
        for name, prepare, call, status, text in rows:
            if prepare:
                prepare(ctx, e)
            with pytest.raises(be.FemcyError) as err:
                call(ctx, e)
            assert err.value.status == status, f"{gname} / {name}: {err.value}"
            assert str(err.value).endswith(f"-> {status}: {text}"), f"{gname} / {name}: {err.value}"
        valid(ctx, e)                                       # the context the refusals left behind is usable


def test_host_backend_refusals():
    made = []

    def make():
        made.append(be.Context(0, backend="cpu"))
        return made[-1]

    try:
        _run_table(make)
    finally:
        for c in made:
            c.close()


def test_host_backend_ranges_adopted_from_the_device():
    ctx = be.Context(0, backend="cpu")
    try:
        _run_table(lambda: ctx, ADOPTED)
    finally:
        ctx.close()


# Both libraries in one process, the device library first and with RTLD_GLOBAL as backend.load_library maps it: each keeps
# its own error buffer, so a refusal of one is read from that one and leaves the other's text alone.  A fresh process,
# because symbols are bound when a library is first loaded and called.  No call here reaches the HIP runtime.
_TWO_LIBRARIES = """
from femcy_amd import backend as be
hip = be.load_library(require_gpu_runtime=False, kind="hip")
cpu = be.load_library(kind="cpu")
assert cpu.femcy_set_option(None, 7, 0) == -1
assert (cpu.femcy_last_error(), hip.femcy_last_error()) == (b"null context", b""), (cpu.femcy_last_error(), hip.femcy_last_error())
assert hip.femcy_ctx_create(0, None) == -1
assert (cpu.femcy_last_error(), hip.femcy_last_error()) == (b"null context", b"out is null")
assert cpu.femcy_direct_plan(None, None) == -1 and cpu.femcy_ctx_create(1, None) == -1
assert (cpu.femcy_last_error(), hip.femcy_last_error()) == (b"out is null", b"out is null")
"""


def test_each_library_keeps_its_own_error_text_when_both_are_loaded():
    done = subprocess.run([sys.executable, "-c", _TWO_LIBRARIES], cwd=be._HERE + "/..", capture_output=True, text=True)
    assert done.returncode == 0, done.stderr


@pytest.mark.gpu
def test_device_refusals(gpu_ctx_factory):
    _run_table(gpu_ctx_factory)


@pytest.mark.gpu
def test_device_ranges_the_host_adopted(gpu_ctx_factory):
    _run_table(gpu_ctx_factory, ADOPTED)
