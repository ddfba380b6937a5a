"""Scenarios of fixed mass scaling (`*Fixed Mass Scaling`; femcy_lumped_mass_scale, femcy_lumped_mass_get_scaling), written
against the C ABI and the deck driver so that the host backend (tests/test_mass_scaling_cpu.py) and the device
(tests/test_gpu_mass_scaling.py) run the same code.

The reference is the numpy restatement below in np.longdouble, written from the rules: with omega_e^2 the element estimate of
explicit_auto_cases.Estimate at u = 0 from the element's current shares, f the factor and tau the target increment,

    f alone                k_e = f
    tau, below min         k_e = f max(1, (omega_e^2 / f) tau^2 / 4)
    tau, set equal dt      k_e = f (omega_e^2 / f) tau^2 / 4
    tau, uniform           k_e = f (max_e omega_e^2 / f) tau^2 / 4

m_a^e *= k_e, the nodal masses are the node sums of the shares, a second call compounds.  Bounds follow explicit_cases: the
same restatement in float64 differs from the long-double one by rounding alone, the F64_WORST_* constants are the worst such
differences on the cases run here (`measure_f64_worst`, asserted by tests/test_mass_scaling_cpu.py) and a backend is held to
4 x that.  Errors are relative to the largest entry of the reference.

Target increments.  `below min` counts the elements with k_e != 1, and an element whose own increment IS tau has
omega_e^2 tau^2 / 4 = 1 up to the last bit, which would decide whether it counts.  The meshes here hold groups of congruent
elements (ties), so tau is the midpoint of the gap between two neighbouring distinct increments that is nearest to the median
(`median_gap`), and `reference_call` asserts that no element is within 1e-6 of the threshold."""
import functools
import os

import numpy as np
import pytest

from femcy_amd import backend as be
from femcy_amd.material_zoo import LinearIsotropic
from femcy_amd.element_zoo import Element_linear_triangular

import explicit_auto_cases as ac
import explicit_cases as ec
import explicit_reference as er
import loads_cases as lc
import loads_reference as lr

LD = np.longdouble
EPS = ec.EPS
RHO = ec.RHO
TYPES = ("below min", "set equal dt", "uniform")
# worst error of the float64 restatement against the long-double one (measure_f64_worst, as measured on the CPU): factors,
# nodal masses, totals and the largest factor over every case of FACTOR_CASES and EDGE_CASES 2.38e-15; the increment
# recomputed after a call 3.73e-16; two calls 9.66e-16; the trajectories (u, v and the two energies at the records) of the
# denser-material pair 5.57e-14 (fixed) / 5.66e-14 (auto) and of the graded bar 1.82e-13 / 1.84e-13
F64_WORST_SCALE = 2.4e-15
F64_WORST_AFTER = 3.8e-16
F64_WORST_COMPOUND = 9.7e-16
F64_WORST_PAIR = {"fixed": 5.6e-14, "auto": 5.7e-14}
F64_WORST_GRADED = {"fixed": 1.9e-13, "auto": 1.9e-13}
SCALE_TOL, AFTER_TOL, COMPOUND_TOL = 4.0 * F64_WORST_SCALE, 4.0 * F64_WORST_AFTER, 4.0 * F64_WORST_COMPOUND


# ------------------------------------------------------------------------------------- the restatement
def factors(w2, factor, tau, kind, dtype):
    """k_e [ne] of one call from the elements' omega_e^2"""
    f = dtype(factor) if factor else dtype(1)
    if not tau:
        return np.full(len(w2), f, dtype=dtype)
    base = np.full(len(w2), w2.max(), dtype=dtype) if kind == "uniform" else w2
    r = (base / f) * (dtype(tau) * dtype(tau)) / 4
    return f * (np.maximum(dtype(1), r) if kind == "below min" else r)


class Reference:
    """the shares, factors and nodal masses of one mesh in one dtype, through any number of calls"""

    def __init__(self, nodes, el, ELE, material, rho, dtype):
        self.est = ac.Estimate(nodes, el, ELE, material, rho, dtype)
        self.el, self.nn, self.dtype = np.asarray(el), len(nodes), dtype
        self.k = np.ones(len(el), dtype=dtype)
        self.u0 = np.zeros(np.asarray(nodes).size)

    def w2(self):
        return self.est.elements(self.u0)[1]

    def nodal(self):
        m = np.zeros(self.nn, dtype=self.dtype)
        np.add.at(m, self.el, self.est.me)
        return m

    def scale(self, factor=None, tau=None, kind="below min"):
        m0 = self.nodal().sum()
        k = factors(self.w2(), factor, tau, kind, self.dtype)
        self.est.me = self.est.me * k[:, None]
        self.k = self.k * k
        return {"mass0": m0, "mass1": self.nodal().sum(), "scaled_elements": int((k != 1).sum()), "max_factor": k.max(), "k": k}


def median_gap(dte):
    """the midpoint of the gap between two distinct neighbouring increments nearest to the median (module docstring)"""
    s = np.sort(np.asarray(dte, dtype=LD))
    gaps = np.nonzero(s[1:] - s[:-1] > 1.0e-4 * s[:-1])[0]
    assert len(gaps), "the mesh has one increment only"
    i = gaps[np.argmin(np.abs(gaps - (len(s) - 1) / 2.0))]
    return float((s[i] + s[i + 1]) / 2)


def target(kind, w2, factor):
    """tau of a case from the long-double omega_e^2 (after the factor): below min the median gap (a mesh of ONE_INCREMENT:
    1.5 x that increment), set equal dt 0.8 x the smallest increment (every factor below 1), uniform 1.5 x the smallest"""
    dte = 2 / np.sqrt(w2 / LD(factor or 1.0))
    if kind == "below min":
        return median_gap(dte) if float(np.ptp(dte)) > 1.0e-4 * float(dte.min()) else float(1.5 * dte.min())
    return float((0.8 if kind == "set equal dt" else 1.5) * dte.min())


def relmax(got, want):
    want = np.asarray(want, dtype=LD)
    return float(np.abs(np.asarray(got, dtype=LD) - want).max() / np.abs(want).max())


def outputs_error(out, k, m, ref_out, ref):
    """worst relative error of what a call returns and leaves behind (factors cumulative, nodal masses) against a Reference"""
    return max(relmax(k, ref.k), relmax(m, ref.nodal()), relmax(out["mass0"], ref_out["mass0"]),
               relmax(out["mass1"], ref_out["mass1"]), relmax(out["max_factor"], ref_out["max_factor"]))


# -------------------------------------------------------------------------- meshes, factors and masses
def strip(ne, seed=5):
    """a strip of ne CPS3 triangles (ne / 2 cells of random width in [0.5, 1.5], ne odd: the last cell gives one) -- no two
    cells alike, so that the increments differ"""
    cells = (ne + 1) // 2
    x = np.concatenate([[0.0], np.cumsum(np.random.default_rng(seed).uniform(0.5, 1.5, cells))])
    nodes = np.array([[xi, y] for xi in x for y in (0.0, 1.0)])
    el = []
    for c in range(cells):
        a, b, d, e = 2 * c, 2 * c + 1, 2 * c + 2, 2 * c + 3
        el += [[a, d, b], [b, d, e]]
    return nodes, np.array(el[:ne], dtype=np.int32), Element_linear_triangular()


def sheet(nx, ny, seed=9):
    """nx x ny cells of two CPS3 triangles each on a grid with random column widths and row heights"""
    rng = np.random.default_rng(seed)
    x = np.concatenate([[0.0], np.cumsum(rng.uniform(0.5, 1.5, nx))])
    y = np.concatenate([[0.0], np.cumsum(rng.uniform(0.5, 1.5, ny))])
    X, Y = np.meshgrid(x, y, indexing="ij")
    nodes = np.column_stack([X.ravel(), Y.ravel()])
    i, j = np.meshgrid(np.arange(nx), np.arange(ny), indexing="ij")
    a = (i * (ny + 1) + j).ravel()
    b, c, d = a + (ny + 1), a + (ny + 1) + 1, a + 1
    el = np.stack([np.column_stack([a, b, c]), np.column_stack([a, c, d])], axis=1).reshape(-1, 3)
    return nodes, el.astype(np.int32), Element_linear_triangular()


# strips at the block edge of the element-per-thread kernel and, with npe = 3, of the apply pass over ne * npe shares; the
# sheet gives 258 workgroup partials: more than one trip of the 256-thread final reduction
EDGE_MESHES = {"strip-255": lambda: strip(255), "strip-256": lambda: strip(256), "strip-257": lambda: strip(257),
               "strip-513": lambda: strip(513), "sheet-65884": lambda: sheet(182, 181)}
SINGLES = ["CPS3", "CPS4", "CPS6", "CPS8", "C3D4", "C3D10", "C3D6", "C3D8"]


@functools.lru_cache(maxsize=None)
def mesh_of(name):
    if name in EDGE_MESHES:
        return EDGE_MESHES[name]()
    if name.startswith("one-"):
        return lr.single(name[4:])[:3]
    if name == "C3D6-3x3x2":
        return lr.mesh("C3D6", cells=(3, 3, 2), perturb=0.25)
    return ec.shape_mesh(name)


# (mesh, type, factor): every perturbed mesh of explicit_cases and one element of every family x the three types x with and
# without a factor; a factor alone on each mesh; the meshes of one increment also below min with tau under it (not scaled)
FACTOR_MESHES = list(ec.SHAPES) + ["C3D6-3x3x2"] + ["one-" + t for t in SINGLES]
# one element, and the 2 x 2 x 1 cells of C3D4 / C3D6 / C3D8, which have no interior node to perturb and so congruent
# elements: one increment, `below min` scales all of them or none.  Every family keeps a mesh with both branches: C3D4-150,
# C3D8-64 and, for the wedge, 3 x 3 x 2 perturbed cells added here
ONE_INCREMENT = ["one-" + t for t in SINGLES] + ["C3D4", "C3D6", "C3D8"]
FACTOR_CASES = [(name, kind, f) for name in FACTOR_MESHES for kind in TYPES for f in (None, 2.5)]
FACTOR_CASES += [(name, None, 0.3) for name in FACTOR_MESHES] + [(name, "unscaled", None) for name in ONE_INCREMENT]
EDGE_CASES = [(name, kind, None) for name in EDGE_MESHES for kind in ("below min", "uniform")]


@functools.lru_cache(maxsize=None)
def reference_call(name, kind, factor):
    """-> tau, the long-double Reference after the call, what the call returns, the error of the float64 restatement"""
    nodes, el, ELE = mesh_of(name)
    material = ec.material_of(ELE)
    ref = Reference(nodes, el, ELE, material, RHO, LD)
    w2 = ref.w2()
    if kind == "unscaled":
        kind, tau = "below min", float(0.5 * (2 / np.sqrt(w2)).min())
    else:
        tau = target(kind, w2, factor) if kind else None
    out = ref.scale(factor, tau, kind)
    if tau:
        r = (w2.max() if kind == "uniform" else w2) / LD(factor or 1.0) * LD(tau) ** 2 / 4
        assert np.abs(r - 1).min() > 1.0e-6, "an element at the threshold: the count would hang on the last bit"
    f64 = Reference(nodes, el, ELE, material, RHO, np.float64)
    out64 = f64.scale(factor, tau, kind)
    assert out64["scaled_elements"] == out["scaled_elements"]
    return tau, kind, ref, out, outputs_error(out64, f64.k, f64.nodal(), out, ref)


def call(name, kind, factor, backend):
    """one femcy_lumped_mass_scale against the restatement: the cumulative factors, the nodal masses, both totals, the count
    and the largest factor"""
    nodes, el, ELE = mesh_of(name)
    material = ec.material_of(ELE)
    tau, kind_used, ref, want, _ = reference_call(name, kind, factor)
    ctx = ac.make_ctx(nodes, el, ELE, material, backend)
    lm = ctx.lumped_mass(ELE, RHO)
    assert (ctx.lumped_mass_scaling(lm) == 1.0).all()
    out = ctx.lumped_mass_scale(lm, float(ac.s_C(material)), factor, tau, kind_used or "below min")
    k, m = ctx.lumped_mass_scaling(lm), ctx.lumped_mass_get(lm)
    ne = ctx.ne
    ctx.close()
    err = outputs_error(out, k, m, want, ref)
    print(f"{name} {kind} factor={factor} [{backend}]: {ne} elements, tau {tau}, {out['scaled_elements']} scaled, largest factor "
          f"{out['max_factor']:.6f}, mass {out['mass0']:.6e} -> {out['mass1']:.6e}, error {err:.3e}")
    assert k.shape == (ne,) and out["scaled_elements"] == want["scaled_elements"], (out["scaled_elements"], want["scaled_elements"])
    if kind == "below min" and name not in ONE_INCREMENT:
        grown = np.asarray(want["k"]) != (factor or 1.0)               # the elements whose increment was below tau
        assert 0 < grown.sum() < ne                                   # neither branch of max(1, .) passes vacuously
        assert (k[~grown] == (factor or 1.0)).all()                   # the others carry the factor alone, to the bit
        assert want["scaled_elements"] == (ne if factor else grown.sum())
    if kind == "unscaled":
        assert want["scaled_elements"] == 0 and (k == 1.0).all()
    if kind == "below min" and name in ONE_INCREMENT:
        assert want["scaled_elements"] == ne
    if kind == "set equal dt" and not factor:
        assert (k < 1.0).all()                                        # tau below every increment: every element is lightened
    if kind == "uniform":
        assert want["scaled_elements"] == ne and float(np.ptp(k)) == 0.0
    if name == "sheet-65884":
        assert -(-ne // 256) > 256                                    # more partials than one trip of the final reduction
    assert err <= SCALE_TOL, err
    return err


# ------------------------------------------------------------------------------ the estimate afterwards
AFTER_SHAPES = ["C3D4-150", "CPS4-65", "C3D10", "C3D8-64"]


@functools.lru_cache(maxsize=None)
def reference_after(name, kind):
    """the float64 restatement's increment after a call against tau"""
    nodes, el, ELE = mesh_of(name)
    tau, _, _, _, _ = reference_call(name, kind, None)
    f64 = Reference(nodes, el, ELE, ec.material_of(ELE), RHO, np.float64)
    f64.scale(None, tau, kind)
    dte = 2 / np.sqrt(f64.w2())
    return float(abs(dte.min() - tau) / tau) if kind == "below min" else float(np.abs(dte - tau).max() / tau)


def after(name, backend):
    """below min: 2 / femcy_explicit_element_bound(u = 0) is tau.  set equal dt: every element's long-double increment from
    the downloaded factors is tau.  femcy_explicit_stable_dt: Gershgorin's bound in numpy with the scaled inverse mass"""
    nodes, el, ELE = mesh_of(name)
    material = ec.material_of(ELE)
    sc = float(ac.s_C(material))
    _, fixed = ec.held_dofs(nodes)
    worst = 0.0
    for kind in ("below min", "set equal dt"):
        tau, _, ref, want, _ = reference_call(name, kind, None)
        ctx = ac.make_ctx(nodes, el, ELE, material, backend)
        lm = ctx.lumped_mass(ELE, RHO)
        ctx.lumped_mass_scale(lm, sc, None, tau, kind)
        k, m = ctx.lumped_mass_scaling(lm), ctx.lumped_mass_get(lm)
        ex = ctx.explicit(lm, [ctx.dofset(fixed)])
        ctx.vector(be.VEC_DOF).fill(0.0)
        dt = 2.0 / ctx.explicit_element_bound(ex, sc, be.VEC_DOF)
        ctx.assemble_K(-1)
        K = ctx.get_K_bsr().toarray()
        gdt, gom = ctx.explicit_stable_dt(ex)
        width = ctx.pattern_info().max_row_blocks * ELE.dm
        ctx.close()
        e1 = abs(dt - tau) / tau
        plain = Reference(nodes, el, ELE, material, RHO, LD)
        plain.est.me = plain.est.me * np.asarray(k, dtype=LD)[:, None]
        dte = 2 / np.sqrt(plain.w2())
        e2 = float(np.abs(dte - tau).max() / tau) if kind == "set equal dt" else float(abs(dte.min() - tau) / tau)
        minv = 1.0 / np.repeat(m, ELE.dm)
        minv[fixed] = 0.0
        e3 = abs(gom - er.gershgorin(K, minv)) / gom
        print(f"{name} {kind} [{backend}]: element bound after the call {e1:.3e}, per element from the factors {e2:.3e}, "
              f"Gershgorin {e3:.3e}")
        assert want["scaled_elements"] > 0
        assert e1 <= AFTER_TOL and e2 <= AFTER_TOL, (e1, e2)
        assert e3 <= (width + 2) * EPS and gdt == 2.0 / gom, e3       # the rounding bound of explicit_cases.omega_bound
        worst = max(worst, e1, e2)
    return worst


# --------------------------------------------------------------------------- same bits and compounding
F1, F2 = 1.3, 1.7


@functools.lru_cache(maxsize=None)
def reference_compound(name):
    """f1 then f2 against f1 f2 at once, in float64, against the long-double product"""
    nodes, el, ELE = mesh_of(name)
    material = ec.material_of(ELE)
    tau = reference_call(name, "below min", None)[0]
    ref = Reference(nodes, el, ELE, material, RHO, LD)
    ref.scale(F1, tau, "below min")
    ref.scale(F2)
    f64 = Reference(nodes, el, ELE, material, RHO, np.float64)
    f64.scale(F1, tau, "below min")
    f64.scale(F2)
    return tau, ref, max(relmax(f64.k, ref.k), relmax(f64.nodal(), ref.nodal()))


def same_bits_and_compounding(backend, name="C3D4-150"):
    """two identical calls on two fresh contexts: the same bits in every output.  A call (f1, tau) and then f2 against the
    restatement, whose factors are the products; and f1, f2 against f1 f2 at once within the bound"""
    nodes, el, ELE = mesh_of(name)
    material = ec.material_of(ELE)
    sc = float(ac.s_C(material))
    tau, ref, _ = reference_compound(name)
    runs = []
    for _ in range(2):
        ctx = ac.make_ctx(nodes, el, ELE, material, backend)
        lm = ctx.lumped_mass(ELE, RHO)
        o1 = ctx.lumped_mass_scale(lm, sc, F1, tau, "below min")
        o2 = ctx.lumped_mass_scale(lm, 0.0, F2)
        runs.append((o1, o2, ctx.lumped_mass_scaling(lm), ctx.lumped_mass_get(lm)))
        ctx.close()
    (a1, a2, ka, ma), (b1, b2, kb, mb) = runs
    assert a1 == b1 and a2 == b2, (a1, b1, a2, b2)
    assert np.array_equal(ka.view(np.uint64), kb.view(np.uint64)) and np.array_equal(ma.view(np.uint64), mb.view(np.uint64))
    assert a2["mass0"] == a1["mass1"] and a2["scaled_elements"] == len(el) and a2["max_factor"] == F2
    err = max(relmax(ka, ref.k), relmax(ma, ref.nodal()))
    ctx = ac.make_ctx(nodes, el, ELE, material, backend)
    lm = ctx.lumped_mass(ELE, RHO)
    ctx.lumped_mass_scale(lm, 0.0, F1)
    ctx.lumped_mass_scale(lm, 0.0, F2)
    k12, m12 = ctx.lumped_mass_scaling(lm), ctx.lumped_mass_get(lm)
    lm2 = ctx.lumped_mass(ELE, RHO)
    ctx.lumped_mass_scale(lm2, 0.0, F1 * F2)
    k1, m1 = ctx.lumped_mass_scaling(lm2), ctx.lumped_mass_get(lm2)
    ctx.close()
    e2 = max(relmax(k12, k1), relmax(m12, m1), relmax(k12, np.full(len(el), LD(F1) * LD(F2))))
    print(f"{name} [{backend}]: two calls against the restatement {err:.3e}, f1 then f2 against f1 f2 {e2:.3e}")
    assert max(err, e2) <= COMPOUND_TOL, (err, e2)
    return max(err, e2)


# ---------------------------------------------------------------------------------------------- decks
EVERY = 8
SF = 0.9


def solve(path, backend):
    """the deck through the driver -> inp, system (closed), u and v after every batch, the nodal masses and the cumulative
    factors the integrator was made from"""
    from femcy_amd.body import Body
    from femcy_amd.reader import InpInfo
    from femcy_amd.stiffnessMtrx import System_of_equations
    inp = InpInfo(path)
    body = Body(nodes=inp.nodes, elements=list(inp.eSets.values())[0], ELE=inp.ELE)
    system = System_of_equations(body, list(inp.materials.values())[0], inp.geometric_nonlinear, verbose=False,
                                 ctx=be.Context(0, backend=backend))
    U, V = [], []
    name = "explicit_auto_advance" if inp.dynamic_auto else "explicit_advance"
    advance = getattr(system.ctx, name)

    def recording(*a, **kw):
        advance(*a, **kw)
        U.append(system.dof.to_numpy())
        V.append(system.ctx.download(be.VEC_VEL))

    setattr(system.ctx, name, recording)
    try:
        system.solve(inp)
        m, k = system.ctx.lumped_mass_get(system.lumped_mass), system.ctx.lumped_mass_scaling(system.lumped_mass)
    finally:
        system.ctx.close()
    return inp, system, np.array(U), np.array(V), m, k


def dynamic_lines(mode, T, keyword=""):
    """fixed: the increment estimated once from the matrix; auto: element by element; one record per EVERY steps"""
    flag = ", element by element" if mode == "auto" else ""
    return "*Dynamic, explicit%s, scale factor=%r, output_every=%d\n, %r\n%s" % (flag, SF, EVERY, T, keyword)


def run_reference(nodes, el, ELE, mat, me, f, v0, fixed, mode, T, h, dtype):
    """the restatement with the element shares me [ne, npe]: fixed: nsteps of h; auto: the element-by-element rule.
    -> steps, U, V, kinetic and strain energy at the records (every EVERY-th step and the last)"""
    est = ac.Estimate(nodes, el, ELE, mat, 1.0, dtype)
    est.me = np.asarray(me, dtype=dtype)
    m = np.zeros(len(nodes), dtype=dtype)
    np.add.at(m, np.asarray(el), est.me)
    minv = 1 / np.repeat(m, ELE.dm)
    minv[fixed] = 0
    if mode == "auto":
        H, _, U, V = ac.verlet_auto(est, minv, f, v0, SF, T, False)
        n = len(H)
    else:
        n = int(round(T / h))
        U, V, _ = est.mdl.verlet(minv, f, v0, dtype(T) / n, n, lambda k: 1.0)
    rec = sorted(set(list(range(EVERY, n + 1, EVERY)) + [n]))
    return n, U[rec], V[rec], np.array([er.kinetic(m, v, ELE.dm, dtype) for v in V[rec]]), \
        np.array([est.mdl.energy(u) for u in U[rec]])


def traj_error(got, want):
    """u, v relative to their largest entries, the two energies relative to the largest total energy"""
    (U, V, ke, se), (Ur, Vr, ker, ser) = got, want
    escale = float((np.asarray(ker, dtype=LD) + np.asarray(ser, dtype=LD)).max())
    return max(relmax(U, Ur), relmax(V, Vr), float(np.abs(np.asarray(ke, dtype=LD) - ker).max()) / escale,
               float(np.abs(np.asarray(se, dtype=LD) - ser).max()) / escale)


def fixed_increment(nodes, el, ELE, mat, m, fixed, T):
    """the driver's rule for a fixed run on the host backend's matrix: scale factor x Gershgorin's 2 / omega with the nodal
    masses m, adjusted down so that T is a whole number of steps -> (stable dt, steps, h)"""
    ctx = ac.make_ctx(nodes, el, ELE, mat, "cpu")
    ctx.assemble_K(-1)
    K = ctx.get_K_bsr().toarray()
    ctx.close()
    minv = 1.0 / np.repeat(np.asarray(m, dtype=np.float64), ELE.dm)
    minv[fixed] = 0.0
    dt = 2.0 / er.gershgorin(K, minv)
    n = max(1, int(np.ceil(T / (SF * dt) * (1.0 - 1.0e-12))))
    return dt, n, T / n


def records_of(system, U, V):
    return U, V, np.array([i["kinetic"] for i in system.increments]), np.array([i["strain_energy"] for i in system.increments])


# ----------------------------------------------------------------------- factor = f is a denser material
PAIR_T = 0.05


def write_pair_deck(path, mode, scaled):
    """the bar of explicit_cases (no bulk viscosity, no body force): `*Fixed Mass Scaling, factor=4` at density rho, or no
    keyword at 4 rho"""
    keyword = "*Fixed Mass Scaling, factor=4.\n" if scaled else ""
    material = "*Density\n%.17g,\n*Elastic\n%.17g, %.17g\n" % (RHO if scaled else 4.0 * RHO, ec.E_MOD, ec.NU)
    nodes, el = ec.dc.bar_mesh()
    nsets = {"all": np.arange(len(nodes)), "foot": np.nonzero(nodes[:, 2] < 1e-12)[0]}
    ec.write_explicit_deck(path, nodes, el, "C3D4", nsets, "*Boundary\nfoot, 1, 1\nfoot, 2, 2\nfoot, 3, 3\n",
                           dynamic_lines(mode, PAIR_T, keyword), material=material,
                           initial="*Initial Conditions, type=VELOCITY\nall, 3, 25.\nall, 1, -4.\n")
    return nodes, el, lr.single("C3D4")[2], LinearIsotropic(ec.E_MOD, ec.NU)


@functools.lru_cache(maxsize=None)
def reference_pair(mode, workdir):
    path = os.path.join(workdir, "ref_pair_%s.inp" % mode)
    nodes, el, ELE, mat = write_pair_deck(path, mode, False)
    inp, f, v0, fixed = ec.deck_loads(path)
    me = ac.element_masses(nodes, el, ELE, 4.0 * RHO, LD)
    m = er.lumped_mass(nodes, el, ELE, 4.0 * RHO, LD)
    dt, n, h = fixed_increment(nodes, el, ELE, mat, m, fixed, PAIR_T) if mode == "fixed" else (None, None, None)
    ref = run_reference(nodes, el, ELE, mat, me, f, v0, fixed, mode, PAIR_T, h, LD)
    f64 = run_reference(nodes, el, ELE, mat, ac.element_masses(nodes, el, ELE, 4.0 * RHO, np.float64), f, v0, fixed, mode,
                        PAIR_T, h, np.float64)
    assert f64[0] == ref[0] and ref[0] > 3 * EVERY
    if mode == "auto":
        dt = float(2 / ac.Estimate(nodes, el, ELE, mat, 4.0 * RHO, LD).omega(np.zeros(nodes.size)))
    return {"m": m, "dt": dt, "steps": ref[0], "traj": ref[1:], "f64": traj_error(f64[1:], ref[1:])}


def denser_material(tmpdir, mode, backend, workdir):
    """both decks against the long-double run at 4 rho: the nodal masses, stable_dt and u, v, kinetic and strain energy at
    every record"""
    ref = reference_pair(mode, workdir)
    runs = {}
    for scaled in (True, False):
        path = os.path.join(str(tmpdir), "pair_%s_%d.inp" % (mode, scaled))
        write_pair_deck(path, mode, scaled)
        inp, system, U, V, m, k = solve(path, backend)
        assert (inp.mass_scaling == {"factor": 4.0, "dt": None, "type": "below min"}) if scaled else inp.mass_scaling is None
        if scaled:
            assert system.mass_scaling["max_factor"] == 4.0 and system.mass_scaling["scaled_elements"] == len(k) and (k == 4.0).all()
            assert relmax(system.mass_scaling["mass1"], 4 * LD(system.mass_scaling["mass0"])) <= SCALE_TOL
        else:
            assert system.mass_scaling is None and (k == 1.0).all()
        assert system.increments[-1]["kinc"] == ref["steps"] and system.increments[-1]["time1"] == PAIR_T
        em, ed = relmax(m, ref["m"]), abs(system.stable_dt - ref["dt"]) / ref["dt"]
        et = traj_error(records_of(system, U, V), ref["traj"])
        print(f"pair {mode} scaled={scaled} [{backend}]: {ref['steps']} steps, masses {em:.3e}, stable dt {ed:.3e}, trajectory {et:.3e}")
        assert max(em, ed, et) <= 4.0 * F64_WORST_PAIR[mode], (em, ed, et)
        runs[scaled] = (m, system.stable_dt, U, V)
    diff = max(relmax(runs[True][0], runs[False][0]), relmax(runs[True][2], runs[False][2]), relmax(runs[True][3], runs[False][3]))
    print(f"pair {mode} [{backend}]: factor=4 against 4 rho {diff:.3e}")
    assert diff <= 8.0 * F64_WORST_PAIR[mode], diff
    return diff


# ---------------------------------------------------------------------------------- a graded bar end to end
GRADED_T = 0.04
SQUEEZE = 0.25


def graded_mesh():
    """the C3D4 column of explicit_cases with six layers, the third and fourth squeezed to a quarter of the others' height"""
    nodes, el, ELE = lr.mesh("C3D4", cells=(1, 1, 6), perturb=0.0)
    nodes = np.array(nodes, dtype=np.float64)
    z = np.unique(np.round(nodes[:, 2], 9))
    assert len(z) == 7
    hgt = np.where(np.isin(np.arange(6), (2, 3)), SQUEEZE, 1.0) * (z[1] - z[0])
    new = np.concatenate([[0.0], np.cumsum(hgt)])
    level = np.searchsorted(z, np.round(nodes[:, 2], 9))
    nodes[:, 2] = new[level]
    return nodes, el, ELE, np.isin(level[el].min(axis=1), (2, 3))


def write_graded_deck(path, mode, tau):
    nodes, el, ELE, _ = graded_mesh()
    keyword = "" if tau is None else "*Fixed Mass Scaling, dt=%r\n" % tau
    nsets = {"all": np.arange(len(nodes)), "foot": np.nonzero(nodes[:, 2] < 1e-12)[0]}
    ec.write_explicit_deck(path, nodes, el, "C3D4", nsets, "*Boundary\nfoot, 1, 1\nfoot, 2, 2\nfoot, 3, 3\n",
                           dynamic_lines(mode, GRADED_T, keyword),
                           initial="*Initial Conditions, type=VELOCITY\nall, 3, 25.\nall, 1, -4.\n")
    return nodes, el, ELE, LinearIsotropic(ec.E_MOD, ec.NU)


@functools.lru_cache(maxsize=None)
def reference_graded(mode, workdir):
    """tau = 0.999 x the smallest long-double increment of the regular elements (at 1 x that element would sit on the
    threshold of `below min`): exactly the squeezed elements are scaled"""
    nodes, el, ELE, squeezed = graded_mesh()
    mat = LinearIsotropic(ec.E_MOD, ec.NU)
    plain = Reference(nodes, el, ELE, mat, RHO, LD)
    dte = 2 / np.sqrt(plain.w2())
    assert dte[squeezed].max() < 0.9 * dte[~squeezed].min()
    tau = float(0.999 * dte[~squeezed].min())
    path = os.path.join(workdir, "ref_graded_%s.inp" % mode)
    write_graded_deck(path, mode, tau)
    inp, f, v0, fixed = ec.deck_loads(path)
    m_plain = plain.nodal()
    out = plain.scale(None, tau, "below min")
    assert np.array_equal(out["k"] != 1, squeezed) and np.abs(plain.w2() * LD(tau) ** 2 / 4 - 1)[~squeezed].min() > 1.0e-6
    f64 = Reference(nodes, el, ELE, mat, RHO, np.float64)
    f64.scale(None, tau, "below min")
    dt = dt_plain = n_plain = h = None
    if mode == "fixed":
        dt_plain, n_plain, _ = fixed_increment(nodes, el, ELE, mat, m_plain, fixed, GRADED_T)
        dt, _, h = fixed_increment(nodes, el, ELE, mat, plain.nodal(), fixed, GRADED_T)
    ref = run_reference(nodes, el, ELE, mat, plain.est.me, f, v0, fixed, mode, GRADED_T, h, LD)
    r64 = run_reference(nodes, el, ELE, mat, f64.est.me, f, v0, fixed, mode, GRADED_T, h, np.float64)
    assert r64[0] == ref[0] and ref[0] > 3 * EVERY
    if mode == "auto":
        dt, dt_plain = tau, float(dte.min())
        n_plain = int(np.ceil(GRADED_T / (SF * dt_plain)))           # at least: the increments of the unscaled run only shrink
    return {"tau": tau, "dt": dt, "dt_plain": dt_plain, "steps": ref[0], "steps_plain": n_plain, "traj": ref[1:],
            "added": float(out["mass1"] / out["mass0"] - 1), "scaled": int(squeezed.sum()), "f64": traj_error(r64[1:], ref[1:])}


def graded(tmpdir, mode, backend, workdir):
    """`*Fixed Mass Scaling, dt=tau` on the graded bar: stable_dt rises to the regular elements' (auto) / to Gershgorin's with
    the scaled masses (fixed), the step count falls to the reference's, the added mass and the trajectory are the reference's"""
    ref = reference_graded(mode, workdir)
    path = os.path.join(str(tmpdir), "graded_%s.inp" % mode)
    write_graded_deck(path, mode, ref["tau"])
    inp, system, U, V, m, k = solve(path, backend)
    ms = system.mass_scaling
    assert inp.mass_scaling == {"factor": None, "dt": ref["tau"], "type": "below min"}
    assert ms["scaled_elements"] == ref["scaled"] == int((k != 1.0).sum()) and system.increments[-1]["time1"] == GRADED_T
    ed = abs(system.stable_dt - ref["dt"]) / ref["dt"]
    ea = abs((ms["mass1"] / ms["mass0"] - 1) - ref["added"]) / ref["added"]
    et = traj_error(records_of(system, U, V), ref["traj"])
    steps = system.increments[-1]["kinc"]
    print(f"graded {mode} [{backend}]: stable dt {ref['dt_plain']:.4e} -> {system.stable_dt:.4e} ({ed:.3e}), steps "
          f"{ref['steps_plain']} -> {steps}, added mass {ref['added']:.4f} ({ea:.3e}), trajectory {et:.3e}")
    assert system.stable_dt > 1.5 * ref["dt_plain"] and steps == ref["steps"] and steps < 0.7 * ref["steps_plain"]
    assert ed <= AFTER_TOL + 64 * EPS * (mode == "fixed"), ed       # fixed: a row sum of the matrix, as in omega_bound
    assert ea <= SCALE_TOL / ref["added"], ea                        # a difference of two totals, each within the bound
    assert et <= 4.0 * F64_WORST_GRADED[mode], et
    return U, V


def host_against_device(tmpdir, mode, workdir):
    """the two backends on the graded deck: each within 4 x the float64 figure of the reference, so within 8 x of each other"""
    Uh, Vh = graded(tmpdir, mode, "cpu", workdir)
    Ud, Vd = graded(tmpdir, mode, "hip", workdir)
    e = max(relmax(Ud, Uh), relmax(Vd, Vh))
    print(f"graded {mode}: host against device {e:.3e}")
    assert e <= 8.0 * F64_WORST_GRADED[mode], e


# --------------------------------------------------------------------------------------------- reader
def deck_with(tmpdir, keyword="", dynamic=None):
    path = os.path.join(str(tmpdir), "ms_%d.inp" % len(os.listdir(str(tmpdir))))
    head = dynamic if dynamic is not None else "*Dynamic, explicit, direct user control, output_every=4\n1e-4, 1.2e-3\n"
    ec.write_case_deck(path, "bar", dynamic=head + keyword)
    return path


def reader(tmpdir, backend="cpu"):
    from femcy_amd.reader import InpInfo
    assert InpInfo(deck_with(tmpdir)).mass_scaling is None
    for line, want in (("*Fixed Mass Scaling, factor=4.", {"factor": 4.0, "dt": None, "type": "below min"}),
                       ("*Fixed Mass Scaling, dt=1e-5", {"factor": None, "dt": 1e-5, "type": "below min"}),
                       ("*FIXED MASS SCALING, FACTOR=2, DT=1e-5, TYPE=UNIFORM", {"factor": 2.0, "dt": 1e-5, "type": "uniform"}),
                       ("*Fixed Mass Scaling, dt=2e-5, type=set equal dt", {"factor": None, "dt": 2e-5, "type": "set equal dt"}),
                       ("*Fixed Mass Scaling, type=below min, dt=3e-5", {"factor": None, "dt": 3e-5, "type": "below min"})):
        assert InpInfo(deck_with(tmpdir, line + "\n")).mass_scaling == want, line
    static = "*Static\n1., 1., 1e-05, 1.\n"
    implicit = "*Dynamic, direct\n1e-4, 1e-3\n"
    for line, dynamic, word in (("*Fixed Mass Scaling, factor=2., elset=all", None, "elset"),
                                ("*Variable Mass Scaling, dt=1e-5, type=below min, frequency=10", None, "Variable Mass Scaling"),
                                ("*Fixed Mass Scaling", None, "needs factor=, dt= or both"),
                                ("*Fixed Mass Scaling, factor=0.", None, "must be positive"),
                                ("*Fixed Mass Scaling, factor=-2.", None, "must be positive"),
                                ("*Fixed Mass Scaling, dt=-1e-5", None, "must be positive"),
                                ("*Fixed Mass Scaling, dt=0", None, "must be positive"),
                                ("*Fixed Mass Scaling, factor=nan", None, "must be positive"),
                                ("*Fixed Mass Scaling, factor=2., type=uniform", None, "needs dt="),
                                ("*Fixed Mass Scaling, dt=1e-5, type=rolling", None, "type=rolling"),
                                ("*Fixed Mass Scaling, factor=2.", static, "outside a \\*Dynamic, explicit step"),
                                ("*Fixed Mass Scaling, factor=2.", implicit, "outside a \\*Dynamic, explicit step")):
        with pytest.raises(ValueError, match=word):
            InpInfo(deck_with(tmpdir, line + "\n", dynamic))
    # no keyword: nothing is scaled, and the run has the bits of the same deck scaled by exactly 1
    runs = [solve(deck_with(tmpdir, keyword), backend) for keyword in ("", "*Fixed Mass Scaling, factor=1.\n")]
    (inp, system, U, V, m, k), (_, system1, U1, V1, m1, k1) = runs
    assert inp.mass_scaling is None and system.mass_scaling is None and (k == 1.0).all() and len(U) == 3
    assert system1.mass_scaling["scaled_elements"] == 0 and system1.mass_scaling["mass0"] == system1.mass_scaling["mass1"]
    for a, b in ((U, U1), (V, V1), (m, m1), (k, k1)):
        assert np.array_equal(a.view(np.uint64), b.view(np.uint64))


# --------------------------------------------------------------------------------------------- refusals
def refusals(backend):
    """every refusal of femcy_lumped_mass_scale returns FEMCY_EINVAL with a word of its message and leaves a context that
    still works; a broken element returns FEMCY_ENUMERIC and leaves the lumped mass bit for bit"""
    import ctypes as C
    nodes, el, ELE = mesh_of("C3D8")
    material = ec.material_of(ELE)
    sc = float(ac.s_C(material))
    ctx = ac.make_ctx(nodes, el, ELE, material, backend)
    lm = ctx.lumped_mass(ELE, RHO)
    m = ctx.lumped_mass_get(lm)
    rows = [((lm + 1, sc, 2.0), "unknown lumped mass"), ((-1, sc, 2.0), "unknown lumped mass"),
            ((lm, sc, None, None), "a factor, a target increment dt or both"), ((lm, sc, 0.0, 0.0), "or both"),
            ((lm, sc, 2.0, 1e-5, 3), "unknown type 3"), ((lm, sc, 2.0, None, -1), "unknown type -1"),
            ((lm, sc, 2.0, 1e-5, "rolling"), "unknown type")]
    for bad in (-1.0, np.nan, np.inf, -np.inf):
        rows += [((lm, sc, bad), "finite and not negative"), ((lm, sc, None, bad), "finite and not negative"),
                 ((lm, sc, 2.0, bad), "finite and not negative")]
    for bad in (0.0, -1.0, np.nan, np.inf):
        rows += [((lm, bad, None, 1e-5), "s_C"), ((lm, bad, 2.0, 1e-5, "uniform"), "s_C")]
    for args, word in rows:
        with pytest.raises(be.FemcyError, match=word) as refused:
            ctx.lumped_mass_scale(*args)
        assert refused.value.status == -1, args                       # FEMCY_EINVAL
    d, i64 = C.c_double(), C.c_int64()
    for hole in range(4):
        outs = [C.byref(d), C.byref(d), C.byref(i64), C.byref(d)]
        outs[hole] = None
        with pytest.raises(be.FemcyError, match="null output") as refused:
            ctx._call("femcy_lumped_mass_scale", lm, sc, 2.0, 0.0, 0, *outs)
        assert refused.value.status == -1
    with pytest.raises(be.FemcyError, match="null output"):
        ctx._call("femcy_lumped_mass_get_scaling", lm, None)
    with pytest.raises(be.FemcyError, match="unknown lumped mass"):
        ctx.lumped_mass_scaling(lm + 1)
    ex = ctx.explicit(lm)
    for args in ((lm, sc, 2.0), (lm, sc, None, 1e-5)):
        with pytest.raises(be.FemcyError, match="scale before femcy_explicit_create") as refused:
            ctx.lumped_mass_scale(*args)
        assert refused.value.status == -1
    assert np.array_equal(ctx.lumped_mass_get(lm).view(np.uint64), m.view(np.uint64)) and (ctx.lumped_mass_scaling(lm) == 1.0).all()
    lm2 = ctx.lumped_mass(ELE, RHO)                                   # the context still works: a mass no integrator refers to
    out = ctx.lumped_mass_scale(lm2, sc, 2.0)
    assert out["max_factor"] == 2.0 and np.array_equal(ctx.lumped_mass_get(lm2), 2.0 * m) and ctx.explicit_kinetic_energy(ex) == 0.0
    ctx.close()
    bare = be.Context(0, backend=backend)                             # before the problem is defined
    with pytest.raises(be.FemcyError, match="not fully defined") as refused:
        bare.lumped_mass_scale(0, sc, 2.0)
    assert refused.value.status == -1
    bare.close()


def broken_element(backend):
    """one node coordinate NaN (18 nodes: below the size at which the pattern orders nodes by coordinate): FEMCY_ENUMERIC
    under every rule, the nodal masses -- those of the sound elements included -- and the factors unchanged bit for bit, and
    the context still works"""
    nodes, el, ELE = mesh_of("C3D4")
    material = ec.material_of(ELE)
    sc = float(ac.s_C(material))
    bad = np.array(nodes, dtype=np.float64)
    bad[el[len(el) // 2][1], 0] = np.nan
    ctx = ac.make_ctx(bad, el, ELE, material, backend)
    lm = ctx.lumped_mass(ELE, RHO)
    m = ctx.lumped_mass_get(lm)
    assert np.isnan(m).any() and np.isfinite(m).any()
    for args in ((lm, sc, 2.0), (lm, sc, None, 1e-5), (lm, sc, 2.0, 1e-5, "set equal dt"), (lm, sc, None, 1e-5, "uniform")):
        with pytest.raises(be.FemcyError, match="broken element") as refused:
            ctx.lumped_mass_scale(*args)
        assert refused.value.status == be.FEMCY_ENUMERIC, args
        assert np.array_equal(ctx.lumped_mass_get(lm).view(np.uint64), m.view(np.uint64)), args
        assert (ctx.lumped_mass_scaling(lm) == 1.0).all()
    ctx.set_mesh(nodes, el)                                           # the context still works, on the sound mesh
    ctx.set_element(ELE)
    ctx.set_material(material)
    ctx.build_pattern()
    lm = ctx.lumped_mass(ELE, RHO)
    assert ctx.lumped_mass_scale(lm, sc, 2.0)["max_factor"] == 2.0
    ctx.close()


def comm_refusal(backend):
    """once femcy_comm_init has run (the route of explicit_cases.comm_refusal; device only)"""
    nodes, el, ELE = ec.shape_mesh("C3D8-64")
    ctx = lc.make_ctx(nodes, el, ELE, backend)
    lm = ctx.lumped_mass(ELE, RHO)
    ctx.assemble_K(-1)
    iface = np.arange(0, ctx.n, 7, dtype=np.int32)
    ctx.comm_init(0, 1, be.Context.comm_unique_id(), iface, np.arange(iface.size, dtype=np.int32), iface.size,
                  np.ones(ctx.n, dtype=np.uint8))
    for call in (lambda: ctx.lumped_mass_scale(lm, 1.0, 2.0), lambda: ctx.lumped_mass_scaling(lm)):
        with pytest.raises(be.FemcyError, match="several ranks") as refused:
            call()
        assert refused.value.status == -1
    ctx.close()


# ------------------------------------------------------------------------------------- the constants
def measure_f64_worst(workdir):
    """the constants at the top, as measured: the float64 restatement against the long-double one on the cases run here"""
    return {"scale": max(reference_call(*case)[4] for case in FACTOR_CASES + EDGE_CASES),
            "after": max(reference_after(name, kind) for name in AFTER_SHAPES for kind in ("below min", "set equal dt")),
            "compound": reference_compound("C3D4-150")[2],
            "pair": {mode: reference_pair(mode, workdir)["f64"] for mode in ("fixed", "auto")},
            "graded": {mode: reference_graded(mode, workdir)["f64"] for mode in ("fixed", "auto")}}
