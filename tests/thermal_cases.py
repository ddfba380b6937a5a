"""Thermal-load scenarios written against the C ABI (femcy_amd.backend.Context) and the deck driver, so that the host
backend (tests/test_thermal_cpu.py, backend "cpu") and the device (tests/test_gpu_thermal.py, backend "hip") run the same
code.  Every function checks its own result.

Bounds.  The reference of the kernel checks is the restatement of tests/thermal_reference.py in np.longdouble.  The same
restatement in float64 differs from it by rounding and summation order alone; F64_WORST_FORCE / F64_WORST_STRESS are the
worst such differences over CASES and the small meshes (measured with `measure_f64_worst`, asserted by
tests/test_thermal_cpu.py::test_the_float64_restatement_stays_within_its_constants), and a backend is held to 4 x that: a
different but legitimate summation order differs by as much.  Errors are relative to the largest entry of the reference
(force) or to the largest entry of the uncorrected stress and of the correction (stress, von Mises)."""
import functools
import types

import numpy as np
import pytest

from femcy_amd import backend as be
from femcy_amd.material_zoo import LinearIsotropic, LinearIsotropicPlaneStrain, LinearIsotropicPlaneStress

import loads_cases as lc
import loads_reference as lr
import thermal_reference as tr

LD = np.longdouble
E_MOD, NU, ALPHA = 2.0e5, 0.3, 1.2e-5
SCALE = 0.75
# worst error of the float64 restatement against the long-double one (measure_f64_worst: 7.01e-15 on the curved CPS8 mesh,
# where the loads of a corner node nearly cancel, and 4.87e-16 as measured)
F64_WORST_FORCE = 7.1e-15
F64_WORST_STRESS = 4.9e-16
FORCE_TOL = 4.0 * F64_WORST_FORCE
STRESS_TOL = 4.0 * F64_WORST_STRESS

# (element type, material kind, anisotropic C): all eight (npe, dm) shapes, the three linear kinds, the general C once
CASES = [("C3D4", tr.LIN3D, False), ("C3D10", tr.LIN3D, False), ("C3D8", tr.LIN3D, False), ("C3D6", tr.LIN3D, False),
         ("C3D8", tr.LIN3D, True)]
CASES += [(e, k, False) for e in ("CPS3", "CPS4", "CPS6", "CPS8") for k in (tr.PSTRESS, tr.PSTRAIN)]
SMALL_CELLS = {2: (3, 2), 3: (2, 2, 1)}                      # fewer than 64 elements: not even one wavefront
KIND_OF = {"C3D": tr.LIN3D, "CPS": tr.PSTRESS, "CPE": tr.PSTRAIN}


def material(kind, aniso=False):
    if kind == tr.LIN3D:
        m = LinearIsotropic(E_MOD, NU)
        if aniso:                                             # fully populated, symmetric, no material symmetry
            A = np.random.default_rng(11).standard_normal((6, 6))
            return types.SimpleNamespace(kind=m.kind, C=m.C + 0.05 * np.abs(m.C).max() * (A + A.T), params=m.params)
        return m
    return LinearIsotropicPlaneStress(E_MOD, NU) if kind == tr.PSTRESS else LinearIsotropicPlaneStrain(E_MOD, NU)


def make_ctx(nodes, el, ELE, mat, backend, pattern=True):
    ctx = be.Context(0, backend=backend)
    ctx.set_mesh(nodes, el)
    ctx.set_element(ELE)
    ctx.set_material(mat)
    if pattern:
        ctx.build_pattern()
    return ctx


def smooth_disp(nodes):
    """a smooth displacement field with strains of the size of alpha dT (1e-3)"""
    x, y = nodes[:, 0], nodes[:, 1]
    u = np.zeros_like(nodes)
    u[:, 0] = 1.0e-3 * np.sin(0.8 * x + 0.3 * y)
    u[:, 1] = 0.7e-3 * np.cos(0.5 * x - 0.9 * y)
    if nodes.shape[1] == 3:
        u[:, 2] = 0.5e-3 * np.sin(0.6 * nodes[:, 2] + 0.2 * x)
    return u.ravel()


def mesh_of(etype, which):
    if which == "mesh":
        return lr.mesh(etype)
    if which == "single":
        return lr.single(etype)[:3]
    if which == "small":
        return lr.mesh(etype, cells=SMALL_CELLS[2 if etype.startswith("CP") else 3])
    assert which == "fan" and etype == "CPS3"
    return lr.fan(40)


def run_backend(etype, kind, aniso, which, backend, zero=False):
    """-> f_unit, the uncorrected sigma, the corrected sigma, the corrected von Mises"""
    nodes, el, ELE = mesh_of(etype, which)
    dT = np.zeros(len(nodes)) if zero else tr.smooth_dT(nodes)
    ctx = make_ctx(nodes, el, ELE, material(kind, aniso), backend)
    th = ctx.thermal(ELE, ALPHA, dT)
    f = ctx.thermal_force(th)
    ctx.upload(be.VEC_DOF, smooth_disp(nodes))
    ctx.compute_strain_stress(be.VEC_DOF, large=False)
    sigma0 = ctx.gauss_field(be.GP_SIGMA).to_numpy()
    ctx.thermal_stress(th, SCALE)
    sigma, mises = ctx.gauss_field(be.GP_SIGMA).to_numpy(), ctx.gauss_field(be.GP_MISES).to_numpy()
    ctx.close()
    return f, sigma0, sigma, mises


@functools.lru_cache(maxsize=None)
def reference_force(etype, kind, aniso, which):
    """-> (long-double f_unit, error of the float64 restatement): computed once, shared by every test"""
    nodes, el, ELE = mesh_of(etype, which)
    mat = material(kind, aniso)
    dT = tr.smooth_dT(nodes)
    ref = tr.thermal_force(nodes, el, ELE, mat.C, kind, NU, ALPHA, dT, LD)
    f64 = tr.thermal_force(nodes, el, ELE, mat.C, kind, NU, ALPHA, dT, np.float64)
    ref.setflags(write=False)
    return ref, float(np.abs(f64 - ref).max() / np.abs(ref).max())


def stress_errors(etype, kind, aniso, which, sigma0, sigma, mises):
    """errors of a corrected (sigma, mises) against the long-double restatement from the same uncorrected sigma0"""
    nodes, el, ELE = mesh_of(etype, which)
    mat = material(kind, aniso)
    dT = tr.smooth_dT(nodes)
    ref_s, ref_m = tr.corrected_stress(el, ELE, mat.C, kind, NU, ALPHA, dT, SCALE, sigma0, LD)
    size = max(np.abs(sigma0).max(), float(np.abs(ref_s - sigma0.astype(LD)).max()))
    return float(np.abs(sigma - ref_s).max() / size), float(np.abs(mises - ref_m).max() / size)


def f64_stress_error(etype, kind, aniso, which, sigma0):
    nodes, el, ELE = mesh_of(etype, which)
    mat = material(kind, aniso)
    s, m = tr.corrected_stress(el, ELE, mat.C, kind, NU, ALPHA, tr.smooth_dT(nodes), SCALE, sigma0, np.float64)
    return max(stress_errors(etype, kind, aniso, which, sigma0, s, m))


def against_restatement(etype, kind, aniso, which, backend):
    """-> (force error, stress error, von Mises error), each asserted against its bound"""
    f, sigma0, sigma, mises = run_backend(etype, kind, aniso, which, backend)
    ref, _ = reference_force(etype, kind, aniso, which)
    ef = float(np.abs(f - ref).max() / np.abs(ref).max())
    es, em = stress_errors(etype, kind, aniso, which, sigma0, sigma, mises)
    print(f"{etype} {kind}{' aniso' if aniso else ''} {which} [{backend}]: force {ef:.3e}, stress {es:.3e}, mises {em:.3e}")
    assert np.abs(sigma0).max() > 0 and not np.array_equal(sigma, sigma0)
    assert ef <= FORCE_TOL and es <= STRESS_TOL and em <= STRESS_TOL, (ef, es, em)
    return ef, es, em


def measure_f64_worst():
    """the two constants at the top, as measured: the float64 restatement against the long-double one on every case"""
    wf = ws = 0.0
    todo = [(e, k, a, "mesh") for e, k, a in CASES] + [(e, KIND_OF[e[:3]], False, w) for e in lr.ETYPES for w in ("single", "small")]
    todo.append(("CPS3", tr.PSTRESS, False, "fan"))
    for etype, kind, aniso, which in todo:
        wf = max(wf, reference_force(etype, kind, aniso, which)[1])
        nodes, el, ELE = mesh_of(etype, which)
        # the uncorrected stress of the float64 restatement itself: C : eps(u) is not under test here, any sigma0 serves
        sigma0 = np.random.default_rng(2).uniform(-300.0, 300.0, (len(el), len(ELE.gaussWeights), ELE.dm, ELE.dm))
        sigma0 = 0.5 * (sigma0 + sigma0.swapaxes(-1, -2))
        ws = max(ws, f64_stress_error(etype, kind, aniso, which, sigma0))
    return wf, ws


def zero_field_and_bits(backend):
    """dT = 0 gives all-zero bits; two creates of the same load give identical bits"""
    for etype, kind in (("C3D10", tr.LIN3D), ("CPS8", tr.PSTRAIN)):
        f, sigma0, sigma, _ = run_backend(etype, kind, False, "mesh", backend, zero=True)
        assert not f.view(np.uint64).any(), "a zero temperature change must give +0.0 everywhere"
        assert np.array_equal(sigma, sigma0)
        a = run_backend(etype, kind, False, "mesh", backend)
        b = run_backend(etype, kind, False, "mesh", backend)
        for x, y in zip(a, b):
            assert np.array_equal(x.view(np.uint64), y.view(np.uint64))
    nodes, el, ELE = lr.mesh("C3D4")
    ctx = make_ctx(nodes, el, ELE, material(tr.LIN3D), backend)
    dT = tr.smooth_dT(nodes)
    f1 = ctx.thermal_force(ctx.thermal(ELE, ALPHA, dT))
    f2 = ctx.thermal_force(ctx.thermal(ELE, ALPHA, dT))            # a second object in the same context
    ctx.close()
    assert np.array_equal(f1.view(np.uint64), f2.view(np.uint64))


def apply(backend):
    """add = 0 overwrites, add = 1 equals the caller's sum bit for bit, scale 0 / 0.25 / 1 are exact multiples"""
    nodes, el, ELE = lr.mesh("C3D8")
    ctx = make_ctx(nodes, el, ELE, material(tr.LIN3D), backend)
    th = ctx.thermal(ELE, ALPHA, tr.smooth_dT(nodes))
    f = ctx.thermal_force(th)
    assert f.size > 256 and f.size % 256                          # more than one block of the apply, the last one partial
    for scale in (0.0, 0.25, 1.0, -1.7):
        ctx.upload(be.VEC_RHS, np.full(nodes.size, 7.0))
        ctx.thermal_apply(th, scale, be.VEC_RHS)                  # add = 0 overwrites
        assert np.array_equal(ctx.download(be.VEC_RHS), scale * f)    # one rounding: the IEEE product
    base = np.random.default_rng(4).standard_normal(nodes.size)
    ctx.upload(be.VEC_RHS, base)
    ctx.thermal_apply(th, 0.3, be.VEC_RHS, add=True)
    assert np.array_equal(ctx.download(be.VEC_RHS), base + 0.3 * f)   # the product is rounded before the sum
    ls = ctx.loadset(ELE, np.array([0, 5, 9, 100], np.int32), np.array([0, 1, 2, 3], np.int32))
    ctx.loadset_neumann(ls, 2.5, None, be.VEC_RHS)
    surface = ctx.download(be.VEC_RHS)
    assert surface.any()
    ctx.thermal_apply(th, 1.0, be.VEC_RHS, add=True)
    assert np.array_equal(ctx.download(be.VEC_RHS), surface + f)
    ctx.close()


def refusals(backend):
    """every refusal returns a status with a message, and the context keeps working"""
    import ctypes as C
    nodes, el, ELE = lr.mesh("C3D8", cells=(2, 2, 2))
    dT = tr.smooth_dT(nodes)
    ctx = make_ctx(nodes, el, ELE, material(tr.LIN3D), backend, pattern=False)
    with pytest.raises(be.FemcyError, match="pattern"):
        ctx.thermal(ELE, ALPHA, dT)                               # before femcy_build_pattern
    ctx.build_pattern()
    th = ctx.thermal(ELE, ALPHA, dT)
    for bad in (np.nan, np.inf):
        with pytest.raises(be.FemcyError, match="not finite"):
            ctx.thermal(ELE, bad, dT)
    N = np.ascontiguousarray(ELE.tables()["N"], dtype=np.float64)
    out = C.c_int32()
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    for args in ((None, ALPHA, ptr(dT)), (ptr(N), ALPHA, None)):
        with pytest.raises(be.FemcyError, match="null"):
            ctx._call("femcy_thermal_create", args[0], args[1], args[2], C.byref(out))
    with pytest.raises(be.FemcyError):
        ctx.thermal(ELE, ALPHA, dT[:-1])                          # nn values are needed
    for call in (lambda: ctx.thermal_force(th + 1), lambda: ctx.thermal_apply(-1, 1.0), lambda: ctx.thermal_stress(7, 1.0)):
        with pytest.raises(be.FemcyError, match="unknown thermal load"):
            call()
    with pytest.raises(be.FemcyError):
        ctx.thermal_apply(th, 1.0, 99)
    with pytest.raises(be.FemcyError, match="femcy_compute_strain_stress"):
        ctx.thermal_stress(th, 1.0)                               # no Gauss-point stress yet
    ctx.upload(be.VEC_DOF, smooth_disp(nodes))
    ctx.compute_strain_stress(be.VEC_DOF, large=True)
    with pytest.raises(be.FemcyError, match="femcy_compute_strain_stress"):
        ctx.thermal_stress(th, 1.0)                               # the nlgeom stress is not the one to correct
    ctx.compute_strain_stress(be.VEC_DOF, large=False)
    ctx.thermal_stress(th, 1.0)
    with pytest.raises(be.FemcyError, match="femcy_compute_strain_stress"):
        ctx.thermal_stress(th, 1.0)                               # once per computed stress
    ctx.thermal_apply(th, 1.0)                                    # the context still works
    assert np.array_equal(ctx.download(be.VEC_RHS), ctx.thermal_force(th))
    from femcy_amd.material_zoo import NeoHookean
    ctx.set_material(NeoHookean(C1=80.0, D1=400.0))
    with pytest.raises(be.FemcyError, match="neo-Hookean"):
        ctx.thermal(ELE, ALPHA, dT)
    ctx.set_material(material(tr.LIN3D))
    assert np.array_equal(ctx.thermal_force(ctx.thermal(ELE, ALPHA, dT)), ctx.thermal_force(th))
    ctx.set_mesh(nodes, el)                                       # a new mesh drops the thermal loads
    with pytest.raises(be.FemcyError, match="unknown thermal load"):
        ctx.thermal_force(th)
    ctx.close()


# --------------------------------------------------------------------------------------------- decks
T0, T1, GRAD = 20.0, 120.0, 35.0
DT = T1 - T0
FAMILIES = ["CPS3", "CPS4", "CPS6", "CPS8", "CPE3", "CPE4", "CPE6", "CPE8", "C3D4", "C3D10", "C3D8", "C3D6"]
QUADRATIC = ["CPS6", "CPS8", "CPE6", "CPE8", "C3D10"]
DECK_CELLS = {2: (5, 4), 3: (3, 3, 2)}
# worst error of the host backend against the closed forms (a), (b), (c) over FAMILIES, as measured: 3.68e-10 (the gradient
# on C3D10 in the 80 x 10 x 120 plate); it scales with the condition of K, not with the kernel, so a backend gets 10 x
# that, capped at the whole-deck tolerance of the project
HOST_DECK_WORST = 4.0e-10
DECK_TOL = min(10.0 * HOST_DECK_WORST, 1.0e-6)


def family_mesh(family, straight=False):
    base = "CPS" + family[3:] if family.startswith("CPE") else family
    dm = 2 if base.startswith("CP") else 3
    flat, el, ELE = lr.mesh(base, cells=DECK_CELLS[dm], perturb=0.0)
    if straight:
        return flat, el, ELE
    if base == "C3D10":
        # moved corners, straight edges: on a curved tetrahedron grad N |det J| is cubic and the four-point rule is not
        # exact for it, so a uniform stress is not in equilibrium there (the bar is 1.6e-7 off) whatever loads the body
        from femcy_amd import meshgen
        corners, tets, _ = lr.mesh("C3D4", cells=DECK_CELLS[dm], perturb=0.25)
        nodes, el2 = meshgen.to_quadratic(corners, tets)
        assert np.array_equal(el2, el)
        return nodes, el, ELE
    nodes = lr.mesh(base, cells=DECK_CELLS[dm], perturb=0.25)[0].copy()
    # the outline stays the box: a bar with a bent lateral side would need a traction there (mid-side nodes of the
    # quadratic meshes are bent on the outline too)
    hi = flat.max(axis=0)
    outline = ((flat < 1e-12) | (flat > hi[None, :] - 1e-12)).any(axis=1)
    nodes[outline] = flat[outline]
    return nodes, el, ELE


def k_of(family):
    return 1.0 + NU if family.startswith("CPE") else 1.0


def _corner(nodes, at):
    i = np.nonzero(np.abs(nodes - np.asarray(at)[None, :]).max(axis=1) < 1e-12)[0]
    assert i.size == 1, at
    return i


def write_thermal_deck(path, family, case, static="1., 1., 1e-05, 1.", nlgeom=False, expansion_first=False,
                       thermal=True, extra_step=""):
    """(a) "free": uniform T0 -> T1, statically determinate supports.  (b) "bar": the same, u_x = 0 on both x faces.
    (c) "gradient": 0 -> GRAD * y by bare node labels, the supports carry the closed form's values.  thermal = False
    leaves the three thermal keywords out (the same deck, cold); extra_step is keyword text put ahead of *Temperature.
    -> nodes"""
    nodes, el, _ = family_mesh(family, straight=case == "gradient")
    dm = nodes.shape[1]
    hi = nodes.max(axis=0)
    zero = [0.0] * dm
    A = _corner(nodes, zero)
    B = _corner(nodes, [hi[0]] + zero[1:])
    Cn = _corner(nodes, [0.0, hi[1]] + zero[2:])
    nsets = {"all": np.arange(len(nodes)), "A": A, "B": B, "C": Cn,
             "left": np.nonzero(nodes[:, 0] < 1e-12)[0], "right": np.nonzero(nodes[:, 0] > hi[0] - 1e-12)[0]}
    elastic, expansion = "*Elastic\n%.17g, %.17g\n" % (E_MOD, NU), "*Expansion, zero=20.\n%.17g,\n" % ALPHA
    mat = expansion + elastic if expansion_first else elastic + expansion
    if not thermal:
        assert case != "gradient"
        mat = elastic
    if case == "gradient":
        k = k_of(family)
        step = "*Boundary\nA, 1, 1\nA, 2, 2\nB, 2, 2, %.17g\n" % (-0.5 * k * ALPHA * GRAD * hi[0] ** 2)
        if dm == 3:
            step += "A, 3, 3\nB, 3, 3\nC, 3, 3\n"
        step += "*Temperature\n" + "".join("%d, %.17g\n" % (i + 1, GRAD * y) for i, y in enumerate(nodes[:, 1]))
    else:
        if thermal:
            mat += "*Initial Conditions, type=TEMPERATURE\nall, %.17g\n" % T0
        if case == "free":
            step = "*Boundary\nA, 1, 1\nA, 2, 2\nB, 2, 2\n" + ("A, 3, 3\nB, 3, 3\nC, 3, 3\n" if dm == 3 else "")
        else:
            step = "*Boundary\nleft, 1, 1\nright, 1, 1\nA, 2, 2\n" + ("A, 3, 3\nC, 3, 3\n" if dm == 3 else "")
        step += extra_step + ("*Temperature\nall, %.17g\n" % T1 if thermal else "")
    lc.write_deck(path, nodes, el, family, nsets, mat, step, nlgeom=nlgeom, static=static)
    return nodes


def exact(family, case, nodes):
    """-> displacements [nn * dm], in-plane stress tensor (None: varies) and von Mises (None: varies) of the closed form"""
    dm, k = nodes.shape[1], k_of(family)
    u = np.zeros_like(nodes)
    sig = np.zeros((dm, dm))
    s = E_MOD * ALPHA * DT
    if case == "free":
        u[:] = k * ALPHA * DT * nodes                                  # x0 = the corner at the origin
        return u.ravel(), sig, s if family.startswith("CPE") else 0.0
    if case == "bar":
        lat = (1.0 + NU) / (1.0 - NU) if family.startswith("CPE") else 1.0 + NU
        u[:, 1:] = lat * ALPHA * DT * nodes[:, 1:]
        sig[0, 0] = -s / (1.0 - NU) if family.startswith("CPE") else -s
        return u.ravel(), sig, abs(sig[0, 0])
    x, y = nodes[:, 0], nodes[:, 1]
    z = nodes[:, 2] if dm == 3 else 0.0 * x
    u[:, 0] = k * ALPHA * GRAD * x * y
    u[:, 1] = 0.5 * k * ALPHA * GRAD * (y * y - x * x - z * z)
    if dm == 3:
        u[:, 2] = k * ALPHA * GRAD * y * z
    return u.ravel(), sig, None


def solve_thermal_deck(path, backend):
    """-> inp, system (closed), the displacements after every increment, sigma, mises"""
    from femcy_amd.body import Body
    from femcy_amd.reader import InpInfo
    from femcy_amd.stiffnessMtrx import System_of_equations
    inp = InpInfo(path)
    body = Body(nodes=inp.nodes, elements=list(inp.eSets.values())[0], ELE=inp.ELE)
    system = System_of_equations(body, list(inp.materials.values())[0], inp.geometric_nonlinear, verbose=False,
                                 ctx=be.Context(0, backend=backend))
    per_inc, advance = [], system.advance_inc

    def recording(*a, **kw):
        out = advance(*a, **kw)
        per_inc.append(system.dof.to_numpy())
        return out

    system.advance_inc = recording
    try:
        system.solve(inp)
        system.compute_strain_stress()
        sigma, mises = system.cauchy_stress.to_numpy(), system.mises_stress.to_numpy()
    finally:
        system.ctx.close()
    return inp, system, per_inc, sigma, mises


def closed_form(tmpdir, family, case, backend):
    """-> the error against the closed form: displacements relative to the largest one, stresses relative to E alpha dT"""
    import os
    path = os.path.join(str(tmpdir), "%s_%s.inp" % (family, case))
    nodes = write_thermal_deck(path, family, case)
    inp, system, per_inc, sigma, mises = solve_thermal_deck(path, backend)
    assert inp.expansion == ALPHA and inp.temperature_info is not None and system.stats["direct_solves"] == 1
    ue, sig, vm = exact(family, case, nodes)
    size = E_MOD * ALPHA * (DT if case != "gradient" else GRAD * np.abs(nodes[:, 1]).max())
    eu = np.abs(per_inc[-1] - ue).max() / np.abs(ue).max()
    es = np.abs(sigma - sig[None, None]).max() / size
    em = 0.0 if vm is None else np.abs(mises - vm).max() / size
    if case == "gradient" and family.startswith("CPE"):               # sigma_zz = -E alpha T_g: von Mises = E alpha |T_g|
        Tg = tr.gauss_dT(list(inp.eSets.values())[0], inp.ELE, GRAD * nodes[:, 1], np.float64)
        em = np.abs(mises - E_MOD * ALPHA * np.abs(Tg)).max() / size
    err = float(max(eu, es, em))
    print(f"{family} ({case}) [{backend}]: displacement {eu:.3e}, stress {es:.3e}, mises {em:.3e}")
    assert np.abs(ue).max() > 0 and err <= DECK_TOL, (eu, es, em)
    return err


def half_increment(tmpdir, family, backend):
    """max_time 1, fixed increments of 0.5: the first increment carries half the temperature change.  The first matrix is
    the undeformed one, so its displacement is half the closed form within the deck tolerance.  The second matrix is
    assembled on the configuration the first left (the driver does so in linear runs, as the reference does), which moves
    the final answer by the order of the strain k alpha dT = 1.6e-3; ten times that bounds `first = final / 2`."""
    import os
    path = os.path.join(str(tmpdir), "%s_half.inp" % family)
    nodes = write_thermal_deck(path, family, "free", static="0.5, 1., 1e-05, 0.5")
    _, system, per_inc, _, _ = solve_thermal_deck(path, backend)
    assert [i["time1"] for i in system.increments] == [0.5, 1.0] and len(per_inc) == 2
    ue = exact(family, "free", nodes)[0]
    e_first = np.abs(per_inc[0] - 0.5 * ue).max() / np.abs(0.5 * ue).max()
    e_half = np.abs(per_inc[0] - 0.5 * per_inc[1]).max() / np.abs(0.5 * per_inc[1]).max()
    print(f"{family} half increment [{backend}]: first against half the closed form {e_first:.3e}, against half the final {e_half:.3e}")
    assert e_first <= DECK_TOL
    assert e_half <= 10.0 * k_of(family) * ALPHA * DT
    assert system._thermal["scale"] == 1.0
