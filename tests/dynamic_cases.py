"""Implicit-dynamics scenarios written against the C ABI (femcy_amd.backend.Context) and the deck driver, so that the host
backend (tests/test_dynamic_cpu.py, backend "cpu") and the device (tests/test_gpu_dynamic.py, backend "hip") run the same
code.  Every function checks its own result and returns the figure it checked.

Bounds.  The reference is the restatement of tests/dynamic_reference.py in np.longdouble.  The same restatement in float64
differs from it by rounding and summation order alone; the F64_WORST_* constants are the worst such differences on the very
cases run here (`measure_f64_worst`, asserted by tests/test_dynamic_cpu.py), and a backend is held to 4 x that.  Errors are
relative to the largest entry of the reference."""
import functools
import os

import numpy as np
import pytest

from femcy_amd import backend as be
from femcy_amd.material_zoo import LinearIsotropic, LinearIsotropicPlaneStrain, LinearIsotropicPlaneStress

import dynamic_reference as dr
import loads_cases as lc
import loads_reference as lr
import thermal_cases as tc

LD = np.longdouble
E_MOD, NU, RHO = 2.0e5, 0.3, 7.85e-3
GRAV = 9.81
FAMILIES = tc.FAMILIES
# worst error of the float64 restatement against the long-double one (measure_f64_worst, as measured): the mass 4.77e-16,
# the product 3.92e-16, the energy drift 2.41e-14 (on the bar the test runs), the trajectories 9.75e-15; free flight against g t^2 / 2 4.42e-9 (K + a0 M
# is nearly singular on translations at dt = 0.125: |K| / (a0 m) ~ 1e8, and the error is that condition times the rounding)
F64_WORST_MASS = 4.8e-16
F64_WORST_APPLY = 4.0e-16
F64_WORST_FLIGHT = 4.5e-9
F64_WORST_ENERGY = 2.5e-14
F64_WORST_TRAJ = 9.8e-15
F64_WORST_SMALL_ENERGY = 4.7e-14   # the energy of the infinitesimal strain, measured 4.67e-14: eps = sym(F) - I loses the digits of 1 / |eps| (1e3 here)
MASS_TOL, APPLY_TOL = 4.0 * F64_WORST_MASS, 4.0 * F64_WORST_APPLY
SMALL_ENERGY_TOL = 4.0 * F64_WORST_SMALL_ENERGY
FLIGHT_TOL, ENERGY_TOL, TRAJ_TOL = 4.0 * F64_WORST_FLIGHT, 4.0 * F64_WORST_ENERGY, 4.0 * F64_WORST_TRAJ

# ABI meshes: (family, cells, perturb).  Fewer than 64 elements where the family allows it; 63, 64 and 65 nodes (one slice of
# the sorted storage less one lane, full, and one node into a second slice); 130 nodes (a third slice with padding lanes);
# perturbed C3D8 / C3D6 / CPS4 cells; curved sides on C3D10 / CPS6 / CPS8 (lr.mesh bends the mid-side nodes).
SHAPES = {"CPS4-63": ("CPS4", (8, 6), 0.25), "C3D8-64": ("C3D8", (3, 3, 3), 0.25), "CPS4-65": ("CPS4", (12, 4), 0.25),
          "CPS4-130": ("CPS4", (12, 9), 0.25), "CPS3": ("CPS3", (3, 2), 0.25), "CPS6": ("CPS6", (3, 2), 0.25),
          "CPS8": ("CPS8", (3, 2), 0.25), "C3D4": ("C3D4", (2, 2, 1), 0.25), "C3D10": ("C3D10", (2, 2, 1), 0.25),
          "C3D6": ("C3D6", (2, 2, 1), 0.25), "C3D8": ("C3D8", (2, 2, 1), 0.25), "C3D4-150": ("C3D4", (5, 4, 4), 0.25)}
CURVED = ("CPS6", "CPS8", "C3D10")


def shape_mesh(name):
    etype, cells, perturb = SHAPES[name]
    return lr.mesh(etype, cells=cells, perturb=perturb)


def make_ctx(nodes, el, ELE, backend, pattern=True):
    return lc.make_ctx(nodes, el, ELE, backend, pattern)


@functools.lru_cache(maxsize=None)
def reference_mass(name):
    """-> (long-double M [nn, nn], error of the float64 restatement): computed once, shared"""
    nodes, el, ELE = shape_mesh(name)
    ref = dr.mass_matrix(nodes, el, ELE, RHO, LD)
    f64 = dr.mass_matrix(nodes, el, ELE, RHO, np.float64)
    ref.setflags(write=False)
    return ref, float(np.abs(f64 - ref).max() / np.abs(ref).max())


# ------------------------------------------------------------------------------------------ the mass
def single_element(etype, backend):
    """one straight C3D4 / CPS3: m_ab = rho V (1 + delta_ab) / 20 and rho A (1 + delta_ab) / 12"""
    nodes, el, ELE, V = lr.single(etype)
    ctx = make_ctx(nodes, el, ELE, backend)
    M = ctx.mass_get(ctx.mass(ELE, RHO)).toarray()
    ctx.close()
    n = len(nodes)
    want = RHO * V * (1.0 + np.eye(n)) / (20.0 if etype == "C3D4" else 12.0)
    err = float(np.abs(M - want).max() / want.max())
    print(f"{etype} [{backend}]: single element, error {err:.3e}")
    assert err <= MASS_TOL, err
    return err


def mass_properties(name, backend):
    """sum = rho V, row sums = rho x the body-load weights (the existing kernel; straight sides), symmetry through the
    stored transposes (bit for bit), re-creation bit-equal, the long-double restatement"""
    nodes, el, ELE = shape_mesh(name)
    ctx = make_ctx(nodes, el, ELE, backend)
    ms = ctx.mass(ELE, RHO)
    M = ctx.mass_get(ms)
    M2 = ctx.mass_get(ctx.mass(ELE, RHO))
    bw = ctx.bodyload_weights(ctx.bodyload(ELE))
    info = ctx.pattern_info()
    ctx.close()
    assert M.nnz == info.nnzb
    assert np.array_equal(M.data.view(np.uint64), M2.data.view(np.uint64)), "re-creation must give the same bits"
    D = M.toarray()
    assert np.array_equal(D, D.T), "m_ab and m_ba are the same sum of the same products"
    ref, _ = reference_mass(name)
    em = float(np.abs(D - ref).max() / np.abs(ref).max())
    V = float(dr.mass_volume(nodes, el, ELE))
    ev = abs(D.sum() - RHO * V) / (RHO * V)
    rows = D.sum(axis=1)
    if SHAPES[name][0] in CURVED:
        # curved sides: N_a |det J| has degree 2p there, which the stiffness rule of the body-load kernel does not integrate
        # exactly; the row sums are held to the mass rule's own integral of N_a instead
        N, dN, w = dr.mass_tables(ELE, LD)
        want = np.zeros(len(nodes), dtype=LD)
        for c in el:
            for q in range(len(w)):
                want[c] += RHO * N[q] * abs(dr._det(np.asarray(nodes[c], dtype=LD).T @ dN[q])) * w[q]
    else:
        want = RHO * bw
    er = float(np.abs(rows - want).max() / np.abs(want).max())
    print(f"{name} [{backend}]: {len(nodes)} nodes, {len(el)} elements, mass {em:.3e}, volume {ev:.3e}, row sums {er:.3e}")
    assert em <= MASS_TOL, em
    # a sum of nnzb rounded entries / a row of at most a few dozen: the restatement's bound per entry times their number
    assert ev <= MASS_TOL * 8 and er <= MASS_TOL * 8, (ev, er)
    return em


def mass_apply(name, backend):
    """y = [y +] scale M x against the dense long-double product: both add modes, scale != 1, an x that is non-zero in the
    rows next to the padding lanes (every entry is non-zero)"""
    nodes, el, ELE = shape_mesh(name)
    dm = ELE.dm
    ref, _ = reference_mass(name)
    rng = np.random.default_rng(7)
    x = rng.uniform(0.5, 1.5, nodes.size) * rng.choice([-1.0, 1.0], nodes.size)
    base = rng.standard_normal(nodes.size)
    Mx = (ref @ x.reshape(-1, dm).astype(LD)).ravel()
    ctx = make_ctx(nodes, el, ELE, backend)
    ms = ctx.mass(ELE, RHO)
    ctx.upload(be.VEC_DOF, x)
    worst = 0.0
    for scale, add in ((1.0, False), (-2.75, False), (0.625, True)):
        ctx.upload(be.VEC_TMP0, base)
        ctx.mass_apply(ms, be.VEC_DOF, be.VEC_TMP0, scale, add=add)
        want = (base.astype(LD) if add else 0) + LD(scale) * Mx
        worst = max(worst, float(np.abs(ctx.download(be.VEC_TMP0) - want).max() / np.abs(want).max()))
    ke = ctx.mass_kinetic_energy(ms, be.VEC_DOF)
    ke2 = ctx.mass_kinetic_energy(ms, be.VEC_DOF)
    want_ke = float(0.5 * (x.astype(LD) @ Mx))
    ek = abs(ke - want_ke) / want_ke
    assert np.array_equal(ctx.download(be.VEC_DOF), x), "x is read only"
    ctx.close()
    print(f"{name} [{backend}]: product {worst:.3e}, kinetic energy {ek:.3e}")
    assert ke == ke2, "the reduction has a fixed order"
    assert worst <= APPLY_TOL and ek <= APPLY_TOL, (worst, ek)
    return worst


def add_to_K(name, backend):
    """K after the call = K before + c m on the block diagonals and only there, exactly (the product is rounded before it is
    added); overwrite leaves exactly c M (x) I"""
    nodes, el, ELE = shape_mesh(name)
    dm = ELE.dm
    ctx = make_ctx(nodes, el, ELE, backend)
    ms = ctx.mass(ELE, RHO)
    m = ctx.mass_get(ms)
    ctx.assemble_K(-1)
    K0 = ctx.get_K_bsr()
    c = 1234.5678
    ctx.mass_add_to_K(ms, c)
    K1 = ctx.get_K_bsr()
    assert np.array_equal(K0.indices, m.indices) and np.array_equal(K0.indptr, m.indptr)
    want = K0.data.copy()
    cm = c * m.data
    for d in range(dm):
        want[:, d, d] = want[:, d, d] + cm
    assert np.array_equal(K1.data, want)
    ctx.mass_add_to_K(ms, -0.5, overwrite=True)
    K2 = ctx.get_K_bsr()
    only = np.zeros_like(K0.data)
    for d in range(dm):
        only[:, d, d] = -0.5 * m.data
    assert np.array_equal(K2.data, only)
    ctx.assemble_K(-1)                                            # the next assembly starts over
    assert np.array_equal(ctx.get_K_bsr().data, K0.data)
    ctx.close()


def newmark_kernels(name, backend):
    """predict and update against numpy; the bound is the rounding of the few operations of one entry"""
    nodes, el, ELE = shape_mesh(name)
    n = nodes.size
    rng = np.random.default_rng(3)
    u, v, a, un = (rng.standard_normal(n) for _ in range(4))
    ctx = make_ctx(nodes, el, ELE, backend)
    for vec, arr in ((be.VEC_DOF_OLD, u), (be.VEC_VEL, v), (be.VEC_ACC, a), (be.VEC_DOF, un)):
        ctx.upload(vec, arr)
    c0, c1, c2 = 3.5, -0.25, 1.75
    ctx.newmark_predict(be.VEC_DOF_OLD, be.VEC_VEL, be.VEC_ACC, be.VEC_RESIDUAL, c0, c1, c2)
    got = ctx.download(be.VEC_RESIDUAL)
    size = np.abs(c0 * u) + np.abs(c1 * v) + np.abs(c2 * a)
    eps = np.finfo(np.float64).eps
    assert (np.abs(got - (c0 * u + c1 * v + c2 * a)) <= 4 * eps * size).all()    # three products, two sums
    beta, gamma, dt = 0.3025, 0.6, 0.125
    ctx.newmark_update(be.VEC_DOF, be.VEC_DOF_OLD, be.VEC_VEL, be.VEC_ACC, beta, gamma, dt)
    b0, b1, b2 = 1 / (beta * dt * dt), 1 / (beta * dt), 1 / (2 * beta) - 1
    an = b0 * (un - u) - b1 * v - b2 * a
    vn = v + dt * ((1 - gamma) * a + gamma * an)
    sa = b0 * (np.abs(un) + np.abs(u)) + b1 * np.abs(v) + abs(b2) * np.abs(a)
    assert (np.abs(ctx.download(be.VEC_ACC) - an) <= 8 * eps * sa).all()
    assert (np.abs(ctx.download(be.VEC_VEL) - vn) <= 8 * eps * (np.abs(v) + dt * (np.abs(a) + sa))).all()
    assert np.array_equal(ctx.download(be.VEC_DOF), un) and np.array_equal(ctx.download(be.VEC_DOF_OLD), u)
    ctx.close()


ENERGY_SHAPES = ["CPS4-65", "CPS8", "C3D8-64", "C3D10", "C3D4-150"]


@functools.lru_cache(maxsize=None)
def reference_small_energy(name):
    """-> (long-double energy of tc.smooth_disp, error of the float64 restatement)"""
    nodes, el, ELE = shape_mesh(name)
    mat = LinearIsotropic(2.0e5, 0.3) if ELE.dm == 3 else LinearIsotropicPlaneStress(2.0e5, 0.3)      # lc.make_ctx's
    u = tc.smooth_disp(nodes)
    ref = dr.small_strain_energy(nodes, el, ELE, mat.C, u, LD)
    f64 = dr.small_strain_energy(nodes, el, ELE, mat.C, u, np.float64)
    return float(ref), float(abs(f64 - ref) / ref)


def small_energy(name, backend):
    """femcy_elastic_energy_small against the long-double restatement of sum eps^T C eps / 2 |det J| w on the undeformed mesh;
    the call leaves the undeformed geometry behind (the next assembly gives the same K), is repeatable bit for bit, and is
    not the reference's energy of the Green strain, which is off by the order of the strain (1e-3 here)."""
    nodes, el, ELE = shape_mesh(name)
    u = tc.smooth_disp(nodes)
    ctx = make_ctx(nodes, el, ELE, backend)
    ctx.assemble_K(-1)
    K = ctx.get_K_bsr().data.copy()
    ctx.upload(be.VEC_DOF, u)
    got = ctx.elastic_energy(be.VEC_DOF, small=True)
    again = ctx.elastic_energy(be.VEC_DOF, small=True)
    green = ctx.elastic_energy(be.VEC_DOF)
    ctx.assemble_K(-1)
    assert np.array_equal(ctx.get_K_bsr().data, K)
    ctx.close()
    want, _ = reference_small_energy(name)
    err = abs(got - want) / want
    print(f"{name} [{backend}]: small-strain energy {got:.6e}, error {err:.3e}, Green-strain energy off by {abs(green - want) / want:.1e}")
    assert got == again and want > 0
    assert err <= SMALL_ENERGY_TOL, err
    assert abs(green - want) / want > 1e-6, "the two energies are different things"
    return err


def small_energy_refusal(backend):
    from femcy_amd.material_zoo import NeoHookean
    nodes, el, ELE = shape_mesh("C3D8")
    ctx = make_ctx(nodes, el, ELE, backend)
    ctx.set_material(NeoHookean(C1=80.0, D1=400.0))
    with pytest.raises(be.FemcyError, match="neo-Hookean"):
        ctx.elastic_energy(be.VEC_DOF, small=True)
    assert ctx.elastic_energy(be.VEC_DOF) == 0.0                  # the context still works
    ctx.close()


def refusals(backend):
    """every refusal returns FEMCY_EINVAL with a message, and the context keeps working"""
    import ctypes as C
    nodes, el, ELE = shape_mesh("C3D8")
    ctx = make_ctx(nodes, el, ELE, backend, pattern=False)
    with pytest.raises(be.FemcyError, match="pattern"):
        ctx.mass(ELE, RHO)                                        # before femcy_build_pattern
    ctx.build_pattern()
    ms = ctx.mass(ELE, RHO)
    for bad in (np.nan, np.inf, 0.0, -1.0):
        with pytest.raises(be.FemcyError, match="density"):
            ctx.mass(ELE, bad)
    t = ELE.mass_tables()
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    out = C.c_int32()
    for args in ((None, ptr(t["dNq"]), ptr(t["wq"])), (ptr(t["Nq"]), None, ptr(t["wq"])), (ptr(t["Nq"]), ptr(t["dNq"]), None)):
        with pytest.raises(be.FemcyError, match="null"):
            ctx._call("femcy_mass_create", t["nq"], args[0], args[1], args[2], RHO, C.byref(out))
    with pytest.raises(be.FemcyError, match="points"):
        ctx._call("femcy_mass_create", 0, ptr(t["Nq"]), ptr(t["dNq"]), ptr(t["wq"]), RHO, C.byref(out))
    for call in (lambda: ctx.mass_get(ms + 1), lambda: ctx.mass_apply(-1, be.VEC_DOF, be.VEC_RHS),
                 lambda: ctx.mass_add_to_K(7, 1.0), lambda: ctx.mass_kinetic_energy(ms + 1, be.VEC_VEL)):
        with pytest.raises(be.FemcyError, match="unknown mass object"):
            call()
    with pytest.raises(be.FemcyError):
        ctx.mass_apply(ms, be.VEC_DOF, 99)
    with pytest.raises(be.FemcyError, match="in place"):
        ctx.mass_apply(ms, be.VEC_DOF, be.VEC_DOF)
    with pytest.raises(be.FemcyError, match="beta"):
        ctx.newmark_update(be.VEC_DOF, be.VEC_DOF_OLD, be.VEC_VEL, be.VEC_ACC, 0.0, 0.5, 0.1)
    for out in (be.VEC_DOF, be.VEC_VEL, be.VEC_ACC):
        with pytest.raises(be.FemcyError, match="output may not be one of the inputs"):
            ctx.newmark_predict(be.VEC_DOF, be.VEC_VEL, be.VEC_ACC, out, 1.0, 1.0, 1.0)
    with pytest.raises(be.FemcyError) as refused:
        ctx.mass(ELE, -1.0)
    assert refused.value.status == -1                             # FEMCY_EINVAL
    assert be.VEC_VEL == 9 and be.VEC_ACC == 10 and be.VEC_TMP1 == 8
    ctx.upload(be.VEC_VEL, np.ones(nodes.size))                   # the context still works
    assert ctx.mass_kinetic_energy(ms, be.VEC_VEL) > 0
    ctx.set_mesh(nodes, el)                                       # a new mesh drops the mass objects
    with pytest.raises(be.FemcyError, match="unknown mass object"):
        ctx.mass_kinetic_energy(ms, be.VEC_VEL)
    ctx.close()


# --------------------------------------------------------------------------------------------- decks
def write_dynamic_deck(path, nodes, el, family, nsets, step, dynamic="*Dynamic, direct\n0.125, 1.\n", amplitude=None,
                       material=None, initial="", nlgeom=False, surface=None):
    mat = material if material is not None else "*Density\n%.17g,\n*Elastic\n%.17g, %.17g\n" % (RHO, E_MOD, NU)
    lc.write_deck(path, nodes, el, family, nsets, mat + initial, step, surface=surface, nlgeom=nlgeom)
    text = open(path).read()
    head = "*Step, name=Step-1%s, nlgeom=%s\n" % ("" if amplitude is None else ", amplitude=" + amplitude, "YES" if nlgeom else "NO")
    old = text[text.index("*Step, name=Step-1"):text.index("*Static\n") + len("*Static\n1., 1., 1e-05, 1.\n")]
    with open(path, "w") as f:
        f.write(text.replace(old, head + dynamic))


def solve_deck(path, backend, **system_kw):
    """-> inp, system (closed), the displacements after every step"""
    from femcy_amd.body import Body
    from femcy_amd.reader import InpInfo
    from femcy_amd.stiffnessMtrx import System_of_equations
    inp = InpInfo(path)
    body = Body(nodes=inp.nodes, elements=list(inp.eSets.values())[0], ELE=inp.ELE)
    system = System_of_equations(body, list(inp.materials.values())[0], inp.geometric_nonlinear, verbose=False,
                                 ctx=be.Context(0, backend=backend), **system_kw)
    per_step, update = [], system.ctx.newmark_update

    def recording(*a, **kw):
        update(*a, **kw)
        per_step.append(system.dof.to_numpy())

    system.ctx.newmark_update = recording
    try:
        system.solve(inp)
    finally:
        system.ctx.close()
    return inp, system, np.array(per_step)


def flight_mesh(family):
    """tc.family_mesh, with straight sides on the quadratic 2-D families: on a curved side N_a |det J| has degree 2p, which the
    stiffness rule of the body-load kernel does not integrate exactly while the mass rule does, so that gravity and inertia
    would not cancel node by node (4.5e-5 on CPS6, 1.0e-5 on CPS8); the curved meshes serve the mass checks only"""
    if family[3:] in ("6", "8") and family.startswith("CP"):
        corners, cells, _ = tc.family_mesh(family[:3] + {"6": "3", "8": "4"}[family[3:]])
        edges = [(0, 1), (1, 2), (2, 0)] if family[3:] == "6" else [(0, 1), (1, 2), (2, 3), (3, 0)]
        nodes, el = lr.with_midsides(corners, cells, edges)
        return nodes, el, tc.family_mesh(family, straight=True)[2]
    return tc.family_mesh(family)


def free_flight(tmpdir, family, backend):
    """an unconstrained body under STEP gravity: every node at u = g t^2 / 2 after every one of 8 steps (the trapezoidal
    rule is exact for a constant acceleration, K annihilates translations); also exercises a_0"""
    nodes, el, _ = flight_mesh(family)
    dm = nodes.shape[1]
    path = os.path.join(str(tmpdir), "%s_flight.inp" % family)
    direction = "0., -1." if dm == 2 else "0., 0., -1."
    write_dynamic_deck(path, nodes, el, family, {"all": np.arange(len(nodes))}, "*Dload\n, GRAV, %.17g, %s\n" % (GRAV, direction))
    inp, system, U = solve_deck(path, backend)
    assert inp.procedure == "dynamic" and inp.amplitude == "STEP" and len(U) == 8
    worst = 0.0
    for inc, u in zip(system.increments, U):
        want = np.zeros_like(nodes)
        want[:, dm - 1] = -0.5 * GRAV * inc["time1"] ** 2
        worst = max(worst, float(np.abs(u - want.ravel()).max() / (0.5 * GRAV * inc["time1"] ** 2)))
    assert system.increments[-1]["time1"] == 1.0
    print(f"{family} [{backend}]: free flight, worst error over 8 steps {worst:.3e}")
    assert worst <= FLIGHT_TOL, worst
    return worst


BAR_DT_T = (6.0e-4, 9.6e-3)


def bar_mesh():
    """a column of 1 x 1 x 4 cells of C3D4 (a family the oracle assembles: measure_f64_worst runs the float64 restatement
    on this very mesh, with these initial velocities and increments)"""
    nodes, el, _ = lr.mesh("C3D4", cells=(1, 1, 4), perturb=0.0)
    return nodes, el


def write_energy_deck(path):
    nodes, el = bar_mesh()
    nsets = {"all": np.arange(len(nodes)), "foot": np.nonzero(nodes[:, 2] < 1e-12)[0]}
    step = "*Boundary\nfoot, 1, 1\nfoot, 2, 2\nfoot, 3, 3\n"
    initial = "*Initial Conditions, type=VELOCITY\nall, 3, 25.\nall, 1, -4.\n"
    # 16 steps of 6e-4 at the wave speed c = sqrt(E / rho) = 5e3: the front travels 48 of the bar's 120 length units
    write_dynamic_deck(path, nodes, el, "C3D4", nsets, step, dynamic="*Dynamic, direct\n%r, %r\n" % BAR_DT_T, initial=initial)
    return nodes, el


def energy(tmpdir, backend):
    """a clamped bar with an initial velocity and no loads, beta = 1/4, gamma = 1/2, 16 steps: kinetic + strain energy of
    every step equals that of t = 0.  `strain_energy` is `get_elasEng`, which in a dynamic run reports u.Ku / 2 (femcy_elastic_energy_small): with the
    reference's energy of the Green strain the sum drifts by the order of the strain (1.62e-3 here)."""
    path = os.path.join(str(tmpdir), "energy.inp")
    write_energy_deck(path)
    inp, system, U = solve_deck(path, backend)
    assert len(U) == 16 and inp.dynamic == {"beta": 0.25, "gamma": 0.5}
    e0 = system.initial_energy["kinetic"] + system.initial_energy["strain_energy"]
    assert system.initial_energy["strain_energy"] == 0.0 and e0 > 0
    drift = max(abs(i["kinetic"] + i["strain_energy"] - e0) / e0 for i in system.increments)
    moved = max(i["strain_energy"] for i in system.increments) / e0
    print(f"energy [{backend}]: drift {drift:.3e}, largest strain-energy share {moved:.3e}")
    assert moved > 0.01, "the bar must have exchanged energy"
    assert drift <= ENERGY_TOL, drift
    return drift


TRAJ = {"cload": dict(family="C3D4", cells=(2, 2, 3), beta=0.25, gamma=0.5, amplitude=None),
        "dsload": dict(family="CPS4", cells=(4, 3), beta=0.25, gamma=0.5, amplitude="RAMP"),
        "damped": dict(family="CPS8", cells=(3, 2), beta=0.3025, gamma=0.6, amplitude=None)}
TRAJ_DT, TRAJ_T = 2.0e-5, 3.2e-4


def write_traj_deck(path, case):
    spec = TRAJ[case]
    fam = spec["family"]
    nodes, el, ELE = lr.mesh(fam, cells=spec["cells"], perturb=0.0 if fam == "CPS8" else 0.2)
    foot = np.nonzero(nodes[:, 0] < 1e-12)[0]
    tip = np.nonzero(nodes[:, 0] > nodes[:, 0].max() - 1e-12)[0]
    nsets = {"foot": foot, "tip": tip}
    dm = nodes.shape[1]
    step = "*Boundary\n" + "".join("foot, %d, %d\n" % (d + 1, d + 1) for d in range(dm))
    surface = None
    elsets = None
    if case == "dsload":
        # the right-hand column of cells, their face S2 (local nodes 1-2) is the side x = max
        nx, ny = spec["cells"]
        right = np.arange(ny) * nx + nx - 1
        step += "*Dsload\nSurf-1, P, -3.5\n"
        elsets, surface = {"right": right}, ("Surf-1", "right", "S2")
    else:
        step += "*Cload\ntip, %d, 12.5\ntip, 1, -4.\n" % dm
    dyn = "*Dynamic, direct%s\n%.17g, %.17g\n" % ("" if spec["beta"] == 0.25 else ", beta=%r, gamma=%r" % (spec["beta"], spec["gamma"]),
                                                  TRAJ_DT, TRAJ_T)
    mat = "*Density\n%.17g,\n*Elastic\n%.17g, %.17g\n" % (RHO, E_MOD, NU)
    lc.write_deck(path, nodes, el, fam, nsets, mat, step, elsets=elsets, surface=surface)
    text = open(path).read()
    head = "*Step, name=Step-1%s, nlgeom=NO\n" % ("" if spec["amplitude"] is None else ", amplitude=" + spec["amplitude"])
    old = text[text.index("*Step, name=Step-1"):text.index("*Static\n") + len("*Static\n1., 1., 1e-05, 1.\n")]
    with open(path, "w") as f:
        f.write(text.replace(old, head + dyn))
    return nodes, el, ELE


@functools.lru_cache(maxsize=None)
def reference_trajectory(case, workdir):
    """-> (long-double U [17, n], error of the float64 restatement): K from the oracle, M from the restatement, the full
    load vector from the host backend's load kernels (the existing load pipeline, not under test here)"""
    from femcy_amd.reader import InpInfo
    from oracle import femcy_oracle as orc
    from oracle.elements import elem_def
    path = os.path.join(workdir, "ref_%s.inp" % case)
    nodes, el, ELE = write_traj_deck(path, case)
    inp = InpInfo(path)
    spec = TRAJ[case]
    dm = ELE.dm
    kind = "lin3d" if dm == 3 else "pstress"
    K = orc.assemble_K(orc.Topology(nodes, el, elem_def(spec["family"])), np.zeros(nodes.size), orc.Material(kind, (E_MOD, NU)).C).toarray()
    fixed = np.unique(np.concatenate([np.asarray(bc["node_set"]) * dm + bc["dof"] for bc in inp.dirichlet_bc_info]))
    f_full = np.zeros(nodes.size)
    for cl in inp.cload_info:
        f_full[np.asarray(cl["node_set"]) * dm + cl["dof"]] += cl["val"]
    if inp.neumann_bc_info:
        topo = orc.Topology(nodes, el, elem_def(spec["family"]))
        for nb in inp.neumann_bc_info:
            f_full += orc.neumann_rhs(topo, [list(f) for f in nb["face_set"]], nb["traction"], nb.get("direction"))
    assert np.abs(f_full).max() > 0
    force = (lambda t: f_full * (t / TRAJ_T)) if inp.amplitude == "RAMP" else (lambda t: f_full)
    out = {}
    for dtype in (LD, np.float64):
        M = out_M = dr.expand(dr.mass_matrix(nodes, el, ELE, RHO, dtype), dm)
        out[dtype] = dr.newmark(M, K, force, fixed, np.zeros(nodes.size), spec["beta"], spec["gamma"], TRAJ_DT, TRAJ_T, dtype)[0]
    ref = out[LD]
    ref.setflags(write=False)
    scale = np.abs(ref).max()
    a0 = 1.0 / (spec["beta"] * TRAJ_DT ** 2)
    free = np.setdiff1d(np.arange(nodes.size), fixed)        # the constrained rows are solved exactly (unit diagonal, r = 0)
    cond = float(np.linalg.cond((K + a0 * np.asarray(out_M, dtype=np.float64))[np.ix_(free, free)]))
    return ref, float(max(np.abs(out[np.float64][k] - ref[k]).max() for k in range(len(ref))) / scale), cond


def trajectory(tmpdir, case, backend):
    """max over the 16 steps of |u - u_ref|_inf / max |u_ref|_inf against the long-double restatement"""
    path = os.path.join(str(tmpdir), "%s.inp" % case)
    write_traj_deck(path, case)
    inp, system, U = solve_deck(path, backend)
    ref = reference_trajectory(case, str(tmpdir))[0]
    assert len(U) == 16 == len(ref) - 1 and inp.amplitude == (TRAJ[case]["amplitude"] or "STEP")
    assert inp.dynamic == {"beta": TRAJ[case]["beta"], "gamma": TRAJ[case]["gamma"]}
    err = float(max(np.abs(U[k] - ref[k + 1]).max() for k in range(16)) / np.abs(ref).max())
    print(f"{case} [{backend}]: trajectory error {err:.3e}")
    assert np.abs(ref[1]).max() > 0 and err <= TRAJ_TOL, err
    return err


def trajectory_pcg(tmpdir, case, backend):
    """the same trajectory with every solve of the driver on its PCG branch (cg_branch_from = 0: the branch of systems of at
    least 1e5 DOF), which a dynamic run takes with the tight setting eps = direct_eps = 1e-12 and not the static 1e-3.
    Bound: a solve stops at max|r| < eps max|r0|, so its solution is off by at most cond(K + a0 M) eps relatively in the
    2-norm, sqrt(n) times that in the maximum norm; the trapezoidal rule does not amplify what a step adds, so 16 steps
    add up to 16 sqrt(n) cond eps, on top of the rounding bound of the direct branch.  cond is that of the reference
    matrix on the free DOFs (numpy, float64)."""
    path = os.path.join(str(tmpdir), "%s_pcg.inp" % case)
    write_traj_deck(path, case)
    inp, system, U = solve_deck(path, backend, cg_branch_from=0)
    ref, _, cond = reference_trajectory(case, str(tmpdir))
    assert len(U) == 16 and system.stats["direct_solves"] == 0 and system.stats["cg_iterations"] > 0
    assert all(e["converged"] and e["rmax"] < 1.0e-12 * e["r0"] for e in system.cg_log if e["r0"] > 0)
    bound = 16.0 * np.sqrt(ref.shape[1]) * cond * 1.0e-12 + TRAJ_TOL
    err = float(max(np.abs(U[k] - ref[k + 1]).max() for k in range(16)) / np.abs(ref).max())
    print(f"{case} [{backend}]: PCG branch, {system.stats['cg_iterations']} iterations, cond {cond:.2e}, error {err:.3e} (bound {bound:.3e})")
    assert err <= bound, (err, bound)
    assert bound < 1.0e-6, "a static eps = 1e-3 would not fit under this bound"
    return err


def comm_refusal(backend):
    """once femcy_comm_init has run, every mass call returns FEMCY_EINVAL with a message (device only: the host backend has
    one rank and its femcy_comm_init never succeeds)"""
    nodes, el, ELE = shape_mesh("C3D8-64")
    ctx = make_ctx(nodes, el, ELE, backend)
    ms = ctx.mass(ELE, RHO)
    iface = np.arange(0, ctx.n, 7, dtype=np.int32)
    ctx.comm_init(0, 1, be.Context.comm_unique_id(), iface, np.arange(iface.size, dtype=np.int32), iface.size,
                  np.ones(ctx.n, dtype=np.uint8))
    for call in (lambda: ctx.mass(ELE, RHO), lambda: ctx.mass_get(ms), lambda: ctx.mass_apply(ms, be.VEC_DOF, be.VEC_RHS),
                 lambda: ctx.mass_add_to_K(ms, 1.0), lambda: ctx.mass_kinetic_energy(ms, be.VEC_VEL)):
        with pytest.raises(be.FemcyError, match="several ranks") as refused:
            call()
        assert refused.value.status == -1
    ctx.close()


def measure_f64_worst(workdir):
    """the constants at the top, as measured: the float64 restatement against the long-double one on the cases run here"""
    from oracle import femcy_oracle as orc
    from oracle.elements import elem_def
    wm = max(reference_mass(name)[1] for name in SHAPES)
    wa = 0.0
    rng = np.random.default_rng(7)
    for name in SHAPES:
        nodes, el, ELE = shape_mesh(name)
        x = rng.uniform(0.5, 1.5, nodes.size) * rng.choice([-1.0, 1.0], nodes.size)
        X = x.reshape(-1, ELE.dm)
        ref = reference_mass(name)[0] @ X.astype(LD)
        f64 = dr.mass_matrix(nodes, el, ELE, RHO, np.float64) @ X
        wa = max(wa, float(np.abs(f64 - ref).max() / np.abs(ref).max()))
    wt = max(reference_trajectory(case, workdir)[1] for case in TRAJ)
    # free flight and the energy of the restatement itself.  Free flight: the families the oracle assembles whose deck mesh
    # (flight_mesh) stays within the 300 DOF of the dense long-double solve: CPS3, CPS4, CPS6, CPS8, C3D4; CPE* run the
    # meshes of CPS* with another C, C3D10 has 1 029 DOF, and C3D8 / C3D6 the oracle does not assemble.  Their errors are
    # governed by the same condition of K + a0 M (the 3-D meshes are the better conditioned ones: 5e-11 against 5e-9)
    wf = we = 0.0
    for fam in ("CPS3", "CPS4", "CPS6", "CPS8", "C3D4", "C3D10"):
        nodes, el, ELE = flight_mesh(fam)
        if nodes.size > 300:
            continue
        dm = ELE.dm
        K = orc.assemble_K(orc.Topology(nodes, el, elem_def(fam)), np.zeros(nodes.size),
                           orc.Material("lin3d" if dm == 3 else "pstress", (E_MOD, NU)).C).toarray()
        M = dr.expand(dr.mass_matrix(nodes, el, ELE, RHO, np.float64), dm)
        g = np.zeros((len(nodes), dm))
        g[:, dm - 1] = -GRAV
        f = M @ g.ravel()
        U, _, _, times = dr.newmark(M, K, lambda t: f, [], np.zeros(nodes.size), 0.25, 0.5, 0.125, 1.0, np.float64)
        for u, t in zip(U[1:], times[1:]):
            want = (0.5 * t * t) * g.ravel()
            wf = max(wf, float(np.abs(u - want).max() / (0.5 * GRAV * t * t)))
    (nodes, el), ELE = bar_mesh(), lr.single("C3D4")[2]
    K = orc.assemble_K(orc.Topology(nodes, el, elem_def("C3D4")), np.zeros(nodes.size), orc.Material("lin3d", (E_MOD, NU)).C).toarray()
    M = dr.expand(dr.mass_matrix(nodes, el, ELE, RHO, np.float64), 3)
    fixed = (np.nonzero(nodes[:, 2] < 1e-12)[0][:, None] * 3 + np.arange(3)[None, :]).ravel()
    v0 = np.zeros((len(nodes), 3))
    v0[:, 2], v0[:, 0] = 25.0, -4.0
    U, V, _, _ = dr.newmark(M, K, lambda t: np.zeros(nodes.size), fixed, v0.ravel(), 0.25, 0.5, BAR_DT_T[0], BAR_DT_T[1], np.float64)
    en = [0.5 * v @ M @ v + 0.5 * u @ K @ u for u, v in zip(U, V)]
    we = max(abs(e - en[0]) / en[0] for e in en)
    ws = max(reference_small_energy(name)[1] for name in ENERGY_SHAPES)
    return {"mass": wm, "apply": wa, "flight": wf, "energy": float(we), "traj": wt, "small_energy": ws}


# ------------------------------------------------------------------------------------------ call log
class CallLog:
    """a thin wrapper around a Context that records the name of every ABI call"""

    def __init__(self, ctx):
        self.calls = []
        inner = ctx._call

        def logged(name, *args):
            self.calls.append(name)
            return inner(name, *args)

        ctx._call = logged
