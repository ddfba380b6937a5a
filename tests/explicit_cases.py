"""Explicit-dynamics scenarios written against the C ABI (femcy_amd.backend.Context) and the deck driver, so that the host
backend (tests/test_explicit_cpu.py, backend "cpu") and the device (tests/test_gpu_explicit.py, backend "hip") run the same
code.  Every function checks its own result and returns the figure it checked.

Bounds.  The reference is the restatement of tests/explicit_reference.py in np.longdouble.  The same restatement in float64
differs from it by rounding and summation order alone; the F64_WORST_* constants are the worst such differences on the very
cases run here (`measure_f64_worst`, asserted by tests/test_explicit_cpu.py), and a backend is held to 4 x that.  Errors are
relative to the largest entry of the reference."""
import functools
import os

import numpy as np
import pytest

from femcy_amd import backend as be
from femcy_amd.material_zoo import LinearIsotropic, LinearIsotropicPlaneStress, NeoHookean

import dynamic_cases as dc
import explicit_reference as er
import loads_cases as lc
import loads_reference as lr

LD = np.longdouble
EPS = float(np.finfo(np.float64).eps)
E_MOD, NU, RHO = dc.E_MOD, dc.NU, dc.RHO
# worst error of the float64 restatement against the long-double one (measure_f64_worst, as measured): the lumped mass
# 9.67e-16, one step 1.92e-15 (CPS4-65); per deck case over 200 steps, the trajectories (u and v) 6.62e-14 / 7.11e-15 /
# 9.86e-14 and the energy balances 1.56e-14 / 1.06e-14 / 9.61e-15 (bar / block / gravity)
F64_WORST_LUMPED = 9.7e-16
F64_WORST_STEP = 2.0e-15
F64_WORST_TRAJ = {"bar": 6.7e-14, "block": 7.2e-15, "gravity": 9.9e-14}
F64_WORST_ENERGY = {"bar": 1.6e-14, "block": 1.1e-14, "gravity": 9.7e-15}
LUMPED_TOL, STEP_TOL = 4.0 * F64_WORST_LUMPED, 4.0 * F64_WORST_STEP

# the meshes of dynamic_cases.SHAPES (63 / 64 / 65 / 130 nodes: eight nodes per 256-thread block of the node kernels, the
# last block partial; every family, perturbed or with curved sides) and the fan: 40 triangles round one hub, the smallest
# mesh whose hub takes the second trip of the gather's `k += 32` loop
SHAPES = list(dc.SHAPES) + ["fan"]
# (mesh, straight): every mesh as it is, and with straight sides / unperturbed cells (the fan has one shape)
LUMPED_CASES = [(name, straight) for name in SHAPES for straight in (False, True) if not (straight and name == "fan")]


def shape_mesh(name, straight=False):
    if name == "fan":
        return lr.fan(40)
    etype, cells, perturb = dc.SHAPES[name]
    return lr.mesh(etype, cells=cells, perturb=0.0 if straight else perturb)


def material_of(ELE):
    return LinearIsotropic(E_MOD, NU) if ELE.dm == 3 else LinearIsotropicPlaneStress(E_MOD, NU)      # lc.make_ctx's


def held_dofs(nodes):
    """the DOFs of the nodes on x = min: (node ids, scalar DOFs)"""
    foot = np.nonzero(nodes[:, 0] < nodes[:, 0].min() + 1e-12)[0]
    dm = nodes.shape[1]
    return foot, (foot[:, None] * dm + np.arange(dm)[None, :]).ravel()


# ------------------------------------------------------------------------------------- the lumped mass
@functools.lru_cache(maxsize=None)
def reference_lumped(name, straight):
    nodes, el, ELE = shape_mesh(name, straight)
    ref = er.lumped_mass(nodes, el, ELE, RHO, LD)
    f64 = er.lumped_mass(nodes, el, ELE, RHO, np.float64)
    ref.setflags(write=False)
    return ref, float(np.abs(f64 - ref).max() / np.abs(ref).max())


def lumped(name, straight, backend):
    """sum = rho V, every mass positive (the corners of C3D10 / CPS6 / CPS8 included), the long-double HRZ restatement,
    re-creation bit-equal"""
    nodes, el, ELE = shape_mesh(name, straight)
    ctx = lc.make_ctx(nodes, el, ELE, backend)
    m = ctx.lumped_mass_get(ctx.lumped_mass(ELE, RHO))
    m2 = ctx.lumped_mass_get(ctx.lumped_mass(ELE, RHO))
    ctx.close()
    assert np.array_equal(m.view(np.uint64), m2.view(np.uint64)), "re-creation must give the same bits"
    assert m.shape == (len(nodes),) and (m > 0).all(), m.min()
    ref, _ = reference_lumped(name, straight)
    err = float(np.abs(m - ref).max() / np.abs(ref).max())
    V = float(er.mesh_volume(nodes, el, ELE))
    ev = abs(float(m.astype(LD).sum()) - RHO * V) / (RHO * V)
    print(f"{name}{' straight' if straight else ''} [{backend}]: {len(nodes)} nodes, lumped mass {err:.3e}, total {ev:.3e}")
    assert err <= LUMPED_TOL, err
    assert ev <= LUMPED_TOL, ev                                    # every entry within the bound, so their sum is
    return err


def single_element(etype, backend):
    """one straight CPS3 / C3D4: every node carries m_e / npe"""
    nodes, el, ELE, V = lr.single(etype)
    ctx = lc.make_ctx(nodes, el, ELE, backend)
    m = ctx.lumped_mass_get(ctx.lumped_mass(ELE, RHO))
    ctx.close()
    err = float(np.abs(m - RHO * V / len(nodes)).max() / (RHO * V / len(nodes)))
    assert err <= LUMPED_TOL, err
    return err


# ------------------------------------------------------------------------------------------ one step
STEP_SHAPES = ["fan", "C3D4", "C3D4-150", "C3D10", "CPS4-65"]


def step_setup(name):
    """-> nodes, el, ELE, held DOFs, f, u0, v0, h, s: a state with strains of a few per cent"""
    nodes, el, ELE = shape_mesh(name)
    rng = np.random.default_rng(11)
    _, fixed = held_dofs(nodes)
    size = np.ptp(nodes, axis=0).max()
    u0 = 0.01 * size * rng.uniform(-1.0, 1.0, nodes.size)
    v0 = rng.uniform(-1.0, 1.0, nodes.size)
    f = rng.uniform(-1.0, 1.0, nodes.size)
    u0[fixed] = v0[fixed] = 0.0
    return nodes, el, ELE, fixed, f, u0, v0, 1.0e-5, 0.75


@functools.lru_cache(maxsize=None)
def reference_step(name):
    """error of the float64 restatement of one step (u, v, a of the new state) against the long-double one"""
    nodes, el, ELE, fixed, f, u0, v0, h, s = step_setup(name)
    out = {}
    for dt in (LD, np.float64):
        mdl = er.Model(nodes, el, ELE, material_of(ELE), dt)
        minv = 1 / np.repeat(er.lumped_mass(nodes, el, ELE, RHO, dt), ELE.dm)
        minv[fixed] = 0
        u0d, v0d, fd, hd = np.asarray(u0, dtype=dt), np.asarray(v0, dtype=dt), np.asarray(f, dtype=dt), dt(h)
        a0 = minv * (dt(s) * fd - mdl.f_int(u0d))
        u1 = u0d + hd * v0d + (hd * hd / 2) * a0
        a1 = minv * (dt(s) * fd - mdl.f_int(u1))
        out[dt] = (u1, v0d + (hd / 2) * (a0 + a1), a1)
    return max(float(np.abs(np.asarray(x64, dtype=LD) - x).max() / np.abs(x).max()) for x64, x in zip(out[np.float64], out[LD]))


def make_explicit(ctx, ELE, fixed):
    lm = ctx.lumped_mass(ELE, RHO)
    return lm, ctx.explicit(lm, [ctx.dofset(fixed)] if len(fixed) else [])


def one_step(name, backend):
    """femcy_explicit_start + one femcy_explicit_advance(1) against femcy_internal_force + the same arithmetic on the host:
    the fused node pass is the node gather of k_nodal_force and four vector kernels"""
    nodes, el, ELE, fixed, f, u0, v0, h, s = step_setup(name)
    ctx = lc.make_ctx(nodes, el, ELE, backend)
    if name == "fan":
        assert ctx.pattern_info().max_node_elems == 40
    lm, ex = make_explicit(ctx, ELE, fixed)
    minv = 1.0 / np.repeat(ctx.lumped_mass_get(lm), ELE.dm)
    minv[fixed] = 0.0
    for vec, arr in ((be.VEC_DOF, u0), (be.VEC_VEL, v0), (be.VEC_RHS, f)):
        ctx.upload(vec, arr)
    ctx.explicit_start(ex, be.VEC_RHS, s)
    a0 = ctx.download(be.VEC_ACC)
    assert np.array_equal(ctx.download(be.VEC_DOF), u0) and np.array_equal(ctx.download(be.VEC_VEL), v0)
    ctx.internal_force(be.VEC_DOF, be.VEC_FORCE)
    want_a0 = minv * (s * f - ctx.download(be.VEC_FORCE))
    ctx.explicit_advance(ex, 1, h, be.VEC_RHS, s, 0.0)
    got = [ctx.download(v) for v in (be.VEC_DOF, be.VEC_VEL, be.VEC_ACC)]
    assert np.array_equal(ctx.download(be.VEC_RHS), f), "the load vector is read only"
    u1 = u0 + h * v0 + (h * h / 2) * a0
    ctx.upload(be.VEC_TMP0, u1)
    ctx.internal_force(be.VEC_TMP0, be.VEC_FORCE)
    a1 = minv * (s * f - ctx.download(be.VEC_FORCE))
    want = [u1, v0 + (h / 2) * (a0 + a1), a1]
    ke = ctx.explicit_kinetic_energy(ex, be.VEC_VEL)
    ke2 = ctx.explicit_kinetic_energy(ex, be.VEC_VEL)
    want_ke = float(er.kinetic(ctx.lumped_mass_get(lm), got[1], ELE.dm, LD))
    ctx.close()
    err = max(float(np.abs(g - w).max() / np.abs(w).max()) for g, w in zip([a0] + got, [want_a0] + want))
    ek = abs(ke - want_ke) / want_ke
    print(f"{name} [{backend}]: one step against the composition {err:.3e}, kinetic energy {ek:.3e}")
    assert ke == ke2, "the reduction has a fixed order"
    assert np.abs(want[2]).max() > 0 and err <= STEP_TOL, err
    assert ek <= (len(nodes) + 4) * EPS, ek                        # a sum of nn positive terms of a few operations each
    return err


# ------------------------------------------------------------------------------- splitting, held DOFs
def split(ramp, backend, name="C3D4-150"):
    """advance(7) + advance(5) against advance(12), bit for bit on u, v and a.  RAMP: s_k = k / 16, sums that are exact in
    float64, so that the second call's scale0 = s_7 carries the bits the single call reaches"""
    nodes, el, ELE, fixed, f, u0, v0, h, _ = step_setup(name)
    s0, ds = (0.0, 1.0 / 16.0) if ramp else (1.0, 0.0)
    ctx = lc.make_ctx(nodes, el, ELE, backend)
    _, ex = make_explicit(ctx, ELE, fixed)
    ctx.upload(be.VEC_RHS, f)
    runs = []
    for parts in ((12,), (7, 5)):
        ctx.upload(be.VEC_DOF, u0)
        ctx.upload(be.VEC_VEL, v0)
        ctx.explicit_start(ex, be.VEC_RHS, s0)
        done = 0
        for k in parts:
            ctx.explicit_advance(ex, k, h, be.VEC_RHS, s0 + done * ds, ds)
            done += k
        runs.append([ctx.download(v) for v in (be.VEC_DOF, be.VEC_VEL, be.VEC_ACC)])
    ctx.explicit_advance(ex, 0, h, be.VEC_RHS, 1.0, 0.0)           # no step: nothing moves
    assert np.array_equal(ctx.download(be.VEC_DOF), runs[1][0])
    ctx.close()
    assert not np.array_equal(runs[0][0], u0)
    for whole, parts, what in zip(runs[0], runs[1], "uva"):
        assert np.array_equal(whole.view(np.uint64), parts.view(np.uint64)), what


def constrained(backend, name="C3D8-64"):
    """the held DOFs stay exactly 0.0 in u, v and a through 50 steps under load"""
    nodes, el, ELE, fixed, f, u0, v0, h, s = step_setup(name)
    assert np.abs(f[fixed]).min() > 0                               # they are loaded
    ctx = lc.make_ctx(nodes, el, ELE, backend)
    _, ex = make_explicit(ctx, ELE, fixed)
    for vec, arr in ((be.VEC_DOF, u0), (be.VEC_VEL, v0), (be.VEC_RHS, f)):
        ctx.upload(vec, arr)
    ctx.explicit_start(ex, be.VEC_RHS, s)
    ctx.explicit_advance(ex, 50, h, be.VEC_RHS, s, 0.0)
    state = [ctx.download(v) for v in (be.VEC_DOF, be.VEC_VEL, be.VEC_ACC)]
    ctx.close()
    for x in state:
        assert (x[fixed] == 0.0).all() and np.isfinite(x).all() and np.abs(x).max() > 0


# ---------------------------------------------------------------------------------------------- decks
def write_explicit_deck(path, nodes, el, family, nsets, step, dynamic, amplitude=None, material=None, initial="", nlgeom=False,
                        elsets=None, surface=None):
    """lc.write_deck with the `*Static` block replaced by `dynamic` (dc.write_dynamic_deck, with element sets)"""
    mat = material if material is not None else "*Density\n%.17g,\n*Elastic\n%.17g, %.17g\n" % (RHO, E_MOD, NU)
    lc.write_deck(path, nodes, el, family, nsets, mat + initial, step, elsets=elsets, surface=surface, nlgeom=nlgeom)
    text = open(path).read()
    head = "*Step, name=Step-1%s, nlgeom=%s\n" % ("" if amplitude is None else ", amplitude=" + amplitude, "YES" if nlgeom else "NO")
    old = text[text.index("*Step, name=Step-1"):text.index("*Static\n") + len("*Static\n1., 1., 1e-05, 1.\n")]
    with open(path, "w") as f:
        f.write(text.replace(old, head + dynamic))


NEO = dict(C1=80.0, D1=400.0, rho=2.0)
CASES = {"bar": dict(dt=1.0e-4, steps=200, amplitude=None), "block": dict(dt=2.0e-3, steps=200, amplitude="STEP"),
         "gravity": dict(dt=5.0e-4, steps=200, amplitude="RAMP")}
SOFT_E = 2.0e2     # the gravity plate: soft enough for strains of 1e-3 (at 1e-6 the Green strain F^T F - I loses ten digits)
EVERY = 8


def write_case_deck(path, case, dynamic=None):
    """bar: the clamped C3D4 column of dynamic_cases released from an initial velocity, linear material.  block: a
    neo-Hookean C3D8 block clamped at z = 0 under a step traction on z = max.  gravity: a plane-stress CPS4 plate held on
    x = 0 under ramped gravity.  -> nodes, el, ELE, material"""
    spec = CASES[case]
    if dynamic is None:
        dynamic = "*Dynamic, explicit, direct user control, output_every=%d\n%r, %r\n" % (EVERY, spec["dt"], spec["dt"] * spec["steps"])
    if case == "bar":
        nodes, el = dc.bar_mesh()
        nsets = {"all": np.arange(len(nodes)), "foot": np.nonzero(nodes[:, 2] < 1e-12)[0]}
        write_explicit_deck(path, nodes, el, "C3D4", nsets, "*Boundary\nfoot, 1, 1\nfoot, 2, 2\nfoot, 3, 3\n", dynamic,
                            initial="*Initial Conditions, type=VELOCITY\nall, 3, 25.\nall, 1, -4.\n")
        return nodes, el, lr.single("C3D4")[2], LinearIsotropic(E_MOD, NU)
    if case == "block":
        from femcy_amd import meshgen
        from femcy_amd.element_zoo import Element_linear_hexahedral
        nodes, el = meshgen.plate_hex(2, 2, 3, perturb=0.2, seed=6, box=(1.0, 1.0, 2.0))
        ELE = Element_linear_hexahedral()
        face = next(k + 1 for k, f in enumerate(ELE.inp_surface_num) if set(f[0]) == {4, 5, 6, 7})
        nsets = {"foot": np.nonzero(nodes[:, 2] < 1e-12)[0]}
        mat = "*Density\n%r,\n*Hyperelastic, neo hooke\n%r, %r\n" % (NEO["rho"], NEO["C1"], 1.0 / NEO["D1"])
        write_explicit_deck(path, nodes, el, "C3D8", nsets, "*Boundary\nfoot, 1, 1\nfoot, 2, 2\nfoot, 3, 3\n*Dsload\nend, P, -14.\n",
                            dynamic, amplitude=spec["amplitude"], material=mat, elsets={"_end": np.arange(len(el))[-4:]},
                            surface=("end", "_end", "S%d" % face))
        return nodes, el, ELE, NeoHookean(C1=NEO["C1"], D1=NEO["D1"])
    nodes, el, ELE = lr.mesh("CPS4", cells=(4, 3), perturb=0.2)
    nsets = {"foot": np.nonzero(nodes[:, 0] < 1e-12)[0]}
    write_explicit_deck(path, nodes, el, "CPS4", nsets, "*Boundary\nfoot, 1, 1\nfoot, 2, 2\n*Dload\n, GRAV, 9.81, 0., -1.\n", dynamic,
                        amplitude=spec["amplitude"], material="*Density\n%.17g,\n*Elastic\n%.17g, %.17g\n" % (RHO, SOFT_E, NU))
    return nodes, el, ELE, LinearIsotropicPlaneStress(SOFT_E, NU)


def solve_deck(path, backend):
    """-> inp, system (closed), u and v after every batch [records, n]"""
    from femcy_amd.body import Body
    from femcy_amd.reader import InpInfo
    from femcy_amd.stiffnessMtrx import System_of_equations
    inp = InpInfo(path)
    body = Body(nodes=inp.nodes, elements=list(inp.eSets.values())[0], ELE=inp.ELE)
    system = System_of_equations(body, list(inp.materials.values())[0], inp.geometric_nonlinear, verbose=False,
                                 ctx=be.Context(0, backend=backend))
    U, V, advance = [], [], system.ctx.explicit_advance

    def recording(*a, **kw):
        advance(*a, **kw)
        U.append(system.dof.to_numpy())
        V.append(system.ctx.download(be.VEC_VEL))

    system.ctx.explicit_advance = recording
    try:
        system.solve(inp)
    finally:
        system.ctx.close()
    return inp, system, np.array(U), np.array(V)


def deck_loads(path):
    """the load vector at scale 1, v_0 and the held DOFs of a deck, through the reader and the host backend's load kernels
    (the existing load pipeline, not under test here)"""
    from femcy_amd.body import Body
    from femcy_amd.reader import InpInfo
    from femcy_amd.stiffnessMtrx import System_of_equations
    import copy
    inp = InpInfo(path)
    dm = int(inp.ELE.dm)
    system = System_of_equations(Body(nodes=inp.nodes, elements=list(inp.eSets.values())[0], ELE=inp.ELE),
                                 list(inp.materials.values())[0], False, verbose=False, ctx=be.Context(0, backend="cpu"))
    loads = {"neumannBCs": copy.deepcopy(inp.neumann_bc_info), "dirichletBCs": [],
             "bodyForces": copy.deepcopy(inp.body_force_info or []), "cloads": copy.deepcopy(inp.cload_info or [])}
    system.rhs.fill(0.0)
    system.impose_boundary_condition(loads)
    f = system.rhs.to_numpy()
    system.ctx.close()
    v0 = np.zeros(inp.nodes.size)
    for iv in inp.initial_velocity_info:
        v0[np.asarray(iv["node_set"]) * dm + iv["dof"]] = iv["val"]
    fixed = np.unique(np.concatenate([np.asarray(bc["node_set"]) * dm + bc["dof"] for bc in inp.dirichlet_bc_info]))
    return inp, f, v0, fixed


@functools.lru_cache(maxsize=None)
def reference_case(case, workdir):
    """-> dict: long-double U, V at the records, the energy balance there, the errors of the float64 restatement, the
    largest stretch |F - I| reached"""
    path = os.path.join(workdir, "ref_%s.inp" % case)
    nodes, el, ELE, mat = write_case_deck(path, case)
    inp, f, v0, fixed = deck_loads(path)
    spec = CASES[case]
    rho = inp.density
    T = spec["dt"] * spec["steps"]
    scale = (lambda k: k * spec["dt"] / T) if inp.amplitude == "RAMP" else (lambda k: 1.0)
    out = {}
    for dt in (LD, np.float64):
        mdl = er.Model(nodes, el, ELE, mat, dt)
        m = er.lumped_mass(nodes, el, ELE, rho, dt)
        minv = 1 / np.repeat(m, ELE.dm)
        minv[fixed] = 0
        U, V, _ = mdl.verlet(minv, f, v0, spec["dt"], spec["steps"], scale)
        rec = np.arange(EVERY, spec["steps"] + 1, EVERY)
        hist = balance(U[rec], [er.kinetic(m, v, ELE.dm, dt) for v in V[rec]], [mdl.energy(u) for u in U[rec]], f,
                       [scale(k) for k in rec], dt)
        out[dt] = (U[rec], V[rec], hist, mdl)
    U, V, hist, mdl = out[LD]
    U64, V64, hist64, _ = out[np.float64]
    stretch = float(max(np.abs(mdl._state(u)[1] - np.eye(ELE.dm)).max() for u in U))
    escale = max(float(h[1]) for h in hist)
    return {"U": U, "V": V, "hist": hist, "escale": escale, "stretch": stretch,
            "traj64": max(float(np.abs(U64 - U).max() / np.abs(U).max()), float(np.abs(V64 - V).max() / np.abs(V).max())),
            "energy64": max(abs(float(a[0] - b[0])) for a, b in zip(hist64, hist)) / escale}


def balance(U, kinetic, strain, f, scales, dtype):
    """[(kinetic + strain - external work, kinetic + strain)] at the records; the work of the dead load s f by the trapezoidal
    rule over the records, from the state u = 0 at scale s_0 = scales[0] - (scales[1] - scales[0]) (RAMP) or 1"""
    f = np.asarray(f, dtype=dtype)
    work, out = dtype(0), []
    u_prev = np.zeros_like(f)
    s_prev = dtype(scales[0] - (scales[1] - scales[0])) if scales[1] != scales[0] else dtype(scales[0])
    for u, k, e, s in zip(U, kinetic, strain, scales):
        u = np.asarray(u, dtype=dtype)
        work = work + (dtype(s) + s_prev) / 2 * (f @ (u - u_prev))
        out.append((dtype(k) + dtype(e) - work, dtype(k) + dtype(e)))
        u_prev, s_prev = u, dtype(s)
    return out


def trajectory(tmpdir, case, backend):
    """u and v after every batch of 8 of the 200 steps against the long-double restatement, and the energy balance kinetic +
    strain - external work of those records against the restatement's"""
    path = os.path.join(str(tmpdir), "%s.inp" % case)
    nodes, el, ELE, mat = write_case_deck(path, case)
    inp, system, U, V = solve_deck(path, backend)
    spec = CASES[case]
    ref = reference_case(case, str(tmpdir))
    assert inp.procedure == "explicit" and inp.amplitude == (spec["amplitude"] or "STEP")
    assert len(U) == spec["steps"] // EVERY == len(system.increments) and system.increments[-1]["kinc"] == spec["steps"]
    assert system.increments[-1]["time1"] == inp.time_incs["max_time"] and system.dt <= spec["dt"]
    assert abs(system.dt - spec["dt"]) <= 4 * EPS * spec["dt"]
    eu = float(np.abs(U - ref["U"]).max() / np.abs(ref["U"]).max())
    ev = float(np.abs(V - ref["V"]).max() / np.abs(ref["V"]).max())
    _, f, _, _ = deck_loads(path)
    T = inp.time_incs["max_time"]
    scales = [i["time1"] / T if inp.amplitude == "RAMP" else 1.0 for i in system.increments]
    hist = balance(U, [i["kinetic"] for i in system.increments], [i["strain_energy"] for i in system.increments], f, scales, LD)
    ee = max(abs(float(a[0] - b[0])) for a, b in zip(hist, ref["hist"])) / ref["escale"]
    print(f"{case} [{backend}]: trajectory u {eu:.3e}, v {ev:.3e}, energy balance {ee:.3e}, largest |F - I| {ref['stretch']:.3f}")
    if case == "block":
        assert 0.05 <= ref["stretch"] <= 0.10, ref["stretch"]      # finite strain, as the reference measures it
    assert max(eu, ev) <= 4.0 * F64_WORST_TRAJ[case], (eu, ev)
    assert ee <= 4.0 * F64_WORST_ENERGY[case], ee
    return max(eu, ev), ee


# ------------------------------------------------------------------------------------ stable increment
def omega_bound(name, backend):
    """omega_bound against Gershgorin's bound in numpy on the backend's own K and lumped mass, and above the largest
    eigenfrequency of M_L^-1 K on the free DOFs (which holds by Gershgorin).  Rounding bound: a row sum of W non-negative
    terms carries at most (W - 1) eps, the product with minv and the square root two more roundings"""
    nodes, el, ELE = shape_mesh(name)
    _, fixed = held_dofs(nodes)
    ctx = lc.make_ctx(nodes, el, ELE, backend)
    lm, ex = make_explicit(ctx, ELE, fixed)
    ctx.assemble_K(-1)
    K = ctx.get_K_bsr().toarray()
    minv = 1.0 / np.repeat(ctx.lumped_mass_get(lm), ELE.dm)
    minv[fixed] = 0.0
    dt, om = ctx.explicit_stable_dt(ex)
    width = ctx.pattern_info().max_row_blocks * ELE.dm
    ctx.close()
    want = er.gershgorin(K, minv)
    free = np.setdiff1d(np.arange(nodes.size), fixed)
    true = float(np.sqrt(np.linalg.eigvals(minv[free, None] * K[np.ix_(free, free)]).real.max()))
    err = abs(om - want) / want
    print(f"{name} [{backend}]: omega bound {om:.6e} (numpy {err:.1e}), largest eigenfrequency {true:.6e}, dt {dt:.3e}")
    assert err <= (width + 2) * EPS, err
    assert om >= true and dt == 2.0 / om
    return om / true


def bar_setup(workdir):
    """the bar of the trajectory case: -> (dt estimated by the host backend, 2 / omega_true by a dense eigenvalue)"""
    path = os.path.join(workdir, "bar_setup.inp")
    nodes, el, ELE, mat = write_case_deck(path, "bar")
    _, _, _, fixed = deck_loads(path)
    ctx = lc.make_ctx(nodes, el, ELE, "cpu")
    lm, ex = make_explicit(ctx, ELE, fixed)
    ctx.assemble_K(-1)
    K = ctx.get_K_bsr().toarray()
    minv = 1.0 / np.repeat(ctx.lumped_mass_get(lm), 3)
    dt, _ = ctx.explicit_stable_dt(ex)
    ctx.close()
    free = np.setdiff1d(np.arange(nodes.size), fixed)
    return dt, 2.0 / float(np.sqrt(np.linalg.eigvals(minv[free, None] * K[np.ix_(free, free)]).real.max()))


def stays_finite(tmpdir, backend):
    """the driver's own estimate at scale factor = 1 carries the bar through 500 steps"""
    dt, _ = bar_setup(str(tmpdir))
    path = os.path.join(str(tmpdir), "auto.inp")
    write_case_deck(path, "bar", dynamic="*Dynamic, explicit\n, %r\n" % (500 * dt))
    inp, system, U, V = solve_deck(path, backend)
    assert inp.time_incs["ini_inc"] is None and inp.dynamic == {"direct_user_control": False, "scale_factor": 1.0, "output_every": 64}
    assert system.increments[-1]["kinc"] == 500 and len(U) == 8 and [i["kinc"] for i in system.increments][:2] == [64, 128]
    assert abs(system.stable_dt - dt) <= 64 * EPS * dt and system.dt <= system.stable_dt
    e0 = system.initial_energy["kinetic"]
    assert np.isfinite(U).all() and np.abs(U).max() > 0 and e0 > 0
    assert all(np.isfinite(i["kinetic"]) and i["kinetic"] + i["strain_energy"] < 2 * e0 for i in system.increments)


UNSTABLE_STEPS = 1500


@functools.lru_cache(maxsize=None)
def reference_blows_up(workdir):
    """the long-double restatement at 1.1 x 2 / omega_true: the displacements leave the range of float64"""
    _, crit = bar_setup(workdir)
    path = os.path.join(workdir, "ref_unstable.inp")
    nodes, el, ELE, mat = write_case_deck(path, "bar")
    inp, f, v0, fixed = deck_loads(path)
    minv = 1 / np.repeat(er.lumped_mass(nodes, el, ELE, inp.density, LD), 3)
    minv[fixed] = 0
    with np.errstate(all="ignore"):
        U, _, _ = er.Model(nodes, el, ELE, mat, LD).verlet(minv, f, v0, 1.1 * crit, UNSTABLE_STEPS, lambda k: 1.0)
    return not np.isfinite(np.abs(U[-1]).max().astype(np.float64))


def unstable(tmpdir, backend):
    """a fixed increment of 1.1 x 2 / omega_true: the driver raises FEMCY_ENUMERIC and does not go on"""
    assert reference_blows_up(str(tmpdir)), "the reference must show the blow-up first"
    _, crit = bar_setup(str(tmpdir))
    path = os.path.join(str(tmpdir), "unstable.inp")
    dt = 1.1 * crit
    write_case_deck(path, "bar", dynamic="*Dynamic, explicit, direct user control\n%r, %r\n" % (dt, UNSTABLE_STEPS * dt))
    with pytest.raises(be.FemcyError, match="unstable increment") as raised:
        solve_deck(path, backend)
    assert raised.value.status == be.FEMCY_ENUMERIC


# --------------------------------------------------------------------------------------------- refusals
def refusals(backend):
    """every refusal returns FEMCY_EINVAL with a message, and the context keeps working"""
    import ctypes as C
    nodes, el, ELE = shape_mesh("C3D8")
    _, fixed = held_dofs(nodes)
    ctx = lc.make_ctx(nodes, el, ELE, backend, pattern=False)
    with pytest.raises(be.FemcyError, match="pattern"):
        ctx.lumped_mass(ELE, RHO)
    ctx.build_pattern()
    for bad in (np.nan, np.inf, 0.0, -1.0):
        with pytest.raises(be.FemcyError, match="density"):
            ctx.lumped_mass(ELE, bad)
    t = ELE.mass_tables()
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    out = C.c_int32()
    for args in ((None, ptr(t["dNq"]), ptr(t["wq"])), (ptr(t["Nq"]), None, ptr(t["wq"])), (ptr(t["Nq"]), ptr(t["dNq"]), None)):
        with pytest.raises(be.FemcyError, match="null"):
            ctx._call("femcy_lumped_mass_create", t["nq"], args[0], args[1], args[2], RHO, C.byref(out))
    for nq in (0, 65):
        with pytest.raises(be.FemcyError, match="points"):
            ctx._call("femcy_lumped_mass_create", nq, ptr(t["Nq"]), ptr(t["dNq"]), ptr(t["wq"]), RHO, C.byref(out))
    lm, ex = make_explicit(ctx, ELE, fixed)
    calls = [(lambda: ctx.lumped_mass_get(lm + 1), "unknown lumped mass"), (lambda: ctx.explicit(lm + 1), "unknown lumped mass"),
             (lambda: ctx.explicit(lm, [99]), "unknown DOF set"),
             (lambda: ctx.explicit_start(ex + 1), "unknown explicit integrator"),
             (lambda: ctx.explicit_advance(-1, 1, 1e-5), "unknown explicit integrator"),
             (lambda: ctx.explicit_kinetic_energy(ex + 1), "unknown explicit integrator"),
             (lambda: ctx.explicit_stable_dt(ex + 1), "unknown explicit integrator"),
             (lambda: ctx.explicit_advance(ex, -1, 1e-5), "-1 steps"),
             (lambda: ctx.explicit_stable_dt(ex), "assemble first")]
    calls += [(lambda bad=bad: ctx.explicit_advance(ex, 1, bad), "increment") for bad in (0.0, -1e-5, np.nan, np.inf)]
    calls += [(lambda v=v: ctx.explicit_advance(ex, 1, 1e-5, v), "state vectors") for v in (be.VEC_DOF, be.VEC_VEL, be.VEC_ACC)]
    calls += [(lambda v=v: ctx.explicit_start(ex, v), "state vectors") for v in (be.VEC_DOF, be.VEC_VEL, be.VEC_ACC)]
    for call, message in calls:
        with pytest.raises(be.FemcyError, match=message) as refused:
            call()
        assert refused.value.status == -1, message                 # FEMCY_EINVAL
    assert not np.abs(ctx.download(be.VEC_DOF)).any() and not np.abs(ctx.download(be.VEC_ACC)).any()     # nothing moved
    ctx.upload(be.VEC_VEL, np.ones(nodes.size))                    # the context still works
    assert ctx.explicit_kinetic_energy(ex) > 0
    ctx.assemble_K(-1)
    assert ctx.explicit_stable_dt(ex)[0] > 0
    ctx.build_pattern()                                            # a new pattern has no matrix yet
    with pytest.raises(be.FemcyError, match="assemble first"):
        ctx.explicit_stable_dt(ex)
    ctx.set_mesh(nodes, el)                                        # a new mesh drops the objects
    with pytest.raises(be.FemcyError, match="unknown explicit integrator"):
        ctx.explicit_kinetic_energy(ex)
    with pytest.raises(be.FemcyError, match="unknown lumped mass"):
        ctx.lumped_mass_get(lm)
    ctx.close()


def comm_refusal(backend):
    """once femcy_comm_init has run, every call of the feature returns FEMCY_EINVAL with a message (device only: the host
    backend has one rank and its femcy_comm_init never succeeds)"""
    nodes, el, ELE = shape_mesh("C3D8-64")
    ctx = lc.make_ctx(nodes, el, ELE, backend)
    lm, ex = make_explicit(ctx, ELE, held_dofs(nodes)[1])
    ctx.assemble_K(-1)
    iface = np.arange(0, ctx.n, 7, dtype=np.int32)
    ctx.comm_init(0, 1, be.Context.comm_unique_id(), iface, np.arange(iface.size, dtype=np.int32), iface.size,
                  np.ones(ctx.n, dtype=np.uint8))
    for call in (lambda: ctx.lumped_mass(ELE, RHO), lambda: ctx.lumped_mass_get(lm), lambda: ctx.explicit(lm),
                 lambda: ctx.explicit_start(ex), lambda: ctx.explicit_advance(ex, 1, 1e-5),
                 lambda: ctx.explicit_kinetic_energy(ex), lambda: ctx.explicit_stable_dt(ex)):
        with pytest.raises(be.FemcyError, match="several ranks") as refused:
            call()
        assert refused.value.status == -1
    ctx.close()


def measure_f64_worst(workdir):
    """the constants at the top, as measured: the float64 restatement against the long-double one on the cases run here"""
    wl = max(reference_lumped(name, straight)[1] for name, straight in LUMPED_CASES)
    ws = max(reference_step(name) for name in STEP_SHAPES)
    refs = {case: reference_case(case, workdir) for case in CASES}
    return {"lumped": wl, "step": ws, "traj": {c: r["traj64"] for c, r in refs.items()},
            "energy": {c: r["energy64"] for c, r in refs.items()}}
