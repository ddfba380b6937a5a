"""Scenarios of the element-by-element increment of explicit dynamics (`*Dynamic, explicit, element by element`;
femcy_explicit_element_bound, femcy_explicit_auto_*), written against the C ABI and the deck driver so that the host backend
(tests/test_explicit_auto_cpu.py) and the device (tests/test_gpu_explicit_auto.py) run the same code.

The reference is the numpy restatement below in np.longdouble, written from the definition

    g_e       = sum_q v_q sum_a |grad_x N_a(xi_q)|^2 / m_a^e,        v_q = |det J_x(xi_q)| w_q  at x = X + u
    omega_e^2 = sum_q v_q (s_C + |sigma_q|_F) sum_a |grad_x N_a(xi_q)|^2 / m_a^e,     omega = sqrt(max_e omega_e^2)
    h_n = min(sf 2 / omega(u_n), T - t_n),  t_{n+1} = T when h_n took the remainder, else t_n + h_n
    u_{n+1} = u_n + h_n v_n + h_n^2 / 2 a_n;  a_{n+1} = minv (s(t_{n+1}) f - f_int(u_{n+1}));  v_{n+1} = v_n + h_n / 2 (a_n + a_{n+1})

with explicit_reference's tables, stress laws and internal force.  Bounds follow explicit_cases: the same restatement in
float64 differs from the long-double one by rounding alone, the F64_WORST_* constants are the worst such differences on the
cases run here (`measure_f64_worst`, asserted by tests/test_explicit_auto_cpu.py) and a backend is held to 4 x that."""
import functools
import os

import numpy as np
import pytest

from femcy_amd import backend as be
from femcy_amd.material_zoo import (LinearIsotropic, LinearIsotropicPlaneStrain, LinearIsotropicPlaneStress, NeoHookean,
                                    NeoHookeanPlaneStrain)

import explicit_cases as ec
import explicit_reference as er
import loads_cases as lc

LD = np.longdouble
EPS = ec.EPS
RHO = ec.RHO
# worst error of the float64 restatement against the long-double one (measure_f64_worst, as measured on the CPU): omega over
# every case of BOUND_CASES 4.57e-16; per deck case the increments (and the clock) 2.28e-15 / 2.28e-15 / 7.35e-15 / 1.84e-14,
# the trajectories (u and v) 1.33e-13 / 1.33e-13 / 7.71e-15 / 3.63e-14 and the energy balances 1.57e-14 / 1.57e-14 /
# 9.86e-15 / 2.59e-14 (bar-STEP / bar-RAMP / block-STEP / block-RAMP; the bar carries no load, so its two runs agree)
F64_WORST_BOUND = 4.6e-16
F64_WORST_H = {"bar-STEP": 2.3e-15, "bar-RAMP": 2.3e-15, "block-STEP": 7.4e-15, "block-RAMP": 1.9e-14}
F64_WORST_TRAJ = {"bar-STEP": 1.4e-13, "bar-RAMP": 1.4e-13, "block-STEP": 7.8e-15, "block-RAMP": 3.7e-14}
F64_WORST_ENERGY = {"bar-STEP": 1.6e-14, "bar-RAMP": 1.6e-14, "block-STEP": 9.9e-15, "block-RAMP": 2.6e-14}
BOUND_TOL = 4.0 * F64_WORST_BOUND


# ------------------------------------------------------------------------------------- the restatement
def s_C(material, dtype=np.float64):
    """max eps:C:eps / eps:eps over symmetric strains, in closed form: 3 lambda + 2 mu (3-D), 2 lambda + 2 mu (plane strain),
    E / (1 - nu) (plane stress); neo-Hookean: lambda = 2 D1, mu = 2 C1 of its constant tangent 4 C1 I + 2 D1 (1 x 1)"""
    p0, p1 = dtype(material.params[0]), dtype(material.params[1])
    if material.kind == er.NEOHOOKE:
        lam, mu = 2 * p1, 2 * p0
        return 3 * lam + 2 * mu if material.dm == 3 else 2 * lam + 2 * mu
    if material.kind == er.PSTRESS:
        return p0 / (1 - p1)
    lam, mu = p0 * p1 / (1 + p1) / (1 - 2 * p1), p0 / 2 / (1 + p1)
    return 3 * lam + 2 * mu if material.kind == er.LIN3D else 2 * lam + 2 * mu


def element_masses(nodes, el, ELE, rho, dtype):
    """[ne, npe] the HRZ shares m_a^e that explicit_reference.lumped_mass sums into the nodal masses"""
    N, dN, w = er.mass_tables(ELE, dtype)
    X = np.asarray(nodes, dtype=dtype)[el]
    vq = dtype(rho) * (np.abs(er._det(np.einsum("eai,qaj->eqij", X, dN))) * w[None, :])
    me, d = vq.sum(axis=1), np.einsum("qa,eq->ea", N * N, vq)
    return d * me[:, None] / d.sum(axis=1)[:, None]


class Estimate:
    """mesh + material + element masses in one dtype: g_e, omega_e^2 and omega at a displacement"""

    def __init__(self, nodes, el, ELE, material, rho, dtype):
        self.mdl = er.Model(nodes, el, ELE, material, dtype)
        self.me = element_masses(nodes, el, ELE, rho, dtype)
        self.sC, self.dtype = s_C(material, dtype), dtype

    def elements(self, u):
        """-> g_e [ne], omega_e^2 [ne]"""
        m = self.mdl
        J, F = m._state(u)
        gx = np.einsum("gak,egkj->egaj", m.dN, er._inv(J))
        q = np.einsum("egaj,egaj,ea->eg", gx, gx, 1 / self.me)
        v = np.abs(er._det(J)) * m.w[None, :]
        sig = er.cauchy(F, m.kind, m.C, m.params, self.dtype)
        return (v * q).sum(axis=1), (v * (self.sC + np.sqrt((sig * sig).sum(axis=(-1, -2)))) * q).sum(axis=1)

    def omega(self, u):
        return np.sqrt(self.elements(u)[1].max())


def verlet_auto(est, minv, f, v0, sf, T, ramp, max_steps=100000, fixed_h=None):
    """the variable-step recurrence in est.dtype: -> H [steps], times [steps + 1], U, V [steps + 1, n].  fixed_h: that
    increment in place of the rule (the last one still takes the remainder)"""
    dt, mdl = est.dtype, est.mdl
    minv, f, T, sf = np.asarray(minv, dtype=dt), np.asarray(f, dtype=dt), dt(T), dt(sf)
    scale = (lambda t: t / T) if ramp else (lambda t: dt(1))
    u, v, t = np.zeros(mdl.nn * mdl.dm, dtype=dt), np.asarray(v0, dtype=dt) * (minv != 0), dt(0)
    a = minv * (scale(t) * f - mdl.f_int(u))
    H, times, U, V = [], [t], [u], [v]
    while t < T and len(H) < max_steps:
        om = est.omega(u) if fixed_h is None else None
        hs = sf * (2 / om) if fixed_h is None else dt(fixed_h)
        if not np.isfinite(np.asarray(hs, dtype=np.float64)) and fixed_h is None and not om == 0:
            break                                                     # omega is not finite: no increment
        rem = T - t
        h, t = (rem, T) if hs >= rem else (hs, min(t + hs, T))
        u = u + h * v + (h * h / 2) * a
        an = minv * (scale(t) * f - mdl.f_int(u))
        v = v + (h / 2) * (a + an)
        a = an
        H.append(h), times.append(t), U.append(u), V.append(v)
        if not np.isfinite(np.abs(u).max().astype(np.float64)):
            break
    return np.array(H), np.array(times), np.array(U), np.array(V)


# ------------------------------------------------------------------------------------------ the estimate
def materials_of(ELE):
    """a linear kind and the neo-Hookean solid of the family's dimension (2-D: plane stress and plane strain both)"""
    if ELE.dm == 3:
        return {"linear": LinearIsotropic(ec.E_MOD, ec.NU), "neo": NeoHookean(C1=ec.NEO["C1"], D1=ec.NEO["D1"])}
    return {"linear": LinearIsotropicPlaneStress(ec.E_MOD, ec.NU), "pstrain": LinearIsotropicPlaneStrain(ec.E_MOD, ec.NU),
            "neo": NeoHookeanPlaneStrain(C1=ec.NEO["C1"], D1=ec.NEO["D1"])}


# (mesh, material, state, which element is made the maximal one): every shape x every material x u = 0 and a smooth u; the
# arrangements with the maximum in element 0 and in element ne - 1 on the mesh of two workgroups and on a small one
BOUND_CASES = [(name, mat, state, None) for name in ec.SHAPES for mat in ("linear", "neo") for state in ("rest", "smooth")]
BOUND_CASES += [(name, "pstrain", "smooth", None) for name in ("CPS4-63", "CPS8")]
BOUND_CASES += [(name, "linear", "smooth", which) for name in ("C3D4-150", "CPS3") for which in ("first", "last")]


def smooth_u(nodes):
    """a smooth displacement with |F - I| of about 0.05: a shear, a stretch and a sine wave"""
    X = np.asarray(nodes, dtype=np.float64)
    size = np.ptp(X, axis=0).max()
    Z = (X - X.min(axis=0)) / size
    u = np.zeros_like(X)
    u[:, 0] = 0.03 * size * Z[:, 1] + 0.01 * size * np.sin(2.0 * Z[:, 0])
    u[:, 1] = -0.02 * size * Z[:, 1] + 0.01 * size * Z[:, 0] * Z[:, 0]
    if X.shape[1] == 3:
        u[:, 2] = 0.02 * size * Z[:, 2] * (1.0 + Z[:, 0])
    return u.ravel()


def bound_setup(name, which):
    nodes, el, ELE = ec.shape_mesh(name)
    if which is not None:                                             # shrink one element about its centroid: it becomes the
        e = 0 if which == "first" else len(el) - 1                   # stiffest of the mesh by far (its neighbours stretch)
        nodes = np.array(nodes, dtype=np.float64)
        c = nodes[el[e]].mean(axis=0)
        nodes[el[e]] = c + 0.5 * (nodes[el[e]] - c)
    return nodes, el, ELE


@functools.lru_cache(maxsize=None)
def reference_bound(name, mat, state, which):
    """-> omega in long double, the error of the float64 restatement, the maximal element, largest |F - I|"""
    nodes, el, ELE = bound_setup(name, which)
    material = materials_of(ELE)[mat]
    u = smooth_u(nodes) if state == "smooth" else np.zeros(nodes.size)
    est = Estimate(nodes, el, ELE, material, RHO, LD)
    w2 = est.elements(u)[1]
    om = np.sqrt(w2.max())
    om64 = Estimate(nodes, el, ELE, material, RHO, np.float64).omega(u)
    stretch = float(np.abs(est.mdl._state(u)[1] - np.eye(ELE.dm)).max())
    return om, float(abs(LD(om64) - om) / om), int(np.argmax(w2)), stretch


def make_ctx(nodes, el, ELE, material, backend):
    ctx = lc.make_ctx(nodes, el, ELE, backend, pattern=False)
    ctx.set_material(material)
    ctx.build_pattern()
    return ctx


def bound(name, mat, state, which, backend):
    """femcy_explicit_element_bound against the long-double restatement; evaluated twice: the same bits"""
    nodes, el, ELE = bound_setup(name, which)
    material = materials_of(ELE)[mat]
    ref, _, arg, stretch = reference_bound(name, mat, state, which)
    u = smooth_u(nodes) if state == "smooth" else np.zeros(nodes.size)
    ctx = make_ctx(nodes, el, ELE, material, backend)
    _, ex = ec.make_explicit(ctx, ELE, ec.held_dofs(nodes)[1])
    ctx.upload(be.VEC_TMP0, u)
    sc = float(s_C(material))
    om = ctx.explicit_element_bound(ex, sc, be.VEC_TMP0)
    om2 = ctx.explicit_element_bound(ex, sc, be.VEC_TMP0)
    ne = ctx.ne
    ctx.close()
    err = float(abs(LD(om) - ref) / ref)
    print(f"{name} {mat} {state} {which} [{backend}]: {ne} elements, omega {om:.6e}, error {err:.3e}, maximal element {arg}, "
          f"|F - I| {stretch:.3f}")
    assert om == om2
    if name == "C3D4-150":
        assert 256 < ne <= 512                                        # two workgroups of the bound kernel, the second partial
    if which is not None:
        assert arg == (0 if which == "first" else ne - 1)
    if state == "smooth":
        assert 0.03 <= stretch <= 0.08, stretch
    assert err <= BOUND_TOL, err
    return err


def proof(name, backend):
    """u = 0, linear material: omega of the element bound >= the largest eigenfrequency of M_L^-1 K on the free DOFs, with no
    margin; Gershgorin's ratio beside it"""
    nodes, el, ELE = ec.shape_mesh(name)
    _, fixed = ec.held_dofs(nodes)
    ctx = lc.make_ctx(nodes, el, ELE, backend)
    lm, ex = ec.make_explicit(ctx, ELE, fixed)
    ctx.assemble_K(-1)
    K = ctx.get_K_bsr().toarray()
    minv = 1.0 / np.repeat(ctx.lumped_mass_get(lm), ELE.dm)
    minv[fixed] = 0.0
    _, gersh = ctx.explicit_stable_dt(ex)
    ctx.vector(be.VEC_DOF).fill(0.0)
    om = ctx.explicit_element_bound(ex, float(s_C(ec.material_of(ELE))), be.VEC_DOF)
    ctx.close()
    free = np.setdiff1d(np.arange(nodes.size), fixed)
    true = float(np.sqrt(np.linalg.eigvals(minv[free, None] * K[np.ix_(free, free)]).real.max()))
    print(f"{name} [{backend}]: element bound / largest eigenfrequency {om / true:.4f}, Gershgorin / largest {gersh / true:.4f}")
    assert om >= true, (om, true)
    return om / true


def scaling(name, backend):
    """x = s X by u = (s - 1) X with the masses of the undeformed mesh: g_e changes by s^(dm - 2).  A uniform dilation has one
    stress sigma(s I) everywhere, so omega^2 = (s_C + |sigma(s I)|_F) max_e g_e; at s = 1 the stress is zero and
    omega^2 = s_C max_e g_e.  Both omegas carry at most BOUND_TOL each."""
    nodes, el, ELE = ec.shape_mesh(name)
    material = ec.material_of(ELE)
    dm = ELE.dm
    est = Estimate(nodes, el, ELE, material, RHO, LD)
    g1, w1 = est.elements(np.zeros(nodes.size))
    assert float(np.abs(w1 - est.sC * g1).max() / w1.max()) <= 4 * EPS    # zero stress: the linear term alone
    ctx = make_ctx(nodes, el, ELE, material, backend)
    _, ex = ec.make_explicit(ctx, ELE, ec.held_dofs(nodes)[1])
    sc = float(est.sC)
    ctx.vector(be.VEC_TMP0).fill(0.0)
    om1 = LD(ctx.explicit_element_bound(ex, sc, be.VEC_TMP0))
    worst = float(abs(om1 - np.sqrt(est.sC * g1.max())) / om1)
    for s in (0.5, 2.0):
        u = (s - 1.0) * np.asarray(nodes, dtype=np.float64).ravel()
        gs, _ = est.elements(u)
        eg = float(np.abs(gs / g1 - LD(s) ** (dm - 2)).max())
        assert eg <= 64 * float(np.finfo(LD).eps), eg                 # the restatement itself, in long double
        sig = er.cauchy(LD(s) * np.eye(dm, dtype=LD), int(material.kind), material.C, np.asarray(material.params), LD)
        ctx.upload(be.VEC_TMP0, u)
        om = LD(ctx.explicit_element_bound(ex, sc, be.VEC_TMP0))
        want = om1 * np.sqrt((est.sC + np.sqrt((sig * sig).sum())) / est.sC * LD(s) ** (dm - 2))
        worst = max(worst, float(abs(om - want) / want))
    ctx.close()
    print(f"{name} [{backend}]: scaling x = s X, worst error {worst:.3e}")
    assert worst <= 2 * BOUND_TOL, worst
    return worst


# ---------------------------------------------------------------------------------------- trajectories
SF = 0.9
TRAJ_CASES = ["bar-STEP", "bar-RAMP", "block-STEP", "block-RAMP"]


def auto_dynamic(T, every, sf=SF):
    return "*Dynamic, explicit, element by element, scale factor=%r, output_every=%d\n, %r\n" % (sf, every, T)


def write_traj_deck(path, key, every=1, T=None):
    """the bar / block of explicit_cases under STEP or RAMP, run with `element by element`"""
    case, amp = key.split("-")
    spec = ec.CASES[case]
    T = spec["dt"] * spec["steps"] if T is None else T
    nodes, el, ELE, mat = ec.write_case_deck(path, case, dynamic=auto_dynamic(T, every))
    text = open(path).read()
    head = text[text.index("*Step, name=Step-1"):].split("\n")[0]
    with open(path, "w") as f:                                        # the writer's *Step line, with this amplitude
        f.write(text.replace(head, "*Step, name=Step-1, amplitude=%s, nlgeom=NO" % amp))
    return nodes, el, ELE, mat, T


def solve_auto(path, backend):
    """-> inp, system (closed), u and v after every batch"""
    from femcy_amd.body import Body
    from femcy_amd.reader import InpInfo
    from femcy_amd.stiffnessMtrx import System_of_equations
    inp = InpInfo(path)
    body = Body(nodes=inp.nodes, elements=list(inp.eSets.values())[0], ELE=inp.ELE)
    system = System_of_equations(body, list(inp.materials.values())[0], inp.geometric_nonlinear, verbose=False,
                                 ctx=be.Context(0, backend=backend))
    U, V, advance = [], [], system.ctx.explicit_auto_advance

    def recording(*a, **kw):
        advance(*a, **kw)
        U.append(system.dof.to_numpy())
        V.append(system.ctx.download(be.VEC_VEL))

    system.ctx.explicit_auto_advance = recording
    try:
        system.solve(inp)
    finally:
        system.ctx.close()
    return inp, system, np.array(U), np.array(V)


@functools.lru_cache(maxsize=None)
def reference_traj(key, workdir):
    """the long-double run of a trajectory case (every step a record) and the errors of the float64 one"""
    path = os.path.join(workdir, "ref_%s.inp" % key)
    nodes, el, ELE, mat, T = write_traj_deck(path, key)
    inp, f, v0, fixed = ec.deck_loads(path)
    ramp = inp.amplitude == "RAMP"
    assert ramp == key.endswith("RAMP")
    out = {}
    for dt in (LD, np.float64):
        est = Estimate(nodes, el, ELE, mat, inp.density, dt)
        m = er.lumped_mass(nodes, el, ELE, inp.density, dt)
        minv = 1 / np.repeat(m, ELE.dm)
        minv[fixed] = 0
        H, times, U, V = verlet_auto(est, minv, f, v0, SF, T, ramp)
        scales = [(t / dt(T)) if ramp else dt(1) for t in times[1:]]
        hist = ec.balance(U[1:], [er.kinetic(m, v, ELE.dm, dt) for v in V[1:]], [est.mdl.energy(u) for u in U[1:]], f, scales, dt)
        out[dt] = (H, times, U[1:], V[1:], hist)
    H, times, U, V, hist = out[LD]
    H64, _, U64, V64, hist64 = out[np.float64]
    assert len(H64) == len(H) and times[-1] == T
    escale = max(float(h[1]) for h in hist)
    return {"H": H, "times": times, "U": U, "V": V, "hist": hist, "escale": escale, "f": f,
            "h64": float(np.abs(H64 - H).max() / H.max()),
            "traj64": max(float(np.abs(U64 - U).max() / np.abs(U).max()), float(np.abs(V64 - V).max() / np.abs(V).max())),
            "energy64": max(abs(float(a[0] - b[0])) for a, b in zip(hist64, hist)) / escale}


def trajectory(tmpdir, key, backend, workdir):
    """one record per step: the increments, u, v and the energy balance against the long-double restatement fed the same rule"""
    path = os.path.join(str(tmpdir), "%s.inp" % key)
    _, _, _, _, T = write_traj_deck(path, key)
    inp, system, U, V = solve_auto(path, backend)
    ref = reference_traj(key, workdir)
    n = len(ref["H"])
    assert inp.dynamic_auto and system.stats["assemblies"] == 0
    assert [i["kinc"] for i in system.increments] == list(range(1, n + 1)) and system.increments[-1]["time1"] == T
    H = np.array([i["dt"] for i in system.increments])
    assert abs(system.stable_dt * SF - H[0]) <= 4 * EPS * H[0] and min(H) == system.increments[-1]["dt_min"]
    eh = float(np.abs(H - ref["H"]).max() / ref["H"].max())
    et = float(np.abs(np.array([i["time1"] for i in system.increments]) - ref["times"][1:]).max() / T)
    eu = float(np.abs(U - ref["U"]).max() / np.abs(ref["U"]).max())
    ev = float(np.abs(V - ref["V"]).max() / np.abs(ref["V"]).max())
    scales = [i["time1"] / T if inp.amplitude == "RAMP" else 1.0 for i in system.increments]
    hist = ec.balance(U, [i["kinetic"] for i in system.increments], [i["strain_energy"] for i in system.increments], ref["f"],
                      scales, LD)
    ee = max(abs(float(a[0] - b[0])) for a, b in zip(hist, ref["hist"])) / ref["escale"]
    print(f"{key} [{backend}]: {n} steps, h in [{H.min():.4e}, {H.max():.4e}], increments {eh:.3e}, clock {et:.3e}, u {eu:.3e}, "
          f"v {ev:.3e}, energy balance {ee:.3e}")
    assert H.max() > 1.0001 * H[:-1].min()                            # the increment does vary along the run
    assert max(eh, et) <= 4.0 * F64_WORST_H[key], (eh, et)
    assert max(eu, ev) <= 4.0 * F64_WORST_TRAJ[key], (eu, ev)
    assert ee <= 4.0 * F64_WORST_ENERGY[key], ee
    return U, V, H


def host_against_device(tmpdir, key, workdir):
    """the two backends on the same deck: each is within 4 x the float64 figure of the reference, so they are within 8 x of
    each other"""
    Uh, Vh, Hh = trajectory(tmpdir, key, "cpu", workdir)
    Ud, Vd, Hd = trajectory(tmpdir, key, "hip", workdir)
    eh = float(np.abs(Hh - Hd).max() / Hh.max())
    eu = max(float(np.abs(Uh - Ud).max() / np.abs(Uh).max()), float(np.abs(Vh - Vd).max() / np.abs(Vh).max()))
    print(f"{key}: host against device, increments {eh:.3e}, trajectory {eu:.3e}")
    assert eh <= 8.0 * F64_WORST_H[key] and eu <= 8.0 * F64_WORST_TRAJ[key], (eh, eu)


# ------------------------------------------------------------------------------------- split = whole
def split(key, backend, tmpdir):
    """batches of 8 against one batch of 10^4, bit for bit on u, v, a and the clock; a batch past T changes nothing"""
    path = os.path.join(str(tmpdir), "split_%s.inp" % key)
    nodes, el, ELE, mat, T = write_traj_deck(path, key)
    inp, f, v0, fixed = ec.deck_loads(path)
    ramp = inp.amplitude == "RAMP"
    ctx = make_ctx(nodes, el, ELE, mat, backend)
    lm = ctx.lumped_mass(ELE, inp.density)
    ex = ctx.explicit(lm, [ctx.dofset(fixed)])
    sc = float(s_C(mat))
    ctx.upload(be.VEC_RHS, f)
    runs = []
    for batch in (10000, 8):
        ctx.vector(be.VEC_DOF).fill(0.0)
        ctx.upload(be.VEC_VEL, v0 * (np.isin(np.arange(v0.size), fixed) == 0))
        ctx.explicit_auto_begin(ex, sc, SF, T, ramp)
        assert ctx.explicit_auto_state(ex) == (0.0, 0.0, 0.0, 0)
        calls = 0
        while ctx.explicit_auto_state(ex)[0] < T:
            ctx.explicit_auto_advance(ex, batch)
            calls += 1
        runs.append(([ctx.download(v) for v in (be.VEC_DOF, be.VEC_VEL, be.VEC_ACC)], ctx.explicit_auto_state(ex), calls))
    (whole, clock_w, calls_w), (parts, clock_p, calls_p) = runs
    assert calls_w == 1 and calls_p == -(-clock_p[3] // 8) and clock_p[3] > 16
    assert clock_w == clock_p and clock_w[0] == T
    for w, p, what in zip(whole, parts, "uva"):
        assert np.isfinite(w).all() and np.abs(w).max() > 0
        assert np.array_equal(w.view(np.uint64), p.view(np.uint64)), what
    ctx.explicit_auto_advance(ex, 8)                                  # past T: no-ops
    ctx.explicit_auto_advance(ex, 0)
    assert ctx.explicit_auto_state(ex) == clock_p
    for p, vec, what in zip(parts, (be.VEC_DOF, be.VEC_VEL, be.VEC_ACC), "uva"):
        assert np.array_equal(ctx.download(vec).view(np.uint64), p.view(np.uint64)), what
    ctx.close()


# ------------------------------------------------------------------------------ the reason for the feature
# A neo-Hookean bar of 1 x 1 x 8 C3D8 cells, every free node thrown at CRUSH_SPEED against the end held at z = 0.  The speed
# was chosen on the CPU with the restatement alone (reference_crush): at 0.9 x the increment estimated at u = 0 the
# long-double run leaves the range of float64, with the element-by-element rule at scale factor 0.9 it stays finite with the
# total energy below twice its initial value, and the shortest element loses CRUSH_LOSS of its length.
CRUSH = dict(cells=(1, 1, 8), box=(1.0, 1.0, 4.0), speed=20.0, T=0.4, C1=80.0, D1=400.0, rho=2.0)


def write_crush_deck(path, dynamic):
    from femcy_amd import meshgen
    from femcy_amd.element_zoo import Element_linear_hexahedral
    nodes, el = meshgen.plate_hex(*CRUSH["cells"], perturb=0.0, seed=0, box=CRUSH["box"])
    nsets = {"foot": np.nonzero(nodes[:, 2] < 1e-12)[0], "body": np.nonzero(nodes[:, 2] >= 1e-12)[0]}
    mat = "*Density\n%r,\n*Hyperelastic, neo hooke\n%r, %r\n" % (CRUSH["rho"], CRUSH["C1"], 1.0 / CRUSH["D1"])
    ec.write_explicit_deck(path, nodes, el, "C3D8", nsets, "*Boundary\nfoot, 1, 1\nfoot, 2, 2\nfoot, 3, 3\n", dynamic, material=mat,
                           initial="*Initial Conditions, type=VELOCITY\nbody, 3, %r\n" % -CRUSH["speed"])
    return nodes, el, Element_linear_hexahedral(), NeoHookean(C1=CRUSH["C1"], D1=CRUSH["D1"])


@functools.lru_cache(maxsize=None)
def reference_crush(workdir):
    """the long-double restatement of both runs -> (the fixed run left float64, the automatic run's worst energy / initial
    energy, its largest loss of length of an element, its smallest increment / the first estimate, the first estimate)"""
    path = os.path.join(workdir, "ref_crush.inp")
    nodes, el, ELE, mat = write_crush_deck(path, auto_dynamic(CRUSH["T"], 8))
    assert len(el) <= 64
    inp, f, v0, fixed = ec.deck_loads(path)
    est = Estimate(nodes, el, ELE, mat, inp.density, LD)
    m = er.lumped_mass(nodes, el, ELE, inp.density, LD)
    minv = 1 / np.repeat(m, 3)
    minv[fixed] = 0
    dt0 = 2 / est.omega(np.zeros(nodes.size))
    with np.errstate(all="ignore"):
        _, _, Uf, _ = verlet_auto(est, minv, f, v0, 1.0, CRUSH["T"], False, fixed_h=0.9 * dt0)
        H, times, U, V = verlet_auto(est, minv, f, v0, SF, CRUSH["T"], False)
        blown = not np.isfinite(np.abs(Uf[-1]).max().astype(np.float64))
    e0 = er.kinetic(m, V[0], 3, LD)
    worst = max(float((er.kinetic(m, v, 3, LD) + est.mdl.energy(u)) / e0) for u, v in zip(U, V))
    z = np.asarray(nodes, dtype=LD)[:, 2][None, :] + U.reshape(len(U), -1, 3)[:, :, 2]
    height = z[:, el].max(axis=2) - z[:, el].min(axis=2)               # [steps, ne] the extent of every element along the bar
    loss = float(1 - (height / height[0]).min())
    return blown, worst, loss, float(H[:-1].min() / dt0), float(dt0), bool(times[-1] == CRUSH["T"])


def crush(tmpdir, backend, workdir):
    blown, worst, loss, ratio, dt0, finished = reference_crush(workdir)
    print(f"restatement: fixed 0.9 x {dt0:.4e} leaves float64: {blown}; element by element: energy / initial <= {worst:.3f}, "
          f"largest loss of length {loss:.3f}, smallest increment / first estimate {ratio:.3f}")
    assert blown and finished and worst < 2.0 and loss >= 0.30 and ratio < 0.75, "the reference must show both outcomes first"
    path = os.path.join(str(tmpdir), "crush_fixed.inp")
    write_crush_deck(path, "*Dynamic, explicit, direct user control\n%r, %r\n" % (0.9 * dt0, CRUSH["T"]))
    with pytest.raises(be.FemcyError, match="unstable increment") as raised:
        ec.solve_deck(path, backend)
    assert raised.value.status == be.FEMCY_ENUMERIC
    path = os.path.join(str(tmpdir), "crush_auto.inp")
    write_crush_deck(path, auto_dynamic(CRUSH["T"], 8))
    inp, system, U, V = solve_auto(path, backend)
    last = system.increments[-1]
    e0 = system.initial_energy["kinetic"]
    assert np.isfinite(U).all() and last["time1"] == CRUSH["T"] and system.stats["assemblies"] == 0
    assert all(i["kinetic"] + i["strain_energy"] < 2 * e0 for i in system.increments)
    assert abs(system.stable_dt - dt0) <= 64 * EPS * dt0
    print(f"[{backend}]: {last['kinc']} steps, dt_min / stable_dt = {last['dt_min'] / system.stable_dt:.3f}")
    assert last["dt_min"] < 0.75 * system.stable_dt


# --------------------------------------------------------------------------------------------- refusals
def refusals(backend):
    """every refusal returns FEMCY_EINVAL with a message, and the context keeps working"""
    nodes, el, ELE = ec.shape_mesh("C3D8")
    _, fixed = ec.held_dofs(nodes)
    ctx = lc.make_ctx(nodes, el, ELE, backend)
    _, ex = ec.make_explicit(ctx, ELE, fixed)
    sc = float(s_C(ec.material_of(ELE)))
    calls = [(lambda: ctx.explicit_element_bound(ex + 1, sc), "unknown explicit integrator"),
             (lambda: ctx.explicit_auto_begin(ex + 1, sc, 1.0, 1.0), "unknown explicit integrator"),
             (lambda: ctx.explicit_auto_advance(-1, 1), "unknown explicit integrator"),
             (lambda: ctx.explicit_auto_state(ex + 1), "unknown explicit integrator"),
             (lambda: ctx.explicit_auto_advance(ex, 1), "before femcy_explicit_auto_begin"),
             (lambda: ctx.explicit_auto_state(ex), "before femcy_explicit_auto_begin")]
    for bad in (0.0, -1.0, np.nan, np.inf):
        calls += [(lambda b=bad: ctx.explicit_element_bound(ex, b), "s_C"),
                  (lambda b=bad: ctx.explicit_auto_begin(ex, b, 1.0, 1.0), "finite and positive"),
                  (lambda b=bad: ctx.explicit_auto_begin(ex, sc, b, 1.0), "finite and positive"),
                  (lambda b=bad: ctx.explicit_auto_begin(ex, sc, 1.0, b), "finite and positive")]
    calls += [(lambda v=v: ctx.explicit_auto_begin(ex, sc, 1.0, 1.0, False, v), "state vectors") for v in (be.VEC_DOF, be.VEC_VEL, be.VEC_ACC)]
    for call, message in calls:
        with pytest.raises(be.FemcyError, match=message) as refused:
            call()
        assert refused.value.status == -1, message                    # FEMCY_EINVAL
    assert not np.abs(ctx.download(be.VEC_ACC)).any()                 # nothing moved
    ctx.explicit_auto_begin(ex, sc, 1.0, 1.0e-4)                      # the context still works
    late = [(lambda: ctx.explicit_auto_advance(ex, -1), "-1 steps")]
    late += [(lambda v=v: ctx.explicit_auto_advance(ex, 1, v), "state vectors") for v in (be.VEC_DOF, be.VEC_VEL, be.VEC_ACC)]
    for call, message in late:
        with pytest.raises(be.FemcyError, match=message) as refused:
            call()
        assert refused.value.status == -1, message
    ctx.explicit_auto_advance(ex, 3)
    assert ctx.explicit_auto_state(ex)[3] >= 1 and ctx.explicit_element_bound(ex, sc) > 0
    ctx.set_mesh(nodes, el)                                           # a new mesh drops the integrator and its clock
    with pytest.raises(be.FemcyError, match="unknown explicit integrator"):
        ctx.explicit_auto_state(ex)
    ctx.close()


def comm_refusal(backend):
    """once femcy_comm_init has run, every call of the feature returns FEMCY_EINVAL (device only, as in explicit_cases)"""
    nodes, el, ELE = ec.shape_mesh("C3D8-64")
    ctx = lc.make_ctx(nodes, el, ELE, backend)
    _, ex = ec.make_explicit(ctx, ELE, ec.held_dofs(nodes)[1])
    sc = float(s_C(ec.material_of(ELE)))
    ctx.explicit_auto_begin(ex, sc, 1.0, 1.0e-4)
    iface = np.arange(0, ctx.n, 7, dtype=np.int32)
    ctx.comm_init(0, 1, be.Context.comm_unique_id(), iface, np.arange(iface.size, dtype=np.int32), iface.size,
                  np.ones(ctx.n, dtype=np.uint8))
    for call in (lambda: ctx.explicit_element_bound(ex, sc), lambda: ctx.explicit_auto_begin(ex, sc, 1.0, 1.0),
                 lambda: ctx.explicit_auto_advance(ex, 1), lambda: ctx.explicit_auto_state(ex)):
        with pytest.raises(be.FemcyError, match="several ranks") as refused:
            call()
        assert refused.value.status == -1
    ctx.close()


def measure_f64_worst(workdir):
    """the constants at the top, as measured: the float64 restatement against the long-double one on the cases run here"""
    refs = {key: reference_traj(key, workdir) for key in TRAJ_CASES}
    return {"bound": max(reference_bound(*case)[1] for case in BOUND_CASES), "h": {k: r["h64"] for k, r in refs.items()},
            "traj": {k: r["traj64"] for k, r in refs.items()}, "energy": {k: r["energy64"] for k, r in refs.items()}}
