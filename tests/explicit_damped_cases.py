"""Damped explicit dynamics (femcy_explicit_set_damping, *Bulk Viscosity, *Damping alpha=) written against the C ABI
(femcy_amd.backend.Context) and the deck reader, so that the host backend (tests/test_explicit_damped_cpu.py) and the device
(tests/test_gpu_explicit_damped.py) run the same code.  Every function checks its own result and returns the figure it checked.

Bounds.  The reference is the restatement of tests/explicit_damped_reference.py in np.longdouble.  The same restatement in
float64 differs from it by rounding and summation order alone; the F64_WORST_* constants are the worst such differences on
the very cases run here (`measure_f64_worst`, asserted by tests/test_explicit_damped_cpu.py), and a backend is held to 4 x
that.  Errors are relative to the largest entry of the reference."""
import functools

import numpy as np
import pytest

from femcy_amd import backend as be

import explicit_auto_cases as eac
import explicit_cases as ec
import explicit_damped_reference as edr
import explicit_reference as er
import loads_cases as lc
import loads_reference as lr

LD = np.longdouble
RHO = ec.RHO
ALPHA, B1, B2 = 50.0, 0.06, 1.2
# the float64 restatement against the long-double one, as measured (measure_f64_worst): one damped step 2.09e-15 (CPS4-65),
# each term alone 2.22e-15, omega_eff 6.67e-16 (rest and deformed), the uniform dilation 3.41e-16, the rigid translation 5.00e-16
F64_WORST_STEP = 2.1e-15
F64_WORST_TERM = 2.3e-15
F64_WORST_OMEGA = 6.7e-16
F64_WORST_DILATION = 3.5e-16
F64_WORST_RIGID = 5.1e-16
# the deck trajectories (u, v, and the increments of the automatic runs), as measured: 3.09e-14, 6.29e-14, 6.41e-15, 1.02e-14
F64_WORST_TRAJ = {("bar", "fixed"): 3.1e-14, ("bar", "auto"): 6.3e-14, ("block", "fixed"): 6.5e-15, ("block", "auto"): 1.1e-14}

STEP_SHAPES = list(ec.STEP_SHAPES) + ["C3D8", "C3D6"]
TERMS = {"alpha": (ALPHA, 0.0, 0.0), "b1": (0.0, B1, 0.0), "b2": (0.0, 0.0, B2)}
TERM_SHAPES = ["C3D4", "CPS4-65"]


def modulus(material):
    """M_d: C[0][0] of the small-strain matrix"""
    return float(np.asarray(material.C, dtype=np.float64)[0][0])


def relerr(got, want):
    return float(np.abs(np.asarray(got, dtype=LD) - want).max() / np.abs(want).max())


# ------------------------------------------------------------------------------------------ one step
@functools.lru_cache(maxsize=None)
def reference_step(name, coeffs):
    """-> (a0, u1, v1, a1) in long double, the error of the float64 restatement, the share of Gauss points with rate < 0"""
    nodes, el, ELE, fixed, f, u0, v0, h, s = ec.step_setup(name)
    mat = ec.material_of(ELE)
    out = {}
    for dt in (LD, np.float64):
        mdl = edr.DampedModel(nodes, el, ELE, mat, dt, RHO, coeffs[0], coeffs[1], coeffs[2], modulus(mat))
        minv = 1 / np.repeat(er.lumped_mass(nodes, el, ELE, RHO, dt), ELE.dm)
        minv[fixed] = 0
        U, V, A = mdl.verlet_damped(minv, f, v0, h, 1, lambda k: s, u0=u0)
        out[dt] = (A[0], U[1], V[1], A[1])
        if dt is LD:
            rate = mdl.points(U[1], V[0] + dt(h) / 2 * A[0])[2]
            neg = float((rate < 0).mean())
    for x in out[LD]:
        x.setflags(write=False)
    return out[LD], max(relerr(x64, x) for x64, x in zip(out[np.float64], out[LD])), neg


def damped_ctx(name, backend, coeffs):
    nodes, el, ELE, fixed, f, u0, v0, h, s = ec.step_setup(name)
    ctx = lc.make_ctx(nodes, el, ELE, backend)
    _, ex = ec.make_explicit(ctx, ELE, fixed)
    for vec, arr in ((be.VEC_DOF, u0), (be.VEC_VEL, v0), (be.VEC_RHS, f)):
        ctx.upload(vec, arr)
    if coeffs is not None:
        ctx.explicit_set_damping(ex, coeffs[0], coeffs[1], coeffs[2], modulus(ec.material_of(ELE)))
    return ctx, ex, h, s


def one_step(name, backend, coeffs=(ALPHA, B1, B2), tol=4.0 * F64_WORST_STEP):
    """start + advance(1) with damping against the reference: a_0, then u, v, a; both signs of the rate occur"""
    ref, _, neg = reference_step(name, coeffs)
    assert 0.1 <= neg <= 0.9, neg                                      # both branches of the quadratic term run
    ctx, ex, h, s = damped_ctx(name, backend, coeffs)
    ctx.explicit_start(ex, be.VEC_RHS, s)
    a0 = ctx.download(be.VEC_ACC)
    ctx.explicit_advance(ex, 1, h, be.VEC_RHS, s, 0.0)
    got = [a0] + [ctx.download(v) for v in (be.VEC_DOF, be.VEC_VEL, be.VEC_ACC)]
    ctx.close()
    err = max(relerr(g, w) for g, w in zip(got, ref))
    print(f"{name} {coeffs} [{backend}]: one damped step {err:.3e}, rate < 0 at {neg:.2f} of the Gauss points")
    assert err <= tol, err
    return err


def term(which, name, backend):
    """each coefficient alone: a term wired to the wrong coefficient shows"""
    ref_all = reference_step(name, (ALPHA, B1, B2))[0]
    ref = reference_step(name, TERMS[which])[0]
    assert relerr(ref_all[3], ref[3]) > 1e-6                            # the terms differ by far more than the bound
    return one_step(name, backend, TERMS[which], 4.0 * F64_WORST_TERM)


# --------------------------------------------------------------------------- zero is the undamped path
def run_fixed(ctx, ex, h, s, parts=(20,), ramp=False):
    s0, ds = (0.0, 1.0 / 32.0) if ramp else (s, 0.0)
    ctx.explicit_start(ex, be.VEC_RHS, s0)
    done = 0
    for k in parts:
        ctx.explicit_advance(ex, k, h, be.VEC_RHS, s0 + done * ds, ds)
        done += k
    return [ctx.download(v) for v in (be.VEC_DOF, be.VEC_VEL, be.VEC_ACC)]


def run_auto(ctx, ex, ELE, h, batches=(20,), ramp=False, steps=20):
    sc = float(eac.s_C(ec.material_of(ELE)))
    ctx.explicit_auto_begin(ex, sc, 0.5, steps * h, ramp, be.VEC_RHS)
    for k in batches:
        ctx.explicit_auto_advance(ex, k, be.VEC_RHS)
    return [ctx.download(v) for v in (be.VEC_DOF, be.VEC_VEL, be.VEC_ACC)] + [np.array(ctx.explicit_auto_state(ex))]


def zero_is_undamped(mode, backend, name="C3D4-150"):
    """set_damping(0, 0, 0, 0), and set_damping(x) followed by set_damping(0, ...): the bits of an integrator that never had
    damping set, over 20 steps"""
    ELE = ec.step_setup(name)[2]
    runs = []
    for setting in (None, "zero", "set-then-zero"):
        ctx, ex, h, s = damped_ctx(name, backend, None)
        if setting == "set-then-zero":
            ctx.explicit_set_damping(ex, ALPHA, B1, B2, modulus(ec.material_of(ELE)))
        if setting is not None:
            ctx.explicit_set_damping(ex, 0.0, 0.0, 0.0, 0.0)
        runs.append(run_fixed(ctx, ex, h, s) if mode == "fixed" else run_auto(ctx, ex, ELE, h))
        ctx.close()
    for other in runs[1:]:
        for x, y in zip(runs[0], other):
            assert np.array_equal(x.view(np.uint64), y.view(np.uint64))
    assert np.abs(runs[0][1]).max() > 0


def split(mode, ramp, backend, name="C3D4-150"):
    """damped: 7 + 13 steps against 20 (fixed), batches that overshoot T against one (automatic), bit for bit"""
    ELE = ec.step_setup(name)[2]
    runs = []
    for parts in ((20,), (7, 13)) if mode == "fixed" else ((40,), (7, 13, 20)):
        ctx, ex, h, s = damped_ctx(name, backend, (ALPHA, B1, B2))
        runs.append(run_fixed(ctx, ex, h, s, parts, ramp) if mode == "fixed" else run_auto(ctx, ex, ELE, h, parts, ramp))
        ctx.close()
    for x, y in zip(*runs):
        assert np.array_equal(x.view(np.uint64), y.view(np.uint64))
    if mode == "auto":
        assert runs[0][3][0] == 20 * ec.step_setup(name)[7] and runs[0][3][3] < 40      # t == T, the batch overshot it
    # and damping acts: the undamped run differs
    ctx, ex, h, s = damped_ctx(name, backend, None)
    plain = run_fixed(ctx, ex, h, s, (20,), ramp) if mode == "fixed" else run_auto(ctx, ex, ELE, h, (40,), ramp)
    ctx.close()
    assert not np.array_equal(plain[1], runs[0][1])


# ------------------------------------------------------------------------------- rigid translation
RIGID = dict(alpha=5000.0, h=2.0e-6, steps=200, v0=(3.0, -2.0, 1.5))       # t = steps h = 2 / alpha


@functools.lru_cache(maxsize=None)
def reference_rigid(name):
    """the scalar recurrence per direction in long double, and the float64 restatement's worst error against it"""
    nodes, el, ELE = ec.shape_mesh(name)
    r = RIGID
    want = [edr.scalar_alpha(r["alpha"], c, r["h"], r["steps"]) for c in r["v0"][:ELE.dm]]
    mdl = edr.DampedModel(nodes, el, ELE, ec.material_of(ELE), np.float64, RHO, r["alpha"])
    minv = 1 / np.repeat(er.lumped_mass(nodes, el, ELE, RHO, np.float64), ELE.dm)
    U, V, A = mdl.verlet_damped(minv, np.zeros(nodes.size), np.tile(r["v0"][:ELE.dm], len(nodes)), r["h"], r["steps"], lambda k: 0.0)
    return want, rigid_error(U[-1], V[-1], A[-1], want, ELE.dm)


def rigid_error(u, v, a, want, dm):
    return max(relerr(np.asarray(x).reshape(-1, dm), np.array([w[k] for w in want])[None, :]) for k, x in enumerate((u, v, a)))


def rigid(backend, name="C3D4"):
    """a free mesh, uniform v_0, no load, alpha alone: every node follows the scalar recurrence (XN_START reads v_0), and
    the kinetic energy after t = 2 / alpha is the recurrence's"""
    nodes, el, ELE = ec.shape_mesh(name)
    r = RIGID
    want, _ = reference_rigid(name)
    ctx = lc.make_ctx(nodes, el, ELE, backend)
    lm, ex = ec.make_explicit(ctx, ELE, [])
    ctx.upload(be.VEC_VEL, np.tile(r["v0"][:ELE.dm], len(nodes)))
    ctx.upload(be.VEC_ACC, np.full(nodes.size, np.nan))                # not read at the start
    ctx.explicit_set_damping(ex, r["alpha"], 0.0, 0.0, 0.0)
    ctx.explicit_start(ex, be.VEC_RHS, 1.0)
    a0 = ctx.download(be.VEC_ACC).reshape(-1, ELE.dm)
    assert np.array_equal(a0, np.tile(-r["alpha"] * np.array(r["v0"][:ELE.dm]), (len(nodes), 1)))
    ctx.explicit_advance(ex, r["steps"], r["h"], be.VEC_RHS, 1.0, 0.0)
    u, v, a = (ctx.download(x) for x in (be.VEC_DOF, be.VEC_VEL, be.VEC_ACC))
    ke = ctx.explicit_kinetic_energy(ex, be.VEC_VEL)
    m = ctx.lumped_mass_get(lm)
    ctx.close()
    err = rigid_error(u, v, a, want, ELE.dm)
    want_ke = float(m.astype(LD).sum() * sum(w[1] ** 2 for w in want) / 2)
    ek = abs(ke - want_ke) / want_ke
    print(f"{name} [{backend}]: rigid translation under alpha {err:.3e}, kinetic energy {ek:.3e}")
    assert err <= 4.0 * F64_WORST_RIGID, err
    assert ek <= 2 * 4.0 * F64_WORST_RIGID + (len(nodes) + 4) * ec.EPS, ek      # v enters squared; the sum as in ec.one_step
    return err


# -------------------------------------------------------------------------------- uniform dilation
def dilation_closed_form(etype, c, dtype):
    """one straight element, u = 0, v_0 = c X: a_0[a] = -p V grad N_a / m_a with rate = dm c, L the smallest altitude and
    grad N_a = -n_a / altitude_a, all by hand from the vertices"""
    nodes, el, ELE, V = lr.single(etype)
    X = np.asarray(nodes, dtype=dtype)[el[0]]
    dm, npe = X.shape[1], len(X)
    grads = []
    for a in range(npe):
        others = np.delete(X, a, axis=0)
        if dm == 2:
            e = others[1] - others[0]
            n = np.array([e[1], -e[0]], dtype=dtype)
        else:
            n = np.cross(others[1] - others[0], others[2] - others[0])
        n = n / np.sqrt((n * n).sum())
        alt = (X[a] - others[0]) @ n                                  # signed altitude of vertex a over the opposite side
        grads.append(n / alt)
    grads = np.array(grads)
    L = 1 / np.sqrt((grads * grads).sum(axis=1).max())
    vol = dtype(V)
    mat = ec.material_of(ELE)
    rate, rho, Md = dtype(dm) * dtype(c), dtype(RHO), dtype(modulus(mat))
    p = dtype(B1) * np.sqrt(rho * Md) * L * rate + rho * (dtype(B2) * L) ** 2 * abs(rate) * min(dtype(0), rate)
    quad = rho * (dtype(B2) * L) ** 2 * abs(rate) * min(dtype(0), rate)
    return -(p * vol) * grads / (rho * vol / npe), quad != 0


def dilation(etype, c, backend):
    nodes, el, ELE, V = lr.single(etype)
    want, quad = dilation_closed_form(etype, c, LD)
    assert quad == (c < 0)                                             # the quadratic term in compression only
    ctx = lc.make_ctx(nodes, el, ELE, backend)
    _, ex = ec.make_explicit(ctx, ELE, [])
    ctx.upload(be.VEC_VEL, (c * np.asarray(nodes, dtype=np.float64)).ravel())
    ctx.explicit_set_damping(ex, 0.0, B1, B2, modulus(ec.material_of(ELE)))
    ctx.explicit_start(ex, be.VEC_RHS, 0.0)
    a0 = ctx.download(be.VEC_ACC).reshape(want.shape)
    ctx.close()
    err = relerr(a0, want)
    print(f"{etype} c = {c} [{backend}]: a_0 of a uniform dilation {err:.3e}")
    assert err <= 4.0 * F64_WORST_DILATION, err
    return err


# ------------------------------------------------------------------------------------------ omega_eff
OMEGA_SHAPES = list(ec.SHAPES)                   # the shapes of explicit_auto_cases.BOUND_CASES


@functools.lru_cache(maxsize=None)
def reference_omega(name):
    nodes, el, ELE, fixed, f, u0, v0, h, s = ec.step_setup(name)
    mat = ec.material_of(ELE)
    out = {}
    for dt in (LD, np.float64):
        mdl = edr.DampedModel(nodes, el, ELE, mat, dt, RHO, ALPHA, B1, B2, modulus(mat))
        est = eac.Estimate(nodes, el, ELE, mat, RHO, dt)
        vh = np.asarray(v0, dtype=dt) * 400
        ud = np.asarray(eac.smooth_u(nodes), dtype=dt)
        out[dt] = (mdl.omega_eff(est, np.zeros(nodes.size), vh), mdl.omega_eff(est, ud, vh))
        if dt is LD:      # a valid deformed state: det F away from 1 and far from 0 (the estimate is singular at det F = 0)
            detF = er._det(mdl._state(ud)[1])
            assert 0.8 < detF.min() and detF.max() < 1.25 and np.abs(detF - 1).max() > 0.01, (detF.min(), detF.max())
    plain = eac.Estimate(nodes, el, ELE, mat, RHO, LD).omega(np.zeros(nodes.size))
    e64 = max(float(abs(LD(x64) - x) / x) for x64, x in zip(out[np.float64], out[LD]))
    return out[LD][0], e64, plain, out[LD][1]


def omega_eff(name, backend):
    """femcy_explicit_element_bound with damping at u = 0 and a non-zero vec[VEL] against max_e omega_e (sqrt(1 + xi^2) + xi);
    with every coefficient 0 the bits of an integrator without damping"""
    nodes, el, ELE, fixed, f, u0, v0, h, s = ec.step_setup(name)
    mat = ec.material_of(ELE)
    ref, _, plain, ref_deformed = reference_omega(name)
    assert ref > 1.05 * plain                                          # the damping shows in the estimate
    ctx = eac.make_ctx(nodes, el, ELE, mat, backend)
    _, ex = ec.make_explicit(ctx, ELE, fixed)
    sc = float(eac.s_C(mat))
    ctx.upload(be.VEC_VEL, v0 * 400)
    om0 = ctx.explicit_element_bound(ex, sc, be.VEC_DOF)
    ctx.explicit_set_damping(ex, ALPHA, B1, B2, modulus(mat))
    om = ctx.explicit_element_bound(ex, sc, be.VEC_DOF)
    # a deformed state, det F != 1 in rho_q: the smooth one of explicit_auto_cases (step_setup's random u_0 inverts Gauss
    # points of the curved C3D10 mesh, det F = -0.03, where the estimate itself is ill-conditioned)
    ctx.upload(be.VEC_TMP0, eac.smooth_u(nodes))
    om_deformed = ctx.explicit_element_bound(ex, sc, be.VEC_TMP0)
    ctx.explicit_set_damping(ex, 0.0, 0.0, 0.0, 0.0)
    om1 = ctx.explicit_element_bound(ex, sc, be.VEC_DOF)
    # vec[ACC] full of NaN before auto_begin: the first increment is the reference's
    ctx.explicit_set_damping(ex, ALPHA, B1, B2, modulus(mat))
    ctx.upload(be.VEC_ACC, np.full(nodes.size, np.nan))
    ctx.explicit_auto_begin(ex, sc, 0.5, 1.0, False, be.VEC_RHS)
    ctx.explicit_auto_advance(ex, 1, be.VEC_RHS)
    t, h_last, _, steps = ctx.explicit_auto_state(ex)
    state = [ctx.download(v) for v in (be.VEC_DOF, be.VEC_VEL, be.VEC_ACC)]
    ctx.close()
    err = max(float(abs(LD(om) - ref) / ref), float(abs(LD(om_deformed) - ref_deformed) / ref_deformed))
    eh = float(abs(LD(h_last) - 0.5 * 2 / ref) / (0.5 * 2 / ref))
    print(f"{name} [{backend}]: omega_eff {om:.6e} ({err:.3e}), undamped {om0:.6e}, first increment {eh:.3e}")
    assert om0 == om1 and abs(om0 - float(plain)) <= 4 * eac.F64_WORST_BOUND * om0
    assert err <= 4.0 * F64_WORST_OMEGA, err
    assert steps == 1 and eh <= 4.0 * F64_WORST_OMEGA + 4 * ec.EPS, eh
    assert all(np.isfinite(x).all() for x in state)
    return err


# ------------------------------------------------------------------------------------------- reader
def deck_with(tmpdir, extra_step="", extra_material="", dynamic=None, case="bar"):
    """the bar deck of explicit_cases with lines inserted after the procedure's data line / before *Density, where Abaqus/CAE writes *Damping"""
    import os
    path = os.path.join(str(tmpdir), "damped_%d.inp" % len(os.listdir(str(tmpdir))))
    ec.write_case_deck(path, case, dynamic=dynamic)
    lines = open(path).read().split("\n")
    out, k = [], 0
    while k < len(lines):
        out.append(lines[k])
        low = lines[k].lower()
        if low.startswith("*density") and extra_material:
            out[-1:] = extra_material.strip().split("\n") + [lines[k]]
        elif (low.startswith("*dynamic") or low.startswith("*static")) and extra_step:
            out.append(lines[k + 1])
            out.extend(extra_step.strip().split("\n"))
            k += 1
        k += 1
    with open(path, "w") as f:
        f.write("\n".join(out))
    return path


def reader(tmpdir):
    from femcy_amd.reader import InpInfo
    inp = InpInfo(deck_with(tmpdir))
    assert inp.bulk_viscosity is None and inp.damping_alpha == 0
    inp = InpInfo(deck_with(tmpdir, "*Bulk Viscosity\n0.1, 1.5\n", "*Damping, alpha=12.5\n"))
    assert inp.bulk_viscosity == (0.1, 1.5) and inp.damping_alpha == 12.5 and inp.procedure == "explicit"
    for data in ("*Bulk Viscosity\n", "*Bulk Viscosity\n,\n", "*Bulk Viscosity\n\n"):
        assert InpInfo(deck_with(tmpdir, data)).bulk_viscosity == (0.06, 1.2), data
    assert InpInfo(deck_with(tmpdir, "*Bulk Viscosity\n0.2,\n")).bulk_viscosity == (0.2, 1.2)
    static = "*Static\n1., 1., 1e-05, 1.\n"
    implicit = "*Dynamic, direct\n1e-4, 1e-3\n"
    for kwargs, word in ((dict(extra_material="*Damping, alpha=1., beta=0.1\n"), "beta"),
                         (dict(extra_material="*Damping, composite=0.1\n"), "composite"),
                         (dict(extra_material="*Damping, structural=0.1\n"), "structural"),
                         (dict(extra_material="*Damping, alpha=-1.\n"), "negative"),
                         (dict(extra_step="*Bulk Viscosity\n-0.06, 1.2\n"), "negative"),
                         (dict(extra_step="*Bulk Viscosity\n", dynamic=static), "Bulk Viscosity"),
                         (dict(extra_material="*Damping, alpha=1.\n", dynamic=implicit), "Damping")):
        with pytest.raises(ValueError, match=word):
            InpInfo(deck_with(tmpdir, **kwargs))


# ----------------------------------------------------------------------------------------- refusals
def refusals(backend):
    """FEMCY_EINVAL with a word of the message, and the context keeps working"""
    ctx, ex, h, s = damped_ctx("C3D4", backend, None)
    rows = [((ex + 1, 1.0, 0.0, 0.0, 0.0), "unknown explicit integrator"), ((-1, 1.0, 0.0, 0.0, 0.0), "unknown explicit integrator")]
    for bad in (np.nan, np.inf, -1.0):
        for k in range(4):
            args = [1.0, 0.06, 1.2, 5.0]
            args[k] = bad
            rows.append(((ex, *args), "finite and not negative"))
    rows += [((ex, 0.0, 0.06, 0.0, 0.0), "dilatational"), ((ex, 0.0, 0.0, 1.2, 0.0), "dilatational")]
    for args, word in rows:
        with pytest.raises(be.FemcyError, match=word) as refused:
            ctx.explicit_set_damping(*args)
        assert refused.value.status == -1, args
    ctx.explicit_set_damping(ex, 1.0, 0.0, 0.0, 0.0)                   # alpha alone needs no modulus
    ctx.explicit_start(ex, be.VEC_RHS, s)
    ctx.explicit_advance(ex, 2, h, be.VEC_RHS, s, 0.0)
    assert np.isfinite(ctx.download(be.VEC_DOF)).all()
    ctx.close()


def comm_refusal(backend):
    """once femcy_comm_init has run (the route of explicit_cases.comm_refusal; device only)"""
    nodes, el, ELE = ec.shape_mesh("C3D8-64")
    ctx = lc.make_ctx(nodes, el, ELE, backend)
    _, ex = ec.make_explicit(ctx, ELE, ec.held_dofs(nodes)[1])
    ctx.assemble_K(-1)
    iface = np.arange(0, ctx.n, 7, dtype=np.int32)
    ctx.comm_init(0, 1, be.Context.comm_unique_id(), iface, np.arange(iface.size, dtype=np.int32), iface.size,
                  np.ones(ctx.n, dtype=np.uint8))
    with pytest.raises(be.FemcyError, match="several ranks") as refused:
        ctx.explicit_set_damping(ex, 1.0, 0.0, 0.0, 0.0)
    assert refused.value.status == -1
    ctx.close()


# ------------------------------------------------------------------------------------- deck driver
TRAJ = {"bar": dict(alpha=200.0), "block": dict(alpha=10.0)}
TRAJ_CASES = [(case, mode) for case in TRAJ for mode in ("fixed", "auto")]
AUTO_SF = 0.9


def traj_deck(tmpdir, case, mode, damped=True):
    spec = ec.CASES[case]
    T = spec["dt"] * spec["steps"]
    dynamic = None if mode == "fixed" else eac.auto_dynamic(T, 1, AUTO_SF)
    if mode == "estimated":
        dynamic = "*Dynamic, explicit, scale factor=0.8\n, %r\n" % T
    if not damped:
        return deck_with(tmpdir, dynamic=dynamic, case=case), T
    return deck_with(tmpdir, "*Bulk Viscosity\n", "*Damping, alpha=%r\n" % TRAJ[case]["alpha"], dynamic=dynamic, case=case), T


@functools.lru_cache(maxsize=None)
def reference_traj(case, mode):
    """the long-double damped run of the deck (fixed: the records of every 8th of 200 steps; auto: every step), the error of
    the float64 one, and the kinetic energy at the end with and without damping"""
    import tempfile
    workdir = tempfile.mkdtemp()
    path, T = traj_deck(workdir, case, mode)
    nodes, el, ELE, mat = ec.write_case_deck(path + ".plain", case)
    inp, f, v0, fixed = ec.deck_loads(path)
    spec, ramp = ec.CASES[case], inp.amplitude == "RAMP"
    out = {}
    for dt in (LD, np.float64):
        mdl = edr.DampedModel(nodes, el, ELE, mat, dt, inp.density, TRAJ[case]["alpha"], 0.06, 1.2, modulus(mat))
        m = er.lumped_mass(nodes, el, ELE, inp.density, dt)
        minv = 1 / np.repeat(m, ELE.dm)
        minv[fixed] = 0
        if mode == "fixed":
            scale = (lambda k: k * spec["dt"] / T) if ramp else (lambda k: 1.0)
            U, V, _ = mdl.verlet_damped(minv, f, v0, spec["dt"], spec["steps"], scale)
            rec = np.arange(ec.EVERY, spec["steps"] + 1, ec.EVERY)
            out[dt] = (U[rec], V[rec], None)
            if dt is LD:
                plain = er.Model(nodes, el, ELE, mat, dt).verlet(minv, f, v0, spec["dt"], spec["steps"], scale)[1][-1]
                ke = (float(er.kinetic(m, V[-1], ELE.dm, dt)), float(er.kinetic(m, plain, ELE.dm, dt)))
        else:
            est = eac.Estimate(nodes, el, ELE, mat, inp.density, dt)
            H, times, U, V = edr.verlet_auto_damped(mdl, est, minv, f, v0, AUTO_SF, T, ramp)
            out[dt] = (U[1:], V[1:], H)
            if dt is LD:
                ke = None
    U, V, H = out[LD]
    U64, V64, H64 = out[np.float64]
    assert U64.shape == U.shape and np.isfinite(U.astype(np.float64)).all()
    e64 = max(relerr(U64, U), relerr(V64, V), 0.0 if H is None else float(np.abs(H64 - H).max() / H.max()))
    return {"U": U, "V": V, "H": H, "e64": e64, "ke": ke}


def trajectory(tmpdir, case, mode, backend):
    """the bar / block deck with `*Bulk Viscosity` (default data) and `*Damping, alpha=` through the deck driver: 200 fixed
    steps, or an `element by element` run, u and v (and the increments) against the long-double restatement.  Fixed, on the
    bar: the kinetic energy of the last batch is below that of the same deck undamped, which the reference shows with a factor
    of at least 2."""
    ref = reference_traj(case, mode)
    path, T = traj_deck(tmpdir, case, mode)
    inp, system, U, V = (ec.solve_deck if mode == "fixed" else eac.solve_auto)(path, backend)
    assert inp.bulk_viscosity == (0.06, 1.2) and inp.damping_alpha == TRAJ[case]["alpha"]
    assert system.increments[-1]["time1"] == T and U.shape == ref["U"].shape
    err = max(relerr(U, ref["U"]), relerr(V, ref["V"]))
    if mode == "auto":
        H = np.array([i["dt"] for i in system.increments])
        err = max(err, float(np.abs(H - ref["H"]).max() / ref["H"].max()))
        assert len(H) > 3
    print(f"{case} {mode} [{backend}]: {len(U)} records, damped trajectory {err:.3e}")
    if mode == "fixed":
        assert ref["ke"][0] * 2 <= ref["ke"][1], ref["ke"]             # the reference first: alpha was chosen so
        if case == "bar":
            plain = ec.solve_deck(traj_deck(tmpdir, case, mode, damped=False)[0], backend)[1]
            assert system.increments[-1]["kinetic"] < plain.increments[-1]["kinetic"]
    assert err <= 4.0 * F64_WORST_TRAJ[(case, mode)], err
    return err


def stable_dt(tmpdir, case, backend):
    """the increment estimated from the matrix: stable_dt is 2 / omega_b (sqrt(1 + xi^2) - xi), xi = b1 + alpha / (2 omega_b),
    with omega_b the restatement's Gershgorin bound (numpy on the host backend's K, the restatement's lumped mass).  A row
    sum of W terms carries (W - 1) eps, the product with minv, the square root and the formula's six operations a few more"""
    path, T = traj_deck(tmpdir, case, "estimated")
    nodes, el, ELE, mat = ec.write_case_deck(path + ".plain", case)
    inp, f, v0, fixed = ec.deck_loads(path)
    ctx = eac.make_ctx(nodes, el, ELE, mat, "cpu")
    ctx.assemble_K(-1)
    K = ctx.get_K_bsr().toarray()
    width = ctx.pattern_info().max_row_blocks * ELE.dm
    ctx.close()
    minv = 1 / np.repeat(er.lumped_mass(nodes, el, ELE, inp.density, LD), ELE.dm)
    minv[fixed] = 0
    om = LD(er.gershgorin(K, minv))
    xi = LD(0.06) + LD(TRAJ[case]["alpha"]) / (2 * om)
    want = float(2 / om * (np.sqrt(1 + xi * xi) - xi))
    _, system, U, _ = ec.solve_deck(path, backend)
    err = abs(system.stable_dt - want) / want
    print(f"{case} [{backend}]: damped stable_dt {system.stable_dt:.6e} ({err:.2e}), undamped {float(2 / om):.6e}")
    assert err <= (width + 10) * ec.EPS, err
    assert system.dt <= 0.8 * system.stable_dt and np.isfinite(U).all()
    return err


def measure_f64_worst():
    """the constants at the top, as measured"""
    return {"step": max(reference_step(n, (ALPHA, B1, B2))[1] for n in STEP_SHAPES),
            "term": max(reference_step(n, TERMS[w])[1] for n in TERM_SHAPES for w in TERMS),
            "omega": max(reference_omega(n)[1] for n in OMEGA_SHAPES),
            "dilation": max(relerr(dilation_closed_form(e, c, np.float64)[0], dilation_closed_form(e, c, LD)[0])
                            for e in ("C3D4", "CPS3") for c in (-40.0, 40.0)),
            "rigid": reference_rigid("C3D4")[1],
            "traj": {key: reference_traj(*key)["e64"] for key in TRAJ_CASES}}


