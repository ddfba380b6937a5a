"""The energy balance of explicit dynamics (femcy_explicit_energy_enable / _get, *Energy Output) written against the C ABI
(femcy_amd.backend.Context), the deck reader and the deck driver, so that the host backend (tests/test_energy_cpu.py) and the
device (tests/test_gpu_energy.py) run the same code.  Every function checks its own result and returns the figure it checked.

Reference.  `energy_sums` restates the four trapezoid sums of include/femcy.h in numpy, in any dtype, on top of the
trajectories of explicit_damped_reference / motion_reference (no library code runs there).  In np.longdouble it is the
reference; the same restatement in float64 differs from it by rounding, summation order and the rounding of its own
trajectory.  F64_WORST is the worst such difference over the cases run here (`measure_f64_worst`, asserted by
tests/test_energy_cpu.py), RELATIVE TO S = sum |addends| of the accumulator -- never to the result, whose terms cancel -- and
a backend is held to 4 x that, relative to the same S.

Split runs.  The library stores the forces of the last kicked state, so the accumulators of a split run are compared bit for
bit with those of one call."""
import functools
import os

import numpy as np
import pytest

from femcy_amd import backend as be

import explicit_auto_cases as eac
import explicit_cases as ec
import explicit_damped_cases as edc
import explicit_damped_reference as edr
import explicit_reference as er
import loads_cases as lc
import loads_reference as lr
import motion_cases as mc
import motion_reference as mr

LD = np.longdouble
RHO = ec.RHO
NAMES = ("LOAD", "INTERNAL", "ALPHA", "BOUNDARY")
# the float64 restatement against the long-double one relative to S, as measured (measure_f64_worst): the fixed runs
# 2.59e-15, the runs with motion 1.53e-15, the automatic runs 4.14e-15
F64_WORST = 4.2e-15
TOL = 4.0 * F64_WORST
N, PARTS = 24, (7, 17)
DAMPINGS = {"none": (0.0, 0.0, 0.0), "alpha": (edc.ALPHA, 0.0, 0.0), "bulk": (0.0, edc.B1, edc.B2),
            "both": (edc.ALPHA, edc.B1, edc.B2)}


def same_bits(x, y):
    return np.array_equal(np.asarray(x).view(np.uint64), np.asarray(y).view(np.uint64))


# ------------------------------------------------------------------------------------- restatement
def energy_sums(mdl, minv, m, f, U, V, A, H, S, moved=None):
    """the four sums over a run, in mdl.dtype.  U, V, A [K + 1, n]: the states; H [K]: the increment of step k; S [K + 1]:
    the load scale of state k; m [nn]; moved: the moved scalar DOFs.  -> W [4], sum |addends| [4]"""
    dt = mdl.dtype
    minv, f = np.asarray(minv, dtype=dt), np.asarray(f, dtype=dt)
    mdof = np.repeat(np.asarray(m, dtype=dt), mdl.dm)
    free = minv != 0
    md = np.zeros(minv.size, dtype=bool)
    if moved is not None:
        md[np.asarray(moved)] = True
    bulk = mdl.b1 != 0 or mdl.b2 != 0
    K = len(H)
    W, Sabs = np.zeros(4, dtype=dt), np.zeros(4, dtype=dt)
    prev = None
    for k in range(K + 1):
        vh_in = V[0] if k == 0 else V[k - 1] + dt(H[k - 1]) / 2 * A[k - 1]          # v_{k-1/2}, v_{-1/2} := v_0
        fint = mdl.f_int(U[k]) + (mdl.f_bv(U[k], vh_in) if bulk else 0)
        g = [dt(S[k]) * f, fint, mdl.alpha * mdof * vh_in * free, (mdof * A[k] + fint - dt(S[k]) * f) * md]
        if prev is not None:
            h = dt(H[k - 1])
            du = h * (V[k - 1] + h / 2 * A[k - 1]) * free
            du[md] = (U[k] - U[k - 1])[md]
            for j in range(4):
                add = du * (prev[j] + g[j]) / 2
                W[j] += add.sum()
                Sabs[j] += np.abs(add).sum()
        prev = g
    return W, Sabs


def check(got, ref, Sabs, what, extra=0.0):
    """|got - ref| <= TOL S, per accumulator; -> the worst ratio to S"""
    worst = 0.0
    for j in range(4):
        s = float(Sabs[j]) + extra
        d = float(abs(LD(got[j]) - ref[j]))
        print(f"{what}: {NAMES[j]} got {got[j]:.17e} ref {float(ref[j]):.17e} |diff| {d:.3e} S {s:.3e}")
        if s == 0.0:
            assert got[j] == 0.0, (what, NAMES[j], got[j])
            continue
        assert d <= TOL * s, (what, NAMES[j], d / s)
        worst = max(worst, d / s)
    return worst


# ------------------------------------------------------------------------------ fixed runs, no motion
SINGLE = {"single-CPS3": "CPS3", "single-C3D4": "C3D4"}
BIG = "CPS4-625"                                   # 313 wavefronts: more slots than one round of the read-back takes


@functools.lru_cache(maxsize=None)
def setup(key):
    """-> nodes, el, ELE, held DOFs, f, u0, v0, h: the state of explicit_cases.step_setup on any mesh.  key: a shape of
    explicit_cases, a single element, BIG, or (family, nn) of motion_cases"""
    if isinstance(key, tuple):
        nodes, el, ELE = mc.mesh(*key)
    elif key in SINGLE:
        nodes, el, ELE, _ = lr.single(SINGLE[key])
    elif key == BIG:
        nodes, el, ELE = lr.mesh("CPS4", cells=(24, 24), perturb=0.2)[:3]
    else:
        nodes, el, ELE = ec.shape_mesh(key)
    nodes = np.asarray(nodes, dtype=np.float64)
    rng = np.random.default_rng(11)
    _, fixed = ec.held_dofs(nodes)
    size = np.ptp(nodes, axis=0).max()
    u0 = 0.01 * size * rng.uniform(-1.0, 1.0, nodes.size)
    v0 = rng.uniform(-1.0, 1.0, nodes.size)
    f = rng.uniform(-1.0, 1.0, nodes.size)
    u0[fixed] = v0[fixed] = 0.0
    om = eac.Estimate(nodes, el, ELE, ec.material_of(ELE), RHO, np.float64).omega(np.zeros(nodes.size))
    h = 2.0 ** np.floor(np.log2(0.4 * 2.0 / float(om)))            # well inside the limit; a power of two: k h is exact
    return nodes, el, ELE, fixed, f, u0, v0, float(h)


def scale_of(ramp):
    return (lambda k: 0.25 + k / 64.0) if ramp else (lambda k: 0.75)


@functools.lru_cache(maxsize=None)
def reference_fixed(key, damping, ramp):
    """-> W, S in long double, the error of the float64 restatement relative to S, and the long-double left side of the
    identity with its magnitude"""
    nodes, el, ELE, fixed, f, u0, v0, h = setup(key)
    mat, coeffs, scale = ec.material_of(ELE), DAMPINGS[damping], scale_of(ramp)
    out = {}
    for dt in (LD, np.float64):
        mdl = edr.DampedModel(nodes, el, ELE, mat, dt, RHO, coeffs[0], coeffs[1], coeffs[2], edc.modulus(mat))
        m = er.lumped_mass(nodes, el, ELE, RHO, dt)
        minv = 1 / np.repeat(m, ELE.dm)
        minv[fixed] = 0
        U, V, A = mdl.verlet_damped(minv, f, v0, h, N, scale, u0=u0)
        out[dt] = energy_sums(mdl, minv, m, f, U, V, A, [h] * N, [scale(k) for k in range(N + 1)])
    (W, S), (W64, _) = out[LD], out[np.float64]
    e64 = max(float(abs(LD(W64[j]) - W[j]) / S[j]) for j in range(4) if S[j] != 0)
    return W, S, e64


def fixed_ctx(key, backend, damping, energy=True):
    nodes, el, ELE, fixed, f, u0, v0, h = setup(key)
    ctx = lc.make_ctx(nodes, el, ELE, backend)
    lm, ex = ec.make_explicit(ctx, ELE, fixed)
    for vec, arr in ((be.VEC_DOF, u0), (be.VEC_VEL, v0), (be.VEC_RHS, f)):
        ctx.upload(vec, arr)
    coeffs = DAMPINGS[damping]
    if any(coeffs):
        ctx.explicit_set_damping(ex, coeffs[0], coeffs[1], coeffs[2], edc.modulus(ec.material_of(ELE)))
    if energy:
        ctx.explicit_energy_enable(ex, True)
    return ctx, ex, lm, h


def run_fixed(ctx, ex, h, ramp, parts=(N,), hs=None):
    """start, then one advance per part (hs: the increment of each part) -> u, v, a"""
    scale = scale_of(ramp)
    ctx.explicit_start(ex, be.VEC_RHS, scale(0))
    done = 0
    for j, k in enumerate(parts):
        ctx.explicit_advance(ex, k, h if hs is None else hs[j], be.VEC_RHS, scale(done), scale(1) - scale(0))
        done += k
    return mc.state(ctx)


def fixed(key, damping, ramp, backend):
    """case 1 and 3: every accumulator of a fixed run against the long-double restatement of the whole run"""
    W, S, _ = reference_fixed(key, damping, ramp)
    ctx, ex, lm, h = fixed_ctx(key, backend, damping)
    run_fixed(ctx, ex, h, ramp)
    got = ctx.explicit_energy(ex)
    ctx.close()
    assert S[0] > 0 and S[1] > 0 and (S[2] > 0) == (DAMPINGS[damping][0] != 0) and S[3] == 0
    return check(got, W, S, f"{key} {damping} {'RAMP' if ramp else 'STEP'} [{backend}]")


def identity(key, damping, backend):
    """case 2: [KE - h^2/8 a.M a]_N - [..]_0 = W_LOAD - W_INTERNAL - W_ALPHA, the left side from the kinetic energy, the
    downloaded a and the lumped mass, the right side from the accumulators; held DOFs (a = 0, du = 0) contribute nothing"""
    W, S, _ = reference_fixed(key, damping, False)
    nodes, el, ELE, fixed, f, u0, v0, h = setup(key)
    ctx, ex, lm, h = fixed_ctx(key, backend, damping)
    m = np.repeat(ctx.lumped_mass_get(lm).astype(LD), ELE.dm)
    ctx.explicit_start(ex, be.VEC_RHS, 0.75)
    left, mag = [], 0.0
    for k in (0, N):
        if k:
            ctx.explicit_advance(ex, N, h, be.VEC_RHS, 0.75, 0.0)
        ke, a = LD(ctx.explicit_kinetic_energy(ex, be.VEC_VEL)), ctx.download(be.VEC_ACC).astype(LD)
        assert not a[fixed].any()
        corr = LD(h) ** 2 / 8 * (m * a * a).sum()
        left.append(ke - corr)
        mag += float(abs(ke) + abs(corr))
    got = ctx.explicit_energy(ex)
    ctx.close()
    lhs = left[1] - left[0]
    rhs = LD(got[0]) - LD(got[1]) - LD(got[2])
    s = float(S[0] + S[1] + S[2]) + mag
    d = float(abs(lhs - rhs))
    print(f"{key} {damping} [{backend}]: identity left {float(lhs):.17e} right {float(rhs):.17e} |diff| {d:.3e} S {s:.3e}")
    assert len(fixed) > 0 and float(abs(lhs)) > 1e-3 * float(S[0])         # held DOFs exist; the energy moved
    assert d <= TOL * s, d / s
    return d / s


def undisturbed_fixed(key, damping, backend):
    """case 4: u, v, a with the balance on equal those with it off, bit for bit; enable(0) after a run: the off run again"""
    runs = []
    for energy in (False, True):
        ctx, ex, lm, h = fixed_ctx(key, backend, damping, energy)
        runs.append(run_fixed(ctx, ex, h, True))
        if energy:
            assert np.abs(ctx.explicit_energy(ex)).max() > 0
            ctx.explicit_energy_enable(ex, False)
            nodes, el, ELE, fixed, f, u0, v0, _ = setup(key)
            ctx.upload(be.VEC_DOF, u0), ctx.upload(be.VEC_VEL, v0)
            runs.append(run_fixed(ctx, ex, h, True))
            with pytest.raises(be.FemcyError, match="not running"):
                ctx.explicit_energy(ex)
        ctx.close()
    for other in runs[1:]:
        assert all(same_bits(x, y) for x, y in zip(runs[0], other))
    assert np.abs(runs[0][1]).max() > 0


def split_fixed(key, damping, backend):
    """case 5: 24 steps in one call against 7 + 17, and 12 of h then 24 of h / 2 in one call each against 12 + (5 + 19):
    u, v, a and the accumulators bit for bit; a second start zeroes them"""
    out = []
    for parts, hs in (((N,), None), (PARTS, None), ((12, 24), (1.0, 0.5)), ((12, 5, 19), (1.0, 0.5, 0.5))):
        ctx, ex, lm, h = fixed_ctx(key, backend, damping)
        st = run_fixed(ctx, ex, h, False, parts, None if hs is None else [h * x for x in hs])
        out.append((st, ctx.explicit_energy(ex)))
        if parts == PARTS:
            ctx.explicit_start(ex, be.VEC_RHS, 0.75)
            assert not ctx.explicit_energy(ex).any()                   # a second start zeroes the sums
        ctx.close()
    for a, b in ((0, 1), (2, 3)):
        assert all(same_bits(x, y) for x, y in zip(out[a][0], out[b][0]))
        assert same_bits(out[a][1], out[b][1]), (out[a][1], out[b][1])
    assert not same_bits(out[0][1], out[2][1])


# -------------------------------------------------------------------------------------- with motion
MOTION = {"smooth": (mr.SMOOTH_STEP, None, 1.0), "tabular": (mr.TABULAR, None, 1.0), "damped": (mr.SMOOTH_STEP, mc.DAMPING, 1.0),
          # T of the curves = half the run: both tables end before the run does, du of every moved DOF becomes exactly 0
          "past-the-end": (mr.TABULAR, None, 0.4)}


@functools.lru_cache(maxsize=None)
def reference_motion(case, family, nn):
    kind, damping, frac = MOTION[case]
    T = frac * mc.STEPS * mc.H
    scale = lambda k: mc.RAMP["s0"] + k * mc.RAMP["ds"]
    out = {}
    for dt in (LD, np.float64):
        mdl, minv, m, motion, f, v0 = mc.model(family, nn, dt, kind, T, damping)
        U, V, A = mr.verlet_motion(mdl, minv, f, v0, mc.H, mc.STEPS, scale, motion)
        out[dt] = energy_sums(mdl, minv, m, f, U, V, A, [mc.H] * mc.STEPS, [scale(k) for k in range(mc.STEPS + 1)], motion.dofs)
        if dt is LD:
            still = bool((U[-1][motion.dofs] == U[-2][motion.dofs]).all())
    (W, S), (W64, _) = out[LD], out[np.float64]
    e64 = max(float(abs(LD(W64[j]) - W[j]) / S[j]) for j in range(4) if S[j] != 0)
    return W, S, e64, still


def motion(case, family, nn, backend):
    """case 1 with prescribed motion (three calls, a ramped load): BOUNDARY is the work of the supports"""
    kind, damping, frac = MOTION[case]
    W, S, _, still = reference_motion(case, family, nn)
    assert S[3] > 0 and still == (case == "past-the-end")
    ctx, ex, lm, ids = mc.make(family, nn, backend, kind, frac * mc.STEPS * mc.H, damping)
    ctx.explicit_energy_enable(ex, True)
    mc.run_fixed(ctx, ex)
    got = ctx.explicit_energy(ex)
    ctx.close()
    return check(got, W, S, f"{case} {family}-{nn} [{backend}]")


def undisturbed_motion(mode, family, nn, backend):
    """case 4 with motion and damping, fixed and automatic"""
    ELE = mc.mesh(family, nn)[2]
    runs = []
    for energy in (False, True):
        ctx, ex, _, _ = mc.make(family, nn, backend, mr.SMOOTH_STEP, mc.STEPS * mc.H, mc.DAMPING)
        if energy:
            ctx.explicit_energy_enable(ex, True)
        runs.append(mc.run_fixed(ctx, ex)[-1] if mode == "fixed" else mc.run_auto(ctx, ex, ELE, mc.auto_T(family, nn))[0])
        ctx.close()
    assert all(same_bits(x, y) for x, y in zip(*runs))


def split_motion(family, nn, backend):
    """case 5 with motion: the time of the last kicked state travels with the accumulators"""
    out = []
    for parts in ((mc.STEPS,), mc.PARTS):
        ctx, ex, _, _ = mc.make(family, nn, backend, mr.TABULAR, mc.STEPS * mc.H, mc.DAMPING)
        ctx.explicit_energy_enable(ex, True)
        st = mc.run_fixed(ctx, ex, parts)[-1]
        out.append((st, ctx.explicit_energy(ex)))
        ctx.close()
    assert all(same_bits(x, y) for x, y in zip(out[0][0], out[1][0])) and same_bits(out[0][1], out[1][1])


# ----------------------------------------------------------------------------------- automatic runs
@functools.lru_cache(maxsize=None)
def reference_auto(family, nn):
    nodes, el, ELE = mc.mesh(family, nn)
    T = mc.auto_T(family, nn)
    out = {}
    for dt in (LD, np.float64):
        mdl, minv, m, motion, f, v0 = mc.model(family, nn, dt, mr.SMOOTH_STEP, T, mc.DAMPING)
        est = eac.Estimate(nodes, el, ELE, ec.material_of(ELE), RHO, dt)
        Hs, times, U, V, A = mr.verlet_auto_motion(mdl, est, minv, f, v0, mc.AUTO_SF, T, True, motion)
        out[dt] = energy_sums(mdl, minv, m, f, U, V, A, Hs, [t / dt(T) for t in times], motion.dofs) + (len(Hs),)
    (W, S, steps), (W64, _, steps64) = out[LD], out[np.float64]
    assert steps == steps64
    e64 = max(float(abs(LD(W64[j]) - W[j]) / S[j]) for j in range(4) if S[j] != 0)
    return W, S, e64, steps


def auto(family, nn, backend):
    """case 1, element by element (damped, with motion, a ramped load): batches that end at T exactly after `steps` real
    steps; a further batch, all no-ops, leaves the accumulators bit for bit alone; a split run gives the same bits"""
    W, S, _, steps = reference_auto(family, nn)
    ELE = mc.mesh(family, nn)[2]
    T = mc.auto_T(family, nn)
    out = []
    for batches in ((steps + 9,), (7, 13, steps)):
        ctx, ex, _, _ = mc.make(family, nn, backend, mr.SMOOTH_STEP, T, mc.DAMPING)
        ctx.explicit_energy_enable(ex, True)
        st, clock, _ = mc.run_auto(ctx, ex, ELE, T, batches)
        got = ctx.explicit_energy(ex)
        assert clock[0] == T and clock[3] == steps                     # the batch overshot T
        ctx.explicit_auto_advance(ex, 5, be.VEC_RHS)                   # no-op steps
        assert same_bits(got, ctx.explicit_energy(ex)) and all(same_bits(x, y) for x, y in zip(st, mc.state(ctx)))
        out.append((st, got))
        ctx.close()
    assert all(same_bits(x, y) for x, y in zip(out[0][0], out[1][0])) and same_bits(out[0][1], out[1][1])
    return check(out[0][1], W, S, f"auto {family}-{nn} [{backend}]")


# ------------------------------------------------------------------------------- rigid translation
def rigid(backend, name="C3D4"):
    """case 6: a free mesh, uniform v_0, no load, alpha alone: INTERNAL is 0 to the tolerance, ALPHA is the kinetic energy
    lost"""
    nodes, el, ELE = ec.shape_mesh(name)
    r = edc.RIGID
    ctx = lc.make_ctx(nodes, el, ELE, backend)
    lm, ex = ec.make_explicit(ctx, ELE, [])
    ctx.upload(be.VEC_VEL, np.tile(r["v0"][:ELE.dm], len(nodes)))
    ctx.explicit_set_damping(ex, r["alpha"], 0.0, 0.0, 0.0)
    ctx.explicit_energy_enable(ex, True)
    ctx.explicit_start(ex, be.VEC_RHS, 0.0)
    ke0 = ctx.explicit_kinetic_energy(ex, be.VEC_VEL)
    ctx.explicit_advance(ex, r["steps"], r["h"], be.VEC_RHS, 0.0, 0.0)
    ke1 = ctx.explicit_kinetic_energy(ex, be.VEC_VEL)
    a = ctx.download(be.VEC_ACC).astype(LD)
    m = np.repeat(ctx.lumped_mass_get(lm).astype(LD), ELE.dm)
    got = ctx.explicit_energy(ex)
    ctx.close()
    # the identity with the start's a_0 = -alpha v_0: KE_0 - KE_N = W_ALPHA + (h^2 / 8)(a_0.M a_0 - a_N.M a_N)
    a0 = -LD(r["alpha"]) * np.tile(np.asarray(r["v0"][:ELE.dm], dtype=LD), len(nodes))
    corr = float(LD(r["h"]) ** 2 / 8 * ((m * a0 * a0).sum() - (m * a * a).sum()))
    lost = ke0 - ke1
    s = ke0 + abs(got[2])
    print(f"rigid {name} [{backend}]: ALPHA {got[2]:.17e}, kinetic energy lost {lost:.17e}, correction {corr:.3e}, "
          f"INTERNAL {got[1]:.3e}, LOAD {got[0]:.3e}")
    assert got[0] == 0.0 and got[3] == 0.0
    assert abs(got[1]) <= TOL * s, got[1]
    assert lost > 0.5 * ke0 and abs(got[2] + corr - lost) <= TOL * s + (len(nodes) + 4) * ec.EPS * ke0, (got[2], lost)
    return abs(got[2] + corr - lost) / s


# ----------------------------------------------------------------------------------------- refusals
def refusals(backend):
    """case 7: FEMCY_EINVAL with a word of the message, one by one, and the context keeps working"""
    ctx, ex, lm, h = fixed_ctx("C3D4", backend, "none", energy=False)
    out = np.zeros(4)
    rows = [(lambda: ctx.explicit_energy_enable(ex + 1, True), "unknown explicit integrator"),
            (lambda: ctx.explicit_energy_enable(-1, True), "unknown explicit integrator"),
            (lambda: ctx.explicit_energy(ex + 1), "unknown explicit integrator"),
            (lambda: ctx._call("femcy_explicit_energy_get", int(ex), None), "null output"),
            (lambda: ctx.explicit_energy(ex), "not running")]                           # off
    for call, word in rows:
        with pytest.raises(be.FemcyError, match=word) as refused:
            call()
        assert refused.value.status == -1, word
    ctx.explicit_energy_enable(ex, True)
    with pytest.raises(be.FemcyError, match="not running") as refused:                  # on, but before a start
        ctx.explicit_energy(ex)
    assert refused.value.status == -1
    ctx.explicit_start(ex, be.VEC_RHS, 0.75)
    assert not ctx.explicit_energy(ex).any()
    ctx.explicit_advance(ex, 2, h, be.VEC_RHS, 0.75, 0.0)
    assert np.isfinite(ctx.download(be.VEC_DOF)).all() and ctx.explicit_energy(ex)[:2].all()
    ctx.close()


def comm_refusal(backend):
    """once femcy_comm_init has run (the route of explicit_damped_cases.comm_refusal; device only)"""
    nodes, el, ELE = ec.shape_mesh("C3D8-64")
    ctx = lc.make_ctx(nodes, el, ELE, backend)
    _, ex = ec.make_explicit(ctx, ELE, ec.held_dofs(nodes)[1])
    ctx.assemble_K(-1)
    iface = np.arange(0, ctx.n, 7, dtype=np.int32)
    ctx.comm_init(0, 1, be.Context.comm_unique_id(), iface, np.arange(iface.size, dtype=np.int32), iface.size,
                  np.ones(ctx.n, dtype=np.uint8))
    for call in (lambda: ctx.explicit_energy_enable(ex, True), lambda: ctx.explicit_energy(ex)):
        with pytest.raises(be.FemcyError, match="several ranks") as refused:
            call()
        assert refused.value.status == -1
    ctx.close()


# ------------------------------------------------------------------------------------------- reader
def reader(tmpdir):
    """case 8"""
    from femcy_amd.reader import InpInfo
    assert InpInfo(edc.deck_with(tmpdir)).energy_output is False
    for lines in ("*Energy Output\n", "*Output, history\n*Energy Output\n", "*Energy Output\nALLKE, ALLSE\nALLIE, ALLWK, ALLVD, ETOTAL\n",
                  "*Output, history, frequency=10\n*Energy Output\nETOTAL\n"):
        inp = InpInfo(edc.deck_with(tmpdir, lines))
        assert inp.energy_output is True and inp.procedure == "explicit", lines
    with pytest.raises(ValueError, match="ALLPD"):
        InpInfo(edc.deck_with(tmpdir, "*Energy Output\nALLKE, ALLPD\n"))
    for dynamic, word in (("*Static\n1., 1., 1e-05, 1.\n", "Energy Output"), ("*Dynamic, direct\n1e-4, 1e-3\n", "Energy Output")):
        with pytest.raises(ValueError, match=word):
            InpInfo(edc.deck_with(tmpdir, "*Energy Output\n", dynamic=dynamic))
    decks = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "decks")
    names = sorted(n for n in os.listdir(decks) if n.endswith(".inp"))
    assert names
    for n in names:
        assert InpInfo(os.path.join(decks, n)).energy_output is False, n


# ------------------------------------------------------------------------------------------- driver
NEW_KEYS = ("external_work", "boundary_work", "internal_work", "viscous_dissipation", "energy_total")
DRIVER_CASE, DRIVER_ALPHA = "bar", 200.0
# x the driver's own (Gershgorin, conservative) estimate of the limit: up to 1.32 the bar is still stable, from 1.325 on the
# restatement inverts an element before step 200; here its drift is 40 times the bound and every displacement a number
UNSTABLE_SF = 1.322


def driver_deck(tmpdir, energy=True, dt=None):
    spec = ec.CASES[DRIVER_CASE]
    steps = spec["steps"]
    h = float(spec["dt"] if dt is None else dt)
    dynamic = "*Dynamic, explicit, direct user control, output_every=%d\n%r, %r\n" % (ec.EVERY, h, h * steps)
    return edc.deck_with(tmpdir, ("*Bulk Viscosity\n" + ("*Output, history\n*Energy Output\nETOTAL\n" if energy else "")),
                         "*Damping, alpha=%r\n" % DRIVER_ALPHA, dynamic=dynamic, case=DRIVER_CASE), h, steps


@functools.lru_cache(maxsize=None)
def reference_driver(dt=None):
    """the long-double restatement of the driver deck: energy_total of every state and its largest drift from state 0"""
    import tempfile
    workdir = tempfile.mkdtemp()
    path, h, steps = driver_deck(workdir, True, dt)
    nodes, el, ELE, mat = ec.write_case_deck(path + ".plain", DRIVER_CASE)
    inp, f, v0, fixed = ec.deck_loads(path)
    ramp = inp.amplitude == "RAMP"
    scale = (lambda k: k / steps) if ramp else (lambda k: 1.0)
    mdl = edr.DampedModel(nodes, el, ELE, mat, LD, inp.density, DRIVER_ALPHA, 0.06, 1.2, edc.modulus(mat))
    m = er.lumped_mass(nodes, el, ELE, inp.density, LD)
    minv = 1 / np.repeat(m, ELE.dm)
    minv[fixed] = 0
    U, V, A = mdl.verlet_damped(minv, f, v0, h, steps, scale)
    total = []
    for k in range(0, steps + 1, ec.EVERY):
        W, _ = energy_sums(mdl, minv, m, f, U[:k + 1], V[:k + 1], A[:k + 1], [h] * k, [scale(j) for j in range(k + 1)])
        total.append(er.kinetic(m, V[k], ELE.dm, LD) + W[1] + W[2] - W[0] - W[3])
    total = np.array(total)
    return float(np.abs(total - total[0]).max()), bool(np.isfinite(U.astype(np.float64)).all())


def stable_limit(tmpdir):
    """2 / omega of the driver deck's matrix, damping included, as the driver estimates it (host backend)"""
    path = edc.traj_deck(tmpdir, DRIVER_CASE, "estimated")[0]
    return ec.solve_deck(path, "cpu")[1].stable_dt


def driver(tmpdir, backend):
    """case 9: the records carry the new keys; energy_total stays within 4 x the restatement's own largest drift; past the
    limit the restatement's drift grows by more than ten times that bound and the driver's grows too, with nothing but
    numbers in the displacements; without the keyword the records are today's"""
    drift_ref, _ = reference_driver()
    bound = 4.0 * drift_ref
    path, h, steps = driver_deck(tmpdir, True)
    inp, system, U, V = ec.solve_deck(path, backend)
    assert inp.energy_output is True
    recs = [system.initial_energy] + list(system.increments)
    for r in recs:
        assert all(k in r and np.isfinite(r[k]) for k in NEW_KEYS), r
    assert all(recs[0][k] == 0.0 for k in NEW_KEYS[:4]) and recs[0]["energy_total"] == recs[0]["kinetic"]
    drift = max(abs(r["energy_total"] - recs[0]["energy_total"]) for r in recs)
    print(f"driver [{backend}]: drift of energy_total {drift:.6e}, the restatement's {drift_ref:.6e}, bound {bound:.6e}")
    assert recs[-1]["viscous_dissipation"] > 0.0
    assert drift <= bound, (drift, bound)
    # past the limit
    h_bad = float(UNSTABLE_SF * stable_limit(tmpdir))
    drift_bad_ref, finite = reference_driver(h_bad)
    assert finite and drift_bad_ref > 10.0 * bound, (drift_bad_ref, bound)
    _, bad, U_bad, _ = ec.solve_deck(driver_deck(tmpdir, True, h_bad)[0], backend)
    recs_bad = [bad.initial_energy] + list(bad.increments)
    drift_bad = max(abs(r["energy_total"] - recs_bad[0]["energy_total"]) for r in recs_bad)
    print(f"driver [{backend}]: past the limit (dt = {h_bad:.4e}) drift {drift_bad:.6e}, the restatement's {drift_bad_ref:.6e}")
    assert np.isfinite(U_bad).all() and drift_bad > 10.0 * bound, (drift_bad, bound)
    # without the keyword
    _, plain, U_plain, _ = ec.solve_deck(driver_deck(tmpdir, False)[0], backend)
    assert same_bits(U_plain, U)
    for r, q in zip([plain.initial_energy] + list(plain.increments), recs):
        assert set(r) == set(q) - set(NEW_KEYS) and all(r[k] == q[k] for k in r), (r, q)
    return drift


# --------------------------------------------------------------------------------------- the cases
FIXED_CASES = ([("C3D4-150", d, r) for d in ("none", "alpha", "bulk", "both") for r in (False, True)]
               + [(k, "both", True) for k in ("single-CPS3", "single-C3D4", "fan", "C3D10", "CPS4-65", BIG)]
               + [((fam, nn), "both", True) for fam in mc.FAMILIES for nn in (7, 8, 9)])
IDENTITY_CASES = [("C3D4-150", d) for d in ("none", "alpha", "bulk", "both")] + [("CPS4-65", "both")]
MOTION_CASES = [("smooth", "C3D4", 9), ("tabular", "C3D4", 9), ("tabular", "CPS4", 8), ("damped", "CPS4", 17),
                ("past-the-end", "C3D4", 16), ("past-the-end", "CPS4", 7)]
AUTO_CASES = [("C3D4", 9), ("CPS4", 16)]


def measure_f64_worst():
    """F64_WORST, as measured"""
    return {"fixed": max(reference_fixed(*c)[2] for c in FIXED_CASES),
            "motion": max(reference_motion(*c)[2] for c in MOTION_CASES),
            "auto": max(reference_auto(*c)[2] for c in AUTO_CASES)}
