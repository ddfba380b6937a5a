"""Frictionless rigid walls of explicit dynamics (femcy_explicit_set_wall / _wall_get, *Rigid Wall) written against the C ABI
(femcy_amd.backend.Context), the deck reader and the deck driver, so that the host backend (tests/test_wall_cpu.py) and the
device (tests/test_gpu_wall.py) run the same code.  Every function checks its own result and returns the figure it checked.

Reference.  wall_reference.WallModel restates the law in numpy on top of explicit_damped_reference / motion_reference, in any
dtype.  In np.longdouble it is the reference; in float64 it differs from it by rounding.  F64_WORST is the worst such
difference of u, v, a over the trajectories run here, relative to the largest entry of the reference (`measure_f64_worst`,
asserted by tests/test_wall_cpu.py); a backend is held to 4 x that.  The energy accumulators are held to energy_cases.TOL.
The force law itself is compared bit for bit (wall_reference.exact_a0) where the rest of the acceleration is exactly 0."""
import functools
import os

import numpy as np
import pytest

from femcy_amd import backend as be

import energy_cases as enc
import explicit_auto_cases as eac
import explicit_cases as ec
import explicit_damped_cases as edc
import explicit_reference as er
import loads_cases as lc
import loads_reference as lr
import motion_cases as mc
import motion_reference as mr
import wall_reference as wr

LD = np.longdouble
RHO = ec.RHO
# the float64 restatement against the long-double one over TRAJ_CASES, as measured (measure_f64_worst): fixed 5.01e-14,
# element by element 7.0e-14
F64_WORST = 7.0e-14
TOL = 4.0 * F64_WORST
N, PARTS = 64, (5, 17, 42)
SF, AUTO_BATCHES = 0.5, (16, 16, 48)
DAMPINGS = {"none": (0.0, 0.0, 0.0), "both": (edc.ALPHA, edc.B1, edc.B2)}
NORMALS = {2: np.array([0.6, 0.8]), 3: np.array([2.0, -1.0, 2.0])}
same_bits, relerr = mc.same_bits, mc.relerr


def make_ctx(nodes, el, ELE, backend, held=()):
    ctx = lc.make_ctx(nodes, el, ELE, backend)
    lm = ctx.lumped_mass(ELE, RHO)
    ids = [ctx.dofset(np.asarray(s, dtype=np.int32)) for s in held]
    return ctx, lm, ctx.explicit(lm, ids), ids


def through(nodes, normal, frac=0.35, shift=0.0):
    """a wall with `normal` that leaves about frac of the nodes behind it"""
    n = np.asarray(normal, dtype=np.float64)
    s = np.sort(np.asarray(nodes) @ n / np.linalg.norm(n))
    k = max(1, int(frac * len(s)))
    return (0.5 * (s[k - 1] + s[k]) + shift) * n / np.linalg.norm(n), n


# ------------------------------------------------------------------------------------- 1: the force law
def force_law(nodes, el, ELE, walls, backend, held_nodes=(1,)):
    """a_0 at u = 0 under no load: bit for bit the wall term on the free DOFs, 0 on the held ones and outside; wall_get
    against the long-double sums.  -> the worst relative error of wall_get"""
    nodes = np.asarray(nodes, dtype=np.float64)
    dm = ELE.dm
    held = np.concatenate([np.arange(dm) + a * dm for a in held_nodes]) if len(held_nodes) else np.zeros(0, np.int32)
    ctx, lm, ex, _ = make_ctx(nodes, el, ELE, backend, [held] if held.size else [])
    ctx.explicit_set_wall(ex, [w[0] for w in walls], [w[1] for w in walls], [w[2] for w in walls])
    for vec in (be.VEC_DOF, be.VEC_VEL, be.VEC_RHS):
        ctx.upload(vec, np.zeros(nodes.size))
    ctx.upload(be.VEC_ACC, np.full(nodes.size, np.nan))
    ctx.explicit_start(ex, be.VEC_RHS, 1.0)
    a = ctx.download(be.VEC_ACC)
    got = [ctx.explicit_wall_get(ex, k) for k in range(len(walls))]
    ctx.close()
    m = er.lumped_mass(nodes, el, ELE, RHO, LD)
    minv = np.ones(nodes.size)
    minv[held] = 0.0
    want = wr.exact_a0(nodes, walls, minv)
    assert np.abs(want).max() > 0 and same_bits(a, want), np.abs(a - want).max()
    assert not a[held].any()
    mdl = wr.WallModel(nodes, el, ELE, ec.material_of(ELE), LD, RHO, walls)
    g = mdl.gaps(np.zeros(nodes.size))
    outside = np.repeat((g > 0).all(axis=0), dm)
    assert not a[outside].any() and (g < 0).any() and (outside.any() or len(nodes) < 16)
    err = 0.0
    for k in range(len(walls)):
        ref = mdl.wall_get(k, np.zeros(nodes.size), m, minv)
        assert got[k][2] == float(ref[2]) > 0, (got[k], ref)
        err = max([err] + [float(abs(LD(got[k][j]) - ref[j]) / ref[j]) for j in (0, 1, 3)])
    assert err <= (len(nodes) + 8) * ec.EPS, err
    return err


def law_case(family, which, backend):
    nodes, el, ELE = mc.mesh(family, 17)
    p, n = through(nodes, NORMALS[ELE.dm])
    walls = [(p, n, 3.0e4)]
    if which == "corner":
        e = np.zeros(ELE.dm)
        e[0] = -1.0
        walls.append(through(nodes, e, frac=0.3) + (7.0e3,))
    return force_law(nodes, el, ELE, walls, backend)


# ------------------------------------------------------------------------------------- 2: trajectories
FAMILIES = ("CPS4", "C3D4")
VARIANTS = ("plain", "motion", "energy", "motion+energy")
TRAJ_CASES = [(mode, v, fam, d) for mode in ("fixed", "auto") for v in VARIANTS for fam in FAMILIES for d in ("none", "both")]
NN = 16


@functools.lru_cache(maxsize=None)
def setup(family, moved):
    """a body flying towards an oblique wall at 2.7 increments' distance: nodes, el, ELE, the wall, the held (moved) DOFs of
    the node farthest from it, f, v0, h, the curve and its value"""
    nodes, el, ELE = mc.mesh(family, NN)
    nodes = np.asarray(nodes, dtype=np.float64)
    dm = ELE.dm
    n = NORMALS[dm] / np.linalg.norm(NORMALS[dm])
    size = np.ptp(nodes, axis=0).max()
    om = float(eac.Estimate(nodes, el, ELE, ec.material_of(ELE), RHO, np.float64).omega(np.zeros(nodes.size)))
    h = float(2.0 ** np.floor(np.log2(0.4 * 2.0 / om)))
    kappa = (np.pi / (5.0 * h)) ** 2                        # a node alone would stay in contact for 5 increments
    speed = 0.0005 * size / h
    proj = nodes @ n
    point = (proj.min() - 2.7 * h * speed) * n
    rng = np.random.default_rng(3)
    v0 = np.tile(-speed * n, len(nodes)) * (1.0 + 0.02 * rng.uniform(-1.0, 1.0, nodes.size))
    # the load pushes the body away from the wall, hard enough to turn it round on its own half way through the run: it
    # has left the wall for good by the end, however its nodes bounce in between
    m = er.lumped_mass(nodes, el, ELE, RHO, np.float64)
    f = np.repeat(m, dm) * np.tile(n, len(nodes)) * (4.0 * speed / (0.375 * N * h)) * (1.0 + 0.1 * rng.uniform(-1.0, 1.0, nodes.size))
    held = np.arange(dm) + int(proj.argmax()) * dm if moved else np.zeros(0, np.int64)
    v0[held] = 0.0
    curve = (mr.SMOOTH_STEP, [0.0, 0.75 * N * h], [0.0, 1.0])
    return nodes, el, ELE, (point, n, kappa), held, f, v0, h, curve, -0.004 * size


def scale(k):
    return 0.25 + k / 64.0


def model(family, moved, damping, dt):
    nodes, el, ELE, wall, held, f, v0, h, curve, g = setup(family, moved)
    mat, c = ec.material_of(ELE), DAMPINGS[damping]
    mdl = wr.WallModel(nodes, el, ELE, mat, dt, RHO, [wall], c[0], c[1], c[2], edc.modulus(mat))
    m = er.lumped_mass(nodes, el, ELE, RHO, dt)
    minv = 1 / np.repeat(m, ELE.dm)
    minv[held] = 0
    motion = mr.Motion([(held, g, curve)] if moved else [], dt)
    return mdl, minv, m, motion


def auto_T(family, moved):
    nodes, el, ELE, wall, held, f, v0, h, curve, g = setup(family, moved)
    return N * h


@functools.lru_cache(maxsize=None)
def reference(mode, moved, family, damping):
    """-> the long-double run (fixed: U, V, A; auto: H, times, U, V, A), the states compared, the error of the float64
    restatement there, the long-double energy sums (W, S) and wall_get at the end"""
    nodes, el, ELE, wall, held, f, v0, h, curve, g = setup(family, moved)
    out = {}
    for dt in (LD, np.float64):
        mdl, minv, m, motion = model(family, moved, damping, dt)
        if mode == "fixed":
            U, V, A = mr.verlet_motion(mdl, minv, f, v0, h, N, scale, motion)      # no entries: nothing is moved
            Hs, S = [h] * N, [scale(k) for k in range(N + 1)]
            run = (U, V, A)
        else:
            est = eac.Estimate(nodes, el, ELE, ec.material_of(ELE), RHO, dt)
            T = auto_T(family, moved)
            Hs, times, U, V, A = mr.verlet_auto_motion(mdl, est, minv, f, v0, SF, T, True, motion)
            S = [t / dt(T) for t in times]
            run = (Hs, times, U, V, A)
        counts = np.array(mdl.counts)[:, 0]
        if dt is LD:
            # the body starts outside, enters, and has left again by the end of the run
            assert counts[0] == 0 and counts.max() >= 1 and counts[-1] == 0, counts
            W = enc.energy_sums(mdl, minv, m, f, U, V, A, Hs, S, held if moved else None)
            got = mdl.wall_get(0, U[int(np.argmax(counts))], m, minv)
        out[dt] = run
    if mode == "fixed":
        ends = list(np.cumsum(PARTS))
        pairs = list(zip(out[np.float64], out[LD]))
    else:
        K = len(out[LD][0])
        assert len(out[np.float64][0]) == K and 30 <= K < sum(AUTO_BATCHES), K
        ends = [k for k in np.cumsum(AUTO_BATCHES) if k < K] + [K]
        pairs = list(zip(out[np.float64][2:], out[LD][2:]))
    e64 = max(relerr(x64[k], x[k]) for x64, x in pairs for k in ends)
    return out[LD], ends, e64, W, (int(np.argmax(counts)), got)


def make(family, moved, damping, energy, backend, wall=True, far=False):
    nodes, el, ELE, w, held, f, v0, h, curve, g = setup(family, moved)
    ctx, lm, ex, ids = make_ctx(nodes, el, ELE, backend, [held] if moved else [])
    if moved:
        amp = ctx.amplitude("smooth step", curve[1], curve[2])
        ctx.explicit_set_motion(ex, ids, [g], [amp])
    c = DAMPINGS[damping]
    if any(c):
        ctx.explicit_set_damping(ex, c[0], c[1], c[2], edc.modulus(ec.material_of(ELE)))
    if energy:
        ctx.explicit_energy_enable(ex, True)
    if wall:
        point = w[0] - (1.0e3 * np.ptp(nodes, axis=0).max() * w[1] if far else 0.0)
        ctx.explicit_set_wall(ex, [point], [w[1]], [w[2]])
    ctx.upload(be.VEC_DOF, np.zeros(nodes.size))
    ctx.upload(be.VEC_VEL, v0)
    ctx.upload(be.VEC_RHS, f)
    ctx.upload(be.VEC_ACC, np.full(nodes.size, np.nan))
    return ctx, ex, lm


def run(ctx, ex, mode, family, moved, parts=None):
    """-> (state, clock or None) after every call"""
    nodes, el, ELE, w, held, f, v0, h, curve, g = setup(family, moved)
    out = []
    if mode == "fixed":
        ctx.explicit_start(ex, be.VEC_RHS, scale(0))
        done = 0
        for k in parts or PARTS:
            ctx.explicit_advance(ex, k, h, be.VEC_RHS, scale(done), scale(1) - scale(0))
            done += k
            out.append((mc.state(ctx), None))
    else:
        ctx.explicit_auto_begin(ex, float(eac.s_C(ec.material_of(ELE))), SF, auto_T(family, moved), True, be.VEC_RHS)
        for k in parts or AUTO_BATCHES:
            ctx.explicit_auto_advance(ex, k, be.VEC_RHS)
            out.append((mc.state(ctx), ctx.explicit_auto_state(ex)))
    return out


def trajectory(mode, variant, family, damping, backend):
    """u, v, a (and the clock) after every call against long double; the energy accumulators; wall_get at the end; an
    automatic run's steps past T write nothing"""
    moved, energy = "motion" in variant, "energy" in variant
    ref, ends, _, W, _ = reference(mode, moved, family, damping)
    ctx, ex, lm = make(family, moved, damping, energy, backend)
    got = run(ctx, ex, mode, family, moved)
    en = ctx.explicit_energy(ex) if energy else None
    wall = ctx.explicit_wall_get(ex, 0)
    if mode == "auto":
        ctx.explicit_auto_advance(ex, 5, be.VEC_RHS)
        assert all(same_bits(x, y) for x, y in zip(got[-1][0], mc.state(ctx))) and ctx.explicit_auto_state(ex) == got[-1][1]
    ctx.close()
    err = 0.0
    if mode == "fixed":
        U, V, A = ref
        for k, (st, _) in zip(ends, got):
            err = max([err] + [relerr(x, w[k]) for x, w in zip(st, (U, V, A))])
    else:
        Hs, times, U, V, A = ref
        assert got[-1][1][0] == auto_T(family, moved) and got[-1][1][3] == len(Hs), got[-1][1]
        for k, (st, clk) in zip(ends, got):
            assert clk[3] == k, (clk, k)
            err = max([err, float(abs(LD(clk[0]) - times[k]) / times[-1]), float(abs(LD(clk[1]) - Hs[k - 1]) / Hs.max())]
                      + [relerr(x, w[k]) for x, w in zip(st, (U, V, A))])
    print(f"{mode} {variant} {family} {damping} [{backend}]: u, v, a at the call ends {err:.3e}")
    assert err <= TOL, err
    assert wall[2] == 0.0 and wall[0] == 0.0 and wall[1] == 0.0 and wall[3] == 0.0, wall      # the body has left
    if energy:
        enc.check(en, W[0], W[1], f"{mode} {variant} {family} {damping} [{backend}]")
    return err


def in_contact(family, backend):
    """wall_get in the state of the reference with the most nodes inside, against the long-double sums"""
    (U, V, A), ends, _, _, (k, ref) = reference("fixed", False, family, "none")
    ctx, ex, lm = make(family, False, "none", False, backend)
    run(ctx, ex, "fixed", family, False, parts=(k,))
    got = ctx.explicit_wall_get(ex, 0)
    ctx.close()
    assert got[2] == float(ref[2]) >= 1, (got, ref)
    err = max(float(abs(LD(got[j]) - ref[j]) / ref[j]) for j in (0, 1, 3))
    assert err <= 1.0e3 * TOL, err          # the depth is the difference of two positions: 1e-3 of them, three digits fewer
    return err


# -------------------------------------------------------------------------------------------- 3: bits
def split(mode, energy, backend, family="C3D4"):
    runs = []
    for parts in ((sum(PARTS),), PARTS) if mode == "fixed" else ((sum(AUTO_BATCHES),), AUTO_BATCHES):
        ctx, ex, _ = make(family, True, "both", energy, backend)
        st, clk = run(ctx, ex, mode, family, True, parts)[-1]
        runs.append(st + ([ctx.explicit_energy(ex)] if energy else []) + ([np.array(clk)] if clk else []))
        ctx.close()
    assert all(same_bits(x, y) for x, y in zip(*runs))


def no_wall_bits(mode, how, backend, family="CPS4"):
    """how = "removed": set_wall(nwalls = 0) after a wall was set; "unreached": a wall far behind the body (a fixed run: an
    automatic one takes other increments as soon as a wall is set, reached or not).  Both against an integrator that never
    had a wall: u, v, a and the four accumulators, bit for bit"""
    runs = []
    for k in range(2):
        ctx, ex, _ = make(family, True, "both", True, backend, wall=(k == 1), far=(how == "unreached"))
        if k == 1 and how == "removed":
            ctx.explicit_set_wall(ex)
            with pytest.raises(be.FemcyError):
                ctx.explicit_wall_get(ex, 0)
        st, clk = run(ctx, ex, mode, family, True)[-1]
        runs.append(st + [ctx.explicit_energy(ex)] + ([np.array(clk)] if clk else []))
        if k == 1 and how == "unreached":
            assert not ctx.explicit_wall_get(ex, 0).any()
        ctx.close()
    assert all(same_bits(x, y) for x, y in zip(*runs))


# --------------------------------------------------------------------------------------- 5: increment
def bound(family, damping, backend):
    """the element bound at u = 0 with two walls: sqrt(omega_e^2 + kappa) maximised over the elements, the damping factor
    after it, against the restatement"""
    nodes, el, ELE, w, held, f, v0, h, curve, g = setup(family, False)
    mat, c = ec.material_of(ELE), DAMPINGS[damping]
    walls = [w, (w[0], -w[1], 0.37 * w[2])]
    mdl = wr.WallModel(nodes, el, ELE, mat, LD, RHO, walls, c[0], c[1], c[2], edc.modulus(mat))
    est = eac.Estimate(nodes, el, ELE, mat, RHO, LD)
    ctx, lm, ex, _ = make_ctx(nodes, el, ELE, backend)
    if any(c):
        ctx.explicit_set_damping(ex, c[0], c[1], c[2], edc.modulus(mat))
    ctx.upload(be.VEC_DOF, np.zeros(nodes.size))
    ctx.upload(be.VEC_VEL, v0)
    s_C = float(eac.s_C(mat))
    plain = ctx.explicit_element_bound(ex, s_C)
    ctx.explicit_set_wall(ex, [x[0] for x in walls], [x[1] for x in walls], [x[2] for x in walls])
    got = ctx.explicit_element_bound(ex, s_C)
    ctx.close()
    want = mdl.omega_eff(est, np.zeros(nodes.size, dtype=LD), np.asarray(v0, dtype=LD))
    err = float(abs(LD(got) - want) / want)
    print(f"bound {family} {damping} [{backend}]: {got:.17e} against {float(want):.17e}: {err:.3e}")
    assert got > plain and err <= 4.0 * max(eac.F64_WORST_BOUND, edc_bound_worst()), err
    if damping == "none":
        assert abs(got * got - (plain * plain + 1.37 * w[2])) <= 8 * ec.EPS * got * got
    return err


def edc_bound_worst():
    return getattr(edc, "F64_WORST_BOUND", eac.F64_WORST_BOUND)


# ------------------------------------------------------------------------------------------ 6: shapes
def shape_mesh(nn):
    """nn nodes: the ring of motion_cases round a hub (odd nn), a CPS4 grid otherwise"""
    if nn % 2:
        nodes, el = mc.ring_quads(nn // 2)
        return nodes, el, lr.mesh("CPS4", cells=(1, 1))[2]
    a = {8: (3, 1), 256: (15, 15)}[nn]
    return lr.mesh("CPS4", cells=a, perturb=0.2)[:3]


def shape(nn, backend):
    """the node pass and the read-back at a node count: contacts planted in the first node (the hub of a ring: a gather of
    several trips at 257 and 513), the last node and both halves of a wavefront; the force law bit for bit"""
    nodes, el, ELE = shape_mesh(nn)
    nodes = np.asarray(nodes, dtype=np.float64)
    # a corner of two walls whose far sides hold node 0, node 1 (the other half of wavefront 0) and the last node
    c = nodes[[0, 1, nn - 1]].mean(axis=0)
    walls = []
    for k, a in enumerate((0, nn - 1)):
        n = c - nodes[a]
        walls.append((nodes[a] + (0.31 + 0.2 * k) * n, n, 2.0e4 * (k + 1)))
    n = c - nodes[1]
    walls.append((nodes[1] + 0.27 * n, n, 1.1e4))
    return force_law(nodes, el, ELE, walls, backend, held_nodes=(2,))


def fan(k, backend):
    """k triangles round one hub that is in contact: the gather takes a second (33) and a third (65) trip before the exchange"""
    nodes, el, ELE = fan_mesh(k)
    nodes = np.asarray(nodes, dtype=np.float64)
    hub = int(np.bincount(np.asarray(el).ravel()).argmax())
    far = nodes[np.argmax(np.linalg.norm(nodes - nodes[hub], axis=1))]
    n = far - nodes[hub]
    return force_law(nodes, el, ELE, [(nodes[hub] + 0.013 * n, n, 5.0e4)], backend, held_nodes=())


def fan_mesh(k):
    """k CPS3 triangles round one hub"""
    from femcy_amd.element_zoo import Element_linear_triangular
    t = 2 * np.pi * np.arange(k) / k
    r = 1.0 + 0.1 * np.cos(5 * t)
    nodes = np.vstack([[0.02, 0.01], np.column_stack([r * np.cos(t), r * np.sin(t)])])
    el = np.array([[0, 1 + i, 1 + (i + 1) % k] for i in range(k)], np.int32)
    return nodes, el, Element_linear_triangular()


def single(etype, backend):
    """the smallest mesh there is, one element: the read-back's one, mostly empty workgroup (no mesh has a single node)"""
    nodes, el, ELE, _ = lr.single(etype)
    p, n = through(nodes, NORMALS[ELE.dm], frac=0.4)
    return force_law(nodes, el, ELE, [(p, n, 2.5e4)], backend, held_nodes=())


def four_walls(backend, family="C3D4"):
    """four walls at once: the first alone gives the same wall_get for wall 0, and a_0 is the sum in ascending order"""
    nodes, el, ELE = mc.mesh(family, 17)
    dm = ELE.dm
    walls = []
    for k in range(4):
        e = np.zeros(dm)
        e[k % dm] = 1.0 if k < dm else -1.0
        e[(k + 1) % dm] = 0.25
        walls.append(through(nodes, e, frac=0.2 + 0.1 * k) + (1.0e4 * (k + 1),))
    return force_law(nodes, el, ELE, walls, backend)


# --------------------------------------------------------------------------------------- 7: refusals
def refusals(backend):
    nodes, el, ELE = mc.mesh("CPS4", 9)
    ctx, lm, ex, _ = make_ctx(nodes, el, ELE, backend)
    p, n, k = [0.0, 0.0], [1.0, 0.0], [10.0]
    ptr = be._ptr
    arr = lambda x: np.ascontiguousarray(x, dtype=np.float64)
    P, Nn, K = arr(p), arr(n), arr(k)
    out = np.zeros(4)
    bad = [
        ("unknown id", lambda: ctx.explicit_set_wall(ex + 1, [p], [n], k)),
        ("5 walls", lambda: ctx.explicit_set_wall(ex, [p] * 5, [n] * 5, k * 5)),
        ("-1 walls", lambda: ctx._call("femcy_explicit_set_wall", ex, -1, ptr(P), ptr(Nn), ptr(K))),
        ("null point", lambda: ctx._call("femcy_explicit_set_wall", ex, 1, None, ptr(Nn), ptr(K))),
        ("null normal", lambda: ctx._call("femcy_explicit_set_wall", ex, 1, ptr(P), None, ptr(K))),
        ("null kappa", lambda: ctx._call("femcy_explicit_set_wall", ex, 1, ptr(P), ptr(Nn), None)),
        ("nan point", lambda: ctx.explicit_set_wall(ex, [[np.nan, 0.0]], [n], k)),
        ("inf normal", lambda: ctx.explicit_set_wall(ex, [p], [[np.inf, 0.0]], k)),
        ("nan kappa", lambda: ctx.explicit_set_wall(ex, [p], [n], [np.nan])),
        ("zero normal", lambda: ctx.explicit_set_wall(ex, [p], [[0.0, 0.0]], k)),
        ("kappa 0", lambda: ctx.explicit_set_wall(ex, [p], [n], [0.0])),
        ("kappa < 0", lambda: ctx.explicit_set_wall(ex, [p], [n], [-1.0])),
        ("get without walls", lambda: ctx.explicit_wall_get(ex, 0)),
    ]
    for what, call in bad:
        with pytest.raises(be.FemcyError) as refused:
            call()
        assert refused.value.status == -1, what
    ctx.explicit_set_wall(ex, [p], [n], k)
    for what, call in [("wall 1 of 1", lambda: ctx.explicit_wall_get(ex, 1)), ("wall -1", lambda: ctx.explicit_wall_get(ex, -1)),
                       ("unknown id", lambda: ctx.explicit_wall_get(ex + 1, 0)),
                       ("null out", lambda: ctx._call("femcy_explicit_wall_get", ex, 0, None)),
                       ("a refused call keeps the walls", lambda: ctx.explicit_set_wall(ex, [p], [n], [-1.0]))]:
        with pytest.raises(be.FemcyError) as refused:
            call()
        assert refused.value.status == -1, what
    # the context is usable, and the wall that was set is still there
    ctx.upload(be.VEC_DOF, np.zeros(nodes.size))
    got = ctx.explicit_wall_get(ex, 0)
    assert got[2] == float((np.asarray(nodes)[:, 0] < 0).sum())
    ctx.close()


def comm_refusal(backend):
    """once femcy_comm_init has run (the route of motion_cases.comm_refusal; device only)"""
    nodes, el, ELE = ec.shape_mesh("C3D8-64")
    ctx = lc.make_ctx(nodes, el, ELE, backend)
    held = ctx.dofset(ec.held_dofs(nodes)[1])
    ex = ctx.explicit(ctx.lumped_mass(ELE, RHO), [held])
    ctx.explicit_set_wall(ex, [[0.0, 0.0, 0.0]], [[0.0, 0.0, 1.0]], [1.0])
    ctx.assemble_K(-1)
    iface = np.arange(0, ctx.n, 7, dtype=np.int32)
    ctx.comm_init(0, 1, be.Context.comm_unique_id(), iface, np.arange(iface.size, dtype=np.int32), iface.size,
                  np.ones(ctx.n, dtype=np.uint8))
    for call in (lambda: ctx.explicit_set_wall(ex, [[0.0, 0.0, 0.0]], [[0.0, 0.0, 1.0]], [1.0]), lambda: ctx.explicit_set_wall(ex),
                 lambda: ctx.explicit_wall_get(ex, 0)):
        with pytest.raises(be.FemcyError, match="several ranks") as refused:
            call()
        assert refused.value.status == -1
    ctx.close()


# ------------------------------------------------------------------------------- reader, driver, deck
DECK = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "decks", "explicit", "block_rigid_wall.inp")


def deck_with(tmpdir, wall, dynamic=None, name="wall.inp"):
    """the golden deck with its *Rigid Wall block (and its *Dynamic line) replaced"""
    text = open(DECK).read()
    a = text.index("*Rigid Wall")
    b = text.index("*", a + 1)
    text = text[:a] + wall + text[b:]
    if dynamic is not None:
        a = text.index("*Dynamic")
        b = text.index("*", text.index("\n", a))
        text = text[:a] + dynamic + text[b:]
    path = os.path.join(str(tmpdir), name)
    with open(path, "w") as f:
        f.write(text)
    return path


def reader(tmpdir):
    from femcy_amd.reader import InpInfo
    inp = InpInfo(DECK)
    assert len(inp.rigid_walls) == 1 and inp.rigid_walls[0]["penalty"] is None and inp.energy_output and inp.dynamic_auto
    assert np.array_equal(inp.rigid_walls[0]["normal"], [0.0, 0.0, 1.0])
    two = InpInfo(deck_with(tmpdir, "*Rigid Wall, penalty=2.5e6\n0., 0., -0.01, 0., 0., 1.\n1., 0., 0., -1., 0., 0.5\n"
                                    "*Rigid Wall\n0., 0., 0., 0., 2., 0.\n"))
    assert [w["penalty"] for w in two.rigid_walls] == [2.5e6, 2.5e6, None]
    assert np.array_equal(two.rigid_walls[1]["normal"], [-1.0, 0.0, 0.5])
    row = "0., 0., 0., 0., 0., 1.\n"
    for wall, words in (("*Rigid Wall\n" + row * 5, "at most 4"), ("*Rigid Wall\n0., 0., 0., 1.\n", "6 fields on a 3-D mesh"),
                        ("*Rigid Wall\n0., 0., 0., 0., 0., 0.\n", "must have a length"),
                        ("*Rigid Wall, penalty=0.\n" + row, "must be positive"),
                        ("*Rigid Wall, penalty=-3.\n" + row, "must be positive")):
        with pytest.raises(ValueError, match=words):
            InpInfo(deck_with(tmpdir, wall))
    with pytest.raises(ValueError, match="outside a \\*Dynamic, explicit step"):
        InpInfo(deck_with(tmpdir, "*Rigid Wall\n" + row, dynamic="*Static\n1., 1., 1e-05, 1.\n"))


def solve(path, backend):
    """-> inp, system (closed), the records with that of t = 0 first, v after every batch"""
    from femcy_amd.body import Body
    from femcy_amd.reader import InpInfo
    from femcy_amd.stiffnessMtrx import System_of_equations
    inp = InpInfo(path)
    body = Body(nodes=inp.nodes, elements=list(inp.eSets.values())[0], ELE=inp.ELE)
    system = System_of_equations(body, list(inp.materials.values())[0], inp.geometric_nonlinear, verbose=False,
                                 ctx=be.Context(0, backend=backend))
    V = []

    def recording(advance):
        def call(*a, **kw):
            advance(*a, **kw)
            V.append(system.ctx.download(be.VEC_VEL))
        return call

    system.ctx.explicit_advance = recording(system.ctx.explicit_advance)
    system.ctx.explicit_auto_advance = recording(system.ctx.explicit_auto_advance)
    try:
        system.solve(inp)
    finally:
        system.ctx.close()
    return inp, system, [system.initial_energy] + list(system.increments), V


def deck(backend):
    """the golden deck through the driver: the block rebounds -- its normal momentum changes sign, the wall is free of
    nodes in the last record -- , energy_total with the contact energy stays, and the penetration obeys the energy bound"""
    inp, system, recs, V = solve(DECK, backend)
    assert all(len(r["wall"]) == 1 and "contact_energy" in r for r in recs)
    n = np.array([0.0, 0.0, 1.0])
    m = er.lumped_mass(inp.nodes, list(inp.eSets.values())[0], inp.ELE, inp.density, np.float64)
    mom = [(m[:, None] * v.reshape(-1, 3) @ n).sum() for v in V]
    assert mom[0] < 0 < mom[-1], (mom[0], mom[-1])
    assert max(r["wall"][0]["nodes"] for r in recs) > 0 and recs[-1]["wall"][0]["nodes"] == 0
    assert max(r["contact_energy"] for r in recs) > 0.01 * recs[0]["kinetic"]
    E0 = recs[0]["energy_total"]
    kappa = system.walls[0]["penalty"]
    assert kappa == 0.1 * (system_omega_ref(backend) * system_omega_ref(backend))
    limit = np.sqrt(2.0 * E0 / (kappa * m.min()))
    drift = max(abs(r["energy_total"] - E0) for r in recs) / E0
    pen = max(r["wall"][0]["penetration"] for r in recs)
    print(f"deck [{backend}]: drift of energy_total {drift:.3e}, penetration {pen:.4e} of at most {limit:.4e}")
    assert 0 < pen <= limit and drift < 0.02, (pen, limit, drift)
    return drift


@functools.lru_cache(maxsize=None)
def system_omega_ref(backend):
    """the element bound at u_0 of the golden deck without its wall, as the driver takes it"""
    import tempfile
    return solve(deck_with(tempfile.mkdtemp(), ""), backend)[1].omega_bound


def driver_increment(tmpdir, backend):
    """the fixed path uses omega_c = sqrt(omega_bound^2 + kappa), the default kappa is 0.1 omega_ref^2 on the fixed routes,
    and a deck without the keyword keeps today's records"""
    fixed = "*Dynamic, explicit, scale factor=0.5, output_every=16\n, 2.e-4\n"
    _, plain, recs0, _ = solve(deck_with(tmpdir, "", dynamic=fixed, name="plain.inp"), backend)
    assert all("wall" not in r and "contact_energy" not in r for r in recs0) and plain.walls == []
    _, sysw, recs, _ = solve(deck_with(tmpdir, "*Rigid Wall\n0., 0., -0.01, 0., 0., 1.\n", dynamic=fixed), backend)
    assert sysw.omega_bound == plain.omega_bound and sysw.walls[0]["penalty"] == 0.1 * (plain.omega_bound * plain.omega_bound)
    assert sysw.omega_contact == np.sqrt(plain.omega_bound ** 2 + sysw.wall_kappa)
    assert abs(sysw.stable_dt - 2.0 / sysw.omega_contact) <= 4 * ec.EPS * sysw.stable_dt
    assert abs(sysw.stable_dt / plain.stable_dt - 1.0 / np.sqrt(1.1)) < 1e-12
    _, sysk, _, _ = solve(deck_with(tmpdir, "*Rigid Wall, penalty=3.e8\n0., 0., -0.01, 0., 0., 1.\n", dynamic=fixed), backend)
    assert sysk.omega_contact == np.sqrt(plain.omega_bound ** 2 + 3.0e8)
    direct = "*Dynamic, explicit, direct user control, output_every=16\n2.e-6, 2.e-4\n"
    _, sysd, _, _ = solve(deck_with(tmpdir, "*Rigid Wall\n0., 0., -0.01, 0., 0., 1.\n", dynamic=direct), backend)
    assert sysd.walls[0]["penalty"] == 0.1 * ((2.0 / 2.0e-6) * (2.0 / 2.0e-6))


# ------------------------------------------------------------------- 4: the energy balance through the driver
# energy_total and contact_energy of the float64 restatement against the long-double one, relative to the largest
# energy_total / the largest contact_energy of the run, as measured (measure_f64_worst_driver): 2.83e-14 and 1.60e-12 (the
# contact energy is the square of a depth of 1e-3 of the positions it is the difference of)
F64_WORST_DRIVER = {"energy_total": 2.9e-14, "contact_energy": 1.6e-12}
DRIVER_EVERY = 8


def driver_energy_deck(tmpdir, family):
    """the body of setup() flying into its wall, undamped and unloaded, as a deck with `direct user control`, *Rigid Wall,
    penalty= and *Energy Output -> path, v0"""
    nodes, el, ELE, (point, n, kappa), held, f, v0, h, curve, g = setup(family, False)
    dm = ELE.dm
    v = -0.0005 * np.ptp(nodes, axis=0).max() / h * n                # one velocity for all nodes: what the keyword can say
    initial = "*Initial Conditions, type=VELOCITY\n" + "".join("all, %d, %.17g\n" % (i + 1, v[i]) for i in range(dm))
    wall = "*Rigid Wall, penalty=%.17g\n%s\n" % (kappa, ", ".join("%.17g" % x for x in list(point) + list(n)))
    dynamic = "*Dynamic, explicit, direct user control, output_every=%d\n%.17g, %.17g\n" % (DRIVER_EVERY, h, N * h)
    path = os.path.join(str(tmpdir), "wall_energy_%s.inp" % family)
    ec.write_explicit_deck(path, nodes, el, family, {"all": np.arange(len(nodes))}, wall + "*Energy Output\n", dynamic, initial=initial)
    return path, np.tile(v, len(nodes))


@functools.lru_cache(maxsize=None)
def reference_driver(family):
    """-> per record (state 0, 8, 16, ...) energy_total and contact_energy of the long-double restatement, and the error
    of the float64 restatement in both, relative to the largest of each"""
    import tempfile
    nodes, el, ELE, wall, held, f, v0, h, curve, g = setup(family, False)
    _, v0 = driver_energy_deck(tempfile.mkdtemp(), family)
    f = np.zeros(nodes.size)
    out = {}
    for dt in (LD, np.float64):
        mdl, minv, m, motion = model(family, False, "none", dt)
        U, V, A = mr.verlet_motion(mdl, minv, f, v0, h, N, lambda k: 1.0, motion)
        counts = np.array(mdl.counts)[:, 0]
        total, contact = [], []
        for k in range(0, N + 1, DRIVER_EVERY):
            W, _ = enc.energy_sums(mdl, minv, m, f, U[:k + 1], V[:k + 1], A[:k + 1], [h] * k, [1.0] * (k + 1))
            Ew = mdl.wall_get(0, U[k], m, minv)[1]
            contact.append(Ew)
            total.append(er.kinetic(m, V[k], ELE.dm, dt) + W[1] + W[2] - W[0] - W[3] + Ew)
        out[dt] = (np.array(total, dtype=dt), np.array(contact, dtype=dt))
        if dt is LD:
            assert counts[0] == 0 and counts.max() >= 1 and max(contact) > 0, counts      # a record catches the contact
    (tot, con), (tot64, con64) = out[LD], out[np.float64]
    return tot, con, {"energy_total": float(np.abs(tot64.astype(LD) - tot).max() / np.abs(tot).max()),
                      "contact_energy": float(np.abs(con64.astype(LD) - con).max() / np.abs(con).max())}


def driver_energy(tmpdir, family, backend):
    """energy_total with the contact energy, and contact_energy itself, of every record of an undamped *Energy Output run
    through the driver against the long-double restatement: within 4 x the float64 restatement's own error"""
    tot, con, _ = reference_driver(family)
    path, _ = driver_energy_deck(tmpdir, family)
    inp, system, recs, _ = solve(path, backend)
    assert inp.energy_output and len(recs) == len(tot) and system.walls[0]["penalty"] == setup(family, False)[3][2]
    worst = {}
    for key, ref in (("energy_total", tot), ("contact_energy", con)):
        got = np.array([r[key] for r in recs])
        worst[key] = float(np.abs(got.astype(LD) - ref).max() / np.abs(ref).max())
        print(f"driver {family} [{backend}]: {key} {worst[key]:.3e} of at most {4.0 * F64_WORST_DRIVER[key]:.3e}")
    for key in worst:
        assert worst[key] <= 4.0 * F64_WORST_DRIVER[key], (key, worst[key])
    assert all(r["contact_energy"] == sum(w["energy"] for w in r["wall"]) for r in recs)
    return worst


def measure_f64_worst_driver():
    return {key: max(reference_driver(fam)[2][key] for fam in FAMILIES) for key in F64_WORST_DRIVER}


def measure_f64_worst():
    """F64_WORST, as measured"""
    out = {}
    for mode in ("fixed", "auto"):
        out[mode] = max(reference(mode, moved, fam, d)[2] for moved in (False, True) for fam in FAMILIES for d in DAMPINGS)
    return out
