"""Prescribed motion in explicit dynamics (femcy_amplitude_create, femcy_explicit_set_motion, *Amplitude, *Boundary amplitude=)
written against the C ABI (femcy_amd.backend.Context), the deck reader and the deck driver, so that the host backend
(tests/test_motion_cpu.py) and the device (tests/test_gpu_motion.py) run the same code.  Every function checks its own result
and returns the figure it checked.

Bounds.  The reference is the restatement of tests/motion_reference.py in np.longdouble.  The same restatement in float64
differs from it by rounding and summation order alone; the F64_WORST_* constants are the worst such differences on the very
cases run here (`measure_f64_worst`, asserted by tests/test_motion_cpu.py), and a backend is held to 4 x that.  Errors are
relative to the largest entry of the reference.

Shapes.  The node pass gives 32 lanes to a node and 8 nodes to a workgroup of 256, and nothing else in it is new: the meshes
have 7, 8, 9 and 15, 16, 17 nodes (one and two workgroups, the last one short, full, and one node over), in CPS4 (dm = 2) and
C3D4 (dm = 3).  Moved: node 0 and the last node with every component, the last node of workgroup 0 (node 7) with its first
component alone, the first node of workgroup 1 (node 8), and node 0's first component a second time, in a later set with
another value and curve, which must win.  Node 3 is held and not moved.  Two curves in one integrator."""
import functools
import os

import numpy as np
import pytest

from femcy_amd import backend as be
from femcy_amd.element_zoo import Element_linear_quadrilateral, Element_linear_tetrahedral

import dynamic_cases as dc
import explicit_auto_cases as eac
import explicit_cases as ec
import explicit_damped_cases as edc
import explicit_damped_reference as edr
import explicit_reference as er
import loads_cases as lc
import loads_reference as lr
import motion_reference as mr

LD = np.longdouble
RHO = ec.RHO
H = 2.0 ** -17                  # every k H is exact in both dtypes: a breakpoint can fall exactly on a step time
STEPS, PARTS = 32, (5, 11, 16)
NODE_COUNTS = (7, 8, 9, 15, 16, 17)
FAMILIES = ("CPS4", "C3D4")
MESHES = [(fam, nn) for fam in FAMILIES for nn in NODE_COUNTS]
DAMPING = (edc.ALPHA, edc.B1, edc.B2)
AUTO_SF, AUTO_STEPS, AUTO_BATCHES = 0.9, 30, (7, 13, 40)
# worst error of the float64 restatement against the long-double one (measure_f64_worst, as measured) over MESHES: u, v, a at
# every batch end of the fixed runs 1.80e-14 (smooth step, C3D4-16), 9.53e-14 (tabular, C3D4-9: a kink in the boundary's
# velocity excites the stiffest modes), 1.75e-14 (damped); the automatic run (u, v, a, the increments and the clock) 2.63e-13
# (CPS4-8); amplitude() itself 2.66e-15 (a relative 1e-9 beside a point, where t - t_k cancels)
F64_WORST_FIXED = {"smooth": 1.85e-14, "tabular": 9.6e-14, "damped": 1.8e-14}
F64_WORST_START = 2.5e-13       # a_0: the forces of a displacement of 1e-3 of the mesh size, which lose three digits
F64_WORST_AUTO = 2.7e-13
F64_WORST_AMP = 2.7e-15


def relerr(got, want):
    return float(np.abs(np.asarray(got, dtype=LD) - want).max() / np.abs(want).max())


def same_bits(x, y):
    return np.array_equal(np.asarray(x).view(np.uint64), np.asarray(y).view(np.uint64))


# -------------------------------------------------------------------------------------------- meshes
def ring_quads(m):
    """m CPS4 round node 0: 2 m + 1 nodes"""
    t = 2 * np.pi * np.arange(2 * m) / (2 * m)
    r = 1.0 + 0.15 * np.cos(3 * t + 0.4)
    nodes = np.vstack([[0.05, -0.03], np.column_stack([r * np.cos(t), 0.8 * r * np.sin(t)])])
    el = np.array([[0, 1 + 2 * i, 2 + 2 * i, 1 + (2 * i + 2) % (2 * m)] for i in range(m)], np.int32)
    return nodes, el


def tet_chain(nn):
    """nn - 3 C3D4 in a chain: every new node is the apex of a tetrahedron over the free face of the one before"""
    X = [np.array(p) for p in lr.single("C3D4")[0]]
    el = [[0, 1, 2, 3]]
    rng = np.random.default_rng(5)
    while len(X) < nn:
        base, face = el[-1][0], el[-1][1:]
        c = sum(X[k] for k in face) / 3.0
        X.append(c + 0.9 * (c - X[base]) + 0.05 * rng.uniform(-1.0, 1.0, 3))
        tet = face + [len(X) - 1]
        if np.linalg.det(np.array([X[k] - X[tet[0]] for k in tet[1:]]).T) < 0:
            tet[0], tet[1] = tet[1], tet[0]
        el.append(tet)
    return np.array(X), np.array(el, np.int32)


@functools.lru_cache(maxsize=None)
def mesh(family, nn):
    if family == "C3D4":
        nodes, el = tet_chain(nn)
        ELE = Element_linear_tetrahedral()
    else:
        ELE = Element_linear_quadrilateral()
        if nn % 2:
            nodes, el = ring_quads(nn // 2)
        else:
            nodes, el, _ = lr.mesh("CPS4", cells={8: (3, 1), 16: (3, 3)}[nn], perturb=0.2)
    assert len(nodes) == nn and (lr.mesh_volume(nodes, el, ELE) > 0)
    nodes.setflags(write=False)
    return nodes, el, ELE


def curves(kind, T):
    """two curves in step time over [0, T]: the first starts at 0 and has its last point before T (the moved DOFs end at
    rest, exactly); the second starts late, from a value that is not 0 (the placed boundary shows in f_int(u_0)), and is cut
    off by T.  tabular: the breakpoints 8 H, 16 H and 20 H fall exactly on step times of the fixed runs"""
    if kind == mr.TABULAR:
        return (kind, [0.0, T / 4, T / 2, 7 * T / 8], [0.0, 1.0, 0.5, 0.75]), (kind, [2.5 * T / 32, 5 * T / 8, 2 * T], [0.2, -1.0, 0.0])
    return (kind, [0.0, 3 * T / 8, 3 * T / 4], [0.0, 1.0, 0.4]), (kind, [T / 8, 5 * T / 4], [0.2, -1.0])


def sets_of(nn, dm):
    """-> the held DOF sets [A, B1, (B2,) C, D] and the motion call (positions in that list, value factors, curve 0 / 1):
    A: node 0 and the last node, every component.  B1: the last node of workgroup 0 (node 7, or the last but one node of a
    smaller mesh), first component alone.  B2: the first node of workgroup 1 (node 8) where it is not the last node.  C: node 3,
    held and not moved.  D: node 0's first component again, later than A"""
    comps = np.arange(dm)
    edge = [k for k in (7, 8) if k <= nn - 2] or [nn - 2]
    sets = [np.concatenate([0 * dm + comps, (nn - 1) * dm + comps]), np.array([edge[0] * dm])]
    if len(edge) > 1:
        sets.append(edge[1] * dm + comps)
    sets += [3 * dm + comps, np.array([0])]
    moved = [k for k in range(len(sets)) if k != len(sets) - 2]
    values = [1.0, -0.7, 0.6][:len(moved) - 1] + [-0.5]
    which = [0] + [1] * (len(moved) - 1)
    return sets, moved, values, which


def setup(family, nn):
    """-> nodes, el, ELE, held sets, (moved positions, values, curve numbers), f, v0"""
    nodes, el, ELE = mesh(family, nn)
    sets, moved, factors, which = sets_of(nn, ELE.dm)
    rng = np.random.default_rng(nn)
    g = 0.004 * np.ptp(nodes, axis=0).max()
    fixed = np.unique(np.concatenate(sets))
    v0, f = 2.0 * rng.uniform(-1.0, 1.0, nodes.size), 50.0 * rng.uniform(-1.0, 1.0, nodes.size)
    v0[fixed] = 0.0
    return nodes, el, ELE, sets, (moved, [g * x for x in factors], which), f, v0


def make(family, nn, backend, kind, T, damping=None, zero=False, motion=True):
    """a context with the integrator of setup(); motion: set, with the values of setup() or (zero) all 0"""
    nodes, el, ELE, sets, (moved, values, which), f, v0 = setup(family, nn)
    ctx = lc.make_ctx(nodes, el, ELE, backend)
    lm = ctx.lumped_mass(ELE, RHO)
    ids = [ctx.dofset(s) for s in sets]
    ex = ctx.explicit(lm, ids)
    if motion:
        amps = [ctx.amplitude("tabular" if k == mr.TABULAR else "smooth step", t, A) for k, t, A in curves(kind, T)]
        ctx.explicit_set_motion(ex, [ids[k] for k in moved], [0.0 * v if zero else v for v in values], [amps[w] for w in which])
    if damping is not None:
        ctx.explicit_set_damping(ex, damping[0], damping[1], damping[2], edc.modulus(ec.material_of(ELE)))
    ctx.upload(be.VEC_VEL, v0)
    ctx.upload(be.VEC_RHS, f)
    ctx.upload(be.VEC_ACC, np.full(nodes.size, np.nan))                # not read at the start
    return ctx, ex, lm, ids


def state(ctx):
    return [ctx.download(v) for v in (be.VEC_DOF, be.VEC_VEL, be.VEC_ACC)]


def model(family, nn, dtype, kind, T, damping=None):
    """-> the restatement's model, minv, the lumped mass, the Motion and f, v0"""
    nodes, el, ELE, sets, (moved, values, which), f, v0 = setup(family, nn)
    mat = ec.material_of(ELE)
    coeffs = damping or (0.0, 0.0, 0.0)
    mdl = edr.DampedModel(nodes, el, ELE, mat, dtype, RHO, coeffs[0], coeffs[1], coeffs[2], edc.modulus(mat))
    m = er.lumped_mass(nodes, el, ELE, RHO, dtype)
    minv = 1 / np.repeat(m, ELE.dm)
    minv[np.unique(np.concatenate(sets))] = 0
    cs = curves(kind, T)
    motion = mr.Motion([(sets[k], v, cs[w]) for k, v, w in zip(moved, values, which)], dtype)
    return mdl, minv, m, motion, f, v0


# --------------------------------------------------------------------------------------- fixed runs
FIXED = {"smooth": (mr.SMOOTH_STEP, None), "tabular": (mr.TABULAR, None), "damped": (mr.SMOOTH_STEP, DAMPING)}
RAMP = dict(s0=0.25, ds=1.0 / 64.0)      # the load scale of state k is s0 + k ds


@functools.lru_cache(maxsize=None)
def reference_fixed(case, family, nn):
    """-> U, V, A [STEPS + 1, n] in long double, the kinetic energy at the end, the error of the float64 restatement at the
    batch ends"""
    kind, damping = FIXED[case]
    out = {}
    for dt in (LD, np.float64):
        mdl, minv, m, motion, f, v0 = model(family, nn, dt, kind, STEPS * H, damping)
        out[dt] = mr.verlet_motion(mdl, minv, f, v0, H, STEPS, lambda k: RAMP["s0"] + k * RAMP["ds"], motion)
        if dt is LD:
            ke = er.kinetic(m, out[dt][1][-1], mdl.dm, dt)
    for x in out[LD]:
        x.setflags(write=False)
    e64 = max(relerr(x64[k], x[k]) for x64, x in zip(out[np.float64], out[LD]) for k in np.cumsum(PARTS))
    start64 = max(relerr(x64[0], x[0]) for x64, x in zip(out[np.float64], out[LD]))
    return out[LD], ke, e64, start64


def run_fixed(ctx, ex, parts=PARTS, h=H):
    """-> the states after every call"""
    ctx.explicit_start(ex, be.VEC_RHS, RAMP["s0"])
    done, out = 0, []
    for k in parts:
        ctx.explicit_advance(ex, k, h, be.VEC_RHS, RAMP["s0"] + done * RAMP["ds"], RAMP["ds"])
        done += k
        out.append(state(ctx))
    return out


def fixed(case, family, nn, backend):
    """STEPS steps in three calls: u, v, a after every call against long double, the kinetic energy at the end, and what is
    exact: the DOFs of the first curve, whose last point lies before T, end at value x A_last bit for bit with v = a = 0,
    the held set that is not moved stays at 0, and the placed boundary was seen by the start (a_0 of the reference)"""
    kind, damping = FIXED[case]
    (U, V, A), ke_ref, _, _ = reference_fixed(case, family, nn)
    nodes, el, ELE, sets, (moved, values, which), f, v0 = setup(family, nn)
    ctx, ex, lm, ids = make(family, nn, backend, kind, STEPS * H, damping)
    ctx.explicit_start(ex, be.VEC_RHS, RAMP["s0"])
    e0 = max(relerr(g, w[0]) for g, w in zip(state(ctx), (U, V, A)))
    assert np.abs(U[0]).max() > 0 and np.abs(A[0]).max() > 0           # the second curve starts from a value that is not 0
    assert e0 <= 4.0 * F64_WORST_START, e0                             # a_0 = -minv f_int(u_0) of the placed boundary
    err = 0.0
    got = run_fixed(ctx, ex)
    ke = ctx.explicit_kinetic_energy(ex, be.VEC_VEL)
    ctx.close()
    for k, st in zip(np.cumsum(PARTS), got):
        err = max([err] + [relerr(g, w[k]) for g, w in zip(st, (U, V, A))])
    ek = float(abs(ke - ke_ref) / ke_ref)
    print(f"{case} {family}-{nn} [{backend}]: u, v, a at the batch ends {err:.3e}, kinetic energy {ek:.3e}")
    tol = 4.0 * F64_WORST_FIXED[case]
    assert err <= tol, err
    assert ek <= 2 * tol + (nn + 4) * ec.EPS, ek                       # v enters squared; the sum as in ec.one_step
    u, v, a = got[-1]
    first = sets[0][1:]                                                 # set A without node 0's first component (set D's)
    last_A = np.float64(curves(kind, STEPS * H)[0][2][-1])
    assert same_bits(u[first], np.full(first.size, np.float64(values[0]) * last_A))
    assert not v[first].any() and not a[first].any()
    held = sets[-2]
    assert not u[held].any() and not v[held].any() and not a[held].any()
    assert np.abs(v[sets[-1]]).max() > 0                               # the second curve is still moving at T
    return err


def split(case, family, nn, backend):
    """one call of STEPS steps against PARTS, bit for bit: the time of a step does not depend on the call that reaches it"""
    kind, damping = FIXED[case]
    runs = []
    for parts in ((STEPS,), PARTS, (1, STEPS - 1)):
        ctx, ex, _, _ = make(family, nn, backend, kind, STEPS * H, damping)
        runs.append(run_fixed(ctx, ex, parts)[-1])
        ctx.close()
    for other in runs[1:]:
        assert all(same_bits(x, y) for x, y in zip(runs[0], other))


def new_increment(family, nn, backend):
    """a call with another dt counts on from the time the clock has reached: 8 steps of H and 12 of H / 2 end at 14 H, where
    the restatement puts the moved DOFs"""
    ctx, ex, _, _ = make(family, nn, backend, mr.SMOOTH_STEP, STEPS * H)
    ctx.explicit_start(ex, be.VEC_RHS, 1.0)
    ctx.explicit_advance(ex, 8, H, be.VEC_RHS, 1.0, 0.0)
    ctx.explicit_advance(ex, 12, H / 2, be.VEC_RHS, 1.0, 0.0)
    got = state(ctx)
    ctx.close()
    motion = model(family, nn, LD, mr.SMOOTH_STEP, STEPS * H)[3]
    err = max(relerr(g[motion.dofs], w) for g, w in zip(got, motion.at(LD(14) * LD(H))))
    assert err <= 4.0 * F64_WORST_AMP, err
    return err


def zero_values(mode, family, nn, backend):
    """a motion whose values are all 0 against no motion at all: the lanes of the policy kernel that are not moved give the
    bits of today's kernel.  On the moved DOFs themselves both runs hold zeros, compared as numbers: today's kernel leaves
    0 x (s f - f_int) there and the policy 0 x A'', either of which may carry a sign"""
    nodes, el, ELE, sets, (moved, _, _), f, v0 = setup(family, nn)
    md = np.unique(np.concatenate([sets[k] for k in moved]))
    others = np.setdiff1d(np.arange(nodes.size), md)
    runs = []
    for zero in (False, True):
        ctx, ex, _, _ = make(family, nn, backend, mr.SMOOTH_STEP, STEPS * H, DAMPING, zero=zero, motion=zero)
        runs.append(run_fixed(ctx, ex)[-1] if mode == "fixed" else run_auto(ctx, ex, ELE, auto_T(family, nn))[0])
        ctx.close()
    for x, y in zip(*runs):
        assert same_bits(x[others], y[others]) and not x[md].any() and not y[md].any()
    assert np.abs(runs[0][1]).max() > 0


def removed(mode, family, nn, backend):
    """set_motion(nsets = 0) after a motion: the bits of an integrator that never had one, moved DOFs included"""
    ELE = mesh(family, nn)[2]
    runs = []
    for motion in (False, True):
        ctx, ex, _, _ = make(family, nn, backend, mr.SMOOTH_STEP, STEPS * H, DAMPING, motion=motion)
        if motion:
            ctx.explicit_set_motion(ex)
        runs.append(run_fixed(ctx, ex)[-1] if mode == "fixed" else run_auto(ctx, ex, ELE, auto_T(family, nn))[0])
        ctx.close()
    assert all(same_bits(x, y) for x, y in zip(*runs))


# ----------------------------------------------------------------------------------- automatic runs
@functools.lru_cache(maxsize=None)
def auto_T(family, nn):
    """about AUTO_STEPS increments of the estimate at rest"""
    nodes, el, ELE = mesh(family, nn)
    om = eac.Estimate(nodes, el, ELE, ec.material_of(ELE), RHO, LD).omega(np.zeros(nodes.size))
    return float(AUTO_STEPS * AUTO_SF * 2 / om)


def run_auto(ctx, ex, ELE, T, batches=AUTO_BATCHES, ramp=True):
    """-> the state and the clock after the last batch, and both after every batch"""
    ctx.explicit_auto_begin(ex, float(eac.s_C(ec.material_of(ELE))), AUTO_SF, T, ramp, be.VEC_RHS)
    out = []
    for k in batches:
        ctx.explicit_auto_advance(ex, k, be.VEC_RHS)
        out.append((state(ctx), ctx.explicit_auto_state(ex)))
    return out[-1][0], out[-1][1], out


@functools.lru_cache(maxsize=None)
def reference_auto(family, nn):
    nodes, el, ELE = mesh(family, nn)
    T = auto_T(family, nn)
    out = {}
    for dt in (LD, np.float64):
        mdl, minv, m, motion, f, v0 = model(family, nn, dt, mr.SMOOTH_STEP, T, DAMPING)
        est = eac.Estimate(nodes, el, ELE, ec.material_of(ELE), RHO, dt)
        out[dt] = mr.verlet_auto_motion(mdl, est, minv, f, v0, AUTO_SF, T, True, motion)
    Hs, times, U, V, A = out[LD]
    H64, t64, U64, V64, A64 = out[np.float64]
    assert len(H64) == len(Hs) and 20 <= len(Hs) <= 60, len(Hs)
    ends = [k for k in np.cumsum(AUTO_BATCHES) if k < len(Hs)] + [len(Hs)]
    e64 = max([relerr(x64[k], x[k]) for x64, x in ((U64, U), (V64, V), (A64, A)) for k in ends] + [relerr(H64, Hs), relerr(t64, times)])
    return out[LD], ends, e64


def auto(family, nn, backend):
    """`element by element` with motion and damping: the clock path.  u, v, a and the clock after every batch against long
    double -- the last batch overshoots T --, the first curve's DOFs at rest at value x A_last exactly, and the state bit
    for bit unchanged by a further batch of no-op steps"""
    nodes, el, ELE, sets, (moved, values, which), f, v0 = setup(family, nn)
    (Hs, times, U, V, A), ends, _ = reference_auto(family, nn)
    T = auto_T(family, nn)
    ctx, ex, _, _ = make(family, nn, backend, mr.SMOOTH_STEP, T, DAMPING)
    last, clock, batches = run_auto(ctx, ex, ELE, T)
    ctx.explicit_auto_advance(ex, 5, be.VEC_RHS)
    again, clock2 = state(ctx), ctx.explicit_auto_state(ex)
    ctx.close()
    assert clock[0] == T and clock[3] == len(Hs) < sum(AUTO_BATCHES), clock      # t == T, and the batch overshot it
    assert clock2 == clock and all(same_bits(x, y) for x, y in zip(last, again))
    err = 0.0
    for k, (st, clk) in zip(ends, batches):
        assert clk[3] == k, (clk, k)
        err = max([err, float(abs(LD(clk[0]) - times[k]) / times[-1]), float(abs(LD(clk[1]) - Hs[k - 1]) / Hs.max())]
                  + [relerr(g, w[k]) for g, w in zip(st, (U, V, A))])
    print(f"auto {family}-{nn} [{backend}]: {len(Hs)} steps, u, v, a and the clock at the batch ends {err:.3e}")
    assert err <= 4.0 * F64_WORST_AUTO, err
    u, v, a = last
    first = sets[0][1:]
    last_A = np.float64(curves(mr.SMOOTH_STEP, T)[0][2][-1])
    assert same_bits(u[first], np.full(first.size, np.float64(values[0]) * last_A))
    assert not v[first].any() and not a[first].any()
    return err


def auto_split(family, nn, backend):
    """one batch against AUTO_BATCHES, bit for bit"""
    ELE = mesh(family, nn)[2]
    T = auto_T(family, nn)
    runs = []
    for batches in ((sum(AUTO_BATCHES),), AUTO_BATCHES):
        ctx, ex, _, _ = make(family, nn, backend, mr.SMOOTH_STEP, T, DAMPING)
        st, clk, _ = run_auto(ctx, ex, ELE, T, batches)
        runs.append(st + [np.array(clk)])
        ctx.close()
    assert all(same_bits(x, y) for x, y in zip(*runs))


# ------------------------------------------------------------------------------------- amplitude()
AMP_T = [0.5, 1.0, 2.5, 3.0, 4.25, 7.0]
AMP_A = [0.25, -1.0, 1.5, 1.5, -2.0, 0.75]
AMP_G = 2.0 ** -10              # the value of the moved DOF: a power of two scales exactly, and the element stays an element


def amp_times():
    """at, one ulp to either side of and a little away from every point; inside every interval; outside the table"""
    ts = [0.25, 9.0]
    for k, t in enumerate(AMP_T):
        ts += [t, np.nextafter(t, 0.0), np.nextafter(t, 10.0), t * (1 - 1e-9), t * (1 + 1e-9)]
        if k:
            ts += [AMP_T[k - 1] + x * (t - AMP_T[k - 1]) for x in (0.25, 0.5, 0.8125)]
    return sorted(float(t) for t in ts)


@functools.lru_cache(maxsize=None)
def reference_amp(kind):
    ref = np.array([mr.amplitude(kind, AMP_T, AMP_A, t, LD) for t in amp_times()], dtype=LD)
    f64 = np.array([mr.amplitude(kind, AMP_T, AMP_A, t, np.float64) for t in amp_times()], dtype=np.float64)
    return ref, max(relerr(f64[:, k], ref[:, k]) for k in range(3) if np.abs(ref[:, k]).max() > 0)


def amplitude_values(kind, backend):
    """amplitude() through the library: one element with every DOF held and one moved with the value 1; start + one step of
    dt = t leave A(t), A'(t), A''(t) in u, v, a of that DOF.  At every point A_k exactly, and for the smooth step A' = A'' = 0
    exactly; beyond the last point (A_last, 0, 0) exactly"""
    nodes, el, ELE, _ = lr.single("CPS3")
    ctx = lc.make_ctx(nodes, el, ELE, backend)
    every, one = ctx.dofset(np.arange(nodes.size)), ctx.dofset(np.array([3]))
    ex = ctx.explicit(ctx.lumped_mass(ELE, RHO), [every, one])
    ctx.explicit_set_motion(ex, [one], [AMP_G], [ctx.amplitude("tabular" if kind == mr.TABULAR else "smooth step", AMP_T, AMP_A)])
    got = []
    for t in amp_times():
        ctx.explicit_start(ex, be.VEC_RHS, 0.0)
        ctx.explicit_advance(ex, 1, t, be.VEC_RHS, 0.0, 0.0)
        got.append([x[3] for x in state(ctx)])
    ctx.close()
    got = np.array(got) / AMP_G
    ref, _ = reference_amp(kind)
    err = max(relerr(got[:, k], ref[:, k]) for k in range(3) if np.abs(ref[:, k]).max() > 0)
    print(f"amplitude kind {kind} [{backend}]: {len(got)} times, {err:.3e}")
    assert err <= 4.0 * F64_WORST_AMP, err
    for t, (A, dA, ddA) in zip(amp_times(), got):
        if t in AMP_T:
            k = AMP_T.index(t)
            assert A == AMP_A[k], (t, A)
            if kind == mr.SMOOTH_STEP or k in (0, len(AMP_T) - 1):      # t <= t_0 and t >= t_last are clamped
                assert dA == 0.0 and ddA == 0.0, (t, dA, ddA)
            else:                                                       # the right-hand slope, in float64's own rounding
                assert dA == (AMP_A[k + 1] - AMP_A[k]) / (AMP_T[k + 1] - AMP_T[k]), (t, dA)
        if t <= AMP_T[0] or t >= AMP_T[-1]:
            assert (A, dA, ddA) == (AMP_A[0] if t <= AMP_T[0] else AMP_A[-1], 0.0, 0.0), (t, A, dA, ddA)
        if kind == mr.TABULAR:
            assert ddA == 0.0
    return err


# ----------------------------------------------------------------------------------------- refusals
def refusals(backend):
    """every refusal of the two entries returns FEMCY_EINVAL with a message, and the context keeps working"""
    import ctypes as C
    family, nn = "C3D4", 9
    ctx, ex, lm, ids = make(family, nn, backend, mr.SMOOTH_STEP, STEPS * H, motion=False)
    free = ctx.dofset(np.array([4]))                                    # a DOF set the integrator does not hold
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    out = C.c_int32()
    good_t, good_A = np.array([0.0, 1.0, 2.0]), np.array([0.0, 1.0, 0.5])
    create = lambda kind, n, t, A, o=out: ctx._call("femcy_amplitude_create", kind, n, None if t is None else ptr(t),
                                                     None if A is None else ptr(A), None if o is None else C.byref(o))
    long_t = np.arange(17.0)
    calls = [(lambda: create(2, 3, good_t, good_A), "unknown kind"), (lambda: create(-1, 3, good_t, good_A), "unknown kind"),
             (lambda: create(0, 1, good_t, good_A), "points"), (lambda: create(1, 17, long_t, long_t), "points"),
             (lambda: create(0, 3, None, good_A), "null"), (lambda: create(0, 3, good_t, None), "null"),
             (lambda: create(0, 3, good_t, good_A, None), "null"),
             (lambda: create(0, 3, np.array([0.0, 1.0, 1.0]), good_A), "strictly increasing"),
             (lambda: create(1, 3, np.array([0.0, 2.0, 1.0]), good_A), "strictly increasing")]
    for bad in (np.nan, np.inf, -np.inf):
        calls += [(lambda bad=bad: create(0, 3, np.array([0.0, bad, 2.0]), good_A), "not finite"),
                  (lambda bad=bad: create(1, 3, good_t, np.array([0.0, 1.0, bad])), "not finite")]
    amp = ctx.amplitude("smooth step", good_t, good_A)
    more = [ctx.amplitude("tabular", good_t + k, good_A) for k in range(1, 5)]
    calls += [(lambda: ctx.explicit_set_motion(ex + 1, [ids[0]], [1.0], [amp]), "unknown explicit integrator"),
              (lambda: ctx.explicit_set_motion(-1, [ids[0]], [1.0], [amp]), "unknown explicit integrator"),
              (lambda: ctx.explicit_set_motion(ex, [99], [1.0], [amp]), "unknown DOF set"),
              (lambda: ctx.explicit_set_motion(ex, [ids[0]], [1.0], [more[-1] + 1]), "unknown amplitude"),
              (lambda: ctx.explicit_set_motion(ex, [ids[0]], [1.0], [-1]), "unknown amplitude"),
              (lambda: ctx.explicit_set_motion(ex, [ids[0], free], [1.0, 1.0], [amp, amp]), "holds"),
              (lambda: ctx.explicit_set_motion(ex, [ids[0]] * 5, [1.0] * 5, [amp] + more), "distinct amplitudes"),
              (lambda: ctx._call("femcy_explicit_set_motion", ex, 1, None, None, None), "null")]
    calls += [(lambda bad=bad: ctx.explicit_set_motion(ex, [ids[0]], [bad], [amp]), "not finite") for bad in (np.nan, np.inf)]
    for call, message in calls:
        with pytest.raises(be.FemcyError, match=message) as refused:
            call()
        assert refused.value.status == -1, message                     # FEMCY_EINVAL
    # nothing was set by a refused call, and the context still works: four curves are taken, and the motion shows
    before = run_fixed(ctx, ex, (4,))[-1]
    ctx.explicit_set_motion(ex, [ids[0]] * 4, [1.0] * 4, more[:3] + [amp])      # the last one wins: it moves from t = 0
    ctx.upload(be.VEC_DOF, np.zeros(ctx.n))
    after = run_fixed(ctx, ex, (4,))[-1]
    assert not before[0][np.asarray(setup(family, nn)[3][0])].any() and after[0][0] != 0.0
    ctx.set_mesh(*mesh(family, nn)[:2])                                 # a new mesh drops the amplitudes with the integrators
    with pytest.raises(be.FemcyError, match="unknown explicit integrator"):
        ctx.explicit_set_motion(ex, [], [], [])
    ctx.close()


def comm_refusal(backend):
    """once femcy_comm_init has run (the route of explicit_cases.comm_refusal; device only)"""
    nodes, el, ELE = ec.shape_mesh("C3D8-64")
    ctx = lc.make_ctx(nodes, el, ELE, backend)
    held = ctx.dofset(ec.held_dofs(nodes)[1])
    ex = ctx.explicit(ctx.lumped_mass(ELE, RHO), [held])
    amp = ctx.amplitude("tabular", [0.0, 1.0], [0.0, 1.0])
    ctx.assemble_K(-1)
    iface = np.arange(0, ctx.n, 7, dtype=np.int32)
    ctx.comm_init(0, 1, be.Context.comm_unique_id(), iface, np.arange(iface.size, dtype=np.int32), iface.size,
                  np.ones(ctx.n, dtype=np.uint8))
    for call in (lambda: ctx.amplitude("tabular", [0.0, 1.0], [0.0, 1.0]), lambda: ctx.explicit_set_motion(ex, [held], [1.0], [amp]),
                 lambda: ctx.explicit_set_motion(ex)):
        with pytest.raises(be.FemcyError, match="several ranks") as refused:
            call()
        assert refused.value.status == -1
    ctx.close()


# ------------------------------------------------------------------------------------- reader, deck
PULL = 0.02


def write_pull_deck(path, boundary=None, amplitude=None, dynamic=None, steps=64):
    """the clamped C3D4 column of dynamic_cases, its top face pulled along z by a smooth step that ends at 3/4 of T"""
    nodes, el = dc.bar_mesh()
    T = steps * 1.0e-5
    top = nodes[:, 2].max()
    nsets = {"foot": np.nonzero(nodes[:, 2] < 1e-12)[0], "top": np.nonzero(nodes[:, 2] > top - 1e-12)[0]}
    if amplitude is None:
        amplitude = "*Amplitude, name=PULL, definition=SMOOTH STEP\n0., 0., %r, 1.\n" % (0.75 * T)
    if boundary is None:
        boundary = "*Boundary, amplitude=PULL\ntop, 3, 3, %r\n" % PULL
    if dynamic is None:
        dynamic = "*Dynamic, explicit, direct user control, output_every=16\n%r, %r\n" % (1.0e-5, T)
    ec.write_explicit_deck(path, nodes, el, "C3D4", nsets, "*Boundary\nfoot, 1, 1\nfoot, 2, 2\nfoot, 3, 3\n" + boundary, dynamic,
                           initial=amplitude)
    return nodes, nsets, T


def reader(tmpdir):
    """*Amplitude and *Boundary, amplitude= as read, and every refusal"""
    from femcy_amd.reader import InpInfo
    path = os.path.join(str(tmpdir), "pull.inp")
    nodes, nsets, T = write_pull_deck(path)
    inp = InpInfo(path)
    assert list(inp.amplitudes) == ["PULL"] and inp.amplitudes["PULL"]["definition"] == "SMOOTH STEP"
    assert np.array_equal(inp.amplitudes["PULL"]["t"], [0.0, 0.75 * T]) and np.array_equal(inp.amplitudes["PULL"]["A"], [0.0, 1.0])
    assert [bc.get("amplitude") for bc in inp.dirichlet_bc_info] == [None, None, None, "PULL"]
    assert all("amplitude" not in bc for bc in inp.dirichlet_bc_info[:3])      # the key is absent, not None
    assert inp.dirichlet_bc_info[3]["val"] == PULL and not inp.dirichlet_bc_info[3]["user"]
    # pairs over several lines, up to four a line; TABULAR is the default and the definition's case and spacing do not matter
    many = "*Amplitude, name=A1\n0., 0., 1., 2., 2., -1., 3., 0.5\n4., 1.,\n5., 0.\n*Amplitude, name=PULL, definition=smooth  step\n0., 0., 1., 1.\n"
    write_pull_deck(path, amplitude=many)
    inp = InpInfo(path)
    assert inp.amplitudes["A1"]["definition"] == "TABULAR" and inp.amplitudes["PULL"]["definition"] == "SMOOTH STEP"
    assert np.array_equal(inp.amplitudes["A1"]["t"], np.arange(6.0)) and np.array_equal(inp.amplitudes["A1"]["A"], [0, 2, -1, 0.5, 1, 0])
    pairs = lambda n: "".join("%d., 1.,\n" % k for k in range(n))
    write_pull_deck(path, amplitude="*Amplitude, name=PULL\n" + pairs(16))
    assert InpInfo(path).amplitudes["PULL"]["t"].size == 16
    static = "*Static\n1., 1., 1e-05, 1.\n"
    implicit = "*Dynamic, direct\n1e-4, 1e-3\n"
    one = "*Amplitude, name=PULL\n0., 0., 1., 1.\n"
    for kwargs, word in ((dict(boundary="*Boundary, amplitude=OTHER\ntop, 3, 3, 0.01\n"), "no \\*Amplitude of that name"),
                         (dict(amplitude=one + one), "twice"),
                         (dict(amplitude="*Amplitude, name=PULL, definition=PERIODIC\n0., 0., 1., 1.\n"), "PERIODIC"),
                         (dict(amplitude="*Amplitude, name=PULL, definition=EQUALLY SPACED\n0., 0., 1., 1.\n"), "EQUALLY SPACED"),
                         (dict(amplitude="*Amplitude, name=PULL\n0., 0.\n"), "1 points"),
                         (dict(amplitude="*Amplitude, name=PULL\n" + pairs(17)), "17 points"),
                         (dict(amplitude="*Amplitude, name=PULL\n0., 0., 1., 1., 1., 2.\n"), "increasing"),
                         (dict(amplitude="*Amplitude, name=PULL\n0., 0., 2., 1., 1., 2.\n"), "increasing"),
                         (dict(boundary="*Boundary, user, amplitude=PULL\ntop, 3, 3, 0.01\n"), "user"),
                         (dict(dynamic=static), "Static"),
                         (dict(dynamic=implicit), "Dynamic, direct"),
                         (dict(boundary="*Boundary\ntop, 3, 3, 0.01\n"), "non-zero \\*Boundary value"),
                         (dict(boundary="*Boundary\ntop, 3, 3, 0.01\n", dynamic=implicit), "non-zero \\*Boundary value")):
        write_pull_deck(path, **kwargs)
        with pytest.raises(ValueError, match=word):
            InpInfo(path)


def pulled_bar(tmpdir, backend, monkeypatch, mode="fixed"):
    """the whole deck through main.run: the top of the clamped column ends at the deck's value exactly and at rest, every record
    carries one reaction per moved entry, and the same deck without amplitude= raises the message it always raised"""
    from femcy_amd import main
    monkeypatch.setenv("FEMCY_BACKEND", backend)
    path = os.path.join(str(tmpdir), "pull_%s.inp" % mode)
    dynamic = None if mode == "fixed" else eac.auto_dynamic(64 * 1.0e-5, 4, 0.05)      # T is a few stable increments
    nodes, nsets, T = write_pull_deck(path, dynamic=dynamic)
    inp, system = main.run(path, verbose=False)
    try:
        u, v = system.dof.to_numpy(), system.ctx.download(be.VEC_VEL)
        top = nsets["top"] * 3 + 2
        assert system.increments[-1]["time1"] == T and len(system.increments) >= 3
        assert same_bits(u[top], np.full(top.size, PULL)) and not v[top].any()
        assert [m["amplitude"] for m in system.motion] == ["PULL"] and np.array_equal(system.motion[0]["node_set"], nsets["top"])
        reactions = [rec["reaction"] for rec in system.increments]
        assert all(len(r) == 1 and np.isfinite(r[0]) for r in reactions)
        print(f"pulled bar {mode} [{backend}]: reactions {[r[0] for r in reactions]}")
        foot = np.concatenate([nsets["foot"] * 3 + k for k in range(3)])
        assert not u[foot].any() and np.abs(u).max() <= 1.5 * PULL
    finally:
        system.ctx.close()
    write_pull_deck(path, boundary="*Boundary\ntop, 3, 3, %r\n" % PULL, dynamic=dynamic)
    with pytest.raises(ValueError, match="a non-zero \\*Boundary value in a \\*Dynamic step \\(prescribed motion\\) has not been supported"):
        main.run(path, verbose=False)
    return reactions


def plain_deck_is_unchanged(tmpdir, backend):
    """a deck without motion: no new key in its records, no motion on its system"""
    path = os.path.join(str(tmpdir), "bar.inp")
    ec.write_case_deck(path, "bar")
    inp, system, U, V = ec.solve_deck(path, backend)
    assert inp.amplitudes == {} and system.motion == [] and all("reaction" not in rec for rec in system.increments)
    assert all("amplitude" not in bc for bc in inp.dirichlet_bc_info)


def gate(backend):
    """_transient_gate on bare namespaces, as the recorded driver cases call it: a value without an amplitude is refused with
    today's text, an amplitude outside the explicit procedure is refused, an unknown name is refused"""
    from types import SimpleNamespace
    from femcy_amd.stiffnessMtrx import System_of_equations, deck_view
    nodes, el, ELE = mesh("C3D4", 9)
    gate_of = System_of_equations._transient_gate
    me = SimpleNamespace(part=None)
    deck = lambda bcs, amps=None: SimpleNamespace(density=1.0, dirichlet_bc_info=bcs, amplitudes=amps or {})
    bc = lambda val, **kw: dict(node_set=[0], dof=0, val=val, user=False, **kw)
    today = "a non-zero \\*Boundary value in a \\*Dynamic step \\(prescribed motion\\) has not been supported"
    for motion in (False, True):
        with pytest.raises(ValueError, match=today):
            gate_of(me, deck([bc(0.0), bc(0.01)]), "step", "mass", motion=motion)
        gate_of(me, deck([bc(0.0)]), "step", "mass", motion=motion)
    with pytest.raises(ValueError, match="explicit alone"):
        gate_of(me, deck([bc(0.0, amplitude="A")], {"A": {}}), "*Dynamic step", "mass matrix")
    with pytest.raises(ValueError, match="no \\*Amplitude of that name"):
        gate_of(me, deck([bc(0.01, amplitude="B")], {"A": {}}), "step", "mass", motion=True)
    gate_of(me, deck([bc(0.01, amplitude="A")], {"A": {}}), "step", "mass", motion=True)
    assert deck_view(SimpleNamespace(neumann_bc_info=[], dirichlet_bc_info=[], time_incs={}, geometric_nonlinear=False)).amplitudes == {}


def measure_f64_worst():
    """the constants at the top, as measured"""
    return {"fixed": {case: max(reference_fixed(case, fam, nn)[2] for fam, nn in MESHES) for case in FIXED},
            "start": max(reference_fixed(case, fam, nn)[3] for fam, nn in MESHES for case in FIXED),
            "auto": max(reference_auto(fam, nn)[2] for fam, nn in MESHES),
            "amp": max(reference_amp(kind)[1] for kind in (mr.TABULAR, mr.SMOOTH_STEP))}
