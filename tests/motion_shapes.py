"""List and slot edges of prescribed motion and the energy balance in explicit dynamics (csrc/kernels_explicit.hip:
k_explicit_place, the curve table of the node pass, energy_wave_sum and the slots of explicit_node_pass_energy,
k_explicit_energy_sum; csrc/element_math.hpp: amplitude, explicit_energy_moved; csrc/motion_tables.hpp), and fixed mass scaling
chained with damping, motion and the balance.  Written against the C ABI (femcy_amd.backend.Context) so that the host backend
(tests/test_motion_shapes_cpu.py, backend "cpu") and the device (tests/test_gpu_motion_shapes.py, backend "hip") run the same
code.  Every function checks its own result and returns the figure it checked.  The case tables are static; nothing is skipped
at run time.

1. place() -- the compact moved list at 255, 256, 257 and 513 entries (one thread per entry, 256 a workgroup) on a CPS4 plate
   of 625 nodes and a C3D4 plate of 343: a seeded permutation of the DOFs dealt round-robin into four held sets, each with its
   own value and curve (PLACE_CURVES: 2, 6, 16 and 16 points), so list order is not DOF order; a fifth set names every 7th
   entry of the list again with another value (and, but for the entries of the second set, another curve), which must win and
   keep its place; a sixth is held and not moved.  u, v, a of every entry after the start, after one step and after three
   more, each relative to |g| max|A|, |g| max|A'|, |g| max|A''| of its own curve; the free DOFs against the long-double
   trajectory.  place_auto(): the same list under the device clock, and bit for bit unchanged by steps past T.
2. curves() -- four curves (16-point tabular, 16-point smooth step, 2-point tabular, 2-point smooth step; interval lengths from
   2^-8 to 4) created as ids 0 .. 3 and handed to set_motion in the order 2, 0, 3, 1, so that the table's index differs from
   the id; every DOF at every time of every table (motion_cases.amp_times extended), the exact assertions of
   motion_cases.amplitude_values, the rest against long double.
3. hubs() -- the fans of 32, 33, 64 and 65 triangles of dyn_shapes (the hub takes a second trip of the node gather and stands
   alone in the last workgroup): the hub moved in both components, or the hub free and the rim moved, damped, with the balance
   running.
4. slots() -- the read-back of the balance at 252, 256, 256, 260, 1024 and 1028 slots (nn = 504, 505, 512, 513, 2041, 2049;
   SLOT_MESHES); an odd nn leaves a wavefront of one node and a workgroup of three empty wavefronts.  A full run, a run whose
   addends start in the last nodes, and a split run.
5. scaled() -- femcy_lumped_mass_scale, create, set_motion, set_damping, energy_enable in the deck driver's order, fixed and
   element by element, against the restatement with the scaled shares (the bulk viscosity keeps the deck's density).

References.  The long-double restatements of motion_reference, explicit_damped_reference, energy_cases.energy_sums and
mass_scaling_cases.Reference; no library code runs in them.  _Offset only adds a constant displacement to what they evaluate,
so that motion_reference.verlet_motion, which starts from u = 0, also serves a run that starts from a random u_0.

Bounds.  measure_f64_worst() measures, per group, the worst difference between the float64 restatement and the long-double
one on the very cases run here; a backend is held to 4 x a constant that is at least that (the rounding of a second float64
evaluation in another order).  Where the measured figure is within a constant that exists -- motion_cases.F64_WORST_AMP,
motion_cases.F64_WORST_FIXED, motion_cases.F64_WORST_AUTO, energy_cases.F64_WORST -- that constant is used (USES below);
otherwise the group has its own, asserted by tests/test_motion_shapes_cpu.py to be the measured one.  Energy figures are
relative to S = sum |addends|, state figures to the largest entry of the reference, moved entries as said in 1."""
import collections
import contextlib
import functools

import numpy as np

from femcy_amd import backend as be

import dyn_shapes as ds
import energy_cases as enc
import explicit_auto_cases as eac
import explicit_cases as ec
import explicit_damped_cases as edc
import explicit_damped_reference as edr
import explicit_reference as er
import loads_cases as lc
import loads_reference as lr
import mass_scaling_cases as msc
import motion_cases as mc
import motion_reference as mr

LD = np.longdouble
RHO = ec.RHO
BOTH = enc.DAMPINGS["both"]
KIND = {mr.TABULAR: "tabular", mr.SMOOTH_STEP: "smooth step"}
# group -> the constant its bound rests on.  A state group takes the tightest of STATE_CONSTANTS that holds its measured figure,
# an energy group energy_cases.F64_WORST; "own": no constant that exists holds it.  As measured (measure_f64_worst): the moved
# entries of place() 4.88e-16, its whole vectors 4.42e-15, the four curves 1.78e-15, the fans 1.82e-14 (state) and 1.21e-15
# (energy), the full runs of slots() 5.22e-16, the scaled fixed runs 8.94e-15, the scaled automatic runs 1.84e-13, their
# accumulators 2.10e-15, the identity 2.74e-17
USES = {"place moved": "amp", "place free": "fixed damped", "curves": "amp", "hubs state": "fixed smooth", "hubs energy": "energy",
        "slots full": "energy", "slots planted": "own", "scaled fixed": "fixed damped", "scaled auto": "auto",
        "scaled energy": "energy", "scaled identity": "energy"}
STATE_CONSTANTS = {"amp": mc.F64_WORST_AMP, "fixed damped": mc.F64_WORST_FIXED["damped"], "fixed smooth": mc.F64_WORST_FIXED["smooth"],
                   "fixed tabular": mc.F64_WORST_FIXED["tabular"], "auto": mc.F64_WORST_AUTO}
EXISTING = dict(STATE_CONSTANTS, energy=enc.F64_WORST)
# the planted runs of slots(), as measured: 3.55e-14 of S (504 nodes).  Everything but one node starts at rest, so the strains
# of the first states are tiny and the float64 forces, differences of numbers near 1, keep few digits of them; the velocity
# they give enters every addend.  energy_cases' runs start from strains of a per cent
F64_WORST_SLOTS_PLANTED = 3.6e-14
OWN = {"slots planted": "F64_WORST_SLOTS_PLANTED"}


def bound_of(group):
    """the float64 figure a group's bound rests on"""
    return globals()[OWN[group]] if USES[group] == "own" else EXISTING[USES[group]]


@contextlib.contextmanager
def energy_bound(group):
    """energy_cases.check holds a backend to energy_cases.TOL = 4 x energy_cases.F64_WORST; for the length of one call it
    holds it to 4 x the figure of `group` (the same number unless the group has its own)"""
    saved = enc.TOL
    enc.TOL = 4.0 * bound_of(group)
    try:
        yield
    finally:
        enc.TOL = saved


same_bits = mc.same_bits
scale_of = lambda k: mc.RAMP["s0"] + k * mc.RAMP["ds"]              # the ramp of motion_cases.run_fixed


class _Offset(edr.DampedModel):
    """the damped model about a constant displacement u0: every force is evaluated at u + u0"""
    u0 = None

    def _state(self, u):
        u = np.asarray(u, dtype=self.dtype)
        return super()._state(u if self.u0 is None else u + self.u0)


# one run: the held sets (DOF arrays), moves = [(set, value, curve)] in the order of the call, curves = [(kind, t, A)],
# damping = (alpha, b1, b2) or None
Case = collections.namedtuple("Case", "nodes el ELE sets moves curves f u0 v0 h damping")


def stable_h(nodes, el, ELE):
    """a power of two well inside the limit of the mesh at rest (energy_cases.setup's rule): k h is exact"""
    om = eac.Estimate(nodes, el, ELE, ec.material_of(ELE), RHO, np.float64).omega(np.zeros(nodes.size))
    return float(2.0 ** np.floor(np.log2(0.4 * 2.0 / float(om))))


def held_of(case):
    return np.unique(np.concatenate([np.asarray(s).ravel() for s in case.sets]))


def motion_of(case, dtype):
    return mr.Motion([(case.sets[k], g, case.curves[c]) for k, g, c in case.moves], dtype)


def build(case, backend, energy=False):
    """the context and the integrator of a case, u_0, v_0 and f uploaded"""
    ctx = lc.make_ctx(case.nodes, case.el, case.ELE, backend)
    lm = ctx.lumped_mass(case.ELE, RHO)
    ex = finish(ctx, lm, case, energy)
    return ctx, ex, lm


def finish(ctx, lm, case, energy):
    """create, set_motion, set_damping, energy_enable: the deck driver's order"""
    ids = [ctx.dofset(s) for s in case.sets]
    ex = ctx.explicit(lm, ids)
    amps = [ctx.amplitude(KIND[k], t, A) for k, t, A in case.curves]
    ctx.explicit_set_motion(ex, [ids[k] for k, _, _ in case.moves], [g for _, g, _ in case.moves], [amps[c] for _, _, c in case.moves])
    if case.damping is not None:
        ctx.explicit_set_damping(ex, case.damping[0], case.damping[1], case.damping[2], edc.modulus(ec.material_of(case.ELE)))
    if energy:
        ctx.explicit_energy_enable(ex, True)
    for vec, arr in ((be.VEC_DOF, case.u0), (be.VEC_VEL, case.v0), (be.VEC_RHS, case.f)):
        ctx.upload(vec, arr)
    ctx.upload(be.VEC_ACC, np.full(case.nodes.size, np.nan))          # not read at the start
    return ex


def restate(case, dtype, nsteps, energy=False, m=None):
    """the fixed run of a case in dtype -> (U, V, A) with U the displacement itself, (W, S) or None, the Motion.
    m: the nodal masses (None: the unscaled lumped mass)"""
    mat = ec.material_of(case.ELE)
    c = case.damping or (0.0, 0.0, 0.0)
    mdl = _Offset(case.nodes, case.el, case.ELE, mat, dtype, RHO, c[0], c[1], c[2], edc.modulus(mat))
    if np.any(case.u0):
        mdl.u0 = np.asarray(case.u0, dtype=dtype)
    m = er.lumped_mass(case.nodes, case.el, case.ELE, RHO, dtype) if m is None else np.asarray(m, dtype=dtype)
    minv = 1 / np.repeat(m, case.ELE.dm)
    minv[held_of(case)] = 0
    motion = motion_of(case, dtype)
    U, V, A = mr.verlet_motion(mdl, minv, case.f, case.v0, case.h, nsteps, scale_of, motion)
    sums = None
    if energy:
        sums = enc.energy_sums(mdl, minv, m, case.f, U, V, A, [case.h] * nsteps, [scale_of(k) for k in range(nsteps + 1)], motion.dofs)
    if mdl.u0 is not None:
        U = U + mdl.u0[None, :]
    return (U, V, A), sums, motion


def energy_error(W64, W, S):
    return max(float(abs(LD(W64[j]) - W[j]) / S[j]) for j in range(4) if S[j] != 0)


def state_error(got, ref, k):
    return max(mc.relerr(g, w[k]) for g, w in zip(got, ref))


# ------------------------------------------------------------------------------------------------ 1. place()
PLACE_MESHES = {"CPS4-625": ("CPS4", (24, 24), 0.2, 625), "C3D4-343": ("C3D4", (6, 6, 6), 0.25, 343)}
PLACE_NMOVED = (255, 256, 257, 513)
PLACE_CASES = [(name, nm) for name in PLACE_MESHES for nm in PLACE_NMOVED]
PLACE_PARTS = (1, 3)
PLACE_AUTO_NMOVED, PLACE_AUTO_STEPS, PLACE_AUTO_BATCHES = 257, 12, (5, 30)
PLACE_VALUES = (1.0, -0.7, 0.6, -0.8, 0.5)                            # x 0.004 of the mesh size; the fifth set's last
PLACE_AGAIN_CURVE = 1
# fractions of T.  The first curve starts at 0 and ends before T; the others start late, from a value that is not 0
_PLACE_LEN = np.array([3, 1, 4, 1, 5, 9, 2, 6, 5, 3, 5, 8, 9, 7, 9], dtype=np.float64)
PLACE_CURVES = ((mr.TABULAR, [0.0, 0.875], [0.0, 1.0]),
                (mr.SMOOTH_STEP, [0.0625, 0.2, 0.45, 0.6, 1.1, 2.0], [0.2, -1.0, 0.5, 0.5, -0.3, 0.8]),
                (mr.TABULAR, list(0.03125 + np.concatenate([[0.0], np.cumsum(_PLACE_LEN)]) * (1.5 / _PLACE_LEN.sum())),
                 [0.3, -0.6, 0.9, 0.1, -1.0, 0.4, 0.4, -0.2, 0.7, -0.9, 0.5, 0.0, -0.3, 0.8, -0.5, 0.25]),
                (mr.SMOOTH_STEP, list(0.046875 + np.concatenate([[0.0], np.cumsum(_PLACE_LEN[::-1])]) * (1.25 / _PLACE_LEN.sum())),
                 [-0.4, 0.7, -0.8, 0.2, 1.0, -0.1, 0.6, 0.6, -0.7, 0.3, -1.0, 0.9, 0.05, -0.45, 0.35, -0.2]))


@functools.lru_cache(maxsize=None)
def place_case(name, nmoved, auto=False):
    """-> the Case, the library's list (the four sets one after the other), the fifth set, the held set that is not moved, T"""
    family, cells, perturb, nn = PLACE_MESHES[name]
    nodes, el, ELE = lr.mesh(family, cells=cells, perturb=perturb)
    nodes = np.ascontiguousarray(nodes, dtype=np.float64)
    assert len(nodes) == nn and nodes.size > nmoved + 8
    rng = np.random.default_rng(nmoved)
    perm = rng.permutation(nodes.size)
    dealt = [perm[:nmoved][j::4] for j in range(4)]
    order = np.concatenate(dealt)
    again, rest = order[::7], perm[nmoved:nmoved + 5]
    h = stable_h(nodes, el, ELE)
    if auto:
        om = eac.Estimate(nodes, el, ELE, ec.material_of(ELE), RHO, np.float64).omega(np.zeros(nodes.size))
        T = float(PLACE_AUTO_STEPS * mc.AUTO_SF * 2 / om)
    else:
        T = sum(PLACE_PARTS) * h
    curves = tuple((k, [float(x) * T for x in t], list(A)) for k, t, A in PLACE_CURVES)
    g = 0.004 * np.ptp(nodes, axis=0).max()
    moves = [(j, g * PLACE_VALUES[j], j) for j in range(4)] + [(4, g * PLACE_VALUES[4], PLACE_AGAIN_CURVE)]
    sets = dealt + [again, rest]
    v0, f = rng.uniform(-1.0, 1.0, nodes.size), rng.uniform(-1.0, 1.0, nodes.size)
    v0[np.concatenate(sets)] = 0.0
    case = Case(nodes, el, ELE, sets, moves, curves, f, np.zeros(nodes.size), v0, h, None)
    assert not np.array_equal(order, np.sort(order)) and len(np.unique(order)) == nmoved
    return case, order, again, rest, T


def curve_max(curve):
    """max |A|, max |A'|, max |A''| of a curve in long double (a smooth step is monotone between two points; 30 xi^2 (1 - xi)^2
    peaks at 15 / 8, 60 xi (1 - xi)(1 - 2 xi) at 10 / sqrt 3)"""
    kind, t, A = curve
    t, A = np.asarray(t, dtype=LD), np.asarray(A, dtype=LD)
    slope = np.abs(np.diff(A) / np.diff(t))
    if kind == mr.TABULAR:
        return np.abs(A).max(), slope.max(), LD(0)
    return np.abs(A).max(), slope.max() * LD(15) / 8, (slope / np.diff(t)).max() * 10 / np.sqrt(LD(3))


def moved_error(got, motion, t):
    """u, v, a of the moved entries at time t against motion (long double), each entry relative to |g| x the maximum of its
    own curve; where that is 0 (A'' of a tabular curve) the entry is 0 exactly"""
    want = motion.at(LD(t))
    scales = np.array([[abs(LD(g)) * x for x in curve_max(c)] for g, c in motion.rows], dtype=LD)
    worst = 0.0
    for col in range(3):
        d = np.abs(np.asarray(got[col], dtype=LD)[motion.dofs] - want[col])
        flat = scales[:, col] == 0
        assert not d[flat].any(), (col, t)
        if (~flat).any():
            worst = max(worst, float((d[~flat] / scales[~flat, col]).max()))
    return worst


@functools.lru_cache(maxsize=None)
def reference_place(name, nmoved):
    """-> U, V, A in long double, the long-double Motion, the float64 figures (moved entries, whole vectors) at the states
    the test reads"""
    case = place_case(name, nmoved)[0]
    n = sum(PLACE_PARTS)
    ref, _, motion = restate(case, LD, n)
    f64, _, motion64 = restate(case, np.float64, n)
    ends = [0] + list(np.cumsum(PLACE_PARTS))
    em = max(moved_error(_full(motion64, k * case.h, case), motion, k * case.h) for k in ends)
    ef = max(state_error([x[k] for x in f64], ref, k) for k in ends)
    for x in ref:
        x.setflags(write=False)
    return ref, motion, em, ef


def _full(motion, t, case):
    """the moved entries of a Motion at t scattered into whole vectors"""
    out = []
    for x in motion.at(motion.dtype(t)):
        full = np.zeros(case.nodes.size, dtype=motion.dtype)
        full[motion.dofs] = x
        out.append(full)
    return out


def place(name, nmoved, backend):
    """k_explicit_place behind the start, behind the first drift of a call of one step and of a call of three"""
    case, order, again, rest, T = place_case(name, nmoved)
    ref, motion, _, _ = reference_place(name, nmoved)
    assert np.array_equal(motion.dofs, np.sort(order)) and len(again) == -(-nmoved // 7)
    late = [i for i, (g, c) in enumerate(motion.rows) if c[1][0] > 0]
    assert len(late) > nmoved // 2 and np.abs(motion.at(LD(0))[0][late]).min() > 0      # a place left out at the start shows
    ctx, ex, _ = build(case, backend)
    junk = np.zeros(case.nodes.size)
    junk[order] = 3.0                                                  # u and v of a moved DOF are set, never read
    ctx.upload(be.VEC_DOF, junk)
    ctx.upload(be.VEC_VEL, case.v0 + junk)
    ctx.explicit_start(ex, be.VEC_RHS, scale_of(0))
    states, done = [mc.state(ctx)], 0
    for k in PLACE_PARTS:
        ctx.explicit_advance(ex, k, case.h, be.VEC_RHS, scale_of(done), mc.RAMP["ds"])
        done += k
        states.append(mc.state(ctx))
    ctx.close()
    em = ef = 0.0
    for k, st in zip([0] + list(np.cumsum(PLACE_PARTS)), states):
        em = max(em, moved_error(st, motion, k * case.h))
        ef = max(ef, state_error(st, ref, k))
        assert not any(x[rest].any() for x in st), k                   # held and not moved: exactly 0
    # the fifth set won, and kept its place: its entries carry its value and curve (the reference's Motion says the same)
    rows = {int(d): r for d, r in zip(motion.dofs, motion.rows)}
    assert all(rows[int(d)][0] == case.moves[4][1] and rows[int(d)][1] is case.curves[PLACE_AGAIN_CURVE] for d in again)
    first = np.setdiff1d(case.sets[0], again)                          # the first curve ends before T: at rest, exactly
    u, v, a = states[-1]
    assert same_bits(u[first], np.full(first.size, np.float64(case.moves[0][1]) * np.float64(case.curves[0][2][-1])))
    assert not v[first].any() and not a[first].any()
    print(f"place {name} {nmoved} [{backend}]: moved entries {em:.3e}, whole vectors {ef:.3e}")
    assert em <= 4.0 * bound_of("place moved"), em
    assert ef <= 4.0 * bound_of("place free"), ef
    return em, ef


@functools.lru_cache(maxsize=None)
def reference_place_auto(name):
    """the float64 Motion against the long-double one at a few times of the automatic run's table"""
    case, _, _, _, T = place_case(name, PLACE_AUTO_NMOVED, True)
    motion, motion64 = motion_of(case, LD), motion_of(case, np.float64)
    return motion, max(moved_error(_full(motion64, x * T, case), motion, np.float64(x * T)) for x in (0.0, 0.21, 0.37, 0.5, 0.77, 1.0))


def place_auto(name, backend):
    """the place under the clock: two batches, the second overshooting T; the moved DOFs sit at the clock's time after each,
    and a further batch (h_next = 0: nothing is written) leaves the state bit for bit alone"""
    case, order, again, rest, T = place_case(name, PLACE_AUTO_NMOVED, True)
    motion, _ = reference_place_auto(name)
    ctx, ex, _ = build(case, backend)
    last, clock, batches = mc.run_auto(ctx, ex, case.ELE, T, PLACE_AUTO_BATCHES)
    ctx.explicit_auto_advance(ex, 5, be.VEC_RHS)
    again_state, clock2 = mc.state(ctx), ctx.explicit_auto_state(ex)
    ctx.close()
    (_, clk1), (_, clk2) = batches
    assert clk1[3] == PLACE_AUTO_BATCHES[0] and 0.0 < clk1[0] < T and clk2[0] == T and clk2[3] < sum(PLACE_AUTO_BATCHES), (clk1, clk2)
    assert clock2 == clock and all(same_bits(x, y) for x, y in zip(last, again_state))
    em = max(moved_error(st, motion, clk[0]) for st, clk in batches)
    assert all(np.isfinite(x).all() and not x[rest].any() for st, _ in batches for x in st)
    print(f"place auto {name} [{backend}]: {clk2[3]} steps, moved entries at the clock's time {em:.3e}")
    assert em <= 4.0 * bound_of("place moved"), em
    return em


# ----------------------------------------------------------------------------------------------- 2. curves()
# interval lengths 2^e x (1 .. 2): from 2^-8 to 4
_CURVE_EXP = (-6, -2, 0, -4, 1, -7, -1, -3, 2, -5, 0, -8, -2, 1, -6)


def _long_table(seed, t0):
    rng = np.random.default_rng(seed)
    t = t0 + np.concatenate([[0.0], np.cumsum(2.0 ** np.array(_CURVE_EXP) * rng.uniform(1.0, 2.0, 15))])
    A = rng.uniform(-2.0, 2.0, 16)
    A[7] = A[6]                                                        # a flat interval
    return [float(x) for x in t], [float(x) for x in A]


CURVE_TABLES = ((mr.TABULAR,) + _long_table(21, 0.5), (mr.SMOOTH_STEP,) + _long_table(22, 0.375),
                (mr.TABULAR, [0.75, 3.0], [0.5, -1.25]), (mr.SMOOTH_STEP, [0.3125, 11.0], [-0.75, 2.0]))
CURVE_ORDER = (2, 0, 3, 1)                                             # the ids in the order of the call
CURVE_DOFS = (0, 2, 3, 5)                                              # the DOF of the k-th set of the call
CURVE_VALUES = (2.0 ** -10, 2.0 ** -8, 2.0 ** -12, 2.0 ** -9)        # powers of two scale exactly


def curve_times():
    """motion_cases.amp_times for every table: at, one ulp to either side of and a little away from every point; three places
    inside every interval; outside both ends of every table"""
    ts = [0.25, 40.0]
    for _, T, _ in CURVE_TABLES:
        for k, t in enumerate(T):
            ts += [t, np.nextafter(t, 0.0), np.nextafter(t, 100.0), t * (1 - 1e-9), t * (1 + 1e-9)]
            if k:
                ts += [T[k - 1] + x * (t - T[k - 1]) for x in (0.25, 0.5, 0.8125)]
    return sorted(set(float(t) for t in ts))


@functools.lru_cache(maxsize=None)
def reference_curves():
    """-> [curve][time, 3] in long double, the float64 figure (every column relative to its own largest entry)"""
    ts = curve_times()
    ref = [np.array([mr.amplitude(k, T, A, t, LD) for t in ts], dtype=LD) for k, T, A in CURVE_TABLES]
    f64 = [np.array([mr.amplitude(k, T, A, t, np.float64) for t in ts], dtype=np.float64) for k, T, A in CURVE_TABLES]
    e = max(mc.relerr(x[:, c], r[:, c]) for x, r in zip(f64, ref) for c in range(3) if np.abs(r[:, c]).max() > 0)
    return ref, e


def curves(backend):
    """one CPS3 element, every DOF held, four moved, each by its own curve; start + one step of dt = t leave A, A', A'' of
    every curve at t in u, v, a"""
    nodes, el, ELE, _ = lr.single("CPS3")
    ctx = lc.make_ctx(nodes, el, ELE, backend)
    every = ctx.dofset(np.arange(nodes.size))
    ones = [ctx.dofset(np.array([d])) for d in CURVE_DOFS]
    ex = ctx.explicit(ctx.lumped_mass(ELE, RHO), [every] + ones)
    ids = [ctx.amplitude(KIND[k], T, A) for k, T, A in CURVE_TABLES]
    assert ids == sorted(ids) and len(set(ids)) == 4
    ctx.explicit_set_motion(ex, ones, list(CURVE_VALUES), [ids[c] for c in CURVE_ORDER])
    ts = curve_times()
    got = []
    for t in ts:
        ctx.explicit_start(ex, be.VEC_RHS, 0.0)
        ctx.explicit_advance(ex, 1, t, be.VEC_RHS, 0.0, 0.0)
        got.append([[x[d] for x in mc.state(ctx)] for d in CURVE_DOFS])
    ctx.close()
    got = np.array(got)                                                # [time, set, 3]
    ref, _ = reference_curves()
    err = 0.0
    for s, c in enumerate(CURVE_ORDER):
        kind, T, A = CURVE_TABLES[c]
        mine = got[:, s, :] / CURVE_VALUES[s]
        err = max([err] + [mc.relerr(mine[:, col], ref[c][:, col]) for col in range(3) if np.abs(ref[c][:, col]).max() > 0])
        inside = set()
        for t, (a0, a1, a2) in zip(ts, mine):
            what = (c, t, a0, a1, a2)
            if t in T:
                k = T.index(t)
                assert a0 == A[k], what
                if kind == mr.SMOOTH_STEP or k in (0, len(T) - 1):
                    assert a1 == 0.0 and a2 == 0.0, what
                else:                                                  # the right-hand slope, in float64's own rounding
                    assert a1 == (A[k + 1] - A[k]) / (T[k + 1] - T[k]), what
            if t <= T[0] or t >= T[-1]:
                assert (a0, a1, a2) == (A[0] if t <= T[0] else A[-1], 0.0, 0.0), what
            else:
                inside.add(int(np.searchsorted(T, t, side="right")) - 1)
            if kind == mr.TABULAR:
                assert a2 == 0.0, what
        assert inside == set(range(len(T) - 1)), (c, inside)           # every interval was evaluated, the last one included
    print(f"curves [{backend}]: {len(ts)} times x 4 curves, {err:.3e}")
    assert err <= 4.0 * bound_of("curves"), err
    return err


# ------------------------------------------------------------------------------------------------- 3. hubs()
HUB_FANS = tuple(ds.GATHER_FANS)
HUB_MOTIONS = ("hub", "rim")
HUB_CASES = [(k, which) for k in HUB_FANS for which in HUB_MOTIONS]
HUB_PARTS = (7, 9)
HUB_SPLIT = 64


@functools.lru_cache(maxsize=None)
def hub_case(k, which):
    """hub: the hub moved in both components, by two curves.  rim: the hub free, the first component of every rim node moved
    (alternating between the two curves), rim node 3 held and not moved"""
    nodes, el, ELE = ds.shape_mesh("fan-%d" % k)
    ds.gather_edge("fan-%d" % k)
    hub = len(nodes) - 1
    rim = np.setdiff1d(np.unique(el[(el == hub).any(axis=1)]), [hub])
    assert len(rim) == k and 3 in rim
    h = stable_h(nodes, el, ELE)
    g = 0.004 * np.ptp(nodes, axis=0).max()
    three = np.array([6, 7])
    if which == "hub":
        sets = [np.array([2 * hub]), np.array([2 * hub + 1]), three]
    else:
        others = rim[rim != 3]
        sets = [2 * others[0::2], 2 * others[1::2], three]
    moves = [(0, g, 0), (1, -0.7 * g, 1)]
    rng = np.random.default_rng(k)
    v0, f = rng.uniform(-1.0, 1.0, nodes.size), rng.uniform(-1.0, 1.0, nodes.size)
    v0[np.concatenate(sets)] = 0.0
    case = Case(nodes, el, ELE, sets, moves, mc.curves(mr.SMOOTH_STEP, sum(HUB_PARTS) * h), f, np.zeros(nodes.size), v0, h, BOTH)
    return case, hub


@functools.lru_cache(maxsize=None)
def reference_hub(k, which):
    """-> U, V, A, W, S in long double, the hub's own share of S[BOUNDARY], the float64 figures (state, energy)"""
    case, hub = hub_case(k, which)
    n = sum(HUB_PARTS)
    ref, (W, S), motion = restate(case, LD, n, True)
    f64, (W64, _), _ = restate(case, np.float64, n, True)
    share = 0.0
    if which == "hub":
        mat = ec.material_of(case.ELE)
        mdl = edr.DampedModel(case.nodes, case.el, case.ELE, mat, LD, RHO, BOTH[0], BOTH[1], BOTH[2], edc.modulus(mat))
        m = er.lumped_mass(case.nodes, case.el, case.ELE, RHO, LD)
        minv = 1 / np.repeat(m, 2)
        minv[held_of(case)] = 0
        own = enc.energy_sums(mdl, minv, m, case.f, ref[0], ref[1], ref[2], [case.h] * n, [scale_of(j) for j in range(n + 1)],
                              [2 * hub, 2 * hub + 1])[1]
        share = float(own[3] / S[3])
    es = max(state_error([x[j] for x in f64], ref, j) for j in np.cumsum(HUB_PARTS))
    for x in ref:
        x.setflags(write=False)
    return ref, W, S, share, es, energy_error(W64, W, S)


def run_parts(case, backend, parts, energy=True):
    """start, one advance per part -> the states after every call, the accumulators"""
    ctx, ex, _ = build(case, backend, energy)
    states = mc.run_fixed(ctx, ex, parts, case.h)
    got = ctx.explicit_energy(ex) if energy else None
    ctx.close()
    return states, got


def hubs(k, which, backend):
    """u, v, a after every call and the four accumulators with a moved DOF on a node whose gather takes two trips (hub), or
    beside one (rim); at 64 triangles a split run against one call, bit for bit"""
    case, hub = hub_case(k, which)
    ref, W, S, share, _, _ = reference_hub(k, which)
    assert S[3] > 0 and (which != "hub" or share >= 0.1), (S, share)
    states, got = run_parts(case, backend, HUB_PARTS)
    es = max(state_error(st, ref, j) for j, st in zip(np.cumsum(HUB_PARTS), states))
    ee = enc.check(got, W, S, f"fan-{k} {which} [{backend}]")
    assert not any(x[case.sets[2]].any() for st in states for x in st)
    if k == HUB_SPLIT:
        one, got1 = run_parts(case, backend, (sum(HUB_PARTS),))
        assert all(same_bits(x, y) for x, y in zip(one[-1], states[-1])) and same_bits(got1, got), (got1, got)
    print(f"fan-{k} {which} [{backend}]: u, v, a {es:.3e}, accumulators {ee:.3e} of S")
    assert es <= 4.0 * bound_of("hubs state"), es
    return es, ee


# ------------------------------------------------------------------------------------------------ 4. slots()
# nn -> (cells of the CPS3 plate, elements kept, slots): the elements cell by cell, r rows of cells and c more, which name
# (r + 1)(nx + 1) + c + 1 nodes; the last node and the one before it stand in the row that was begun
SLOT_MESHES = {504: ((15, 31), 914, 252), 505: ((15, 31), 916, 256), 512: ((12, 39), 920, 256), 513: ((12, 39), 922, 260),
               2041: ((30, 65), 3890, 1024), 2049: ((28, 70), 3900, 1028)}
SLOT_VARIANTS = ("full", "planted")
SLOT_CASES = [(nn, variant) for nn in SLOT_MESHES for variant in SLOT_VARIANTS]
SLOT_PARTS = {"full": (3, 5), "planted": (2,)}
SLOT_SPLIT = (505, 513)


@functools.lru_cache(maxsize=None)
def slot_mesh(nn):
    cells, keep, slots = SLOT_MESHES[nn]
    nodes, el, ELE = lr.mesh("CPS3", cells=cells, perturb=0.2)
    el = el.reshape(2, cells[0] * cells[1], 3).transpose(1, 0, 2).reshape(-1, 3)       # cell by cell: lower, upper
    nodes, el = ds._first(nodes, el, keep)
    assert len(nodes) == nn and len(np.unique(el)) == nn and 4 * -(-nn // 8) == slots, (nn, len(nodes))
    assert lr.mesh_volume(nodes, el, ELE) > 0
    return np.ascontiguousarray(nodes, dtype=np.float64), np.ascontiguousarray(el, dtype=np.int32), ELE


@functools.lru_cache(maxsize=None)
def slot_case(nn, variant):
    """the last node moved with every component, node nn - 2 with its first; the nodes on x = min held.  full: random u_0, v_0
    and f (energy_cases.setup; u_0 of 5 % of a cell).  planted: everything 0 but v_0 and f of the last free node, nn - 3"""
    nodes, el, ELE = slot_mesh(nn)
    cells = SLOT_MESHES[nn][0]
    _, foot = ec.held_dofs(nodes)
    sets = [np.array([2 * nn - 2, 2 * nn - 1]), np.array([2 * nn - 4]), foot]
    assert not np.intersect1d(foot, np.arange(2 * nn - 6, 2 * nn)).size
    h = stable_h(nodes, el, ELE)
    g = 0.004 * min(3.0 / cells[0], 2.0 / cells[1]) * 8
    rng = np.random.default_rng(11)
    u0 = 0.05 * min(3.0 / cells[0], 2.0 / cells[1]) * rng.uniform(-1.0, 1.0, nodes.size)
    v0, f = rng.uniform(-1.0, 1.0, nodes.size), rng.uniform(-1.0, 1.0, nodes.size)
    if variant == "planted":
        u0[:], keep = 0.0, np.array([2 * nn - 6, 2 * nn - 5])
        v0p, fp = np.zeros(nodes.size), np.zeros(nodes.size)
        v0p[keep], fp[keep] = (1.0, -0.5), (0.7, 0.4)
        v0, f = v0p, fp
    held = np.concatenate(sets)
    u0[held] = v0[held] = 0.0
    return Case(nodes, el, ELE, sets, [(0, g, 0), (1, -0.7 * g, 1)], mc.curves(mr.SMOOTH_STEP, 8 * h), f, u0, v0, h, BOTH)


@functools.lru_cache(maxsize=None)
def reference_slots(nn, variant):
    """-> W, S in long double and the float64 figure.  (The long-double run of 8 steps at 2049 nodes takes about a second:
    no case is shortened)"""
    case = slot_case(nn, variant)
    n = sum(SLOT_PARTS[variant])
    _, (W, S), _ = restate(case, LD, n, True)
    _, (W64, _), _ = restate(case, np.float64, n, True)
    return W, S, energy_error(W64, W, S)


def slots(nn, variant, backend):
    """the four accumulators of a run whose read-back sums SLOT_MESHES[nn][2] slots"""
    case = slot_case(nn, variant)
    W, S, _ = reference_slots(nn, variant)
    assert S[0] > 0 and S[1] > 0 and S[2] > 0 and S[3] > 0, S
    states, got = run_parts(case, backend, SLOT_PARTS[variant])
    assert all(np.isfinite(x).all() for x in states[-1])
    with energy_bound("slots " + variant):
        return enc.check(got, W, S, f"slots {nn} {variant} [{backend}]")


def slots_split(nn, backend):
    """one call of 8 steps against 3 + 5, bit for bit: the wavefront of one node and the three empty ones of the last
    workgroup carry the load scale and the time across the calls"""
    case = slot_case(nn, "full")
    n = sum(SLOT_PARTS["full"])
    one, got1 = run_parts(case, backend, (n,))
    two, got2 = run_parts(case, backend, SLOT_PARTS["full"])
    assert nn % 8 == 1 and np.abs(got1).min() > 0
    assert all(same_bits(x, y) for x, y in zip(one[-1], two[-1])) and same_bits(got1, got2), (got1, got2)


# ----------------------------------------------------------------------------------------------- 5. scaled()
SCALED_MESHES = (("C3D4", 17), ("CPS4", 17))


@functools.lru_cache(maxsize=None)
def scaled_setup(family, nn):
    """-> nodes, el, ELE, tau (mass_scaling_cases.median_gap of the long-double increments), the number of scaled elements"""
    nodes, el, ELE = mc.mesh(family, nn)
    ref = msc.Reference(nodes, el, ELE, ec.material_of(ELE), RHO, LD)
    w2 = ref.w2()
    tau = msc.median_gap(2 / np.sqrt(w2))
    k = ref.scale(None, tau, "below min")["k"]
    assert 0 < (k != 1).sum() < len(el), k                             # both branches of max(1, .)
    assert np.abs(w2 * LD(tau) ** 2 / 4 - 1).min() > 1.0e-6            # mass_scaling_cases.reference_call's condition
    return nodes, el, ELE, tau, int((k != 1).sum())


def scaled_case(family, nn, T):
    nodes, el, ELE, sets, (moved, values, which), f, v0 = mc.setup(family, nn)
    return Case(nodes, el, ELE, sets, [(k, g, c) for k, g, c in zip(moved, values, which)], mc.curves(mr.SMOOTH_STEP, T), f,
                np.zeros(nodes.size), v0, mc.H, mc.DAMPING)


def scaled_parts(family, nn, dtype):
    """-> the scaled nodal masses and the estimate with the scaled shares, in dtype"""
    nodes, el, ELE, tau, _ = scaled_setup(family, nn)
    ref = msc.Reference(nodes, el, ELE, ec.material_of(ELE), RHO, dtype)
    ref.scale(None, tau, "below min")
    return ref.nodal(), ref.est


def scaled_build(case, family, nn, backend):
    """scale, create, set_motion, set_damping, energy_enable"""
    nodes, el, ELE, tau, count = scaled_setup(family, nn)
    mat = ec.material_of(ELE)
    ctx = eac.make_ctx(nodes, el, ELE, mat, backend)
    lm = ctx.lumped_mass(ELE, RHO)
    out = ctx.lumped_mass_scale(lm, float(eac.s_C(mat)), None, tau, "below min")
    assert out["scaled_elements"] == count and out["mass1"] > out["mass0"], out
    return ctx, finish(ctx, lm, case, True), lm


@functools.lru_cache(maxsize=None)
def reference_scaled_fixed(family, nn):
    """-> U, V, A, W, S, the Motion in long double; the float64 figures (state at the batch ends, energy)"""
    case = scaled_case(family, nn, mc.STEPS * mc.H)
    ref, (W, S), motion = restate(case, LD, mc.STEPS, True, scaled_parts(family, nn, LD)[0])
    f64, (W64, _), _ = restate(case, np.float64, mc.STEPS, True, scaled_parts(family, nn, np.float64)[0])
    es = max(state_error([x[k] for x in f64], ref, k) for k in np.cumsum(mc.PARTS))
    for x in ref:
        x.setflags(write=False)
    return ref, W, S, motion, es, energy_error(W64, W, S)


def identity_sides(m, dm, h, v0, a0, vN, aN, ke0, keN, W, md, held, Um, Am):
    """both sides of  [KE - h^2/8 a.M a]_N - [.]_0 = W_LOAD + W_BOUNDARY - W_INTERNAL - W_ALPHA - I  on the free DOFs, where
    I = sum 1/2 m du (a_prev + a) over the moved DOFs and steps is the work the supports spend on the moved nodes' own
    inertia (LOAD + BOUNDARY - INTERNAL of a moved DOF add up to exactly that); -> left, right, the magnitude of the terms.
    Everything in the dtype of m; Um, Am [K + 1, moved]: u and a of the moved DOFs at every state"""
    dt = m.dtype.type
    md_m = np.repeat(m, dm)
    left, mag = [], dt(0)
    for ke, v, a in ((ke0, v0, a0), (keN, vN, aN)):
        v, a = np.asarray(v, dtype=dt), np.asarray(a, dtype=dt)
        assert not a[np.setdiff1d(held, md)].any()
        ke_moved = (md_m[md] * v[md] * v[md]).sum() / 2
        a_free = a.copy()
        a_free[md] = 0
        corr = dt(h) ** 2 / 8 * (md_m * a_free * a_free).sum()
        left.append(dt(ke) - ke_moved - corr)
        mag += abs(dt(ke)) + ke_moved + corr
    add = md_m[md][None, :] * (Um[1:] - Um[:-1]) * (Am[:-1] + Am[1:]) / 2
    right = dt(W[0]) + dt(W[3]) - dt(W[1]) - dt(W[2]) - add.sum()
    return left[1] - left[0], right, mag + np.abs(add).sum()


@functools.lru_cache(maxsize=None)
def reference_scaled_identity(family, nn):
    """the float64 restatement's own miss of the identity, relative to the magnitudes"""
    case = scaled_case(family, nn, mc.STEPS * mc.H)
    m = scaled_parts(family, nn, np.float64)[0]
    (U, V, A), (W, S), motion = restate(case, np.float64, mc.STEPS, True, m)
    md = motion.dofs
    ke = [er.kinetic(m, V[k], case.ELE.dm, np.float64) for k in (0, -1)]
    lhs, rhs, mag = identity_sides(m, case.ELE.dm, case.h, V[0], A[0], V[-1], A[-1], ke[0], ke[1], W, md, held_of(case),
                                   U[:, md], A[:, md])
    return float(abs(lhs - rhs) / (S.sum() + mag))


def scaled_fixed(family, nn, backend):
    """motion_cases.STEPS steps in motion_cases.PARTS on the scaled mass: u, v, a at the batch ends, the accumulators, and the
    identity with the kinetic energy taken through the scaled mass"""
    case = scaled_case(family, nn, mc.STEPS * mc.H)
    ref, W, S, motion, _, _ = reference_scaled_fixed(family, nn)
    assert all(S[j] > 0 for j in range(4)), S
    ctx, ex, lm = scaled_build(case, family, nn, backend)
    m = ctx.lumped_mass_get(lm)
    em = msc.relmax(m, scaled_parts(family, nn, LD)[0])
    ctx.explicit_start(ex, be.VEC_RHS, scale_of(0))
    (_, v0, a0), ke0 = mc.state(ctx), ctx.explicit_kinetic_energy(ex, be.VEC_VEL)
    states, done = [], 0
    for k in mc.PARTS:
        ctx.explicit_advance(ex, k, case.h, be.VEC_RHS, scale_of(done), mc.RAMP["ds"])
        done += k
        states.append(mc.state(ctx))
    keN, got = ctx.explicit_kinetic_energy(ex, be.VEC_VEL), ctx.explicit_energy(ex)
    ctx.close()
    es = max(state_error(st, ref, k) for k, st in zip(np.cumsum(mc.PARTS), states))
    ee = enc.check(got, W, S, f"scaled {family}-{nn} [{backend}]")
    md = motion.dofs
    lhs, rhs, mag = identity_sides(m.astype(LD), case.ELE.dm, case.h, v0, a0, states[-1][1], states[-1][2], ke0, keN, got, md,
                                   held_of(case), ref[0][:, md], ref[2][:, md])
    s = float(S.sum() + mag)
    ei = float(abs(lhs - rhs)) / s
    print(f"scaled {family}-{nn} [{backend}]: scaled mass {em:.3e}, u, v, a {es:.3e}, accumulators {ee:.3e} of S, identity left "
          f"{float(lhs):.17e} right {float(rhs):.17e} ({ei:.3e} of {s:.3e})")
    assert em <= msc.SCALE_TOL, em
    assert es <= 4.0 * bound_of("scaled fixed"), es
    assert float(abs(lhs)) > 1e-3 * float(S[0]) and ei <= 4.0 * bound_of("scaled identity"), ei
    return es, ee, ei


@functools.lru_cache(maxsize=None)
def scaled_T(family, nn):
    """about motion_cases.AUTO_STEPS increments of the scaled estimate at rest"""
    est = scaled_parts(family, nn, LD)[1]
    return float(mc.AUTO_STEPS * mc.AUTO_SF * 2 / est.omega(np.zeros(mc.mesh(family, nn)[0].size)))


@functools.lru_cache(maxsize=None)
def reference_scaled_auto(family, nn):
    """-> (H, times, U, V, A), W, S, the batch ends in long double; the float64 figures (state and clock, energy)"""
    T = scaled_T(family, nn)
    case = scaled_case(family, nn, T)
    mat = ec.material_of(case.ELE)
    out = {}
    for dt in (LD, np.float64):
        m, est = scaled_parts(family, nn, dt)
        mdl = edr.DampedModel(case.nodes, case.el, case.ELE, mat, dt, RHO, mc.DAMPING[0], mc.DAMPING[1], mc.DAMPING[2], edc.modulus(mat))
        minv = 1 / np.repeat(m, case.ELE.dm)
        minv[held_of(case)] = 0
        motion = motion_of(case, dt)
        run = mr.verlet_auto_motion(mdl, est, minv, case.f, case.v0, mc.AUTO_SF, T, True, motion)
        Hs, times, U, V, A = run
        out[dt] = run, enc.energy_sums(mdl, minv, m, case.f, U, V, A, Hs, [t / dt(T) for t in times], motion.dofs)
    (run, (W, S)), (run64, (W64, _)) = out[LD], out[np.float64]
    Hs = run[0]
    assert len(run64[0]) == len(Hs) and 20 <= len(Hs) < sum(mc.AUTO_BATCHES), len(Hs)
    ends = [k for k in np.cumsum(mc.AUTO_BATCHES) if k < len(Hs)] + [len(Hs)]
    es = max([mc.relerr(x64[k], x[k]) for x64, x in zip(run64[2:], run[2:]) for k in ends]
             + [mc.relerr(run64[0], Hs), mc.relerr(run64[1], run[1])])
    return run, W, S, ends, es, energy_error(W64, W, S)


def scaled_auto(family, nn, backend):
    """element by element on the scaled mass: the increments and the clock follow the scaled estimate (the damped bound reads
    the scaled shares, the bulk viscosity the deck's density), the accumulators the scaled nodal mass; a further batch, all
    no-ops, leaves everything bit for bit alone"""
    T = scaled_T(family, nn)
    case = scaled_case(family, nn, T)
    (Hs, times, U, V, A), W, S, ends, _, _ = reference_scaled_auto(family, nn)
    ctx, ex, _ = scaled_build(case, family, nn, backend)
    last, clock, batches = mc.run_auto(ctx, ex, case.ELE, T)
    got = ctx.explicit_energy(ex)
    ctx.explicit_auto_advance(ex, 5, be.VEC_RHS)
    again, clock2, got2 = mc.state(ctx), ctx.explicit_auto_state(ex), ctx.explicit_energy(ex)
    ctx.close()
    assert clock[0] == T and clock[3] == len(Hs), clock
    assert clock2 == clock and same_bits(got, got2) and all(same_bits(x, y) for x, y in zip(last, again))
    es = 0.0
    for k, (st, clk) in zip(ends, batches):
        assert clk[3] == k, (clk, k)
        es = max([es, float(abs(LD(clk[0]) - times[k]) / times[-1]), float(abs(LD(clk[1]) - Hs[k - 1]) / Hs.max())]
                 + [mc.relerr(g, w[k]) for g, w in zip(st, (U, V, A))])
    ee = enc.check(got, W, S, f"scaled auto {family}-{nn} [{backend}]")
    print(f"scaled auto {family}-{nn} [{backend}]: {len(Hs)} steps, u, v, a and the clock {es:.3e}, accumulators {ee:.3e} of S")
    assert es <= 4.0 * bound_of("scaled auto"), es
    return es, ee


# ------------------------------------------------------------------------------------------- the constants
def measure_f64_worst():
    """group -> the worst difference between the float64 restatement and the long-double one on the cases run here"""
    hub = [reference_hub(*c) for c in HUB_CASES]
    fixed = [reference_scaled_fixed(*c) for c in SCALED_MESHES]
    auto = [reference_scaled_auto(*c) for c in SCALED_MESHES]
    return {"place moved": max([reference_place(*c)[2] for c in PLACE_CASES] + [reference_place_auto(n)[1] for n in PLACE_MESHES]),
            "place free": max(reference_place(*c)[3] for c in PLACE_CASES),
            "curves": reference_curves()[1],
            "hubs state": max(r[4] for r in hub), "hubs energy": max(r[5] for r in hub),
            "slots full": max(reference_slots(nn, "full")[2] for nn in SLOT_MESHES),
            "slots planted": max(reference_slots(nn, "planted")[2] for nn in SLOT_MESHES),
            "scaled fixed": max(r[4] for r in fixed), "scaled energy": max([r[5] for r in fixed] + [r[5] for r in auto]),
            "scaled auto": max(r[4] for r in auto),
            "scaled identity": max(reference_scaled_identity(*c) for c in SCALED_MESHES)}
