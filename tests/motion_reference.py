"""numpy restatement of prescribed motion in explicit dynamics (femcy_amplitude_create, femcy_explicit_set_motion), in any
dtype, written from the formulas

    xi = (t - t_k) / (t_{k+1} - t_k) on [t_k, t_{k+1})
    TABULAR      A = A_k + (A_{k+1} - A_k) xi,                              A' = (A_{k+1} - A_k) / dt_k,   A'' = 0
    SMOOTH STEP  A = A_k + (A_{k+1} - A_k) xi^3 (10 - 15 xi + 6 xi^2),      A' = rise / dt_k 30 xi^2 (1 - xi)^2,
                                                                            A'' = rise / dt_k^2 60 xi (1 - xi)(1 - 2 xi)
    clamped: (A_0, 0, 0) for t <= t_0, (A_last, 0, 0) for t >= t_last
    a moved DOF with the value g: u = g A(t), v = g A'(t), a = g A''(t) at the time of the state; every other DOF follows
    the damped velocity-Verlet recurrence of explicit_damped_reference, which reads the moved v and a in v_{n+1/2}

on top of explicit_damped_reference.DampedModel.  No library code runs here."""
import numpy as np

import explicit_damped_reference as edr

TABULAR, SMOOTH_STEP = 0, 1


def amplitude(kind, tp, Ap, t, dtype):
    """-> A(t), A'(t), A''(t) of the curve (tp, Ap) in dtype"""
    tp, Ap, t = np.asarray(tp, dtype=dtype), np.asarray(Ap, dtype=dtype), dtype(t)
    zero = dtype(0)
    if t <= tp[0]:
        return Ap[0], zero, zero
    if t >= tp[-1]:
        return Ap[-1], zero, zero
    k = int(np.searchsorted(tp, t, side="right")) - 1          # t_k <= t < t_{k+1}: the right-hand interval at a point
    dt, rise = tp[k + 1] - tp[k], Ap[k + 1] - Ap[k]
    xi = (t - tp[k]) / dt
    if kind == TABULAR:
        return Ap[k] + rise * xi, rise / dt, zero
    return (Ap[k] + rise * xi ** 3 * (10 - 15 * xi + 6 * xi * xi), rise / dt * 30 * xi * xi * (1 - xi) ** 2,
            rise / (dt * dt) * 60 * xi * (1 - xi) * (1 - 2 * xi))


class Motion:
    """the moved DOFs of one integrator: `entries` = [(dofs, value, (kind, tp, Ap))] in the order of the call, a later entry
    winning where two name the same DOF"""

    def __init__(self, entries, dtype):
        self.dtype, table = dtype, {}
        for dofs, g, curve in entries:
            for d in np.asarray(dofs).ravel():
                table[int(d)] = (g, curve)
        self.dofs = np.array(sorted(table), dtype=np.int64)
        self.rows = [table[int(d)] for d in self.dofs]

    def at(self, t):
        """-> u, v, a of the moved DOFs at time t"""
        dt = self.dtype
        out = np.array([[dt(g) * x for x in amplitude(c[0], c[1], c[2], t, dt)] for g, c in self.rows], dtype=dt).reshape(-1, 3)
        return out[:, 0], out[:, 1], out[:, 2]


def verlet_motion(mdl, minv, f, v0, h, nsteps, scale, motion):
    """the fixed-step recurrence of mdl (an edr.DampedModel) with the DOFs of `motion` moved; state k is at t = k h
    -> U, V, A [nsteps + 1, n]"""
    dt = mdl.dtype
    minv, f, h = np.asarray(minv, dtype=dt), np.asarray(f, dtype=dt), dt(h)
    md = motion.dofs
    assert (minv[md] == 0).all()
    u = np.zeros(mdl.nn * mdl.dm, dtype=dt)
    v = np.asarray(v0, dtype=dt) * (minv != 0)
    u[md], v[md], a_m = motion.at(dt(0))
    a = mdl.acceleration(minv, dt(scale(0)) * f, u, v)
    a[md] = a_m
    U, V, A = [u], [v], [a]
    for k in range(1, nsteps + 1):
        um, vm, am = motion.at(dt(k) * h)
        vh = v + (h / 2) * a
        u = u + h * v + (h * h / 2) * a
        u[md] = um
        an = mdl.acceleration(minv, dt(scale(k)) * f, u, vh)
        an[md] = am
        v = v + (h / 2) * (a + an)
        v[md] = vm
        a = an
        U.append(u), V.append(v), A.append(a)
    return np.array(U), np.array(V), np.array(A)


def verlet_auto_motion(mdl, est, minv, f, v0, sf, T, ramp, motion, max_steps=100000):
    """the variable-step recurrence of edr.verlet_auto_damped with the DOFs of `motion` moved, in the order of the library:
    the moved DOFs are placed at t = 0 before the first bound; a step drifts to t + h and places u there, evaluates the forces
    and the bound, kicks, and places v and a.  -> H [steps], times [steps + 1], U, V, A [steps + 1, n]"""
    dt = mdl.dtype
    minv, f, T, sf = np.asarray(minv, dtype=dt), np.asarray(f, dtype=dt), dt(T), dt(sf)
    scale = (lambda t: t / T) if ramp else (lambda t: dt(1))
    md = motion.dofs
    u, v, t = np.zeros(mdl.nn * mdl.dm, dtype=dt), np.asarray(v0, dtype=dt) * (minv != 0), dt(0)
    u[md], v[md], a_m = motion.at(t)
    a = mdl.acceleration(minv, scale(t) * f, u, v)
    a[md] = a_m
    om = mdl.omega_eff(est, u, v)
    H, times, U, V, A = [], [t], [u], [v], [a]
    while t < T and len(H) < max_steps:
        hs, rem = sf * (2 / om), T - t
        h, t = (rem, T) if hs >= rem else (hs, min(t + hs, T))
        um, vm, am = motion.at(t)
        vh = v + (h / 2) * a
        u = u + h * v + (h * h / 2) * a
        u[md] = um
        an = mdl.acceleration(minv, scale(t) * f, u, vh)
        an[md] = am
        om = mdl.omega_eff(est, u, vh)
        v = v + (h / 2) * (a + an)
        v[md] = vm
        a = an
        H.append(h), times.append(t), U.append(u), V.append(v), A.append(a)
    return np.array(H), np.array(times), np.array(U), np.array(V), np.array(A)
