"""numpy restatement of damped explicit dynamics (femcy_explicit_set_damping), in any dtype, written from the formulas

    v_{n+1/2} = v_n + h/2 a_n                      (v_{-1/2} := v_0 at the start)
    rate_q = sum_a v_{a,n+1/2} . grad_x N_a,   L_q = (max_a |grad_x N_a|^2)^(-1/2),   rho_q = rho_0 / det F_q
    p_q    = b1 sqrt(rho_q M_d) L_q rate_q + rho_q (b2 L_q)^2 |rate_q| min(0, rate_q)
    f_bv[a] = sum_e sum_q grad_x N_a p_q det J_q(x) w_q
    a_{n+1} = minv (s f - f_int(u_{n+1}) - f_bv(u_{n+1}, v_{n+1/2})) - alpha v_{n+1/2},   v_{n+1} = v_n + h/2 (a_n + a_{n+1})
    omega_eff,e = omega_e (sqrt(1 + xi_e^2) + xi_e),   xi_e = alpha / (2 omega_e) + b1 + b2^2 max_q [L_q sqrt(rho_q / M_d) max(0, -rate_q)]

on top of explicit_reference.Model.  A held DOF (minv = 0) takes no damping force.  No library code runs here."""
import numpy as np

import explicit_reference as er


class DampedModel(er.Model):
    def __init__(self, nodes, el, ELE, material, dtype, rho0, alpha=0.0, b1=0.0, b2=0.0, Md=0.0):
        super().__init__(nodes, el, ELE, material, dtype)
        self.rho0, self.alpha, self.b1, self.b2, self.Md = (dtype(x) for x in (rho0, alpha, b1, b2, Md))

    def points(self, u, vhalf):
        """-> grad_x N [e, g, a, j], det J_x [e, g], rate, L, rho [e, g]"""
        J, F = self._state(u)
        gx = np.einsum("gak,egkj->egaj", self.dN, er._inv(J))
        V = np.asarray(vhalf, dtype=self.dtype).reshape(self.nn, self.dm)[self.el]
        rate = np.einsum("eaj,egaj->eg", V, gx)
        L = 1 / np.sqrt((gx * gx).sum(axis=-1).max(axis=-1))
        return gx, er._det(J), rate, L, self.rho0 / np.abs(er._det(F))

    def pressure(self, u, vhalf):
        gx, detJ, rate, L, rho = self.points(u, vhalf)
        p = self.b1 * np.sqrt(rho * self.Md) * L * rate + rho * (self.b2 * L) ** 2 * np.abs(rate) * np.minimum(0, rate)
        return p, gx, detJ

    def f_bv(self, u, vhalf):
        p, gx, detJ = self.pressure(u, vhalf)
        fe = np.einsum("egai,eg->eai", gx, p * detJ * self.w[None, :])
        f = np.zeros((self.nn, self.dm), dtype=self.dtype)
        np.add.at(f, self.el, fe)
        return f.ravel()

    def acceleration(self, minv, sf, u, vhalf):
        """minv (s f - f_int - f_bv) - alpha v_{n+1/2}; sf = the scaled load vector"""
        a = minv * (sf - self.f_int(u) - (self.f_bv(u, vhalf) if (self.b1 != 0 or self.b2 != 0) else 0))
        return a - self.alpha * vhalf * (minv != 0)

    def verlet_damped(self, minv, f, v0, h, nsteps, scale, u0=None):
        """-> U, V, A [nsteps + 1, n]; scale(k) = the load scale of state k"""
        dt = self.dtype
        minv, f, h = np.asarray(minv, dtype=dt), np.asarray(f, dtype=dt), dt(h)
        u = np.zeros(self.nn * self.dm, dtype=dt) if u0 is None else np.asarray(u0, dtype=dt)
        v = np.asarray(v0, dtype=dt) * (minv != 0)
        a = self.acceleration(minv, dt(scale(0)) * f, u, v)
        U, V, A = [u], [v], [a]
        for k in range(1, nsteps + 1):
            vh = v + (h / 2) * a
            u = u + h * v + (h * h / 2) * a
            an = self.acceleration(minv, dt(scale(k)) * f, u, vh)
            v = v + (h / 2) * (a + an)
            a = an
            U.append(u), V.append(v), A.append(a)
        return np.array(U), np.array(V), np.array(A)

    def omega_eff(self, est, u, vhalf):
        """max_e omega_eff,e from an explicit_auto_cases.Estimate of the same mesh and dtype"""
        om = np.sqrt(est.elements(u)[1])
        xi = self.b1 + (self.alpha / (2 * om) if self.alpha != 0 else 0)
        if self.b2 != 0:
            _, _, rate, L, rho = self.points(u, vhalf)
            xi = xi + self.b2 ** 2 * (L * np.sqrt(rho / self.Md) * np.maximum(0, -rate)).max(axis=1)
        return (om * (np.sqrt(1 + xi * xi) + xi)).max()


def verlet_auto_damped(mdl, est, minv, f, v0, sf, T, ramp, max_steps=100000):
    """the variable-step damped recurrence in mdl.dtype, in the order of the library: the bound at (u_0, v_0) gives h_0; a step
    drifts by h, evaluates the forces and the bound at (u_{n+1}, v_{n+1/2}) -- which gives the next h -- and kicks.
    -> H [steps], times [steps + 1], U, V [steps + 1, n]"""
    dt = mdl.dtype
    minv, f, T, sf = np.asarray(minv, dtype=dt), np.asarray(f, dtype=dt), dt(T), dt(sf)
    scale = (lambda t: t / T) if ramp else (lambda t: dt(1))
    u, v, t = np.zeros(mdl.nn * mdl.dm, dtype=dt), np.asarray(v0, dtype=dt) * (minv != 0), dt(0)
    a = mdl.acceleration(minv, scale(t) * f, u, v)
    om = mdl.omega_eff(est, u, v)
    H, times, U, V = [], [t], [u], [v]
    while t < T and len(H) < max_steps:
        hs, rem = sf * (2 / om), T - t
        h, t = (rem, T) if hs >= rem else (hs, min(t + hs, T))
        vh = v + (h / 2) * a
        u = u + h * v + (h * h / 2) * a
        an = mdl.acceleration(minv, scale(t) * f, u, vh)
        om = mdl.omega_eff(est, u, vh)
        v = v + (h / 2) * (a + an)
        a = an
        H.append(h), times.append(t), U.append(u), V.append(v)
    return np.array(H), np.array(times), np.array(U), np.array(V)


def scalar_alpha(alpha, v0, h, nsteps, dtype=np.longdouble):
    """a rigid translation under alpha: a' = -alpha (v + h/2 a), v' = v + h/2 (a + a'), u' = u + h v + h^2/2 a -> u, v, a"""
    alpha, h, v, u = dtype(alpha), dtype(h), dtype(v0), dtype(0)
    a = -alpha * v
    for _ in range(nsteps):
        u = u + h * v + (h * h / 2) * a
        an = -alpha * (v + (h / 2) * a)
        v = v + (h / 2) * (a + an)
        a = an
    return u, v, a
