"""Restatement of the frictionless rigid walls of explicit dynamics (include/femcy.h at femcy_explicit_set_wall) in numpy, in
any dtype, on top of explicit_damped_reference.DampedModel; no library code runs here.  A wall is (point, normal, kappa); the
normal is normalised here as the library does it, in the model's dtype.

`exact_*` restate the float64 arithmetic of the law bit for bit (fused multiply-adds through exact rationals), for the one
state where the rest of the acceleration is exactly 0."""
from fractions import Fraction

import numpy as np

import explicit_damped_reference as edr

LD = np.longdouble


class WallModel(edr.DampedModel):
    def __init__(self, nodes, el, ELE, material, dtype, rho0, walls, alpha=0.0, b1=0.0, b2=0.0, Md=0.0, mesh_size=None):
        super().__init__(nodes, el, ELE, material, dtype, rho0, alpha, b1, b2, Md)
        self.X0 = np.asarray(nodes, dtype=dtype)
        self.walls = []
        for p, n, kappa in walls:
            n = np.asarray(n, dtype=dtype)
            n = n / np.sqrt((n * n).sum())
            self.walls.append((n, (n * np.asarray(p, dtype=dtype)).sum(), dtype(kappa)))
        self.kappa = sum(w[2] for w in self.walls)
        self.size = float(np.ptp(np.asarray(nodes, dtype=np.float64), axis=0).max()) if mesh_size is None else mesh_size
        self.counts = []            # per acceleration call: the number of nodes inside each wall

    def gaps(self, u):
        """-> g [walls, nn]"""
        x = self.X0 + np.asarray(u, dtype=self.dtype).reshape(self.X0.shape)
        return np.array([x @ n - d for n, d, _ in self.walls], dtype=self.dtype).reshape(len(self.walls), -1)

    def wall_acceleration(self, minv, u):
        g = self.gaps(u)
        # the contact count is not continuous in g: every case keeps |g| away from 0 where it is compared
        assert (np.abs(g) > 1e-9 * self.size).all(), "a node sits on a wall: the contact count is not defined"
        self.counts.append((g < 0).sum(axis=1))
        a = np.zeros(self.X0.shape, dtype=self.dtype)
        for (n, _, kappa), gw in zip(self.walls, g):
            a = a + (-kappa * np.minimum(gw, 0))[:, None] * n[None, :]
        return a.ravel() * (minv != 0)

    def acceleration(self, minv, sf, u, vhalf):
        """minv (s f - f_int - f_bv) + the walls - alpha v_{n+1/2}"""
        a = minv * (sf - self.f_int(u) - (self.f_bv(u, vhalf) if (self.b1 != 0 or self.b2 != 0) else 0))
        return a + self.wall_acceleration(minv, u) - self.alpha * vhalf * (minv != 0)

    def omega_eff(self, est, u, vhalf):
        """max_e omega_eff,e with kappa added to omega_e^2 before the damping factor"""
        om = np.sqrt(est.elements(u)[1] + self.kappa)
        xi = self.b1 + (self.alpha / (2 * om) if self.alpha != 0 else 0)
        if self.b2 != 0:
            _, _, rate, L, rho = self.points(u, vhalf)
            xi = xi + self.b2 ** 2 * (L * np.sqrt(rho / self.Md) * np.maximum(0, -rate)).max(axis=1)
        return (om * (np.sqrt(1 + xi * xi) + xi)).max()

    def wall_get(self, k, u, m, minv):
        """-> force, E_w, count, penetration of wall k, in the model's dtype"""
        dt = self.dtype
        g = self.gaps(u)[k]
        p = np.maximum(-g, 0)
        free = (np.asarray(minv).reshape(self.X0.shape) != 0).any(axis=1)
        km = self.walls[k][2] * np.asarray(m, dtype=dt) * free
        return np.array([(km * p).sum(), (km * p * p).sum() / 2, dt((g < 0).sum()), p.max()], dtype=dt)


# ------------------------------------------------------------------------------------------- bit for bit
def fma(a, b, c):
    return float(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)))


def exact_wall(point, normal):
    """-> the unit normal and d as the library forms them in float64"""
    len2 = 0.0
    for nj in normal:
        len2 = fma(nj, nj, len2)
    n = [float(np.float64(nj) / np.sqrt(np.float64(len2))) for nj in normal]
    d = 0.0
    for nj, pj in zip(n, point):
        d = fma(nj, pj, d)
    return n, d


def exact_gap(n, d, x):
    g = fma(n[0], x[0], -d)
    for j in range(1, len(x)):
        g = fma(n[j], x[j], g)
    return g


def exact_a0(nodes, walls, minv):
    """a_0 of a mesh at u = 0 under no load with a linear material -- f_int = 0 --: the wall term alone, in float64 bits"""
    nodes = np.asarray(nodes, dtype=np.float64)
    a = np.zeros(nodes.shape)
    ws = [exact_wall(p, n) + (float(k),) for p, n, k in walls]
    for i, x in enumerate(nodes):
        for c in range(nodes.shape[1]):
            ai = 0.0
            for n, d, kappa in ws:
                g = exact_gap(n, d, x)
                if g < 0.0:
                    ai = fma(-kappa * g, n[c], ai)
            a[i, c] = ai
    return np.where(np.asarray(minv) != 0, a.ravel(), 0.0)
