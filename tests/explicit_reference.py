"""numpy restatement of explicit dynamics (femcy_lumped_mass_*, femcy_explicit_*), in any dtype (np.longdouble: the reference;
np.float64: what its rounding alone is worth), written from the formulas

    m_e = sum_q rho |det J_q| w_q,   d_a = sum_q N_a(xi_q)^2 rho |det J_q| w_q,   m_a^e = d_a m_e / sum_b d_b      (HRZ lumping)
    f_int[a] = sum_e sum_g grad_x N_a . sigma(F_g) det J_g(x) w_g,   F = I + sum_a u_a (x) grad_X N_a
    a_0 = minv (s_0 f - f_int(u_0));  u_{n+1} = u_n + h v_n + h^2 / 2 a_n;  a_{n+1} = minv (s_{n+1} f - f_int(u_{n+1}));
    v_{n+1} = v_n + h / 2 (a_n + a_{n+1})
    energy = sum_g W(F_g) det J_g(x) w_g   (the reference's get_elasEng: the weights of the CURRENT configuration)
    omega^2 <= max_i minv_i sum_j |K_ij|   (Gershgorin)

with the plug-in's own tables and the four stress laws of the reference's constitutiveOfLargeDeform.  Vectorised over the
elements.  No library code runs here."""
import numpy as np

LIN3D, PSTRAIN, PSTRESS, NEOHOOKE = 0, 1, 2, 3


def _det(J):
    if J.shape[-1] == 2:
        return J[..., 0, 0] * J[..., 1, 1] - J[..., 0, 1] * J[..., 1, 0]
    return (J[..., 0, 0] * (J[..., 1, 1] * J[..., 2, 2] - J[..., 1, 2] * J[..., 2, 1])
            - J[..., 0, 1] * (J[..., 1, 0] * J[..., 2, 2] - J[..., 1, 2] * J[..., 2, 0])
            + J[..., 0, 2] * (J[..., 1, 0] * J[..., 2, 1] - J[..., 1, 1] * J[..., 2, 0]))


def _inv(J):
    d = _det(J)
    out = np.empty_like(J)
    if J.shape[-1] == 2:
        out[..., 0, 0], out[..., 0, 1], out[..., 1, 0], out[..., 1, 1] = J[..., 1, 1], -J[..., 0, 1], -J[..., 1, 0], J[..., 0, 0]
    else:
        for i in range(3):
            for j in range(3):
                a, b = [k for k in range(3) if k != i], [k for k in range(3) if k != j]
                out[..., j, i] = (-1) ** (i + j) * (J[..., a[0], b[0]] * J[..., a[1], b[1]] - J[..., a[0], b[1]] * J[..., a[1], b[0]])
    return out / d[..., None, None]


def gauss_tables(ELE, dtype):
    gp = np.asarray(ELE.gaussPoints, dtype=np.float64)
    dN = np.array([ELE.dshape_dnat(p) for p in gp], dtype=dtype)      # [nGP, npe, dm]
    return dN, np.asarray(ELE.gaussWeights, dtype=dtype)


def mass_tables(ELE, dtype):
    pts, w = ELE.mass_rule()
    N = np.array([ELE.shapeFunc(p) for p in pts], dtype=dtype)
    dN = np.array([ELE.dshape_dnat(p) for p in pts], dtype=dtype)
    return N, dN, np.asarray(w, dtype=dtype)


def lumped_mass(nodes, el, ELE, rho, dtype):
    """[nn] nodal masses by HRZ lumping over the plug-in's mass rule"""
    N, dN, w = mass_tables(ELE, dtype)
    X = np.asarray(nodes, dtype=dtype)[el]                            # [ne, npe, dm]
    vq = dtype(rho) * (np.abs(_det(np.einsum("eai,qaj->eqij", X, dN))) * w[None, :])      # [ne, nq]
    me, d = vq.sum(axis=1), np.einsum("qa,eq->ea", N * N, vq)
    m = np.zeros(len(nodes), dtype=dtype)
    np.add.at(m, el, d * me[:, None] / d.sum(axis=1)[:, None])
    return m


def mesh_volume(nodes, el, ELE, dtype=np.longdouble):
    _, dN, w = mass_tables(ELE, dtype)
    X = np.asarray(nodes, dtype=dtype)[el]
    return (np.abs(_det(np.einsum("eai,qaj->eqij", X, dN))) * w[None, :]).sum()


def _green3(F3):
    E = (np.einsum("...ki,...kj->...ij", F3, F3) - np.eye(3, dtype=F3.dtype)) / 2
    return np.stack([E[..., 0, 0], E[..., 1, 1], E[..., 2, 2], 2 * E[..., 0, 1], 2 * E[..., 2, 0], 2 * E[..., 1, 2]], axis=-1)


def _push3(F3, sv):
    S = np.empty(F3.shape, dtype=F3.dtype)
    for (i, j), k in {(0, 0): 0, (1, 1): 1, (2, 2): 2, (0, 1): 3, (0, 2): 4, (1, 2): 5}.items():
        S[..., i, j] = S[..., j, i] = sv[..., k]
    return np.einsum("...ik,...kl,...jl->...ij", F3, S, F3) / _det(F3)[..., None, None]


def _embed(F, kind, nu):
    """the 3 x 3 deformation gradient of a 2-D one: F33 = 1, or the plane-stress thickness stretch of the reference"""
    F3 = np.zeros(F.shape[:-2] + (3, 3), dtype=F.dtype)
    F3[..., :2, :2] = F
    F3[..., 2, 2] = (-nu / (1 - nu) * (F[..., 0, 0] + F[..., 1, 1] - 2) + 1) if kind == PSTRESS else 1
    return F3


def _c6(kind, C, params, dtype):
    C = np.asarray(C, dtype=dtype)
    if kind == LIN3D:
        return C
    C6 = np.zeros((6, 6), dtype=dtype)
    if kind == PSTRESS:
        E, nu = dtype(params[0]), dtype(params[1])
        c00 = E / (1 - nu * nu)
        C6[0, 0] = C6[1, 1] = c00
        C6[0, 1] = C6[1, 0] = c00 * nu
        C6[3, 3] = E / 2 / (1 + nu)
    else:
        C6[0, 0] = C6[1, 1] = C[0, 0]
        C6[0, 1] = C6[1, 0] = C6[0, 2] = C6[2, 0] = C6[1, 2] = C6[2, 1] = C[0, 1]
        C6[3, 3] = C[2, 2]
    return C6


def cauchy(F, kind, C, params, dtype):
    """Cauchy stress [..., dm, dm] of constitutiveOfLargeDeform for F [..., dm, dm]"""
    dm = F.shape[-1]
    p0, p1 = dtype(params[0]), dtype(params[1])
    eye = np.eye(dm, dtype=dtype)
    if kind == NEOHOOKE:
        J = _det(F)[..., None, None]
        return 2 * p0 / J * (np.einsum("...ik,...jk->...ij", F, F) - eye) + 2 * p1 * (J - 1) * eye
    if kind == LIN3D:
        return _push3(F, np.einsum("pq,...q->...p", np.asarray(C, dtype=dtype), _green3(F)))
    if kind == PSTRESS:
        F3 = _embed(F, kind, p1)
        sv = np.einsum("pq,...q->...p", _c6(kind, C, params, dtype), _green3(F3))
        sv[..., 2] = 0
        return _push3(F3, sv)[..., :2, :2]
    C3 = np.asarray(C, dtype=dtype)                                   # plane strain: in the plane throughout
    E2 = (np.einsum("...ki,...kj->...ij", F, F) - eye) / 2
    sv = np.einsum("pq,...q->...p", C3, np.stack([E2[..., 0, 0], E2[..., 1, 1], 2 * E2[..., 0, 1]], axis=-1))
    S = np.empty(F.shape, dtype=dtype)
    S[..., 0, 0], S[..., 1, 1] = sv[..., 0], sv[..., 1]
    S[..., 0, 1] = S[..., 1, 0] = sv[..., 2]
    return np.einsum("...ik,...kl,...jl->...ij", F, S, F) / _det(F)[..., None, None]


class Model:
    """mesh + material in one dtype: internal force, energy, the velocity-Verlet recurrence"""

    def __init__(self, nodes, el, ELE, material, dtype):
        self.dtype, self.el, self.nn, self.dm = dtype, np.asarray(el), len(nodes), int(ELE.dm)
        self.kind, self.C, self.params = int(material.kind), np.asarray(material.C), np.asarray(material.params, dtype=np.float64)
        self.dN, self.w = gauss_tables(ELE, dtype)
        self.X = np.asarray(nodes, dtype=dtype)[self.el]
        self.gX = np.einsum("gak,egkj->egaj", self.dN, _inv(np.einsum("eai,gaj->egij", self.X, self.dN)))   # grad_X N

    def _state(self, u):
        U = np.asarray(u, dtype=self.dtype).reshape(self.nn, self.dm)[self.el]
        J = np.einsum("eai,gaj->egij", self.X + U, self.dN)
        F = np.eye(self.dm, dtype=self.dtype) + np.einsum("eai,egaj->egij", U, self.gX)
        return J, F

    def f_int(self, u):
        J, F = self._state(u)
        gx = np.einsum("gak,egkj->egaj", self.dN, _inv(J))
        sig = cauchy(F, self.kind, self.C, self.params, self.dtype)
        fe = np.einsum("egaj,egji,eg->eai", gx, sig, _det(J) * self.w[None, :])
        f = np.zeros((self.nn, self.dm), dtype=self.dtype)
        np.add.at(f, self.el, fe)
        return f.ravel()

    def energy(self, u):
        """the reference's get_elasEng at u: the density of the Green strain (or the neo-Hookean one) times the weights of
        the configuration u"""
        J, F = self._state(u)
        F3 = F if self.dm == 3 else _embed(F, self.kind, self.dtype(self.params[1]))
        if self.kind == NEOHOOKE:
            J3 = _det(F3)
            W = self.dtype(self.params[0]) * ((F3 * F3).sum(axis=(-1, -2)) - 3 - 2 * np.log(J3)) + self.dtype(self.params[1]) * (J3 - 1) ** 2
        else:
            ev = _green3(F3)
            W = np.einsum("...p,pq,...q->...", ev, _c6(self.kind, self.C, self.params, self.dtype), ev) / 2
        return (W * _det(J) * self.w[None, :]).sum()

    def verlet(self, minv, f, v0, h, nsteps, scale):
        """-> U, V, A [nsteps + 1, n]; scale(k) = the load scale of state k"""
        dt = self.dtype
        minv, f, h = np.asarray(minv, dtype=dt), np.asarray(f, dtype=dt), dt(h)
        u, v = np.zeros(self.nn * self.dm, dtype=dt), np.asarray(v0, dtype=dt) * (minv != 0)
        a = minv * (dt(scale(0)) * f - self.f_int(u))
        U, V, A = [u], [v], [a]
        for k in range(1, nsteps + 1):
            u = u + h * v + (h * h / 2) * a
            an = minv * (dt(scale(k)) * f - self.f_int(u))
            v = v + (h / 2) * (a + an)
            a = an
            U.append(u), V.append(v), A.append(a)
        return np.array(U), np.array(V), np.array(A)


def kinetic(m, v, dm, dtype):
    v = np.asarray(v, dtype=dtype).reshape(-1, dm)
    return (np.asarray(m, dtype=dtype) * (v * v).sum(axis=1)).sum() / 2


def gershgorin(K, minv):
    """omega bound: sqrt(max over the rows with minv != 0 of minv_i sum_j |K_ij|); K dense"""
    rows = np.abs(np.asarray(K, dtype=np.longdouble)).sum(axis=1) * np.asarray(minv, dtype=np.longdouble)
    return float(np.sqrt(rows[np.asarray(minv) != 0].max()))
