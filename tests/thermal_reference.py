"""numpy restatement of the thermal load (femcy_thermal_*), written from the formulas

    dT_g = sum_a N_a(xi_g) dT_a,      sigma_th = alpha dT_g  C : (k I)
    f[a][i] = sum_e sum_g sum_j dN_a/dx_j sigma_th[i][j] |det J_g| w_g,      J_g = X_e^T dN(xi_g)   (undeformed)
    sigma = sigma_0 - scale sigma_th,   von Mises of sigma (plane strain: sigma_zz = nu (s_xx + s_yy) - E alpha dT_g scale)

as array expressions over the plug-in's own `shapeFunc` / `dshape_dnat` at its Gauss points, in the dtype the caller
names: float64, or np.longdouble as the reference of the bounds (tests/thermal_cases.py).  No library code runs here;
the small matrices are inverted by cofactors because numpy.linalg has no long-double path."""
import numpy as np

import loads_reference as lr

LIN3D, PSTRAIN, PSTRESS = "lin3d", "pstrain", "pstress"


def unit_stress(C, kind, nu, dtype):
    """stress of full restraint at alpha dT = 1 as a dm x dm tensor; C is what femcy_set_material receives (Voigt order
    [xx, yy, zz, xy, zx, yz] or [xx, yy, xy])"""
    C = np.asarray(C, dtype=dtype)
    if kind == LIN3D:
        v = C[:, 0] + C[:, 1] + C[:, 2]
        return np.array([[v[0], v[3], v[4]], [v[3], v[1], v[5]], [v[4], v[5], v[2]]], dtype=dtype)
    k = dtype(1) + dtype(nu) if kind == PSTRAIN else dtype(1)
    v = k * (C[:, 0] + C[:, 1])
    return np.array([[v[0], v[2]], [v[2], v[1]]], dtype=dtype)


def _det_inv(J):
    """J [ne, dm, dm] -> det [ne], inverse [ne, dm, dm], by cofactors"""
    if J.shape[1] == 2:
        det = J[:, 0, 0] * J[:, 1, 1] - J[:, 0, 1] * J[:, 1, 0]
        inv = np.empty_like(J)
        inv[:, 0, 0], inv[:, 0, 1], inv[:, 1, 0], inv[:, 1, 1] = J[:, 1, 1], -J[:, 0, 1], -J[:, 1, 0], J[:, 0, 0]
        return det, inv / det[:, None, None]
    r0, r1, r2 = J[:, 0], J[:, 1], J[:, 2]
    c0, c1, c2 = np.cross(r1, r2), np.cross(r2, r0), np.cross(r0, r1)
    det = (r0 * c0).sum(axis=1)
    return det, np.stack([c0, c1, c2], axis=2) / det[:, None, None]


def gauss_dT(el, ELE, dT, dtype):
    """dT at the Gauss points [ne, nGP]"""
    N = lr.element_tables(ELE)[0].astype(dtype)
    return np.einsum("ga,ea->eg", N, np.asarray(dT, dtype=dtype)[el])


def thermal_force(nodes, el, ELE, C, kind, nu, alpha, dT, dtype=np.float64):
    """the load vector at scale 1, [nn * dm]"""
    _, dN, w = lr.element_tables(ELE)
    dN, w = dN.astype(dtype), w.astype(dtype)
    X = np.asarray(nodes, dtype=dtype)[el]                                   # [ne, npe, dm]
    S = unit_stress(C, kind, nu, dtype) * dtype(alpha)
    tg = gauss_dT(el, ELE, dT, dtype)
    f = np.zeros(nodes.shape, dtype=dtype)
    for g in range(len(w)):
        det, inv = _det_inv(np.einsum("eai,aj->eij", X, dN[g]))
        grad = np.einsum("ak,ekj->eaj", dN[g], inv)                          # dN_a / dx_j
        fe = np.einsum("eaj,ij->eai", grad, S) * (np.abs(det) * w[g] * tg[:, g])[:, None, None]
        np.add.at(f, el, fe)
    return f.ravel()


def mises(sig, kind, nu, szz_extra, dtype):
    """sig [..., dm, dm] -> von Mises; plane strain: sigma_zz = nu (s_xx + s_yy) + szz_extra, plane stress: 0"""
    s3 = np.zeros(sig.shape[:-2] + (3, 3), dtype=dtype)
    dm = sig.shape[-1]
    s3[..., :dm, :dm] = sig
    if kind == PSTRAIN:
        s3[..., 2, 2] = dtype(nu) * (sig[..., 0, 0] + sig[..., 1, 1]) + szz_extra
    tr = (s3[..., 0, 0] + s3[..., 1, 1] + s3[..., 2, 2]) / dtype(3)
    dev = s3 - tr[..., None, None] * np.eye(3, dtype=dtype)
    return np.sqrt(dtype(1.5) * (dev * dev).sum(axis=(-1, -2)))


def corrected_stress(el, ELE, C, kind, nu, alpha, dT, scale, sigma0, dtype=np.float64):
    """sigma0 [ne, nGP, dm, dm] (C : eps(u), as femcy_compute_strain_stress leaves it) -> corrected sigma and von Mises"""
    S = unit_stress(C, kind, nu, dtype) * dtype(alpha)
    th = dtype(scale) * gauss_dT(el, ELE, dT, dtype)                         # [ne, nGP]
    sig = np.asarray(sigma0, dtype=dtype) - th[..., None, None] * S
    extra = -(dtype(1) - dtype(2) * dtype(nu)) * th * S[0, 0] if kind == PSTRAIN else 0   # - E alpha dT_g scale
    return sig, mises(sig, kind, nu, extra, dtype)


def smooth_dT(nodes):
    """a smooth, non-polynomial temperature change (coordinates scaled to a box of edge 3)"""
    q = 3.0 * nodes / np.abs(nodes).max(axis=0)
    x, y = q[:, 0], q[:, 1]
    z = q[:, 2] if nodes.shape[1] == 3 else 0.0 * x
    return 40.0 * np.sin(1.3 * x + 0.4) * np.cos(0.9 * y - 0.2) + 25.0 * np.exp(-0.5 * (x - 1.0) ** 2) + 7.0 * np.sin(2.1 * z)

