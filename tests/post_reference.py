"""numpy restatements, in the dtype the caller names (float64, or np.longdouble as the reference of tests/post_shapes.py), of
what has no such reference yet:

  neumann()      one loaded facet after the other as csrc/element_math.hpp states it (neumann_facet): the facet's size from its
                 first sorted local nodes (edge length, corner-triangle area) or, for a four-node facet in 3-D, the surface
                 Jacobian |det J| |n_nat J^-1| at every facet point; flux = traction x (direction or unit normal) x size x weight;
                 the load of facet node a is flux N_a.  Also the resultant, traction x the loaded area as a vector.
  gauss_F()      F = I + U^T (dN (X^T dN)^-1) at the Gauss points of the undeformed element
  small() / large_stress() / energy() / energy_small()
                 the infinitesimal strain, C : eps and its von Mises stress; the Cauchy stress F S F^T / J of the Green strain
                 (St. Venant-Kirchhoff; plane stress with the synthesised F33; compressible neo-Hookean, in 2-D at F33 = 1); the energy density of
                 the Green strain; sigma : eps / 2.

The tables are the plug-in's own `shapeFunc` / `dshape_dnat`; the small matrices are inverted by cofactors
(thermal_reference._det_inv) because numpy.linalg has no long-double path.  No library code runs here."""
import numpy as np

import loads_reference as lr
import thermal_reference as tr

LIN3D, PSTRAIN, PSTRESS, NEOHOOKE = 0, 1, 2, 3                       # the `kind` codes of femcy_set_material


# ------------------------------------------------------------------------------------------------ surface loads
def neumann(nodes, el, ELE, load_elem, load_ft, nfn, traction, direction, dtype):
    """-> (rhs [nn * dm], resultant [dm]); direction None: along the outward normal"""
    t = ELE.facet_tables(nfn)
    dm = nodes.shape[1]
    keys, nip = t["ft_nodes"][load_ft], t["nip"]                       # [nload, nfn] local nodes
    conn = el[load_elem]                                               # [nload, npe]
    X = np.asarray(nodes, dtype=dtype)[conn]                           # [nload, npe, dm]
    rows = np.arange(len(conn))[:, None]
    P = X[rows, keys]                                                  # [nload, nfn, dm]
    nanson = dm == 3 and t["nfn"] == 4
    if dm == 2:
        size = np.sqrt(((P[:, 0] - P[:, 1]) ** 2).sum(axis=1))
    else:
        c = np.cross(P[:, 1] - P[:, 0], P[:, 2] - P[:, 0])
        size = np.sqrt((c * c).sum(axis=1)) / 2
    d = None if direction is None else np.asarray(direction, dtype=dtype)[:dm]
    contrib = np.zeros((len(conn), t["nfn"], dm), dtype=dtype)
    total = np.zeros(dm, dtype=dtype)
    for ip in range(nip):
        dN = t["dN"][load_ft, ip].astype(dtype)                        # [nload, npe, dm]
        det, inv = tr._det_inv(np.einsum("lai,laj->lij", X, dN))
        v = np.einsum("li,lij->lj", t["normal"][load_ft, ip].astype(dtype), inv)
        nrm = np.sqrt((v * v).sum(axis=1))
        w = t["weight"][load_ft, ip].astype(dtype)
        area = np.abs(det) * nrm * w if nanson else size * w
        unit = v / (nrm + dtype(1.e-30))[:, None] if d is None else np.broadcast_to(d, v.shape)
        flux = dtype(traction) * unit * area[:, None]
        shape = t["N"][load_ft, ip].astype(dtype)[rows, keys]          # [nload, nfn]
        contrib += flux[:, None, :] * shape[:, :, None]
        total += flux.sum(axis=0)
    rhs = np.zeros(nodes.shape, dtype=dtype)
    np.add.at(rhs, conn[rows, keys], contrib)
    return rhs.ravel(), total


# ---------------------------------------------------------------------------------------------- post-processing
def gauss_F(nodes, el, ELE, u, dtype):
    """-> F [ne, nGP, dm, dm], det J w of the undeformed element [ne, nGP]"""
    _, dN, w = lr.element_tables(ELE)
    dN, w = dN.astype(dtype), w.astype(dtype)
    dm = nodes.shape[1]
    X = np.asarray(nodes, dtype=dtype)[el]
    U = np.asarray(u, dtype=dtype).reshape(-1, dm)[el]
    F = np.empty((len(el), len(w), dm, dm), dtype=dtype)
    vol = np.empty((len(el), len(w)), dtype=dtype)
    for g in range(len(w)):
        det, inv = tr._det_inv(np.einsum("eai,aj->eij", X, dN[g]))
        grad = np.einsum("ak,ekj->eaj", dN[g], inv)                    # dN_a / dX_j
        F[:, g] = np.einsum("eai,eaj->eij", U, grad) + np.eye(dm, dtype=dtype)
        vol[:, g] = det * w[g]
    return F, vol


def _sym3(v):
    """Voigt [xx, yy, zz, xy, zx, yz] -> tensor"""
    s = np.empty(v.shape[:-1] + (3, 3), dtype=v.dtype)
    for (i, j), k in {(0, 0): 0, (1, 1): 1, (2, 2): 2, (0, 1): 3, (0, 2): 4, (1, 2): 5}.items():
        s[..., i, j] = s[..., j, i] = v[..., k]
    return s


def _hooke(eps, C, dtype):
    """C : eps for a symmetric eps [..., dm, dm] with the engineering shears of femcy_set_material's Voigt order"""
    C = np.asarray(C, dtype=dtype)
    if eps.shape[-1] == 3:
        ev = np.stack([eps[..., 0, 0], eps[..., 1, 1], eps[..., 2, 2], 2 * eps[..., 0, 1], 2 * eps[..., 0, 2], 2 * eps[..., 1, 2]], axis=-1)
        return _sym3(ev @ C.T)
    v = np.stack([eps[..., 0, 0], eps[..., 1, 1], 2 * eps[..., 0, 1]], axis=-1) @ C.T
    s = np.empty_like(eps)
    s[..., 0, 0], s[..., 1, 1] = v[..., 0], v[..., 1]
    s[..., 0, 1] = s[..., 1, 0] = v[..., 2]
    return s


def _embed(F, kind, params, C, dtype):
    """-> F3 [..., 3, 3] and the 6 x 6 matrix the Green strain of F3 is taken through"""
    if F.shape[-1] == 3:
        return F, np.asarray(C, dtype=dtype)
    C = np.asarray(C, dtype=dtype)
    F3 = np.zeros(F.shape[:-2] + (3, 3), dtype=dtype)
    F3[..., :2, :2] = F
    C6 = np.zeros((6, 6), dtype=dtype)
    C6[:2, :2], C6[3, 3] = C[:2, :2], C[2, 2]
    if kind == PSTRESS:
        nu = dtype(params[1])
        F3[..., 2, 2] = -nu / (1 - nu) * (F[..., 0, 0] + F[..., 1, 1] - 2) + 1
    else:
        F3[..., 2, 2] = 1
        C6[0, 2] = C6[2, 0] = C6[1, 2] = C6[2, 1] = C[0, 1]
    return F3, C6


def _det3(A):
    return (A[..., 0, 0] * (A[..., 1, 1] * A[..., 2, 2] - A[..., 1, 2] * A[..., 2, 1])
            - A[..., 0, 1] * (A[..., 1, 0] * A[..., 2, 2] - A[..., 1, 2] * A[..., 2, 0])
            + A[..., 0, 2] * (A[..., 1, 0] * A[..., 2, 1] - A[..., 1, 1] * A[..., 2, 0]))


def _neo_F3(F, dtype):
    if F.shape[-1] == 3:
        return F
    F3 = np.zeros(F.shape[:-2] + (3, 3), dtype=dtype)
    F3[..., :2, :2] = F
    F3[..., 2, 2] = 1
    return F3


def _green(F3):
    return (np.swapaxes(F3, -1, -2) @ F3 - np.eye(3, dtype=F3.dtype)) / 2


def _mises(sig, kind, params, dtype, szz=0):
    """von Mises stress by material type: sigma_zz = nu (s_xx + s_yy) in plane strain, 0 in plane stress, `szz` as given for the
    plane-strain neo-Hookean solid"""
    if kind == PSTRAIN:
        return tr.mises(sig, tr.PSTRAIN, params[1], 0, dtype)
    return tr.mises(sig, tr.PSTRAIN if sig.shape[-1] == 2 and kind == NEOHOOKE else None, 0.0, szz, dtype)


def small(F, kind, params, C, dtype):
    """linear kinds -> (infinitesimal strain, C : eps, von Mises)"""
    assert kind != NEOHOOKE
    eps = (F + np.swapaxes(F, -1, -2)) / 2 - np.eye(F.shape[-1], dtype=dtype)
    sig = _hooke(eps, C, dtype)
    return eps, sig, _mises(sig, kind, params, dtype)


def large_stress(F, kind, params, C, dtype):
    """-> (Green strain [..., dm, dm], Cauchy stress, von Mises)"""
    dm = F.shape[-1]
    green = (np.swapaxes(F, -1, -2) @ F - np.eye(dm, dtype=dtype)) / 2
    if kind == NEOHOOKE:                                               # 2-D: plane strain, the 3-D expression at F33 = 1
        C1, D1 = dtype(params[0]), dtype(params[1])
        F3 = _neo_F3(F, dtype)
        J = _det3(F3)[..., None, None]
        I = np.eye(3, dtype=dtype)
        s3 = 2 * C1 / J * (F3 @ np.swapaxes(F3, -1, -2) - I) + 2 * D1 * (J - 1) * I
        return green, s3[..., :dm, :dm], _mises(s3[..., :dm, :dm], kind, params, dtype, s3[..., 2, 2])
    elif kind == PSTRAIN:
        pk2 = _hooke(green, C, dtype)
        sig = F @ pk2 @ np.swapaxes(F, -1, -2) / (F[..., 0, 0] * F[..., 1, 1] - F[..., 0, 1] * F[..., 1, 0])[..., None, None]
    else:
        F3, C6 = _embed(F, kind, params, C, dtype)
        pk2 = _hooke(_green(F3), C6, dtype)
        sig = (F3 @ pk2 @ np.swapaxes(F3, -1, -2) / _det3(F3)[..., None, None])[..., :dm, :dm]
    return green, sig, _mises(sig, kind, params, dtype)


def energy(F, kind, params, C, dtype):
    """the energy density of the Green strain (neo-Hookean: C1 (I1 - 3 - 2 ln J) + D1 (J - 1)^2)"""
    if kind == NEOHOOKE:
        F3 = _neo_F3(F, dtype)
        J = _det3(F3)
        return dtype(params[0]) * ((F3 * F3).sum(axis=(-1, -2)) - 3 - 2 * np.log(J)) + dtype(params[1]) * (J - 1) ** 2
    F3, C6 = _embed(F, kind, params, C, dtype)
    E = _green(F3)
    return (_hooke(E, C6, dtype) * E).sum(axis=(-1, -2)) / 2


def energy_small(F, kind, params, C, dtype):
    eps, sig, _ = small(F, kind, params, C, dtype)
    return (sig * eps).sum(axis=(-1, -2)) / 2
