"""Independent numpy statement of the C3D6 wedge, written from the definitions (femcy_amd.element_zoo is deliberately not
imported): N and dN in Abaqus node order, the 3 x 2 rule, K^e = sum_g B^T C B |J| w in the reference's Voigt order
[xx, yy, zz, xy, zx, yz], F and the Cauchy stresses of the oracle's laws, the nodal-force gather, the facet loads of
both face kinds, and an ElemDef so that the oracle's generic assembly can run on wedges."""
import numpy as np
import scipy.sparse as sp

from oracle import femcy_oracle as orc
from oracle.elements import ElemDef

NODES = np.array([[0., 0., -1.], [1., 0., -1.], [0., 1., -1.], [0., 0., 1.], [1., 0., 1.], [0., 1., 1.]])
_T = [(1. / 6., 1. / 6.), (2. / 3., 1. / 6.), (1. / 6., 2. / 3.)]
_Z = 1. / np.sqrt(3.)
GP = np.array([[a, b, z] for z in (-_Z, _Z) for a, b in _T])
GW = np.full(6, 1. / 6.)
# Abaqus faces S1..S5: node cycle (outward by the right-hand rule) and the natural coordinate constant on the face
FACES = [((0, 2, 1), "zeta-"), ((3, 4, 5), "zeta+"), ((0, 1, 4, 3), "eta0"), ((1, 2, 5, 4), "L0"), ((2, 0, 3, 5), "xi0")]


def N(p):
    xi, eta, z = p
    L = np.array([1. - xi - eta, xi, eta])
    return np.concatenate([L * (1. - z) / 2., L * (1. + z) / 2.])


def dN(p):
    xi, eta, z = p
    L = np.array([1. - xi - eta, xi, eta])
    out = np.zeros((6, 3))
    for a, (dx, de) in enumerate([(-1., -1.), (1., 0.), (0., 1.)]):
        out[a] = [dx * (1. - z) / 2., de * (1. - z) / 2., -L[a] / 2.]
        out[a + 3] = [dx * (1. + z) / 2., de * (1. + z) / 2., L[a] / 2.]
    return out


def dN_table():
    return np.stack([dN(g) for g in GP])


def face_param(face, s, t):
    """natural point of face `face` at in-face coordinates: triangles (s, t) on the unit triangle, quadrilaterals s in
    [0, 1] along the triangle edge and t = zeta."""
    kind = FACES[face][1]
    return {"zeta-": [s, t, -1.], "zeta+": [s, t, 1.], "eta0": [s, 0., t], "L0": [1. - s, s, t],
            "xi0": [0., 1. - s, t]}[kind]


_TANGENTS = {"zeta-": ([1., 0., 0.], [0., 1., 0.]), "zeta+": ([1., 0., 0.], [0., 1., 0.]),
             "eta0": ([1., 0., 0.], [0., 0., 1.]), "L0": ([-1., 1., 0.], [0., 0., 1.]), "xi0": ([0., -1., 0.], [0., 0., 1.])}


def face_points(face):
    """points and weights in the in-face parametrisation: 3-point triangle rule (weights 1/6, the parameter area
    1/2) or 2 x 2 Gauss on [0, 1] x [-1, 1] (weights 1/2)."""
    if face < 2:
        return [face_param(face, a, b) for a, b in _T], [1. / 6.] * 3
    g = [(1. - _Z) / 2., (1. + _Z) / 2.]
    return [face_param(face, s, z) for z in (-_Z, _Z) for s in g], [0.5] * 4


def C_iso(E, nu):
    return orc.Material("lin3d", (E, nu)).C


def C_neo(C1, D1):
    return orc.Material("neohooke", (C1, D1)).C


def B_matrix(g):
    B = np.zeros((6, 18))
    B[0, 0::3], B[1, 1::3], B[2, 2::3] = g[:, 0], g[:, 1], g[:, 2]
    B[3, 0::3], B[3, 1::3] = g[:, 1], g[:, 0]
    B[4, 0::3], B[4, 2::3] = g[:, 2], g[:, 0]
    B[5, 1::3], B[5, 2::3] = g[:, 2], g[:, 1]
    return B


def element_K(x, C):
    K = np.zeros((18, 18))
    for g, w in zip(GP, GW):
        d = dN(g)
        J = x.T @ d
        B = B_matrix(d @ np.linalg.inv(J))
        K += B.T @ C @ B * np.linalg.det(J) * w
    return K


def elem_def():
    """the wedge in the oracle's element vocabulary (its assembly, force and extrapolation are generic)."""
    keys = [tuple(sorted(f)) for f, _ in FACES]
    nat_n = {"zeta-": [0., 0., -1.], "zeta+": [0., 0., 1.], "eta0": [0., -1., 0.], "L0": [1., 1., 0.], "xi0": [-1., 0., 0.]}
    return ElemDef(name="C3D6", npe=6, dm=3, gauss_points=GP, gauss_weights=GW, N=N, dN=dN,
                   facet_natural_coos={k: face_points(i)[0] for i, k in enumerate(keys)},
                   facet_point_weights={k: ([1. / 3.] * 3 if i < 2 else [0.5] * 4) for i, k in enumerate(keys)},
                   facet_natural_normals={k: [nat_n[FACES[i][1]]] * (3 if i < 2 else 4) for i, k in enumerate(keys)},
                   inp_surface_num=[(k,) for k in keys],
                   extrap=np.linalg.inv(np.array([N(g) for g in GP])))


def assemble_K(nodes, el, C, u=None):
    u = np.zeros(nodes.size) if u is None else u
    x = nodes + u.reshape(-1, 3)
    n = nodes.size
    rows, cols, vals = [], [], []
    for e in el:
        Ke = element_K(x[e], C)
        gd = (e[:, None] * 3 + np.arange(3)[None, :]).ravel()
        rows.append(np.repeat(gd, 18))
        cols.append(np.tile(gd, 18))
        vals.append(Ke.ravel())
    return sp.coo_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(n, n)).tocsr()


def internal_force(nodes, el, u, mat):
    f = np.zeros(nodes.size)
    U = u.reshape(-1, 3)
    for e in el:
        X, Ue = nodes[e], U[e]
        for g, w in zip(GP, GW):
            d = dN(g)
            F = np.eye(3) + Ue.T @ (d @ np.linalg.inv(X.T @ d))
            sig = orc.cauchy_large(mat, F)
            J = (X + Ue).T @ d
            fe = (d @ np.linalg.inv(J)) @ sig * np.linalg.det(J) * w
            for a in range(6):
                f[e[a] * 3:e[a] * 3 + 3] += fe[a]
    return f


def facet_load(x, face, traction, direction=None):
    """consistent nodal load [nfn, 3] (rows in sorted local node order) of a traction on face `face` of one element:
    surface Jacobian |dx/ds x dx/dt| of the in-face parametrisation, normal oriented away from the element."""
    cyc = FACES[face][0]
    key = sorted(cyc)
    pts, wts = face_points(face)
    out = np.zeros((len(key), 3))
    centre = x.mean(axis=0)
    ds, dt = _TANGENTS[FACES[face][1]]          # d(natural point) / d(s, t): face_param is affine
    for p, w in zip(pts, wts):
        J = x.T @ dN(p)
        ts, tt = J @ np.asarray(ds), J @ np.asarray(dt)
        nvec = np.cross(ts, tt)
        da = np.linalg.norm(nvec)
        n = nvec / da
        if np.dot(n, x.T @ N(p) - centre) < 0:
            n = -n
        t = traction * (n if direction is None else np.asarray(direction, float))
        out += np.outer(N(p)[key], t) * da * w
    return out

