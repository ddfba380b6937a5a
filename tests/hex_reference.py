"""Independent numpy statement of the C3D8 hexahedron, written from the definitions (the oracle has no hexahedron and
femcy_amd.element_zoo is deliberately not imported): trilinear N and dN in Abaqus node order, the 2 x 2 x 2 Gauss rule,
K^e = sum_g B^T C B |J| w in the reference's Voigt order [xx, yy, zz, xy, zx, yz], F and the Cauchy stresses of the
oracle's laws, the nodal-force gather, and an ElemDef so that the oracle's generic assembly can run on hexahedra."""
import numpy as np
import scipy.sparse as sp

from oracle import femcy_oracle as orc
from oracle.elements import ElemDef

CORNERS = np.array([[-1., -1., -1.], [1., -1., -1.], [1., 1., -1.], [-1., 1., -1.],
                    [-1., -1., 1.], [1., -1., 1.], [1., 1., 1.], [-1., 1., 1.]])
GP = CORNERS / np.sqrt(3.)
GW = np.ones(8)
# Abaqus faces S1..S6: sorted local nodes, the fixed natural axis and its value
FACES = [((0, 1, 2, 3), 2, -1.), ((4, 5, 6, 7), 2, 1.), ((0, 1, 4, 5), 1, -1.),
         ((1, 2, 5, 6), 0, 1.), ((2, 3, 6, 7), 1, 1.), ((0, 3, 4, 7), 0, -1.)]


def N(xi):
    xi = np.asarray(xi, float)
    return np.prod(1. + CORNERS * xi[None, :], axis=1) / 8.


def dN(xi):
    xi = np.asarray(xi, float)
    f = 1. + CORNERS * xi[None, :]
    out = np.empty((8, 3))
    for k in range(3):
        others = [j for j in range(3) if j != k]
        out[:, k] = CORNERS[:, k] * f[:, others[0]] * f[:, others[1]] / 8.
    return out


def dN_table():
    return np.stack([dN(g) for g in GP])


def face_points(face):
    _, ax, side = FACES[face]
    g = 1. / np.sqrt(3.)
    pts = []
    for a in (-g, g):
        for b in (-g, g):
            p = [a, b]
            p.insert(ax, side)
            pts.append(p)
    return np.array(pts)


def C_iso(E, nu):
    return orc.Material("lin3d", (E, nu)).C


def C_neo(C1, D1):
    return orc.Material("neohooke", (C1, D1)).C


def B_matrix(g):
    """g [8, 3] = grad N -> B [6, 24], engineering shear in the order xx, yy, zz, xy, zx, yz."""
    B = np.zeros((6, 24))
    B[0, 0::3], B[1, 1::3], B[2, 2::3] = g[:, 0], g[:, 1], g[:, 2]
    B[3, 0::3], B[3, 1::3] = g[:, 1], g[:, 0]
    B[4, 0::3], B[4, 2::3] = g[:, 2], g[:, 0]
    B[5, 1::3], B[5, 2::3] = g[:, 2], g[:, 1]
    return B


def element_K(x, C):
    """K^e [24, 24] at nodal positions x [8, 3]."""
    K = np.zeros((24, 24))
    for g, w in zip(GP, GW):
        d = dN(g)
        J = x.T @ d
        grad = d @ np.linalg.inv(J)
        B = B_matrix(grad)
        K += B.T @ C @ B * np.linalg.det(J) * w
    return K


def elem_def():
    """the hexahedron in the oracle's element vocabulary (its assembly, force and extrapolation are generic)."""
    keys = [f for f, _, _ in FACES]
    return ElemDef(name="C3D8", npe=8, dm=3, gauss_points=GP, gauss_weights=GW, N=N, dN=dN,
                   facet_natural_coos={f: face_points(i).tolist() for i, f in enumerate(keys)},
                   facet_point_weights={f: [1.] * 4 for f in keys},
                   facet_natural_normals={f: [[s if k == ax else 0. for k in range(3)]] * 4 for f, ax, s in FACES},
                   inp_surface_num=[(f,) for f in keys],
                   extrap=np.array([N(c * np.sqrt(3.)) for c in CORNERS]))


def assemble_K(nodes, el, C, u=None):
    """global K (CSR, n x n) from element_K at x = X + u."""
    u = np.zeros(nodes.size) if u is None else u
    x = nodes + u.reshape(-1, 3)
    n = nodes.size
    rows, cols, vals = [], [], []
    for e in el:
        Ke = element_K(x[e], C)
        gd = (e[:, None] * 3 + np.arange(3)[None, :]).ravel()
        rows.append(np.repeat(gd, 24))
        cols.append(np.tile(gd, 24))
        vals.append(Ke.ravel())
    return sp.coo_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(n, n)).tocsr()


def internal_force(nodes, el, u, mat):
    """f = sum_e sum_g grad N (current) . sigma(F) |J| w, F from the reference configuration."""
    f = np.zeros(nodes.size)
    U = u.reshape(-1, 3)
    for e in el:
        X, Ue = nodes[e], U[e]
        for g, w in zip(GP, GW):
            d = dN(g)
            F = np.eye(3) + Ue.T @ (d @ np.linalg.inv(X.T @ d))
            sig = orc.cauchy_large(mat, F)
            J = (X + Ue).T @ d
            grad = d @ np.linalg.inv(J)
            fe = grad @ sig * np.linalg.det(J) * w
            for a in range(8):
                f[e[a] * 3:e[a] * 3 + 3] += fe[a]
    return f


def facet_load(x, face, traction, direction=None):
    """consistent nodal load [4, 3] of a traction on face `face` of one element (x [8, 3]): 2 x 2 Gauss points of the
    face, surface Jacobian |dx/da x dx/db| from the two in-face natural tangents."""
    key, ax, side = FACES[face]
    inplane = [k for k in range(3) if k != ax]
    out = np.zeros((4, 3))
    for p in face_points(face):
        d = dN(p)
        J = x.T @ d                               # columns dx/dxi_k
        nvec = np.cross(J[:, inplane[0]], J[:, inplane[1]])
        da = np.linalg.norm(nvec)
        n = nvec / da
        if np.dot(n, J[:, ax]) * side < 0:
            n = -n
        t = traction * (n if direction is None else np.asarray(direction, float))
        out += np.outer(N(p)[list(key)], t) * da
    return out
