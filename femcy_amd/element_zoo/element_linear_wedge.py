"""C3D6 linear wedge (6-node prism).  Abaqus node order: nodes 0-2 are the triangle zeta = -1, nodes 3-5 the triangle
zeta = +1, node k + 3 above node k.  Natural coordinates (xi, eta) on the unit triangle and zeta in [-1, 1]:
N_a = L_a (1 - zeta) / 2, N_(a+3) = L_a (1 + zeta) / 2 with L = (1 - xi - eta, xi, eta).

Integration (this code's choice): the 3-point triangle rule (1/6, 1/6), (2/3, 1/6), (1/6, 2/3),
weight 1/6 each, times the 2-point Gauss rule in zeta (-+1/sqrt 3, weight 1): six points whose weights sum to 1, the
volume of the reference prism.  It integrates the stiffness of a prism with parallel triangular faces exactly.  The
reference has no wedge; the faces follow Abaqus' S1..S5 numbering."""
import numpy as np
from .element_base import ElementBase

_G = 1. / 3. ** 0.5
_TRI = [(1. / 6., 1. / 6.), (2. / 3., 1. / 6.), (1. / 6., 2. / 3.)]
_NODES = np.array([[0., 0., -1.], [1., 0., -1.], [0., 1., -1.], [0., 0., 1.], [1., 0., 1.], [0., 1., 1.]])
_S = [(1. - _G) / 2., (1. + _G) / 2.]                   # 2-point Gauss rule on [0, 1] (weight 1/2 each)
# Abaqus faces S1..S5 as node cycles (outward by the right-hand rule), the face points as functions of the in-face
# coordinates and the natural normal (the gradient of the natural coordinate that is constant on the face)
_FACES = [((0, 2, 1), [0., 0., -1.]), ((3, 4, 5), [0., 0., 1.]), ((0, 1, 4, 3), [0., -1., 0.]),
          ((1, 2, 5, 4), [1., 1., 0.]), ((2, 0, 3, 5), [-1., 0., 0.])]


def _face_points(face):
    """natural coordinates and weights of the integration points of face `face` (0..4)."""
    if face < 2:                                         # triangles: weights 1/3 times the facet area (globalNormal)
        z = -1. if face == 0 else 1.
        return [[a, b, z] for a, b in _TRI], [1. / 3.] * 3
    pts = []
    for z in (-_G, _G):
        for s in _S:                                     # in-face coordinate s in [0, 1] along the triangle edge
            pts.append([[s, 0., z], [1. - s, s, z], [0., 1. - s, z]][face - 2])
    return pts, [0.5] * 4                                # ds dzeta: the surface Jacobian follows from n_nat (Nanson)


def wedge_N(c):
    L = np.array([1. - c[0] - c[1], c[0], c[1]])
    return np.concatenate([L * (1. - c[2]) / 2., L * (1. + c[2]) / 2.])


def wedge_dN(c):
    L = np.array([1. - c[0] - c[1], c[0], c[1]])
    dL = np.array([[-1., -1.], [1., 0.], [0., 1.]])
    lo, hi = (1. - c[2]) / 2., (1. + c[2]) / 2.
    return np.concatenate([np.column_stack([dL * lo, -L / 2.]), np.column_stack([dL * hi, L / 2.])])


_GP = [[a, b, z] for z in (-_G, _G) for a, b in _TRI]


class Element_linear_wedge(ElementBase):
    dm, npe = 3, 6
    _parent_shape, _order = "wedge", 1          # mass_rule()
    _gauss_points = _GP
    _gauss_weights = [1. / 6.] * 6
    facet_natural_coos = {tuple(sorted(f)): _face_points(i)[0] for i, (f, _) in enumerate(_FACES)}
    facet_point_weights = {tuple(sorted(f)): _face_points(i)[1] for i, (f, _) in enumerate(_FACES)}
    facet_natural_normals = {tuple(sorted(f)): [n] * len(_face_points(i)[1]) for i, (f, n) in enumerate(_FACES)}
    inp_surface_num = [(tuple(sorted(f)),) for f, _ in _FACES]
    _quad_faces = [f for f, _ in _FACES if len(f) == 4]
    _tri_faces = [f for f, _ in _FACES if len(f) == 3]
    _tri_split = _tri_faces + [t for f in _quad_faces for t in ((f[0], f[1], f[2]), (f[0], f[2], f[3]))]
    # Gauss-point values -> nodal values: the inverse of [N_a(x_g)], exact for fields in the element's shape space
    _extrap_matrix = np.linalg.inv(np.array([wedge_N(np.asarray(p)) for p in _GP]))

    def shapeFunc_pyscope(self, natCoo):
        return wedge_N(natCoo)

    def dshape_dnat_pyscope(self, natCoo):
        return wedge_dN(natCoo)
