"""C3D8 trilinear hexahedron, full 2 x 2 x 2 Gauss rule.  Abaqus node order: nodes 0-3 are the face zeta = -1
(counter-clockwise seen from +zeta), nodes 4-7 the face zeta = +1, node k + 4 above node k.  The reference has no
hexahedron; the faces follow Abaqus' S1..S6 numbering."""
import numpy as np
from .element_base import ElementBase

_G = 1. / 3. ** 0.5
_CORNERS = np.array([[-1., -1., -1.], [1., -1., -1.], [1., 1., -1.], [-1., 1., -1.],
                     [-1., -1., 1.], [1., -1., 1.], [1., 1., 1.], [-1., 1., 1.]])
# Abaqus faces S1..S6 as node cycles (outward by the right-hand rule), the natural coordinate fixed on each and its sign
_FACES = [((0, 3, 2, 1), 2, -1.), ((4, 5, 6, 7), 2, 1.), ((0, 1, 5, 4), 1, -1.),
          ((1, 2, 6, 5), 0, 1.), ((2, 3, 7, 6), 1, 1.), ((3, 0, 4, 7), 0, -1.)]


def trilinear(c):
    return (1. + _CORNERS[:, 0] * c[0]) * (1. + _CORNERS[:, 1] * c[1]) * (1. + _CORNERS[:, 2] * c[2]) / 8.


def _face_points(axis, side):
    """2 x 2 Gauss points on the face (natural coordinate `axis` = side), weight 1 each."""
    pts = []
    for a in (-_G, _G):
        for b in (-_G, _G):
            p = [a, b]
            p.insert(axis, side)
            pts.append(p)
    return pts


def _normal(axis, side):
    n = [0., 0., 0.]
    n[axis] = side
    return n


class Element_linear_hexahedral(ElementBase):
    dm, npe = 3, 8
    _parent_shape, _order = "cube", 1          # mass_rule()
    _gauss_points = (_CORNERS * _G).tolist()
    _gauss_weights = [1.] * 8
    facet_natural_coos = {tuple(sorted(f)): _face_points(ax, sd) for f, ax, sd in _FACES}
    facet_point_weights = {tuple(sorted(f)): [1.] * 4 for f, _, _ in _FACES}
    facet_natural_normals = {tuple(sorted(f)): [_normal(ax, sd)] * 4 for f, ax, sd in _FACES}
    inp_surface_num = [(tuple(sorted(f)),) for f, _, _ in _FACES]
    _quad_faces = [f for f, _, _ in _FACES]
    _tri_split = [t for f, _, _ in _FACES for t in ((f[0], f[1], f[2]), (f[0], f[2], f[3]))]
    _extrap_points = (_CORNERS * 3. ** 0.5).tolist()

    def shapeFunc_pyscope(self, natCoo):
        return trilinear(natCoo)

    def dshape_dnat_pyscope(self, natCoo):
        s, c = _CORNERS, natCoo
        return np.stack([s[:, 0] * (1. + s[:, 1] * c[1]) * (1. + s[:, 2] * c[2]),
                         s[:, 1] * (1. + s[:, 0] * c[0]) * (1. + s[:, 2] * c[2]),
                         s[:, 2] * (1. + s[:, 0] * c[0]) * (1. + s[:, 1] * c[1])], axis=1) / 8.
