"""Element plugin interface of femcy_amd (the drop-in for /root/reference/element_zoo).

`ElementBase` keeps the reference's abstract surface (element_base.py:9-53: shapeFunc,
dshape_dnat, *_pyscope twins, globalNormal, strainMtrx, getMesh, extrapolate and the data
attributes dm, gaussPoints, gaussWeights, integPointNum_eachFacet, facet_natural_coos,
facet_point_weights, facet_natural_normals, inp_surface_num) but is table-driven: a concrete
element only declares its data and its two shape-function callables; everything else is generic
numpy here.  What the HIP kernels consume is `tables()`: dN[nGP][npe][dm], w[nGP], the Voigt
pattern and, for body loads, N[nGP][npe] -- the derivative table depends only on the Gauss point, never on the element
(SURVEY.md 2b), so it is staged once into LDS/constant memory by the device code.
"""
import abc
from typing import Dict, List, Sequence, Tuple

import numpy as np

from ..fields import HostField

VOIGT_2D = 0   # [xx, yy, xy]            (engineering shear)
VOIGT_3D = 1   # [xx, yy, zz, xy, zx, yz]


class ElementBase(abc.ABC):
    #: filled by subclasses -------------------------------------------------------------
    dm: int
    npe: int
    _gauss_points: Sequence[Sequence[float]]
    _gauss_weights: Sequence[float]
    facet_natural_coos: Dict[Tuple[int, ...], List[List[float]]]
    facet_point_weights: Dict[Tuple[int, ...], List[float]]
    facet_natural_normals: Dict[Tuple[int, ...], List[List[float]]]
    inp_surface_num: List[Tuple[Tuple[int, ...], ...]]
    _tri_split: Sequence[Tuple[int, int, int]]      # visualisation triangles per element / per face
    _extrap_points = None                           # natural coords fed to _extrap_basis
    _extrap_matrix = None                           # or an explicit [npe, nGP] matrix
    _parent_shape: str                              # "simplex" (unit triangle / tetrahedron), "cube" ([-1, 1]^dm), "wedge"
    _order: int                                     # polynomial degree p of the shape functions (per direction on a cube)

    def __init__(self):
        self.gaussPoints = HostField(self._gauss_points)
        self.gaussWeights = HostField(self._gauss_weights)
        self.gaussPoints_visualize = self.gaussPoints
        # the point count of the first facet; an element with facets of two arities (wedge) has one per arity:
        # facet_tables(nfn)["nip"]
        self.integPointNum_eachFacet = len(next(iter(self.facet_point_weights.values())))

    # ---- shape functions: subclasses implement the two *_pyscope methods ---------------
    @abc.abstractmethod
    def shapeFunc_pyscope(self, natCoo) -> np.ndarray: ...

    @abc.abstractmethod
    def dshape_dnat_pyscope(self, natCoo) -> np.ndarray: ...

    def shapeFunc(self, natCoo):
        return self.shapeFunc_pyscope(np.asarray(natCoo, dtype=np.float64))

    def dshape_dnat(self, natCoo):
        return self.dshape_dnat_pyscope(np.asarray(natCoo, dtype=np.float64))

    # ---- what the device kernels need --------------------------------------------------
    def tables(self) -> dict:
        gp = np.asarray(self.gaussPoints, dtype=np.float64)
        dN = np.ascontiguousarray(np.stack([self.dshape_dnat_pyscope(p) for p in gp]), dtype=np.float64)
        assert dN.shape == (gp.shape[0], self.npe, self.dm)
        N = np.ascontiguousarray(np.stack([self.shapeFunc_pyscope(p) for p in gp]), dtype=np.float64)
        assert N.shape == (gp.shape[0], self.npe)
        return {"nGP": gp.shape[0], "npe": self.npe, "dm": self.dm, "dN": dN, "N": N,
                "w": np.ascontiguousarray(self.gaussWeights, dtype=np.float64),
                "voigt_kind": VOIGT_2D if self.dm == 2 else VOIGT_3D}

    def mass_rule(self) -> Tuple[np.ndarray, np.ndarray]:
        """(points [nq, dm], weights [nq]) on the parent element for the consistent mass.  The integrand N_a N_b has
        twice the degree of the shape functions, which the stiffness rule under-integrates (the four-point rule of C3D10
        gives an element mass of rank 4), so the mass has a rule of its own, generated and not typed in: tensor
        Gauss-Legendre of p + 1 points per direction on [-1, 1]^dm (exact to degree 2p per direction), and on the unit
        triangle / tetrahedron the same rule collapsed by the Duffy map x = u, y = v (1 - u), z = w (1 - u)(1 - v), with
        enough points per direction for the Jacobian (1 - u)^(dm-1) (1 - v)^(dm-2) on top of total degree 2p (C3D10:
        4 x 3 x 3 = 36 points).  The wedge takes the triangle's rule times the line's.  All weights are positive."""
        from numpy.polynomial.legendre import leggauss
        p, dm = int(self._order), int(self.dm)

        def unit(n):                                 # n-point Gauss-Legendre rule on [0, 1]
            x, w = leggauss(n)
            return 0.5 * (x + 1.0), 0.5 * w

        def simplex(d, degree):                      # exact for total degree `degree` on the unit d-simplex
            rules = [unit((degree + (d - 1 - i) + 2) // 2) for i in range(d)]      # 2n - 1 >= degree + (d - 1 - i)
            pts, wts = [], []
            for idx in np.ndindex(*[len(r[0]) for r in rules]):
                t = [rules[i][0][k] for i, k in enumerate(idx)]
                w = np.prod([rules[i][1][k] for i, k in enumerate(idx)])
                x, shrink = [], 1.0
                for i in range(d):
                    x.append(t[i] * shrink)
                    w *= (1.0 - t[i]) ** (d - 1 - i)
                    shrink *= 1.0 - t[i]
                pts.append(x)
                wts.append(w)
            return np.array(pts), np.array(wts)

        if self._parent_shape == "cube":
            x, w = leggauss(p + 1)
            grids = np.meshgrid(*([x] * dm), indexing="ij")
            wg = np.meshgrid(*([w] * dm), indexing="ij")
            return np.column_stack([g.ravel() for g in grids]), np.prod([g.ravel() for g in wg], axis=0)
        if self._parent_shape == "simplex":
            return simplex(dm, 2 * p)
        assert self._parent_shape == "wedge"
        tp, tw = simplex(2, 2 * p)
        z, wz = leggauss(p + 1)
        pts = np.array([[a, b, c] for c in z for a, b in tp])
        return pts, np.array([u * v for v in wz for u in tw])

    def mass_tables(self) -> dict:
        """what femcy_mass_create takes: the shape functions Nq [nq, npe], their natural derivatives dNq [nq, npe, dm] and
        the weights wq [nq] at the points of mass_rule()"""
        pts, w = self.mass_rule()
        return {"nq": len(w), "Nq": np.ascontiguousarray([self.shapeFunc_pyscope(q) for q in pts], dtype=np.float64),
                "dNq": np.ascontiguousarray([self.dshape_dnat_pyscope(q) for q in pts], dtype=np.float64),
                "wq": np.ascontiguousarray(w, dtype=np.float64), "points": pts}

    def facet_arities(self) -> List[int]:
        """the node counts of the element's facets, ascending (the wedge has triangles and quadrilaterals)."""
        return sorted({len(k) for k in self.facet_natural_coos})

    def facet_tables(self, nfn: int = None) -> dict:
        """the facet dictionaries (facet_natural_coos / facet_point_weights / facet_natural_normals, keyed by the
        sorted local node tuple) as the plain arrays femcy_loadset_create takes; facet type = position of the key.
        nfn selects the facets of nfn nodes (one load set per facet arity); None takes every facet, which needs an
        element with one facet arity."""
        keys = list(self.facet_natural_coos.keys())
        if nfn is None:
            if len(self.facet_arities()) > 1:
                raise ValueError(f"{type(self).__name__} has facets of {self.facet_arities()} nodes: pass nfn")
            nip = self.integPointNum_eachFacet
        else:
            keys = [k for k in keys if len(k) == nfn]
            if not keys:
                raise ValueError(f"{type(self).__name__} has no facet of {nfn} nodes")
            nip = len(self.facet_point_weights[keys[0]])
        coos = np.array([[self.facet_natural_coos[k][i] for i in range(nip)] for k in keys], dtype=np.float64)
        return {"keys": keys, "nft": len(keys), "nfn": len(keys[0]), "nip": nip,
                "ft_nodes": np.ascontiguousarray(keys, dtype=np.int32),
                "N": np.ascontiguousarray([[self.shapeFunc_pyscope(c) for c in row] for row in coos], dtype=np.float64),
                "dN": np.ascontiguousarray([[self.dshape_dnat_pyscope(c) for c in row] for row in coos], dtype=np.float64),
                "normal": np.ascontiguousarray([[self.facet_natural_normals[k][i] for i in range(nip)] for k in keys],
                                               dtype=np.float64),
                "weight": np.ascontiguousarray([[self.facet_point_weights[k][i] for i in range(nip)] for k in keys],
                                               dtype=np.float64)}

    # ---- generic numpy bodies ----------------------------------------------------------
    def strainMtrx(self, dsdx) -> np.ndarray:
        """B(grad N) with the reference's Voigt ordering, shape (s, npe*dm)."""
        g = np.asarray(dsdx, dtype=np.float64)
        npe, dm = g.shape
        if dm == 2:
            B = np.zeros((3, 2 * npe))
            B[0, 0::2], B[1, 1::2] = g[:, 0], g[:, 1]
            B[2, 0::2], B[2, 1::2] = g[:, 1], g[:, 0]
        else:
            B = np.zeros((6, 3 * npe))
            B[0, 0::3], B[1, 1::3], B[2, 2::3] = g[:, 0], g[:, 1], g[:, 2]
            B[3, 0::3], B[3, 1::3] = g[:, 1], g[:, 0]
            B[4, 0::3], B[4, 2::3] = g[:, 2], g[:, 0]
            B[5, 1::3], B[5, 2::3] = g[:, 2], g[:, 1]
        return B

    def globalNormal(self, nodes: np.ndarray, facet: list, integPointId=0):
        """outward unit normal n_g = n_nat (dx/dxi)^-1 (normalised with +1e-30) and
        (facet size) x (facet point weight) for one facet integration point.  A 3-D facet of four nodes (hexahedron
        face) takes the surface Jacobian instead of a size: |det J| |n_nat J^-1| x weight (Nanson's formula)."""
        key = tuple(sorted(facet))
        nat = np.asarray(self.facet_natural_coos[key][integPointId], dtype=np.float64)
        jac = np.asarray(nodes).T @ self.dshape_dnat_pyscope(nat)
        n = np.asarray(self.facet_natural_normals[key][integPointId]) @ np.linalg.inv(jac)
        if self.dm == 3 and len(key) == 4:
            nrm = np.linalg.norm(n)
            return n / (nrm + 1.e-30), abs(np.linalg.det(jac)) * nrm * self.facet_point_weights[key][integPointId]
        n = n / (np.linalg.norm(n) + 1.e-30)
        p = np.asarray(nodes)
        if self.dm == 2:
            size = np.linalg.norm(p[key[0]] - p[key[1]])
        else:
            size = 0.5 * np.linalg.norm(np.cross(p[key[1]] - p[key[0]], p[key[2]] - p[key[0]]))
        return n, size * self.facet_point_weights[key][integPointId]

    def getMesh(self, elements: np.ndarray):
        """triangles for drawing, face -> elements map, and the outer surface (vectorised).  Elements with
        quadrilateral faces (`_quad_faces`, node cycles) find the outer surface on the faces themselves, keyed by their
        sorted nodes, so that it does not depend on how neighbours would split a shared face; `mesh` and the map are then
        keyed by faces, and the outer faces are split into two triangles each."""
        el = np.asarray(elements)
        if getattr(self, "_quad_faces", None) and getattr(self, "_tri_faces", None):
            # faces of both kinds (wedge): each kind keyed by its sorted nodes; `mesh` is then a list of face keys of
            # both sizes, and the outer surface the outer triangles plus two triangles per outer quadrilateral
            face2ele = {}
            outer = []
            for cycles, split in ((self._tri_faces, [[0, 1, 2]]), (self._quad_faces, [[0, 1, 2], [0, 2, 3]])):
                faces = np.concatenate([el[:, list(f)] for f in cycles], axis=0)
                owner = np.tile(np.arange(el.shape[0]), len(cycles))
                keys = np.sort(faces, axis=1)
                _, inv, cnt = np.unique(keys, axis=0, return_inverse=True, return_counts=True)
                for f, e in zip(map(tuple, keys.tolist()), owner.tolist()):
                    face2ele.setdefault(f, set()).add(e)
                out = faces[cnt[inv.ravel()] == 1]
                outer += [out[:, t] for t in split]
            return list(face2ele.keys()), face2ele, np.concatenate(outer, axis=0)
        if getattr(self, "_quad_faces", None):
            quads = np.concatenate([el[:, list(f)] for f in self._quad_faces], axis=0)
            owner = np.tile(np.arange(el.shape[0]), len(self._quad_faces))
            keys = np.sort(quads, axis=1)
            mesh, inv, cnt = np.unique(keys, axis=0, return_inverse=True, return_counts=True)
            face2ele: Dict[Tuple[int, ...], set] = {}
            for f, e in zip(map(tuple, keys.tolist()), owner.tolist()):
                face2ele.setdefault(f, set()).add(e)
            outer = quads[cnt[inv.ravel()] == 1]
            surfaces = np.concatenate([outer[:, [0, 1, 2]], outer[:, [0, 2, 3]]], axis=0)
            return mesh, face2ele, surfaces
        tris = np.sort(np.concatenate([el[:, list(t)] for t in self._tri_split], axis=0), axis=1)
        owner = np.tile(np.arange(el.shape[0]), len(self._tri_split))
        face2ele: Dict[Tuple[int, ...], set] = {}
        for f, e in zip(map(tuple, tris.tolist()), owner.tolist()):
            face2ele.setdefault(f, set()).add(e)
        mesh = np.array(list(face2ele.keys()))
        surfaces = np.array([f for f, es in face2ele.items() if len(es) == 1])
        return mesh, face2ele, surfaces

    def extrap_matrix(self) -> np.ndarray:
        """[npe, nGP]: Gauss-point values -> patch-wise nodal values."""
        if self._extrap_matrix is not None:
            return np.asarray(self._extrap_matrix, dtype=np.float64)
        return np.array([self._extrap_basis(np.asarray(p, dtype=np.float64)) for p in self._extrap_points])

    def _extrap_basis(self, nat):           # overridden where extrapolation uses another basis
        return self.shapeFunc_pyscope(nat)

    def extrapolate(self, internal_vals, nodal_vals, comp: int = 0):
        """Gauss-point values -> patch-wise nodal values (no averaging across elements).  A device
        Gauss-point field (`backend.GaussField`) is extrapolated by the HIP kernel of its context;
        a host array by one matrix product."""
        if hasattr(internal_vals, "ctx"):
            out = internal_vals.ctx.extrapolate(internal_vals.which, self.extrap_matrix(), comp)
        else:
            out = np.asarray(internal_vals) @ self.extrap_matrix().T
        if hasattr(nodal_vals, "from_numpy"):
            nodal_vals.from_numpy(out)
        elif nodal_vals is not None:
            nodal_vals[...] = out
        return out
