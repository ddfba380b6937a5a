"""C3D6 wedge on the CPU: element tables, exact element stiffness, reader, the facet measure of both face kinds, the
outer surface, the host backend in a child process (FEMCY_BACKEND=cpu) and the VTK output."""
import os
import subprocess
import sys

import numpy as np
import pytest

import wedge_reference as wr
from femcy_amd import meshgen
from femcy_amd.element_zoo import Element_linear_wedge

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ELE = Element_linear_wedge()
RNG = np.random.default_rng(7)


def _nat_points(k):
    p = RNG.uniform(0, 1, (k, 2))
    p = np.where(p.sum(axis=1, keepdims=True) > 1, 1 - p, p)       # inside the unit triangle
    return np.column_stack([p, RNG.uniform(-1, 1, k)])


def _distorted_wedge(seed=0, amp=0.15):
    rng = np.random.default_rng(seed)
    return (wr.NODES + [0., 0., 1.]) * np.array([1.5, 1.2, 0.8]) + rng.uniform(-amp, amp, (6, 3))


# ------------------------------------------------------------------------------------------------ element tables
def test_partition_of_unity_and_zero_gradient_sums():
    for p in _nat_points(20):
        assert abs(ELE.shapeFunc(p).sum() - 1.0) < 1e-15
        assert np.abs(ELE.dshape_dnat(p).sum(axis=0)).max() < 1e-15
    t = ELE.tables()
    assert t["nGP"] == 6 and t["npe"] == 6 and t["dm"] == 3
    assert np.abs(t["dN"].sum(axis=1)).max() < 1e-15
    assert abs(t["w"].sum() - 1.0) < 1e-15                  # the volume of the reference prism


def test_gradients_match_central_differences():
    h = 1e-6
    for p in _nat_points(10):
        num = np.stack([(ELE.shapeFunc(p + h * e) - ELE.shapeFunc(p - h * e)) / (2 * h) for e in np.eye(3)], axis=1)
        assert np.abs(num - ELE.dshape_dnat(p)).max() < 1e-9


def test_nodes_are_abaqus_ordered_and_interpolate():
    for a, c in enumerate(wr.NODES):
        assert np.allclose(ELE.shapeFunc(c), np.eye(6)[a])
    assert np.all(wr.NODES[:3, 2] == -1) and np.all(wr.NODES[3:, 2] == 1)
    assert np.array_equal(wr.NODES[3:, :2], wr.NODES[:3, :2])      # node k + 3 above node k


def test_extrapolation_is_exact_in_the_shape_space():
    E = ELE.extrap_matrix()
    gp = np.asarray(ELE.gaussPoints)
    for _ in range(5):
        c = RNG.normal(size=6)
        field = lambda p: c[0] + c[1] * p[0] + c[2] * p[1] + c[3] * p[2] + c[4] * p[0] * p[2] + c[5] * p[1] * p[2]
        vals = np.array([field(p) for p in gp])
        assert np.abs(E @ vals - np.array([field(p) for p in wr.NODES])).max() < 1e-12


def test_plugin_tables_equal_the_reference_restatement():
    assert np.array_equal(np.asarray(ELE.gaussPoints), wr.GP)
    assert np.array_equal(np.asarray(ELE.gaussWeights), wr.GW)
    assert np.abs(ELE.tables()["dN"] - wr.dN_table()).max() < 1e-16
    for p in _nat_points(5):
        assert np.abs(ELE.shapeFunc(p) - wr.N(p)).max() < 1e-16
    assert [k for k, in ELE.inp_surface_num] == [tuple(sorted(f)) for f, _ in wr.FACES]
    assert [k for k, in ELE.inp_surface_num] == [(0, 1, 2), (3, 4, 5), (0, 1, 3, 4), (1, 2, 4, 5), (0, 2, 3, 5)]
    d = wr.elem_def()
    for k in ELE.facet_natural_coos:
        assert np.allclose(ELE.facet_natural_coos[k], d.facet_natural_coos[k])
        assert np.allclose(ELE.facet_natural_normals[k], d.facet_natural_normals[k])
        assert np.allclose(ELE.facet_point_weights[k], d.facet_point_weights[k])
    assert np.allclose(ELE.extrap_matrix(), d.extrap)


def test_facet_tables_per_arity():
    assert ELE.facet_arities() == [3, 4]
    with pytest.raises(ValueError, match="pass nfn"):
        ELE.facet_tables()
    tri, quad = ELE.facet_tables(3), ELE.facet_tables(4)
    assert tri["keys"] == [(0, 1, 2), (3, 4, 5)] and tri["nip"] == 3 and tri["nfn"] == 3
    assert quad["keys"] == [(0, 1, 3, 4), (1, 2, 4, 5), (0, 2, 3, 5)] and quad["nip"] == 4 and quad["nfn"] == 4
    assert np.allclose(tri["weight"].sum(axis=1), 1.0) and np.allclose(quad["weight"].sum(axis=1), 2.0)
    assert quad["N"].shape == (3, 4, 6) and quad["dN"].shape == (3, 4, 6, 3) and tri["normal"].shape == (2, 3, 3)


def test_single_arity_facet_tables_are_unchanged():
    from femcy_amd.element_zoo import Element_linear_hexahedral, Element_quadratic_tetrahedral
    for cls in (Element_linear_hexahedral, Element_quadratic_tetrahedral):
        e = cls()
        a, b = e.facet_tables(), e.facet_tables(e.facet_arities()[0])
        assert a["keys"] == b["keys"] and a["nip"] == b["nip"] == e.integPointNum_eachFacet
        for k in ("N", "dN", "normal", "weight", "ft_nodes"):
            assert np.array_equal(a[k], b[k])


# ------------------------------------------------------------------------------------------------ element stiffness
def _plugin_Ke(x, C):
    t = ELE.tables()
    K = np.zeros((18, 18))
    for dN, w in zip(t["dN"], t["w"]):
        J = x.T @ dN
        B = ELE.strainMtrx(dN @ np.linalg.inv(J))
        K += B.T @ C @ B * np.linalg.det(J) * w
    return K


def test_exact_stiffness_of_a_sheared_right_prism():
    """a right prism sheared by an affine map x = A xi + b (parallel triangular faces): K^e against the exact
    integral over the reference prism, in rational arithmetic."""
    import sympy as s
    xi = s.symbols("x y z")
    A = s.Matrix([[2, s.Rational(1, 2), s.Rational(1, 3)], [0, 1, s.Rational(1, 4)], [0, 0, s.Rational(3, 2)]])
    L = [1 - xi[0] - xi[1], xi[0], xi[1]]
    Nsym = [l * (1 - xi[2]) / 2 for l in L] + [l * (1 + xi[2]) / 2 for l in L]
    dN = s.Matrix([[s.diff(n, v) for v in xi] for n in Nsym])                   # [6, 3]
    X = s.Matrix([list(A * s.Matrix([s.nsimplify(v) for v in c])) for c in wr.NODES])
    J = X.T * dN
    grad = dN * J.inv()
    Enu = (s.Integer(1000), s.Rational(1, 4))
    lam = Enu[0] * Enu[1] / ((1 + Enu[1]) * (1 - 2 * Enu[1]))
    mu = Enu[0] / (2 * (1 + Enu[1]))
    C = s.zeros(6, 6)
    for i in range(3):
        for j in range(3):
            C[i, j] = lam + (2 * mu if i == j else 0)
        C[3 + i, 3 + i] = mu
    B = s.zeros(6, 18)
    for a in range(6):
        g = grad[a, :]
        B[0, 3 * a], B[1, 3 * a + 1], B[2, 3 * a + 2] = g[0], g[1], g[2]
        B[3, 3 * a], B[3, 3 * a + 1] = g[1], g[0]
        B[4, 3 * a], B[4, 3 * a + 2] = g[2], g[0]
        B[5, 3 * a + 1], B[5, 3 * a + 2] = g[2], g[1]
    integrand = (B.T * C * B) * J.det()

    def integ(e):
        inner = s.integrate(s.integrate(s.expand(e), (xi[1], 0, 1 - xi[0])), (xi[0], 0, 1))
        return s.integrate(inner, (xi[2], -1, 1))
    K_exact = np.array([[float(integ(integrand[i, j])) if j >= i else 0.0 for j in range(18)] for i in range(18)])
    K_exact = K_exact + np.triu(K_exact, 1).T
    x = wr.NODES @ np.array(A, dtype=float).T
    Cn = np.array(C, dtype=float)
    for K in (_plugin_Ke(x, Cn), wr.element_K(x, Cn)):
        assert np.abs(K - K_exact).max() < 1e-13 * np.abs(K_exact).max()


def test_distorted_element_has_exactly_six_rigid_modes():
    x = _distorted_wedge(3)
    K = _plugin_Ke(x, wr.C_iso(1000.0, 0.3))
    ev = np.linalg.eigvalsh(K)
    assert np.sum(np.abs(ev) < 1e-10 * ev.max()) == 6, ev[:8]
    assert np.abs(K - wr.element_K(x, wr.C_iso(1000.0, 0.3))).max() < 1e-12 * np.abs(K).max()


# ------------------------------------------------------------------------------------------------ reader
def test_reader_maps_c3d6_decks_and_surfaces(tmp_path):
    import wedge_cases as wc
    from femcy_amd.reader.inp_info import InpInfo
    path = str(tmp_path / "bar.inp")
    nodes, el = wc.write_bar_deck(path)
    inp = InpInfo(path)
    assert isinstance(inp.ELE, Element_linear_wedge)
    assert np.array_equal(list(inp.eSets.values())[0], el)
    faces = inp.face_sets["end"]
    assert len(faces) == 4                     # 2 x 2 cells on x = 4, one quadrilateral each
    for f in faces:
        assert len(f) == 4 and np.allclose(nodes[list(f), 0], 4.0)
    (nb,) = inp.neumann_bc_info
    assert nb["traction"] == 100.0


@pytest.mark.parametrize("face", range(5))
def test_surface_numbers_select_faces_with_outward_normals(tmp_path, face):
    import wedge_cases as wc
    from femcy_amd.reader.inp_info import InpInfo
    path = str(tmp_path / "bar.inp")
    wc.write_bar_deck(path)
    txt = open(path).read().replace("_end_S3, S3", "_end_S3, S%d" % (face + 1))
    open(path, "w").write(txt)
    inp = InpInfo(path)
    el = list(inp.eSets.values())[0]
    key = ELE.inp_surface_num[face][0]
    assert inp.face_sets["end"]
    for f in inp.face_sets["end"]:
        owner = [e for e in el[inp.ele_sets["_end_S3"]] if set(f) <= set(e.tolist()) and
                 tuple(sorted(int(np.nonzero(e == v)[0][0]) for v in f)) == key]
        assert len(owner) == 1
        X = inp.nodes[owner[0]]
        centroid = X.mean(axis=0)
        for ip in range(len(ELE.facet_point_weights[key])):
            n, aw = ELE.globalNormal(X, list(key), ip)
            assert abs(np.linalg.norm(n) - 1) < 1e-12 and aw > 0
            assert np.dot(n, X[list(key)].mean(axis=0) - centroid) > 0


# ------------------------------------------------------------------------------------------------ facet measure
def _plugin_facet_load(x, face, p, direction=None):
    key = ELE.inp_surface_num[face][0]
    out = np.zeros((len(key), 3))
    for ip in range(len(ELE.facet_point_weights[key])):
        n, aw = ELE.globalNormal(x, list(key), ip)
        t = p * (n if direction is None else np.asarray(direction))
        out += np.outer(ELE.shapeFunc(ELE.facet_natural_coos[key][ip])[list(key)], t) * aw
    return out


def test_flat_faces_carry_pressure_times_area():
    A = np.array([[2.0, 0.5, 0.3], [0.0, 1.0, 0.25], [0.0, 0.0, 1.5]])
    x = wr.NODES @ A.T
    for face in range(5):
        cyc = wr.FACES[face][0]
        p = x[list(cyc)]
        if len(cyc) == 3:
            area = 0.5 * np.linalg.norm(np.cross(p[1] - p[0], p[2] - p[0]))
        else:                                    # a parallelogram (faces of an affine prism)
            area = np.linalg.norm(np.cross(p[1] - p[0], p[3] - p[0]))
        load = _plugin_facet_load(x, face, 3.0)
        assert abs(np.linalg.norm(load.sum(axis=0)) - 3.0 * area) < 1e-13 * area
        assert np.abs(load - wr.facet_load(x, face, 3.0)).max() < 1e-14 * np.abs(load).max()


def test_warped_quadrilateral_face_matches_a_fine_surface_quadrature():
    """a warped S3..S5 face against a 40 x 40 midpoint rule of |dx/ds x dx/dzeta| N_a on the face."""
    for seed in range(3):
        x = _distorted_wedge(seed, amp=0.25)
        for face in (2, 3, 4):
            got = _plugin_facet_load(x, face, 2.0)
            key = sorted(wr.FACES[face][0])
            ds, dz = wr._TANGENTS[wr.FACES[face][1]]
            m = 40
            want = np.zeros((4, 3))
            centre = x.mean(axis=0)
            for i in range(m):
                for j in range(m):
                    s, z = (i + 0.5) / m, -1 + 2 * (j + 0.5) / m
                    p = wr.face_param(face, s, z)
                    J = x.T @ wr.dN(p)
                    nvec = np.cross(J @ np.asarray(ds), J @ np.asarray(dz))
                    if np.dot(nvec, x.T @ wr.N(p) - centre) < 0:
                        nvec = -nvec
                    want += np.outer(wr.N(p)[key], 2.0 * nvec) * (1 / m) * (2 / m)
            assert np.abs(got - want).max() < 2e-3 * np.abs(want).max()        # midpoint rule, h^2
            assert np.abs(got - wr.facet_load(x, face, 2.0)).max() < 1e-14 * np.abs(got).max()


def test_mixed_surface_is_the_sum_of_its_parts():
    assert "ok" in _child("import wedge_cases as wc; wc.mixed_surface_check(); print('ok')")


def test_system_splits_a_mixed_surface_by_arity(tmp_path):
    """the solver's load sets: one per facet arity, the triangles first; the whole surface's load is the sum of the
    loads of its two parts (to rounding: the deck's own set of the end face lists its facets in another order)."""
    code = ("import numpy as np, wedge_cases as wc\nfrom femcy_amd import main, backend as be\n"
            "p = %r\nn, e = wc.write_bar_deck(p)\n_, s = main.run(p, verbose=False)\n"
            "b = s.body.get_boundary()\nend = [f for f in b if np.allclose(n[list(f), 0], 4.0)]\n"
            "bottom = [f for f in b if np.allclose(n[list(f), 2], 0.0)]\n"
            "assert {len(f) for f in end} == {4} and {len(f) for f in bottom} == {3}\n"
            "assert len(s._loadset(end + bottom)) == 2 and len(s._loadset(end)) == 2\n"
            "s.neumannBC(end + bottom, 3.0)\nboth = s.ctx.download(be.VEC_RHS)\n"
            "s.neumannBC(end, 3.0)\nq = s.ctx.download(be.VEC_RHS)\ns.neumannBC(bottom, 3.0)\n"
            "t = s.ctx.download(be.VEC_RHS)\nassert np.abs(both - (t + q)).max() <= 1e-14 * np.abs(both).max()\n"
            "print('ok')\n") % str(tmp_path / "bar.inp")
    assert "ok" in _child(code)


def test_load_set_count_depends_on_the_element_alone(tmp_path):
    """every rank of a partitioned run makes one load-set call per facet arity of the element, whichever facets of the
    surface it holds (none, one kind or both): the interface sums of neumannBC stay in step across the ranks."""
    code = ("import numpy as np, wedge_cases as wc, hex_cases as hc\nfrom femcy_amd import main\n"
            "for mod, p, k in ((wc, %r, 2), (hc, %r, 1)):\n"
            "    n, e = mod.write_bar_deck(p)\n    _, s = main.run(p, verbose=False)\n    b = s.body.get_boundary()\n"
            "    end = [f for f in b if np.allclose(n[list(f), 0], 4.0)]\n"
            "    top = [f for f in b if np.allclose(n[list(f), 2], 1.0)]\n"
            "    for faces in ([], end, top, end + top):\n"
            "        assert len(s._loadset(faces)) == k, (p, len(faces))\n"
            "print('ok')\n") % (str(tmp_path / "w.inp"), str(tmp_path / "h.inp"))
    assert "ok" in _child(code)


# ------------------------------------------------------------------------------------------------ outer surface
@pytest.mark.parametrize("n", [1, 2, 3])
def test_outer_surface_of_a_block(n):
    nodes, el = meshgen.plate_wedge(n, n, n, box=(1.0, 1.0, 1.0))
    mesh, face2ele, tris = ELE.getMesh(el)
    assert tris.shape == (12 * n * n, 3)                           # 4 z faces of 2 n^2 triangles, 4 x/y faces of n^2 quads
    ntri = 2 * n * n * (n + 1)                                     # triangles on the z = const planes
    nquad = 2 * n * n * (n + 1) + n * n * n                        # x / y planes, and the cut diagonals
    assert len(face2ele) == len(mesh) == ntri + nquad
    assert sum(len(k) == 3 for k in face2ele) == ntri
    assert all(len(v) == 1 or len(v) == 2 for v in face2ele.values())
    for t in tris:                                                 # every triangle lies in a face plane of the block
        p = nodes[t]
        assert any(np.all(np.abs(p[:, k] - p[0, k]) < 1e-12) and (p[0, k] < 1e-12 or p[0, k] > 1 - 1e-12)
                   for k in range(3))
        # and its right-hand normal points out of the block
        nrm = np.cross(p[1] - p[0], p[2] - p[0])
        assert np.dot(nrm, p.mean(axis=0) - 0.5) > 0


def test_plate_wedge_volumes_and_valence():
    nodes, el = meshgen.plate_wedge(3, 2, 4, box=(3.0, 2.0, 4.0))
    assert el.shape == (48, 6)
    vol = np.array([sum(np.linalg.det(nodes[e].T @ wr.dN(g)) * w for g, w in zip(wr.GP, wr.GW)) for e in el])
    assert vol.min() > 0 and abs(vol.sum() - 24.0) < 1e-12
    inner = np.nonzero(np.all((nodes > 0.5) & (nodes < np.array([3.0, 2.0, 4.0]) - 0.5), axis=1))[0]
    cnt = np.bincount(el.ravel(), minlength=len(nodes))
    assert np.all(cnt[inner] == 12)
    nb = [set(el[np.any(el == a, axis=1)].ravel()) for a in inner]
    assert all(len(s) == 21 for s in nb)
    m = meshgen.twist_plate_wedge(4, 2, 6)
    mh = meshgen.twist_plate_hex(4, 2, 6)
    assert m["etype"] == "C3D6" and np.array_equal(m["nodes"], mh["nodes"])
    for k in mh["node_sets"]:
        assert np.array_equal(m["node_sets"][k], mh["node_sets"][k])


# ------------------------------------------------------------------------------------------------ host backend
def _child(code):
    env = dict(os.environ, FEMCY_BACKEND="cpu")
    out = subprocess.run([sys.executable, "-c", "import sys; sys.path[:0] = [%r, %r]\n" % (ROOT, os.path.join(ROOT, "tests"))
                          + code], capture_output=True, text=True, timeout=600, cwd=ROOT, env=env)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    return out.stdout


def test_host_backend_patch_test():
    assert "ok" in _child("import wedge_cases as wc; wc.patch_test(); print('ok')")


def test_host_backend_uniaxial_bar(tmp_path):
    assert "ok" in _child("import wedge_cases as wc; wc.bar_end_to_end(%r); print('ok')" % str(tmp_path))


def test_host_backend_homogeneous_stretch_forces():
    assert "ok" in _child("import wedge_cases as wc; wc.homogeneous_stretch('lin'); wc.homogeneous_stretch('neo'); "
                          "print('ok')")


def test_host_backend_matches_the_restatement():
    code = ("import numpy as np, wedge_cases as wc, wedge_reference as wr\nfrom femcy_amd import backend as be\n"
            "n, e = wc.box_mesh(3, 2, 2, perturb=0.2, seed=4)\nc = wc.make_ctx(n, e)\n"
            "u = 1e-3 * np.sin(np.arange(n.size))\nc.upload(be.VEC_DOF, u)\nc.assemble_K(be.VEC_DOF)\n"
            "K = c.get_K_bsr().tocsr()\nKr = wr.assemble_K(n, e, wr.C_iso(wc.E, wc.NU), u)\n"
            "assert abs(K - Kr).max() <= 1e-12 * abs(Kr).max()\nprint('ok')\n")
    assert "ok" in _child(code)


# ------------------------------------------------------------------------------------------------ output
def test_vtk_wedges_follow_the_vtk_orientation(tmp_path):
    """VTK_WEDGE: the right-hand normal of points (0, 1, 2) points away from the triangle (3, 4, 5)."""
    from types import SimpleNamespace
    from femcy_amd import vtk_out
    nodes, el = meshgen.plate_wedge(2, 1, 2, perturb=0.2, seed=1)
    vec = SimpleNamespace(to_numpy=lambda: np.zeros(nodes.size))
    system = SimpleNamespace(body=SimpleNamespace(np_nodes=nodes, np_elements=el), dof=vec)
    path = str(tmp_path / "m.vtk")
    vtk_out.write_vtk(path, system)
    txt = open(path).read()
    cells = txt.split("CELLS %d %d\n" % (len(el), 7 * len(el)))[1].split("CELL_TYPES")[0].split()
    conn = np.array(cells, dtype=np.int64).reshape(len(el), 7)
    assert np.all(conn[:, 0] == 6)
    assert txt.split("CELL_TYPES %d\n" % len(el))[1].split()[:len(el)] == ["13"] * len(el)
    for c, e in zip(conn[:, 1:], el):
        assert sorted(c) == sorted(e)
        p = nodes[c]
        nrm = np.cross(p[1] - p[0], p[2] - p[0])
        assert np.dot(nrm, p[3:].mean(axis=0) - p[:3].mean(axis=0)) < 0
