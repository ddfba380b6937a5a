"""C3D8 hexahedron on the CPU: element tables, exact element stiffness, reader, quadrilateral facet measure, the host
backend in a child process (FEMCY_BACKEND=cpu) and the VTK / PNG output."""
import os
import subprocess
import sys

import numpy as np
import pytest

import hex_reference as hr
from femcy_amd import meshgen
from femcy_amd.element_zoo import Element_linear_hexahedral

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ELE = Element_linear_hexahedral()
RNG = np.random.default_rng(7)


def _distorted_hex(seed=0, amp=0.2):
    rng = np.random.default_rng(seed)
    return hr.CORNERS * np.array([1.5, 1.0, 0.8]) + rng.uniform(-amp, amp, (8, 3))


# ------------------------------------------------------------------------------------------------ element tables
def test_partition_of_unity_and_zero_gradient_sums():
    for p in RNG.uniform(-1, 1, (20, 3)):
        assert abs(ELE.shapeFunc(p).sum() - 1.0) < 1e-15
    t = ELE.tables()
    assert t["nGP"] == 8 and t["npe"] == 8 and t["dm"] == 3
    assert np.abs(t["dN"].sum(axis=1)).max() < 1e-15
    assert abs(t["w"].sum() - 8.0) < 1e-15


def test_gradients_match_central_differences():
    h = 1e-6
    for p in RNG.uniform(-1, 1, (10, 3)):
        num = np.stack([(ELE.shapeFunc(p + h * e) - ELE.shapeFunc(p - h * e)) / (2 * h) for e in np.eye(3)], axis=1)
        assert np.abs(num - ELE.dshape_dnat(p)).max() < 1e-9


def test_nodes_are_abaqus_ordered_and_interpolate():
    for a, c in enumerate(hr.CORNERS):
        assert np.allclose(ELE.shapeFunc(c), np.eye(8)[a])
    assert np.allclose(hr.CORNERS[4:, :2], hr.CORNERS[:4, :2]) and np.all(hr.CORNERS[:4, 2] == -1)


def test_extrapolation_is_exact_for_trilinear_fields():
    E = ELE.extrap_matrix()
    gp = np.asarray(ELE.gaussPoints)
    for _ in range(5):
        c = RNG.normal(size=8)
        field = lambda p: c[0] + c[1] * p[0] + c[2] * p[1] + c[3] * p[2] + c[4] * p[0] * p[1] + c[5] * p[1] * p[2] + \
            c[6] * p[0] * p[2] + c[7] * p[0] * p[1] * p[2]
        vals = np.array([field(p) for p in gp])
        assert np.abs(E @ vals - np.array([field(p) for p in hr.CORNERS])).max() < 1e-12


def test_plugin_tables_equal_the_reference_restatement():
    assert np.array_equal(np.asarray(ELE.gaussPoints), hr.GP)
    assert np.abs(ELE.tables()["dN"] - hr.dN_table()).max() < 1e-16
    for p in RNG.uniform(-1, 1, (5, 3)):
        assert np.abs(ELE.shapeFunc(p) - hr.N(p)).max() < 1e-16
    assert [k for k, in ELE.inp_surface_num] == [f for f, _, _ in hr.FACES]
    assert [k for k, in ELE.inp_surface_num] == [(0, 1, 2, 3), (4, 5, 6, 7), (0, 1, 4, 5), (1, 2, 5, 6), (2, 3, 6, 7),
                                                  (0, 3, 4, 7)]
    d = hr.elem_def()
    for k in ELE.facet_natural_coos:
        assert np.allclose(ELE.facet_natural_coos[k], d.facet_natural_coos[k])
        assert np.allclose(ELE.facet_natural_normals[k], d.facet_natural_normals[k])


# ------------------------------------------------------------------------------------------------ element stiffness
def _plugin_Ke(x, C):
    t = ELE.tables()
    K = np.zeros((24, 24))
    for dN, w in zip(t["dN"], t["w"]):
        J = x.T @ dN
        B = ELE.strainMtrx(dN @ np.linalg.inv(J))
        K += B.T @ C @ B * np.linalg.det(J) * w
    return K


def test_exact_stiffness_of_a_sheared_parallelepiped():
    import sympy as s
    xi = s.symbols("x y z")
    A = s.Matrix([[2, s.Rational(1, 2), s.Rational(1, 3)], [0, 1, s.Rational(1, 4)], [0, 0, s.Rational(3, 2)]])
    corners = [s.Matrix([int(v) for v in c]) for c in hr.CORNERS]
    Nsym = [s.Rational(1, 8) * (1 + c[0] * xi[0]) * (1 + c[1] * xi[1]) * (1 + c[2] * xi[2]) for c in corners]
    dN = s.Matrix([[s.diff(n, v) for v in xi] for n in Nsym])                   # [8, 3]
    X = s.Matrix([list(A * c) for c in corners])                              # x = A xi
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
    B = s.zeros(6, 24)
    for a in range(8):
        g = grad[a, :]
        B[0, 3 * a], B[1, 3 * a + 1], B[2, 3 * a + 2] = g[0], g[1], g[2]
        B[3, 3 * a], B[3, 3 * a + 1] = g[1], g[0]
        B[4, 3 * a], B[4, 3 * a + 2] = g[2], g[0]
        B[5, 3 * a + 1], B[5, 3 * a + 2] = g[2], g[1]
    integrand = (B.T * C * B) * J.det()

    def integ(e):
        p = s.Poly(s.expand(e), *xi)
        tot = s.Integer(0)
        for mon, co in p.terms():
            f = 1
            for k in mon:
                f *= 0 if k % 2 else s.Rational(2, k + 1)
            tot += co * f
        return tot
    K_exact = np.array([[float(integ(integrand[i, j])) for j in range(24)] for i in range(24)])
    x = np.array(hr.CORNERS) @ np.array(A, dtype=float).T
    Cn = np.array(C, dtype=float)
    for K in (_plugin_Ke(x, Cn), hr.element_K(x, Cn)):
        assert np.abs(K - K_exact).max() < 1e-13 * np.abs(K_exact).max()


def test_distorted_element_has_exactly_six_rigid_modes():
    x = _distorted_hex(3)
    K = _plugin_Ke(x, hr.C_iso(1000.0, 0.3))
    ev = np.linalg.eigvalsh(K)
    small = np.sum(np.abs(ev) < 1e-10 * ev.max())
    assert small == 6, ev[:8]
    assert np.abs(K - hr.element_K(x, hr.C_iso(1000.0, 0.3))).max() < 1e-12 * np.abs(K).max()


# ------------------------------------------------------------------------------------------------ reader
def test_reader_maps_c3d8_decks_and_surfaces(tmp_path):
    import hex_cases as hc
    from femcy_amd.reader.inp_info import InpInfo
    path = str(tmp_path / "bar.inp")
    nodes, el = hc.write_bar_deck(path)
    inp = InpInfo(path)
    assert isinstance(inp.ELE, Element_linear_hexahedral)
    assert np.array_equal(list(inp.eSets.values())[0], el)
    faces = inp.face_sets["end"]
    assert len(faces) == 4                     # 2 x 2 cells on x = 4
    for f in faces:
        assert np.allclose(nodes[list(f), 0], 4.0)
    (nb,) = inp.neumann_bc_info
    assert nb["traction"] == 100.0


@pytest.mark.parametrize("face", range(6))
def test_surface_numbers_select_faces_with_outward_normals(tmp_path, face):
    import hex_cases as hc
    from femcy_amd.reader.inp_info import InpInfo
    path = str(tmp_path / "bar.inp")
    hc.write_bar_deck(path)
    txt = open(path).read().replace("_end_S4, S4", "_end_S4, S%d" % (face + 1))
    open(path, "w").write(txt)
    inp = InpInfo(path)
    el = list(inp.eSets.values())[0]
    key = ELE.inp_surface_num[face][0]
    for f in inp.face_sets["end"]:
        # the element of the set whose face S<face+1> this is (a face between two cells of the set has two owners)
        owner = [e for e in el[inp.ele_sets["_end_S4"]] if set(f) <= set(e.tolist()) and
                 tuple(sorted(int(np.nonzero(e == v)[0][0]) for v in f)) == key]
        assert len(owner) == 1
        X = inp.nodes[owner[0]]
        centroid = X.mean(axis=0)
        for ip in range(4):
            n, aw = ELE.globalNormal(X, list(key), ip)
            assert abs(np.linalg.norm(n) - 1) < 1e-12 and aw > 0
            assert np.dot(n, X[list(key)].mean(axis=0) - centroid) > 0


def test_reduced_and_incompatible_hexahedra_read_as_c3d8(tmp_path):
    import hex_cases as hc
    from femcy_amd.reader.inp_info import InpInfo
    for t in ("C3D8R", "C3D8I"):
        path = str(tmp_path / ("bar_%s.inp" % t))
        hc.write_bar_deck(path, etype=t)
        assert isinstance(InpInfo(path).ELE, Element_linear_hexahedral)


# ------------------------------------------------------------------------------------------------ facet measure
def _plugin_facet_load(x, face, p):
    key = ELE.inp_surface_num[face][0]
    out = np.zeros((4, 3))
    for ip in range(4):
        n, aw = ELE.globalNormal(x, list(key), ip)
        out += np.outer(ELE.shapeFunc(ELE.facet_natural_coos[key][ip])[list(key)], p * n) * aw
    return out


def test_flat_parallelogram_face_carries_pressure_times_area():
    A = np.array([[2.0, 0.5, 0.3], [0.0, 1.0, 0.25], [0.0, 0.0, 1.5]])
    x = hr.CORNERS @ A.T
    for face in range(6):
        key = ELE.inp_surface_num[face][0]
        load = _plugin_facet_load(x, face, 3.0)
        _, ax, _ = hr.FACES[face]
        e = [A[:, k] * 2 for k in range(3) if k != ax]
        area = np.linalg.norm(np.cross(e[0], e[1]))
        assert abs(np.linalg.norm(load.sum(axis=0)) - 3.0 * area) < 1e-13 * area
        assert np.abs(load - hr.facet_load(x, face, 3.0)).max() < 1e-14 * np.abs(load).max()


def test_warped_face_matches_the_surface_jacobian_quadrature():
    for seed in range(4):
        x = _distorted_hex(seed, amp=0.3)
        for face in range(6):
            got, want = _plugin_facet_load(x, face, 2.0), hr.facet_load(x, face, 2.0)
            assert np.abs(got - want).max() < 1e-14 * np.abs(want).max()


# ------------------------------------------------------------------------------------------------ host backend
def _child(code):
    env = dict(os.environ, FEMCY_BACKEND="cpu")
    out = subprocess.run([sys.executable, "-c", "import sys; sys.path[:0] = [%r, %r]\n" % (ROOT, os.path.join(ROOT, "tests"))
                          + code], capture_output=True, text=True, timeout=600, cwd=ROOT, env=env)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    return out.stdout


def test_host_backend_patch_test():
    assert "ok" in _child("import hex_cases as hc; hc.patch_test(); print('ok')")


def test_host_backend_uniaxial_bar(tmp_path):
    assert "ok" in _child("import hex_cases as hc; hc.bar_end_to_end(%r); print('ok')" % str(tmp_path))


def test_host_backend_homogeneous_stretch_forces():
    assert "ok" in _child("import hex_cases as hc; hc.homogeneous_stretch('lin'); hc.homogeneous_stretch('neo'); "
                          "print('ok')")


def test_host_backend_reports_its_assembly():
    out = _child("import hex_cases as hc\nfrom femcy_amd import backend as be\n"
                 "n, e = hc.box_mesh(2, 2, 2)\nc = hc.make_ctx(n, e)\nc.assemble_K(-1)\nprint('mode', c.assembly_used())")
    assert "mode 1" in out


# ------------------------------------------------------------------------------------------------ output
def test_vtk_writes_hexahedra(tmp_path):
    from types import SimpleNamespace
    from femcy_amd import vtk_out
    nodes, el = meshgen.plate_hex(2, 1, 2)
    vec = SimpleNamespace(to_numpy=lambda: np.zeros(nodes.size))
    system = SimpleNamespace(body=SimpleNamespace(np_nodes=nodes, np_elements=el), dof=vec)
    path = str(tmp_path / "m.vtk")
    vtk_out.write_vtk(path, system)
    txt = open(path).read().split("CELL_TYPES %d\n" % len(el))[1].split()[:len(el)]
    assert txt == ["12"] * len(el)


@pytest.mark.parametrize("n", [1, 2, 3])
def test_outer_surface_of_a_block(n):
    nodes, el = meshgen.plate_hex(n, n, n, box=(1.0, 1.0, 1.0))
    _, face2ele, tris = ELE.getMesh(el)
    assert tris.shape == (12 * n * n, 3)
    assert len(face2ele) == 3 * n * n * (n + 1)
    on_box = np.any((nodes[tris] < 1e-12) | (nodes[tris] > 1 - 1e-12), axis=2)
    # every triangle lies in one face plane of the block
    assert all(np.any(np.all(np.abs(nodes[t][:, k] - nodes[t][0, k]) < 1e-12) and
                      (nodes[t][0, k] < 1e-12 or nodes[t][0, k] > 1 - 1e-12) for k in range(3)) for t in tris)
    assert on_box.all()
