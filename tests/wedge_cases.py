"""C3D6 scenarios written against the C ABI (femcy_amd.backend.Context) and the deck driver, so that the host backend
(tests/test_wedge_cpu.py, in a child process with FEMCY_BACKEND=cpu) and the device (tests/test_gpu_wedge.py) run the
same code.  Every function checks its own result and returns a few numbers for the caller to compare."""
import os

import numpy as np

from femcy_amd import backend as be, meshgen
from femcy_amd.element_zoo import Element_linear_wedge
from femcy_amd.material_zoo import LinearIsotropic, NeoHookean

import wedge_reference as wr
from oracle import femcy_oracle as orc

E, NU = 2.0e5, 0.3


def box_mesh(nx, ny, nz, size=(4.0, 1.0, 1.0), perturb=0.0, seed=0):
    return meshgen.plate_wedge(nx, ny, nz, perturb=perturb, seed=seed, box=size)


def make_ctx(nodes, el, mat=("lin", E, NU)):
    ctx = be.Context(0)
    ctx.set_mesh(nodes, el)
    ctx.set_element(Element_linear_wedge())
    ctx.set_material(LinearIsotropic(mat[1], mat[2]) if mat[0] == "lin" else NeoHookean(mat[1], mat[2]))
    ctx.build_pattern()
    return ctx


def interior_dofs(nodes, size):
    lo = np.all(nodes > 1e-9, axis=1)
    hi = np.all(nodes < np.asarray(size) - 1e-9, axis=1)
    idx = np.nonzero(lo & hi)[0]
    return (idx[:, None] * 3 + np.arange(3)[None, :]).ravel()


def patch_test():
    """linear u = A X on a distorted mesh: F constant, so sigma is the same at every Gauss point and the interior
    nodal forces (internal force and K u) vanish."""
    size = (2.0, 1.5, 1.0)
    nodes, el = box_mesh(4, 3, 3, size, perturb=0.25, seed=3)
    A = np.array([[1e-3, 2e-4, -3e-4], [5e-4, -7e-4, 1e-4], [-2e-4, 3e-4, 6e-4]])
    u = (nodes @ A.T).ravel()
    ctx = make_ctx(nodes, el)
    ctx.upload(be.VEC_DOF, u)
    ctx.internal_force(be.VEC_DOF, be.VEC_FORCE)
    f = ctx.download(be.VEC_FORCE)
    ctx.compute_strain_stress(be.VEC_DOF, large=True)
    sig = ctx.gauss_field(be.GP_SIGMA).to_numpy().reshape(len(el), 6, -1)
    ctx.assemble_K(-1)
    Ku = ctx.get_K_bsr().tocsr() @ u
    inner = interior_dofs(nodes, size)
    scale = np.abs(f).max()
    assert np.abs(f[inner]).max() < 1e-10 * scale, np.abs(f[inner]).max() / scale
    assert np.abs(Ku[inner]).max() < 1e-10 * np.abs(Ku).max()
    spread = np.abs(sig - sig[0, 0]).max() / np.abs(sig).max()
    assert spread < 1e-10, spread
    ctx.close()
    return {"f_inner": float(np.abs(f[inner]).max() / scale), "sigma_spread": float(spread)}


def write_bar_deck(path, nx=4, ny=2, nz=2, perturb=0.2, sigma=100.0, etype="C3D6", top=False):
    """a bar 4 x 1 x 1 held by three symmetry planes (x = 0, y = 0, z = 0) and pulled by a pressure of -sigma on its
    face x = 4: face S3 (a quadrilateral) of the second wedge of every cell of the last column.  top: the same
    surface also holds the face z = 1, faces S2 (triangles) of both wedges of every cell of the top layer."""
    size = (4.0, 1.0, 1.0)
    nodes, el = box_mesh(nx, ny, nz, size, perturb=perturb, seed=1)
    cells = np.arange(len(el) // 2).reshape(nz, ny, nx)
    inst = "Part-1-1"
    with open(path, "w") as f:
        f.write("*Heading\n*Part, name=Part-1\n*End Part\n*Assembly, name=Assembly\n")
        f.write("*Instance, name=%s, part=Part-1\n*Node\n" % inst)
        for i, p in enumerate(nodes):
            f.write("%d, %.17g, %.17g, %.17g\n" % (i + 1, p[0], p[1], p[2]))
        f.write("*Element, type=%s\n" % etype)
        for i, e in enumerate(el):
            f.write(", ".join(str(v) for v in [i + 1] + (e + 1).tolist()) + "\n")
        f.write("*End Instance\n")
        for name, axis in (("symx", 0), ("symy", 1), ("symz", 2)):
            ids = np.nonzero(np.abs(nodes[:, axis]) < 1e-12)[0] + 1
            f.write("*Nset, nset=%s, instance=%s\n" % (name, inst))
            f.write("".join("%d\n" % v for v in ids))
        f.write("*Elset, elset=_end_S3, internal, instance=%s\n" % inst)
        f.write("".join("%d\n" % (2 * v + 2) for v in cells[:, :, -1].ravel()))
        if top:
            f.write("*Elset, elset=_top_S2, internal, instance=%s\n" % inst)
            f.write("".join("%d\n%d\n" % (2 * v + 1, 2 * v + 2) for v in cells[-1].ravel()))
        f.write("*Surface, type=ELEMENT, name=end\n_end_S3, S3\n%s*End Assembly\n" % ("_top_S2, S2\n" if top else ""))
        f.write("*Material, name=Material-1\n*Elastic\n%.17g, %.17g\n" % (E, NU))
        f.write("*Step, name=Step-1, nlgeom=NO\n*Static\n1., 1., 1e-05, 1.\n")
        f.write("*Boundary\nsymx, 1, 1\nsymy, 2, 2\nsymz, 3, 3\n")
        f.write("*Dsload\nend, P, %.17g\n*End Step\n" % (-sigma))
    return nodes, el


def bar_exact(nodes, sigma=100.0):
    return np.stack([sigma * nodes[:, 0] / E, -NU * sigma * nodes[:, 1] / E, -NU * sigma * nodes[:, 2] / E], axis=1).ravel()


def bar_end_to_end(tmpdir, sigma=100.0):
    """femcy_amd.main on the generated deck reproduces the uniaxial solution (exact for linear wedges)."""
    from femcy_amd import main
    path = os.path.join(tmpdir, "bar_c3d6.inp")
    nodes, _ = write_bar_deck(path, sigma=sigma)
    _, system = main.run(path, verbose=False)
    u = system.dof.to_numpy()
    ue = bar_exact(nodes, sigma)
    err = np.abs(u - ue).max() / np.abs(ue).max()
    assert err < 1e-10, err
    return {"err": float(err)}


def boundary_faces(nodes, el, size):
    """(element, face) of every element face that lies on a face of the box, with the box face's outward normal."""
    out = []
    for e, conn in enumerate(el):
        for face, (cyc, _) in enumerate(wr.FACES):
            p = nodes[conn[list(cyc)]]
            for ax in range(3):
                for side, sgn in ((0.0, -1.0), (size[ax], 1.0)):
                    if np.all(np.abs(p[:, ax] - side) < 1e-12):
                        n = np.zeros(3)
                        n[ax] = sgn
                        out.append((e, face, n))
    return out


def homogeneous_stretch(kind):
    """u = (F - I) X with a diagonal stretch: sigma is constant, so the internal force of node a is the boundary
    integral of N_a sigma n over the deformed box -- summed here from the restatement's facet loads of both face kinds."""
    size = (1.0, 1.0, 1.0)
    nodes, el = box_mesh(2, 2, 2, size)
    Fm = np.diag([1.3, 0.9, 1.1])
    u = (nodes @ (Fm - np.eye(3)).T).ravel()
    mat = ("lin", E, NU) if kind == "lin" else ("neo", 80.0, 2.5e-3)
    ctx = make_ctx(nodes, el, mat)
    ctx.upload(be.VEC_DOF, u)
    ctx.internal_force(be.VEC_DOF, be.VEC_FORCE)
    f = ctx.download(be.VEC_FORCE).reshape(-1, 3)
    omat = orc.Material("lin3d" if kind == "lin" else "neohooke", mat[1:])
    sig = orc.cauchy_large(omat, Fm)
    x = nodes @ Fm.T
    want = np.zeros_like(f)
    for e, face, n in boundary_faces(nodes, el, size):
        key = sorted(wr.FACES[face][0])
        want[el[e][key]] += wr.facet_load(x[el[e]], face, 1.0, sig @ n)
    err = np.abs(f - want).max() / np.abs(want).max()
    assert err < 1e-12, err
    ctx.close()
    return {"err": float(err)}


def mixed_surface_loads(ctx, nodes, el, faces, traction, direction=None):
    """device / host load sets of a surface of both face kinds: (rhs of the whole surface, rhs of the triangle part,
    rhs of the quadrilateral part, the restatement's rhs).  faces: (element, face number 0..4)."""
    ELE = Element_linear_wedge()
    parts = {}
    for nfn in (3, 4):
        sel = [(e, f) for e, f in faces if len(wr.FACES[f][0]) == nfn]
        keys = ELE.facet_tables(nfn)["keys"]
        ft = np.array([keys.index(ELE.inp_surface_num[f][0]) for _, f in sel], np.int32)
        parts[nfn] = ctx.loadset(ELE, np.array([e for e, _ in sel], np.int32), ft, nfn)
    ctx.loadset_neumann(parts[3], traction, direction, be.VEC_RHS)
    tri = ctx.download(be.VEC_RHS)
    ctx.loadset_neumann(parts[4], traction, direction, be.VEC_RHS)
    quad = ctx.download(be.VEC_RHS)
    ctx.loadset_neumann(parts[3], traction, direction, be.VEC_RHS)
    ctx.loadset_neumann(parts[4], traction, direction, be.VEC_RHS, add=True)
    both = ctx.download(be.VEC_RHS)
    want = np.zeros(nodes.size)
    for e, f in faces:
        key = sorted(wr.FACES[f][0])
        fl = wr.facet_load(nodes[el[e]], f, traction, direction)
        for i, a in enumerate(key):
            want[el[e][a] * 3:el[e][a] * 3 + 3] += fl[i]
    return both, tri, quad, want


def mixed_surface_check(warp=True):
    """the outer surface x = 0 (quadrilaterals) and z = 0 (triangles) of a warped block as one surface."""
    size = (2.0, 1.0, 1.5)
    nodes, el = box_mesh(3, 2, 2, size)
    if warp:
        nodes = nodes.copy()
        nodes[:, 0] += 0.1 * np.sin(nodes[:, 1]) * nodes[:, 2]
    faces = [(e, f) for e, f, n in boundary_faces(meshgen.plate_wedge(3, 2, 2, box=size)[0], el, size)
             if (n[0] < 0 or n[2] < 0)]
    assert {len(wr.FACES[f][0]) for _, f in faces} == {3, 4}
    ctx = make_ctx(nodes, el)
    out = []
    for direction in (None, np.array([0.2, -0.5, 1.0])):
        both, tri, quad, want = mixed_surface_loads(ctx, nodes, el, faces, 3.0, direction)
        err = np.abs(both - want).max() / np.abs(want).max()
        assert err < 1e-13, err
        assert np.array_equal(both, tri + quad)
        out.append(float(err))
    ctx.close()
    return {"err": out}
