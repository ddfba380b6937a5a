"""C3D6 on the MI355X: K from every mode that accepts the wedge against the numpy restatement (tests/wedge_reference.py),
the path AUTO takes (the one profiles/wedge_asm_record.json chose), determinism across the pair-list knobs, refusals, the
full-size plate, forces, loads on both face kinds, both solver legs and whole decks."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import wedge_cases as hc
import wedge_reference as hr
from femcy_amd import backend as be, meshgen
from femcy_amd.element_zoo import Element_linear_wedge
from oracle import femcy_oracle as orc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = [be.ASM_GATHER, be.ASM_GATHER_SYM, be.ASM_GATHER_SYM_ROWSUM, be.ASM_ROWS, be.ASM_ATOMIC, be.ASM_PAIRS, be.ASM_AUTO]
MATS = {"lin": (("lin", 2.0e5, 0.3), hr.C_iso(2.0e5, 0.3)), "neo": (("neo", 80.0, 2.5e-3), hr.C_neo(80.0, 2.5e-3))}


def _smooth_u(nodes):
    X = nodes / nodes.max(axis=0)
    return (0.01 * np.stack([np.sin(2 * X[:, 1]) * X[:, 2], X[:, 0] ** 2 - X[:, 2], np.cos(X[:, 0] + X[:, 1])], 1)).ravel()


def _rel(A, B):
    return abs(A - B).max() / abs(B).max()


def _meshes():
    small = meshgen.plate_wedge(6, 5, 4, perturb=0.25, seed=11, box=(6.0, 5.0, 4.0))
    plate = meshgen.plate_wedge(40, 5, 50, perturb=0.2, seed=5)           # 20 000 C3D6
    return {"small": small, "plate": plate}


MESHES = _meshes()


def _reference_K(nodes, el, C, u):
    if len(el) < 1000:
        return hr.assemble_K(nodes, el, C, u)
    topo = orc.Topology(nodes, el, hr.elem_def())
    return orc.assemble_K(topo, u, C)


@pytest.mark.parametrize("mesh", ["small", "plate"])
@pytest.mark.parametrize("mat", ["lin", "neo"])
@pytest.mark.parametrize("deformed", [False, True])
def test_every_mode_matches_the_reference(mesh, mat, deformed):
    nodes, el = MESHES[mesh]
    u = _smooth_u(nodes) if deformed else np.zeros(nodes.size)
    Kr = _reference_K(nodes, el, MATS[mat][1], u)
    ctx = hc.make_ctx(nodes, el, MATS[mat][0])
    ctx.upload(be.VEC_DOF, u)
    for mode in MODES:
        ctx.set_option(be.OPT_ASSEMBLY, mode)
        ctx.assemble_K(be.VEC_DOF)
        K = ctx.get_K_bsr().tocsr()
        assert _rel(K, Kr) <= 1e-12, (mode, _rel(K, Kr))
    ctx.close()


def _auto_mode():
    """the mode the record chose for C3D6 (tools/wedge_asm_record.py: the faster of PAIRS and the best generic mode)."""
    with open(os.path.join(ROOT, "profiles", "wedge_asm_record.json")) as f:
        return getattr(be, "ASM_" + json.load(f)["auto_choice"])


def test_auto_takes_the_recorded_mode_deterministically():
    nodes, el = MESHES["plate"]
    ctx = hc.make_ctx(nodes, el)
    ctx.upload(be.VEC_DOF, _smooth_u(nodes))
    ctx.assemble_K(be.VEC_DOF)
    assert ctx.assembly_used() == _auto_mode()
    K1 = ctx.get_K_ell()[1].copy()
    ctx.assemble_K(be.VEC_DOF)
    assert np.array_equal(ctx.get_K_ell()[1], K1)
    ctx.set_option(be.OPT_ASSEMBLY, _auto_mode())
    ctx.assemble_K(be.VEC_DOF)
    assert ctx.assembly_used() == _auto_mode() and np.array_equal(ctx.get_K_ell()[1], K1)
    ctx.close()


# FEMCY_TUNE_PAIRS values that change only how the chunks are processed: XCD ranges (bit 0), rows per wave (bits 1-2),
# steps in flight (bits 3-4), Morton order (bit 5), chunks per wave (bits 6-9).  Every stored block sums its elements
# in ascending element order whatever the value, and no two lanes of one LDS add hit the same word, so the bits agree.
KNOBS = [163, 162, 161, 171, 179, 131, 35, 99, 227]


def test_pairs_bits_do_not_depend_on_the_knobs():
    nodes, el = MESHES["plate"]
    ctx = hc.make_ctx(nodes, el, MATS["neo"][0])
    ctx.upload(be.VEC_DOF, _smooth_u(nodes))
    ctx.set_option(be.OPT_ASSEMBLY, be.ASM_PAIRS)
    ref = None
    for tune in KNOBS:
        ctx.set_option(be.TUNE_PAIRS, tune)
        ctx.assemble_K(be.VEC_DOF)
        assert ctx.assembly_used() == be.ASM_PAIRS
        K = ctx.get_K_ell()[1].copy()
        if ref is None:
            ref = K
        assert np.array_equal(K, ref), tune
    ctx.close()


@pytest.mark.parametrize("mode", [be.ASM_ROWS2, be.ASM_ROWS4])
def test_c3d10_only_modes_refuse_wedges(mode):
    nodes, el = MESHES["small"]
    ctx = hc.make_ctx(nodes, el)
    ctx.set_option(be.OPT_ASSEMBLY, mode)
    with pytest.raises(be.FemcyError, match="instantiated"):
        ctx.assemble_K(-1)
    with pytest.raises(be.FemcyError, match="no assembly has run"):
        ctx.assembly_used()
    with pytest.raises(be.FemcyError, match="retired"):
        ctx.set_option(be.OPT_ASSEMBLY, 7)
    ctx.close()


def test_residual_and_K_leaves_the_same_bits():
    nodes, el = MESHES["plate"]
    for mat in ("lin", "neo"):
        ctx = hc.make_ctx(nodes, el, MATS[mat][0])
        ctx.upload(be.VEC_DOF, _smooth_u(nodes))
        ctx.internal_force(be.VEC_DOF, be.VEC_FORCE)
        f1 = ctx.download(be.VEC_FORCE)
        ctx.assemble_K(be.VEC_DOF)
        K1 = ctx.get_K_ell()[1].copy()
        ctx.vector(be.VEC_FORCE).fill(0.0)
        ctx.residual_and_K(be.VEC_DOF, be.VEC_FORCE)
        assert ctx.assembly_used() == _auto_mode()
        assert np.array_equal(ctx.download(be.VEC_FORCE), f1) and np.array_equal(ctx.get_K_ell()[1], K1)
        ctx.close()


def test_internal_force_matches_reference_and_closed_form():
    hc.homogeneous_stretch("lin")
    hc.homogeneous_stretch("neo")
    hc.patch_test()
    nodes, el = MESHES["small"]
    u = _smooth_u(nodes)
    for mat, om in (("lin", orc.Material("lin3d", (2.0e5, 0.3))), ("neo", orc.Material("neohooke", (80.0, 2.5e-3)))):
        ctx = hc.make_ctx(nodes, el, MATS[mat][0])
        ctx.upload(be.VEC_DOF, u)
        ctx.internal_force(be.VEC_DOF, be.VEC_FORCE)
        fr = hr.internal_force(nodes, el, u, om)
        assert _rel(ctx.download(be.VEC_FORCE), fr) < 1e-12
        ctx.close()


def test_device_loadset_matches_the_facet_quadrature():
    nodes, el = MESHES["small"]
    nodes = nodes.copy()
    nodes[:, 0] += 0.1 * np.sin(nodes[:, 1]) * nodes[:, 2]          # warp the faces
    ELE = Element_linear_wedge()
    ctx = hc.make_ctx(nodes, el)
    elems = np.arange(len(el))
    for ft in range(5):
        key = ELE.inp_surface_num[ft][0]
        t = ELE.facet_tables(len(key))["keys"].index(key)
        ls = ctx.loadset(ELE, elems.astype(np.int32), np.full(len(el), t, np.int32), len(key))
        for direction in (None, np.array([0.2, -0.5, 1.0])):
            ctx.loadset_neumann(ls, 3.0, direction, be.VEC_RHS)
            got = ctx.download(be.VEC_RHS)
            want = np.zeros(nodes.size)
            for e in elems:
                fl = hr.facet_load(nodes[el[e]], ft, 3.0, direction)
                for i, a in enumerate(key):
                    want[el[e][a] * 3:el[e][a] * 3 + 3] += fl[i]
            assert _rel(got, want) < 1e-13, (ft, _rel(got, want))
    ctx.close()


def test_device_mixed_surface_loads():
    hc.mixed_surface_check()


def test_fullsize_plate_pairs_against_gather_sym_rowsum():
    m = meshgen.twist_plate_wedge(192, 24, 216)
    nodes, el = m["nodes"], m["elements"]
    assert len(el) == 1990656 and len(nodes) == 1047025
    ctx = hc.make_ctx(nodes, el, ("lin", *m["elastic"]))
    ctx.set_option(be.OPT_ASSEMBLY, be.ASM_PAIRS)
    ctx.assemble_K(-1)
    assert ctx.assembly_used() == be.ASM_PAIRS
    Kp = ctx.get_K_bsr()
    ctx.set_option(be.OPT_ASSEMBLY, be.ASM_GATHER_SYM_ROWSUM)
    ctx.assemble_K(-1)
    Kg = ctx.get_K_bsr()
    assert np.array_equal(Kp.indptr, Kg.indptr) and np.array_equal(Kp.indices, Kg.indices)
    assert abs(Kp.data - Kg.data).max() <= 1e-12 * abs(Kg.data).max()
    diag = Kp.data[Kp.indptr[:-1]]                       # diagonal block first in every row
    rows = np.repeat(np.arange(Kp.shape[0] // 3), np.diff(Kp.indptr))
    is_diag = Kp.indices[Kp.indptr[:-1]] == np.arange(Kp.shape[0] // 3)
    if not is_diag.all():
        d = Kp.indices == rows
        diag = Kp.data[d]
    assert abs(diag - np.swapaxes(diag, 1, 2)).max() <= 1e-12 * abs(diag).max()
    ctx.close()


def test_persistent_and_three_launch_pcg_agree():
    nodes, el = meshgen.plate_wedge(16, 4, 24)
    ctx = hc.make_ctx(nodes, el)
    ctx.assemble_K(-1)
    fixed = np.nonzero(nodes[:, 2] < 1e-9)[0]
    cons = (fixed[:, None] * 3 + np.arange(3)).ravel().astype(np.int32)
    b = np.tile([0.0, 0.0, 1.0], len(nodes))
    res = []
    ctx.set_option(be.OPT_PCG_SMALL, 0)                  # 6 375 DOF would otherwise take the small-system kernel
    for persist, path in ((2, "solves_persist"), (0, "solves_three")):
        ctx.set_option(be.OPT_PCG_PERSIST, persist)
        ctx.upload(be.VEC_RESIDUAL, b)
        ctx.assemble_K(-1)
        ctx.dirichlet_newton(cons, be.VEC_RESIDUAL)
        ctx.timing_reset()
        it, _, _ = ctx.pcg(be.VEC_RESIDUAL, be.VEC_X, eps=1e-8)
        tm = ctx.timing()
        assert tm[path] == 1 and tm["solves_persist"] + tm["solves_three"] + tm["solves_small"] == 1, tm
        res.append((it, ctx.download(be.VEC_X)))
    assert res[0][0] == res[1][0]
    assert np.linalg.norm(res[0][1] - res[1][1]) <= 1e-10 * np.linalg.norm(res[1][1])
    ctx.close()


def _host(code):
    env = dict(os.environ, FEMCY_BACKEND="cpu")
    out = subprocess.run([sys.executable, "-c", "import sys; sys.path[:0] = [%r, %r]\n" % (ROOT, os.path.join(ROOT, "tests"))
                          + code], capture_output=True, text=True, timeout=1200, cwd=ROOT, env=env)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    return out.stdout


def test_direct_branch_matches_the_host_backend(tmp_path):
    nodes, el = meshgen.plate_wedge(8, 3, 10, perturb=0.2, seed=2)
    np.savez(tmp_path / "m.npz", nodes=nodes, el=el)
    code = ("import numpy as np, wedge_cases as hc\nfrom femcy_amd import backend as be\n"
            "d = np.load(%r)\nctx = hc.make_ctx(d['nodes'], d['el'])\nctx.assemble_K(-1)\n"
            "cons = np.nonzero(d['nodes'][:, 2] < 1e-9)[0]\ncons = (cons[:, None] * 3 + np.arange(3)).ravel().astype(np.int32)\n"
            "ctx.upload(be.VEC_RESIDUAL, np.tile([1.0, -0.5, 2.0], len(d['nodes'])))\n"
            "ctx.dirichlet_newton(cons, be.VEC_RESIDUAL)\nctx.direct_solve(be.VEC_RESIDUAL, be.VEC_TMP0)\n"
            "np.save(%r, ctx.download(be.VEC_TMP0))\n") % (str(tmp_path / "m.npz"), str(tmp_path / "x.npy"))
    _host(code)
    xh = np.load(tmp_path / "x.npy")
    exec(code.replace("np.save(%r, ctx.download(be.VEC_TMP0))" % str(tmp_path / "x.npy"), "X = ctx.download(be.VEC_TMP0)"),
         g := {})
    assert np.linalg.norm(g["X"] - xh) <= 1e-10 * np.linalg.norm(xh)


def test_uniaxial_bar_deck_end_to_end(tmp_path):
    hc.bar_end_to_end(str(tmp_path))


def _twist_deck(path, cells=(4, 1, 6)):
    m = meshgen.twist_plate_wedge(*cells, perturb=0.15, seed=4)
    m["neo_hookean"] = (80.0e3, 2.5e-6)
    m["time_incs"] = {"ini_inc": 0.05, "max_time": 0.1, "min_inc": 1e-5, "max_inc": 0.05}
    meshgen.write_inp(path, m)


def test_neo_hookean_twist_plate_matches_the_host_backend(tmp_path):
    path = str(tmp_path / "twist_c3d6.inp")
    _twist_deck(path)
    code = ("import numpy as np\nfrom femcy_amd import main\n_, s = main.run(%r, verbose=False)\n"
            "np.save(%r, s.dof.to_numpy())\nprint('STATS', s.stats)\n") % (path, str(tmp_path / "u.npy"))
    out = _host(code)
    host_stats = out.split("STATS ")[-1].strip()
    from femcy_amd import main
    _, s = main.run(path, verbose=False)
    uh = np.load(tmp_path / "u.npy")
    u = s.dof.to_numpy()
    assert str(s.stats) == host_stats
    assert np.abs(u - uh).max() <= 1e-8 * np.abs(uh).max()
    assert s.ctx.assembly_used() == _auto_mode()


def test_large_wedge_plate_runs_the_cg_leg(tmp_path):
    path = str(tmp_path / "twist_big.inp")
    m = meshgen.twist_plate_wedge(48, 10, 72)             # 39 347 nodes, 118 k DOF
    m["geometric_nonlinear"] = False
    m["bc_blocks"] = [(False, ["Set-10, %d, %d" % (d, d) for d in (1, 2, 3)]), (False, ["fit_right_z, 1, 1, 0.5"])]
    m["time_incs"] = {"ini_inc": 1.0, "max_time": 1.0, "min_inc": 1e-5, "max_inc": 1.0}
    meshgen.write_inp(path, m)
    from femcy_amd import main
    _, s = main.run(path, verbose=False)
    assert s.ctx.n >= 100000
    assert s.stats["cg_iterations"] > 0 and s.stats["direct_solves"] == 0
    assert np.isfinite(s.dof.to_numpy()).all() and np.abs(s.dof.to_numpy()).max() > 0


def _fan(k=30, layers=2):
    """k wedges around a vertical axis per layer: the axis node of the middle level has 3 (k + 1) = 93 blocks in its
    row, so the PAIRS tile (2 304 B per block slot at 8 rows per wave) does not fit a workgroup's LDS."""
    t = 2 * np.pi * np.arange(k) / k
    ring = np.column_stack([np.cos(t), np.sin(t)])
    level = np.vstack([[0.0, 0.0], ring])                                  # node 0 on the axis, then the ring
    nodes = np.vstack([np.column_stack([level, np.full(k + 1, 0.5 * z)]) for z in range(layers + 1)])
    el = []
    for z in range(layers):
        b, a = z * (k + 1), (z + 1) * (k + 1)
        for i in range(k):
            j = (i + 1) % k
            el.append([b, b + 1 + i, b + 1 + j, a, a + 1 + i, a + 1 + j])
    return nodes, np.asarray(el, np.int32)


def test_auto_falls_back_to_the_faster_generic_mode_when_the_tile_does_not_fit():
    nodes, el = _fan()
    u = _smooth_u(nodes - nodes.min(axis=0) + 1.0)
    ctx = hc.make_ctx(nodes, el)
    assert ctx.pattern_info().max_row_blocks == 93
    ctx.upload(be.VEC_DOF, u)
    ctx.assemble_K(be.VEC_DOF)
    assert ctx.assembly_used() == be.ASM_GATHER_SYM_ROWSUM
    Kr = hr.assemble_K(nodes, el, MATS["lin"][1], u)
    assert _rel(ctx.get_K_bsr().tocsr(), Kr) <= 1e-12
    ctx.set_option(be.OPT_ASSEMBLY, be.ASM_PAIRS)
    with pytest.raises(be.FemcyError, match="LDS"):
        ctx.assemble_K(be.VEC_DOF)
    ctx.close()


def _run_ranks(nranks, fn):
    """fn(rank) on one thread per rank (the in-process group transport); re-raises the first failure."""
    import threading
    out, err = [None] * nranks, []

    def work(r):
        try:
            out[r] = fn(r)
        except BaseException as e:                      # noqa: BLE001 - reported below
            err.append(e)

    threads = [threading.Thread(target=work, args=(r,), daemon=True) for r in range(nranks)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=180)
    assert not any(t.is_alive() for t in threads), "a rank is still running"
    if err:
        raise err[0]
    return out


def test_partitioned_mixed_surface_equals_single_context(tmp_path):
    """a C3D6 deck whose *Dsload surface holds quadrilaterals (x = 4) and triangles (z = 1), split over 3 ranks along x:
    the first rank holds triangles of the surface only, the last both kinds.  Every rank makes one load-set call per
    facet arity, so the interface sums stay in step, and the displacements equal the single-context solve."""
    from femcy_amd import partition
    from femcy_amd.body import Body
    from femcy_amd.reader import InpInfo
    from femcy_amd.stiffnessMtrx import System_of_equations
    path = str(tmp_path / "bar_mixed.inp")
    hc.write_bar_deck(path, nx=6, top=True)
    inp = InpInfo(path)
    assert {len(f) for f in inp.face_sets["end"]} == {3, 4}
    el = list(inp.eSets.values())[0]
    mat = list(inp.materials.values())[0]
    ref = System_of_equations(Body(inp.nodes, el, inp.ELE), mat, inp.geometric_nonlinear, verbose=False, direct="pcg")
    ref.solve(inp)
    u_ref = ref.dof.to_numpy()
    ref.ctx.close()
    parts = partition.build_all_parts(inp.nodes, el, 3, axis=0)
    uid = be.Context.comm_local_id()

    def rank_main(r):
        p = parts[r]
        body = Body(p.nodes, p.elements, inp.ELE)
        system = System_of_equations(body, mat, inp.geometric_nonlinear, verbose=False, part=p, comm_uid=uid)
        try:
            deck = partition.LocalDeck(inp, p, body)
            kinds = {len(f) for f in deck.neumann_bc_info[0]["face_set"]}
            system.solve(deck)
            return system.dof.to_numpy(), kinds
        finally:
            system.ctx.close()

    outs = _run_ranks(3, rank_main)
    kinds = [o[1] for o in outs]
    assert {3, 4} in kinds and any(k != {3, 4} for k in kinds), kinds
    u = partition.gather_owned(parts, [o[0] for o in outs], inp.nodes.size)
    assert np.linalg.norm(u - u_ref) <= 1e-7 * np.linalg.norm(u_ref)
