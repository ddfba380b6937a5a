"""*Dload / *Cload on the device: femcy_bodyload_* (k_body_weights, k_node_sum, k_body_apply) and femcy_dofset_add
against closed forms, the numpy restatement (tests/loads_reference.py) and the host backend; the scenarios are those of
tests/loads_cases.py, which tests/test_loads_cpu.py runs on the host."""
import os
import subprocess
import sys
import threading
import types

import numpy as np
import pytest

import loads_cases as lc
import loads_reference as lr
from femcy_amd import backend as be

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("etype", lr.ETYPES)
def test_closed_forms(etype):
    lc.closed_form(etype, "hip")


@pytest.mark.parametrize("etype", lr.ETYPES)
def test_weights_and_vector_match_the_restatement(etype):
    """perturbed meshes of all eight (npe, dm) shapes, 240 .. 720 elements (more than one block, the last one partial)"""
    lc.against_restatement(etype, "hip")


def test_node_with_more_than_32_incident_elements():
    lc.fan_centre("hip")


def test_selection_empty_selection_and_bits():
    lc.selections("hip")


def test_dofset_add():
    lc.dofset_add("hip")


def test_refusals_are_not_fatal():
    lc.refusals("hip")


# ------------------------------------------------------------------------------------- several ranks
def _run_ranks(nranks, fn):
    """fn(rank) on one thread per rank (the in-process group transport); re-raises the first failure."""
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


@pytest.mark.parametrize("nranks", [2, 3])
def test_partitioned_loads_equal_single_context(nranks):
    """a body force on the whole mesh, one on an element set that the cut divides, and a *Cload on a node set that
    holds nodes of the interface, through LocalDeck and the driver: every rank's right-hand side equals the
    single-context one on all of its nodes, the shared ones included"""
    from femcy_amd import partition
    from femcy_amd.body import Body
    from femcy_amd.material_zoo import LinearIsotropic
    from femcy_amd.stiffnessMtrx import System_of_equations
    nodes, el, ELE = lr.mesh("C3D4", cells=(4, 3, 6))
    mat = LinearIsotropic(2.0e5, 0.3)
    parts = partition.build_all_parts(nodes, el, nranks, axis=2)
    shared = np.intersect1d(parts[0].l2g, parts[1].l2g)
    assert shared.size
    upper = np.nonzero(nodes[el].mean(axis=1)[:, 0] > 0.5 * nodes[:, 0].max())[0]          # cut by every z-slab
    inp = types.SimpleNamespace(
        time_incs=None, geometric_nonlinear=False, materials={"Elastic": mat}, ELE=ELE, dirichlet_bc_info=[],
        neumann_bc_info=[], density=None,
        body_force_info=[{"ele_set": None, "force": lc.B3}, {"ele_set": upper, "force": np.array([-2.0, 0.5, 0.0])}],
        cload_info=[{"node_set": np.concatenate([shared[:3], [0]]), "dof": 1, "val": 4.5}])
    bcs = lambda deck: {"neumannBCs": [], "dirichletBCs": [], "bodyForces": deck.body_force_info, "cloads": deck.cload_info}
    ref = System_of_equations(Body(nodes, el, ELE), mat, False, verbose=False)
    ref.rhs.fill(3.0)                                   # no *Dsload: the driver starts from zero
    ref.impose_boundary_condition(bcs(inp))
    want = ref.rhs.to_numpy()
    ref.ctx.close()
    m = lr.nodal_weights(nodes, el, ELE)
    host = lr.load_vector(m, lc.B3) + lr.load_vector(lr.nodal_weights(nodes, el, ELE, upper), [-2.0, 0.5, 0.0])
    host.reshape(-1, 3)[inp.cload_info[0]["node_set"], 1] += 4.5
    assert np.abs(want - host).max() <= 1e-12 * np.abs(host).max()
    uid = be.Context.comm_local_id()

    def rank_main(r):
        p = parts[r]
        body = Body(p.nodes, p.elements, ELE)
        system = System_of_equations(body, mat, False, verbose=False, part=p, comm_uid=uid)
        try:
            deck = partition.LocalDeck(inp, p, body)
            system.impose_boundary_condition(bcs(deck))
            with pytest.raises(be.FemcyError, match="TMP1"):
                system.ctx.bodyload_apply(system._bodyload(None), lc.B3, be.VEC_TMP1, add=True)
            return system.rhs.to_numpy()
        finally:
            system.ctx.close()

    outs = _run_ranks(nranks, rank_main)
    for p, v in zip(parts, outs):                       # every replica, not only the owner's
        local = p.scatter_global(want)
        assert np.linalg.norm(v - local) <= 1e-7 * np.linalg.norm(local)
    u = partition.gather_owned(parts, outs, nodes.size)
    assert np.linalg.norm(u - want) <= 1e-7 * np.linalg.norm(want)


# --------------------------------------------------------------------------------------- whole decks
def test_hanging_bar_c3d8(tmp_path):
    """u_z = -rho g (L z - z^2 / 2) / E at the nodes of a column of four bricks; the bound is the direct solve's own
    (smoke(): 1e-9)"""
    _, err = lc.hanging_bar(str(tmp_path / "bar.inp"), "C3D8", "hip")
    print(f"hanging bar, C3D8: relative error {err:.3e}")
    assert err <= 1e-9


HOST_CODE = """
import sys
sys.path[:0] = [%r, %r]
import numpy as np, loads_cases as lc
out = {}
for etype in ("C3D4", "C3D6", "CPS4"):
    out[etype] = lc.hanging_bar(%r + "/host_" + etype + ".inp", etype, "cpu")[0]
lc.write_neo_hookean_plate(%r + "/host_neo.inp")
_, s, out["neo"] = lc.solve_deck(%r + "/host_neo.inp", "cpu")
out["neo_stats"] = np.array(str(s.stats))
np.savez(%r + "/host.npz", **out)
"""


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    """the host backend's answers to the decks below, from one child process (FEMCY_BACKEND=cpu)"""
    d = str(tmp_path_factory.mktemp("host"))
    env = dict(os.environ, FEMCY_BACKEND="cpu")
    out = subprocess.run([sys.executable, "-c", HOST_CODE % (ROOT, os.path.join(ROOT, "tests"), d, d, d, d)],
                         capture_output=True, text=True, timeout=600, cwd=ROOT, env=env)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    return np.load(os.path.join(d, "host.npz"))


@pytest.mark.parametrize("etype", ["C3D4", "C3D6", "CPS4"])
def test_hanging_bar_matches_the_host_backend(tmp_path, host, etype):
    u, _ = lc.hanging_bar(str(tmp_path / "bar.inp"), etype, "hip")
    err = np.abs(u - host[etype]).max() / np.abs(host[etype]).max()
    print(f"hanging bar, {etype}: device against host {err:.3e}")
    assert err <= 1e-9                                  # two direct solves of the same system


def test_cload_deck_equals_dsload_deck(tmp_path):
    lc.cload_equals_dsload(str(tmp_path), "hip")


def test_neo_hookean_plate_under_gravity_matches_the_host_backend(tmp_path, host):
    """nlgeom = YES, two increments: the bound and the increment / solve counts of the wedge file's
    ...matches_the_host_backend tests"""
    path = str(tmp_path / "neo.inp")
    lc.write_neo_hookean_plate(path)
    inp, s, u = lc.solve_deck(path, "hip")
    assert inp.geometric_nonlinear and inp.body_force_info and len(s.increments) == 2
    uh = host["neo"]
    err = np.abs(u - uh).max() / np.abs(uh).max()
    print(f"neo-Hookean plate under gravity: device against host {err:.3e}, stats {s.stats}")
    assert str(s.stats) == str(host["neo_stats"])
    assert err <= 1e-8
    assert np.abs(u).max() > 1e-2                        # it sags
