"""*Expansion + *Temperature on the device: femcy_thermal_* (k_thermal_force, k_nodal_force, k_thermal_apply,
k_thermal_post) against the long-double restatement (tests/thermal_reference.py), closed forms through the deck driver
and the host backend; the scenarios are those of tests/thermal_cases.py, which tests/test_thermal_cpu.py runs on the
host."""
import os
import subprocess
import sys
import threading
import types

import numpy as np
import pytest

import loads_reference as lr
import thermal_cases as tc
import thermal_reference as tr
from femcy_amd import backend as be

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASE_IDS = ["%s-%s%s" % (e, k, "-aniso" if a else "") for e, k, a in tc.CASES]


@pytest.mark.parametrize("etype,kind,aniso", tc.CASES, ids=CASE_IDS)
def test_kernels_match_the_restatement(etype, kind, aniso):
    """perturbed meshes of all eight (npe, dm) shapes, 240 .. 720 elements (more than one block, the last one partial),
    the three linear material kinds and the anisotropic C: f_unit, corrected sigma and von Mises"""
    tc.against_restatement(etype, kind, aniso, "mesh", "hip")


@pytest.mark.parametrize("etype", lr.ETYPES)
def test_single_element_and_less_than_a_wavefront(etype):
    for which in ("single", "small"):
        tc.against_restatement(etype, tc.KIND_OF[etype[:3]], False, which, "hip")


def test_node_with_more_than_32_incident_elements():
    tc.against_restatement("CPS3", tr.PSTRESS, False, "fan", "hip")


def test_zero_field_gives_zero_bits_and_two_creates_the_same_bits():
    tc.zero_field_and_bits("hip")


def test_apply():
    tc.apply("hip")


def test_refusals_are_not_fatal():
    tc.refusals("hip")


# --------------------------------------------------------------------------------------- whole decks
@pytest.mark.parametrize("case", ["free", "bar"])
@pytest.mark.parametrize("family", tc.FAMILIES)
def test_closed_forms(tmp_path, family, case):
    tc.closed_form(tmp_path, family, case, "hip")


@pytest.mark.parametrize("family", tc.QUADRATIC)
def test_linear_gradient_is_stress_free(tmp_path, family):
    tc.closed_form(tmp_path, family, "gradient", "hip")


@pytest.mark.parametrize("family", ["C3D8", "CPE4"])
def test_half_increment(tmp_path, family):
    tc.half_increment(tmp_path, family, "hip")


def test_nlgeom_with_a_thermal_load_raises(tmp_path):
    path = str(tmp_path / "nl.inp")
    tc.write_thermal_deck(path, "C3D8", "free", nlgeom=True)
    with pytest.raises(ValueError, match="nlgeom"):
        tc.solve_thermal_deck(path, "hip")


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
def test_partitioned_thermal_load_equals_single_context(nranks):
    """a temperature field that varies across the cut, through LocalDeck and the driver, after a body force: every
    rank's right-hand side equals the single-context one on all of its nodes, the shared ones included"""
    from femcy_amd import partition
    from femcy_amd.body import Body
    from femcy_amd.stiffnessMtrx import System_of_equations
    nodes, el, ELE = lr.mesh("C3D4", cells=(4, 3, 6))
    mat = tc.material(tr.LIN3D)
    parts = partition.build_all_parts(nodes, el, nranks, axis=2)
    assert np.intersect1d(parts[0].l2g, parts[1].l2g).size
    initial = np.full(len(nodes), 20.0)
    final = initial + tr.smooth_dT(nodes) + 0.5 * nodes[:, 2]                  # varies along the cut axis
    inp = types.SimpleNamespace(
        time_incs=None, geometric_nonlinear=False, materials={"Elastic": mat}, ELE=ELE, dirichlet_bc_info=[],
        neumann_bc_info=[], density=None, body_force_info=[{"ele_set": None, "force": np.array([0.7, -1.3, 2.1])}],
        cload_info=[], expansion=tc.ALPHA, temperature_info={"initial": initial, "final": final})

    def impose(system, deck):
        ti = deck.temperature_info
        th = system.ctx.thermal(ELE, deck.expansion, ti["final"] - ti["initial"])
        system.rhs.fill(3.0)                            # no *Dsload: the driver starts from zero
        system.impose_boundary_condition({"neumannBCs": [], "dirichletBCs": [], "bodyForces": deck.body_force_info,
                                          "cloads": [], "thermal": {"id": th, "scale": 0.75}})
        return th

    ref = System_of_equations(Body(nodes, el, ELE), mat, False, verbose=False)
    th = impose(ref, inp)
    want = ref.rhs.to_numpy()
    thermal_part = 0.75 * ref.ctx.thermal_force(th)
    ref.ctx.close()
    host = tr.thermal_force(nodes, el, ELE, mat.C, tr.LIN3D, tc.NU, tc.ALPHA, final - initial, np.longdouble)
    assert np.abs(thermal_part - 0.75 * host).max() <= tc.FORCE_TOL * np.abs(host).max()
    assert np.abs(want).max() > 0 and np.abs(thermal_part).max() > 1e-3 * np.abs(want).max()
    uid = be.Context.comm_local_id()

    def rank_main(r):
        p = parts[r]
        body = Body(p.nodes, p.elements, ELE)
        system = System_of_equations(body, mat, False, verbose=False, part=p, comm_uid=uid)
        try:
            th = impose(system, partition.LocalDeck(inp, p, body))
            with pytest.raises(be.FemcyError, match="TMP1"):
                system.ctx.thermal_apply(th, 1.0, be.VEC_TMP1, add=True)
            return system.rhs.to_numpy()
        finally:
            system.ctx.close()

    outs = _run_ranks(nranks, rank_main)
    for p, v in zip(parts, outs):                       # every replica, not only the owner's
        local = p.scatter_global(want)
        assert np.linalg.norm(v - local) <= 1e-7 * np.linalg.norm(local)
    u = partition.gather_owned(parts, outs, nodes.size)
    assert np.linalg.norm(u - want) <= 1e-7 * np.linalg.norm(want)


# ---------------------------------------------------------------------------------- host and device
HOST_CODE = """
import sys
sys.path[:0] = [%r, %r]
import numpy as np, thermal_cases as tc
out = {}
for i, (etype, kind, aniso) in enumerate(tc.CASES):
    f, sigma0, sigma, mises = tc.run_backend(etype, kind, aniso, "mesh", "cpu")
    out["f%%d" %% i], out["s0%%d" %% i], out["s%%d" %% i], out["m%%d" %% i] = f, sigma0, sigma, mises
np.savez(%r + "/host.npz", **out)
"""


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    """the host backend's answers on tc.CASES, from one child process (FEMCY_BACKEND=cpu)"""
    d = str(tmp_path_factory.mktemp("host"))
    env = dict(os.environ, FEMCY_BACKEND="cpu")
    out = subprocess.run([sys.executable, "-c", HOST_CODE % (ROOT, os.path.join(ROOT, "tests"), d)],
                         capture_output=True, text=True, timeout=600, cwd=ROOT, env=env)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    return np.load(os.path.join(d, "host.npz"))


@pytest.mark.parametrize("i", range(len(tc.CASES)), ids=CASE_IDS)
def test_host_and_device_agree(host, i):
    """f_unit and the corrected stress of the two backends: each is within its bound of the long-double restatement, and
    they are within one bound of each other"""
    etype, kind, aniso = tc.CASES[i]
    f, sigma0, sigma, mises = tc.run_backend(etype, kind, aniso, "mesh", "hip")
    ef = np.abs(f - host["f%d" % i]).max() / np.abs(host["f%d" % i]).max()
    size = max(np.abs(sigma0).max(), np.abs(sigma - sigma0).max())
    e0 = np.abs(sigma0 - host["s0%d" % i]).max() / size
    es = np.abs(sigma - host["s%d" % i]).max() / size
    em = np.abs(mises - host["m%d" % i]).max() / size
    print(f"{etype} {kind}: device against host: force {ef:.3e}, uncorrected stress {e0:.3e}, stress {es:.3e}, mises {em:.3e}")
    assert ef <= tc.FORCE_TOL
    # the uncorrected stress C : eps(u) of the two backends differs by its own rounding, which the correction inherits
    assert es <= tc.STRESS_TOL + e0 and em <= tc.STRESS_TOL + 2.0 * e0
