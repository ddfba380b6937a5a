"""Implicit dynamics on the host backend: the mass rule, the reader, the C ABI of femcy_mass_* / femcy_newmark_* and the
driver of `*Dynamic` decks (tests/dynamic_cases.py holds the scenarios, shared with tests/test_gpu_dynamic.py)."""
import itertools
import math
import os

import numpy as np
import pytest

from femcy_amd import backend as be
from femcy_amd.reader import InpInfo
from femcy_amd.reader.inp_info_base import InpInfoBase

import dynamic_cases as dc
import loads_cases as lc
import loads_reference as lr
import thermal_cases as tc

BACKEND = "cpu"
pytestmark = pytest.mark.skipif(not os.path.exists(be.CPU_LIB_PATH), reason="libfemcy_cpu.so has not been built")


# ------------------------------------------------------------------------------------------ mass rule
@pytest.mark.parametrize("etype", lr.ETYPES)
def test_mass_rule_integrates_every_required_monomial(etype):
    """exact integrals: prod k_i! / (sum k_i + d)! on the unit simplex, prod (1 + (-1)^k) / (k + 1) on [-1, 1]^d"""
    ELE = lr.single(etype)[2]
    pts, w = ELE.mass_rule()
    p, dm, shape = ELE._order, ELE.dm, ELE._parent_shape
    assert (w > 0).all() and len(w) <= 36
    line = lambda k: (1 + (-1) ** k) / (k + 1)
    worst = 0.0
    for ex in itertools.product(range(2 * p + 1), repeat=dm):
        tri = ex[:2] if shape == "wedge" else (ex if shape == "simplex" else ())
        if sum(tri) > 2 * p:
            continue
        if shape == "cube":
            exact = math.prod(line(k) for k in ex)
        else:
            exact = math.prod(math.factorial(k) for k in tri) / math.factorial(sum(tri) + len(tri))
            if shape == "wedge":
                exact *= line(ex[2])
        worst = max(worst, abs(float((w * np.prod(pts ** np.array(ex), axis=1)).sum()) - exact))
    assert worst <= 1e-14, worst
    if etype == "C3D10":
        assert len(w) == 36


def test_the_stiffness_rule_under_integrates_the_c3d10_mass():
    nodes, el, ELE, _ = lr.single("C3D10")
    N = ELE.tables()["N"]
    assert np.linalg.matrix_rank(N.T @ N) == 4
    Nq = ELE.mass_tables()["Nq"]
    assert np.linalg.matrix_rank(Nq.T @ np.diag(ELE.mass_tables()["wq"]) @ Nq) == 10


# --------------------------------------------------------------------------------------------- reader
def _flight_deck(tmp_path, name="d.inp", **kw):
    nodes, el, _ = tc.family_mesh("C3D8")
    path = os.path.join(str(tmp_path), name)
    kw.setdefault("step", "*Dload\n, GRAV, 9.81, 0., 0., -1.\n")
    dc.write_dynamic_deck(path, nodes, el, "C3D8", {"all": np.arange(len(nodes)), "one": np.array([0])}, **kw)
    return path


def test_dynamic_step_is_read(tmp_path):
    inp = InpInfo(_flight_deck(tmp_path, dynamic="*Dynamic, direct\n0.05, 1.\n",
                               initial="*Initial Conditions, type=VELOCITY\nall, 3, 2.5\n7, 1, -1.\n"))
    assert inp.procedure == "dynamic" and inp.dynamic == {"beta": 0.25, "gamma": 0.5} and inp.amplitude == "STEP"
    assert inp.time_incs["ini_inc"] == inp.time_incs["max_inc"] == 0.05 and inp.time_incs["max_time"] == 1.0
    iv = inp.initial_velocity_info
    assert len(iv) == 2 and iv[0]["dof"] == 2 and iv[0]["val"] == 2.5 and len(iv[0]["node_set"]) == len(inp.nodes)
    assert iv[1]["dof"] == 0 and list(iv[1]["node_set"]) == [6] and iv[1]["val"] == -1.0
    for attr in ("procedure", "dynamic", "amplitude", "initial_velocity_info"):
        assert attr in InpInfoBase.ATTRIBUTES
    damped = InpInfo(_flight_deck(tmp_path, "b.inp", dynamic="*Dynamic, direct, beta=0.3025, gamma=0.6\n0.05, 1.\n", amplitude="RAMP"))
    assert damped.dynamic == {"beta": 0.3025, "gamma": 0.6} and damped.amplitude == "RAMP"


@pytest.mark.parametrize("dynamic", [None, "*Dynamic, direct\n0.05, 1.\n"])
@pytest.mark.parametrize("nlgeom", ["NO", "YES"])
def test_nlgeom_is_read_wherever_it_stands(tmp_path, dynamic, nlgeom):
    """`*Step, name=, nlgeom=, amplitude=`: the new parameter may follow nlgeom, under *Static and under *Dynamic.  Any
    other trailing parameter still makes the step nlgeom, the reference's rule that test_reader_quirks pins."""
    kw = dict(step="*Dload\n, GRAV, 9.81, 0., 0., -1.\n")
    if dynamic is None:
        path = os.path.join(str(tmp_path), "s.inp")
        tc.write_thermal_deck(path, "C3D8", "free")
    else:
        path = _flight_deck(tmp_path, dynamic=dynamic, **kw)
    text = open(path).read()
    old = text[text.index("*Step, name=Step-1"):].split("\n")[0]
    for order in ("*Step, name=Step-1, nlgeom=%s, amplitude=STEP" % nlgeom, "*Step, name=Step-1, amplitude=RAMP, nlgeom=%s" % nlgeom, "*Step, name=Step-1, nlgeom=%s , amplitude=STEP" % nlgeom,
                  "*Step, name=Step-1, amplitude=STEP, nlgeom=%s" % nlgeom, "*Step, name=Step-1, nlgeom=%s" % nlgeom):
        with open(path, "w") as f:
            f.write(text.replace(old, order))
        inp = InpInfo(path)
        assert inp.geometric_nonlinear == (nlgeom == "YES"), order
        assert inp.procedure == ("static" if dynamic is None else "dynamic")
        want = "RAMP" if "RAMP" in order else ("STEP" if "STEP" in order or dynamic else "RAMP")
        assert inp.amplitude == want, order
    with open(path, "w") as f:
        f.write(text.replace(old, "*Step, name=Step-1, nlgeom=%s, inc=100, amplitude=RAMP" % nlgeom))
    assert InpInfo(path).geometric_nonlinear is True              # the reference's last-field rule, amplitude= aside


def test_a_static_solve_after_a_dynamic_one_reports_the_reference_energy(tmp_path):
    from femcy_amd.body import Body
    from femcy_amd.stiffnessMtrx import System_of_equations
    dyn = InpInfo(_flight_deck(tmp_path))
    body = Body(nodes=dyn.nodes, elements=list(dyn.eSets.values())[0], ELE=dyn.ELE)
    system = System_of_equations(body, list(dyn.materials.values())[0], False, verbose=False, ctx=be.Context(0, backend=BACKEND))
    system.solve(dyn)
    assert system._linear_energy
    path = os.path.join(str(tmp_path), "s.inp")
    tc.write_thermal_deck(path, "C3D8", "free")
    system.time0 = system.time1 = 0.0
    log = dc.CallLog(system.ctx)
    system.solve(InpInfo(path))
    system.get_elasEng()
    system.ctx.close()
    assert not system._linear_energy and log.calls[-1] == "femcy_elastic_energy"


def test_static_decks_read_as_before(tmp_path):
    path = os.path.join(str(tmp_path), "s.inp")
    tc.write_thermal_deck(path, "C3D8", "free")
    inp = InpInfo(path)
    assert inp.procedure == "static" and inp.dynamic is None and inp.amplitude == "RAMP" and inp.initial_velocity_info == []
    assert inp.time_incs == {"ini_inc": 1.0, "max_time": 1.0, "min_inc": 1e-05, "max_inc": 1.0}


@pytest.mark.parametrize("kw, message", [
    (dict(dynamic="*Dynamic\n0.05, 1.\n"), "without `direct`"),
    (dict(dynamic="*Dynamic, direct, alpha=-0.05\n0.05, 1.\n"), "alpha=-0.05"),
    (dict(dynamic="*Dynamic, direct, beta=0.\n0.05, 1.\n"), "beta = 0.0"),
    (dict(dynamic="*Dynamic, direct, gamma=0.4\n0.05, 1.\n"), "gamma = 0.4"),
    (dict(material="*Elastic\n2e5, 0.3\n", step=""), "needs a \\*Density"),
    (dict(step="*Boundary\none, 1, 1, 0.01\n"), "non-zero \\*Boundary"),
    (dict(amplitude="SMOOTH"), "amplitude=SMOOTH"),
])
def test_reader_refusals(tmp_path, kw, message):
    with pytest.raises(ValueError, match=message):
        InpInfo(_flight_deck(tmp_path, **kw))


def test_solve_refuses_nlgeom_and_neo_hooke_before_solving(tmp_path):
    from femcy_amd.body import Body
    from femcy_amd.stiffnessMtrx import System_of_equations
    for kw, message in ((dict(nlgeom=True), "nlgeom=YES"),
                        (dict(material="*Density\n1e-3,\n*Hyperelastic, neo hooke\n80., 2.5e-3\n"), "neo-Hookean")):
        inp = InpInfo(_flight_deck(tmp_path, **kw))
        body = Body(nodes=inp.nodes, elements=list(inp.eSets.values())[0], ELE=inp.ELE)
        system = System_of_equations(body, list(inp.materials.values())[0], inp.geometric_nonlinear, verbose=False,
                                     ctx=be.Context(0, backend=BACKEND))
        with pytest.raises(ValueError, match=message):
            system.solve(inp)
        assert system.stats["linear_solves"] == 0 and system.stats["assemblies"] == 0
        system.ctx.close()


def test_main_refuses_several_ranks(tmp_path, monkeypatch):
    from femcy_amd import distributed, main
    monkeypatch.setattr(distributed, "wanted", lambda: True)
    with pytest.raises(ValueError, match="more than one rank"):
        main.run(_flight_deck(tmp_path), verbose=False)


def test_a_static_deck_makes_the_calls_it_made(tmp_path):
    """the sequence of ABI calls of a static deck with every load kind, recorded through a wrapper: none of the new entry
    points, and the same sequence as the static branch written out (what the parent made)"""
    path = os.path.join(str(tmp_path), "s.inp")
    tc.write_thermal_deck(path, "C3D8", "bar", static="0.5, 1., 1e-05, 0.5", extra_step="*Cload\nB, 2, 3.\n*Dload\n, BX, 2.\n")
    from femcy_amd.body import Body
    from femcy_amd.stiffnessMtrx import System_of_equations
    inp = InpInfo(path)
    body = Body(nodes=inp.nodes, elements=list(inp.eSets.values())[0], ELE=inp.ELE)
    system = System_of_equations(body, list(inp.materials.values())[0], False, verbose=False, ctx=be.Context(0, backend=BACKEND))
    log = dc.CallLog(system.ctx)
    system.solve(inp)
    system.ctx.close()
    assert not [c for c in log.calls if "mass" in c or "newmark" in c]
    nbc = len(inp.dirichlet_bc_info)
    inc = (["femcy_assemble_K", "femcy_vec_fill", "femcy_bodyload_apply", "femcy_dofset_add", "femcy_thermal_apply"]
           + ["femcy_dofset_dirichlet_linear"] * nbc + ["femcy_direct_plan", "femcy_direct_solve", "femcy_vec_copy", "femcy_vec_copy", "femcy_vec_copy"])
    first = [c for c in log.calls if c not in ("femcy_dofset_create", "femcy_bodyload_create", "femcy_sync")]
    want = ["femcy_thermal_create"] + inc + [c for c in inc if c != "femcy_direct_plan"]
    assert first == want, first


# ------------------------------------------------------------------------------------------------ ABI
@pytest.mark.parametrize("etype", ["C3D4", "CPS3"])
def test_single_element_mass(etype):
    dc.single_element(etype, BACKEND)


@pytest.mark.parametrize("name", list(dc.SHAPES))
def test_mass_properties(name):
    dc.mass_properties(name, BACKEND)


@pytest.mark.parametrize("name", list(dc.SHAPES))
def test_mass_apply(name):
    dc.mass_apply(name, BACKEND)


@pytest.mark.parametrize("name", ["CPS4-65", "C3D8-64", "C3D10", "CPS4-130"])
def test_mass_add_to_K(name):
    dc.add_to_K(name, BACKEND)


@pytest.mark.parametrize("name", ["CPS4-63", "C3D8-64", "CPS4-65"])
def test_newmark_kernels(name):
    dc.newmark_kernels(name, BACKEND)


def test_refusals():
    dc.refusals(BACKEND)


@pytest.mark.parametrize("name", dc.ENERGY_SHAPES)
def test_small_strain_energy_is_the_quadratic_form(name):
    dc.small_energy(name, BACKEND)


def test_small_strain_energy_refuses_neo_hooke():
    dc.small_energy_refusal(BACKEND)


# ---------------------------------------------------------------------------------------------- decks
@pytest.mark.parametrize("family", dc.FAMILIES)
def test_free_flight(tmp_path, family):
    dc.free_flight(tmp_path, family, BACKEND)


def test_energy_is_conserved(tmp_path):
    dc.energy(tmp_path, BACKEND)


@pytest.mark.parametrize("case", list(dc.TRAJ))
def test_trajectory(tmp_path, case):
    dc.trajectory(tmp_path, case, BACKEND)


@pytest.mark.parametrize("case", ["cload", "damped"])
def test_trajectory_on_the_pcg_branch(tmp_path, case):
    dc.trajectory_pcg(tmp_path, case, BACKEND)


def test_the_float64_restatement_stays_within_its_constants(tmp_path):
    w = dc.measure_f64_worst(str(tmp_path))
    print(w)
    assert w["mass"] <= dc.F64_WORST_MASS and w["apply"] <= dc.F64_WORST_APPLY and w["flight"] <= dc.F64_WORST_FLIGHT
    assert w["energy"] <= dc.F64_WORST_ENERGY and w["traj"] <= dc.F64_WORST_TRAJ
    assert w["small_energy"] <= dc.F64_WORST_SMALL_ENERGY


def test_main_runs_a_dynamic_deck(tmp_path, monkeypatch, capsys):
    from femcy_amd import main
    monkeypatch.setenv("FEMCY_BACKEND", BACKEND)
    inp, system = main.run(_flight_deck(tmp_path), verbose=False)
    assert len(system.increments) == 8 and {"kinetic", "strain_energy"} <= set(system.increments[-1])
    system.ctx.close()
