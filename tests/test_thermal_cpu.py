"""*Expansion / *Initial Conditions, type=TEMPERATURE / *Temperature without a GPU: the reader, the restatement's own
constants, and the host backend (libfemcy_cpu.so, the same per-element functions as the device kernels) through
tests/thermal_cases.py."""
import glob
import os

import numpy as np
import pytest

import loads_cases as lc
import loads_reference as lr
import thermal_cases as tc
import thermal_reference as tr
from femcy_amd.reader import InpInfo
from femcy_amd.reader.inp_info_base import InpInfoBase

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DECKS = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "decks", "*.inp")))
EXP = "*Expansion\n1.2e-5,\n"
ELAS = "*Elastic\n2e5, 0.3\n"


# ------------------------------------------------------------------------------------------ reader
def _deck(tmp_path, etype="C3D8", material=ELAS, step="", name="d.inp"):
    nodes, el = lc.bar_mesh(etype)
    path = str(tmp_path / name)
    nsets = {"foot": np.nonzero(nodes[:, -1] < 1e-12)[0], "tip": np.nonzero(nodes[:, -1] > lc.LEN - 1e-12)[0],
             "all": np.arange(len(nodes))}
    lc.write_deck(path, nodes, el, etype, nsets, material, "*Boundary\nfoot, 1, 1\n" + step)
    return path, nodes, el


def test_expansion_is_not_the_material_type(tmp_path):
    """before *Elastic the parent's reader took *Expansion for the material type and refused it"""
    plain = InpInfo(_deck(tmp_path, name="a.inp")[0])
    first = InpInfo(_deck(tmp_path, material=EXP + ELAS, name="b.inp")[0])
    last = InpInfo(_deck(tmp_path, material=ELAS + "*Expansion, zero=20.\n1.2e-5\n", name="c.inp")[0])
    both = InpInfo(_deck(tmp_path, material="*Density\n7.8e-3,\n" + EXP + ELAS, name="d2.inp")[0])
    assert plain.expansion is None and plain.temperature_info is None
    for inp in (first, last, both):
        assert inp.expansion == 1.2e-5 and isinstance(inp.expansion, float) and inp.temperature_info is None
        assert list(inp.materials) == list(plain.materials) == ["Elastic"]
        assert np.array_equal(inp.materials["Elastic"].C, plain.materials["Elastic"].C)
    assert both.density == 7.8e-3
    flat = InpInfo(_deck(tmp_path, "CPS4", material=EXP + ELAS, name="e.inp")[0])
    assert flat.expansion == 1.2e-5 and list(flat.materials) == ["Elastic"]
    for attr in ("expansion", "temperature_info"):
        assert attr in InpInfoBase.ATTRIBUTES


def test_temperatures_are_read(tmp_path):
    """node-set and bare-label lines; a node *Temperature does not name keeps its initial value, a missing one is 0"""
    mat = ELAS + EXP + "*Initial Conditions, type=TEMPERATURE\nfoot, 20.\n7, 35.5\n"
    path, nodes, _ = _deck(tmp_path, material=mat, step="*Temperature\ntip, 120.\n3, -4.\n")
    inp = InpInfo(path)
    foot, tip = np.nonzero(nodes[:, 2] < 1e-12)[0], np.nonzero(nodes[:, 2] > lc.LEN - 1e-12)[0]
    ini = np.zeros(len(nodes))
    ini[foot] = 20.0
    ini[6] = 35.5                                                  # label 7 -> position 6
    fin = ini.copy()
    fin[tip] = 120.0
    fin[2] = -4.0
    assert sorted(inp.temperature_info) == ["final", "initial"]
    assert inp.temperature_info["initial"].dtype == np.float64 and np.array_equal(inp.temperature_info["initial"], ini)
    assert np.array_equal(inp.temperature_info["final"], fin)
    only_initial = InpInfo(_deck(tmp_path, material=ELAS + "*Initial Conditions, type=TEMPERATURE\nall, 20.\n", name="i.inp")[0])
    assert np.array_equal(only_initial.temperature_info["final"], np.full(len(nodes), 20.0)) and only_initial.expansion is None
    other = InpInfo(_deck(tmp_path, material=ELAS + "*Initial Conditions, type=STRESS\nall, 1., 2., 3.\n", name="o.inp")[0])
    assert other.temperature_info is None                          # any other type is left alone


@pytest.mark.parametrize("material,step,word", [
    (ELAS + "*Expansion, type=ORTHO\n1e-5, 2e-5, 3e-5\n", "", "ORTHO"),
    (ELAS + "*Expansion, type=ANISO\n1e-5, 2e-5, 3e-5, 0., 0., 0.\n", "", "ANISO"),
    (ELAS + "*Expansion\n1e-5, 20.\n2e-5, 100.\n", "", "temperature-dependent"),
    (ELAS + "*Expansion\n1e-5, 20.\n", "", "temperature-dependent"),
    (ELAS + "*Expansion\n", "", "data line"),
    (ELAS, "*Temperature\nall, 100.\n", r"\*Temperature needs an \*Expansion"),
    (ELAS + EXP, "*Temperature\nnowhere, 100.\n", "nowhere"),
    (ELAS + EXP, "*Temperature\n7777, 100.\n", "no node with label 7777"),
    (ELAS + EXP + "*Initial Conditions, type=TEMPERATURE\nnowhere, 1.\n", "", "nowhere"),
    (ELAS + EXP, "*Temperature\nall\n", "nset-or-node, T"),
])
def test_reader_refusals(tmp_path, material, step, word):
    with pytest.raises(ValueError, match=word):
        InpInfo(_deck(tmp_path, material=material, step=step)[0])


@pytest.mark.parametrize("path", DECKS, ids=[os.path.basename(p) for p in DECKS])
def test_shipped_decks_have_no_thermal_load(path):
    text = open(path).read().lower()
    assert "*expansion" not in text and "*temperature" not in text
    inp = InpInfo(path)
    assert inp.expansion is None and inp.temperature_info is None


def test_a_deck_without_the_keywords_makes_the_calls_it_made(tmp_path):
    """spy on the context calls of impose_boundary_condition and compute_strain_stress: no thermal entry point is
    reached without the keywords, and with them the load is applied after the *Cload and before the Dirichlet treatment"""
    from femcy_amd import backend as be
    seen = []
    orig = be.Context._call

    def spy(self, name, *args):
        seen.append(name)
        return orig(self, name, *args)

    path, hot = str(tmp_path / "cold.inp"), str(tmp_path / "hot.inp")
    tc.write_thermal_deck(path, "C3D8", "bar", thermal=False, extra_step="*Cload\nB, 2, 2.\n")
    tc.write_thermal_deck(hot, "C3D8", "bar", extra_step="*Cload\nB, 2, 2.\n")
    be.Context._call = spy
    try:
        inp, system, _, _, _ = tc.solve_thermal_deck(path, "cpu")
        cold = list(seen)
        del seen[:]
        tc.solve_thermal_deck(hot, "cpu")
    finally:
        be.Context._call = orig
    assert inp.expansion is None and inp.temperature_info is None and system._thermal is None
    assert not any("thermal" in n for n in cold)
    assert [n for n in seen if "thermal" not in n] == cold       # the same calls in the same order, plus the new ones
    assert [n for n in seen if "thermal" in n] == ["femcy_thermal_create", "femcy_thermal_apply", "femcy_thermal_stress"]
    i = seen.index("femcy_thermal_apply")
    before, after = seen[:i], seen[i + 1:]
    assert "femcy_dofset_add" in before and "femcy_dofset_add" not in after                  # after the *Cload loop
    first = next(k for k, n in enumerate(seen) if "dirichlet" in n)
    assert first > i, seen                                                                     # before the Dirichlet treatment


def test_local_deck_hands_over_the_rank_temperatures(tmp_path):
    from femcy_amd import partition
    from femcy_amd.body import Body
    mat = ELAS + EXP + "*Initial Conditions, type=TEMPERATURE\nall, 20.\n"
    path, nodes, el = _deck(tmp_path, "C3D4", material=mat, step="*Temperature\ntip, 90.\n5, 33.\n")
    inp = InpInfo(path)
    for p in partition.build_all_parts(inp.nodes, el, 2, axis=2):
        deck = partition.LocalDeck(inp, p, Body(p.nodes, p.elements, inp.ELE))
        assert deck.expansion == 1.2e-5
        for key in ("initial", "final"):
            assert np.array_equal(deck.temperature_info[key], inp.temperature_info[key][p.l2g])
    cold = InpInfo(_deck(tmp_path, "C3D4", name="cold.inp")[0])
    p = partition.build_all_parts(cold.nodes, el, 2, axis=2)[0]
    deck = partition.LocalDeck(cold, p, Body(p.nodes, p.elements, cold.ELE))
    assert deck.expansion is None and deck.temperature_info is None


# ----------------------------------------------------------------------------------- the restatement
def test_the_float64_restatement_stays_within_its_constants():
    """F64_WORST_FORCE / F64_WORST_STRESS of thermal_cases are the float64 restatement's worst errors against the
    long-double one; the bounds of every kernel check are 4 x these"""
    assert np.finfo(np.longdouble).eps < 1e-18                    # an extended type, not an alias of float64
    wf, ws = tc.measure_f64_worst()
    print(f"float64 restatement against long double: force {wf:.3e}, stress {ws:.3e}")
    assert wf <= tc.F64_WORST_FORCE and ws <= tc.F64_WORST_STRESS
    assert tc.F64_WORST_FORCE <= 2.0 * wf and tc.F64_WORST_STRESS <= 2.0 * ws     # and they are not padded


@pytest.mark.parametrize("etype", lr.ETYPES)
def test_restatement_closed_form_uniform_field(etype):
    """a uniform temperature change on one straight-sided element: the loads of every node sum to zero, and the nodal
    load is sigma_th times the integral of grad N_a, which the rule integrates exactly there"""
    nodes, el, ELE, V = lr.single(etype)
    kind = tc.KIND_OF["CPS" if ELE.dm == 2 else "C3D"]
    mat = tc.material(kind)
    f = tr.thermal_force(nodes, el, ELE, mat.C, kind, tc.NU, tc.ALPHA, np.full(len(nodes), 50.0), np.longdouble)
    f = f.reshape(-1, ELE.dm)
    size = np.abs(f).max()
    assert size > 0 and np.abs(f.sum(axis=0)).max() <= 1e-17 * size * len(nodes)
    # virtual work with the linear field v = x: sum_a f_a . x_a = integral of tr(sigma_th) = dm * s * V
    s = tc.ALPHA * 50.0 * float(tr.unit_stress(mat.C, kind, tc.NU, np.longdouble)[0, 0])
    assert abs(float((f * nodes).sum()) - ELE.dm * s * V) <= 1e-13 * ELE.dm * s * V


# ------------------------------------------------------------------------------------ host backend
@pytest.mark.parametrize("etype,kind,aniso", tc.CASES, ids=["%s-%s%s" % (e, k, "-aniso" if a else "") for e, k, a in tc.CASES])
def test_host_matches_the_restatement(etype, kind, aniso):
    tc.against_restatement(etype, kind, aniso, "mesh", "cpu")


@pytest.mark.parametrize("etype", lr.ETYPES)
def test_host_single_element_and_small_mesh(etype):
    for which in ("single", "small"):
        tc.against_restatement(etype, tc.KIND_OF[etype[:3]], False, which, "cpu")


def test_host_fan_zero_field_and_bits():
    tc.against_restatement("CPS3", tr.PSTRESS, False, "fan", "cpu")
    tc.zero_field_and_bits("cpu")


def test_host_apply_and_refusals():
    tc.apply("cpu")
    tc.refusals("cpu")


@pytest.mark.parametrize("case", ["free", "bar"])
@pytest.mark.parametrize("family", tc.FAMILIES)
def test_closed_forms_on_the_host(tmp_path, family, case):
    err = tc.closed_form(tmp_path, family, case, "cpu")
    assert 10.0 * err <= tc.DECK_TOL                               # the measured value itself has that room


@pytest.mark.parametrize("family", tc.QUADRATIC)
def test_gradient_on_the_host(tmp_path, family):
    err = tc.closed_form(tmp_path, family, "gradient", "cpu")
    assert 10.0 * err <= tc.DECK_TOL


@pytest.mark.parametrize("family", ["C3D8", "CPE4"])
def test_half_increment_on_the_host(tmp_path, family):
    tc.half_increment(tmp_path, family, "cpu")


def test_expansion_before_elastic_gives_the_same_answer(tmp_path):
    a, b = str(tmp_path / "a.inp"), str(tmp_path / "b.inp")
    tc.write_thermal_deck(a, "C3D8", "bar", expansion_first=False)
    tc.write_thermal_deck(b, "C3D8", "bar", expansion_first=True)
    assert np.array_equal(tc.solve_thermal_deck(a, "cpu")[2][-1], tc.solve_thermal_deck(b, "cpu")[2][-1])


def test_nlgeom_with_a_thermal_load_is_refused_before_anything_is_solved(tmp_path):
    from femcy_amd import backend as be
    path = str(tmp_path / "nl.inp")
    tc.write_thermal_deck(path, "C3D8", "free", nlgeom=True)
    seen = []
    orig = be.Context._call

    def spy(self, name, *args):
        seen.append(name)
        return orig(self, name, *args)

    be.Context._call = spy
    try:
        with pytest.raises(ValueError, match="nlgeom"):
            tc.solve_thermal_deck(path, "cpu")
    finally:
        be.Context._call = orig
    assert not any(n in ("femcy_assemble_K", "femcy_direct_solve", "femcy_pcg", "femcy_residual_and_K") for n in seen)
