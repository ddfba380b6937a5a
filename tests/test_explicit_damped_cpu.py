"""Damped explicit dynamics on the host backend (tests/explicit_damped_cases.py), the reader's two keywords, and the measured
float64 constants the bounds of both backends rest on."""
import pytest

import explicit_damped_cases as edc

BACKEND = "cpu"


def test_f64_constants_are_the_measured_ones():
    worst = edc.measure_f64_worst()
    print(worst)
    for key, const in (("step", edc.F64_WORST_STEP), ("term", edc.F64_WORST_TERM), ("omega", edc.F64_WORST_OMEGA),
                       ("dilation", edc.F64_WORST_DILATION), ("rigid", edc.F64_WORST_RIGID)):
        assert worst[key] <= const <= 1.1 * worst[key] + 1e-17, (key, worst[key], const)
    for key, w in worst["traj"].items():
        assert w <= edc.F64_WORST_TRAJ[key] <= 1.1 * w + 1e-17, (key, w)


@pytest.mark.parametrize("name", edc.STEP_SHAPES)
def test_one_damped_step(name):
    edc.one_step(name, BACKEND)


@pytest.mark.parametrize("name", edc.TERM_SHAPES)
@pytest.mark.parametrize("which", list(edc.TERMS))
def test_each_term_alone(which, name):
    edc.term(which, name, BACKEND)


@pytest.mark.parametrize("mode", ["fixed", "auto"])
def test_zero_is_the_undamped_path(mode):
    edc.zero_is_undamped(mode, BACKEND)


def test_rigid_translation_under_alpha():
    edc.rigid(BACKEND)


@pytest.mark.parametrize("c", [-40.0, 40.0])
@pytest.mark.parametrize("etype", ["C3D4", "CPS3"])
def test_uniform_dilation(etype, c):
    edc.dilation(etype, c, BACKEND)


@pytest.mark.parametrize("ramp", [False, True])
@pytest.mark.parametrize("mode", ["fixed", "auto"])
def test_split_run(mode, ramp):
    edc.split(mode, ramp, BACKEND)


@pytest.mark.parametrize("name", edc.OMEGA_SHAPES)
def test_omega_eff(name):
    edc.omega_eff(name, BACKEND)


def test_reader(tmp_path):
    edc.reader(tmp_path)


def test_refusals():
    edc.refusals(BACKEND)


@pytest.mark.parametrize("case,mode", edc.TRAJ_CASES)
def test_deck_trajectory(tmp_path, case, mode):
    edc.trajectory(tmp_path, case, mode, BACKEND)


@pytest.mark.parametrize("case", list(edc.TRAJ))
def test_deck_stable_dt(tmp_path, case):
    edc.stable_dt(tmp_path, case, BACKEND)
