"""Damped explicit dynamics on the device: the scenarios of tests/explicit_damped_cases.py with backend "hip"."""
import pytest

import explicit_damped_cases as edc

pytestmark = pytest.mark.gpu
BACKEND = "hip"


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


def test_refusals():
    edc.refusals(BACKEND)


def test_comm_refusal():
    edc.comm_refusal(BACKEND)


@pytest.mark.parametrize("case,mode", edc.TRAJ_CASES)
def test_deck_trajectory(tmp_path, case, mode):
    edc.trajectory(tmp_path, case, mode, BACKEND)


@pytest.mark.parametrize("case", list(edc.TRAJ))
def test_deck_stable_dt(tmp_path, case):
    edc.stable_dt(tmp_path, case, BACKEND)
