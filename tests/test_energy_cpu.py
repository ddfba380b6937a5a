"""The energy balance of explicit dynamics on the host backend (tests/energy_cases.py), the reader's keyword, and the
measured float64 constant the bounds of both backends rest on."""
import pytest

import energy_cases as enc

BACKEND = "cpu"


def test_f64_constant_is_the_measured_one():
    worst = enc.measure_f64_worst()
    print(worst)
    w = max(worst.values())
    assert w <= enc.F64_WORST <= 1.1 * w + 1e-17, (worst, enc.F64_WORST)


def test_reader(tmp_path):
    enc.reader(tmp_path)


@pytest.mark.parametrize("key,damping,ramp", enc.FIXED_CASES)
def test_fixed_run(key, damping, ramp):
    enc.fixed(key, damping, ramp, BACKEND)


@pytest.mark.parametrize("key,damping", enc.IDENTITY_CASES)
def test_identity(key, damping):
    enc.identity(key, damping, BACKEND)


@pytest.mark.parametrize("case,family,nn", enc.MOTION_CASES)
def test_with_motion(case, family, nn):
    enc.motion(case, family, nn, BACKEND)


@pytest.mark.parametrize("family,nn", enc.AUTO_CASES)
def test_element_by_element(family, nn):
    enc.auto(family, nn, BACKEND)


@pytest.mark.parametrize("damping", ["none", "both"])
def test_on_does_not_disturb_a_fixed_run(damping):
    enc.undisturbed_fixed("C3D4-150", damping, BACKEND)


@pytest.mark.parametrize("mode", ["fixed", "auto"])
def test_on_does_not_disturb_a_run_with_motion(mode):
    enc.undisturbed_motion(mode, "C3D4", 9, BACKEND)


@pytest.mark.parametrize("damping", ["none", "both"])
def test_split_fixed_run(damping):
    enc.split_fixed("C3D4-150", damping, BACKEND)


def test_split_run_with_motion():
    enc.split_motion("CPS4", 9, BACKEND)


def test_rigid_translation():
    enc.rigid(BACKEND)


def test_refusals():
    enc.refusals(BACKEND)


def test_driver(tmp_path):
    enc.driver(tmp_path, BACKEND)
