"""Prescribed motion in explicit dynamics on the host backend (tests/motion_cases.py), the reader's *Amplitude and *Boundary,
amplitude=, the driver's gate, and the measured float64 constants the bounds of both backends rest on."""
import pytest

import motion_cases as mc
import motion_reference as mr

BACKEND = "cpu"
EDGES = [("CPS4", 9), ("C3D4", 16), ("C3D4", 17)]      # the exact comparisons: one mesh per family side of a workgroup edge


def test_f64_constants_are_the_measured_ones():
    worst = mc.measure_f64_worst()
    print(worst)
    for case, w in worst["fixed"].items():
        assert w <= mc.F64_WORST_FIXED[case] <= 1.1 * w + 1e-17, (case, w)
    assert worst["start"] <= mc.F64_WORST_START <= 1.1 * worst["start"] + 1e-17, worst["start"]
    assert worst["auto"] <= mc.F64_WORST_AUTO <= 1.1 * worst["auto"] + 1e-17, worst["auto"]
    assert worst["amp"] <= mc.F64_WORST_AMP <= 1.1 * worst["amp"] + 1e-17, worst["amp"]


@pytest.mark.parametrize("kind", [mr.TABULAR, mr.SMOOTH_STEP])
def test_amplitude_at_and_around_every_point(kind):
    mc.amplitude_values(kind, BACKEND)


@pytest.mark.parametrize("family,nn", mc.MESHES)
@pytest.mark.parametrize("case", list(mc.FIXED))
def test_fixed_increment(case, family, nn):
    mc.fixed(case, family, nn, BACKEND)


@pytest.mark.parametrize("family,nn", mc.MESHES)
def test_element_by_element(family, nn):
    mc.auto(family, nn, BACKEND)


@pytest.mark.parametrize("family,nn", EDGES)
@pytest.mark.parametrize("case", ["tabular", "damped"])
def test_split_run(case, family, nn):
    mc.split(case, family, nn, BACKEND)


@pytest.mark.parametrize("family,nn", EDGES)
def test_split_automatic_run(family, nn):
    mc.auto_split(family, nn, BACKEND)


@pytest.mark.parametrize("family,nn", EDGES[:2])
def test_another_increment_counts_on(family, nn):
    mc.new_increment(family, nn, BACKEND)


@pytest.mark.parametrize("family,nn", EDGES)
@pytest.mark.parametrize("mode", ["fixed", "auto"])
def test_zero_values_leave_the_other_lanes_alone(mode, family, nn):
    mc.zero_values(mode, family, nn, BACKEND)


@pytest.mark.parametrize("family,nn", EDGES[:2])
@pytest.mark.parametrize("mode", ["fixed", "auto"])
def test_removed_motion_restores_the_bits(mode, family, nn):
    mc.removed(mode, family, nn, BACKEND)


def test_refusals():
    mc.refusals(BACKEND)


def test_reader(tmp_path):
    mc.reader(tmp_path)


def test_gate():
    mc.gate(BACKEND)


@pytest.mark.parametrize("mode", ["fixed", "auto"])
def test_pulled_bar_through_the_deck_driver(tmp_path, monkeypatch, mode):
    reactions = mc.pulled_bar(tmp_path, BACKEND, monkeypatch, mode)
    assert all(r[0] * mc.PULL < 0 for r in reactions), reactions       # the sign opposes the pull


def test_a_deck_without_motion_is_unchanged(tmp_path):
    mc.plain_deck_is_unchanged(tmp_path, BACKEND)
