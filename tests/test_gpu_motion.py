"""Prescribed motion in explicit dynamics on the device: the scenarios of tests/motion_cases.py with backend "hip"."""
import pytest

import motion_cases as mc
import motion_reference as mr

pytestmark = pytest.mark.gpu
BACKEND = "hip"
EDGES = [("CPS4", 9), ("C3D4", 16), ("C3D4", 17)]      # the exact comparisons: one mesh per family side of a workgroup edge


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


def test_comm_refusal():
    mc.comm_refusal(BACKEND)


@pytest.mark.parametrize("mode", ["fixed", "auto"])
def test_pulled_bar_through_the_deck_driver(tmp_path, monkeypatch, mode):
    reactions = mc.pulled_bar(tmp_path, BACKEND, monkeypatch, mode)
    assert all(r[0] * mc.PULL < 0 for r in reactions), reactions       # the sign opposes the pull


def test_a_deck_without_motion_is_unchanged(tmp_path):
    mc.plain_deck_is_unchanged(tmp_path, BACKEND)
