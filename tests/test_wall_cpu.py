"""Frictionless rigid walls of explicit dynamics on the host backend: the scenarios of tests/wall_cases.py with backend "cpu"."""
import pytest

import wall_cases as wc

BACKEND = "cpu"


def test_f64_worst_is_the_measured_one():
    got = wc.measure_f64_worst()
    print(got)
    worst = max(got.values())
    assert 0.5 * wc.F64_WORST <= worst <= wc.F64_WORST, got


def test_f64_worst_of_the_driver_is_the_measured_one():
    got = wc.measure_f64_worst_driver()
    print(got)
    for key, worst in got.items():
        assert 0.5 * wc.F64_WORST_DRIVER[key] <= worst <= wc.F64_WORST_DRIVER[key], got


@pytest.mark.parametrize("family", wc.FAMILIES)
@pytest.mark.parametrize("which", ["oblique", "corner"])
def test_force_law(family, which):
    wc.law_case(family, which, BACKEND)


@pytest.mark.parametrize("mode,variant,family,damping", wc.TRAJ_CASES)
def test_trajectory(mode, variant, family, damping):
    wc.trajectory(mode, variant, family, damping, BACKEND)


@pytest.mark.parametrize("family", wc.FAMILIES)
def test_wall_get_in_contact(family):
    wc.in_contact(family, BACKEND)


@pytest.mark.parametrize("mode", ["fixed", "auto"])
@pytest.mark.parametrize("energy", [False, True])
def test_split_run(mode, energy):
    wc.split(mode, energy, BACKEND)


@pytest.mark.parametrize("mode,how", [("fixed", "removed"), ("auto", "removed"), ("fixed", "unreached")])
def test_no_wall_bits(mode, how):
    wc.no_wall_bits(mode, how, BACKEND)


@pytest.mark.parametrize("family", wc.FAMILIES)
@pytest.mark.parametrize("damping", ["none", "both"])
def test_element_bound(family, damping):
    wc.bound(family, damping, BACKEND)


@pytest.mark.parametrize("nn", [7, 8, 9, 255, 256, 257, 513])
def test_shape(nn):
    wc.shape(nn, BACKEND)


@pytest.mark.parametrize("k", [33, 65])
def test_hub_in_contact(k):
    wc.fan(k, BACKEND)


@pytest.mark.parametrize("etype", ["CPS3", "C3D4"])
def test_single_element(etype):
    wc.single(etype, BACKEND)


@pytest.mark.parametrize("family", wc.FAMILIES)
def test_driver_energy(tmp_path, family):
    wc.driver_energy(tmp_path, family, BACKEND)


def test_four_walls():
    wc.four_walls(BACKEND)


def test_refusals():
    wc.refusals(BACKEND)


def test_reader(tmp_path):
    wc.reader(tmp_path)


def test_deck():
    wc.deck(BACKEND)


def test_deck_through_main(monkeypatch):
    from femcy_amd import main
    monkeypatch.setenv("FEMCY_BACKEND", BACKEND)
    assert main.main([wc.DECK, "--quiet"]) in (0, None)


def test_driver_increment(tmp_path):
    wc.driver_increment(tmp_path, BACKEND)
