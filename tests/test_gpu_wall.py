"""Frictionless rigid walls of explicit dynamics on the device: the scenarios of tests/wall_cases.py with backend "hip"."""
import pytest

import wall_cases as wc

pytestmark = pytest.mark.gpu
BACKEND = "hip"


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


def test_comm_refusal():
    wc.comm_refusal(BACKEND)


def test_deck():
    wc.deck(BACKEND)


def test_deck_through_main(monkeypatch):
    from femcy_amd import main
    monkeypatch.setenv("FEMCY_BACKEND", BACKEND)
    assert main.main([wc.DECK, "--quiet"]) in (0, None)


def test_driver_increment(tmp_path):
    wc.driver_increment(tmp_path, BACKEND)
