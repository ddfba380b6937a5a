"""Fixed mass scaling on the host backend (tests/mass_scaling_cases.py), the reader's keyword, and the measured float64
constants the bounds of both backends rest on."""
import pytest

import mass_scaling_cases as mc

BACKEND = "cpu"


@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    return str(tmp_path_factory.mktemp("mass_scaling_ref"))


def test_f64_constants_are_the_measured_ones(workdir):
    worst = mc.measure_f64_worst(workdir)
    print(worst)
    for key, const in (("scale", mc.F64_WORST_SCALE), ("after", mc.F64_WORST_AFTER), ("compound", mc.F64_WORST_COMPOUND)):
        assert worst[key] <= const <= 1.1 * worst[key] + 1e-17, (key, worst[key], const)
    for key, consts in (("pair", mc.F64_WORST_PAIR), ("graded", mc.F64_WORST_GRADED)):
        for mode, w in worst[key].items():
            assert w <= consts[mode] <= 1.1 * w + 1e-17, (key, mode, w)


@pytest.mark.parametrize("name,kind,factor", mc.FACTOR_CASES)
def test_factors_and_masses(name, kind, factor):
    mc.call(name, kind, factor, BACKEND)


@pytest.mark.parametrize("name,kind,factor", mc.EDGE_CASES)
def test_kernel_edges(name, kind, factor):
    mc.call(name, kind, factor, BACKEND)


@pytest.mark.parametrize("name", mc.AFTER_SHAPES)
def test_estimates_afterwards(name):
    mc.after(name, BACKEND)


def test_same_bits_and_compounding():
    mc.same_bits_and_compounding(BACKEND)


@pytest.mark.parametrize("mode", ["fixed", "auto"])
def test_factor_is_a_denser_material(tmp_path, mode, workdir):
    mc.denser_material(tmp_path, mode, BACKEND, workdir)


@pytest.mark.parametrize("mode", ["fixed", "auto"])
def test_graded_bar(tmp_path, mode, workdir):
    mc.graded(tmp_path, mode, BACKEND, workdir)


def test_reader(tmp_path):
    mc.reader(tmp_path, BACKEND)


def test_refusals():
    mc.refusals(BACKEND)


def test_broken_element():
    mc.broken_element(BACKEND)
