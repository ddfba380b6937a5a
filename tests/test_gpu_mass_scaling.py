"""Fixed mass scaling on the device: the scenarios of tests/mass_scaling_cases.py with backend "hip"."""
import os

import pytest

from femcy_amd import backend as be

import mass_scaling_cases as mc

pytestmark = pytest.mark.gpu
BACKEND = "hip"


@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    return str(tmp_path_factory.mktemp("mass_scaling_ref"))


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


@pytest.mark.skipif(not os.path.exists(be.CPU_LIB_PATH), reason="libfemcy_cpu.so has not been built")
@pytest.mark.parametrize("mode", ["fixed", "auto"])
def test_host_against_device(tmp_path, mode, workdir):
    mc.host_against_device(tmp_path, mode, workdir)


def test_deck_without_the_keyword(tmp_path):
    mc.reader(tmp_path, BACKEND)


def test_refusals():
    mc.refusals(BACKEND)


def test_broken_element():
    mc.broken_element(BACKEND)


def test_comm_refusal():
    mc.comm_refusal(BACKEND)
