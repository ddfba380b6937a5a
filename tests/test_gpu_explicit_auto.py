"""The element-by-element increment of explicit dynamics on the device: the scenarios of tests/explicit_auto_cases.py on
backend "hip" (tests/test_explicit_auto_cpu.py runs them on the host backend), the host against the device, and the refusal
on a context with a communicator."""
import os

import pytest

from femcy_amd import backend as be

import explicit_auto_cases as ac
import explicit_cases as ec

BACKEND = "hip"
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    """the reference decks and their long-double runs are made once per module (the reference_* functions cache by this path)"""
    return str(tmp_path_factory.mktemp("explicit_auto_reference"))


@pytest.mark.parametrize("name, mat, state, which", ac.BOUND_CASES)
def test_element_bound(name, mat, state, which):
    ac.bound(name, mat, state, which, BACKEND)


@pytest.mark.parametrize("name", ec.SHAPES)
def test_the_bound_is_a_bound_at_rest(name):
    ac.proof(name, BACKEND)


@pytest.mark.parametrize("name", ["CPS4-63", "CPS8", "C3D4", "C3D10", "C3D8-64"])
def test_scaling(name):
    ac.scaling(name, BACKEND)


@pytest.mark.parametrize("key", ac.TRAJ_CASES)
def test_trajectory(tmp_path, key, workdir):
    ac.trajectory(tmp_path, key, BACKEND, workdir)


@pytest.mark.skipif(not os.path.exists(be.CPU_LIB_PATH), reason="libfemcy_cpu.so has not been built")
@pytest.mark.parametrize("key", ["bar-STEP", "block-RAMP"])
def test_host_against_device(tmp_path, key, workdir):
    ac.host_against_device(tmp_path, key, workdir)


@pytest.mark.parametrize("key", ["bar-STEP", "block-RAMP"])
def test_a_split_run_gives_the_same_bits(tmp_path, key):
    ac.split(key, BACKEND, tmp_path)


def test_a_crushed_bar_needs_the_element_by_element_increment(tmp_path, workdir):
    ac.crush(tmp_path, BACKEND, workdir)


def test_refusals():
    ac.refusals(BACKEND)


def test_calls_are_refused_on_a_context_with_a_communicator():
    ac.comm_refusal(BACKEND)
