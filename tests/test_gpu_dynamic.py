"""Implicit dynamics on the device: the scenarios of tests/dynamic_cases.py with backend "hip", and host against device."""
import numpy as np
import pytest

import dynamic_cases as dc

pytestmark = pytest.mark.gpu
BACKEND = "hip"


@pytest.mark.parametrize("etype", ["C3D4", "CPS3"])
def test_single_element_mass(etype):
    dc.single_element(etype, BACKEND)


@pytest.mark.parametrize("name", list(dc.SHAPES))
def test_mass_properties(name):
    dc.mass_properties(name, BACKEND)


@pytest.mark.parametrize("name", list(dc.SHAPES))
def test_mass_apply(name):
    dc.mass_apply(name, BACKEND)


@pytest.mark.parametrize("name", ["CPS4-65", "C3D8-64", "C3D10", "CPS4-130"])
def test_mass_add_to_K(name):
    dc.add_to_K(name, BACKEND)


@pytest.mark.parametrize("name", ["CPS4-63", "C3D8-64", "CPS4-65"])
def test_newmark_kernels(name):
    dc.newmark_kernels(name, BACKEND)


def test_refusals():
    dc.refusals(BACKEND)


def test_mass_calls_refuse_a_context_with_a_communicator():
    dc.comm_refusal(BACKEND)


@pytest.mark.parametrize("name", dc.ENERGY_SHAPES)
def test_small_strain_energy_is_the_quadratic_form(name):
    dc.small_energy(name, BACKEND)


def test_small_strain_energy_refuses_neo_hooke():
    dc.small_energy_refusal(BACKEND)


@pytest.mark.parametrize("family", dc.FAMILIES)
def test_free_flight(tmp_path, family):
    dc.free_flight(tmp_path, family, BACKEND)


def test_energy_is_conserved(tmp_path):
    dc.energy(tmp_path, BACKEND)


@pytest.mark.parametrize("case", list(dc.TRAJ))
def test_trajectory(tmp_path, case):
    dc.trajectory(tmp_path, case, BACKEND)


@pytest.mark.parametrize("case", ["cload", "damped"])
def test_trajectory_on_the_pcg_branch(tmp_path, case):
    dc.trajectory_pcg(tmp_path, case, BACKEND)


@pytest.mark.parametrize("name", ["CPS4-65", "C3D8-64", "C3D10", "C3D4-150"])
def test_host_and_device_mass_agree(name):
    """the same mesh on both backends: both are within MASS_TOL of the long-double restatement, so within twice that of
    each other"""
    nodes, el, ELE = dc.shape_mesh(name)
    out = []
    for backend in ("cpu", "hip"):
        ctx = dc.make_ctx(nodes, el, ELE, backend)
        out.append(ctx.mass_get(ctx.mass(ELE, dc.RHO)).toarray())
        ctx.close()
    assert np.abs(out[0] - out[1]).max() <= 2 * dc.MASS_TOL * np.abs(out[0]).max()


@pytest.mark.parametrize("case", list(dc.TRAJ))
def test_host_and_device_trajectories_agree(tmp_path, case):
    import os
    path = os.path.join(str(tmp_path), "%s.inp" % case)
    dc.write_traj_deck(path, case)
    U = [dc.solve_deck(path, backend)[2] for backend in ("cpu", "hip")]
    assert np.abs(U[0] - U[1]).max() <= 2 * dc.TRAJ_TOL * np.abs(U[0]).max()
