"""The scenarios of tests/dyn_shapes.py on the host backend (libfemcy_cpu.so), which shares the element, node-pass and clock
arithmetic and restates the device's reduction orders: the same functions, references and bounds as
tests/test_gpu_dyn_shapes.py.  Also what needs no backend: the margins of the planted maxima on the reference alone, the
tables' own arithmetic, and the float64 constants measured again."""
import os

import numpy as np
import pytest

from femcy_amd import backend as be

import dyn_shapes as ds

BACKEND = "cpu"
pytestmark = pytest.mark.skipif(not os.path.exists(be.CPU_LIB_PATH), reason="libfemcy_cpu.so has not been built")


def test_the_bounds_are_the_measured_float64_errors():
    """4 x the worst error of the float64 restatement against the long-double one on the gather cases: the constants are at
    least what is measured now and at most 1.5 x it"""
    worst = ds.measure_f64_worst()
    print(worst)
    for measured, constant in ((worst["lumped"], ds.F64_WORST_GATHER_LUMPED), (worst["step"], ds.F64_WORST_GATHER_STEP),
                               (worst["force"], ds.F64_WORST_GATHER_FORCE)):
        assert measured <= constant <= 1.5 * measured, (measured, constant)


@pytest.mark.parametrize("family", ds.PLANT_MESHES)
def test_the_planted_element_exceeds_the_rest(family):
    ds.planted_margin(family)


@pytest.mark.parametrize("at", ds.ROWABS_AT)
def test_the_planted_row_exceeds_the_rest(at):
    ds.rowabs_margin(at)


@pytest.mark.parametrize("name", ds.GATHER_CASES)
def test_gather_tables(name):
    ds.gather_edge(name)


def test_tables_cover_what_they_name():
    assert {m.family for n, m in ds.MESHES.items() if n in ds.BLOCK_CASES} == {"CPS3", "CPS4", "CPS8", "C3D4", "C3D8", "C3D6", "C3D10"}
    assert sorted(set(ds.ADD_TO_K_CASES.values())) == [256 - 64, 256, 256 + 64]
    assert {nn for _, _, _, nn in ds.ENERGY_MESHES.values()} == {255, 256, 257, 8 * 256 + 1} and ds.ENERGY_BIG[3] == 1024 * 256 + 1
    for name in ds.ENERGY_MESHES:
        ds.energy_mesh(name)
    assert {(n + 1) // 2 for n in ds.VECTOR_N} >= {255, 256, 257, 512, 513} and sum(n % 2 for n in ds.VECTOR_N) == 2
    assert all(n == nn * (2 if fam == "CPS3" else 3) for n, (fam, nn) in ds.VECTOR_N.items())
    saved = ds.dc.SHAPES, ds.dc.shape_mesh, ds.ec.shape_mesh
    with ds.registered():
        assert ds.dc.shape_mesh("CPS3")[0].shape == saved[1]("CPS3")[0].shape      # the neighbours' own names still resolve
    assert (ds.dc.SHAPES, ds.dc.shape_mesh, ds.ec.shape_mesh) == saved and not set(ds.MESHES) & set(saved[0])


@pytest.mark.parametrize("family, at", ds.PLANT_CASES)
def test_planted_element_bound(family, at):
    ds.planted(family, at, BACKEND)


@pytest.mark.parametrize("at", ds.ROWABS_AT)
def test_planted_gershgorin_row(at):
    ds.rowabs(at, BACKEND)


@pytest.mark.parametrize("variant", ds.ENERGY_VARIANTS)
@pytest.mark.parametrize("name", list(ds.ENERGY_MESHES) + ["big"])
def test_kinetic_energy(name, variant):
    ds.energy(name, variant, BACKEND)


@pytest.mark.parametrize("check", ds.BLOCK_CHECKS)
@pytest.mark.parametrize("name", ds.BLOCK_CASES)
def test_block_edge(name, check):
    ds.block_edge(check, name, BACKEND)


@pytest.mark.parametrize("name", ds.GATHER_CASES)
def test_gather_step(name):
    ds.gather_step(name, BACKEND)


@pytest.mark.parametrize("name", ds.GATHER_CASES)
def test_gather_lumped(name):
    ds.gather_lumped(name, BACKEND)


@pytest.mark.parametrize("name", ds.GATHER_CASES)
def test_gather_force(name):
    ds.gather_force(name, BACKEND)


@pytest.mark.parametrize("n", ds.VECTOR_N)
def test_vectors_under_a_small_grid_cap(n):
    ds.vectors(n, BACKEND)


@pytest.mark.parametrize("name", ds.ADD_TO_K_CASES)
def test_mass_add_to_K(name):
    ds.add_to_K(name, BACKEND)
