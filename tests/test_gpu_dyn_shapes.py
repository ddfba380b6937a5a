"""-m gpu: the dynamics kernels at their block, partial and gather edges (tests/dyn_shapes.py): a maximum planted in partial 0,
63, 64, 255, 256 and the last of more than 256 partials of the element bound, plain, damped and through the device clock; the
largest Gershgorin row in the first and last lane of either workgroup; kinetic-energy sums at 255, 256, 257, 2049 and
1024 x 256 + 1 nodes; every one-thread-per-element kernel at 255, 256 and 257 elements of seven families; node gathers of 32,
33, 64 and 65 rows by a hub that is alone in the last workgroup; the element-wise kernels and the reductions under a grid cap
of 1 and 2; mass_add_to_K on either side of 256 stored blocks.  tests/test_dyn_shapes_cpu.py runs the same functions on the
host backend and checks the tables, the margins and the constants."""
import pytest

import dyn_shapes as ds

pytestmark = pytest.mark.gpu
BACKEND = "hip"


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
