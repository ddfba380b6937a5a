"""-m gpu: prescribed motion and the energy balance at their list and slot edges (tests/motion_shapes.py): k_explicit_place at
255, 256, 257 and 513 entries, fixed and under the device clock; four curves of up to 16 points used out of id order; a moved
hub of 32, 33, 64 and 65 triangles and a moved rim with the balance running; the read-back of the balance at 252, 256, 260,
1024 and 1028 slots, with a wavefront of one node and three empty ones; mass scaling chained with damping, motion and the
balance.  tests/test_motion_shapes_cpu.py runs the same functions on the host backend and checks the tables and the constants."""
import pytest

import motion_shapes as ms

pytestmark = pytest.mark.gpu
BACKEND = "hip"


@pytest.mark.parametrize("name,nmoved", ms.PLACE_CASES)
def test_place(name, nmoved):
    ms.place(name, nmoved, BACKEND)


@pytest.mark.parametrize("name", list(ms.PLACE_MESHES))
def test_place_under_the_clock(name):
    ms.place_auto(name, BACKEND)


def test_four_curves_out_of_id_order():
    ms.curves(BACKEND)


@pytest.mark.parametrize("k,which", ms.HUB_CASES)
def test_moved_hub_and_rim(k, which):
    ms.hubs(k, which, BACKEND)


@pytest.mark.parametrize("nn,variant", ms.SLOT_CASES)
def test_energy_slots(nn, variant):
    ms.slots(nn, variant, BACKEND)


@pytest.mark.parametrize("nn", ms.SLOT_SPLIT)
def test_energy_slots_split_run(nn):
    ms.slots_split(nn, BACKEND)


@pytest.mark.parametrize("family,nn", ms.SCALED_MESHES)
def test_scaled_mass_fixed_run(family, nn):
    ms.scaled_fixed(family, nn, BACKEND)


@pytest.mark.parametrize("family,nn", ms.SCALED_MESHES)
def test_scaled_mass_element_by_element(family, nn):
    ms.scaled_auto(family, nn, BACKEND)
