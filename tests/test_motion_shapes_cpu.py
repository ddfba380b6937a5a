"""The list and slot edges of prescribed motion and the energy balance, and mass scaling chained with damping, motion and the
balance, on the host backend (tests/motion_shapes.py); the tables' own arithmetic and the measured float64 constants the
bounds of both backends rest on."""
import numpy as np
import pytest

import motion_shapes as ms

BACKEND = "cpu"


def test_f64_constants_are_the_measured_ones():
    worst = ms.measure_f64_worst()
    print(worst)
    assert set(worst) == set(ms.USES)
    for group, w in worst.items():
        c = ms.bound_of(group)
        if ms.USES[group] == "own":                                    # the measured figure, which energy_cases' does not hold
            assert w <= c <= 1.1 * w + 1e-17 and w > ms.enc.F64_WORST, (group, w)
        elif ms.USES[group] == "energy":
            assert w <= c, (group, w)
        else:                                                          # the tightest of the constants that exist
            assert w <= c and not any(w <= other < c for other in ms.STATE_CONSTANTS.values()), (group, w)


def test_tables():
    for nn, (cells, keep, slots) in ms.SLOT_MESHES.items():
        nodes, el, _ = ms.slot_mesh(nn)
        assert len(el) == keep < 2 * cells[0] * cells[1] and slots == 4 * -(-nn // 8)
    assert sorted(s for _, _, s in ms.SLOT_MESHES.values()) == [252, 256, 256, 260, 1024, 1028]
    for name, nm in ms.PLACE_CASES:
        case, order, again, rest, T = ms.place_case(name, nm)
        assert len(order) == nm
        assert [len(t) for _, t, _ in case.curves] == [2, 6, 16, 16]
        assert case.curves[0][1][0] == 0.0 and case.curves[0][1][-1] < T and all(c[1][0] > 0 and c[2][0] != 0 for c in case.curves[1:])
    lengths = np.diff(ms.CURVE_TABLES[0][1])
    assert lengths.max() / lengths.min() > 2 ** 8 and [len(t) for _, t, _ in ms.CURVE_TABLES] == [16, 16, 2, 2]


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
