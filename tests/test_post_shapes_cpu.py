"""The scenarios of tests/post_shapes.py on the host backend (libfemcy_cpu.so), which shares the element arithmetic
(csrc/element_math.hpp) and restates the device's gathers and sums: the same functions, references and bounds as
tests/test_gpu_post_shapes.py.  Also what needs no backend: the tables' own arithmetic, the conditions placed on the
references (the last facet, node, DOF, element and Gauss point carry a signal; the oracle agrees with the long-double
restatements), and the float64 constants measured again."""
import os

import numpy as np
import pytest

from femcy_amd import backend as be

import post_shapes as ps

BACKEND = "cpu"
pytestmark = pytest.mark.skipif(not os.path.exists(be.CPU_LIB_PATH), reason="libfemcy_cpu.so has not been built")


def test_the_bounds_are_the_measured_float64_errors():
    """4 x the worst error of the float64 restatement against the long-double one on these very cases: every constant is at
    least what is measured now and at most 1.5 x it"""
    worst = ps.measure_f64_worst()
    print(worst)
    assert set(worst) == set(ps.F64_WORST)
    for key, measured in worst.items():
        assert measured <= ps.F64_WORST[key] <= 1.5 * measured, (key, measured, ps.F64_WORST[key])


def test_tables_cover_what_they_name():
    assert ps.SURFACE_NLOAD == (ps.SURFACE_WG - 2, ps.SURFACE_WG - 1, ps.SURFACE_WG, ps.SURFACE_WG + 1, 2 * ps.SURFACE_WG + 1)
    assert sorted(nfn for _, nfn in ps.SURFACE_PLATES.values()) == [2, 3, 4, 6]
    assert [T for _, _, T in ps.DIRICHLET_CASES.values()] == [256 - 8, 256, 256 + 8, 512 - 8, 512 + 4]
    assert ps.SCATTER_K == (255, 256, 257) == ps.BLOCK_NE and ps.SCATTER_N > max(ps.SCATTER_K)
    assert set(ps.POST_SHAPE) == set(ps.ds.BLOCK_PLATES) | {"CPS6"} == set(ps.BLOCK_FAMILIES)
    assert {f for f, _, _ in ps.POST_CASES} == set(ps.POST_SHAPE)
    assert {k for _, _, k in ps.POST_CASES} == {ps.pr.LIN3D, ps.pr.PSTRAIN, ps.pr.PSTRESS, ps.pr.NEOHOOKE}
    for family in ps.POST_GEOM_EDGE:
        assert {255, 256, 257} <= set(ps.POST_NE[family])
    assert {f[:3] for f in ps.POST_GEOM_EDGE} == {"CPS", "C3D"}
    assert ps.ENERGY_BIG[2] == 1024 * 256 + 1 and 2 * ps.ENERGY_BIG[1][0] * ps.ENERGY_BIG[1][1] >= ps.ENERGY_BIG[2]


@pytest.mark.parametrize("family", ps.POST_SHAPE)
def test_post_thread_counts(family):
    ps.post_table(family)


@pytest.mark.parametrize("family, nload", ps.SURFACE_CASES)
def test_surface_reference(family, nload):
    ps.surface_reference_conditions(family, nload)


@pytest.mark.parametrize("name", ps.DIRICHLET_CASES)
def test_dirichlet_tables(name):
    ps.dirichlet_dofs(name)


@pytest.mark.parametrize("family, ne, kind", ps.POST_CASES)
def test_post_reference(family, ne, kind):
    ps.post_reference_conditions(family, ne, kind)


@pytest.mark.parametrize("variant", ps.DT_VARIANTS)
@pytest.mark.parametrize("family, ne", ps.BLOCK_CASES)
def test_thermal_reference_stays_within_its_constant(family, ne, variant):
    """thermal_cases' own bound is 4 x its measured float64 error: the float64 restatement stays within that on these meshes"""
    ref, err = ps.reference_thermal(family, ne, variant)
    assert np.abs(ref.reshape(-1, 2 if family.startswith("CP") else 3)[ps.post_mesh(family, ne)[1][-1]]).max() > 0
    assert err <= ps.tc.FORCE_TOL, err


@pytest.mark.parametrize("variant", ps.ENERGY_VARIANTS)
def test_the_float64_restatement_of_the_large_case_is_within_its_bounds(variant):
    """the bounds of the 262 145 triangles come from reasoning; the float64 restatement must sit well inside them"""
    ref, bounds = ps.big_case(variant)[4:]
    assert ps._rel(ref[np.float64][0], ref[ps.LD][0]) <= 0.25 * bounds["density"]
    assert ps._rel(ref[np.float64][1], ref[ps.LD][1]) <= 0.25 * bounds["vol"]
    assert bounds["density"] <= 1e-8 and bounds["vol"] <= 1e-12     # far below what a stale tail (x 0.16) would show


@pytest.mark.parametrize("family, nload", ps.SURFACE_CASES)
def test_surface_loads(family, nload):
    ps.surface(family, nload, BACKEND)


@pytest.mark.parametrize("name", ps.DIRICHLET_CASES)
def test_dirichlet(name):
    ps.dirichlet(name, BACKEND)


@pytest.mark.parametrize("k", ps.SCATTER_K)
def test_scatters(k):
    ps.scatters(k, BACKEND)


@pytest.mark.parametrize("family, ne, kind", ps.POST_CASES)
def test_post(family, ne, kind):
    ps.post(family, ne, kind, BACKEND)


@pytest.mark.parametrize("variant", ps.ENERGY_VARIANTS)
def test_energy_of_262145_triangles(variant):
    ps.energy_big(variant, BACKEND)


@pytest.mark.parametrize("family, ne", ps.BLOCK_CASES)
def test_bodyload_at_block_edges(family, ne):
    ps.bodyload(family, ne, BACKEND)


@pytest.mark.parametrize("variant", ps.DT_VARIANTS)
@pytest.mark.parametrize("family, ne", ps.BLOCK_CASES)
def test_thermal_at_block_edges(family, ne, variant):
    ps.thermal(family, ne, variant, BACKEND)
