"""-m gpu: the load, boundary and post-processing kernels at their edges (tests/post_shapes.py): surface loads of 126, 127,
128, 129 and 257 facets of two, three, four and six nodes and a hub of 128 contribution slots as the last loaded node; the
Dirichlet 0 / 1 kernel at 248, 256, 264, 504 and 516 threads with the last one in a longest row; scatters of 255, 256 and 257
entries; the Gauss-point and extrapolation kernels on either side of 256 threads for eight families, small and large, with
the energy totals up to 1024 x 256 + 1 Gauss points; the element passes of the body and thermal loads at 255, 256 and 257
elements with the signal in the last element alone.  tests/test_post_shapes_cpu.py runs the same functions on the host
backend and checks the tables, the reference conditions and the constants."""
import pytest

import post_shapes as ps

pytestmark = pytest.mark.gpu
BACKEND = "hip"


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
