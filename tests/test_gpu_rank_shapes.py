"""-m gpu: the multi-rank exchange and owner-masked kernels at their edges (tests/rank_shapes.py), N contexts of one process on
one GPU through the in-process transport: interface vectors of 254 / 255 / 256 / 258 / 513 slots, local and global counts on
different sides of 256 with hole slots, nodes shared by 3, 4, 5 and 8 ranks, ranks whose every node is on the interface, a rank
that owns nothing, a rank without interface, a 1-rank communicator and odd local n; exact interface sums, products, masked
norms and maxima, both Dirichlet variants with the ownership diagonal, the three-launch PCG iterate by iterate against the
long-double restatement of the partitioned recurrence, and loads through the interface -- under both exchanges, the solves with
and without the overlapped schedule.  tests/test_rank_shapes_cpu.py checks the tables, the references and the constants."""
import pytest

import rank_shapes as rs

pytestmark = pytest.mark.gpu
BACKEND = "hip"


@pytest.mark.parametrize("name", rs.CASES)
def test_interface_sums_are_exact(name):
    rs.iface_sums(name, BACKEND)


@pytest.mark.parametrize("name", rs.CASES)
def test_product(name):
    rs.product(name, BACKEND)


@pytest.mark.parametrize("name", rs.CASES)
def test_masked_reductions(name):
    rs.reductions(name, BACKEND)


@pytest.mark.parametrize("name", rs.CASES)
def test_dirichlet(name):
    rs.dirichlet(name, BACKEND)


@pytest.mark.parametrize("name", rs.CASES)
def test_three_launch_pcg(name):
    rs.pcg(name, BACKEND)


@pytest.mark.parametrize("name", rs.LOAD_CASES)
def test_loads_through_the_interface(name):
    rs.loads(name, BACKEND)
