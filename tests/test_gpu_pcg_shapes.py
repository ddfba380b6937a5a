"""-m gpu: the SpMV split and the three-launch PCG at every range edge (tests/pcg_shapes.py): empty first, first-but-one,
middle and last ranges, 1 .. 17 slices, range lengths 0 and 1 mod the slices per task for 1 / 2 / 4 waves per slice, slices
of length 1 / 3 / 5 (waves with an empty chunk), rounds that differ from range to range with a partial last one, rotated and
balanced task lists, odd n, clamped element ranges in node order, and the second and third batch of the vector kernels
under FEMCY_OPT_EW_GRID = 8 / 16 -- each against a long-double reference of the same operation, row by row for the product.
Then the same iterates through k_pcg_small and the persistent kernel.  tests/test_pcg_shapes_cpu.py runs the same
functions on the host backend."""
import functools

import pytest

import pcg_shapes as ps

pytestmark = pytest.mark.gpu
CHECKS = {"edge": ps.check_edge, "product": ps.check_product, "iterates": ps.check_recurrence,
          "convergence": ps.check_convergence, "small": lambda name, backend: _path(name, "small"),
          "persist": lambda name, backend: _path(name, "persist")}


@functools.lru_cache(maxsize=None)
def _path(name, path):
    """-> whether the path took the mesh (check_path asserts the iterates either way); kept, so that the count below costs
    nothing behind the rows and still carries its own evidence when it runs alone"""
    return ps.check_path(name, "hip", path)[0]


@pytest.mark.parametrize("row,check", [(r, c) for r in ps.ROWS for c in CHECKS], ids=lambda v: getattr(v, "name", v))
def test_row(row, check):
    """row by row, so that each mesh is assembled once"""
    CHECKS[check](row.name, "hip")


def test_at_most_a_quarter_of_the_rows_is_declined():
    for path in ("small", "persist"):
        declined = [r.name for r in ps.ROWS if not _path(r.name, path)]
        print(f"path {path} declined {declined}")
        assert 4 * len(declined) <= len(ps.ROWS), (path, declined)
