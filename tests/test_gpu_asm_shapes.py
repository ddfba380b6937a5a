"""-m gpu: every assembly kernel at its slice, step and batch edges (tests/asm_shapes.py): nn = 0, 1, 2, 3, 63 mod 64, a last
slice of one row, waves with an odd row count, loose rows inside and next to coupled ones, sort-window boundaries inside
the mesh, ROWS4 steps and write-out trips, ROWS2 passes of E - 1 .. 2 E + 1 elements, ROWS lanes below / at / above 64 and the
capped grid, PAIRS chunks of 64 and 65 pairs and of loose rows only under every knob, dynamic LDS just under and over 48 KiB,
refusals beyond what a workgroup may allocate, k_geom's last workgroup and the node sums of 0 .. 65 rows -- each entry
against a long-double reference within a bound relative to what was summed into it, then one product and a second,
bit-equal assembly.  tests/test_asm_shapes_cpu.py runs the same functions on the host backend."""
import pytest

import asm_shapes as ash

pytestmark = pytest.mark.gpu
CHECKS = {"edge": ash.check_edge, "assembly": ash.check_assembly, "force": ash.check_force}


@pytest.mark.parametrize("row,check", [(r, c) for r in ash.ROWS for c in CHECKS], ids=lambda v: getattr(v, "name", v))
def test_row(row, check):
    """row by row, so that each mesh is built once"""
    CHECKS[check](row.name, "hip")
