"""-m gpu: the consistent tangent (FEMCY_OPT_TANGENT = 1) at every family, material and slice edge (tests/tangent_shapes.py):
k_assemble_gather_consistent and k_diag_from_rowsum on every element family with the Saint Venant-Kirchhoff and the
neo-Hookean branch of kblock_consistent in both dimensions -- a last workgroup of 0 .. 3 slice rows, padding and mirrored
lanes, mirrored stores across slices and sort windows, blocks of 0 .. 65 contributors, loose rows -- entry by entry
against a long-double complex-step derivative of the element force within a bound relative to what was summed into the
entry; k_geom's one-pass sweep (gradients, F, sigma and element forces through one staging area in one launch) at 1, 63 ..
257 elements of every family against the same reference and bit for bit against the lazy split; and what switching the
option leaves behind on a context with a pending force evaluation.  tests/test_tangent_shapes_cpu.py runs the same functions
on the host backend and checks the reference itself."""
import pytest

import tangent_shapes as ts

pytestmark = pytest.mark.gpu
ITEMS = ([(t.name, c) for t in ts.TABLE for c in ("edge", "tangent")] + [(r.name, "sweep") for r in ts.SWEEP]
         + [(n, "state") for n in ts.STATE])
CHECKS = {"edge": ts.check_edge, "tangent": ts.check_tangent, "sweep": ts.check_sweep, "state": ts.check_state}


@pytest.mark.parametrize("name,check", ITEMS)
def test_row(name, check):
    """row by row, so that each mesh is built once"""
    CHECKS[check](name, "hip")


def test_worst_ratios_over_all_rows():
    """(-s) the device column of the docstring's table; every constant of it has been exercised by the items above"""
    print("worst ratios on the device:", {k: float("%.4g" % v) for k, v in sorted(ts.WORST.items())})
    assert set(ts.C) - {"CLOSED"} <= set(ts.WORST), sorted(ts.WORST)
