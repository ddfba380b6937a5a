"""-m gpu: femcy_direct_solve at every tile and panel edge of its band storage (tests/direct_shapes.py): one panel, pad
rows or none, bw = 32 / 33, T > P - 1 (every panel clipped), T odd and even (the tile pairing of the sweeps), Tp = 1, 2, 3
under every update kernel, and T = 7 / 8 / 9 around the switch to the matrix cores -- on manufactured systems that a
correct factor solves WITHOUT refinement, and on indefinite ones whose inertia the pivots must reproduce exactly.
The yardsticks are scipy's sparse LU and dense eigenvalues on the matrix exported from the device, and the host backend
(libfemcy_cpu.so, one child process); tests/test_direct_shapes_cpu.py runs the same scenarios on the host."""
import os
import subprocess
import sys

import numpy as np
import pytest

import direct_shapes as ds

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

HOST_CODE = """
import sys
sys.path[:0] = [%r, %r]
import direct_shapes as ds
ds.host_figures(%r)
"""


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    """the host backend's errors and residuals on the same meshes, from one child process (FEMCY_BACKEND=cpu)"""
    path = str(tmp_path_factory.mktemp("host") / "host.npz")
    env = dict(os.environ, FEMCY_BACKEND="cpu")
    out = subprocess.run([sys.executable, "-c", HOST_CODE % (ROOT, os.path.join(ROOT, "tests"), path)],
                         capture_output=True, text=True, timeout=600, cwd=ROOT, env=env)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    return np.load(path)


@pytest.mark.parametrize("row", ds.ROWS, ids=ds.row_id)
def test_manufactured_solution_needs_no_refinement(host, row):
    """b = K x_true, update variants -1, 0, 1, 2, 3: refinements == 0, residual within x 100 of the sparse LU's, error
    within x 10 of the LU's and the host backend's, variant 3 = variant 1 and (T < 8) auto = VALU bit for bit"""
    ds.manufactured(row, "hip", host_err=float(host["row/" + ds.row_id(row)]))


@pytest.mark.parametrize("mesh,k", ds.inertia_ids())
def test_negative_pivots_equal_negative_eigenvalues(host, mesh, k):
    """Sylvester's law on a configuration with inverted elements, for every update variant"""
    res, err = host["inertia/%s/%d" % (mesh, k)]
    ds.inertia(mesh, k, "hip", host=(float(res), float(err)))
