"""The table of tests/pcg_shapes.py on the host backend (libfemcy_cpu.so, one child process with FEMCY_BACKEND=cpu): the
pinned counts, the numpy restatement of the split, every row's own edge, its fitness for the checks (the float64 oracle's
own error: pcg_shapes.check_fit), and the same product / recurrence / convergence checks against the same long-double
references -- which keeps the references and the tolerances honest on a machine without a GPU.  The host library takes
the device's schedule knobs as no-ops and has one PCG loop, so each check runs once per row and the one-launch paths
(check_path) are left to tests/test_gpu_pcg_shapes.py, which runs the same functions on the device."""
import json
import os
import subprocess
import sys

import pytest

import pcg_shapes as ps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECKS = ("edge", "fit", "product", "recurrence", "convergence")

CHILD = """
import json, sys, traceback
sys.path[:0] = [%r, %r]
import pcg_shapes as ps
out, worst = {}, [0.0] * 4
for row in ps.ROWS:
    for name, fn in (("edge", ps.check_edge), ("fit", ps.check_fit), ("product", ps.check_product),
                     ("recurrence", ps.check_recurrence), ("convergence", ps.check_convergence)):
        try:
            fn(row.name, "cpu")
            out[row.name + "/" + name] = "ok"
        except Exception:
            out[row.name + "/" + name] = traceback.format_exc()[-3000:]
    c_prod, t = ps.measure_constants("cpu", [row])
    worst = [max(a, b) for a, b in zip(worst, (c_prod, t[1], t[2], t[7]))]
out["constants"] = worst
json.dump(out, open(%r, "w"))
"""


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("pcg_shapes") / "host.json")
    env = dict(os.environ, FEMCY_BACKEND="cpu")
    out = subprocess.run([sys.executable, "-c", CHILD % (ROOT, os.path.join(ROOT, "tests"), path)],
                         capture_output=True, text=True, timeout=900, cwd=ROOT, env=env)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    with open(path) as f:
        return json.load(f)


@pytest.mark.parametrize("check", CHECKS)
@pytest.mark.parametrize("row", ps.ROWS, ids=ps.row_id)
def test_row_on_the_host(host, row, check):
    assert host[row.name + "/" + check] == "ok", host[row.name + "/" + check]


def test_constants_are_the_measured_ones(host):
    """float64 against long double over the table: the recorded constants bound what is measured here, and by no more than
    a rounding of the third digit"""
    c_prod, t1, t2, t7 = host["constants"]
    for got, rec in ((c_prod, ps.C_PROD), (t1, ps.T_ALPHA), (t2, ps.T_X[2]), (t7, ps.T_X[7])):
        assert got <= rec <= 1.02 * got, (got, rec)


def test_table_covers_what_it_names():
    """the table's own arithmetic (no library): slice counts, empty ranges, tails, families"""
    import numpy as np
    import scipy.sparse as sp
    seen = {"ns": set(), "empty": set(), "dm": set(), "kind": set(), "L": set()}
    for row in ps.ROWS:
        nodes, el, ELE, mat, cons = ps.build(row)
        nn, dm = nodes.shape
        A = sp.csr_matrix((np.ones(el.size), (np.repeat(np.arange(len(el)), el.shape[1]), el.ravel())), shape=(len(el), nn))
        rowlen = np.diff((A.T @ A + sp.identity(nn)).tocsr().indptr)
        node_of, L = ps.layout(rowlen)
        S = lambda w=1, cap=0: ps.split_of(L, dm, nn, w, cap, True)
        N = ps.split_of(L, dm, nn, 1, 0, False)
        assert (nn * dm, len(L), int(L.sum()) * ps.SLICE) == (row.n, row.nslices, row.stored), row.name
        assert row.edge(S, N), (row.name, row.why)
        seen["ns"].add(len(L))
        seen["empty"] |= {k for k in range(ps.NX) if S().lens[k] == 0}
        seen["dm"].add(dm)
        seen["kind"].add(row.kind)
        seen["L"] |= set(L.tolist())
    assert {1, 2, 7, 8, 9, 17} <= seen["ns"]
    assert {0, 1, 4, 7} <= seen["empty"]                 # first, first-but-one, middle, last
    assert seen["dm"] == {2, 3} and {"C3D4", "C3D10", "C3D8", "C3D6", "CPS3", "beam", "sliver"} <= seen["kind"]
    assert {1, 3} <= seen["L"]                           # (L = 2 cannot exist: pcg_shapes.py)
    assert any(r.n % 2 == 1 for r in ps.ROWS if r.kind.startswith("C3D")) and any(r.n % 2 == 0 for r in ps.ROWS if r.kind.startswith("C3D"))
