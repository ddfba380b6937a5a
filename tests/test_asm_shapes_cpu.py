"""The table of tests/asm_shapes.py on the host backend (libfemcy_cpu.so, one child process with FEMCY_BACKEND=cpu): the pinned
counts, the numpy restatement of the layout, every row's own edge, the host library's one assembly, its geometry and its
nodal force against the same long-double reference and bounds as the device half (tests/test_gpu_asm_shapes.py), the float64
constants measured again, and every row's fitness: the float64 restatement alone keeps every bound with half the margin."""
import json
import os
import subprocess
import sys

import pytest

import asm_shapes as ash

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECKS = ("edge", "fit", "assembly", "force")

CHILD = """
import json, sys, traceback
sys.path[:0] = [%r, %r]
import asm_shapes as ash
out, worst = {}, [0.0] * 7
for row in ash.ROWS:
    for name, fn in (("edge", lambda: ash.check_edge(row.name, "cpu")), ("fit", lambda: ash.check_fit(row)),
                     ("assembly", lambda: ash.check_assembly(row.name, "cpu")), ("force", lambda: ash.check_force(row.name, "cpu"))):
        try:
            got = fn()
            out[row.name + "/" + name] = "ok"
            if name == "fit":
                worst = [max(a, b) for a, b in zip(worst, got)]
        except Exception:
            out[row.name + "/" + name] = traceback.format_exc()[-3000:]
out["constants"] = worst
json.dump(out, open(%r, "w"))
"""


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("asm_shapes") / "host.json")
    env = dict(os.environ, FEMCY_BACKEND="cpu")
    out = subprocess.run([sys.executable, "-c", CHILD % (ROOT, os.path.join(ROOT, "tests"), path)],
                         capture_output=True, text=True, timeout=900, cwd=ROOT, env=env)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    with open(path) as f:
        return json.load(f)


@pytest.mark.parametrize("check", CHECKS)
@pytest.mark.parametrize("row", ash.ROWS, ids=ash.row_id)
def test_row_on_the_host(host, row, check):
    assert host[row.name + "/" + check] == "ok", host[row.name + "/" + check]


def test_constants_are_the_measured_ones(host):
    """float64 against long double over the table: the recorded constants bound what is measured here, and by no more than
    a rounding of the third digit"""
    for got, rec in zip(host["constants"], ash.CONSTANTS()):
        assert got <= rec <= 1.02 * got, (got, rec)


@pytest.mark.parametrize("row", ash.ROWS, ids=ash.row_id)
def test_table_pins_and_edges(row):
    """the table's own arithmetic (no library): the pinned counts and the predicate of every row"""
    ash.check_table(row)


def test_table_covers_what_it_names():
    fam = {r.mesh[1][0] for r in ash.ROWS}
    assert fam == set(ash.PLUGINS)
    ys = {r.name: ash.check_table(r) for r in ash.ROWS if not r.name.startswith("geom-")}
    assert {y.nn % 64 for y in ys.values()} >= {0, 1, 2, 3, 63}
    for mode in (ash.G, ash.A, ash.R, ash.S, ash.SR, ash.R2, ash.R4, ash.P):
        assert any(mode in r.modes for r in ash.ROWS), ash.NAMES[mode]
    pairs = {r.mesh[1][0] for r in ash.ROWS if ash.P in r.modes}
    assert pairs == {"CPS3", "CPS4", "CPS6", "CPS8", "C3D8", "C3D6"}            # every instantiated family
    knobs = {k for r in ash.ROWS for k in r.knobs}
    assert {k[0] for k in knobs} == {16, 8} and {k[1] for k in knobs} == {2, 3, 4} and {k[2] for k in knobs} == {False, True}
    assert {1, 2, 16} <= {k[3] for k in knobs}
    assert {ne for r in ash.ROWS if r.mesh[0] == "first" for ne in [r.mesh[1][2]]} == {1, 63, 64, 65, 255, 256, 257}
    node_of, L = ash.sell_layout(ys["c3d4-fans"].rowlen, 4096)
    assert (node_of == ash.ps.layout(ys["c3d4-fans"].rowlen)[0]).all()
