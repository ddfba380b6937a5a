"""The tables of tests/tangent_shapes.py on the host backend (libfemcy_cpu.so, one child process with FEMCY_BACKEND=cpu): every
row's pins and edges, the consistent tangent, the one-pass sweep and the state the option leaves behind against the same
long-double references and bounds as the device half (tests/test_gpu_tangent_shapes.py) -- and the reference's own
conditions, which need no library: the restatement the complex step differentiates is asm_shapes.reference's, the closed form
in long double agrees with the complex step, every constant of the docstring measured again, and no mutation of the closed
form hides under the bound."""
import json
import os
import subprocess
import sys

import pytest

import tangent_shapes as ts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = [t.name for t in ts.TABLE]
SWEEP = [r.name for r in ts.SWEEP]

CHILD = """
import json, sys, traceback
sys.path[:0] = [%r, %r]
import tangent_shapes as ts
out, worst, hidden = {}, {}, {}
def run(key, fn):
    try:
        got = fn()
        out[key] = "ok"
        return got
    except Exception:
        out[key] = traceback.format_exc()[-3000:]
def note(got):
    for k, v in (got or {}).items():
        worst[k] = max(worst.get(k, 0.0), v)
for t in ts.TABLE:
    run(t.name + "/edge", lambda: ts.check_edge(t.name, "cpu"))
    run(t.name + "/tangent", lambda: ts.check_tangent(t.name, "cpu"))
    run(t.name + "/restatement", lambda: ts.check_restatement(t.name))
    note(run(t.name + "/measure", lambda: ts.measure(t.name, ts.SCALES + (ts.STATE_SCALES[1:] if t.name in ts.STATE else ()))))
    for mat in ts.MATS:
        hidden[t.name + "/" + mat] = run(t.name + "/mutations/" + mat, lambda: ts.mutations(t.name, mat))
for r in ts.SWEEP:
    run(r.name + "/edge", lambda: ts.check_edge(r.name, "cpu"))
    run(r.name + "/sweep", lambda: ts.check_sweep(r.name, "cpu"))
    note(run(r.name + "/measure", lambda: ts.measure(r.name, ts.SCALES[1:])))
for name in ts.STATE:
    run(name + "/state", lambda: ts.check_state(name, "cpu"))
out["constants"], out["hidden"] = worst, hidden
json.dump(out, open(%r, "w"))
"""


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("tangent_shapes") / "host.json")
    env = dict(os.environ, FEMCY_BACKEND="cpu")
    out = subprocess.run([sys.executable, "-c", CHILD % (ROOT, os.path.join(ROOT, "tests"), path)],
                         capture_output=True, text=True, timeout=1800, cwd=ROOT, env=env)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    with open(path) as f:
        return json.load(f)


@pytest.mark.parametrize("check", ("edge", "tangent", "restatement", "measure", "mutations/stvk", "mutations/neo"))
@pytest.mark.parametrize("name", TABLE)
def test_row_on_the_host(host, name, check):
    assert host[name + "/" + check] == "ok", host[name + "/" + check]


@pytest.mark.parametrize("check", ("edge", "sweep", "measure"))
@pytest.mark.parametrize("name", SWEEP)
def test_sweep_on_the_host(host, name, check):
    assert host[name + "/" + check] == "ok", host[name + "/" + check]


@pytest.mark.parametrize("name", ts.STATE)
def test_state_on_the_host(host, name):
    assert host[name + "/state"] == "ok", host[name + "/state"]


def test_constants_are_the_measured_ones(host):
    """float64 (C_CLOSED: the long-double closed form) against the long-double complex step and restatement over both tables:
    the recorded constants bound what is measured here, and by no more than a rounding of the third digit; asm_shapes' C_ASM
    bounds the OPT_TANGENT = 0 matrix on these rows and scales as well"""
    got = host["constants"]
    assert set(got) == set(ts.C) | {"APPLY_ASM"}, sorted(got)
    for k, rec in ts.C.items():
        assert got[k] <= rec <= 1.02 * got[k], (k, got[k], rec)
    assert got["APPLY_ASM"] <= ts.ash.C_ASM, got["APPLY_ASM"]


@pytest.mark.parametrize("mat", ts.MATS)
@pytest.mark.parametrize("name", TABLE)
def test_no_mutation_hides_under_the_bound(host, name, mat):
    """a Gauss point left out (the least visible one), a contribution taken twice (the least visible one), the geometric
    term dropped, sigma or F of the other displacement, lambda' and mu' swapped, an upper block untransposed at its mirror:
    each moves a stored entry by more than 100 x the bound allowed there, at the non-zero scale"""
    got = host["hidden"][name + "/" + mat]
    assert got is not None and set(got) == set(ts.MUTATIONS), got
    for k, v in got.items():
        assert v > 100.0, (name, mat, k, v)


@pytest.mark.parametrize("name", TABLE + SWEEP)
def test_table_pins_and_edges(name):
    """the tables' own arithmetic (no library)"""
    ts.check_table(name)


def test_tables_cover_what_they_name():
    ys = {n: ts.check_table(n) for n in TABLE}
    assert {ts.stored_rows(y) % 4 for y, _ in ys.values()} == {0, 1, 2, 3}        # the last workgroup of 256 lanes
    assert any(ts._padding(y) for y, _ in ys.values())                              # tpos == -1
    assert any(ts.ash._cross(y, ts.SLICE) for y, _ in ys.values())                  # a mirrored store into another slice
    assert any(y.sigma < y.nn and ts.ash._cross(y, y.sigma) for y, _ in ys.values())      # ... into another sort window
    con = set().union(*(set(y.contributors.tolist()) for y, _ in ys.values()))
    assert {0, 1, 2} <= con and max(con) >= 16
    assert any(ts.ash._loose_slice(y) for y, _ in ys.values())                      # a slice made only of loose rows
    # every Gauss rule the element families have (CPS8 integrates with 2 x 2 points here: no family has 9)
    assert {g for _, g in ys.values()} == {1, 3, 4, 6, 8}
    fam = {ts.ROWS[n].mesh[1][0] for n in TABLE}
    assert fam == set(ts.ash.PLUGINS) == {r.mesh[1][0] for r in ts.SWEEP}
    assert {y.dm for y, _ in ys.values()} == {2, 3}
    assert {r.mesh[1][2] for r in ts.SWEEP} == set(ts.NES) and len(ts.SWEEP) == 8 * len(ts.NES)
    plug = {et: ts.ash.PLUGINS[et]().tables() for et in fam}
    # k_geom's staging: whole records of 6, 8, 12 and 16 doubles, chunks of 9, 12 and 15
    assert {et: ts.chunk(int(t["npe"]) * int(t["dm"])) for et, t in plug.items()} == {
        "CPS3": 6, "CPS4": 8, "C3D4": 12, "CPS6": 12, "CPS8": 16, "C3D6": 9, "C3D8": 12, "C3D10": 15}
    assert set(ts.STATE) <= set(TABLE)
