"""The table of tests/persist_shapes.py on the host backend (libfemcy_cpu.so, one child process with FEMCY_BACKEND=cpu): the
pinned counts, the numpy restatement of the launch shape, the hand-out and the residency, every row's own edge, the fit of
the rows for the stopping check (pcg_shapes.check_fit: the float64 oracle's own scatter) and the constants, measured again.
The host library has one PCG loop and takes the launch knobs as no-ops, so the once-per-shape checks run there against the
same long-double references, which keeps the references honest on a machine without a GPU; the configurations are left to
tests/test_gpu_persist_shapes.py."""
import json
import os
import subprocess
import sys

import pytest

import persist_shapes as pp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECKS = ("table", "fit", "once")

CHILD = """
import json, sys, traceback
sys.path[:0] = [%r, %r]
import numpy as np
import pcg_shapes as ps, persist_shapes as pp
out, worst, seen = {}, {1: 0.0, 2: 0.0, 7: 0.0}, {}
for row in pp.ROWS:
    for name, fn in (("table", lambda n: pp.check_table(n, "cpu")), ("fit", lambda n: ps.check_fit(n, "cpu")),
                     ("once", lambda n: pp.check_once(n, "cpu", fit=n not in pp.UNFIT))):
        try:
            fn(row.name)
            out[row.name + "/" + name] = "ok"
        except Exception:
            out[row.name + "/" + name] = traceback.format_exc()[-3000:]
    t = pp.measure_constants("cpu", [row])
    worst = {m: max(worst[m], t[m]) for m in worst}
    out[row.name + "/seen"] = pp.seen(pp.case(row.name, "cpu").T)
out["constants"] = [worst[1], worst[2], worst[7]]
json.dump(out, open(%r, "w"))
"""


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("persist_shapes") / "host.json")
    env = dict(os.environ, FEMCY_BACKEND="cpu")
    out = subprocess.run([sys.executable, "-c", CHILD % (ROOT, os.path.join(ROOT, "tests"), path)],
                         capture_output=True, text=True, timeout=1500, cwd=ROOT, env=env)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    with open(path) as f:
        return json.load(f)


@pytest.mark.parametrize("check", CHECKS)
@pytest.mark.parametrize("row", pp.ROWS, ids=pp.row_id)
def test_row_on_the_host(host, row, check):
    got = host[row.name + "/" + check]
    if check == "fit" and row.name in pp.UNFIT:
        assert got != "ok", "the row fits the stopping check: take it out of UNFIT"
        last = got.strip().splitlines()[-1]                       # check_fit's own verdict, not some other exception
        assert last.startswith("AssertionError: ('%s'" % row.name), got
    else:
        assert got == "ok", got


def test_at_most_a_quarter_of_the_rows_is_left_out_of_the_stopping_check():
    assert set(pp.UNFIT) <= set(pp.BY_NAME) and 4 * len(pp.UNFIT) <= len(pp.ROWS), pp.UNFIT


def test_constants_are_the_measured_ones(host):
    """float64 against long double over the table: the recorded constants bound what is measured here, and by no more than
    a rounding of the third digit"""
    t1, t2, t7 = host["constants"]
    for got, rec in ((t1, pp.T_ALPHA), (t2, pp.T_X[2]), (t7, pp.T_X[7])):
        assert got <= rec <= 1.02 * got, (got, rec)


def test_table_covers_the_ladder_and_the_edges(host):
    """every instantiation of the launch ladder is named by a (row, configuration), and the union of the residencies holds
    every edge the table exists for"""
    shapes, u = set(), {}
    for row in pp.ROWS:
        for k, v in host[row.name + "/seen"].items():
            if k == "shapes":
                shapes |= {tuple(s) for s in v}
            else:
                u.setdefault(k, set()).update(v)
    want = {(3, 3, 0, v) for v in (6, 14, 0)} | {(3, 3, 4, v) for v in (6, 14, 0)} | {(3, 3, 5, v) for v in (6, 14, 0)}
    want |= {(3, 4, r, v) for r in (0, 3) for v in (6, 14, 0)} | {(3, 5, 0, 6), (3, 5, 1, 6), (3, 6, 0, 6), (3, 6, 1, 6), (3, 7, 0, 6)}
    want |= {(2, s, r, v) for s, rj in ((3, 5), (4, 5), (6, 3), (8, 2)) for r in (0, rj) for v in (6, 14, 0)}
    assert want <= shapes, sorted(want - shapes)
    assert u["G"] == {8, 16, 24} and u["declined"] == {2, 3}                          # block sizes of the declined rows
    assert {3, 4, 5, 6, 7} <= u["per_wave3"] and {3, 4, 5, 6, 7, 8} <= u["per_wave2"]
    assert {0, 1, 2, 3, 4} <= u["npf"]
    assert {1, 4, 5} <= u["lds_batch"]                                                 # LDS rows of a slice: je - jl
    assert {0, 1, 4} <= u["streamed"] and any(v >= 5 for v in u["streamed"]) and any(v >= 13 for v in u["streamed"])
    assert {3, 4, 5} <= u["rj_above_L"]                                                # RJ of a slice with L < RJ
    assert {3, 5} <= u["rj_equals_L"]
    assert {"inside", "boundary", "before-slot-0", "nothing-streamed", "none"} <= u["budget"]
    assert u["free_slots"] and u["empty_wave"] and u["empty_workgroup"] and u["empty_range"]
    assert u["odd_n"] and u["padding_last"]
