"""The table of tests/small_shapes.py on the host backend (libfemcy_cpu.so, one child process with FEMCY_BACKEND=cpu): the
pins, the Python restatement of pcg_small_solve's selection and of the waves' chunks, every row's own edge, the fit of the
rows (pcg_shapes.check_fit: the float64 oracle's own scatter), the sensitivity of the chunk rows to a missing block, the
stop every row must offer -- with the float64 oracle stopping where the long-double recurrence says --, and the constants,
measured again.  The host library has one PCG loop and takes FEMCY_TUNE_SMALL_REG_ROWS as a no-op, so the iterate and stop
checks run there against the same long-double references, which keeps them honest on a machine without a GPU."""
import json
import os
import subprocess
import sys

import pytest

import small_shapes as ss

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECKS = ("table", "fit", "iterates", "stop", "oracle-stop", "sensitivity")

CHILD = """
import json, sys, traceback
sys.path[:0] = [%r, %r]
import pcg_shapes as ps, small_shapes as ss
out, worst = {}, {1: 0.0, 2: 0.0, 7: 0.0}
for row in ss.ROWS:
    for name, fn in (("table", lambda n: ss.check_table(n, "cpu")), ("fit", lambda n: ps.check_fit(n, "cpu")),
                     ("iterates", lambda n: ss.check_iterates(n, "cpu")), ("stop", lambda n: ss.check_stop(n, "cpu")),
                     ("oracle-stop", lambda n: ss.stop_on_the_oracle(n, "cpu")),
                     ("sensitivity", lambda n: ss.check_sensitivity(n, "cpu") if row.group in ("chunk", "share") else None)):
        try:
            fn(row.name)
            out[row.name + "/" + name] = "ok"
        except Exception:
            out[row.name + "/" + name] = traceback.format_exc()[-3000:]
    t = ss.measure_constants("cpu", [row])
    worst = {m: max(worst[m], t[m]) for m in worst}
    T = ss.case(row.name, "cpu").T
    out[row.name + "/seen"] = [T.dm, T.K, T.RR, sorted(ss.case(row.name, "cpu").stops)]
out["constants"] = [worst[1], worst[2], worst[7]]
json.dump(out, open(%r, "w"))
"""


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("small_shapes") / "host.json")
    env = dict(os.environ, FEMCY_BACKEND="cpu")
    out = subprocess.run([sys.executable, "-c", CHILD % (ROOT, os.path.join(ROOT, "tests"), path)],
                         capture_output=True, text=True, timeout=1500, cwd=ROOT, env=env)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    with open(path) as f:
        return json.load(f)


@pytest.mark.parametrize("check", CHECKS)
@pytest.mark.parametrize("row", ss.ROWS, ids=ss.row_id)
def test_row_on_the_host(host, row, check):
    assert host[row.name + "/" + check] == "ok", host[row.name + "/" + check]


def test_constants_are_the_measured_ones(host):
    """float64 against long double over this table: the recorded figures bound what is measured here by no more than a
    rounding of the third digit, and the constants in use are pcg_shapes' where those cover the figure, else the figure"""
    import pcg_shapes as ps
    t1, t2, t7 = host["constants"]
    print("measured over the table:", t1, t2, t7)
    for got, rec, used, theirs in zip((t1, t2, t7), ss.MEASURED, (ss.T_ALPHA, ss.T_X[2], ss.T_X[7]), (ps.T_ALPHA, ps.T_X[2], ps.T_X[7])):
        assert got <= rec <= 1.02 * got, (got, rec)
        assert used == (theirs if rec <= theirs else rec), (rec, used, theirs)


def test_every_instantiation_runs_and_every_row_can_stop(host):
    """the 14 instantiations of k_pcg_small, both declined block sizes, and a stop for every row"""
    ran = {tuple(host[r.name + "/seen"][:3]) for r in ss.ROWS}
    print("instantiations the table runs:", sorted(i for i in ran if i[1] is not None))
    assert set(ss.INSTANCES) <= ran, sorted(set(ss.INSTANCES) - ran)
    assert {(2, None, None), (3, None, None)} <= ran
    assert all(host[r.name + "/seen"][3] for r in ss.ROWS)


def test_table_holds_the_edges_it_names():
    """the table's own arithmetic (no library): bucket and share boundaries from both sides, the LDS threshold, odd n in
    every bucket, and the chunk cases"""
    pins = [r.pin for r in ss.ROWS]
    ns = {(p[0], p[1]) for p in pins}
    assert {(2, 2048), (2, 2050), (2, 6144), (2, 6146), (2, 12288), (2, 12290)} <= ns
    assert {(3, 2046), (3, 2049), (3, 6144), (3, 6147), (3, 12288), (3, 12291)} <= ns
    for K in (8, 24, 48):
        assert any(p[1] % 2 == 1 for p in pins if p[4] == K), K
    for r in ss.ROWS:
        assert ss.select(r.pin[0], r.pin[1], r.pin[2], r.pin[3], r.knob) == (None if r.pin[4] is None else r.pin[4:]), r.name
    for dm in (2, 3):
        assert {p[6] for p in pins if p[0] == dm and p[4] == 24} >= {ss.ATTR_LDS, ss.ATTR_LDS + 16}
        assert {(p[3], p[5]) for r, p in zip(ss.ROWS, pins) if p[0] == dm and r.knob < 0} >= {(32, 8), (33, 16), (33, 12)}
    seen = set()
    for r in ss.ROWS:
        if r.pin[4] is not None and r.fan:
            for c in ss.chunks(r.pin[3], r.pin[5]):
                seen.add(("empty" if c.rows == 0 else "short" if c.missing else "exact" if c.streamed == 0 else
                          "odd" if c.streamed % 2 else "even", r.pin[5]))
    assert {("short", 8), ("exact", 8), ("odd", 8), ("even", 8), ("exact", 12), ("short", 12), ("exact", 16), ("odd", 16),
            ("short", 16), ("odd", 0)} <= seen, sorted(seen)
    assert ss.chunks(5, 8)[3].j0 > 5 and ss.chunks(1, 8)[2].j0 > 1 and ss.chunks(3, 8)[3].rows == 0


def test_row_names_are_free():
    """pcg_shapes.case finds a row by its name across every table built on it: no name of this table is another's"""
    import pcg_shapes as ps
    import persist_shapes as pp
    mine = {r.name for r in ss.ROWS}
    assert len(mine) == len(ss.ROWS)
    assert not mine & {r.name for r in pp.ROWS} and not mine & {r.name for r in ps.ROWS}
    assert all(ps.TABLES[r.name][0] is r for r in ss.ROWS) and all(ps.TABLES[r.name][0] is r for r in pp.ROWS)
