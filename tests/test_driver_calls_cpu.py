"""The driver's call traces on the host backend against tests/golden/driver_calls.json (tests/driver_calls_cases.py)."""
import pytest

import driver_calls_cases as dcc

BACKEND = "cpu"


def test_the_golden_file_holds_every_case_and_stays_small():
    import os
    assert list(dcc.golden()) == dcc.CASES
    assert os.path.getsize(dcc.GOLDEN) < 100 * 1024
    assert set(dcc.DEVICE_CASES) <= set(dcc.CASES)


@pytest.mark.parametrize("name", dcc.CASES)
def test_driver_calls(tmp_path, name):
    dcc.check(name, tmp_path, BACKEND)


def test_a_run_without_any_load_does_not_refresh_rhs(tmp_path):
    """the static driver leaves rhs to impose_boundary_condition, which zeroes it only ahead of an added load: a deck with no
    load at all never fills it (the reference does not either), while the two dynamic drivers do"""
    trace = dcc.record("static-no-load", tmp_path, BACKEND)[0]
    assert len([c for c in trace if c[0] == "femcy_assemble_K"]) == 2
    assert not [c for c in trace if c[0] == "femcy_vec_fill"]
    trace = dcc.record("dynamic-energy", tmp_path, BACKEND)[0]
    assert [c for c in trace if c[0] == "femcy_vec_fill" and c[1] == dcc.be.VEC_RHS]
