"""What tests/rank_shapes.py needs no backend for (the host backend has no communicator, so nothing runs one here): the case
table's own claims -- interface sizes on their side of 256 and 512, sharing multiplicities, hole slots, a rank without
interface, a rank that owns nothing, an odd local n -- with the partition invariants of tests/test_distributed_cpu.py; the
conditions placed on the references (the partitioned restatements agree with the oracle's global matrix, every shared DOF
counts once, replicas are equal); and the float64 constants measured again.  tests/test_gpu_rank_shapes.py runs the checks."""
import numpy as np
import pytest

import rank_shapes as rs


def test_tables_cover_what_they_name():
    assert {c[3]["glob"] for n, c in rs.CASES.items() if n.startswith("edge2d")} == {rs.BS - 2, rs.BS, rs.BS + 2}
    assert {c[3]["glob"] for n, c in rs.CASES.items() if n.startswith("edge3d")} == {rs.BS - 1, rs.BS + 2, 2 * rs.BS + 1}
    assert [rs.CASES[n][2] for n in rs.FANS] == [3, 5, 8] and max(c[2] for c in rs.CASES.values()) == rs.MAX_RANKS
    assert {rs.CASES[n][3]["mult"] for n in rs.MULTIPLICITY_CASES} == {3, 4, 5, 8}
    assert any(c[3].get("empty") and c[2] > 1 for c in rs.CASES.values()) and rs.CASES["single"][2] == 1
    assert any(c[3].get("odd") for c in rs.CASES.values()) and set(rs.LOAD_CASES) <= set(rs.CASES)
    assert rs.MODES == ((0, 0), (0, 1), (1, 0), (1, 1)) and rs.PCG_ITERS == (1, 3, 9)
    assert rs.SOLVE_BOUND == 10 * rs.SOLVE_EPS


@pytest.mark.parametrize("name", rs.CASES)
def test_case_table(name):
    rs.case_table(name)


@pytest.mark.parametrize("name", rs.CASES)
def test_reference_conditions(name):
    """the float64 restatement stays within every constant on every case"""
    fig = rs.reference_conditions(name)
    for key, v in fig.items():
        assert v <= rs.worst_of(key, rs.case(name).family), (name, key, v)


def test_the_bounds_are_the_measured_float64_errors():
    """4 x the worst error of the float64 restatement against the long-double one on these very cases: every constant is at
    least what is measured now and at most 1.5 x it"""
    worst = rs.measure_f64_worst()
    print(worst)
    want = {(k, f) for k, v in rs.F64_WORST.items() for f in (rs.FAMILIES if isinstance(v, dict) else (None,))}
    assert set(worst) == want and {rs.case(n).family for n in rs.CASES} == set(rs.FAMILIES)
    for (key, family), measured in worst.items():
        const = rs.worst_of(key, family)
        assert measured <= const <= 1.5 * measured, (key, family, measured, const)


def test_restatement_of_the_rank_ordered_sum():
    """s = 0.0; for r in sorted(sharing ranks): s += v_r -- adding the zeros of the absent ranks changes no bits"""
    c = rs.case("octants")
    rnds = [rs.local_vectors(c, r)[1] for r in range(c.nranks)]
    got = rs.rr.iface_sum(c.parts, rnds, np.float64)
    for p, gd, w in zip(c.parts, c.gd, got):
        for ld in p.iface_local_dofs[::7]:
            s = 0.0
            for q in range(c.nranks):
                hit = np.nonzero(c.gd[q] == gd[ld])[0]
                s += rnds[q][hit[0]] if hit.size else 0.0
            assert s == w[ld]
