"""The band shapes of tests/direct_shapes.py on the host backend (libfemcy_cpu.so): the table's (n, bandwidth) pins, the
manufactured systems and the inertia of the displaced configurations -- band_order.hpp (the order both libraries share,
the host's factorisation and sweeps), the refinement policy and the scenarios themselves, without a GPU.
tests/test_gpu_direct_shapes.py runs the same functions on the device."""
import pytest

import direct_shapes as ds


@pytest.mark.parametrize("row", ds.ROWS, ids=ds.row_id)
def test_manufactured_solution_needs_no_refinement_on_the_host(row):
    ds.manufactured(row, "cpu")


@pytest.mark.parametrize("mesh,k", ds.inertia_ids())
def test_negative_pivots_equal_negative_eigenvalues_on_the_host(mesh, k):
    ds.inertia(mesh, k, "cpu")


def test_table_covers_the_edges_it_names():
    """the table's own arithmetic: which tile and panel counts the rows reach"""
    T = {r.T for r in ds.ROWS}
    assert {1, 2, 3, 5, 6, 7, 8, 9} <= T                                   # odd and even, both sides of the switch at 8
    assert any(r.P == 1 for r in ds.ROWS) and any(r.T > r.P - 1 > 0 for r in ds.ROWS) and any(r.T == r.P - 1 for r in ds.ROWS)
    assert any(r.n % 32 == 0 and r.P > 1 for r in ds.ROWS) and any(r.n % 32 == 0 and r.P == 1 for r in ds.ROWS)
    assert any(r.bw == 32 for r in ds.ROWS) and any(r.bw == 33 for r in ds.ROWS)
    # k_band_update_mfma2's grid (Tp + 1) / 2 and its `mine` mask at Tp = 1, 2, 3: Tp = min(T, P - 1 - p) runs down to 1
    # at the last panels of every row with P > 1
    assert any(r.P > 3 and r.T >= 3 for r in ds.ROWS)
    for r in ds.ROWS:
        assert r.T == -(-r.bw // 32) and r.P == -(-r.n // 32) and r.P <= 110
