"""-m gpu: the persistent one-launch PCG at every slices-per-wave and residency edge (tests/persist_shapes.py): every shape of
the launch ladder -- 3 x 3 blocks with 3 .. 7 slices per wave, 2 x 2 blocks with 3, 4, 6 and 8 -- at grids of 8, 16 and 24
workgroups, the two patterns just above the ceilings (three launches), waves with free slots, workgroups and ranges without a
slice, slices shorter than the register rows, LDS budgets that end inside a slice, at a slice boundary and before slot 0,
prefetched batches of 0 .. 4 rows, each under the variants, register rows and prefetch settings the build carries -- entry by
entry against the long-double recurrence.  One test per (row, configuration); tests/test_persist_shapes_cpu.py checks the
table, its predicates, the fit conditions and the constants on the host backend."""
import pytest

import persist_shapes as pp

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("row", pp.ROWS, ids=pp.row_id)
def test_table(row):
    pp.check_table(row.name, "hip")


@pytest.mark.parametrize("row,cfg", [(r, c) for r in pp.ROWS for c in pp.configs(r)],
                         ids=lambda v: v.name if isinstance(v, pp.Row) else pp.config_id(v))
def test_config(row, cfg):
    pp.check_config(row.name, cfg, "hip")


@pytest.mark.parametrize("row", pp.ROWS, ids=pp.row_id)
def test_once(row):
    pp.check_once(row.name, "hip", fit=row.name not in pp.UNFIT)
