"""-m gpu: the one-launch small-system PCG at every bucket and chunk edge (tests/small_shapes.py): all 14 instantiations
k_pcg_small<DM, K, RR>, the K buckets from both sides at n = 2048, 6144 and 12288 (and the two systems just above, declined to
three launches without a time-out), the share boundary at hub rows of 32 and 33 blocks, the launches at and above 48 KiB of
dynamic LDS, and a wave's chunk of a slice empty, short of RR, equal to it and one and two block rows beyond -- x after 1, 2
and 7 iterations entry by entry against the long-double recurrence, and the stop under eps at the iteration the long-double
recurrence names.  tests/test_small_shapes_cpu.py checks the table, its predicates and conditions on the host backend."""
import pytest

import small_shapes as ss

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("row", ss.ROWS, ids=ss.row_id)
def test_table(row):
    ss.check_table(row.name, "hip")


@pytest.mark.parametrize("row", ss.ROWS, ids=ss.row_id)
def test_iterates(row):
    ss.check_iterates(row.name, "hip")


@pytest.mark.parametrize("row", ss.ROWS, ids=ss.row_id)
def test_stop(row):
    ss.check_stop(row.name, "hip")


@pytest.mark.parametrize("poll", (1, 32))
@pytest.mark.parametrize("row", [r for r in ss.ROWS if r.pin[1] <= ss.THREE_MAX_N], ids=ss.row_id)
def test_stop_through_three_launches(row, poll):
    ss.check_stop(row.name, "hip", poll=poll)
