"""The driver's call traces on the device against tests/golden/driver_calls.json, which was recorded on the host backend: the
decks of tests/driver_calls_cases.py whose trace does not depend on the arithmetic of the backend."""
import pytest

import driver_calls_cases as dcc

pytestmark = pytest.mark.gpu
BACKEND = "hip"


@pytest.mark.parametrize("name", dcc.DEVICE_CASES)
def test_driver_calls(tmp_path, name):
    dcc.check(name, tmp_path, BACKEND)
