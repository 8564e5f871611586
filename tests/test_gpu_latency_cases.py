"""The latency case table (tests/latency_cases.py) on gfx950: every case fed as device
columns on their 16-byte boundary (a.vec == 1), one element past it (a.vec == 0) and
host-fed, against the oracle: the whole latency_state, capacity fields included, exactly."""

import pytest

from . import latency_cases as LC

pytestmark = pytest.mark.gpu

GPU_PATHS = ("aligned", "misaligned", "host")


@pytest.mark.parametrize("path", GPU_PATHS)
@pytest.mark.parametrize("cid", LC.CASE_IDS)
def test_case_matches_oracle(gpu_device, cid, path):
    c = LC.case(cid)
    LC.check_state(c, LC.run_case(c, path, gpu_device))


@pytest.fixture(scope="module")
def big():
    yield LC.case(LC.BIG)
    LC.case.cache_clear()  # 340 MB of columns
    LC.big_case.cache_clear()


@pytest.mark.parametrize("path", GPU_PATHS)
def test_1026_units_match_oracle(gpu_device, big, path):
    """lat_scan_kernel with two units a thread and idle threads from 513 up; events in the
    first, the 512th, the 513th and the last unit."""
    assert LC.units(len(big.recs))[0] == 1026
    LC.check_state(big, LC.run_case(big, path, gpu_device))
