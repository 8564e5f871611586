"""The latency case table (tests/latency_cases.py) without a GPU: every case reaches its
edge on the oracle alone and matches the CPU backend exactly; the reduced replay that the
1026-unit case relies on equals the full one; and the table's restatement of the join's
sort key is pinned to lat_hash of gpuagg_internal.h, compiled host-only with g++."""

import os
import subprocess

import numpy as np
import pytest

from . import latency_cases as LC
from .latency_helpers import as_state

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("cid", LC.CASE_IDS)
def test_case_reaches_its_edge(cid):
    """check_expect inside: the oracle's state is the one the rows were written for."""
    c = LC.case(cid)
    st = LC.want(cid)
    assert all(b - a >= 0 for a, b in c.batches)
    assert st["capacity_evictions"] == c.expect["capacity_evictions"]


@pytest.mark.parametrize("cid", LC.CASE_IDS)
def test_cpu_backend_matches_oracle(cid):
    c = LC.case(cid)
    LC.check_state(c, LC.run_case(c, "cpu"))


def test_big_case_reaches_its_edge_and_cpu_backend():
    """The 1026-unit batch: the oracle over the reduced rows, the CPU backend over all."""
    c = LC.case(LC.BIG)
    assert int(LC.reduced_mask(c).sum()) == 11  # 9 events (the first row among them), two clock jumps
    try:
        LC.check_state(c, LC.run_case(c, "cpu"))
    finally:
        LC.case.cache_clear()
        LC.big_case.cache_clear()


@pytest.mark.parametrize("cid", LC.UNIT3_IDS)
def test_reduced_replay_equals_full(cid):
    """Replaying only the events and the rows that raise the running maximum of the times
    leaves the oracle in the state of the full replay, every field of it."""
    c = LC.case(cid)
    keep = LC.reduced_mask(c)
    assert 0 < keep.sum() < len(keep) // 50  # a real reduction
    full, red = LC.oracle_metrics(c, False), LC.oracle_metrics(c, True)
    assert as_state(full, capacity=True) == as_state(red, capacity=True)
    assert full.clock == red.clock and list(full.cache.items()) == list(red.cache.items())


@pytest.fixture(scope="module")
def hasher(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("lat") / "lat_hash_test")
    subprocess.run(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "retina_amd", "csrc"),
                    os.path.join(ROOT, "tests", "lat_hash_test.cpp"), "-o", exe], check=True)
    return exe


def test_hash_restatement_matches_header(hasher):
    """The colliding keys of the table and 2000 random ones through lat_hash of the header."""
    rng = np.random.default_rng(7)
    keys = [LC.lat_key(*k) for k in LC.COLLIDING_KEYS]
    keys += [(int(a), int(b)) for a, b in rng.integers(0, 2**64, (2000, 2), dtype=np.uint64)]
    keys += [(0, 0), (2**64 - 1, 2**64 - 1)]
    text = "%d\n" % len(keys) + "".join("%d %d\n" % k for k in keys)
    out = subprocess.run([hasher], input=text, capture_output=True, text=True, check=True).stdout.split()
    assert [int(x) for x in out] == [LC.lat_hash(*k) for k in keys]
    assert len(set(out[:3])) == 1 and len(set(out)) == len(keys) - 2


def test_hash_defined_once():
    """lat_hash lives in the header alone: the kernel file and the runtime do not restate it."""
    src = os.path.join(ROOT, "retina_amd", "csrc")
    files = [f for f in sorted(os.listdir(src)) if f.endswith((".h", ".hip", ".cpp"))]
    hits = [f for f in files if "lat_hash(uint64_t" in open(os.path.join(src, f), encoding="utf-8").read()]
    assert hits == ["gpuagg_internal.h"]
