"""The packed fields of a wide segment-list entry, the remote-context counterpart of
test_gpu_scale.test_packed_field_overflow_exact.

A list entry's last word is home:12 | count:12 | bytes:40 (kWideHomeShift = 52,
kWideCountShift = 40 in gpuagg_internal.h), so wide_append may write an update into a list
only while

    count < 2^(52 - 40) = 4,096    and    bytes < 2^40;

anything larger goes straight to the table.  Updates of count 1 never come near either
limit: only the flush of the LDS hot-key cache does, once a key was hit more than 4,095
times -- or for 2^40 bytes -- by one workgroup in one launch.  Two launches sized from the
device's CU count (the engine runs one 1,024-thread workgroup per CU, each over one
contiguous chunk of the batch) take every key across a limit in every workgroup:

launch 1 -- three keys (forwarded pod -> pod, dropped pod -> pod, forwarded pod -> an
  address that is no pod's), each more than 4,095 times a chunk.  The forwarded pair stays
  far below 2^40 bytes, so there the count alone decides; it comes 4,096, 4,097 or 4,098
  times a chunk (by workgroup), twice in the chunk's first 4,096 records -- the first round
  of the workgroup's 1,024 lanes, where the doorkeeper lets the second sighting claim the
  cache entry -- and only later again, so that its cached count passes through exactly
  4,096, the first value the count field cannot hold, in some workgroups.
launch 2 -- one key, 1,024 records a chunk of 2^32 - 1 bytes each: the count stays below
  4,096 and the bytes reach 2^40.

Expected: the C port's series of one 1-byte record of each key, times the key's records
(the count series) or its bytes (the byte series) -- linearity, as in the local test.
Both facts about the input are asserted from the input itself, in numpy."""

import numpy as np
import pytest

from retina_amd import _abi
from retina_amd import workloads as W

from .growth_inputs import (WIDE_BYTES, WIDE_BYTES_LIMIT, WIDE_COUNT_LIMIT, ref_series, snapshot_values,
                            wide_field_batch, wide_field_rows)
from .helpers import diff_series, make_engine, to_device

pytestmark = pytest.mark.gpu

FWD, DROP, EXT = 0, 1, 2  # rows of wide_field_rows()
ROUND = 4096              # records the 1,024 lanes of a workgroup take in one round (4 a lane)
PER_KEY = 4100            # records of each key in a chunk after its first round


def _launch1_keys(cus: int) -> np.ndarray:
    """Key ids of launch 1, (workgroups, chunk)."""
    chunk = ROUND + 3 * PER_KEY
    keys = np.empty((cus, chunk), np.int64)
    first = np.where(np.arange(ROUND) % 2 == 0, DROP, EXT)
    first[[0, ROUND // 2]] = FWD  # two sightings, in different waves
    keys[:, :ROUND] = first
    keys[:, ROUND:] = np.tile([FWD, DROP, EXT], PER_KEY)
    for w in range(cus):  # FWD: 4,096 + w % 3 records in workgroup w, the rest become EXT
        extra = PER_KEY + 2 - (WIDE_COUNT_LIMIT + w % 3)
        tail = ROUND + 3 * np.arange(PER_KEY - extra, PER_KEY)
        keys[w, tail] = EXT
    return keys


def _bytes_for(keys: np.ndarray) -> np.ndarray:
    """Every key cycles through its byte values: FWD the three small ones (count decides),
    DROP all five, EXT the two largest."""
    flat = keys.reshape(-1)
    out = np.empty(flat.shape, np.uint32)
    for k, vals in ((FWD, WIDE_BYTES[:3]), (DROP, WIDE_BYTES), (EXT, WIDE_BYTES[3:])):
        at = np.flatnonzero(flat == k)
        out[at] = np.asarray(vals, np.uint32)[np.arange(len(at)) % len(vals)]
    return out.reshape(keys.shape)


def _per_workgroup(keys, nbytes, cus):
    """(counts, byte sums), each (workgroups, 3), under the engine's split of a batch: chunk =
    ceil(n / workgroups) rounded up to 4 records."""
    n = keys.size
    chunk = ((n + cus - 1) // cus + 3) & ~3
    assert chunk == keys.shape[1] and n == chunk * cus
    cnt = np.stack([(keys == k).sum(1) for k in (FWD, DROP, EXT)], 1)
    byt = np.stack([np.where(keys == k, nbytes.astype(np.uint64), np.uint64(0)).sum(1) for k in (FWD, DROP, EXT)], 1)
    return cnt, byt


@pytest.fixture(scope="module")
def launches(gpu_device):
    """(pods, device columns and length of launch 1 and 2, expected series)."""
    import torch
    cus = torch.cuda.get_device_properties(gpu_device).multi_processor_count
    pods, _ = wide_field_rows()
    k1 = _launch1_keys(cus)
    b1 = _bytes_for(k1)
    k2 = np.full((cus, 1024), DROP, np.int64)
    b2 = np.full(k2.shape, WIDE_BYTES[-1], np.uint32)

    # launch 1: every key crosses the count limit in every workgroup; the forwarded pair by
    # the count alone, passing through each of 4,096 .. 4,098
    cnt, byt = _per_workgroup(k1, b1, cus)
    assert cnt.min() >= WIDE_COUNT_LIMIT, cnt.min(0)
    assert set(cnt[:, FWD].tolist()) == {WIDE_COUNT_LIMIT + j for j in range(min(3, cus))}
    assert byt[:, FWD].max() < WIDE_BYTES_LIMIT // 8
    assert (k1[:, :ROUND] == FWD).sum(1).tolist() == [2] * cus
    # launch 2: the bytes cross their limit (with room for the 1-count entries appended
    # before the key is cached), the count does not
    cnt2, byt2 = _per_workgroup(k2, b2, cus)
    assert cnt2[:, DROP].max() < WIDE_COUNT_LIMIT and byt2[:, DROP].min() >= 2 * WIDE_BYTES_LIMIT
    assert set(np.unique(np.concatenate([b1.reshape(-1), b2.reshape(-1)])).tolist()) == set(WIDE_BYTES)

    want = {}
    for k in (FWD, DROP, EXT):
        n_k = int((k1 == k).sum() + (k2 == k).sum())
        b_k = int(b1[k1 == k].astype(np.uint64).sum() + b2[k2 == k].astype(np.uint64).sum())
        unit = ref_series(pods, wide_field_batch([k], [1]), W.C1_REMOTE, True)
        assert sorted(unit.values()) == [1, 1], unit  # one count and one byte series
        for (metric, labels), _ in unit.items():
            assert (metric, labels) not in want  # three distinct keys
            want[(metric, labels)] = b_k if metric.endswith("_bytes") else n_k
    cols = [to_device(wide_field_batch(k.reshape(-1), b.reshape(-1)), gpu_device) for k, b in ((k1, b1), (k2, b2))]
    return pods, cols, (k1.size, k2.size), want


VARIANTS = [("default", {}),
            # every update a 1-count entry; the fold sums them
            ("no-hot-keys", {"flags": _abi.FLAG_NO_HOT_KEYS}),
            ("narrow-entries", {"flags": _abi.FLAG_NARROW_ENTRIES}),
            ("no-wide-lists", {"flags": _abi.FLAG_NO_WIDE_LISTS}),
            ("growth-from-16", {"sparse_capacity_log2": 4, "sparse_max_log2": 22})]


@pytest.mark.parametrize("name,kw", VARIANTS, ids=[v[0] for v in VARIANTS])
def test_wide_packed_field_overflow_exact(gpu_device, launches, name, kw):
    from retina_amd import GpuAgg
    pods, cols, sizes, want = launches
    g = make_engine(pods, W.C1_REMOTE, True, gpu_device, **kw)
    try:
        for ts, n in zip(cols, sizes):
            g.submit_device(GpuAgg.device_columns(*ts), n)
        got = snapshot_values(g)
        assert g.last_dropped == 0 and g.stats()["sparse_dropped"] == 0
        assert got == want, diff_series(got, want)
        if name == "default":
            assert g.kernel_name().startswith("wide_kernel<"), g.kernel_name()
    finally:
        g.close()
