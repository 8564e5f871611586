"""The state-operation cases of sketch_ops_cases.py on the GPU: gpuagg_reset / drop_pending, a
resetting reconcile, layout_dense with keep, gpuagg_retire_slots (zero_hll_rows_kernel) and the
peer-copy merge (add_u32_kernel, max_u8_kernel, the candidate union), each straight after an
unsynced, unread submit whose count-min and HLL scatter lists still wait.  Their CPU-backend
twins are in test_sketch_ops_cpu.py."""

import pytest

from . import sketch_cases as K
from . import sketch_ops_cases as O

pytestmark = pytest.mark.gpu
FLAGS = pytest.mark.parametrize("flags", list(O.FLAGS.values()), ids=list(O.FLAGS))


@pytest.fixture(scope="module")
def be(gpu_device):
    return K.Backend(gpu_device)


@FLAGS
def test_reset(be, flags):
    O.reset(be, flags)


@FLAGS
@pytest.mark.parametrize("same", [True, False], ids=["same-options", "other-options"])
def test_reconcile(be, flags, same):
    O.reconcile(be, flags, same)


@FLAGS
def test_load_endpoints(be, flags):
    O.load_endpoints(be, flags)


@FLAGS
def test_retire(be, flags):
    O.retire(be, flags)


@FLAGS
@pytest.mark.parametrize("peer", [False, True], ids=["default", "peer"])
def test_merge(be, flags, peer):
    O.merge(be, flags, peer)


@FLAGS
@pytest.mark.parametrize("which", O.READS)
def test_read(be, flags, which):
    O.read(be, flags, which)
