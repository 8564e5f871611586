"""The state-operation cases of sketch_ops_cases.py on the CPU backend (GPUAGG_FLAG_CPU_BACKEND:
the host threads' accumulators are what waits there, flushed or dropped by the same
fold_pending / drop_pending calls), host-fed.  Their GPU twins are in test_gpu_sketch_ops.py."""

import pytest

from . import sketch_cases as K
from . import sketch_ops_cases as O

BE = K.Backend(None)
FLAGS = pytest.mark.parametrize("flags", list(O.FLAGS.values()), ids=list(O.FLAGS))


@pytest.fixture(scope="module", autouse=True)
def lib():
    from retina_amd import _abi, build
    build.build()
    return _abi.load()


@FLAGS
def test_reset(flags):
    O.reset(BE, flags)


@FLAGS
@pytest.mark.parametrize("same", [True, False], ids=["same-options", "other-options"])
def test_reconcile(flags, same):
    O.reconcile(BE, flags, same)


@FLAGS
def test_load_endpoints(flags):
    O.load_endpoints(BE, flags)


@FLAGS
def test_retire(flags):
    O.retire(BE, flags)


@FLAGS
@pytest.mark.parametrize("peer", [False, True], ids=["default", "peer"])
def test_merge(flags, peer):
    O.merge(BE, flags, peer)


@FLAGS
@pytest.mark.parametrize("which", O.READS)
def test_read(flags, which):
    O.read(BE, flags, which)
