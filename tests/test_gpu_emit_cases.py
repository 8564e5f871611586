"""The per-record streaming kernels at their edges on the device (tests/emit_cases.py: the
inputs, the references and the case tables, shared with test_emit_cases_cpu.py):

* hubble_decode_kernel through gpuagg_hubble_decode_device: images with a probe chain that
  wraps, duplicate keys, 0.0.0.0 as a key and none at all; 255.255.255.255 and every other
  near miss of a key as an address; the full product of the meta word; image swaps;
* packet_decode_kernel / drop_decode_kernel through gpuagg_decode_device: the full product of
  the fields read with every ignored byte filled, every optional output, time offsets,
  sizes around the workgroup and the tile, raw buffers 16, 32 and 48 bytes into their
  allocation, and one size above the launcher's grid cap for each kind;
* enrich_kernel through gpuagg_enrich_device: all 16 alignments of its four pointers at sizes
  around the 4-record vector, and the vector and the scalar path above the grid cap.

Bit-exact throughout; every output lies in a sentinel-filled buffer whose guard words are
checked after every run."""

import pytest

from . import emit_cases as EC

pytestmark = pytest.mark.gpu


# ---- hubble_decode_kernel ------------------------------------------------------------------------

def test_broadcast_resolves_to_world(gpu_device):
    EC.check_broadcast(gpu_device)


@pytest.mark.parametrize("cid", [c.id for c in EC.HUBBLE_CASES])
def test_hubble_cases(gpu_device, cid):
    EC.check_hubble_case(cid, gpu_device)


def test_hubble_swap_sequence(gpu_device):
    EC.check_swap_sequence(gpu_device)


# ---- packet_decode_kernel / drop_decode_kernel -------------------------------------------------------

KINDS = pytest.mark.parametrize("kind", [EC.PACKET, EC.DROP], ids=["packet", "drop"])
DECODE_SIZES = [(k, n) for k in (EC.PACKET, EC.DROP) for n in EC.SIZES] + [(EC.PACKET, EC.N_PACKET_SWEEP)]


@pytest.fixture(scope="module")
def decoder(gpu_device):
    g = EC.bare_engine(gpu_device)
    yield g, EC.Mem(gpu_device)
    g.close()


@pytest.mark.parametrize("kind,n", DECODE_SIZES, ids=["%s-%d" % (EC.KIND_NAME[k], n) for k, n in DECODE_SIZES])
def test_decode_sizes(decoder, kind, n):
    EC.check_decode(*decoder, kind, n)


@KINDS
def test_decode_above_cap(decoder, kind):
    g, mem = decoder
    EC.check_decode(g, mem, kind, EC.decode_above_cap(kind, mem.n_cu()), offset=123456789)


@pytest.mark.parametrize("offset", EC.TIME_OFFSETS)
@KINDS
def test_decode_time_offsets(decoder, kind, offset):
    EC.check_decode(*decoder, kind, 1025, offset=offset)


@KINDS
def test_decode_optional_outputs(decoder, kind):
    for present in EC.OPTIONAL_COMBOS:
        EC.check_decode(*decoder, kind, 1025, offset=-1, present=present)


def test_decode_refusals(gpu_device):
    EC.check_decode_refusals(gpu_device)


@KINDS
def test_decode_raw_offsets(decoder, kind):
    for shift in (16, 32, 48):
        EC.check_decode(*decoder, kind, 1025, raw_shift=shift)


def test_submit_raw_device(gpu_device):
    EC.check_submit_raw_device(gpu_device)


# ---- enrich_kernel -------------------------------------------------------------------------------

ENRICH = [(f, n) for f in EC.ENRICH_PODS for n in EC.ENRICH_SIZES]


@pytest.mark.parametrize("form,n", ENRICH, ids=["%s-%d" % c for c in ENRICH])
def test_enrich_offsets(gpu_device, form, n):
    EC.check_enrich_offsets(form, n, gpu_device)


@pytest.mark.parametrize("form,path", [("radix", "vec"), ("bucket", "scalar")])
def test_enrich_above_cap(gpu_device, form, path):
    EC.check_enrich_above_cap(form, path, gpu_device)
