"""The per-record streaming kernels' cases of tests/emit_cases.py without a GPU: every case
through GPUAGG_FLAG_CPU_BACKEND with host memory (Engine::hubble, Engine::decode and
Engine::enrich of gpuagg_cpu.cpp restate hubble_decode_kernel, packet_decode_kernel /
drop_decode_kernel and enrich_kernel) -- the inputs, the references and the host restatements
agree before a device sees them.  Here too: the hash and capacity restatement pinned to
ipc_build.h (compiled host-only with g++), the self-checks of the inputs, and each
vectorised reference pinned to the per-record oracle."""

import os
import subprocess

import numpy as np
import pytest

from . import emit_cases as EC
from . import iptable_cases as IC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", autouse=True)
def lib():
    from retina_amd import _abi, build
    build.build()
    return _abi.load()


# ---- the ipcache image: ipc_build.h against its restatement -------------------------------------

@pytest.fixture(scope="module")
def ipc_images(tmp_path_factory):
    """{image: (capacity, max_probe, [(slot, identity, metadata id) of each input key])} from
    ipc_build of the header, plus "refused": a set with 255.255.255.255."""
    exe = str(tmp_path_factory.mktemp("ipc") / "ipc_build_test")
    subprocess.run(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "retina_amd", "csrc"),
                    os.path.join(ROOT, "tests", "ipc_build_test.cpp"), "-o", exe], check=True)
    sets = [EC.image(name) for name in EC.IMAGES]
    sets.append((np.array([5, EC.IPC_EMPTY, 9], np.uint32),) * 3)
    lines = [str(len(sets))]
    for keys, ident, meta in sets:
        lines.append(str(len(keys)))
        lines.extend("%d %d %d" % t for t in zip(keys.tolist(), ident.tolist(), meta.tolist()))
    out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True,
                         check=True).stdout.strip().split("\n")
    assert len(out) == len(sets)
    res = {}
    for name, ln in zip(EC.IMAGES + ("refused",), out):
        w = [int(x) for x in ln.split()]
        assert w[0] == (name != "refused"), name
        res[name] = (w[1], w[2], list(zip(w[3::3], w[4::3], w[5::3])))
    return res


def test_ipc_restatement_pinned(ipc_images):
    """ip_h1, the seed and the capacity rule as emit_cases restates them place every key of
    every image in the slot ipc_build of the header puts it in, with the same capacity and
    max_probe; the payload there is the last entry's for the key."""
    assert ipc_images["refused"] == (0, 0, [])
    for name in EC.IMAGES:
        keys = EC.image(name)[0]
        cap, max_probe, where = EC.ipc_place(keys)
        got_cap, got_probe, slots = ipc_images[name]
        assert (got_cap, got_probe) == (cap, max_probe), name
        assert len(slots) == len(keys)
        d = EC.image_dict(name)
        for k, (slot, ident, meta) in zip(keys.tolist(), slots):
            assert slot == where[k] and (ident, meta) == d[k], (name, k)
    caps = {name: ipc_images[name][0] for name in EC.IMAGES}
    assert caps == {"n0": 64, "n1": 64, "n32": 64, "n33": 128, "n3000": 8192, "wrap": 64, "dups": 64, "zero": 64}
    assert len(EC.image("n3000")[0]) == 3008


def test_wrap_chain(ipc_images):
    """The "wrap" image, from the header's builder: 20 keys of home slot 62 in 64 slots lie
    in 62, 63, 0, 1 .. 17 and max_probe is 19; the aimed absent addresses have home slots 62
    (the walk covers the whole chain and stops at max_probe without meeting a free slot), 63
    (it meets the free slot 18 at probe 19 = max_probe) and 0 (it enters the chain in the
    middle and meets slot 18 at probe 18)."""
    cap, max_probe, slots = ipc_images["wrap"]
    assert (cap, max_probe) == (EC.WRAP_CAP, EC.WRAP_KEYS - 1) == (64, 19)
    assert [s for s, _, _ in slots] == [(EC.WRAP_HOME + i) % 64 for i in range(20)]
    keys = EC.image("wrap")[0]
    assert (EC.ip_h1(keys) & 63 == 62).all()
    absent = EC.wrap_absent()
    assert not np.isin(absent, keys).any()
    assert (EC.ip_h1(absent) & 63).tolist() == [62] * 8 + [63] * 8 + [0] * 8
    src, dst, st = EC.addresses("wrap")
    for col in (src, dst):
        assert np.isin(absent, col).all() and np.isin(keys, col).all()


def test_dups_and_zero_images():
    keys, ident, meta = EC.image("dups")
    a = keys[1]
    at = np.flatnonzero(keys == a)
    assert at.tolist() == [1, 4, 8]
    assert EC.image_dict("dups")[int(a)] == (int(ident[8]), int(meta[8]))  # the last entry
    src, dst, _ = EC.addresses("dups")
    assert (src == a).any() and (dst == a).any()
    assert 0 in EC.image_dict("zero")
    for name in EC.IMAGES:  # 0.0.0.0 against images with and without that key
        src, dst, _ = EC.addresses(name)
        assert (src == 0).any() and (dst == 0).any()
        assert (src == EC.IPC_EMPTY).any() and (dst == EC.IPC_EMPTY).any()


def test_address_self_checks():
    """Every class at least 20 times in each column of the main case and a quarter to three
    quarters of its sources absent: on the inputs and the reference alone."""
    EC.check_address_stats("n3000")
    src, dst, st = EC.addresses("n3000")
    assert len(src) == len(dst) == 3008 + 8 * 376
    want = EC.hubble_want("main")
    for side in ("src", "dst"):  # the reference sees hits and misses of every payload kind
        ids = want[side + "_identity"]
        assert set(EC.IDENTITIES) <= set(ids.tolist())
        assert set(EC.META_IDS) <= set(want[side + "_meta"].tolist())
    miss = (want["src_identity"] == EC.WORLD) & (want["src_meta"] == EC.NO_META)
    assert 0.25 <= miss.mean() <= 0.75
    hit = np.isin(src, EC.image("n3000")[0])
    near = src[~hit]  # near misses that another key answers, and ones no key does
    assert st["counts"]["src_ip"][1:9].sum() - (~hit).sum() > 100 and len(near) > 1000


def test_meta_product_self_checks():
    meta, dns = EC.meta_product()
    assert len(meta) == 6144
    want = EC.hubble_want("product")
    kinds = np.bincount(want["summary_kind"], minlength=5)
    # verdict 2: drop; 16: DNS; TCP under verdicts 0, 1 and 15; UDP under every verdict but 2 and 16
    per = 6144 // (6 * 8)
    assert kinds.tolist() == [6144 - per * (6 + 6 + 3 + 6), 3 * per, 6 * per, 6 * per, 6 * per]
    dnsrows = want["summary_kind"] == 4
    assert set((want["summary_arg"][dnsrows] >> 30).tolist()) == {0, 1, 2, 3}
    assert (want["summary_arg"][dnsrows] & 0x3FFFFFFF).max() > 1 << 29
    null = EC.hubble_want("product-null-dns")
    assert set(null["summary_arg"][dnsrows].tolist()) == {0, 1 << 30, 2 << 30, 3 << 30}


@pytest.mark.parametrize("cid", ["main", "product", "product-null-dns", "wrap", "dups", "zero", "n0"])
def test_vectorised_hubble_reference_pinned(cid):
    """np.searchsorted over the sorted keys and the table over the meta words give what the
    per-record oracle gives."""
    case = EC.HUBBLE_BY_ID[cid]
    recs = EC.hubble_records(cid)
    EC.check_hubble(EC.hubble_want_vec(case.image, *recs), EC.hubble_want(cid), cid)


# ---- the cases on the CPU backend ---------------------------------------------------------------

def test_broadcast_resolves_to_world():
    EC.check_broadcast(None)


@pytest.mark.parametrize("cid", [c.id for c in EC.HUBBLE_CASES])
def test_hubble_cases_cpu_backend(cid):
    EC.check_hubble_case(cid, None)


def test_hubble_swap_sequence_cpu_backend():
    EC.check_swap_sequence(None)


def test_raw_sweeps_self_checks():
    EC.check_sweeps_selfcheck()


DECODE_SIZES = [(k, n) for k in (EC.PACKET, EC.DROP) for n in EC.SIZES] + [(EC.PACKET, EC.N_PACKET_SWEEP)]


@pytest.fixture(scope="module")
def decoder():
    g = EC.bare_engine(None)
    yield g, EC.Mem(None)
    g.close()


@pytest.mark.parametrize("kind,n", DECODE_SIZES, ids=["%s-%d" % (EC.KIND_NAME[k], n) for k, n in DECODE_SIZES])
def test_decode_sizes_cpu_backend(decoder, kind, n):
    EC.check_decode(*decoder, kind, n)


@pytest.mark.parametrize("kind", [EC.PACKET, EC.DROP], ids=["packet", "drop"])
def test_decode_above_cap_cpu_backend(decoder, kind):
    EC.check_decode(*decoder, kind, EC.decode_above_cap(kind, EC.CPU_N_CU), offset=123456789)


@pytest.mark.parametrize("offset", EC.TIME_OFFSETS)
@pytest.mark.parametrize("kind", [EC.PACKET, EC.DROP], ids=["packet", "drop"])
def test_decode_time_offsets_cpu_backend(decoder, kind, offset):
    EC.check_decode(*decoder, kind, 1025, offset=offset)


@pytest.mark.parametrize("kind", [EC.PACKET, EC.DROP], ids=["packet", "drop"])
def test_decode_optional_outputs_cpu_backend(decoder, kind):
    for present in EC.OPTIONAL_COMBOS:
        EC.check_decode(*decoder, kind, 1025, offset=-1, present=present)


def test_decode_refusals_cpu_backend():
    EC.check_decode_refusals(None)


@pytest.mark.parametrize("kind", [EC.PACKET, EC.DROP], ids=["packet", "drop"])
def test_decode_raw_offsets_cpu_backend(decoder, kind):
    for shift in (16, 32, 48):
        EC.check_decode(*decoder, kind, 1025, raw_shift=shift)


def test_submit_raw_device_cpu_backend():
    EC.check_submit_raw_device(None)


ENRICH = [(f, n) for f in EC.ENRICH_PODS for n in EC.ENRICH_SIZES]


@pytest.mark.parametrize("form,n", ENRICH, ids=["%s-%d" % c for c in ENRICH])
def test_enrich_offsets_cpu_backend(form, n):
    EC.check_enrich_offsets(form, n, None)


@pytest.mark.parametrize("form,path", [("radix", "vec"), ("bucket", "scalar")])
def test_enrich_above_cap_cpu_backend(form, path):
    EC.check_enrich_above_cap(form, path, None)


def test_enrich_inputs_self_checks():
    """The pod sets reach the two HBM forms enrich_kernel has (up to 64 prefixes the `pre`
    table, beyond them cuckoo buckets), and the large cases' sizes are what the launcher's
    arithmetic needs: a second round for some lanes, and a tail."""
    for form, npfx in (("radix", 4), ("bucket", 65)):
        pods, recs = EC.enrich_inputs(form)
        assert len(np.unique(pods.ips & np.uint32(0xFFFF))) == npfx and len(recs) == 1025
        IC.check_mutation_stats(IC.inputs(EC.ENRICH_PODS[form], 1025)[2])
    n, off = EC.enrich_above_cap("vec", 256)
    assert n % 4 == 3 and n // 4 == 8 * 256 * 256 + 256 and off == (0, 0, 0, 0)
    n, off = EC.enrich_above_cap("scalar", 256)
    assert n == 8 * 256 * 256 + 259 and sum(off) == 1
    assert EC.decode_above_cap(EC.PACKET, 256) == 1_049_095 and EC.decode_above_cap(EC.DROP, 256) == 524_547
