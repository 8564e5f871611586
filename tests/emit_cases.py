"""Inputs and references of the per-record streaming kernels' tests, written once and run on
both backends: test_emit_cases_cpu.py (GPUAGG_FLAG_CPU_BACKEND, host memory) and
test_gpu_emit_cases.py (gfx950, device memory).

* hubble_decode_kernel (gpuagg_hubble.hip) with the ipcache image gpuagg_ipcache_set builds
  (ipc_build.h): images whose keys are placed by home slot -- the hash and the capacity rule
  are restated here and pinned to the header by tests/ipc_build_test.cpp --, record addresses
  that are keys, near misses of keys (the MUTATIONS of iptable_cases) and absent addresses
  aimed at a probe chain, and the full product of the meta word's fields the summary reads;
* packet_decode_kernel / drop_decode_kernel (gpuagg_decode.hip): the full product of the
  fields the decode reads, every byte it must ignore filled, every optional output, sizes
  around the workgroup, the tile and the launcher's grid cap;
* launch_enrich (gpuagg_kernels.hip): every combination of pointer alignments, sizes around
  the 4-records-a-lane vector, and both paths above the grid cap.

Every comparison is bit-exact.  Every output column is a view into one sentinel-filled buffer
(Guarded) with GUARD sentinel words after it (and before it, for the enrich outputs); reading
the columns back asserts the sentinels unconditionally."""

from __future__ import annotations

import ctypes as C
import functools
import itertools
from typing import Dict, NamedTuple, Optional, Tuple

import numpy as np

from oracle import decode as D
from oracle import hubble as H
from oracle import oracle as O
from oracle import records as R
from retina_amd import _abi
from retina_amd import workloads as W

from . import iptable_cases as IC
from .helpers import oracle_cache

CPU = _abi.FLAG_CPU_BACKEND
GUARD = 64
SENTINEL = 0x5A5AA5A5
CPU_N_CU = 256  # the launchers' n_cu the CPU backend's cases are sized for
U32 = np.uint32


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


# ---- memory of a backend ------------------------------------------------------------------
class Mem:
    """Buffers the engine reads and writes: numpy arrays for the CPU backend (device None),
    torch tensors on a GPU.  Addresses are plain integers."""

    def __init__(self, device: Optional[int] = None):
        self.device = device
        if device is not None:
            import torch
            self.torch = torch
            self.dev = torch.device("cuda", device)

    def n_cu(self) -> int:
        if self.device is None:
            return CPU_N_CU
        return int(self.torch.cuda.get_device_properties(self.device).multi_processor_count)

    def put(self, a: np.ndarray, shift_bytes: int = 0):
        """The bytes of `a`, starting shift_bytes past a 16-byte boundary: (address, owner)."""
        raw = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
        if self.device is None:
            buf = np.zeros(raw.size + shift_bytes + 16, np.uint8)
            off = (-buf.ctypes.data) % 16 + shift_bytes
            buf[off:off + raw.size] = raw
            addr = buf.ctypes.data + off
        else:
            buf = self.torch.zeros(raw.size + shift_bytes, dtype=self.torch.uint8, device=self.dev)
            # (the shared inputs are read-only arrays, which torch does not wrap quietly)
            buf[shift_bytes:].copy_(self.torch.from_numpy(raw if raw.flags.writeable else raw.copy()))
            addr = buf.data_ptr() + shift_bytes
        assert addr % 16 == shift_bytes % 16
        return addr, buf

    def get(self, addr: int, owner, nbytes: int) -> np.ndarray:
        """nbytes at addr of a buffer put() returned, as a host copy."""
        if self.device is None:
            off = addr - owner.ctypes.data
            return owner[off:off + nbytes].copy()
        off = addr - owner.data_ptr()
        return owner[off:off + nbytes].cpu().numpy()

    def sync(self) -> None:
        """The engine runs on its own stream: torch's copies have landed before it starts."""
        if self.device is not None:
            self.torch.cuda.synchronize(self.device)


class Guarded:
    """Output columns as views into one SENTINEL-filled u32 buffer: `pre` sentinel words
    before each column (after rounding up to 16 bytes), `shift` more words to move it off
    the boundary, GUARD sentinel words after it.  cols: (name, words, shift); 0 words is a
    null column.  read() asserts that every word outside the columns is still SENTINEL."""

    def __init__(self, mem: Mem, cols, pre: int = 0):
        self.mem, self.at, cur = mem, {}, 0
        for name, words, shift in cols:
            if not words:
                self.at[name] = None
                continue
            start = ((cur + pre + 3) & ~3) + shift
            self.at[name] = (start, words)
            cur = start + words + GUARD
        self.words = max(cur, GUARD)
        self.addr, self.owner = mem.put(np.full(self.words, SENTINEL, U32))

    def ptr(self, name: str) -> int:
        return 0 if self.at[name] is None else self.addr + 4 * self.at[name][0]

    def read(self) -> Dict[str, np.ndarray]:
        full = self.mem.get(self.addr, self.owner, 4 * self.words).view(U32)
        outside = np.ones(self.words, bool)
        out = {}
        for name, at in self.at.items():
            if at is not None:
                outside[at[0]:at[0] + at[1]] = False
                out[name] = full[at[0]:at[0] + at[1]].copy()
        hit = np.flatnonzero(outside & (full != U32(SENTINEL)))
        assert hit.size == 0, ("guard words written", hit[:8].tolist(), self.at)
        return out


def _p32(addr: int):
    return C.cast(C.c_void_p(addr), _abi.u32p) if addr else None


def columns(src_ip=0, dst_ip=0, nbytes=0, meta=0, ports=0, dns_id=0, tcp_id=0, time_ns=0) -> "_abi.Columns":
    """gpuagg_columns from addresses (0: NULL)."""
    return _abi.Columns(_p32(src_ip), _p32(dst_ip), _p32(nbytes), _p32(meta), _p32(ports), _p32(dns_id),
                        _p32(tcp_id), C.cast(C.c_void_p(time_ns), _abi.u64p) if time_ns else None)


def bare_engine(device: Optional[int]):
    """An engine with no metric and no endpoint (device None: the CPU backend)."""
    from retina_amd import GpuAgg
    g = GpuAgg(device=device or 0, flags=CPU if device is None else 0, max_slots=64, max_ips=64,
               sparse_capacity_log2=16, wide_list_mib=64)
    try:
        g.reconcile([])
    except Exception:
        g.close()
        raise
    return g


def assert_equal(got: np.ndarray, want: np.ndarray, what) -> None:
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (what, "%d rows differ" % bad.size, bad[:5].tolist(), got[bad[:5]].tolist(),
                           want[bad[:5]].tolist())


# ==== Hubble / ipcache =======================================================================
# ---- ip_h1, the seed and the capacity rule, restated (gpuagg_internal.h, ipc_build.h) --------
IPC_SEED, IPC_EMPTY = 0x7F4A7C15, 0xFFFFFFFF
WORLD, NO_META = 2, 0xFFFFFFFF


def ip_h1(ip, seed: int = IPC_SEED):
    """ip_h1 of gpuagg_internal.h over a u32 or an array of them."""
    x = (np.asarray(ip).astype(np.uint64) ^ np.uint64(seed)) & np.uint64(0xFFFFFFFF)
    x ^= x >> np.uint64(16)
    h = (x * np.uint64(0x9E3779B1)) & np.uint64(0xFFFFFFFF)
    return (h ^ (h >> np.uint64(15))).astype(U32)


def ipc_capacity(n: int) -> int:
    cap = 64
    while cap < 2 * n:
        cap <<= 1
    return cap


def ipc_place(keys) -> Tuple[int, int, Dict[int, int]]:
    """(capacity, max_probe, slot of each key) of the image ipc_build makes of `keys`."""
    cap = ipc_capacity(len(keys))
    tab: Dict[int, int] = {}
    where: Dict[int, int] = {}
    max_probe = 0
    for k in (int(x) for x in keys):
        h, p = int(ip_h1(k)) & (cap - 1), 0
        while h in tab and tab[h] != k:
            h, p = (h + 1) & (cap - 1), p + 1
        tab[h] = k
        where[k] = h
        max_probe = max(max_probe, p)
    return cap, max_probe, where


def keys_with_home(slot: int, cap: int, count: int, seed: int, avoid=()) -> np.ndarray:
    """`count` distinct addresses whose home slot in a cap-slot image is `slot`."""
    rng = np.random.default_rng(seed)
    c = np.unique(rng.integers(1, 2**32 - 1, 400 * count * (cap // 64), dtype=np.uint64).astype(U32))
    c = rng.permutation(c[((ip_h1(c) & U32(cap - 1)) == slot) & ~np.isin(c, np.asarray(avoid, U32))])
    assert len(c) >= count
    return c[:count].astype(U32)


# ---- images: (keys, identities, metadata ids) ------------------------------------------------
IDENTITIES = (0, 1, 2, 6, 7, 2**24 - 1, 0xFFFFFFFF)
META_IDS = (0, 0xFFFFFFFE, NO_META)
IMAGES = ("n0", "n1", "n32", "n33", "n3000", "wrap", "dups", "zero")
WRAP_CAP, WRAP_HOME, WRAP_KEYS = 64, 62, 20


def _payloads(n: int, seed: int):
    """The listed identities and metadata ids in turn, other values between them."""
    rng = np.random.default_rng(seed)
    i = np.arange(n)
    ident = np.where(i % 2 == 0, np.asarray(IDENTITIES, np.uint64)[(i // 2) % len(IDENTITIES)],
                     rng.integers(256, 1 << 24, n, dtype=np.uint64)).astype(U32)
    meta = np.where(i % 3 != 2, np.asarray(META_IDS, np.uint64)[(i - i // 3) % len(META_IDS)],
                    i.astype(np.uint64)).astype(U32)
    return ident, meta


@functools.lru_cache(maxsize=None)
def image(name: str):
    """(keys, identities, metadata ids) of an image; shared, never changed.  Key 0 of every
    image has identity 0 and metadata id 0: what a hit on a free slot {0xFFFFFFFF, 0, 0, 0}
    would also return."""
    rng = np.random.default_rng(1000 + IMAGES.index(name))

    def rand(n):
        c = np.unique(rng.integers(1, 2**32 - 1, 2 * n + 8, dtype=np.uint64).astype(U32))
        return rng.permutation(c)[:n].astype(U32)
    if name == "n0":
        keys = np.zeros(0, U32)
    elif name == "n1":
        keys = np.array([W.ip_le(10, 1, 2, 3)], U32)
    elif name in ("n32", "n33"):
        keys = rand(int(name[1:]))
    elif name == "n3000":  # random addresses and a cluster's: near misses of those hit other keys
        keys = np.concatenate([rand(2000), IC.pods_in_prefixes(9, 112).ips.astype(U32)])
        keys = rng.permutation(np.unique(keys)).astype(U32)
    elif name == "wrap":
        keys = keys_with_home(WRAP_HOME, WRAP_CAP, WRAP_KEYS, 77)
    elif name == "dups":  # one key three times, other keys between: the last entry wins
        o = rand(9)
        a = U32(W.ip_le(10, 9, 8, 7))
        keys = np.array([o[0], a, o[1], o[2], a, o[3], o[4], o[5], a, o[6], o[7], o[8]], U32)
    elif name == "zero":
        keys = np.concatenate([rand(7), np.zeros(1, U32), rand(8)]).astype(U32)
    else:
        raise ValueError(name)
    assert not (keys == IPC_EMPTY).any() and ((keys == 0).any() == (name == "zero"))
    ident, meta = _payloads(len(keys), 2000 + IMAGES.index(name))
    if name == "dups":  # three different payloads of the repeated key
        at = np.flatnonzero(keys == keys[1])
        assert len(at) == 3 and len({(int(ident[i]), int(meta[i])) for i in at}) == 3
    else:
        assert len(np.unique(keys)) == len(keys)
    if len(keys) >= 33:
        assert set(IDENTITIES) <= set(ident.tolist()) and set(META_IDS) <= set(meta.tolist())
    return _frozen(keys, ident, meta)


def image_dict(name: Optional[str]) -> Dict[int, Tuple[int, int]]:
    """ip -> (identity, metadata id), the last entry of a key winning; None: no image."""
    if name is None:
        return {}
    keys, ident, meta = image(name)
    return {int(k): (int(i), int(m)) for k, i, m in zip(keys, ident, meta)}


def set_image(g, name: str) -> None:
    keys, ident, meta = image(name)
    g.ipcache_set(keys.tolist(), ident.tolist(), meta.tolist())


# ---- record addresses ----------------------------------------------------------------------
# classes of an address column: 0 a key of the image, 1 + k the k-th MUTATION of a key,
# 9 an absent address aimed at the "wrap" chain
N_CLASSES = 2 + len(IC.MUTATIONS)
WRAP_ABSENT_HOMES = (WRAP_CAP - 2, WRAP_CAP - 1, 0)  # the whole chain; ends at max_probe; enters in the middle


@functools.lru_cache(maxsize=None)
def wrap_absent() -> np.ndarray:
    """8 absent addresses for each of WRAP_ABSENT_HOMES."""
    keys = image("wrap")[0]
    return _frozen(np.concatenate([keys_with_home(h, WRAP_CAP, 8, 500 + h, avoid=keys)
                                   for h in WRAP_ABSENT_HOMES]).astype(U32))


@functools.lru_cache(maxsize=None)
def addresses(name: str, seed: int = 0):
    """(src, dst, statistics) for an image: per column, independently, every key, then each
    of the eight MUTATIONS of as many sampled keys (of random addresses for the empty image),
    then for "wrap" the aimed absent addresses -- in a random order of their own."""
    keys = np.unique(image(name)[0])
    rng = np.random.default_rng(3000 + 17 * IMAGES.index(name) + seed)
    per = max(24, len(keys) // len(IC.MUTATIONS))
    cols, counts = [], {}
    for col in ("src_ip", "dst_ip"):
        base = keys if len(keys) else rng.integers(1, 2**32 - 1, 64, dtype=np.uint64).astype(U32)
        parts, cls = [keys], [np.zeros(len(keys), np.int64)]
        for k, (_, f) in enumerate(IC.MUTATIONS):
            parts.append(f(base[rng.integers(0, len(base), per)].astype(U32)).astype(U32))
            cls.append(np.full(per, 1 + k))
        if name == "wrap":
            parts.append(wrap_absent())
            cls.append(np.full(len(wrap_absent()), N_CLASSES - 1))
        order = rng.permutation(sum(len(p) for p in parts))
        cols.append(np.concatenate(parts).astype(U32)[order])
        counts[col] = np.bincount(np.concatenate(cls)[order], minlength=N_CLASSES)
    st = dict(counts=counts, miss_share=float((~np.isin(cols[0], keys)).mean()))
    return _frozen(cols[0], cols[1]) + (st,)


def check_address_stats(name: str) -> None:
    """The main case does not degenerate: every key in each column, every mutation class at
    least IC.MIN_PER_CLASS times in each column, a quarter to three quarters of the sources
    absent (the bounds of iptable_cases), both one-value classes present."""
    src, dst, st = addresses(name)
    keys = image(name)[0]
    for col, a in (("src_ip", src), ("dst_ip", dst)):
        c = st["counts"][col]
        assert (c[1:1 + len(IC.MUTATIONS)] >= IC.MIN_PER_CLASS).all(), (col, c.tolist())
        assert np.isin(keys, a).all()
        assert (a == IPC_EMPTY).sum() >= IC.MIN_PER_CLASS and (a == 0).sum() >= IC.MIN_PER_CLASS
    assert IC.MISS_SHARE[0] <= st["miss_share"] <= IC.MISS_SHARE[1], st["miss_share"]


# ---- meta words: the full product -------------------------------------------------------------
PROTOS = (0, 1, 6, 17, 58, 255)
VERDICTS = (0, 1, 2, 3, 15, 16, 99, 255)
FLAGS = (0, 1, 0x12, 0x3F)
REASONS = tuple(range(8))
DNS_TYPES = tuple(range(4))
N_PRODUCT = len(PROTOS) * len(VERDICTS) * len(FLAGS) * len(REASONS) * len(DNS_TYPES)
assert N_PRODUCT == 6144
# the DNS dictionary the host would render from; ids 0 .. N_DNS - 1 in interning order
DNS_ENTRIES = [R.DnsEntry(0, ["A"], "a.example.com.", ["10.0.0.1"], 1),
               R.DnsEntry(3, ["AAAA"], "nx.example.com.", [], 0),
               R.DnsEntry(0, [], "noq.example.com.", [], 0),
               R.DnsEntry(0, ["A", "AAAA"], "b.example.com.", ["10.0.0.2", "10.0.0.3"], 2),
               R.DnsEntry(2, ["A"], "last.example.com.", [], 0)]
N_DNS = len(DNS_ENTRIES)
# dns_id column values: 0, the last interned id, and -- for the summary argument only -- ids
# with bits 30 and 31 set (include/gpuagg.h: arg = (dns_id & 0x3FFFFFFF) | DNS type << 30)
DNS_IDS = (0, N_DNS - 1, 1 | 1 << 30, (N_DNS - 1) | 1 << 31, 2 | 3 << 30, 0x3FFFFFFF & ~7 | 3)


@functools.lru_cache(maxsize=None)
def meta_product():
    """(meta words, dns ids) of the 6144 combinations; the bits the summary does not read
    (traffic direction, is_reply, observation point) change from row to row."""
    f = np.array(list(itertools.product(PROTOS, VERDICTS, FLAGS, REASONS, DNS_TYPES)), U32)
    i = np.arange(len(f))
    meta = W.pack_meta(f[:, 0], f[:, 1], i % 3, f[:, 3], f[:, 2], i % 2, f[:, 4], (i // 2) % 4).astype(U32)
    assert len(np.unique(meta & U32(0x37FCFFFF))) == N_PRODUCT  # (proto, verdict, reason, flags, DNS type)
    dns = np.asarray(DNS_IDS, np.uint64)[(i // len(DNS_TYPES)) % len(DNS_IDS)].astype(U32)
    sel = f[:, 1] == 16
    assert {int(x) for x in dns[sel]} == {x & 0xFFFFFFFF for x in DNS_IDS}
    return _frozen(meta, dns)


def product_rows(n: int):
    """n rows of the product, every 997th in turn: a short stretch still mixes the fields."""
    meta, dns = meta_product()
    k = (np.arange(n) * 997) % len(meta)
    return meta[k], dns[k]


def intern_dns(g) -> None:
    for i, e in enumerate(DNS_ENTRIES):
        assert g.dns_intern(e.rcode, e.qtypes, e.query, e.ips, e.num_answers) == i


# ---- references ---------------------------------------------------------------------------------
HUBBLE_OUT = ("src_identity", "dst_identity", "src_meta", "dst_meta", "summary_kind", "summary_arg")
_DD = dict(enumerate(DNS_ENTRIES))


def _summary(meta: int, dns_id: Optional[int]) -> Tuple[int, int]:
    """(summary kind, argument) of one record through records.flow_from_record and
    oracle.hubble.summary; the DNS argument as include/gpuagg.h states it, and the string
    a host renders from it equal to the oracle's."""
    low = (dns_id or 0) & 0x3FFFFFFF  # (a null column: id 0)
    f = R.flow_from_record(1, 2, 0, meta, 0, low if low in _DD else 0, _DD)
    code, payload, text = H.summary(f)
    if code != H.SUM_DNS:
        assert H.render_summary(code, payload) == text
        return code, payload
    arg = low | (((meta >> R.META_DNSTYPE_SHIFT) & 3) << 30)
    if low in _DD:  # (ids past the dictionary: the argument alone)
        e = _DD[arg & 0x3FFFFFFF]
        l7 = {1: "REQUEST", 2: "RESPONSE"}.get(arg >> 30, "UNKNOWN_L7_TYPE")
        assert H.dns_summary(O.DNS(rcode=e.rcode, query=e.query, qtypes=e.qtypes, ips=e.ips), l7) == text
    return code, arg


def hubble_want_records(img: Optional[str], src, dst, meta, dns) -> Dict[str, np.ndarray]:
    """Per record: oracle.hubble.decode_endpoint over a dict (the last entry of a key
    wins) and _summary."""
    d = image_dict(img)
    ipc = {O.int2ip(k): H.IPCacheEntry(i, None if m == NO_META else m) for k, (i, m) in d.items()}
    names = {m: ("p%d" % m, "n%d" % m) for _, m in d.values() if m != NO_META}
    out = {k: np.zeros(len(src), U32) for k in HUBBLE_OUT}
    for r in range(len(src)):
        for side, col in (("src", src), ("dst", dst)):
            ip = O.int2ip(int(col[r]))
            ep = H.decode_endpoint(ipc, names, ip)
            e = ipc.get(ip)
            m = e.meta if e is not None and e.meta is not None else NO_META
            assert ep.id == ep.identity and (ep.pod_name, ep.namespace) == (names[m] if m != NO_META else ("", ""))
            out[side + "_identity"][r], out[side + "_meta"][r] = ep.identity, m
        out["summary_kind"][r], out["summary_arg"][r] = _summary(int(meta[r]), None if dns is None else int(dns[r]))
    return out


@functools.lru_cache(maxsize=None)
def _meta_lut(meta: int) -> Tuple[int, int]:
    return _summary(meta, None)


def hubble_want_vec(img: Optional[str], src, dst, meta, dns) -> Dict[str, np.ndarray]:
    """The same in numpy: the dict as sorted keys under np.searchsorted, the summary as a
    lookup table over the distinct meta words."""
    d = image_dict(img)
    keys = np.array(sorted(d), U32)
    ident = np.array([d[int(k)][0] for k in keys], U32)
    mid = np.array([d[int(k)][1] for k in keys], U32)
    out = {}
    for side, col in (("src", src), ("dst", dst)):
        if len(keys):
            pos = np.minimum(np.searchsorted(keys, col), len(keys) - 1)
            hit = keys[pos] == col
            out[side + "_identity"] = np.where(hit, ident[pos], U32(WORLD)).astype(U32)
            out[side + "_meta"] = np.where(hit, mid[pos], U32(NO_META)).astype(U32)
        else:
            out[side + "_identity"] = np.full(len(col), WORLD, U32)
            out[side + "_meta"] = np.full(len(col), NO_META, U32)
    um, inv = np.unique(meta, return_inverse=True)
    lut = np.array([_meta_lut(int(m)) for m in um], np.uint64).reshape(-1, 2)
    kind, arg = lut[inv, 0].astype(U32), lut[inv, 1].astype(U32)
    if dns is not None:
        arg = np.where(kind == H.SUM_DNS, arg | (dns & U32(0x3FFFFFFF)), arg).astype(U32)
    out["summary_kind"], out["summary_arg"] = kind, arg
    return out


# ---- cases ---------------------------------------------------------------------------------------
class HubbleCase(NamedTuple):
    id: str
    image: str
    recs: str   # "addr": the image's addresses, the meta product tiled over them; "product": the
                # 6144 meta words, the image's addresses tiled over them; "large": above the grid cap
    dns: bool   # with the dns_id column, or null


# launch_hubble: (n + 255) / 256 workgroups of 256 lanes, at most 16 * n_cu; one record a lane
# and round of the grid-stride loop.  Every case but "above-cap" stays below the cap (16 * 256
# * n_cu records): the loop body runs once.  "above-cap": n = 16 * n_cu * 256 + 259, so the
# first 259 lanes run it twice, workgroup 1's lanes 0..2 among them and its other lanes not.
HUBBLE_CASES = [
    HubbleCase("main", "n3000", "addr", True),     # capacity 8192; chains of a random fill
    HubbleCase("n0", "n0", "addr", True),          # 64 free slots: every probe ends at once
    HubbleCase("n1", "n1", "addr", True),
    HubbleCase("n32", "n32", "addr", True),        # capacity 64 at load 1/2
    HubbleCase("n33", "n33", "addr", False),       # capacity 128
    HubbleCase("wrap", "wrap", "addr", True),      # one chain 62, 63, 0 .. 17; max_probe 19
    HubbleCase("dups", "dups", "addr", True),
    HubbleCase("zero", "zero", "addr", True),      # 0.0.0.0 is a key
    HubbleCase("product", "n33", "product", True),
    HubbleCase("product-null-dns", "n33", "product", False),
    HubbleCase("above-cap", "n3000", "large", True),
]
HUBBLE_BY_ID = {c.id: c for c in HUBBLE_CASES}


def hubble_above_cap(n_cu: int) -> int:
    return 16 * n_cu * 256 + 259


@functools.lru_cache(maxsize=None)
def hubble_records(cid: str, n_cu: int = 0):
    """(src, dst, meta, dns ids or None) of a case; n_cu sizes "above-cap" alone."""
    case = HUBBLE_BY_ID[cid]
    src, dst, _ = addresses(case.image)
    meta, dns = meta_product()
    if case.recs == "addr":
        meta, dns = product_rows(len(src))
    elif case.recs == "product":
        src, dst = np.resize(src, len(meta)), np.resize(dst, len(meta))
    else:  # drawn row by row, so that no two stretches of the batch are alike
        rng = np.random.default_rng(99)
        n = hubble_above_cap(n_cu)
        src, dst = src[rng.integers(0, len(src), n)], dst[rng.integers(0, len(dst), n)]
        k = rng.integers(0, len(meta), n)
        meta, dns = meta[k], dns[k]
    cols = _frozen(src.astype(U32), dst.astype(U32), meta.astype(U32))
    return cols + (_frozen(dns.astype(U32)) if case.dns else None,)


@functools.lru_cache(maxsize=None)
def hubble_want(cid: str, n_cu: int = 0):
    """The reference of a case, computed once and shared by the backends: per record, but
    for "above-cap" the vectorised form (pinned to it by test_emit_cases_cpu.py)."""
    case = HUBBLE_BY_ID[cid]
    fn = hubble_want_vec if case.recs == "large" else hubble_want_records
    return fn(case.image, *hubble_records(cid, n_cu))


def run_hubble(g, mem: Mem, src, dst, meta, dns) -> Dict[str, np.ndarray]:
    """gpuagg_hubble_decode_device of the records into guarded columns."""
    n = len(src)
    ins = [mem.put(a) for a in (src, dst, meta)] + ([mem.put(dns)] if dns is not None else [])
    out = Guarded(mem, [(k, n, 0) for k in HUBBLE_OUT])
    cols = columns(src_ip=ins[0][0], dst_ip=ins[1][0], meta=ins[2][0], dns_id=ins[3][0] if dns is not None else 0)
    hc = _abi.HubbleCols(*[_p32(out.ptr(k)) for k in HUBBLE_OUT])
    mem.sync()
    g._check(g.lib.gpuagg_hubble_decode_device(g.h, C.byref(cols), n, C.byref(hc)))
    g.sync()
    got = out.read()
    del ins
    return got


def check_hubble(got, want, what) -> None:
    for k in HUBBLE_OUT:
        assert_equal(got[k], want[k], (what, k))


def check_hubble_case(cid: str, device: Optional[int]) -> None:
    case, mem = HUBBLE_BY_ID[cid], Mem(device)
    n_cu = mem.n_cu() if case.recs == "large" else 0
    recs, want = hubble_records(cid, n_cu), hubble_want(cid, n_cu)
    g = bare_engine(device)
    try:
        intern_dns(g)
        set_image(g, case.image)
        check_hubble(run_hubble(g, mem, *recs), want, cid)
    finally:
        g.close()
    kinds = set(want["summary_kind"].tolist())
    assert kinds == {H.SUM_NONE, H.SUM_TCP, H.SUM_UDP, H.SUM_DROP, H.SUM_DNS} or len(recs[0]) < 300, kinds


def check_broadcast(device: Optional[int]) -> None:
    """255.255.255.255 is the key of a free slot and no ipcache key: as a source or a
    destination it resolves to World with no metadata, whatever the image holds -- not to
    the free slot's zeros, which are identity 0 and the first pod's metadata id."""
    mem = Mem(device)
    key = image("n1")[0][0]
    src = np.array([IPC_EMPTY, key, IPC_EMPTY, key], U32)
    dst = np.array([key, IPC_EMPTY, IPC_EMPTY, key], U32)
    meta = np.full(4, W.pack_meta(17, 1), U32)
    g = bare_engine(device)
    try:
        for img in (None, "n0", "n1", "n3000"):
            if img is not None:
                set_image(g, img)
            got = run_hubble(g, mem, src, dst, meta, None)
            hit = (0, 0) if img == "n1" else (WORLD, NO_META)  # (key 0 of every image: identity 0, id 0)
            for side, col in (("src", src), ("dst", dst)):
                want = np.array([(WORLD, NO_META) if a == IPC_EMPTY else hit for a in col], U32)
                assert_equal(got[side + "_identity"], want[:, 0].copy(), (img, side, "identity"))
                assert_equal(got[side + "_meta"], want[:, 1].copy(), (img, side, "meta"))
    finally:
        g.close()


# the swap sequence: (image or None for "never set", what the step exercises)
SWAP_STEPS = (None, "n32", "n3000", "n0", "n32")


@functools.lru_cache(maxsize=None)
def swap_records():
    """Addresses of both images of the sequence (every key of the small one, 1500 rows of the
    large one's), the meta product tiled over them."""
    s32, d32, _ = addresses("n32")
    s3k, d3k, _ = addresses("n3000")
    src, dst = np.concatenate([s32, s3k[:1500]]), np.concatenate([d32, d3k[:1500]])
    return _frozen(src, dst, *product_rows(len(src)))


def check_swap_sequence(device: Optional[int]) -> None:
    """One engine: no image at all (the decode installs an empty one), 32 keys, 3008 keys (a
    larger capacity: the image is reallocated), n = 0, 32 keys again (the capacity goes
    back); then a refused image (255.255.255.255 as a key: GPUAGG_ERANGE), after which the
    image before it is still in force."""
    from retina_amd import GpuAggError
    mem, recs = Mem(device), swap_records()
    g = bare_engine(device)
    try:
        intern_dns(g)
        for step, img in enumerate(SWAP_STEPS):
            if img is not None:
                set_image(g, img)
            check_hubble(run_hubble(g, mem, *recs), hubble_want_vec(img, *recs), ("swap", step, img))
        keys, ident, meta = image("n33")
        bad = keys.tolist()
        bad[17] = IPC_EMPTY
        with_err = None
        try:
            g.ipcache_set(bad, ident.tolist(), meta.tolist())
        except GpuAggError as e:
            with_err = e.code
        assert with_err == _abi.ERANGE
        check_hubble(run_hubble(g, mem, *recs), hubble_want_vec(SWAP_STEPS[-1], *recs), ("swap", "refused"))
    finally:
        g.close()


# ==== raw decode ==================================================================================
OBS = (0, 1, 2, 3, 4, 255)
TDIRS = (0, 1, 2, 3, 4, 255)
RAW_PROTOS = (0, 1, 6, 17, 132, 255)
FLAG_BYTES = (0, 0x12, 0x3F, 0x40, 0x80, 0xC0, 0xFF)
REPLY_BYTES = (0, 1, 2, 0x80, 0xFF)
N_PACKET_SWEEP = len(OBS) * len(TDIRS) * len(RAW_PROTOS) * len(FLAG_BYTES) * len(REPLY_BYTES)
assert N_PACKET_SWEEP == 7560
DROP_TYPES = tuple(range(9)) + (0xFF, 0x100, 0x107, 0xFFFF)  # 0x100, 0x107: an in-range low byte
N_DROP_SWEEP = len(DROP_TYPES) * len(RAW_PROTOS)
PORTS = (0, 0xFFFF, 0x0100, 0x00FF)
BYTES = (0, 2**32 - 1)
TIME_OFFSETS = (0, 123456789, -1, -2**63)
SIZES = (1, 255, 256, 257, 1023, 1024, 1025)
OPTIONAL = ("ports", "dns_id", "tcp_id", "time_ns")
PACKET, DROP = _abi.RAW_PACKET, _abi.RAW_DROP
KIND_NAME = {PACKET: "packet", DROP: "drop"}


def _pick(rng, n, fixed, period_shift=0):
    """The fixed values in turn and a random u32 after them, row by row."""
    i = (np.arange(n) // (1 + period_shift)) % (len(fixed) + 1)
    r = rng.integers(0, 2**32, n, dtype=np.uint64)
    return np.where(i < len(fixed), np.asarray(fixed + (0,), np.uint64)[i], r)


def _times(rng, n):
    """Record times with a non-zero high dword; 0 and 2^64 - 1 every 7 rows."""
    t = rng.integers(1 << 32, 2**63, n, dtype=np.uint64) * np.uint64(2) + np.uint64(1)
    i = np.arange(n) % 7
    t[i == 3] = 0
    t[i == 5] = np.uint64(2**64 - 1)
    assert ((t >> np.uint64(32)) != 0)[(i != 3)].all()
    return t


@functools.lru_cache(maxsize=None)
def packet_sweep() -> np.ndarray:
    """The 7560 combinations as struct packet records.  Every byte the decode must ignore is
    0xFF or random: the three padding bytes after is_reply, seq, ack_num, the conntrack
    metadata (byte and packet counters), and TSval / TSecr whichever is not used."""
    rng = np.random.default_rng(41)
    n = N_PACKET_SWEEP
    raw = rng.integers(0, 256, (n, D.PACKET_SIZE), dtype=np.uint8)
    raw[::2, 45:48] = 0xFF  # the padding bytes that share a dword with is_reply
    raw[1::2, 45:48] |= 1
    r = raw.reshape(-1).view(D.PACKET_DTYPE)
    f = np.array(list(itertools.product(OBS, TDIRS, RAW_PROTOS, FLAG_BYTES, REPLY_BYTES)), np.uint8)
    r["obs"], r["tdir"], r["proto"], r["flags"], r["is_reply"] = f.T
    r["src_port"] = _pick(rng, n, PORTS)
    r["dst_port"] = _pick(rng, n, PORTS, 4)
    r["bytes"] = _pick(rng, n, BYTES)
    r["t_nsec"] = _times(rng, n)
    r["tsval"] = rng.integers(1, 2**31, n) * 2       # even and odd: never equal, never 0
    r["tsecr"] = rng.integers(1, 2**31, n) * 2 + 1
    assert (raw[:, 45:48] != 0).all() and (r["seq"] != 0).any() and (r["ack_num"] != 0).any()
    for v in PORTS:
        assert (r["src_port"] == v).any() and (r["dst_port"] == v).any()
    return _frozen(r)


@functools.lru_cache(maxsize=None)
def drop_sweep() -> np.ndarray:
    """drop_type x proto, 13 times over with other addresses, ports and times (1014 records);
    in_filtermap and return_val are garbage."""
    rng = np.random.default_rng(43)
    reps = 13
    n = N_DROP_SWEEP * reps
    raw = rng.integers(0, 256, (n, D.DROP_SIZE), dtype=np.uint8)
    r = raw.reshape(-1).view(D.DROP_DTYPE)
    f = np.array(list(itertools.product(DROP_TYPES, RAW_PROTOS)) * reps, np.uint32)
    r["drop_type"], r["proto"] = f[:, 0], f[:, 1]
    r["in_filtermap"] = np.where(np.arange(n) % 2, 0xFF, rng.integers(1, 256, n))
    r["src_port"] = _pick(rng, n, PORTS)
    r["dst_port"] = _pick(rng, n, PORTS, 4)
    r["skb_len"] = _pick(rng, n, BYTES)
    r["ts"] = _times(rng, n)
    assert (r["in_filtermap"] != 0).all() and (r["return_val"] != 0).any()
    return _frozen(r)


def decode_above_cap(kind: int, n_cu: int) -> int:
    """launch_decode caps the grid at 8 * n_cu workgroups.  Packets: a workgroup stages tiles
    of 512 records through one LDS buffer, so with (8 n_cu + 1) * 512 + 7 records workgroup 0
    stages two full tiles in turn and workgroup 1 a full tile, then a 7-record partial one.
    Drops: one record a lane; 8 n_cu * 256 + 259 gives 259 lanes a second round."""
    return (8 * n_cu + 1) * 512 + 7 if kind == PACKET else 8 * n_cu * 256 + 259


@functools.lru_cache(maxsize=4)
def raw_records(kind: int, n: int) -> np.ndarray:
    """n records as bytes: the sweep truncated or tiled; beyond one sweep the addresses are
    the row number and a hash of it, so that a row decoded into another's place shows."""
    sweep = packet_sweep() if kind == PACKET else drop_sweep()
    rows = sweep.view(np.uint8).reshape(len(sweep), -1)  # (as bytes: the padding travels too)
    r = rows[np.arange(n) % len(sweep)].reshape(-1).view(sweep.dtype)
    if n > len(sweep):
        i = np.arange(n, dtype=np.uint64)
        r["src_ip"] = i.astype(U32)
        r["dst_ip"] = ((i * np.uint64(2654435761)) >> np.uint64(7)).astype(U32)
    return _frozen(r.view(np.uint8).reshape(-1))


@functools.lru_cache(maxsize=4)
def decode_want(kind: int, n: int):
    """(oracle.decode's batch, its out-of-range mask) of raw_records(kind, n)."""
    b, bad = (D.decode_packets if kind == PACKET else D.decode_drops)(raw_records(kind, n))
    if n >= (N_PACKET_SWEEP if kind == PACKET else N_DROP_SWEEP):
        assert 0 < bad.sum() < n
    return b, bad


def want_time(t: np.ndarray, offset: int) -> np.ndarray:
    """(t + offset) mod 2^64: what the decode adds to a record time."""
    return (t.astype(np.uint64) + np.uint64(offset % 2**64)).astype(np.uint64)  # (u64 wraps)


def run_decode(g, mem: Mem, kind: int, raw: np.ndarray, n: int, present=OPTIONAL, raw_shift: int = 0, omit=()):
    """gpuagg_decode_device into guarded columns -> {column: array}.  present: the optional
    outputs passed, the others null; omit: required columns passed as null (refused)."""
    words = {k: n for k in ("src_ip", "dst_ip", "bytes", "meta", "ports", "dns_id", "tcp_id")}
    words["time_ns"] = 2 * n
    for k in OPTIONAL:
        if k not in present:
            words[k] = 0
    for k in omit:
        words[k] = 0
    out = Guarded(mem, [(k, w, 0) for k, w in words.items()])
    addr, owner = mem.put(raw, raw_shift)
    cols = columns(out.ptr("src_ip"), out.ptr("dst_ip"), out.ptr("bytes"), out.ptr("meta"), out.ptr("ports"),
                   out.ptr("dns_id"), out.ptr("tcp_id"), out.ptr("time_ns"))
    mem.sync()
    try:
        g._check(g.lib.gpuagg_decode_device(g.h, kind, C.c_void_p(addr), n, C.byref(cols)))
    finally:
        g.sync()
        got = out.read()  # (the guards hold after a refusal too)
    del owner
    if "time_ns" in got:
        got["time_ns"] = got["time_ns"].view(np.uint64)
    return got


def check_decode(g, mem: Mem, kind: int, n: int, offset: int = 0, present=OPTIONAL, raw_shift: int = 0) -> None:
    """One decode on engine g (its decode counters are read as differences)."""
    raw = raw_records(kind, n)
    want, bad = decode_want(kind, n)
    g.set_time_offset(offset)
    before = g.stats()
    got = run_decode(g, mem, kind, raw, n, present, raw_shift)
    what = (KIND_NAME[kind], n, offset, tuple(present), raw_shift)
    assert set(got) == {"src_ip", "dst_ip", "bytes", "meta"} | set(present), what
    for k in ("src_ip", "dst_ip", "bytes", "meta", "ports", "dns_id", "tcp_id"):
        if k in got:
            assert_equal(got[k], getattr(want, k), what + (k,))
    if "time_ns" in got:
        with np.errstate(over="ignore"):
            assert_equal(got["time_ns"], want_time(want.time_ns, offset), what + ("time_ns",))
    after = g.stats()
    assert after["decoded"] - before["decoded"] == n, what
    assert after["decode_out_of_range"] - before["decode_out_of_range"] == int(bad.sum()), what


def check_sweeps_selfcheck() -> None:
    """The sweeps hold what the cases claim, seen through the oracle's decode."""
    b, bad = decode_want(PACKET, N_PACKET_SWEEP)
    r = packet_sweep()
    assert len(np.unique(np.stack([r[k] for k in ("obs", "tdir", "proto", "flags", "is_reply")]), axis=1).T) == 7560
    assert int(bad.sum()) == 7560 // 3  # traffic directions 4 and 255
    assert ((b.meta >> 27) & 1).sum() == 7560 * 4 // 5  # every non-zero is_reply byte
    used = np.where(r["obs"] == 3, r["tsval"], np.where(r["obs"] == 2, r["tsecr"], 0))
    assert np.array_equal(b.tcp_id, used) and (b.tcp_id != 0).sum() == 7560 // 3
    assert (b.time_ns == 0).any() and (b.time_ns == np.uint64(2**64 - 1)).any()
    b, bad = decode_want(DROP, len(drop_sweep()))
    r = drop_sweep()
    assert np.array_equal(bad, r["drop_type"] > 7) and int(bad.sum()) == 5 * len(RAW_PROTOS) * 13
    assert bad[r["drop_type"] == 0x100].all() and bad[r["drop_type"] == 0x107].all()
    assert (b.tcp_id == 0).all() and (b.time_ns == 0).any() and (b.time_ns == np.uint64(2**64 - 1)).any()


OPTIONAL_COMBOS = [tuple(k for k, on in zip(OPTIONAL, bits) if on) for bits in itertools.product((1, 0), repeat=4)]
assert len(OPTIONAL_COMBOS) == 16 and OPTIONAL_COMBOS[0] == OPTIONAL


def check_decode_refusals(device: Optional[int]) -> None:
    """include/gpuagg.h lets ports, dns_id, tcp_id and time_ns be null and nothing else: a null
    src_ip, dst_ip, bytes or meta output is GPUAGG_EINVAL, and nothing is written or counted."""
    from retina_amd import GpuAggError
    mem = Mem(device)
    g = bare_engine(device)
    try:
        for kind in (PACKET, DROP):
            for col in ("src_ip", "dst_ip", "bytes", "meta"):
                code = None
                try:
                    run_decode(g, mem, kind, raw_records(kind, 257), 257, omit=(col,))
                except GpuAggError as e:
                    code = e.code
                assert code == _abi.EINVAL, (KIND_NAME[kind], col, code)
        assert g.stats()["decoded"] == 0
    finally:
        g.close()


def check_submit_raw_device(device: Optional[int]) -> None:
    """gpuagg_submit_raw_device decodes into the engine's own columns (ports and dns_id null
    when no metric reads them): the sweeps' out-of-range rows are counted there too, and the
    rest is aggregated as forwarded / dropped records of no pod."""
    mem = Mem(device)
    pods = IC.pods_in_prefixes(4)
    g = IC.make_case_engine(pods, W.LOCAL_FWD_DROP, False, 0, device)
    try:
        total = 0
        for kind, n in ((PACKET, N_PACKET_SWEEP), (DROP, 1014)):
            addr, owner = mem.put(raw_records(kind, n))
            mem.sync()
            g._check(g.lib.gpuagg_submit_raw_device(g.h, kind, C.c_void_p(addr), n))
            g.sync()
            del owner
            total += int(decode_want(kind, n)[1].sum())
            st = g.stats()
            assert st["decode_out_of_range"] == total, (KIND_NAME[kind], st["decode_out_of_range"], total)
        assert st["decoded"] == N_PACKET_SWEEP + 1014
    finally:
        g.close()


# ==== enrich launcher ================================================================================
# launch_enrich: the vector path (4 records a lane: one 16-byte load per input column, one
# 16-byte store per output) only when src, dst, src_slot and dst_slot are all 16-byte
# aligned; else one record a lane.  (n + 3) / 4 or n lanes in workgroups of 256, at most
# 8 * n_cu of them.  In the vector path n >> 2 vectors go through the first loop and the
# n & 3 records after them through the second (n < 4: the second alone).
ENRICH_PODS = {"radix": (4, "run"), "bucket": (65, "run")}  # the `pre` table; cuckoo buckets
ENRICH_SIZES = (1, 2, 3, 4, 5, 1023, 1024, 1025)
ENRICH_OFFSETS = list(itertools.product((0, 1), repeat=4))  # src, dst, src_slot, dst_slot: elements
assert ENRICH_OFFSETS[0] == (0, 0, 0, 0) and len(ENRICH_OFFSETS) == 16


def enrich_above_cap(path: str, n_cu: int):
    """(n, offsets): "vec": every lane of the capped grid takes a vector, the first 256 a
    second one, and 3 records are left for the scalar tail; "scalar": one pointer one element
    off its boundary, 259 lanes run the loop twice."""
    if path == "vec":
        return 8 * n_cu * 256 * 4 + 4 * 256 + 3, (0, 0, 0, 0)
    return 8 * n_cu * 256 + 259, (0, 0, 1, 0)


def enrich_inputs(form: str):
    """(pods, 1025 near-miss records) of a pod set; shared."""
    pods, recs, _ = IC.inputs(ENRICH_PODS[form], 1025)
    return pods, recs


@functools.lru_cache(maxsize=None)
def enrich_large(form: str, n: int):
    """n addresses a column drawn row by row from the near-miss records."""
    _, recs = enrich_inputs(form)
    rng = np.random.default_rng(7 + n % 1000)
    return _frozen(recs.src_ip[rng.integers(0, len(recs), n)].astype(U32),
                   recs.dst_ip[rng.integers(0, len(recs), n)].astype(U32))


def enrich_engine(form: str, device: Optional[int]):
    """(engine, {(namespace, pod): slot}) with the pod set loaded."""
    pods, recs = enrich_inputs(form)
    g = IC.make_case_engine(pods, [], False, 0, device, recs)
    slot_of = {}
    for ep in pods.endpoints:
        own = ep.owner_refs[0] if ep.owner_refs else (None, None)
        slot_of[(ep.namespace, ep.name)] = g.slot_intern(ep.namespace, ep.name, own[0], own[1])
    return g, slot_of


def enrich_want_oracle(form: str, slot_of, n: int):
    """Enricher.enrich per record (test_gpu_enrich._want) of the first n records."""
    from .test_gpu_enrich import _want
    pods, recs = enrich_inputs(form)
    cut = W.Records(recs.src_ip[:n], recs.dst_ip[:n], recs.bytes[:n], recs.meta[:n], recs.ports[:n],
                    recs.dns_id[:n], recs.dns)
    return _want(oracle_cache(pods), cut, slot_of)


def enrich_want_vec(form: str, slot_of, col: np.ndarray) -> np.ndarray:
    """A dict lookup over the pod IPs in numpy (every pod of these sets has one IP)."""
    pods, _ = enrich_inputs(form)
    order = np.argsort(pods.ips)
    ips = pods.ips[order].astype(U32)
    slots = np.array([slot_of[(e.namespace, e.name)] for e in pods.endpoints], np.int32)[pods.ip_owner][order]
    pos = np.minimum(np.searchsorted(ips, col), len(ips) - 1)
    return np.where(ips[pos] == col, slots[pos], np.int32(-1)).astype(np.int32)


def run_enrich(g, mem: Mem, src, dst, off=(0, 0, 0, 0)):
    """gpuagg_enrich_device with each pointer off[k] elements past a 16-byte boundary; the
    outputs between GUARD sentinel words on both sides -> (src slots, dst slots)."""
    n = len(src)
    a_src, o_src = mem.put(src, 4 * off[0])
    a_dst, o_dst = mem.put(dst, 4 * off[1])
    out = Guarded(mem, [("src_slot", n, off[2]), ("dst_slot", n, off[3])], pre=GUARD)
    for addr, o in zip((a_src, a_dst, out.ptr("src_slot"), out.ptr("dst_slot")), off):
        assert addr % 16 == 4 * o
    cols = columns(src_ip=a_src, dst_ip=a_dst)
    mem.sync()
    g._check(g.lib.gpuagg_enrich_device(g.h, C.byref(cols), n, C.c_void_p(out.ptr("src_slot")),
                                        C.c_void_p(out.ptr("dst_slot"))))
    g.sync()
    got = out.read()
    del o_src, o_dst
    return got["src_slot"].view(np.int32), got["dst_slot"].view(np.int32)


def check_enrich_offsets(form: str, n: int, device: Optional[int]) -> None:
    """All 16 alignments of the four pointers give the oracle's slots (and so each other's);
    the numpy lookup the large cases use gives them too."""
    mem = Mem(device)
    _, recs = enrich_inputs(form)
    src, dst = recs.src_ip[:n].astype(U32), recs.dst_ip[:n].astype(U32)
    g, slot_of = enrich_engine(form, device)
    try:
        ws, wd = enrich_want_oracle(form, slot_of, n)
        assert_equal(enrich_want_vec(form, slot_of, src), ws, (form, n, "numpy lookup, src"))
        assert_equal(enrich_want_vec(form, slot_of, dst), wd, (form, n, "numpy lookup, dst"))
        if n >= 1023:
            assert (ws == -1).mean() > 0.25 and (ws >= 0).mean() > 0.25 and (wd >= 0).any() and (wd == -1).any()
        for off in ENRICH_OFFSETS:
            gs, gd = run_enrich(g, mem, src, dst, off)
            assert_equal(gs, ws, (form, n, off, "src_slot"))
            assert_equal(gd, wd, (form, n, off, "dst_slot"))
    finally:
        g.close()


def check_enrich_above_cap(form: str, path: str, device: Optional[int]) -> None:
    mem = Mem(device)
    n, off = enrich_above_cap(path, mem.n_cu())
    src, dst = enrich_large(form, n)
    g, slot_of = enrich_engine(form, device)
    try:
        ws, wd = enrich_want_vec(form, slot_of, src), enrich_want_vec(form, slot_of, dst)
        assert (ws == -1).mean() > 0.25 and (ws >= 0).mean() > 0.25
        gs, gd = run_enrich(g, mem, src, dst, off)
        assert_equal(gs, ws, (form, path, n, "src_slot"))
        assert_equal(gd, wd, (form, path, n, "dst_slot"))
    finally:
        g.close()
