"""Inputs of the node-apiserver latency edge tests, written once and run on both backends:
test_latency_cases_cpu.py (GPUAGG_FLAG_CPU_BACKEND against the oracle, the reduced-replay
proof, the hash pin) and test_gpu_latency_cases.py (gfx950: device columns on and off
their 16-byte boundary, and host-fed batches).

Every case is a small hand-built W.Records with tcp_id and time_ns, its batch split, the
apiserver set of each batch, the metric names and latency_limit, and `expect`: the fields
of the oracle's state that the rows were written to produce, derived by hand from
latency.go's rules (TTL 500 ms, strict expiry, touch on a repeated request, math.Round,
LinearBuckets(0, 0.5, 10), capacity eviction of the least recently touched entry).  A
case whose rows stop reaching its edge fails on the oracle alone (check_expect).

Row order is record order; a row's time is free (the clock is the running maximum)."""

from __future__ import annotations

import functools
from typing import Callable, Dict, List, NamedTuple, Sequence, Tuple

import numpy as np

from oracle import latency as L
from oracle import oracle as O
from oracle import records as R
from retina_amd import _abi
from retina_amd import workloads as W

from .latency_helpers import as_state

T0 = 1_700_000_000 * 10**9  # a second boundary: Time.Nanos of T0 + x is x mod 1e9
MS = 1_000_000
TTL = 500 * MS
SYN, ACK, PSH = W.SYN, W.ACK, W.PSH
NODE, NODE2 = W.ip_le(10, 240, 0, 1), W.ip_le(10, 240, 0, 2)
API0, API1 = W.ip_le(10, 255, 0, 1), W.ip_le(10, 255, 0, 2)
POD_A, POD_B = W.ip_le(10, 0, 0, 1), W.ip_le(10, 0, 0, 2)
FILL = tuple(W.ip_le(10, 254, 0, i) for i in range(1, 66))  # apiserver-set fillers
ALL = (L.LATENCY, L.HANDSHAKE, L.NO_RESPONSE)
PATHS = ("aligned", "misaligned", "host", "cpu")

Row = Tuple[int, int, int, int, int, int, int, int, int, int]
# (time_ns, src, dst, sport, dport, observation point, tcp flags, tcp id, protocol, verdict)


def req(t, sport, tid, flags=ACK | PSH, src=NODE, dst=API0, dport=443, verdict=1, proto=6, obs=3) -> Row:
    """A TO_NETWORK packet src:sport -> dst:dport carrying TSval tid."""
    return (t, src, dst, sport, dport, obs, flags, tid, proto, verdict)


def rep(t, sport, tid, flags=ACK, src=NODE, dst=API0, dport=443, verdict=1, proto=6, obs=2) -> Row:
    """The FROM_NETWORK answer to req(., sport, tid, src=src, dst=dst): mirrored addresses."""
    return (t, dst, src, dport, sport, obs, flags, tid, proto, verdict)


def bg(t) -> Row:
    """A pod-to-pod row without a TCP id: no latency event, but it advances the clock."""
    return (t, POD_A, POD_B, 5000, 80, 3, ACK, 0, 6, 1)


def records(rows: Sequence[Row]) -> W.Records:
    a = np.array(rows, np.uint64).reshape(-1, 10)
    return _columns(a[:, 0], *[a[:, k].astype(np.uint32) for k in range(1, 10)])


def _columns(t, src, dst, sport, dport, obs, flags, tid, proto, verdict) -> W.Records:
    u = np.uint32
    n = len(t)
    meta = W.pack_meta(proto, verdict, np.where(obs == 3, 2, 1), 0, flags, obs=obs)
    return W.Records(np.ascontiguousarray(src, u), np.ascontiguousarray(dst, u), np.full(n, 100, u),
                     np.ascontiguousarray(meta, u), np.ascontiguousarray(sport | (dport << u(16)), u),
                     np.zeros(n, u), [], np.ascontiguousarray(tid, u), np.ascontiguousarray(t, np.uint64))


def placed(n: int, t_bg: int, at: Dict[int, Row]) -> W.Records:
    """n background rows of time t_bg with the rows of `at` at their positions (vectorised:
    the 1026-unit batch is 8.4M rows)."""
    b = bg(t_bg)
    cols = [np.full(n, b[0], np.uint64)] + [np.full(n, b[k], np.uint32) for k in range(1, 10)]
    pos = np.array(sorted(at), np.int64)
    assert len(pos) == len(at) and pos.min() >= 0 and pos.max() < n
    rows = np.array([at[int(p)] for p in pos], np.uint64).reshape(-1, 10)
    for k in range(10):
        cols[k][pos] = rows[:, k].astype(cols[k].dtype)
    return _columns(*cols)


def by_time(rows: List[Row]) -> List[Row]:
    return sorted(rows, key=lambda r: r[0])  # stable: equal times keep their order


# ---- the sort key of the join, restated (pinned to the header by test_latency_cases_cpu) ------
_M = (1 << 64) - 1


def fmix64(k: int) -> int:
    k ^= k >> 33
    k = (k * 0xFF51AFD7ED558CCD) & _M
    k ^= k >> 33
    k = (k * 0xC4CEB9FE1A85EC53) & _M
    return k ^ (k >> 33)


_LAT_SEED = 0x9E3779B97F4A7C15


def lat_key(src: int, dst: int, sport: int, dport: int, tid: int) -> Tuple[int, int]:
    """The exact key of the request src:sport -> dst:dport with TCP id tid."""
    return src | (dst << 32), sport | (dport << 16) | (tid << 32)


def lat_hash(k0: int, k1: int) -> int:
    return fmix64(k0 ^ fmix64(k1 ^ _LAT_SEED))


def colliding(src, dst, sport, dport, tid, sport2, dport2, tid2) -> Tuple[int, int]:
    """(src2, dst2) of the request with ports sport2 -> dport2 and id tid2 whose key has the
    hash of (src, dst, sport, dport, tid): k0' = k0 ^ fmix64(k1 ^ C) ^ fmix64(k1' ^ C)."""
    k0, k1 = lat_key(src, dst, sport, dport, tid)
    _, k1b = lat_key(0, 0, sport2, dport2, tid2)
    k0b = k0 ^ fmix64(k1 ^ _LAT_SEED) ^ fmix64(k1b ^ _LAT_SEED)
    return k0b & 0xFFFFFFFF, k0b >> 32


# ---- the front end's units, restated from launch_latency (gpuagg_runtime.cpp) ------------------
def units(n: int) -> Tuple[int, int]:
    """(units, rows per unit): one wave per >= 8192 rows, unit sizes rounded up to 4 rows."""
    blocks = min(1 << 16, (n + 8191) // 8192)
    return blocks, ((n + blocks - 1) // blocks + 3) & ~3


def unit_bounds(n: int) -> List[int]:
    blocks, chunk = units(n)
    return [min(u * chunk, n) for u in range(blocks + 1)]


# ---- expectations --------------------------------------------------------------------------------
def hist(lats: Sequence[int]) -> Tuple[List[int], int, int]:
    """(buckets, count, sum) of integer millisecond latencies under le 0, 0.5, ..., 4.5, +Inf."""
    b = [0] * 11
    for v in lats:
        b[0 if v <= 0 else 10 if v >= 5 else 2 * v] += 1
    return b, len(lats), sum(lats)


def expect(lats=(), handshakes=(), no_response=0, pending=0, peak_live=0, evictions=0) -> dict:
    lb, lc, ls = hist(lats)
    hb, hc, hs = hist(handshakes)
    return {"latency_buckets": lb, "latency_count": lc, "latency_sum": ls, "handshake_buckets": hb,
            "handshake_count": hc, "handshake_sum": hs, "no_response": no_response, "pending": pending,
            "capacity_evictions": evictions, "peak_live": peak_live}


class Case(NamedTuple):
    id: str
    recs: W.Records
    batches: Tuple[Tuple[int, int], ...]   # row ranges, in order; (a, a) is an n = 0 submit
    api: Tuple[Tuple[int, ...], ...]       # the apiserver set in force during each batch
    names: Tuple[str, ...]
    limit: int                             # latency_limit (0: latency.go's 100000)
    bound: bool                            # some batch exceeds the capacity (capacity_batches >= 1)
    expect: dict                           # the oracle's state, derived by hand
    reduced: bool = False                  # the oracle replays reduced_mask's rows only
    rejected_set: Tuple[int, ...] = ()     # set before the first batch; must fail and change nothing


def _case(cid, recs, exp, batches=None, api=(API0,), names=ALL, limit=0, bound=False, **kw) -> Case:
    n = len(recs)
    batches = tuple(batches) if batches is not None else ((0, n),)
    assert batches[0][0] == 0 and batches[-1][1] == n
    assert all(a[1] == b[0] for a, b in zip(batches[:-1], batches[1:]))
    if api and not isinstance(api[0], tuple):
        api = (tuple(api),) * len(batches)
    elif not api:
        api = ((),) * len(batches)
    assert len(api) == len(batches)
    return Case(cid, recs, batches, tuple(api), tuple(names), limit, bound, exp, **kw)


BUILDERS: Dict[str, Callable[[], Case]] = {}


def builder(cid: str):
    def deco(f):
        assert cid not in BUILDERS
        BUILDERS[cid] = lambda: f(cid)
        return f
    return deco


# ---- time edges: a few dozen rows, one unit ---------------------------------------------------
@builder("ttl-edge-by-event")
def _ttl_event(cid):
    """A reply whose own time is insert + 500 ms is observed (expiry is clock > expires);
    one nanosecond later the entry has expired before the reply and counts no_response."""
    t = T0
    rows = [req(t, 40000, 1), req(t + 1000, 40001, 2), rep(t + TTL, 40000, 1), rep(t + 1000 + TTL + 1, 40001, 2)]
    return _case(cid, records(rows), expect(lats=[500], no_response=1, peak_live=2))


@builder("ttl-edge-by-background")
def _ttl_background(cid):
    """The same two edges with the clock moved by rows that are no events: the replies'
    own times lie before their requests' expiries."""
    t = T0
    rows = [req(t, 40000, 1), req(t + 10, 40001, 2), bg(t + TTL), rep(t + TTL - 1, 40000, 1),
            bg(t + 10 + TTL + 1), rep(t + 400 * MS, 40001, 2)]
    return _case(cid, records(rows), expect(lats=[500], no_response=1, peak_live=2))


@builder("touch-extends")
def _touch(cid):
    """Request, the same request again at +400 ms (a Get hit: expiry = +900 ms), reply at
    +650 ms, at +900 ms (== expires) and at +900 ms + 1 ns (expired)."""
    rows = []
    for k, late in enumerate((650 * MS, 900 * MS, 900 * MS + 1)):
        t = T0 + 1000 * k
        rows += [req(t, 40000 + k, 1 + k), req(t + 400 * MS, 40000 + k, 1 + k), rep(t + late, 40000 + k, 1 + k)]
    return _case(cid, records(by_time(rows)), expect(lats=[650, 900], no_response=1, peak_live=3))


DELTAS = (0, 499_999, 500_000, 1_499_999, 1_500_000, 4_499_999, 4_500_000, 5_500_000)
ROUNDED = (0, 0, 1, 1, 2, 4, 5, 6)  # math.Round(delta / 1e6): half away from zero


@builder("round-positive")
def _round_pos(cid):
    rows = []
    for k, d in enumerate(DELTAS):
        t = T0 + 10 * MS * k
        rows += [req(t, 40000 + k, 1 + k), rep(t + d, 40000 + k, 1 + k)]
    return _case(cid, records(by_time(rows)), expect(lats=ROUNDED, peak_live=1))


@builder("round-negative")
def _round_neg(cid):
    """Time.Nanos differences of -delta: the request 10 ms before a second boundary, kept
    alive by two touches, the reply 1 s - delta after it; and a pair 1 us before / 2 ms
    after a boundary (-998 ms).  All land in bucket 0; the sum is negative."""
    rows = []
    for k, d in enumerate(DELTAS[1:]):
        t = T0 + 3 * 10**9 + 990 * MS + k * MS
        rows += [req(t, 40000 + k, 1 + k), req(t + 400 * MS, 40000 + k, 1 + k), req(t + 800 * MS, 40000 + k, 1 + k),
                 rep(t + 10**9 - d, 40000 + k, 1 + k)]
    t = T0 + 8 * 10**9 + 999_999_000
    rows += [req(t, 40100, 100), rep(t + 2 * MS, 40100, 100)]
    lats = [-x for x in ROUNDED[1:]] + [-998]
    assert sum(lats) == -1017
    return _case(cid, records(by_time(rows)), expect(lats=lats, peak_live=7))


@builder("duplicate-orphan-reuse")
def _dup(cid):
    """A second reply and a reply to no request find nothing; a key is used again after its
    reply (two observations) and after its expiry (no_response, then the new request's
    nanos: 1 ms, not 601)."""
    t = T0
    rows = [req(t, 40000, 1), rep(t + MS, 40000, 1), rep(t + 2 * MS, 40000, 1),
            rep(t + 3 * MS, 40001, 2),
            req(t + 4 * MS, 40002, 3), rep(t + 5 * MS, 40002, 3), req(t + 6 * MS, 40002, 3), rep(t + 8 * MS, 40002, 3),
            req(t + 10 * MS, 40003, 4), req(t + 610 * MS, 40003, 4), rep(t + 611 * MS, 40003, 4)]
    return _case(cid, records(rows), expect(lats=[1, 1, 2, 1], no_response=1, peak_live=1))


@builder("handshake-flags")
def _handshake(cid):
    """SYN answered by SYN+ACK is a handshake only when both sides carry their flags:
    AddTCPFlags runs for verdicts FORWARDED (ToFlow turns 0 into it) and RETRANSMISSION."""
    V_FWD, V_DROP, V_RETRANS = W.V_FWD, W.V_DROP, W.V_RETRANS
    pairs = [  # (request flags, verdict, reply flags, verdict, handshake)
        (SYN, V_FWD, SYN | ACK, V_FWD, True),
        (SYN, V_FWD, ACK, V_FWD, False),
        (SYN, V_FWD, SYN, V_FWD, False),
        (ACK | PSH, V_FWD, SYN | ACK, V_FWD, False),
        (SYN, V_DROP, SYN | ACK, V_FWD, False),       # the request has no flags
        (SYN, V_RETRANS, SYN | ACK, V_RETRANS, True),
        (SYN, V_FWD, SYN | ACK, V_DROP, False),       # the reply has no flags
        (SYN, 0, SYN | ACK, 0, True),                 # verdict 0 is FORWARDED (flow_utils.go:94-96)
    ]
    rows, hs = [], []
    for k, (rf, rv, pf, pv, shake) in enumerate(pairs):
        t = T0 + 10 * MS * k
        rows += [req(t, 40000 + k, 1 + k, flags=rf, verdict=rv), rep(t + 2 * MS, 40000 + k, 1 + k, flags=pf, verdict=pv)]
        hs += [2] if shake else []
    assert len(hs) == 3
    return _case(cid, records(rows), expect(lats=[2] * 8, handshakes=hs, peak_live=1))


@builder("filtered-rows")
def _filters(cid):
    """Rows that are no events although they look like a live key's reply or like a pair of
    their own: observation points 0 and 1, UDP, tcp_id 0, neither address an apiserver."""
    t = T0
    rows = [req(t, 40000, 5),
            rep(t + MS, 40000, 5, obs=0), rep(t + MS + 1, 40000, 5, obs=1),
            req(t + 2 * MS, 40001, 6, proto=17), rep(t + 3 * MS, 40001, 6, proto=17),
            req(t + 4 * MS, 40002, 0), rep(t + 5 * MS, 40002, 0),
            req(t + 6 * MS, 40003, 7, dst=NODE2), rep(t + 7 * MS, 40003, 7, dst=NODE2),
            req(t + 8 * MS, 40004, 8, obs=1), rep(t + 9 * MS, 40004, 8),
            rep(t + 10 * MS, 40000, 5)]
    return _case(cid, records(rows), expect(lats=[10], peak_live=1))


# ---- two and three exact keys in one hash segment -----------------------------------------------
KEY_A = (NODE, API0, 40000, 443, 77)
_B = colliding(*KEY_A, 40001, 443, 78)
_C = colliding(*KEY_A, 40002, 443, 79)
KEY_B = (_B[0], _B[1], 40001, 443, 78)
KEY_C = (_C[0], _C[1], 40002, 443, 79)
COLLIDING_KEYS = (KEY_A, KEY_B, KEY_C)
COLLIDE_API = (API0, KEY_B[1], KEY_C[1])  # the foreign keys pass the filter by their destination


def _kreq(t, key, flags=ACK | PSH):
    return req(t, key[2], key[4], flags=flags, src=key[0], dst=key[1], dport=key[3])


def _krep(t, key, flags=ACK):
    return rep(t, key[2], key[4], flags=flags, src=key[0], dst=key[1], dport=key[3])


def _assert_collide(keys):
    assert len(set(keys)) == len(keys)
    assert len({lat_hash(*lat_key(*k)) for k in keys}) == 1, "the keys no longer share a hash"
    assert KEY_B[:2] == (0xF7ECEDF2, 0xA8BCE8B3)  # worked by hand for the case table


def _collide2_rows():
    a, b, t = KEY_A, KEY_B, T0
    b0 = [_kreq(t, a), _kreq(t + MS, b), _krep(t + 2 * MS, a), _kreq(t + 3 * MS, a)]
    b1 = [_krep(t + 4 * MS, b), _kreq(t + 300 * MS, b), _krep(t + 503 * MS + 1, a), _krep(t + 700 * MS, b)]
    return b0, b1


@builder("collide-2")
def _collide2(cid):
    """A and B interleaved in one segment; both carried over the batch boundary; A's second
    request expires (its reply comes 1 ns late) while B's second one is answered."""
    _assert_collide((KEY_A, KEY_B))
    b0, b1 = _collide2_rows()
    return _case(cid, records(b0 + b1), expect(lats=[2, 3, 400], no_response=1, peak_live=2),
                 batches=[(0, 4), (4, 8)], api=COLLIDE_API)


@builder("collide-2-bound")
def _collide2_bound(cid):
    """The same rows with room for one entry: every Set evicts the other key, uncounted
    (the first walk feeds the live count from a collision segment; the host replays)."""
    _assert_collide((KEY_A, KEY_B))
    b0, b1 = _collide2_rows()
    return _case(cid, records(b0 + b1), expect(lats=[400], peak_live=1, evictions=3),
                 batches=[(0, 4), (4, 8)], api=COLLIDE_API, limit=1, bound=True)


def _collide3_rows():
    a, b, c, t = KEY_A, KEY_B, KEY_C, T0
    b0 = [_kreq(t, a, SYN), _kreq(t + MS, b), _kreq(t + 2 * MS, c), _krep(t + 3 * MS, b),
          _krep(t + 4 * MS, a, SYN | ACK), _kreq(t + 5 * MS, b)]
    b1 = [_krep(t + 7 * MS, c), _kreq(t + 8 * MS, a), _krep(t + 505 * MS + 1, b), _krep(t + 508 * MS, a)]
    return b0, b1


@builder("collide-3")
def _collide3(cid):
    """Three keys in one segment: B and C carried; B's second request expires 1 ns before
    its reply while A's is answered at clock == expires."""
    _assert_collide(COLLIDING_KEYS)
    b0, b1 = _collide3_rows()
    return _case(cid, records(b0 + b1), expect(lats=[2, 4, 5, 500], handshakes=[4], no_response=1, peak_live=3),
                 batches=[(0, 6), (6, 10)], api=COLLIDE_API)


@builder("collide-3-bound")
def _collide3_bound(cid):
    """The same rows with room for two: C's request evicts A, so A's SYN+ACK finds nothing."""
    _assert_collide(COLLIDING_KEYS)
    b0, b1 = _collide3_rows()
    return _case(cid, records(b0 + b1), expect(lats=[2, 5, 500], no_response=1, peak_live=2, evictions=1),
                 batches=[(0, 6), (6, 10)], api=COLLIDE_API, limit=2, bound=True)


# ---- units: mostly background rows of one early time ---------------------------------------------
LATE = T0 + 600 * MS  # a background row of this time expires every request made at T0 + 1 ms


@builder("units-1-of-8192")
def _units1(cid):
    """One unit.  A late background row expires the open requests for the events after it,
    not for the reply before it; the last row of the batch is an event."""
    n = 8192
    assert units(n) == (1, 8192)
    t = T0 + MS
    at = {5: req(t, 40000, 1), 6: req(t, 40001, 2), 7: req(t, 40002, 3), 100: rep(T0 + 3 * MS, 40000, 1),
          4100: bg(LATE), 4200: rep(T0 + 4 * MS, 40002, 3), n - 1: rep(T0 + 5 * MS, 40001, 2)}
    return _case(cid, placed(n, T0, at), expect(lats=[2], no_response=2, peak_live=3))


@builder("units-2-of-8193")
def _units2(cid):
    """Two units, n % 4 == 1.  A request in the last row of unit 0 is answered by the first
    row of unit 1; unit 0's late row (after its events) expires Q only from then on, so
    Q's reply in unit 1 -- early time, the clock handed over -- finds nothing."""
    n = 8193
    b = unit_bounds(n)
    assert b == [0, 4100, 8193]
    t = T0 + MS
    at = {10: req(t, 40000, 1), 11: req(t, 40001, 2), 50: rep(T0 + 3 * MS, 40000, 1), 60: bg(LATE),
          b[1] - 1: req(t, 40002, 3), b[1]: rep(T0 + 2 * MS, 40002, 3), b[1] + 10: rep(T0 + 5 * MS, 40001, 2),
          n - 1: req(t, 40003, 4)}
    return _case(cid, placed(n, T0, at), expect(lats=[2, 1], no_response=1, pending=1, peak_live=2))


N4 = 3 * 8192 + 5


@builder("units-4-middle-jump")
def _units4_jump(cid):
    """Four units, n % 4 == 1.  Unit 2 holds no event, only the late row: the emit pass skips
    it, yet its maximum must expire unit 0's requests P and Q before their replies in unit
    3.  X crosses the boundary of units 0 / 1; R's reply is the last row of unit 1."""
    n = N4
    b = unit_bounds(n)
    assert b == [0, 6148, 12296, 18444, 24581]
    t = T0 + MS
    at = {5: req(t, 40000, 1), 6: req(t, 40001, 2), b[1] - 1: req(t, 40002, 3),
          b[1]: rep(T0 + 2 * MS, 40002, 3), b[1] + 50: req(t, 40003, 4), b[2] - 1: rep(T0 + 4 * MS, 40003, 4),
          b[2] + 100: bg(LATE),
          b[3]: rep(T0 + 3 * MS, 40000, 1), b[3] + 1: rep(T0 + 3 * MS, 40001, 2), n - 1: req(t, 40004, 5)}
    assert not any(b[2] <= p < b[3] and r != bg(LATE) for p, r in at.items())
    return _case(cid, placed(n, T0, at), expect(lats=[1, 3], no_response=2, pending=1, peak_live=3))


@builder("units-4-late-row")
def _units4_late(cid):
    """Unit 0's late row comes after P's reply (observed: no retroactive expiry within the
    unit) and before S's (expired); Q's reply in unit 1 and V's request in unit 2 carry
    early times, so only the handed-over clock can expire Q and date V's expiry."""
    n = N4
    b = unit_bounds(n)
    t = T0 + MS
    at = {5: req(t, 40000, 1), 6: req(t, 40001, 2), 7: req(t, 40002, 3), 100: rep(T0 + 3 * MS, 40000, 1),
          200: bg(LATE), 300: rep(T0 + 4 * MS, 40002, 3),
          b[1] + 5: rep(T0 + 5 * MS, 40001, 2),
          b[2] + 1: req(t, 40003, 4), b[3] + 7: rep(T0 + 9 * MS, 40003, 4)}
    return _case(cid, placed(n, T0, at), expect(lats=[2, 8], no_response=2, peak_live=3))


BIG = "units-1026-scan-per-2"
N_BIG = 1025 * 8192 + 1


@functools.lru_cache(maxsize=1)
def big_case() -> Case:
    """1026 units: lat_scan_kernel's threads take two units each and those from 513 up none.
    Events in the first, the 512th, the 513th and the last unit; clock jumps in units that
    hold no event (300, 700).  About 340 MB of columns: built vectorised, the oracle
    replays reduced_mask's rows."""
    n = N_BIG
    blocks, chunk = units(n)
    assert (blocks, chunk) == (1026, 8188) and (blocks + 1023) // 1024 == 2
    b = unit_bounds(n)
    t = T0 + MS
    at = {0: req(t, 40000, 1), 1: req(t, 40001, 2),
          b[300] + 17: bg(T0 + 100 * MS),
          b[511]: rep(T0 + 3 * MS, 40000, 1), b[512] - 1: req(T0 + 2 * MS, 40002, 3),
          b[512]: rep(T0 + 5 * MS, 40002, 3), b[512] + 1: req(t, 40003, 4),
          b[700] + 4000: bg(T0 + 700 * MS),
          b[1025]: rep(T0 + 2 * MS, 40001, 2), b[1025] + 1: rep(T0 + 2 * MS, 40003, 4), n - 1: req(t, 40004, 5)}
    return _case(BIG, placed(n, T0, at), expect(lats=[2, 3], no_response=2, pending=1, peak_live=2), reduced=True)


# ---- the capacity equality -----------------------------------------------------------------------
def _cap_rows(k_req: int):
    """k_req requests 1 us apart (keys 41000 + k), then a reply to each: latency 1 + k ms."""
    reqs = [req(T0 + 1000 * k, 41000 + k, 100 + k) for k in range(k_req)]
    reps = [rep(T0 + 1000 * k + (1 + k) * MS, 41000 + k, 100 + k) for k in range(k_req)]
    return reqs, reps


@builder("capacity-8-of-8")
def _cap8(cid):
    """`limit` outstanding requests need no eviction: the parallel walk stays valid."""
    reqs, reps = _cap_rows(8)
    return _case(cid, records(reqs + reps), expect(lats=range(1, 9), peak_live=8), limit=8)


@builder("capacity-9-of-8")
def _cap9(cid):
    """One more: exactly one eviction, of the least recently touched (the first) request;
    its reply finds nothing and it is no no_response."""
    reqs, reps = _cap_rows(9)
    return _case(cid, records(reqs + reps), expect(lats=range(2, 10), peak_live=8, evictions=1), limit=8, bound=True)


@builder("capacity-9-touched-carried")
def _cap9_carried(cid):
    """The first request is touched in batch 0 (8 live: not bound), so the ninth request in
    batch 1 evicts the second: the carried entries keep their order of last touch."""
    reqs, reps = _cap_rows(9)
    rows = reqs[:8] + [req(T0 + 8000, 41000, 100)] + [req(T0 + 9000, 41008, 108)] + reps
    lats = [1] + list(range(3, 10))
    return _case(cid, records(rows), expect(lats=lats, peak_live=8, evictions=1), batches=[(0, 9), (9, 19)],
                 limit=8, bound=True)


@builder("capacity-51-of-50-three-units")
def _cap51(cid):
    """51 outstanding requests over three units of a 20000-row batch with latency_limit 50."""
    n = 20000
    b = unit_bounds(n)
    assert b == [0, 6668, 13336, 20000]
    at = {}
    for k in range(51):
        at[b[k // 17] + 10 + 100 * (k % 17)] = req(T0 + MS, 41000 + k, 100 + k)
        at[b[2] + 3000 + k] = rep(T0 + MS + (1 + k % 7) * MS, 41000 + k, 100 + k)
    lats = [1 + k % 7 for k in range(1, 51)]
    assert sum(lats) == 198
    return _case(cid, placed(n, T0, at), expect(lats=lats, peak_live=50, evictions=1), limit=50, bound=True)


# ---- set-up ----------------------------------------------------------------------------------------
def _setup_rows():
    """A handshake (2 ms), a plain pair (3 ms), a request answered 600 ms later (expired by
    then: no_response, the reply unobserved) and one still pending at the end."""
    t = T0
    return [req(t, 40000, 1, flags=SYN), req(t + MS, 40001, 2), rep(t + 2 * MS, 40000, 1, flags=SYN | ACK),
            rep(t + 4 * MS, 40001, 2), req(t + 5 * MS, 40002, 3), rep(t + 605 * MS, 40002, 3),
            req(t + 700 * MS, 40003, 4)]


def _setup_expect(names=ALL, **kw):
    return expect(lats=[2, 3] if L.LATENCY in names else [], handshakes=[2] if L.HANDSHAKE in names else [],
                  no_response=1 if L.NO_RESPONSE in names else 0, pending=1, peak_live=2, **kw)


def _subset(mask: int):
    names = tuple(nm for i, nm in enumerate(ALL) if mask >> i & 1)

    def f(cid):
        return _case(cid, records(_setup_rows()), _setup_expect(names), names=names)
    f.__doc__ = "Metrics %s only: the enabled bits gate the booking, not the state machine." % ", ".join(names)
    return f


for _mask in range(1, 8):
    builder("metrics-" + "".join(c for i, c in enumerate("lhn") if _mask >> i & 1))(_subset(_mask))


@builder("api-set-empty")
def _api0(cid):
    return _case(cid, records(_setup_rows()), expect(), api=())


@builder("api-set-64-match-last")
def _api64(cid):
    """64 apiserver IPs, the one the set-up rows match last.  Then the apiserver as the
    source only of a TO_NETWORK packet, both addresses apiservers, and the first IP of the
    set; requests to the node or to a 65th address stay unmatched."""
    api = FILL[:63] + (API0,)
    t = T0 + 10 * MS
    rows = _setup_rows() + [
        req(t, 40010, 10, src=API0, dst=NODE2), rep(t + 2 * MS, 40010, 10, src=API0, dst=NODE2),
        req(t + 3 * MS, 40011, 11, src=FILL[5], dst=API0), rep(t + 4 * MS, 40011, 11, src=FILL[5], dst=API0),
        req(t + 5 * MS, 40012, 12, dst=FILL[0]), rep(t + 6 * MS, 40012, 12, dst=FILL[0]),
        req(t + 7 * MS, 40013, 13, dst=NODE2), rep(t + 8 * MS, 40013, 13, dst=NODE2),
        req(t + 9 * MS, 40014, 14, dst=FILL[63]), rep(t + 10 * MS, 40014, 14, dst=FILL[63])]
    assert len(api) == 64 and api[-1] == API0 and FILL[63] not in api
    return _case(cid, records(by_time(rows)), expect(lats=[2, 3, 2, 1, 1], handshakes=[2], no_response=1, pending=1,
                                                     peak_live=2), api=api)


@builder("api-set-65-rejected")
def _api65(cid):
    """Setting 65 IPs fails and leaves [API0] in force: the NODE -> NODE2 pair, which the
    refused set would match, stays unobserved."""
    t = T0 + 10 * MS
    rows = _setup_rows() + [req(t, 40013, 13, dst=NODE2), rep(t + MS, 40013, 13, dst=NODE2)]
    return _case(cid, records(by_time(rows)), _setup_expect(), rejected_set=(NODE2,) + FILL[:64])


@builder("api-set-replaced")
def _api_replaced(cid):
    """K is carried out of batch 0; the set then changes, K's reply no longer passes the
    filter, and K expires and counts.  A pair with the new apiserver is observed."""
    t = T0
    rows = [req(t, 40000, 1), req(t + MS, 40001, 2), rep(t + 2 * MS, 40001, 2),
            rep(t + 3 * MS, 40000, 1), req(t + 4 * MS, 40002, 3, dst=API1), rep(t + 6 * MS, 40002, 3, dst=API1),
            bg(LATE)]
    return _case(cid, records(rows), expect(lats=[1, 2], no_response=1, peak_live=2),
                 batches=[(0, 3), (3, 7)], api=((API0,), (API1,)))


# ---- batch shapes ------------------------------------------------------------------------------------
@builder("one-row-batches")
def _one_row(cid):
    """64 batches of one row: every entry is carried, every expiry happens at a batch end."""
    rows = []
    for k in range(20):
        t, key = T0 + 10 * MS * k, (40000 + k, 1 + k)
        rows.append(req(t, *key))
        if k % 4 == 1:
            rows.append(rep(t + 3 * MS, *key))
        elif k % 4 == 2:
            rows += [req(t + 400 * MS, *key), rep(t + 650 * MS, *key)]
        elif k % 4 == 3:
            rows.append(rep(t + 501 * MS, *key))
    rows += [bg(T0 + 37 * MS * j) for j in range(1, 24)] + [bg(T0 + 2 * 10**9)]
    assert len(rows) == 64
    return _case(cid, records(by_time(rows)), expect(lats=[3] * 5 + [650] * 5, no_response=10, peak_live=15),
                 batches=[(i, i + 1) for i in range(64)])


@builder("clock-only-batch-then-empty")
def _clock_only(cid):
    """Batch 1 holds no event and only advances the clock: the three carried requests expire
    in it, so the replies of batch 3 (early times) find nothing.  Batch 2 is an n = 0 submit."""
    t = T0
    rows = [req(t, 40000, 1), req(t + 1, 40001, 2), req(t + 2, 40002, 3)] + [bg(LATE + j) for j in range(5)] + \
           [rep(t + 2 * MS, 40000, 1), rep(t + 2 * MS, 40001, 2), rep(t + 2 * MS, 40002, 3)]
    return _case(cid, records(rows), expect(no_response=3, peak_live=3), batches=[(0, 3), (3, 8), (8, 8), (8, 11)])


@builder("times-before-carried-clock")
def _early_batch(cid):
    """Every time of batch 1 lies before the clock batch 0 left (T0 + 300 ms): nothing
    expires, the replies match (one of them 50 ms `before` its request), and the new
    request's expiry counts from the carried clock."""
    t = T0
    rows = [req(t + 100 * MS, 40000, 1), req(t + 100 * MS, 40001, 2), bg(t + 300 * MS),
            bg(t + MS), rep(t + 101 * MS, 40000, 1), rep(t + 50 * MS, 40001, 2), req(t + 10 * MS, 40002, 3)]
    return _case(cid, records(rows), expect(lats=[1, -50], pending=1, peak_live=2), batches=[(0, 3), (3, 7)])


CASE_IDS = tuple(BUILDERS)         # every case but the 1026-unit one
UNIT3_IDS = ("units-2-of-8193", "units-4-middle-jump", "units-4-late-row", "capacity-51-of-50-three-units")


@functools.lru_cache(maxsize=None)
def case(cid: str) -> Case:
    c = big_case() if cid == BIG else BUILDERS[cid]()
    assert c.id == cid
    return c


# ---- the oracle ------------------------------------------------------------------------------------------
def event_rows(recs: W.Records, api: Sequence[int]) -> np.ndarray:
    """Rows that LatencyMetrics.process_flow may act on under any of the apiserver IPs in
    `api`: TCP, a non-zero TCP id, and an apiserver address."""
    ips = np.array(sorted(api), np.uint32)
    return ((recs.meta & np.uint32(0xFF)) == 6) & (recs.tcp_id != 0) & (np.isin(recs.src_ip, ips) |
                                                                       np.isin(recs.dst_ip, ips))


def reduced_mask(c: Case) -> np.ndarray:
    """By process_flow's own code a row changes the oracle's state only if it is an event
    (event_rows, under the union of the case's apiserver sets) or strictly raises the
    clock, the running maximum of the times: any other row leaves the clock where it was,
    so _expire finds nothing new, and then returns.  The rows of this mask, replayed in
    order, therefore give the state of the full replay
    (test_latency_cases_cpu.test_reduced_replay_equals_full proves it on the multi-unit cases)."""
    t = c.recs.time_ns
    run = np.maximum.accumulate(t)
    raises = np.empty(len(t), bool)
    raises[0] = t[0] > 0
    raises[1:] = t[1:] > run[:-1]
    return event_rows(c.recs, sorted({ip for s in c.api for ip in s})) | raises


def oracle_metrics(c: Case, reduced: bool) -> L.LatencyMetrics:
    m = L.LatencyMetrics(set(c.names), limit=c.limit or L.LIMIT)
    r = c.recs
    keep = reduced_mask(c) if reduced else None
    cur: Tuple[int, ...] = ()
    for (a, b), api in zip(c.batches, c.api):
        if set(api) != set(cur):  # apiserverWatcherCallbackFn between batches
            m.remove_ips([O.int2ip(x) for x in cur if x not in api])
            m.add_ips([O.int2ip(x) for x in api if x not in cur])
            cur = api
        idx = range(a, b) if keep is None else (a + np.flatnonzero(keep[a:b])).tolist()
        for i in idx:
            m.process_flow(R.flow_from_record(int(r.src_ip[i]), int(r.dst_ip[i]), int(r.bytes[i]), int(r.meta[i]),
                                              int(r.ports[i]), 0, {}, int(r.tcp_id[i]), int(r.time_ns[i])))
    return m


@functools.lru_cache(maxsize=None)
def want(cid: str) -> dict:
    """The oracle's state of a case, in gpuagg_latency_state form with the capacity fields:
    computed once, shared by the backends and paths, checked against the case's `expect`."""
    c = case(cid)
    st = as_state(oracle_metrics(c, c.reduced), capacity=True)
    check_expect(c, st)
    return st


def check_expect(c: Case, st: dict) -> None:
    """Non-vacuity: the oracle alone must give what the rows were written to produce."""
    assert set(c.expect) == set(st)
    bad = {k: (st[k], v) for k, v in c.expect.items() if st[k] != v}
    assert not bad, "case %s no longer reaches its edge (oracle, expected): %r" % (c.id, bad)
    assert c.bound == (c.expect["capacity_evictions"] > 0)


# ---- the engine --------------------------------------------------------------------------------------------
def spec_of(c: Case) -> List[dict]:
    return [{"metric_name": nm} for nm in c.names] + \
           [{"metric_name": "forward_count", "source_labels": ["namespace", "podname"]}]


COLUMNS = ("src_ip", "dst_ip", "bytes", "meta", "ports", "dns_id", "tcp_id", "time_ns")


def _device_batch(recs: W.Records, a: int, b: int, device: int, misaligned: bool):
    """Rows [a, b) as device tensors of their own: on a 16-byte boundary (a.vec == 1), or
    every column one element past it (meta, tcp_id and time_ns misaligned: a.vec == 0)."""
    import torch
    dev = torch.device("cuda", device)
    out = []
    for name in COLUMNS:
        col = getattr(recs, name)[a:b]
        t = torch.from_numpy(col.view(np.int64 if name == "time_ns" else np.int32))
        if misaligned:
            t = torch.cat([t.new_zeros(1), t]).to(dev)[1:]
            assert b == a or t.data_ptr() % 16 == t.element_size()
        else:
            t = t.to(dev)
            assert b == a or t.data_ptr() % 16 == 0
        out.append(t)
    return out


def run_case(c: Case, path: str, device: int = 0) -> dict:
    """latency_state of a case fed to a fresh engine by one of PATHS."""
    import pytest
    from retina_amd import GpuAgg
    from retina_amd.engine import GpuAggError
    from .helpers import make_engine
    assert path in PATHS
    kw = dict(latency_limit=c.limit, sparse_capacity_log2=16, wide_list_mib=64)
    if path == "cpu":
        kw["flags"] = _abi.FLAG_CPU_BACKEND
    g = make_engine(W.make_pods(8, seed=1), spec_of(c), False, device, **kw)
    try:
        hb = None
        if path in ("host", "cpu"):
            hb = g.alloc_batch(max(1, max(b - a for a, b in c.batches)))
        cur = None
        for k, ((a, b), api) in enumerate(zip(c.batches, c.api)):
            if api != cur:
                g.set_apiserver_ips(list(api))
                cur = api
            if k == 0 and c.rejected_set:
                assert len(c.rejected_set) == 65
                with pytest.raises(GpuAggError) as err:
                    g.set_apiserver_ips(list(c.rejected_set))
                assert err.value.code == _abi.ECAPACITY
            if hb is not None:
                hb.fill(c.recs, a, b - a)
                g.submit(hb, b - a)
                g.sync()
            else:
                ts = _device_batch(c.recs, a, b, device, path == "misaligned")
                g.submit_device(GpuAgg.device_columns(*ts), b - a)
                g.sync()  # the tensors are freed behind it
                del ts
        return g.latency_state()
    finally:
        g.close()


def check_state(c: Case, st: dict) -> None:
    """Exact equality with the oracle, the capacity fields included."""
    w = want(c.id)
    assert {k: st[k] for k in w} == w
    assert st["limit"] == (c.limit or L.LIMIT)
    if c.bound:
        assert st["capacity_batches"] >= 1
    else:
        assert st["capacity_batches"] == 0
