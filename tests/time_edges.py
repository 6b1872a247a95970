"""Shared streams for the time-edge tests (no GPU).

Every pattern, window and multi-query kernel stores an event's time as a
32-bit offset from the first row of its chunk (unsigned on the event-time
closed form, biased by 2^31 on the order-tolerant closed form and the hot-key
scans, signed on the general, window and multi-query paths) and rebuilds the
64-bit value when it compares against `within` or a window length.  The
seeded generator only ever produces consecutive milliseconds from
workload.T0, so these helpers move a generated stream along the time axis:

    remap(w, base, jumps): ts'[i] = base + (ts[i] - ts[0]) + sum of J for every
                           (row, J) in jumps with row <= i

Order is preserved, so every oracle applies unchanged.  BASES puts the stream
across the lines where a wrong decode shows (zero, 2^31, 2^32, the wrap of the
low word of a realistic epoch, the far ends of int64); the jump sets put the
`within` edge on tile, chunk and batch borders (`edge`), stretch one chunk to
the widest span every path accepts (`wide`), and let partials live across
chunks whose bases lie more than 2^31 ms apart (`long_within`).

|ts| stays within 2^62 + 2^41, so no int64 difference overflows.
"""
from __future__ import annotations

import numpy as np

from flink_siddhi import workload

T0 = workload.T0
W = 10_000                      # `within 10 sec` in ms
N = 1 << 15
KEYS = 64
CHUNK = 8192                    # chunk_events: one closed-form tile
SIZES = (20481, N - 20481)      # two batches split at an odd row
SPAN_MAX = (1 << 31) - 1        # widest accepted distance from a chunk's first row

BASES = {
    "T0": T0,
    "zero": 0,
    "neg5000": -5000,                        # crosses zero
    "2^31": (1 << 31) - 9000,                # |ts| crosses 2^31
    "2^32": (1 << 32) - 9000,                # |ts| crosses 2^32
    "epoch_wrap": 349 * (1 << 32) - 7000,    # low word of a realistic epoch wraps
    "neg2^32": -(1 << 32) - 7000,
    "2^62": 1 << 62,
    "neg2^62": -(1 << 62),
}
# T0 and the non-control bases every path runs with the `edge` jumps: a
# negative one, a zero-crossing one, 2^32-wrapping ones and a far one
GPU_BASES = ("T0", "neg5000", "epoch_wrap", "neg2^32", "2^62")
WIDE_BASES = ("neg5000", "epoch_wrap")

TS_LIMIT = (1 << 62) + (1 << 41)

DAY = 86_400_000
LONG_WITHIN = {"30 days": 30 * DAY, "1 year": 31_556_900_000}   # SiddhiQL's year
LONG_N = 1 << 16
LONG_SIZES = (36865, LONG_N - 36865)
LONG_JUMP = (1 << 31) - 20000
EDGE_KEY = 5
LONG_KEY_1, LONG_KEY_2 = 62, 63


def chunk_starts(sizes, chunk=CHUNK):
    """First row of every chunk when batches of `sizes` rows are sent in order."""
    out, first = [], 0
    for n in sizes:
        out.extend(range(first, first + n, chunk))
        first += n
    return out


def remap(w, base, jumps=()):
    """The rows of `w` with ts' = base + (ts - ts[0]) + the jumps at or before
    each row, as int64.  `ts` is both the event time and the `ts` attribute."""
    ts = w["ts"].astype(np.int64)
    rel = ts - ts[0]
    add = np.zeros(len(ts), np.int64)
    for row, j in jumps:
        add[row:] += j
    out = {c: v.copy() for c, v in w.items()}
    out["ts"] = (np.int64(base) + rel + add).astype(np.int64)
    assert int(np.abs(out["ts"]).max()) <= TS_LIMIT
    return out


def shifted(w, delta):
    out = {c: v.copy() for c, v in w.items()}
    out["ts"] = out["ts"] + np.int64(delta)
    return out


def plant_pair(w, r, key=EDGE_KEY):
    """Rows r-1 and r become an f-passing A and a g-passing B of one key
    (PATTERN_PLAN: A[price > 0.5] -> B[id % 7 == 0], and SHORT_PLAN).  The
    prices also make them an A and a B under three_streams()."""
    w["k"][r - 1] = w["k"][r] = key
    w["stream"][r - 1], w["price"][r - 1] = 0, 0.9
    w["stream"][r], w["id"][r], w["price"][r] = 1, 14, 0.1


_gen = {}


def generated(n=N, keys=KEYS):
    if (n, keys) not in _gen:
        _gen[(n, keys)] = workload.generate(0, n, keys, rate=1)
    return {c: v.copy() for c, v in _gen[(n, keys)].items()}


# ---- jump sets ---------------------------------------------------------------
def edge_stream(base, n=N, keys=KEYS, sizes=SIZES):
    """J = W-1 at a mid-tile row and at the batch border (the pair planted
    across it is exactly W apart: it matches), J = W at a chunk border (the
    pair planted across it is W+1 apart: it does not)."""
    w = generated(n, keys)
    jumps = ((4001, W - 1), (16384, W), (sizes[0], W - 1))
    assert 16384 in chunk_starts(sizes) and 4001 not in chunk_starts(sizes)
    for r, _ in jumps:
        plant_pair(w, r)
    return remap(w, base, jumps), jumps


def wide_stream(base, n=N, keys=KEYS, sizes=SIZES, chunk=CHUNK, which=1):
    """Chunk number `which` (a full one) ends exactly 2^31 - 1 ms after its
    first row (one jump inside it), and a 2^40 jump sits on the next chunk
    border: the chunk base moves and all state expires."""
    w = generated(n, keys)
    starts = chunk_starts(sizes, chunk)
    c0, c1 = starts[which], starts[which + 1]
    assert c1 - c0 == chunk
    jumps = ((c0 + chunk // 2 - 95, SPAN_MAX - (chunk - 1)), (c1, 1 << 40))
    out = remap(w, base, jumps)
    assert int(out["ts"][c1 - 1] - out["ts"][c0]) == SPAN_MAX
    return out, jumps


def long_stream(base):
    """2^16 rows; jumps of 2^31 - 20000 at two chunk borders, one in each
    batch.  Key 62 has three A's in the first chunk and its first B 20000+
    rows later, across the first jump only: t2 - t1 > 2^31 and < 30 days.  Key
    63 has two A's in the first chunk and its first B after the second jump:
    t2 - t1 > 2^32, alive under `within 1 year`, expired under `within 30
    days`.  (Two jumps of this size put t2 - t1 past 2^32 only when the pair
    is more than 40000 rows apart, hence 2^16 rows here and not 2^15.)"""
    n = LONG_N
    w = generated(n, KEYS)
    starts = chunk_starts(LONG_SIZES)
    j1, j2 = starts[1], starts[-2]
    assert j1 == CHUNK and j2 > LONG_SIZES[0] and j2 < 60000
    for key in (LONG_KEY_1, LONG_KEY_2):
        w["k"][w["k"] == key] -= 2
    for key, a_rows, b_row in ((LONG_KEY_1, (100, 4000, 8000), 30001), (LONG_KEY_2, (200, 5000), 60001)):
        for r in a_rows:
            w["k"][r], w["stream"][r], w["price"][r] = key, 0, 0.75
        w["k"][b_row], w["stream"][b_row], w["id"][b_row], w["price"][b_row] = key, 1, 14, 0.1
        # a g-failing B 1000 rows on (no partial is left for it to expire);
        # under three_streams() the three kinds of row are an A, a B and a C
        c_row = b_row + 1000
        w["k"][c_row], w["stream"][c_row], w["id"][c_row], w["price"][c_row] = key, 1, 1, 0.2
    jumps = ((j1, LONG_JUMP), (j2, LONG_JUMP))
    return remap(w, base, jumps), jumps


def records_wide_stream(base, n_per=CHUNK, world=2, steps=2, key=4):
    """For the two-rank key shuffle: `steps` steps of `world` senders with
    n_per rows each.  The first and the last row of step 0 are kept rows of
    one key, so their owner receives both in one chunk, exactly 2^31 - 1 ms
    apart; a 2^40 jump sits on the step border."""
    n, step = n_per * world * steps, n_per * world
    w = generated(n, KEYS)
    w["k"][0], w["stream"][0], w["price"][0] = key, 0, 0.9
    w["k"][step - 1], w["stream"][step - 1], w["id"][step - 1] = key, 1, 14
    jumps = ((step // 2 + 777, SPAN_MAX - (step - 1)), (step, 1 << 40))
    out = remap(w, base, jumps)
    assert int(out["ts"][step - 1] - out["ts"][0]) == SPAN_MAX
    return out, jumps


_streams = {}


def stream(jump_set, base_name):
    """(rows, jumps, batch sizes) of a named jump set at a named base, built once."""
    key = (jump_set, base_name)
    if key not in _streams:
        base = BASES[base_name]
        if jump_set == "edge":
            w, j = edge_stream(base)
            _streams[key] = (w, j, SIZES)
        elif jump_set == "wide":
            w, j = wide_stream(base)
            _streams[key] = (w, j, SIZES)
        elif jump_set == "wide16k":     # for paths whose chunks hold 16384 rows
            w, j = wide_stream(base, chunk=2 * CHUNK, which=0)
            _streams[key] = (w, j, SIZES)
        elif jump_set == "long_within":
            w, j = long_stream(base)
            _streams[key] = (w, j, LONG_SIZES)
        else:
            raise KeyError(jump_set)
    w, j, sizes = _streams[key]
    return {c: v.copy() for c, v in w.items()}, j, sizes


def plan_within(text, plan=workload.PATTERN_PLAN):
    return plan.replace("within 10 sec", "within " + text)


def three_streams(w):
    """The N-state tests' stream assignment: A / B / C by price."""
    out = {c: v.copy() for c, v in w.items()}
    out["stream"] = ((out["price"] * 1000).astype(np.int64) % 3).astype(np.uint8)
    return out


def late_blocks(w, sizes, chunk=CHUNK, at=1000, rows=50, back=3000):
    """A block of `rows` rows moved `back` ms back in every chunk; with at <
    back they lie before the chunk's first row (negative offsets)."""
    out = {c: v.copy() for c, v in w.items()}
    n = len(out["ts"])
    for c0 in chunk_starts(sizes, chunk):
        if c0 + at + rows <= min(n, c0 + chunk):
            out["ts"][c0 + at:c0 + at + rows] -= back
            assert out["ts"][c0 + at] < out["ts"][c0]
    return out


def hot_key(w, key=17, share=4):
    """One key on 1 / share of the rows (about 650 kept records per 8192-row
    chunk at share 4, against the hot-key threshold of 256)."""
    out = {c: v.copy() for c, v in w.items()}
    pick = workload.splitmix64(np.arange(len(out["k"]), dtype=np.uint64) ^ np.uint64(0xABCDEF)) % np.uint64(share) == 0
    pick &= ~np.isin(out["k"], (EDGE_KEY, LONG_KEY_1, LONG_KEY_2))   # the planted rows keep their keys
    out["k"] = np.where(pick, key, out["k"]).astype(np.int32)
    return out


def span_stream(base, s_ms, chunk=CHUNK, keys=KEYS):
    """Three chunks in order; the second chunk's last row lies s_ms after that chunk's first row."""
    w = generated(3 * chunk, keys)
    out = remap(w, base, ((chunk + chunk // 2, s_ms - (chunk - 1)),))
    assert int(out["ts"][2 * chunk - 1] - out["ts"][chunk]) == s_ms and (np.diff(out["ts"]) >= 0).all()
    return out


# ---- references --------------------------------------------------------------
# The general two-state walk keeps a key's partials in 16 LDS slots and has no
# overflow pool; PATTERN_PLAN's lists outgrow that with 64 keys (at any base).
# This plan keeps them short: fewer A's pass f, every other B passes g.
SHORT_F, SHORT_G = 0.7, 2
SHORT_PLAN = workload.PATTERN_PLAN.replace("price > 0.5", "price > 0.7").replace("id % 7 == 0", "id % 2 == 0")


def c_pairs(w, within=W, keys=KEYS, f_above=0.5, g_mod=7):
    """oracle/cep_oracle.c on PATTERN_PLAN's conditions (or SHORT_PLAN's:
    f_above = SHORT_F, g_mod = SHORT_G): matched (A row, B row) index arrays."""
    import cep_oracle as CO
    f = CO.cond(("price", 0, ">", f_above))
    g = CO.cond(("id", g_mod, "==", 0))
    a, b, m = CO.PatternOracle(keys, f, g, every=True, within=within).run(w)
    assert m == len(a)
    return a, b


def pair_rows(w, a, b):
    """PATTERN_PLAN's output rows of the pairs, as helpers.engine_rows gives them."""
    k, p, ts = w["k"].tolist(), w["price"].tolist(), w["ts"].tolist()
    return [(ts[j], j, (k[i], p[i], p[j], ts[j])) for i, j in zip(a.tolist(), b.tolist())]


def pair_columns(w, a, b):
    """The same rows as the column dict assert_same_per_key compares."""
    return {"k": w["k"][a], "p1": w["price"][a], "p2": w["price"][b], "t": w["ts"][b], "ts": w["ts"][b], "seq": b}


def rows_columns(rows):
    """[(ts, seq, (k, p1, p2, t))] -> the column dict assert_same_per_key compares."""
    return {"k": np.array([r[2][0] for r in rows], np.int64), "p1": np.array([r[2][1] for r in rows], np.float64),
            "p2": np.array([r[2][2] for r in rows], np.float64), "t": np.array([r[2][3] for r in rows], np.int64),
            "ts": np.array([r[0] for r in rows], np.int64), "seq": np.array([r[1] for r in rows], np.int64)}


_want = {}


def pattern_want(jump_set, base_name, within=W):
    """(rows, batch sizes, reference rows, reference columns) of a two-state
    case from the C oracle, computed once (tests/test_time_edges.py holds the
    C and the Python oracle equal on every one of these)."""
    key = (jump_set, base_name, within)
    if key not in _want:
        w, _, sizes = stream(jump_set, base_name)
        a, b = c_pairs(w, within)
        _want[key] = (w, sizes, pair_rows(w, a, b), pair_columns(w, a, b))
    return _want[key]
