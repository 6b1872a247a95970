"""The paths of k_cfwalk (csrc/cf_kernels.hip) that a common chunk never
takes, each driven on purpose and compared row for row (and in order per key)
with oracle/cep_oracle.c: a (tile, bucket) segment larger than an LDS window,
a pending list past pending_slots that is carried in the overflow pool, hot-key
diversion switching on and off, received records whose output stores arrival
numbers, and the same oversize stream through the sparse-key, adaptive and
order-tolerant builds.

launch_cf_walk picks the walk instance per launch from what the host knows
(diagnostics, received records with seq, diversion); the common-case instance
holds no code for those.  Every case runs several chunks (chunk_events <=
2^16) and mixes chunks that take a cold path with chunks that do not, so state
written by one is read by the other.  Each case first checks on the CPU, from
the input and the oracle alone, that the stream triggers what it is meant to.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import cep_oracle as CO  # noqa: E402
import flink_siddhi as fs  # noqa: E402
from flink_siddhi import _lib as L  # noqa: E402
from flink_siddhi import workload  # noqa: E402
from test_gpu_geometry import assert_same_per_key  # noqa: E402

KEYS = 4096
RATE = 8                 # events per ms: W = 10 s spans 80 k events
LG = 4                   # 16 key buckets of 256 keys
TILE = 8192              # rows per partition tile (kCfTile)
WINDOW = 2048            # records per walk window (kCfWindow)
F = CO.cond(("price", 0, ">", 0.5))
G = CO.cond(("id", 7, "==", 0))
COLS = ("k", "ts", "id", "price", "stream")


def kept(w):
    """Rows the event-time partition keeps: f-passing A's and g-passing B's."""
    return ((w["stream"] == 0) & (w["price"] > 0.5)) | ((w["stream"] == 1) & (w["id"] % 7 == 0))


def max_segment_per_chunk(w, sizes, chunk, key_of_bucket=None):
    """Largest (tile, bucket) segment of every chunk, in send order (dense keys:
    bucket = key mod 2^LG; tiles count from the chunk's first row)."""
    keep, out, first = kept(w), [], 0
    for n in sizes:
        for c0 in range(first, first + n, chunk):
            c1, big = min(c0 + chunk, first + n), 0
            for t0 in range(c0, c1, TILE):
                rows = slice(t0, min(t0 + TILE, c1))
                b = w["k"][rows][keep[rows]] & ((1 << LG) - 1)
                big = max(big, int(np.bincount(b, minlength=1 << LG).max()))
            out.append(big)
        first += n
    return out


def run(w, sizes, chunk, plan=workload.PATTERN_PLAN, key_value=None, snapshot_after=(), **opts):
    """Device batches through the engine -> (rows as numpy, stats, stats after each batch)."""
    import torch
    opts.setdefault("key_capacity", KEYS)
    opts.setdefault("buckets_log2", LG)
    mk = lambda: fs.SiddhiAppRuntime(plan, chunk_events=chunk, ordered_output=0, **opts)  # noqa: E731
    rt = mk()
    parts, mids, first = [], [], 0
    for i, n in enumerate(sizes):
        t = {c: torch.from_numpy(np.ascontiguousarray(w[c][first:first + n])).cuda() for c in COLS}
        k = t["k"] if key_value is None else key_value(t["k"])
        rt.send("A", t["ts"], [k, t["ts"], t["id"], t["price"]], streams=t["stream"])
        parts.append(rt.output_tensors("O", copy=True))
        rt.flush()
        mids.append(rt.stats())
        if i in snapshot_after:
            snap = rt.snapshot()
            rt.shutdown()
            rt = mk()
            rt.restore(snap)
        first += n
    torch.cuda.synchronize()
    st = rt.stats()
    rt.shutdown()
    cat = lambda i: torch.cat([p[2][i] for p in parts]).cpu().numpy()  # noqa: E731
    out = {"k": cat(0), "p1": cat(1), "p2": cat(2), "t": cat(3),
           "ts": torch.cat([p[0] for p in parts]).cpu().numpy(),
           "seq": torch.cat([p[1] for p in parts]).cpu().numpy()}
    return out, st, mids


def oracle_rows(w, keys=KEYS, g=G, within=10000):
    po = CO.PatternOracle(keys, F, g, every=True, within=within)
    a, b, m = po.run(w)
    assert m == len(a)
    return {"k": w["k"][a], "p1": w["price"][a], "p2": w["price"][b], "t": w["ts"][b],
            "ts": w["ts"][b], "seq": b}, a, b


# ---- the streams, generated once -------------------------------------------
CHUNK = 1 << 15          # 4 tiles
BIG_KEY = 1234


def oversize_stream():
    """Five chunks of uniform traffic; in chunk 2, tile 1, every other row
    belongs to one key and is kept (A's pass f, B's pass g): 4096 kept records
    of one key in one tile, two windows' worth."""
    w = CO.generate(0, 5 * CHUNK, KEYS, rate=RATE, threads=8)
    w = {c: w[c].copy() for c in COLS}
    r = np.arange(2 * CHUNK + TILE, 2 * CHUNK + 2 * TILE, 2)
    w["k"][r] = BIG_KEY
    w["price"][r] = 0.5 + w["price"][r] / 2 + 1e-9
    w["id"][r] -= w["id"][r] % 7
    return w


_cache = {}


def cached(name, make):
    if name not in _cache:
        _cache[name] = make()
    return _cache[name]


def oversize_case():
    def make():
        w = oversize_stream()
        segs = max_segment_per_chunk(w, [5 * CHUNK], CHUNK)
        # the chunk with the oversize segment sits between chunks with none
        assert segs[2] > 2 * WINDOW - 1 and all(s <= WINDOW // 2 for i, s in enumerate(segs) if i != 2), segs
        in_tile = slice(2 * CHUNK + TILE, 2 * CHUNK + 2 * TILE)
        assert int(((w["k"][in_tile] == BIG_KEY) & kept(w)[in_tile]).sum()) > WINDOW
        return w, oracle_rows(w)[0]
    return cached("oversize", make)


def test_common_case():
    # 4096 keys, 2^18 events in three batches: no segment near a window, no
    # key near the hot threshold, nothing diverted
    n, chunk = 1 << 18, 1 << 16
    sizes = [chunk + 777, 2 * chunk - 777, chunk]
    w = CO.generate(0, n, KEYS, rate=RATE, threads=8)
    assert max(max_segment_per_chunk(w, sizes, chunk)) <= WINDOW // 2
    want, _, _ = oracle_rows(w)
    got, st, _ = run(w, sizes, chunk, ts_order=1)
    assert st.kernel_launches[L.K_CF_WALK] >= 5 and st.kernel_launches[L.K_WALK] == 0
    assert st.kernel_launches[L.K_HOT] == 0 and st.hot_keys == 0
    assert len(want["k"]) > 10_000
    assert_same_per_key(got, want)


def test_oversize_segment_between_common_chunks():
    w, want = oversize_case()
    got, st, _ = run(w, [5 * CHUNK], CHUNK, ts_order=1)
    assert st.kernel_launches[L.K_CF_WALK] == 5 and st.kernel_launches[L.K_HOT] == 0
    assert_same_per_key(got, want)
    assert int((want["k"] == BIG_KEY).sum()) > 1000


def test_overflow_list_carried_across_a_chunk_and_a_snapshot():
    # pending_slots 4; key 77 collects 40 live partials in chunk 0, has no
    # record in chunk 1 (the run is carried: read pool -> write pool), the
    # state is snapshotted and restored, and a B completes all 40 in chunk 2
    key, other = 77, 78
    w = CO.generate(0, 4 * CHUNK, KEYS, rate=RATE, threads=8)
    w = {c: w[c].copy() for c in COLS}
    w["k"][w["k"] == key] = other
    a_rows = 1000 + 50 * np.arange(40)
    b_row = 2 * CHUNK + 333
    w["k"][a_rows], w["stream"][a_rows], w["price"][a_rows] = key, 0, 0.9
    w["k"][b_row], w["stream"][b_row], w["id"][b_row] = key, 1, 7
    assert a_rows.max() < CHUNK and not (w["k"][CHUNK:2 * CHUNK] == key).any()
    assert w["ts"][b_row] - w["ts"][a_rows[0]] <= 10000
    want, a, b = oracle_rows(w)
    assert sorted(a[b == b_row]) == sorted(a_rows)    # the list held 40 live partials (> 4 slots)
    sizes = [2 * CHUNK, 2 * CHUNK]
    got, st, _ = run(w, sizes, CHUNK, ts_order=1, pending_slots=4, snapshot_after=(0,))
    assert st.kernel_launches[L.K_CF_WALK] == 2 and st.kernel_launches[L.K_WALK] == 0   # (after the restore)
    assert_same_per_key(got, want)


def test_hot_key_diversion_on_and_off():
    # Zipf batches (the busiest keys pass 256 records per 2^16-event chunk and
    # are diverted from the next batch on), then uniform ones (they go cold and
    # their slots are freed): keys move walk -> hot scans -> walk
    chunk, nb = 1 << 16, 1 << 17
    z = workload.zipf_map(KEYS, seed=7)
    w = CO.generate(0, 6 * nb, KEYS, rate=RATE, threads=8)
    w = {c: w[c].copy() for c in COLS}
    w["k"][:3 * nb] = z[w["k"][:3 * nb]]
    keep = kept(w)
    per_chunk = [int(np.bincount(w["k"][c:c + chunk][keep[c:c + chunk]], minlength=KEYS).max())
                 for c in range(0, 6 * nb, chunk)]
    assert min(per_chunk[:6]) > 4 * 256 and max(per_chunk[6:]) < 256 // 4, per_chunk
    want, _, _ = oracle_rows(w)
    got, st, mids = run(w, [nb] * 6, chunk, ts_order=1)
    assert st.kernel_launches[L.K_HOT] > 0 and st.kernel_launches[L.K_CF_WALK] == 12
    assert mids[2].hot_keys > 0 and st.hot_keys == 0, (mids[2].hot_keys, st.hot_keys)
    assert_same_per_key(got, want)


def test_received_records_store_arrival_numbers():
    # two simulated shuffle ranks: each owner walks received records and its
    # output stores their global arrival numbers (omit_seq 0: the in_seq lookup)
    import torch
    world, n_per, steps = 2, 1 << 16, 3
    rts = [fs.SiddhiAppRuntime(workload.PATTERN_PLAN, ts_order=1, key_stride=world, key_offset=r,
                               chunk_events=TILE, key_capacity=KEYS // world, buckets_log2=LG,
                               ordered_output=0) for r in range(world)]
    assert all(rt.options.omit_seq == 0 for rt in rts)
    parts = []
    for s in range(steps):
        segs = [[] for _ in range(world)]
        for src in range(world):
            first = (s * world + src) * n_per
            d = workload.generate_device(first, n_per, KEYS, rate=RATE)
            recs, counts = rts[src].route("A", d["ts"], [d["k"], d["ts"], d["id"], d["price"]], world,
                                          seq0=first, streams=d["stream"])
            off = np.concatenate([[0], np.cumsum(counts)])
            for r in range(world):
                segs[r].append(recs[off[r]:off[r + 1]].clone())
        for r in range(world):
            recv = torch.cat(segs[r], dim=0)
            assert recv.shape[0] > 2 * TILE    # three one-tile chunks per owner and step
            rts[r].send_records(recv, recv.shape[0], n_per)
            parts.append(rts[r].output_tensors("O", copy=True))
            rts[r].flush()
    torch.cuda.synchronize()
    walks = sum(rt.stats().kernel_launches[L.K_CF_WALK] for rt in rts)
    for rt in rts:
        rt.shutdown()
    got = {c: torch.cat([p[2][i] for p in parts]).cpu().numpy() for i, c in enumerate(("k", "p1", "p2", "t"))}
    got["ts"] = torch.cat([p[0] for p in parts]).cpu().numpy()
    got["seq"] = torch.cat([p[1] for p in parts]).cpu().numpy()
    w = CO.generate(0, steps * world * n_per, KEYS, rate=RATE, threads=8)
    want, _, _ = oracle_rows(w)
    assert walks >= world * steps and len(want["k"]) > 10_000
    assert_same_per_key(got, want)    # seq = the completing record's global arrival number


@pytest.mark.parametrize("build", ["sparse", "adaptive", "tolerant"])
def test_oversize_segment_other_builds(build):
    w, want = oversize_case()
    if build == "sparse":
        # 64-bit partition values through the device key map (event-time build)
        base, mul = 1 << 40, 7919
        got, st, _ = run(w, [5 * CHUNK], CHUNK, plan=workload.PATTERN_PLAN.replace("k int", "k long"),
                         key_value=lambda k: k.long() * mul + base, ts_order=1, sparse_keys=1)
        got["k"] = ((got["k"].astype(np.int64) - base) // mul).astype(np.int32)
    elif build == "adaptive":
        # ts_order 0, every chunk in order: the adaptive build walks them
        assert (np.diff(w["ts"]) >= 0).all()
        got, st, _ = run(w, [5 * CHUNK], CHUNK, ts_order=0)
        assert st.kernel_launches[L.K_OTHER] >= 2 * st.kernel_launches[L.K_CF_WALK] > 0
    else:
        # ts_order 0 and a block of late rows in every chunk: each chunk's
        # adaptive partition finds the descent and the order-tolerant build takes it
        w = {c: w[c].copy() for c in COLS}
        for c0 in range(0, 5 * CHUNK, CHUNK):
            w["ts"][c0 + 5000:c0 + 5050] -= 3000
            assert (np.diff(w["ts"][c0:c0 + CHUNK]) < 0).any()
        want = oracle_rows(w)[0]
        got, st, _ = run(w, [5 * CHUNK], CHUNK, ts_order=0)
    assert st.kernel_launches[L.K_WALK] == 0 and st.kernel_launches[L.K_HOT] == 0
    assert_same_per_key(got, want)
