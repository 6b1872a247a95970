"""Sliding-window aggregates on the device (`#window.length(N)` /
`#window.time(T)`, k_winwalk) against the naive window model
(tests/window_model.py), bit-exact, fp64 included: one lane per key performs
the model's expire -> remove -> add sequence in the model's order, so there is
no tolerance to choose."""
import numpy as np
import pytest

import flink_siddhi as fs
from flink_siddhi import workload
from helpers import assert_same_rows, engine_rows, oracle_run, workload_events
from window_model import model_run
import window_kats as K

pytestmark = pytest.mark.gpu

EV2 = ("define stream A (k int, ts long, id int, price double);"
       "define stream B (k int, ts long, id int, price double);")


def part(q):
    return "partition with (k of A) begin " + q + " end;"


_W = {}
_MODEL = {}


def gen(n, keys, rate, jitter=0):
    """The aggregation tests' generator; jitter: ts moved by [-jitter, jitter] (out of order)."""
    key = (n, keys, rate, jitter)
    if key not in _W:
        w = workload.generate(0, n, keys, rate=rate)
        if jitter:
            j = (workload.splitmix64(np.arange(n, dtype=np.uint64)) % np.uint64(2 * jitter + 1)).astype(np.int64)
            w["ts"] = w["ts"] + j - jitter
        _W[key] = w
    return _W[key]


def model(plan, wkey):
    """Reference rows and largest live count, computed once per (plan, input)."""
    if (plan, wkey) not in _MODEL:
        _MODEL[(plan, wkey)] = model_run(plan, workload_events(gen(*wkey)))
    return _MODEL[(plan, wkey)]


def cols(w, s, e):
    return [w["k"][s:e], w["ts"][s:e], w["id"][s:e], w["price"][s:e]]


def run(plan, w, batches=1, outs=("O",), **opts):
    rt = fs.SiddhiAppRuntime(plan, **opts)
    for o in outs:
        rt.add_callback(o)
    n = len(w["ts"])
    cuts = np.linspace(0, n, batches + 1).astype(int)
    for b in range(batches):
        s, e = cuts[b], cuts[b + 1]
        rt.send("A", w["ts"][s:e], cols(w, s, e), streams=w["stream"][s:e])
        rt.flush()
    got = {o: engine_rows(rt.collect(o)) for o in outs}
    rt.shutdown()
    return got


def case(query, n=20000, keys=512, rate=1, jitter=0, batches=1, min_rows=1000, **opts):
    plan = EV2 + query
    wkey = (n, keys, rate, jitter)
    want, live = model(plan, wkey)
    if "#window.time" in query:
        # the ring of a time window holds pending_slots rows per key
        assert live <= opts["pending_slots"], "test shape: model occupancy %d" % live
    got = run(plan, gen(*wkey), batches=batches, **opts)["O"]
    assert_same_rows(got, want.get("O", []), query)
    assert len(got) >= min_rows
    return live


# ---------------------------------------------------------------- KATs ------
S_COLS = (np.int32, np.int64, np.float64)


def run_kat(plan, events, **opts):
    rt = fs.SiddhiAppRuntime(plan, **opts)
    rt.add_callback("O")
    ts = np.array([e[1] for e in events], np.int64)
    c = [np.array([e[2][i] for e in events], S_COLS[i]) for i in range(3)]
    rt.send("S", ts, c)
    rt.flush()
    got = engine_rows(rt.collect("O"))
    rt.shutdown()
    assert [s for _, s, _ in got] == list(range(len(events)))     # arrival numbers
    assert [t for t, _, _ in got] == [e[1] for e in events]       # the current row's ts
    return [d for _, _, d in got]


def test_kat_length():
    assert run_kat(K.KAT_L_PLAN, K.KAT_L_EVENTS) == K.KAT_L_ROWS


def test_kat_time_exact_boundary():
    assert run_kat(K.KAT_T_PLAN, K.KAT_T_EVENTS) == K.KAT_T_ROWS


def test_kat_time_any_order():
    for ts, vs, sums in K.KAT_O_CASES:
        got = run_kat(K.KAT_O_PLAN, K.kat_o_events(ts, vs), ts_order=0)
        assert [d[0] for d in got] == sums, (ts, vs)


def test_kat_fp64_drift():
    got = run_kat(K.KAT_F_PLAN, K.KAT_F_EVENTS)
    assert [d[0] for d in got] == K.KAT_F_SUMS
    assert [d[1] for d in got] == K.KAT_F_AVGS


# ------------------------------------------------------- length windows -----
# Geometry: by default every key of these inputs has a bucket of its own (4
# keys: a key's records of a chunk fill several LDS windows); key_capacity =
# 1024 with buckets_log2 = 2 / 1 puts 128 / 512 keys into one workgroup.
ALL_AGGS = ("select k, sum(id) as si, avg(id) as ai, min(id) as mni, max(id) as mxi, sum(price) as sp, "
            "avg(price) as ap, min(price) as mnp, max(price) as mxp insert into O;")


@pytest.mark.parametrize("n_rows", [1, 2, 5, 16])
def test_length_all_aggregates_4_keys(n_rows):
    # 4 keys: one key's records of a chunk fill several LDS windows
    case(part("from A#window.length(%d) " % n_rows + ALL_AGGS), keys=4)


@pytest.mark.parametrize("n_rows", [1, 2, 5, 16])
def test_length_512_keys(n_rows):
    case(part("from A#window.length(%d) select k, sum(price) as s, min(id) as mn, max(price) as mx, "
              "count() as c insert into O;" % n_rows), keys=512, key_capacity=1024, buckets_log2=2)


@pytest.mark.parametrize("n_rows", [1, 2, 5, 16])
def test_length_ring_crosses_chunks_and_batches(n_rows):
    # most keys see fewer than N rows per 4096-row chunk
    case(part("from A#window.length(%d) select k, sum(id) as s, avg(price) as a, max(id) as mx "
              "group by k insert into O;" % n_rows), n=30000, keys=1024, batches=3, chunk_events=4096,
         key_capacity=1024, buckets_log2=1)


def test_length_255_ring_at_its_cap():
    case(part("from A#window.length(255) select k, sum(price) as s, min(price) as mn, count() as c "
              "insert into O;"), keys=4, key_capacity=1024)


def test_length_256_exceeds_the_ring():
    with pytest.raises(fs.CepCapacityError, match="256"):
        fs.SiddhiAppRuntime(EV2 + part("from A#window.length(256) select k, sum(price) as s insert into O;"))


def test_length_global_window_with_filter():
    case("from A[id < 25]#window.length(5) select sum(price) as s, count() as c, max(id) as m insert into O;",
         keys=64)


def test_length_global_window_whole_tiles_in_one_bucket():
    # no filter: the single bucket holds whole partition tiles (more than an LDS window each)
    case("from A#window.length(3) select sum(id) as s, min(price) as m insert into O;", n=20000, keys=64)


# --------------------------------------------------------- time windows -----
def test_time_window_of_the_current_row_only():
    live = case(part("from A#window.time(1) select k, sum(price) as s, count() as c insert into O;"),
                keys=4, rate=1, pending_slots=4)
    assert live == 1


def test_time_partitioned_rate_1():
    live = case(part("from A#window.time(50) " + ALL_AGGS), keys=4, rate=1, pending_slots=32)
    assert live > 8


def test_time_many_rows_share_a_ts():
    # 8 rows per ms: front.ts + T == e.ts happens constantly
    live = case(part("from A#window.time(5) select k, sum(price) as s, avg(id) as a, min(price) as mn, "
                     "count() as c insert into O;"), keys=4, rate=8, pending_slots=32)
    assert live > 8


def test_time_512_keys_three_batches():
    case(part("from A#window.time(3000) select k, sum(price) as s, max(id) as mx, count() as c insert into O;"),
         n=30000, keys=512, rate=1, batches=3, chunk_events=4096, pending_slots=16, key_capacity=1024,
         buckets_log2=2)


def test_time_out_of_order_front_blocks():
    live = case(part("from A#window.time(20) select k, sum(id) as s, max(price) as mx, count() as c "
                     "insert into O;"), keys=8, rate=1, jitter=15, pending_slots=32, ts_order=0)
    assert live > 4


# ------------------------------------- group by + time outside a partition --
GROUPED_TIME = "from A#window.time(20) select k, sum(price) as s, min(id) as mn, count() as c group by k insert into O;"


def test_grouped_time_window_equals_the_global_window():
    # the model keeps Siddhi's one window for all groups, the engine one per group
    case(GROUPED_TIME, keys=64, rate=1, pending_slots=32, ts_order=1)


def test_grouped_time_window_needs_ordered_input():
    with pytest.raises(fs.UnsupportedPlanException, match="ts_order"):
        fs.SiddhiAppRuntime(EV2 + GROUPED_TIME, ts_order=0)


def test_grouped_time_window_reports_a_descent():
    # ts_order = 1 is a promise: the partition pass checks it for this query
    w = gen(20000, 64, 1, 15)
    rt = fs.SiddhiAppRuntime(EV2 + GROUPED_TIME, pending_slots=32, ts_order=1)
    rt.add_callback("O")
    rt.send("A", w["ts"], cols(w, 0, len(w["ts"])), streams=w["stream"])
    with pytest.raises(ValueError, match="event-time order"):
        rt.flush()
    rt.shutdown()


# ------------------------------------------------ having, options, inputs ---
def test_having_over_aggregate_and_current_attribute():
    case(part("from A[price < 0.6]#window.length(4) select k, id, price, sum(price) as s, count() as c "
              "having s > 1.2 and id > 10 insert into O;"), keys=256, min_rows=300)
    case(part("from A#window.time(40) select k, id, sum(id) as s group by k having s > 60 and id < 30 "
              "insert into O;"), keys=8, pending_slots=32, min_rows=300)


def shim_defaults_case(query, wkey, **extra):
    # the Flink shim's options; arrival numbers are not delivered (omit_seq),
    # rows come in emission order (ordered_output)
    plan = EV2 + query
    want, live = model(plan, wkey)
    rt = fs.SiddhiAppRuntime(plan, sparse_keys=1, ordered_output=1, ts_order=0, omit_seq=1, **extra)
    rt.add_callback("O")
    w = gen(*wkey)
    rt.send("A", w["ts"], cols(w, 0, len(w["ts"])), streams=w["stream"])
    rt.flush()
    out = rt.collect("O")
    rt.shutdown()
    assert len(out.seq) == 0
    got = [(t, d) for t, d in zip(out.ts.tolist(), out.rows())]
    assert got == [(t, d) for t, _, d in want["O"]]
    assert len(got) > 1000
    return live


def test_shim_default_options():
    # (sparse_keys maps partition values of keyed closed-form patterns; the
    # keyed group-by, windowed or not, is refused with it, so these are the
    # global windows)
    shim_defaults_case("from A[id < 30]#window.length(5) select sum(price) as s, count() as c insert into O;",
                       (20000, 64, 1, 0))
    live = shim_defaults_case("from A[id < 30]#window.time(12) select sum(id) as s, max(price) as m insert into O;",
                              (20000, 64, 1, 0), pending_slots=16)
    assert live <= 16
    with pytest.raises(fs.UnsupportedPlanException, match="sparse_keys"):
        fs.SiddhiAppRuntime(EV2 + part("from A#window.length(5) select k, sum(price) as s insert into O;"),
                            sparse_keys=1)


def test_device_resident_input():
    import torch
    query = part("from A#window.length(5) select k, sum(price) as s, avg(price) as a, count() as c insert into O;")
    wkey = (20000, 512, 1, 0)
    want, _ = model(EV2 + query, wkey)
    w = gen(*wkey)
    d = {c: torch.from_numpy(np.ascontiguousarray(w[c])).cuda() for c in ("k", "ts", "id", "price", "stream")}
    rt = fs.SiddhiAppRuntime(EV2 + query)
    rt.add_callback("O")
    rt.send("A", d["ts"], [d["k"], d["ts"], d["id"], d["price"]], streams=d["stream"])
    rt.flush()
    got = engine_rows(rt.collect("O"))
    rt.shutdown()
    assert_same_rows(got, want["O"], "device input")


def test_buffered_input_released_by_watermarks():
    query = part("from A#window.time(30) select k, sum(price) as s, count() as c insert into O;")
    plan = EV2 + query
    n, keys = 20000, 8
    w0 = workload.generate(0, n, keys, rate=1)
    rng = np.random.default_rng(5)
    arrival = np.argsort(np.arange(n) + rng.integers(0, 300, n), kind="stable")
    names = ("k", "ts", "id", "price", "stream")
    w = {c: w0[c][arrival] for c in names}
    o = np.argsort(w["ts"], kind="stable")            # released in (ts, arrival) order
    want, live = model_run(plan, workload_events({c: w[c][o] for c in names}))
    assert live <= 32
    rt = fs.SiddhiAppRuntime(plan, pending_slots=32)
    rt.add_callback("O")
    cuts = np.linspace(0, n, 6).astype(int)
    suffix_min = np.minimum.accumulate(w["ts"][::-1])[::-1]
    for b in range(5):
        s, e = cuts[b], cuts[b + 1]
        rt.process_elements("A", w["ts"][s:e], cols(w, s, e), streams=w["stream"][s:e])
        if e < n:
            rt.process_watermark(int(suffix_min[e]) - 1)
    rt.process_watermark(int(w["ts"].max()))
    rt.flush()
    got = engine_rows(rt.collect("O"))
    rt.shutdown()
    assert_same_rows(got, want["O"], "buffer + watermark")
    assert len(got) > 1000


# ------------------------------------------------------ snapshot / restore --
def snapshot_case(query, wkey, **opts):
    plan = EV2 + query
    want, _ = model(plan, wkey)
    w = gen(*wkey)
    n = len(w["ts"])
    h = n // 2
    rt = fs.SiddhiAppRuntime(plan, **opts)
    rt.add_callback("O")
    rt.send("A", w["ts"][:h], cols(w, 0, h), streams=w["stream"][:h])
    rt.flush()
    first = engine_rows(rt.collect("O"))
    snap = rt.snapshot()
    rt.shutdown()
    rt2 = fs.SiddhiAppRuntime(plan, **opts)
    rt2.add_callback("O")
    rt2.restore(snap)
    rt2.send("A", w["ts"][h:], cols(w, h, n), streams=w["stream"][h:])
    rt2.flush()
    second = engine_rows(rt2.collect("O"))
    rt2.shutdown()
    assert_same_rows(first + second, want["O"], "snapshot/restore " + query)
    return snap


def test_snapshot_restore_length_window():
    q5 = part("from A#window.length(5) select k, sum(price) as s, min(id) as mn, count() as c insert into O;")
    snap = snapshot_case(q5, (20000, 256, 1, 0))
    # the plan hash and the state geometry cover the window parameter
    rt = fs.SiddhiAppRuntime(EV2 + q5.replace("length(5)", "length(6)"))
    with pytest.raises(fs.CepStateError):
        rt.restore(snap)
    rt.shutdown()


def test_snapshot_restore_time_window():
    snapshot_case(part("from A#window.time(60) select k, sum(price) as s, max(id) as mx, count() as c "
                       "insert into O;"), (20000, 8, 1, 0), pending_slots=32)


# ------------------------------------------------------------- overflow -----
def test_time_window_overflow_is_a_capacity_error():
    query = part("from A#window.time(50) select k, sum(price) as s, count() as c insert into O;")
    plan = EV2 + query
    wkey = (20000, 4, 1, 0)
    want, live = model(plan, wkey)
    assert live > 8
    w = gen(*wkey)
    rt = fs.SiddhiAppRuntime(plan, pending_slots=8)
    rt.add_callback("O")
    rt.send("A", w["ts"], cols(w, 0, len(w["ts"])), streams=w["stream"])
    with pytest.raises(fs.CepCapacityError, match="pending_slots"):
        rt.flush()
    rt.shutdown()
    # the process carries on: a fresh runtime with room gives the model's rows
    got = run(plan, w, pending_slots=32)["O"]
    assert_same_rows(got, want["O"], "after overflow")


# -------------------------------------------- next to other queries ---------
def test_window_query_beside_group_by_and_filter():
    win = part("from A#window.length(5) select k, sum(price) as s, count() as c insert into O;")
    rest = ("from A select k, sum(price) as total, count() as n group by k insert into G;"
            "from A[price > 0.9] select k, id, price insert into F;")
    wkey = (20000, 512, 1, 0)
    w = gen(*wkey)
    want_w, _ = model(EV2 + win, wkey)
    want_o = oracle_run(EV2 + rest, workload_events(w))
    got = run(EV2 + win + rest, w, outs=("O", "G", "F"))
    assert_same_rows(got["O"], want_w["O"], "window query")
    assert_same_rows(got["G"], want_o["G"], "plain group-by")
    assert_same_rows(got["F"], want_o["F"], "filter")
    assert len(got["G"]) > 1000 and len(got["F"]) > 500


# ------------------------------------------------------------- sharding -----
@pytest.mark.parametrize("query,opts", [
    (part("from A#window.length(5) select k, sum(price) as s, min(id) as mn, count() as c insert into O;"), {}),
    (part("from A#window.time(400) select k, sum(price) as s, count() as c insert into O;"),
     {"pending_slots": 32}),
])
def test_row_shuffle_two_worlds(query, opts):
    # simulated worlds on one GPU: source slices are routed whole-row
    # (cep_route_rows), owner r runs its segments through cep_send_rows on a
    # runtime owning keys k % world == r; the merged outputs equal the model
    import torch
    world = 2
    plan = EV2 + query
    wkey = (8000, 48, 1, 0)
    want, live = model(plan, wkey)
    assert live <= opts.get("pending_slots", 255)
    w = gen(*wkey)
    n = len(w["ts"])
    sender = fs.SiddhiAppRuntime(plan, key_capacity=64, **opts)
    owners = [fs.SiddhiAppRuntime(plan, key_capacity=64, key_stride=world, key_offset=r, **opts)
              for r in range(world)]
    for o in owners:
        o.add_callback("O")
    m = n // (2 * world)
    for step in range(2):
        segs = [[] for _ in range(world)]
        for src in range(world):
            s = (step * world + src) * m
            e = s + m
            d = {c: torch.from_numpy(np.ascontiguousarray(w[c][s:e])).cuda()
                 for c in ("k", "ts", "id", "price", "stream")}
            rows, counts = sender.route_rows("A", d["ts"], [d["k"], d["ts"], d["id"], d["price"]],
                                             world, seq0=int(s), streams=d["stream"])
            off = np.concatenate([[0], np.cumsum(counts)])
            for r in range(world):
                segs[r].append(rows[off[r]:off[r + 1]].clone())
        for r in range(world):
            recv = torch.cat(segs[r], dim=0)
            owners[r].send_rows(recv, recv.shape[0], 0)
    got = []
    for r in range(world):
        owners[r].flush()
        got += engine_rows(owners[r].collect("O"))
    got.sort(key=lambda t: t[1])
    assert_same_rows(got, want["O"], "row shuffle")
    assert len(got) > 1000
    for rt in owners + [sender]:
        rt.shutdown()
