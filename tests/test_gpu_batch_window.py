"""Tumbling-window aggregates on the device (`#window.lengthBatch(N)` /
`#window.externalTimeBatch(c, T)`, k_batchwalk) against the naive batch model
(tests/batch_window_model.py), bit-exact, fp64 included: one lane per key
folds its rows in the model's order, so there is no tolerance to choose."""
import numpy as np
import pytest

import flink_siddhi as fs
from flink_siddhi import _lib as L
from flink_siddhi import workload
from helpers import assert_same_rows, engine_rows, oracle_run, workload_events
import batch_window_model as M

pytestmark = pytest.mark.gpu

EV2 = ("define stream A (k int, ts long, id int, price double);"
       "define stream B (k int, ts long, id int, price double);")
NAMES = ("k", "ts", "id", "price", "stream")


def part(q, of="k of A"):
    return "partition with (" + of + ") begin " + q + " end;"


_W = {}
_MODEL = {}


def gen(n, keys, rate, jitter=0):
    """The aggregation tests' generator; jitter: the ts column moved by [-jitter, jitter]."""
    key = (n, keys, rate, jitter)
    if key not in _W:
        w = workload.generate(0, n, keys, rate=rate)
        if jitter:
            j = (workload.splitmix64(np.arange(n, dtype=np.uint64)) % np.uint64(2 * jitter + 1)).astype(np.int64)
            w["ts"] = w["ts"] + j - jitter
        _W[key] = w
    return _W[key]


def model(plan, wkey):
    """Reference rows and batch statistics, computed once per (plan, input)."""
    if (plan, wkey) not in _MODEL:
        _MODEL[(plan, wkey)] = M.model_run(plan, workload_events(gen(*wkey)))
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
    kl = list(rt.stats().kernel_launches)
    rt.shutdown()
    return got, kl


def check_model(want, st, having):
    """What every test asserts about its own input."""
    assert len(want) >= 1000, len(want)
    if having:
        assert st["silent"] > 0 and st["early"] > 0, st


def case(query, n=20000, keys=512, rate=1, jitter=0, batches=1, **opts):
    plan = EV2 + query
    wkey = (n, keys, rate, jitter)
    want, st = model(plan, wkey)
    check_model(want.get("O", []), st, " having " in query)
    got, kl = run(plan, gen(*wkey), batches=batches, **opts)
    assert kl[L.K_AGG] > 0 and kl[L.K_WALK] == 0 and kl[L.K_MQ_WALK] == 0, kl
    assert_same_rows(got["O"], want["O"], query)


# ---------------------------------------------------------------- KATs ------
KAT_DTYPES = (np.int32, np.int64, np.int64, np.float64)


def run_kat(plan, events):
    rt = fs.SiddhiAppRuntime(plan)
    rt.add_callback("O")
    ts = np.array([e[1] for e in events], np.int64)
    c = [np.array([e[2][i] for e in events], KAT_DTYPES[i]) for i in range(4)]
    rt.send("S", ts, c)
    rt.flush()
    got = engine_rows(rt.collect("O"))
    rt.shutdown()
    return got


def test_kat1_length_batch():
    assert run_kat(M.KAT1_PLAN, M.KAT1_EVENTS) == M.KAT1_ROWS


def test_kat2_having_picks_an_earlier_row_or_none():
    assert run_kat(M.KAT2_PLAN, M.KAT2_EVENTS) == M.KAT2_ROWS


def test_kat3_external_time_batch_is_positional():
    assert run_kat(M.KAT3_PLAN, M.KAT3_EVENTS) == M.KAT3_ROWS


def test_kat4_fp64_left_fold_from_plus_zero():
    assert M.bits(run_kat(M.KAT4_PLAN, M.KAT4_EVENTS)) == M.bits(M.KAT4_ROWS)
    assert M.bits(run_kat(M.KAT4Z_PLAN, M.KAT4Z_EVENTS)) == M.bits(M.KAT4Z_ROWS)


# -------------------------------------------------------- lengthBatch -------
ALL_AGGS = ("select k, sum(id) as si, avg(id) as ai, min(id) as mni, max(id) as mxi, sum(price) as sp, "
            "avg(price) as ap, min(price) as mnp, max(price) as mxp insert into O;")
LEN_PLAIN = "select k, id, sum(price) as s, min(id) as mn, count() as c insert into O;"
LEN_HAVING = "select k, id, price * 2.0 as p2, sum(id) as s having s < 60 and id > 5 insert into O;"
TIME_HAVING = "select k, id, sum(price) as s, count() as c having s < 1.6 and id > 5 insert into O;"


@pytest.mark.parametrize("n_rows", [1, 3, 7])
def test_length_batch(n_rows):
    case(part("from A#window.lengthBatch(%d) " % n_rows + LEN_PLAIN), key_capacity=1024, buckets_log2=2)


@pytest.mark.parametrize("col", ["price", "id"])
def test_length_batch_all_five_aggregates(col):
    # sum, count, avg, min, max over a double and over an int column
    case(part("from A#window.lengthBatch(3) select k, sum(%s) as s, count() as c, avg(%s) as a, min(%s) as mn, "
              "max(%s) as mx insert into O;" % (col, col, col, col)))


def test_length_batch_eight_aggregates_double_and_int():
    # the most a query may hold: sum, avg, min, max of both columns (count() is in the case above)
    case(part("from A#window.lengthBatch(3) " + ALL_AGGS))


def test_length_batch_side_filter():
    case(part("from A[id < 40 and price > 0.1]#window.lengthBatch(3) select k, sum(price) as s, max(id) as mx, "
              "count() as c group by k insert into O;"))


def test_length_batch_having_and_computed_item():
    case(part("from A#window.lengthBatch(3) " + LEN_HAVING), key_capacity=1024, buckets_log2=1)


def test_length_batch_plain_form():
    case(part("from A#window.lengthBatch(3) select k, sum(price) as s, count() as c insert into O;"))


# -------------------------------------------------- externalTimeBatch -------
def test_time_batch_in_order_column():
    case(part("from A#window.externalTimeBatch(ts, 4000) select k, id, sum(price) as s, min(id) as mn, count() as c "
              "insert into O;"))


def test_time_batch_jittered_column():
    # rows behind `end` join the open batch
    case(part("from A#window.externalTimeBatch(ts, 4000) select k, ts, id, sum(price) as s, count() as c "
              "insert into O;"), jitter=3000, ts_order=0)


def test_time_batch_having():
    case(part("from A#window.externalTimeBatch(ts, 4000) " + TIME_HAVING), jitter=3000, ts_order=0)


# ----------------------------------------------------------- geometry -------
FOUR_KEYS = [
    "from A#window.lengthBatch(3) " + ALL_AGGS,
    "from A#window.lengthBatch(7) " + LEN_HAVING.replace("id > 5", "id > 25"),
    "from A#window.externalTimeBatch(ts, 8) select k, id, sum(price) as s, count() as c insert into O;",
    "from A#window.externalTimeBatch(ts, 8) " + TIME_HAVING,
]
LDS_WINDOW = 2048     # records per LDS window of the walk (kWinWindow)


# 4 keys, the default options, one send: every key has a bucket of its own,
# the whole send is one chunk, and a key's records of it fill more than one
# LDS window.  So batches close mid-window and across the windows of one
# launch, and a candidate that one window committed to state is emitted by the
# next.
@pytest.mark.parametrize("query", FOUR_KEYS)
def test_four_keys_many_lds_windows(query):
    w = gen(20000, 4, 1)
    kept = np.bincount(w["k"][w["stream"] == 0], minlength=4)      # no side filter: every A row is kept
    assert kept.min() > LDS_WINDOW, kept                           # the premise: several windows per key
    assert len(w["ts"]) <= 4 << 20                                 # one default chunk
    case(part(query), keys=4)


# 4096-event chunks and several sends: a candidate from an earlier chunk or
# send is emitted by a later one (each launch holds one LDS window per key).
@pytest.mark.parametrize("batches", [3, 7])
@pytest.mark.parametrize("query", FOUR_KEYS)
def test_four_keys_4096_event_chunks(query, batches):
    case(part(query), keys=4, batches=batches, chunk_events=4096)


@pytest.mark.parametrize("batches", [3, 7])
@pytest.mark.parametrize("query", [
    "from A#window.lengthBatch(7) " + LEN_PLAIN,
    "from A#window.lengthBatch(3) " + LEN_HAVING,
    "from A#window.externalTimeBatch(ts, 4000) " + TIME_HAVING,
])
def test_batches_straddle_sends(query, batches):
    case(part(query), batches=batches, chunk_events=4096, key_capacity=1024, buckets_log2=2)


# ------------------------------------------------- options and paths --------
JIT = (20000, 512, 1, 3000)
TIME_JIT = part("from A#window.externalTimeBatch(ts, 4000) select k, ts, id, sum(price) as s, count() as c "
                "insert into O;")


def test_ordered_output_orders_by_arrival_number_only():
    # the emitted row's ts is its own, not the trigger's: rows in arrival order are not in ts order
    plan = EV2 + TIME_JIT + "from A[price > 0.9] select k, id, price insert into F;"
    want, st = model(EV2 + TIME_JIT, JIT)
    check_model(want["O"], st, False)
    assert any(a[0] > b[0] for a, b in zip(want["O"], want["O"][1:]))
    w = gen(*JIT)
    want_f = oracle_run(EV2 + "from A[price > 0.9] select k, id, price insert into F;", workload_events(w))["F"]
    got, _ = run(plan, w, outs=("O", "F"), ordered_output=1, ts_order=0)
    assert_same_rows(got["O"], want["O"], "ordered output")
    assert_same_rows(got["F"], want_f, "filter beside it")


def test_omit_seq():
    want, _ = model(EV2 + TIME_JIT, JIT)
    w = gen(*JIT)
    rt = fs.SiddhiAppRuntime(EV2 + TIME_JIT, ordered_output=1, ts_order=0, omit_seq=1)
    rt.add_callback("O")
    rt.send("A", w["ts"], cols(w, 0, len(w["ts"])), streams=w["stream"])
    rt.flush()
    out = rt.collect("O")
    rt.shutdown()
    assert len(out.seq) == 0
    assert [(t, d) for t, d in zip(out.ts.tolist(), out.rows())] == [(t, d) for t, _, d in want["O"]]


def test_device_resident_input():
    import torch
    query = part("from A#window.lengthBatch(3) " + LEN_HAVING)
    wkey = (20000, 512, 1, 0)
    want, st = model(EV2 + query, wkey)
    check_model(want["O"], st, True)
    w = gen(*wkey)
    d = {c: torch.from_numpy(np.ascontiguousarray(w[c])).cuda() for c in NAMES}
    rt = fs.SiddhiAppRuntime(EV2 + query)
    rt.add_callback("O")
    rt.send("A", d["ts"], [d["k"], d["ts"], d["id"], d["price"]], streams=d["stream"])
    rt.flush()
    got = engine_rows(rt.collect("O"))
    rt.shutdown()
    assert_same_rows(got, want["O"], "device input")


def test_buffered_input_released_by_watermarks():
    plan = EV2 + part("from A#window.externalTimeBatch(ts, 40) select k, id, sum(price) as s, count() as c "
                      "insert into O;")
    n, keys = 20000, 8
    w0 = workload.generate(0, n, keys, rate=1)
    rng = np.random.default_rng(5)
    arrival = np.argsort(np.arange(n) + rng.integers(0, 300, n), kind="stable")
    w = {c: w0[c][arrival] for c in NAMES}
    o = np.argsort(w["ts"], kind="stable")            # released in (ts, arrival) order
    want, st = M.model_run(plan, workload_events({c: w[c][o] for c in NAMES}))
    check_model(want["O"], st, False)
    rt = fs.SiddhiAppRuntime(plan)
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


@pytest.mark.parametrize("query", [
    part("from A#window.lengthBatch(3) " + LEN_HAVING),
    part("from A#window.externalTimeBatch(ts, 300) select k, id, sum(price) as s, count() as c insert into O;"),
])
def test_row_shuffle_two_worlds(query):
    # simulated worlds on one GPU: source slices are routed whole-row
    # (cep_route_rows), owner r runs its segments through cep_send_rows on a
    # runtime owning keys k % world == r; the merged outputs equal the model
    import torch
    world = 2
    plan = EV2 + query
    wkey = (8000, 48, 1, 0)
    want, st = model(plan, wkey)
    check_model(want["O"], st, " having " in query)
    w = gen(*wkey)
    n = len(w["ts"])
    sender = fs.SiddhiAppRuntime(plan, key_capacity=64)
    owners = [fs.SiddhiAppRuntime(plan, key_capacity=64, key_stride=world, key_offset=r) for r in range(world)]
    for o in owners:
        o.add_callback("O")
    m = n // (2 * world)
    for step in range(2):
        segs = [[] for _ in range(world)]
        for src in range(world):
            s = (step * world + src) * m
            e = s + m
            d = {c: torch.from_numpy(np.ascontiguousarray(w[c][s:e])).cuda() for c in NAMES}
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
    for rt in owners + [sender]:
        rt.shutdown()
    assert_same_rows(got, want["O"], "row shuffle")


def test_batch_window_reads_a_derived_stream():
    # the producer is a filter with plain copies: the window over M equals the
    # window over A with the producer's filter in front
    prod = "from A[price > 0.1] select k, ts, id, price insert into M;"
    q = "from %s#window.lengthBatch(3) select k, id, sum(price) as s, count() as c insert into O;"
    wkey = (20000, 512, 1, 0)
    want, st = model(EV2 + part(q % "A[price > 0.1]"), wkey)
    check_model(want["O"], st, False)
    got, kl = run(EV2 + prod + part(q % "M", of="k of M"), gen(*wkey))
    assert kl[L.K_AGG] > 0 and kl[L.K_OTHER] > 0, kl      # k_batchwalk behind k_derive
    assert_same_rows(got["O"], want["O"], "derived stream")


def test_batch_window_beside_a_multi_query_group():
    win = part("from A#window.lengthBatch(3) " + LEN_HAVING)
    rest = ("from A select k, sum(price) as total, count() as n group by k insert into G1;"
            "from A[id > 10] select k, max(price) as top, count() as n group by k insert into G2;")
    wkey = (20000, 512, 1, 0)
    w = gen(*wkey)
    want_w, st = model(EV2 + win, wkey)
    check_model(want_w["O"], st, True)
    want_o = oracle_run(EV2 + rest, workload_events(w))
    got, kl = run(EV2 + win + rest, w, outs=("O", "G1", "G2"))
    assert kl[L.K_MQ_WALK] > 0 and kl[L.K_AGG] > 0, kl     # the group is formed, the batch query walks alone
    assert_same_rows(got["O"], want_w["O"], "batch window")
    assert_same_rows(got["G1"], want_o["G1"], "group-by 1")
    assert_same_rows(got["G2"], want_o["G2"], "group-by 2")


# ------------------------------------------------------ snapshot / restore --
def snapshot_case(query, wkey, **opts):
    plan = EV2 + query
    want, st = model(plan, wkey)
    check_model(want["O"], st, " having " in query)
    w = gen(*wkey)
    n = len(w["ts"])
    h = n // 2
    # the snapshot is taken while batches are half full
    half = M.BatchWindowModel(plan)
    for sid, ts, row in workload_events({c: w[c][:h] for c in NAMES}):
        half.send(sid, ts, row)
    assert sum(1 for inst in half.instances[0].values() if inst.rows) > 100
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


def test_snapshot_restore_length_batch():
    q3 = part("from A#window.lengthBatch(3) " + LEN_HAVING)
    snap = snapshot_case(q3, (20000, 512, 1, 0))
    # the plan hash covers the window kind and its parameter
    for other in (q3.replace("lengthBatch(3)", "lengthBatch(4)"), q3.replace("lengthBatch(3)", "length(3)")):
        rt = fs.SiddhiAppRuntime(EV2 + other)
        with pytest.raises(fs.CepStateError):
            rt.restore(snap)
        rt.shutdown()


def test_snapshot_restore_time_batch():
    snapshot_case(part("from A#window.externalTimeBatch(ts, 4000) " + TIME_HAVING), JIT, ts_order=0)
