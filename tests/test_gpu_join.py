"""Windowed stream joins on the device (join_kernels.hip) against the naive
join model (tests/join_model.py): the same rows, bit for bit, in the same
order.  Every value is copied or computed by one interpreter program per row
pair, so there is no tolerance to choose."""
import json
from pathlib import Path

import numpy as np
import pytest

import flink_siddhi as fs
from flink_siddhi import _lib as L
from flink_siddhi import workload
from helpers import assert_same_rows, engine_rows, workload_events
from join_model import model_run
import join_kats as K

pytestmark = pytest.mark.gpu

FIXTURE = json.loads((Path(__file__).parent / "golden" / "join_itcase.json").read_text())
EV2 = ("define stream A (k int, ts long, id int, price double);"
       "define stream B (k int, ts long, id int, price double);")
TILE = 256          # kJoinTile: window entries staged in LDS at a time
WG = 256            # kJoinThreads: probes per workgroup
TAIL_CAP = 65536    # kJoinTailCap

_W = {}
_MODEL = {}


def gen(n, keys, rate=1, jitter=0):
    key = (n, keys, rate, jitter)
    if key not in _W:
        w = workload.generate(0, n, keys, rate=rate)
        if jitter:
            j = (workload.splitmix64(np.arange(n, dtype=np.uint64)) % np.uint64(2 * jitter + 1)).astype(np.int64)
            w["ts"] = w["ts"] + j - jitter
        _W[key] = w
    return _W[key]


def model(plan, wkey):
    """Reference rows and the model (live counts, rows per triggering side), once per (plan, input)."""
    if (plan, wkey) not in _MODEL:
        _MODEL[(plan, wkey)] = model_run(plan, workload_events(gen(*wkey)))
    return _MODEL[(plan, wkey)]


def cols(w, s, e):
    return [w["k"][s:e], w["ts"][s:e], w["id"][s:e], w["price"][s:e]]


def run(plan, w, batches=1, outs=("O",), cuts=None, stats=None, **opts):
    rt = fs.SiddhiAppRuntime(plan, **opts)
    for o in outs:
        rt.add_callback(o)
    n = len(w["ts"])
    cuts = np.linspace(0, n, batches + 1).astype(int) if cuts is None else cuts
    for s, e in zip(cuts[:-1], cuts[1:]):
        rt.send("A", w["ts"][s:e], cols(w, s, e), streams=w["stream"][s:e])
        rt.flush()
    got = {o: engine_rows(rt.collect(o)) for o in outs}
    if stats is not None:
        stats.append(rt.stats())
    rt.shutdown()
    return got


def case(query, wkey=(20000, 8), min_rows=1000, min_side=100, vm=None, **opts):
    plan = EV2 + query
    want, m = model(plan, wkey)
    want = want.get("O", [])
    # the shape exercises both probing sides (checked on the CPU, from the model alone)
    assert len(want) >= min_rows and min(m.joins[0].triggered) >= min_side, (len(want), m.joins[0].triggered)
    st = []
    got = run(plan, gen(*wkey), stats=st, **opts)["O"]
    assert_same_rows(got, want, query)
    assert st[0].kernel_launches[L.K_JOIN] > 0
    if vm is not None:
        assert (st[0].kernel_launches[L.K_JOIN_VM] > 0) == vm
    return m


def custom(stream, ts, k, idv=None, price=None):
    """Hand-made input in the generator's layout."""
    n = len(stream)
    return {"stream": np.asarray(stream, np.uint8), "ts": np.asarray(ts, np.int64), "k": np.asarray(k, np.int32),
            "id": np.zeros(n, np.int32) if idv is None else np.asarray(idv, np.int32),
            "price": np.arange(n, dtype=np.float64) / 8 if price is None else np.asarray(price, np.float64)}


def custom_case(query, w, cuts, **opts):
    plan = EV2 + query
    want, m = model_run(plan, workload_events(w))
    got = run(plan, w, cuts=cuts, **opts)["O"]
    assert_same_rows(got, want.get("O", []), query)
    return got, m


# ------------------------------------------------------- small and fixture --
def run_kat(plan, events, **opts):
    rt = fs.SiddhiAppRuntime(plan, **opts)
    rt.add_callback("O")
    h = {"A": rt.input_handle("A"), "B": rt.input_handle("B")}
    ts = np.array([e[1] for e in events], np.int64)
    c = [np.array([e[2][i] for e in events], np.int32) for i in range(2)]
    rt.send("A", ts, c, streams=np.array([h[e[0]] for e in events], np.uint8))
    rt.flush()
    got = engine_rows(rt.collect("O"))
    rt.shutdown()
    return got


@pytest.mark.parametrize("name", sorted(K.KATS))
def test_kats(name):
    # "time_boundary": r.ts + T == e.ts has left, r.ts + T == e.ts + 1 stays
    plan, events, rows = K.KATS[name]
    assert run_kat(plan, events, ts_order=1) == rows


def test_kat_row_never_joins_its_own_side():
    plan, events, _ = K.KATS["length"]
    assert run_kat(plan, [e for e in events if e[0] == "A"]) == []
    assert run_kat(plan, [e for e in events if e[0] == "B"]) == []


def run_fixture(plan, order, name2="test_event"):
    rt = fs.SiddhiAppRuntime(plan, ts_order=1)
    rt.add_callback("JoinStream")
    ev = FIXTURE[order]
    h = {s: rt.input_handle(s) for s in ("inputStream1", "inputStream2")}
    names = {"inputStream1": rt.intern("test_event"), "inputStream2": rt.intern(name2)}
    ts = np.array([e[1] for e in ev], np.int64)
    c = [np.array([e[2][0] for e in ev], np.int32), np.array([names[e[0]] for e in ev], np.int32),
         np.array([e[2][2] for e in ev], np.float64), np.array([e[2][3] for e in ev], np.int64)]
    rt.send("inputStream1", ts, c, streams=np.array([h[e[0]] for e in ev], np.uint8))
    rt.flush()
    out = rt.collect("JoinStream")
    rows = [[t, rt.lookup(n), p1, p2] for t, n, p1, p2 in out.rows()]
    rt.shutdown()
    return rows, out


@pytest.mark.parametrize("order", ["events_stream1_first", "events_stream2_first"])
def test_itcase_fixture(order):
    # SiddhiCEPITCase.java:306-327: 5 rows, one per id
    rows, out = run_fixture(FIXTURE["plan"], order)
    assert rows == FIXTURE["expected"]
    assert out.ts.tolist() == [e[0] for e in FIXTURE["expected"]]
    assert out.seq.tolist() == [1, 3, 5, 7, 9]


@pytest.mark.parametrize("order", ["events_stream1_first", "events_stream2_first"])
def test_itcase_string_column_compares_through_the_dictionary(order):
    plan = FIXTURE["plan"].replace("on s1.id == s2.id", "on s1.id == s2.id and s1.name == s2.name")
    assert plan != FIXTURE["plan"]
    assert run_fixture(plan, order)[0] == FIXTURE["expected"]
    assert run_fixture(plan, order, name2="another_event")[0] == []
    ne = plan.replace("s1.name == s2.name", "s1.name != s2.name")
    assert run_fixture(ne, order, name2="another_event")[0] == FIXTURE["expected"]


# ------------------------------------------- model parity on generator rows --
# 20,000 rows, 8 keys (a.k == b.k hits one pair in 8), one row per ms.  T = 400
# ms holds about 200 live rows per side (asserted from the model).
LT = ("from A#window.length(5) as a join B#window.time(400) as b on a.k == b.k "
      "select a.id as x, b.price as p, a.price - b.price as d insert into O;")
LL = ("from A#window.length(100) as a join B#window.length(3) as b on a.id + b.id > 3 and a.k == b.k "
      "select a.id as x, b.price as p, b.ts as t insert into O;")
TT = ("from A#window.time(400) as a join B#window.time(30) as b on a.k == b.k and a.price < b.price "
      "select a.id as x, b.ts as t, a.price as p insert into O;")
LAYOUTS = [dict(batches=1), dict(batches=3), dict(batches=1, chunk_events=4096), dict(batches=3, chunk_events=4096)]
LAYOUT_IDS = ["one_batch", "three_batches", "chunks_4096", "three_batches_chunks_4096"]


@pytest.mark.parametrize("layout", LAYOUTS, ids=LAYOUT_IDS)
def test_length_and_time_direct_term_computed_item(layout):
    m = case(LT, vm=False, ts_order=1, **layout)
    assert 150 <= m.joins[0].sides[1].max_live <= 400


@pytest.mark.parametrize("layout", LAYOUTS, ids=LAYOUT_IDS)
def test_length_and_length_interpreter(layout):
    case(LL, vm=True, **layout)


@pytest.mark.parametrize("layout", LAYOUTS, ids=LAYOUT_IDS)
def test_time_and_time_two_direct_terms(layout):
    m = case(TT, vm=False, ts_order=1, **layout)
    assert 150 <= m.joins[0].sides[0].max_live <= 400


def test_ts_in_any_order_length_and_length():
    # jittered ts, ts_order = 0: length windows never look at ts
    w = gen(20000, 8, 1, 15)
    assert (np.diff(w["ts"]) < 0).any()
    case(LL, wkey=(20000, 8, 1, 15), ts_order=0, batches=3, chunk_events=4096)
    case(LL, wkey=(20000, 8, 1, 15), ts_order=1)


# ------------------------------------------------------------- boundaries ---
@pytest.mark.parametrize("n", [WG - 1, WG, WG + 1])
def test_probes_at_the_workgroup_edge_one_sided_chunk(n):
    # batch 1: 4 B rows; batch 2: n A rows and nothing else: n probes, all of
    # one side, against a tail an earlier batch left
    stream = [1] * 4 + [0] * n
    w = custom(stream, np.arange(4 + n) + 1000, [0, 1, 2, 1] + [i % 3 for i in range(n)])
    got, m = custom_case("from A#window.length(2) as a join B#window.length(3) as b on a.k == b.k "
                         "select a.price as pa, b.price as pb insert into O;", w, cuts=[0, 4, 4 + n])
    assert m.joins[0].triggered[0] == len(got) > n // 2 and m.joins[0].triggered[1] == 0


@pytest.mark.parametrize("span", [TILE - 1, TILE, TILE + 1, 3 * TILE + 5])
def test_staged_span_at_the_tile_edge(span):
    # `span` live B rows, then 3 A rows whose ranges are all of them
    stream = [1] * span + [0] * 3
    w = custom(stream, np.arange(span + 3) + 1000, [i % 4 for i in range(span)] + [0, 1, 3])
    got, m = custom_case("from A#window.length(1) as a join B#window.time(1 hour) as b on a.k == b.k "
                         "select a.k as k, b.price as pb insert into O;", w, cuts=[0, span, span + 3], ts_order=1)
    assert m.joins[0].sides[1].max_live == span and len(got) >= 3 * (span // 4)


def test_length_255_behind_a_selective_filter_spans_chunks():
    # 1 A row in 50 is kept: the 255-row window reaches back over 3 chunks of 4096
    m = case("from A[id == 7]#window.length(255) as a join B[id < 5]#window.length(5) as b on a.k == b.k "
             "select a.ts as ta, b.ts as tb insert into O;", chunk_events=4096, min_side=20)
    assert m.joins[0].sides[0].max_live < 255           # 20,000 rows hold about 200 kept A rows
    m = case("from A[id < 13]#window.length(255) as a join B[id < 5]#window.length(5) as b on a.k == b.k "
             "select a.ts as ta, b.ts as tb insert into O;", chunk_events=1024)
    assert m.joins[0].sides[0].max_live == 255


def test_length_1():
    case("from A#window.length(1) as a join B#window.length(1) as b on a.k == b.k "
         "select a.ts as ta, b.ts as tb insert into O;", batches=3, chunk_events=4096)


def test_a_side_without_kept_rows_gives_no_rows():
    plan = EV2 + ("from A[id > 100]#window.length(5) as a join B#window.length(5) as b on a.k == b.k "
                  "select a.ts as ta, b.ts as tb insert into O;")
    assert model(plan, (20000, 8))[0] == {}
    assert run(plan, gen(20000, 8), batches=2, chunk_events=4096)["O"] == []


# -------------------------------------------------------------- event time --
def test_event_time_shuffled_arrival_equals_send_in_ts_order():
    w = gen(20000, 8)                      # one row per ms: every ts is its own
    plan = EV2 + LT
    want = model(plan, (20000, 8))[0]["O"]
    rt = fs.SiddhiAppRuntime(plan, ts_order=1)
    rt.add_callback("O")
    perm = np.random.default_rng(5).permutation(20000)
    half = 10000
    for part in (perm[:half], perm[half:]):
        rt.process_elements("A", w["ts"][part], [w[c][part] for c in ("k", "ts", "id", "price")],
                            streams=w["stream"][part])
    rt.process_watermark(int(w["ts"][12345]))     # a prefix now, the rest at the end
    rt.flush()
    rt.process_watermark(int(w["ts"][-1]))
    rt.flush()
    got = engine_rows(rt.collect("O"))
    rt.shutdown()
    assert_same_rows(got, want, "event time")


# ---------------------------------------------------------------- snapshot --
@pytest.mark.parametrize("query,opts", [(LT, dict(ts_order=1)), (LL, dict())], ids=["length_time", "length_length"])
def test_snapshot_restore_continues_the_run(query, opts):
    w = gen(20000, 8)
    plan = EV2 + query
    want = model(plan, (20000, 8))[0]["O"]
    cut = 9001
    first = fs.SiddhiAppRuntime(plan, chunk_events=4096, **opts)
    first.add_callback("O")
    first.send("A", w["ts"][:cut], cols(w, 0, cut), streams=w["stream"][:cut])
    first.flush()
    got = engine_rows(first.collect("O"))
    snap = first.snapshot()
    first.shutdown()
    second = fs.SiddhiAppRuntime(plan, chunk_events=4096, **opts)
    second.add_callback("O")
    second.restore(snap)
    second.send("A", w["ts"][cut:], cols(w, cut, 20000), streams=w["stream"][cut:])
    second.flush()
    got += engine_rows(second.collect("O"))
    second.shutdown()
    assert_same_rows(got, want, "snapshot " + query)


def test_snapshot_of_a_different_plan_is_refused():
    w = gen(2000, 8)
    rt = fs.SiddhiAppRuntime(EV2 + LL)
    rt.send("A", w["ts"], cols(w, 0, 2000), streams=w["stream"])
    rt.flush()
    snap = rt.snapshot()
    rt.shutdown()
    for other in (LL.replace("length(100)", "length(50)"), LL.replace("length(3)", "time(3)"),
                  "from A[id > 3] select k, id insert into O;"):
        rt2 = fs.SiddhiAppRuntime(EV2 + other, ts_order=1)
        with pytest.raises(fs.CepStateError):
            rt2.restore(snap)
        rt2.shutdown()


# ------------------------------------------------------------------ errors --
def test_time_window_join_needs_ts_order_1():
    with pytest.raises(fs.UnsupportedPlanException, match="join"):
        fs.SiddhiAppRuntime(EV2 + LT, ts_order=0)
    with pytest.raises(fs.UnsupportedPlanException, match="join"):
        fs.SiddhiAppRuntime(EV2 + TT)              # ts_order defaults to 0


def test_key_stride_2_is_refused():
    with pytest.raises(fs.UnsupportedPlanException, match="join"):
        fs.SiddhiAppRuntime(EV2 + LL, key_stride=2, key_offset=1)


def test_ts_descent_fails_the_flush():
    w = dict(gen(4000, 8))
    ts = w["ts"].copy()
    ts[3000] -= 5
    w["ts"] = ts
    rt = fs.SiddhiAppRuntime(EV2 + LT, ts_order=1)
    rt.add_callback("O")
    rt.send("A", w["ts"], cols(w, 0, 4000), streams=w["stream"])
    with pytest.raises(ValueError, match="event-time order"):
        rt.flush()
    rt.shutdown()


@pytest.mark.parametrize("extra", [0, 1])
def test_time_tail_cap(extra):
    # TAIL_CAP (+ 1) live A rows, then a single probing B row
    n = TAIL_CAP + extra
    stream = np.zeros(n + 1, np.uint8)
    stream[n] = 1
    k = np.arange(n + 1, dtype=np.int32) % 1000
    k[n] = 999
    w = custom(stream, np.full(n + 1, 5000, np.int64), k, price=np.zeros(n + 1))
    rt = fs.SiddhiAppRuntime(EV2 + "from A#window.time(1 hour) as a join B#window.length(1) as b on a.k == b.k "
                                   "select a.ts as ta, b.k as kb insert into O;", ts_order=1)
    rt.add_callback("O")
    rt.send("A", w["ts"], cols(w, 0, n + 1), streams=w["stream"])
    if extra:
        with pytest.raises(fs.CepCapacityError, match="join"):
            rt.flush()
    else:
        rt.flush()
        assert len(rt.collect("O")) == int((k[:n] == 999).sum())
    rt.shutdown()


def test_route_calls_are_refused():
    import torch
    rt = fs.SiddhiAppRuntime(EV2 + LL)
    z = torch.zeros(8, dtype=torch.int64, device="cuda")
    c = [torch.zeros(8, dtype=torch.int32, device="cuda"), z, torch.zeros(8, dtype=torch.int32, device="cuda"),
         torch.zeros(8, dtype=torch.float64, device="cuda")]
    with pytest.raises(fs.UnsupportedPlanException, match="join"):
        rt.route("A", z, c, 2, 0)
    with pytest.raises(fs.UnsupportedPlanException, match="join"):
        rt.route_rows("A", z, c, 2, 0)
    rt.shutdown()


# ---------------------------------------------------- stats and coexistence --
def test_join_stat_stays_zero_without_a_join():
    st = []
    run(EV2 + "from A[id > 3] select k, id insert into O;", gen(5000, 8), stats=st)
    assert st[0].kernel_launches[L.K_JOIN] == 0 and st[0].kernel_launches[L.K_JOIN_VM] == 0


def test_set_enabled():
    w = gen(6000, 8)
    plan = EV2 + LL
    rt = fs.SiddhiAppRuntime(plan)
    rt.add_callback("O")
    rt.send("A", w["ts"][:2000], cols(w, 0, 2000), streams=w["stream"][:2000])
    rt.set_enabled(False)
    rt.send("A", w["ts"][2000:4000], cols(w, 2000, 4000), streams=w["stream"][2000:4000])   # dropped
    rt.set_enabled(True)
    rt.send("A", w["ts"][4000:], cols(w, 4000, 6000), streams=w["stream"][4000:])
    rt.flush()
    got = engine_rows(rt.collect("O"))
    rt.shutdown()
    keep = np.r_[0:2000, 4000:6000]
    seen = {c: w[c][keep] for c in w}
    want = model_run(plan, workload_events(seen))[0]["O"]
    # (arrival numbers count the rows the engine consumed)
    assert [(t, d) for t, _, d in got] == [(t, d) for t, _, d in want]


def test_join_beside_a_filter_and_a_pattern():
    join = ("from A#window.length(50) as a join B#window.time(100) as b on a.id == b.id "
            "select a.k as ka, b.k as kb, a.price + b.price as s insert into J;")
    flt = "from A[price > 0.9] select k, id insert into F;"
    pat = ("partition with (k of A, k of B) begin from every s1=A[price > 0.5] -> s2=B[id % 7 == 0] within 10 sec "
           "select s1.k as k, s1.price as p1, s2.price as p2 insert into P; end;")
    wkey = (6000, 512)
    alone = {"J": model(EV2 + join, wkey)[0]["J"], "F": model(EV2 + flt, wkey)[0]["F"],
             "P": model(EV2 + pat, wkey)[0]["P"]}
    assert min(len(v) for v in alone.values()) > 100
    got = run(EV2 + join + flt + pat, gen(*wkey), outs=("J", "F", "P"), batches=2, ts_order=1, key_capacity=1024)
    for o in ("J", "F", "P"):
        assert_same_rows(got[o], alone[o], "coexistence " + o)
