"""Query chaining on the device: queries reading streams other queries insert
into (derive.hip k_derive builds the readers' views of each batch).

Reference.  A stateless producer can be folded into its reader by hand
(`from M[c]` becomes `from S[p and c']`), so where that twin is expressible it
is run through siddhi_oracle (helpers.oracle_run) and must equal both the
engine on the chained plan and the explicit model (chain_model.chain_run:
the producer's rows, carrying ts and the source row's arrival number, fed to
the reader as events of a defined stream).  Where it is not (`sum(price *
id)`, windows, strict sequences, whose contiguity counts the rows the producer
dropped) the model alone is the reference.  Everything is compared row for
row, bit-exact: ts, arrival number, data.  Parity with Siddhi itself is
unpinned: Siddhi is not buildable here.

Inputs: workload.generate, 20 000 events over 512 keys, one mixed A/B batch.
Each model runs once per (layers, input) and is shared; prefixes of the input
reuse it (every query is causal: the rows of the first n events are the rows
with arrival number < n)."""
import numpy as np
import pytest

import flink_siddhi as fs
from flink_siddhi import _lib as L
from flink_siddhi import workload
from chain_model import chain_run
from helpers import assert_same_rows, engine_rows, oracle_run, workload_events

pytestmark = pytest.mark.gpu

N, KEYS = 20000, 512
EV = ("define stream A (k int, ts long, id int, price double);"
      "define stream B (k int, ts long, id int, price double);")
DEF_B = "define stream B (k int, ts long, id int, price double);"


def part(keys, q):
    return "partition with (" + keys + ") begin " + q + " end;"


_W = {}
_EVENTS = {}
_MODEL = {}
_TWIN = {}


def gen(n=N, keys=KEYS, rate=1):
    if (n, keys, rate) not in _W:
        _W[(n, keys, rate)] = workload.generate(0, n, keys, rate=rate)
    return _W[(n, keys, rate)]


def events(wkey=(N, KEYS, 1)):
    if wkey not in _EVENTS:
        _EVENTS[wkey] = workload_events(gen(*wkey))
    return _EVENTS[wkey]


def model(layers, wkey=(N, KEYS, 1)):
    key = (tuple(layers), wkey)
    if key not in _MODEL:
        _MODEL[key] = chain_run(layers, events(wkey))
    return _MODEL[key]


def twin(plan, wkey=(N, KEYS, 1)):
    if (plan, wkey) not in _TWIN:
        _TWIN[(plan, wkey)] = oracle_run(plan, events(wkey))
    return _TWIN[(plan, wkey)]


def cols(w, s, e):
    return [w["k"][s:e], w["ts"][s:e], w["id"][s:e], w["price"][s:e]]


def run(plan, w, outs=("O",), cuts=None, device=False, stats=None, **opts):
    """The chained plan on the engine: the input as mixed A/B batches cut at `cuts`."""
    rt = fs.SiddhiAppRuntime(plan, **opts)
    for o in outs:
        rt.add_callback(o)
    n = len(w["ts"])
    cuts = [0, n] if cuts is None else cuts
    if device:
        import torch
        d = {c: torch.from_numpy(np.ascontiguousarray(w[c])).cuda() for c in ("k", "ts", "id", "price", "stream")}
    for s, e in zip(cuts[:-1], cuts[1:]):
        if device:   # slices of one allocation: odd first rows, odd pointers
            rt.send("A", d["ts"][s:e], [d["k"][s:e], d["ts"][s:e], d["id"][s:e], d["price"][s:e]],
                    streams=d["stream"][s:e])
        else:
            rt.send("A", w["ts"][s:e], cols(w, s, e), streams=w["stream"][s:e])
        rt.flush()
    got = {o: engine_rows(rt.collect(o)) for o in outs}
    if stats is not None:
        stats.append(rt.stats())
    rt.shutdown()
    return got


def check(plan, layers, outs=("O",), min_rows=200, twin_plan=None, twin_outs=None, **kw):
    want, _ = model(layers)
    if twin_plan is not None:
        tw = twin(twin_plan)
        for o in (outs if twin_outs is None else twin_outs):
            assert_same_rows(want.get(o, []), tw.get(o, []), "model vs inlined twin, " + o)
    got = run(plan, gen(), outs=outs, **kw)
    for o in outs:
        assert_same_rows(got[o], want.get(o, []), o + ": " + plan)
        assert len(got[o]) >= min_rows, (o, len(got[o]))
    return got


# ------------------------------------------------------ the config-3 shape --
A1 = "from A[price > 0.1] select k, ts, id, price insert into A1;"
B1 = "from B[id % 7 != 0] select k, ts, id, price insert into B1;"
DEF_A1B1 = ("define stream A1 (k int, ts long, id int, price double);"
            "define stream B1 (k int, ts long, id int, price double);")
CFG3_SEL = "select s1.k as k, s1.price as p1, s2.price as p2, s2.ts as t insert into O;"
CFG3_Q = part("k of A1, k of B1", "from every s1=A1[price > 0.5] -> s2=B1[id % 5 == 0] within 1 sec " + CFG3_SEL)
CFG3 = EV + A1 + B1 + CFG3_Q
CFG3_TWIN = EV + part("k of A, k of B", "from every s1=A[price > 0.1 and price > 0.5] -> "
                                        "s2=B[id % 7 != 0 and id % 5 == 0] within 1 sec " + CFG3_SEL)
CFG3_LAYERS = [EV + A1 + B1, DEF_A1B1 + CFG3_Q]


@pytest.mark.parametrize("ts_order", [1, 0])
def test_config3_shape(ts_order):
    st = []
    want, _ = model(CFG3_LAYERS)
    assert_same_rows(want["O"], twin(CFG3_TWIN)["O"], "model vs inlined twin")
    got = run(CFG3, gen(), outs=("O", "A1", "B1"), stats=st, ts_order=ts_order)
    for o in ("O", "A1", "B1"):
        assert_same_rows(got[o], want[o], o)
    assert len(got["O"]) >= 200
    if ts_order == 1:   # the closed form survives the view (aligned, term lists)
        assert st[0].kernel_launches[L.K_CF_PARTITION] > 0
    assert st[0].kernel_launches[L.K_OTHER] > 0   # k_derive


# ---------------------------------------------------------- computed column --
M = "from A[price > 0.1] select k, ts, id, price * 2.0 as p2 insert into M;"
DEF_M = "define stream M (k int, ts long, id int, p2 double);"

FILTER_Q = "from M[p2 > 1.0 and id < 40] select k, id, p2 insert into O;"
GROUP_Q = "from M[id > 4] select k, sum(p2) as s, avg(p2) as a, count() as c group by k having s > 3.0 insert into O;"
WLEN_Q = part("k of M", "from M#window.length(4) select k, sum(p2) as s, min(p2) as mn, count() as c insert into O;")
WTIME_Q = part("k of M", "from M#window.time(50) select k, sum(p2) as s, max(id) as mx, count() as c insert into O;")
PAT3_Q = part("k of M, k of B", "from every a=M[p2 > 1.0] -> b=B[id > 20] -> c=M[p2 < 1.0] within 2 sec "
                                "select a.id as x, b.id as y, c.p2 as z, c.ts as t insert into O;")
SEQ_Q = part("k of M, k of B", "from every s1=M[p2 > 1.0], s2=B[id < 40]+, s3=M[p2 < 1.0] within 10 sec "
                               "select s1.k as k, s1.p2 as p1, s2[last].price as pl, s3.ts as t3 insert into O;")


def test_computed_column_filter():
    check(EV + M + FILTER_Q, [EV + M, DEF_M + FILTER_Q], outs=("O", "M"),
          twin_plan=EV + M + "from A[price > 0.1 and price * 2.0 > 1.0 and id < 40] "
                             "select k, id, price * 2.0 as p2 insert into O;")


def test_computed_column_group_by_having():
    check(EV + M + GROUP_Q, [EV + M, DEF_M + GROUP_Q])


def test_computed_column_length_window():
    check(EV + M + WLEN_Q, [EV + M, DEF_M + WLEN_Q])


def test_computed_column_time_window():
    _, live = model([EV + M, DEF_M + WTIME_Q])
    assert 1 < live <= 16, "test shape: model occupancy %d" % live
    check(EV + M + WTIME_Q, [EV + M, DEF_M + WTIME_Q], pending_slots=16)


def test_computed_column_three_state_pattern():
    check(EV + M + PAT3_Q, [EV + M, DEF_M + DEF_B + PAT3_Q], min_rows=50,
          twin_plan=EV + part("k of A, k of B",
                              "from every a=A[price > 0.1 and price * 2.0 > 1.0] -> b=B[id > 20] -> "
                              "c=A[price > 0.1 and price * 2.0 < 1.0] within 2 sec "
                              "select a.id as x, b.id as y, c.price * 2.0 as z, c.ts as t insert into O;"))


def test_computed_column_sequence_count_state_last_capture():
    check(EV + M + SEQ_Q, [EV + M, DEF_M + DEF_B + SEQ_Q], min_rows=50)


def test_computed_key():
    g = "from A select id % 64 as g, ts, id, price insert into G;"
    q = part("g of G", "from G[price > 0.2]#window.length(3) select g, sum(price) as s, count() as c insert into O;")
    check(EV + g + q, [EV + g, "define stream G (g int, ts long, id int, price double);" + q])


def test_string_column_passed_through():
    sdef = "define stream S (k int, name string, v long);"
    p = "from S[v > 10] select k, name, v * 2 as w insert into T;"
    q = "from T[name == 'x' or name == 'z'] select k, name, w insert into O;"
    w = gen()
    names = ["x", "y", "z"]
    pick = (w["id"] % 3).astype(np.int64)
    v = w["id"].astype(np.int64)
    evs = [("S", int(t), (int(k), names[int(i)], int(x)))
           for t, k, i, x in zip(w["ts"], w["k"], pick, v)]
    want, _ = chain_run([sdef + p, "define stream T (k int, name string, w long);" + q], evs)
    rt = fs.SiddhiAppRuntime(sdef + p + q)
    ids = np.array([rt.intern(s) for s in names], np.int32)
    for o in ("O", "T"):
        rt.add_callback(o)
    rt.send("S", w["ts"], [w["k"], ids[pick], v])
    rt.flush()
    for o in ("O", "T"):
        got = [(t, s, (d[0], rt.lookup(d[1]), d[2])) for t, s, d in engine_rows(rt.collect(o))]
        assert_same_rows(got, want[o], "string pass-through " + o)
        assert len(got) >= 1000
    rt.shutdown()


def test_sum_of_an_expression_through_a_producer():
    p = "from A select k, price * id as notional insert into NT;"
    q = "from NT select k, sum(notional) as s, count() as c group by k insert into O;"
    check(EV + p + q, [EV + p, "define stream NT (k int, notional double);" + q], min_rows=5000)


# ------------------------------------------------------- depth 3, fan-out ----
M2 = "from M[p2 < 1.6] select k, ts, id, p2 + 1.0 as p3 insert into M2;"
M3 = "from M2[id % 3 != 0] select k, ts, id, p3 * 0.5 as p4 insert into M3;"
FAN = ("from M[p2 > 1.2] select k, p2 insert into O1;"
       "from M select k, sum(p2) as s, count() as c group by k insert into O2;" +
       part("k of M", "from every a=M[p2 > 1.5] -> b=M[p2 < 0.5] select a.id as x, b.id as y, b.ts as t insert into O3;"))
DEEP_Q = "from M3[p4 > 0.7] select k, id, p4 insert into O4;"


def test_depth_three_and_fan_out():
    plan = EV + M + M2 + M3 + FAN + DEEP_Q
    layers = [EV + M, DEF_M + M2 + FAN, "define stream M2 (k int, ts long, id int, p3 double);" + M3,
              "define stream M3 (k int, ts long, id int, p4 double);" + DEEP_Q]
    outs = ("O1", "O2", "O3", "O4", "M", "M2", "M3")
    # the two filters at depth 1 and depth 3 have single-layer twins
    tw = (EV + "from A[price > 0.1 and price * 2.0 > 1.2] select k, price * 2.0 as p2 insert into O1;"
          "from A[price > 0.1 and price * 2.0 < 1.6 and id % 3 != 0 and (price * 2.0 + 1.0) * 0.5 > 0.7] "
          "select k, id, (price * 2.0 + 1.0) * 0.5 as p4 insert into O4;")
    got = check(plan, layers, outs=outs, min_rows=100, twin_plan=tw, twin_outs=("O1", "O4"))
    # the derived stream's own rows are the producer's, run alone
    alone = run(EV + M, gen(), outs=("M",))["M"]
    assert_same_rows(got["M"], alone, "M vs its producer alone")


# ------------------------------------------------------------ mixed reader ---
MIX_SEL = "select a.k as k, a.id as x, b.id as y, b.ts as t insert into O;"


def test_mixed_reader_identity_layout():
    q = part("k of A1, k of B", "from every a=A1[id > 10] -> b=B[id > 20] within 1 sec " + MIX_SEL)
    check(EV + A1 + q, [EV + A1, "define stream A1 (k int, ts long, id int, price double);" + DEF_B + q],
          twin_plan=EV + A1 + part("k of A, k of B", "from every a=A[price > 0.1 and id > 10] -> b=B[id > 20] "
                                                     "within 1 sec " + MIX_SEL))


def test_mixed_reader_reordered_columns():
    # R swaps k and id: B's rows of the same batch must keep reading their own columns
    r = "from A[price > 0.1] select id as k, ts, k as id, price insert into R;"
    q = part("k of R, k of B", "from every a=R[id > 100] -> b=B[id > 20] within 1 sec " + MIX_SEL)
    check(EV + r + q, [EV + r, "define stream R (k int, ts long, id int, price double);" + DEF_B + q], min_rows=50,
          twin_plan=EV + part("id of A, k of B", "from every a=A[price > 0.1 and k > 100] -> b=B[id > 20] within 1 sec "
                                                 "select a.id as k, a.k as x, b.id as y, b.ts as t insert into O;"))


# ------------------------------------------------- a config-5-style group ----
def test_multi_query_group_over_a_derived_stream():
    qs = "".join("from M[p2 > %s] select k, sum(p2) as total, count() as n group by k having total > 1.0 "
                 "insert into Agg%d;" % (repr(0.25 * i + 0.25), i) for i in range(4))
    outs = tuple("Agg%d" % i for i in range(4))
    st = []
    check(EV + M + qs, [EV + M, DEF_M + qs], outs=outs, stats=st)
    assert st[0].kernel_launches[L.K_MQ_PARTITION] > 0   # one group, one view


# ---------------------------------------------------------------- ambiguity --
XY_Q = part("k of X, k of Y", "from every x=X[id > 5] -> y=Y[id > 5] within 1 sec "
                              "select x.k as k, x.id as a, y.id as b, y.ts as t insert into O;")
DEF_XY = ("define stream X (k int, ts long, id int, price double);"
          "define stream Y (k int, ts long, id int, price double);")


def test_two_producers_one_source_disjoint():
    xy = ("from A[price > 0.5] select k, ts, id, price insert into X;"
          "from A[price <= 0.5] select k, ts, id, price insert into Y;")
    check(EV + xy + XY_Q, [EV + xy, DEF_XY + XY_Q],
          twin_plan=EV + xy + part("k of A", "from every x=A[price > 0.5 and id > 5] -> y=A[price <= 0.5 and id > 5] "
                                             "within 1 sec select x.k as k, x.id as a, y.id as b, y.ts as t "
                                             "insert into O;"))


def test_two_producers_one_source_overlapping_is_refused_at_flush():
    xy = ("from A[price > 0.3] select k, ts, id, price insert into X;"
          "from A[price < 0.6] select k, ts, id, price insert into Y;")
    w = gen()
    rt = fs.SiddhiAppRuntime(EV + xy + XY_Q)
    rt.add_callback("O")
    rt.send("A", w["ts"], cols(w, 0, N), streams=w["stream"])
    with pytest.raises(fs.UnsupportedPlanException, match="two derived streams"):
        rt.flush()
    rt.shutdown()


# ------------------------------------------------------------------ geometry --
GEO = EV + M + B1 + FILTER_Q + part("k of M, k of B1", "from every a=M[p2 > 1.0] -> b=B1[id > 20] within 1 sec "
                                                       "select a.k as k, a.p2 as p, b.id as y insert into P;")
GEO_LAYERS = [EV + M + B1, DEF_M + "define stream B1 (k int, ts long, id int, price double);" + FILTER_Q +
              part("k of M, k of B1", "from every a=M[p2 > 1.0] -> b=B1[id > 20] within 1 sec "
                                      "select a.k as k, a.p2 as p, b.id as y insert into P;")]
GEO_OUTS = ("O", "P", "M", "B1")


def prefix(rows, n):
    return [r for r in rows if r[1] < n]


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 4095, 4097])
@pytest.mark.parametrize("device", [False, True])
def test_geometry_one_send(n, device):
    want, _ = model(GEO_LAYERS)
    w = {c: v[:n] for c, v in gen().items()}
    got = run(GEO, w, outs=GEO_OUTS, device=device)
    for o in GEO_OUTS:
        assert_same_rows(got[o], prefix(want[o], n), "%s n=%d" % (o, n))
    assert len(got["M"]) + len(got["B1"]) > 0 or n < 3
    if n >= 4095:
        assert len(got["O"]) >= 100 and len(got["P"]) >= 10


@pytest.mark.parametrize("device", [False, True])
@pytest.mark.parametrize("chunk", [0, 4096])
def test_geometry_ragged_batches(device, chunk):
    want, _ = model(GEO_LAYERS)
    # odd lengths, odd first rows (seven odd lengths cannot add up to an even N: the last row goes alone)
    cuts = [0, 1, 1234, 4097, 8192, 12345, 17778, N - 1, N]
    assert all((b - a) % 2 == 1 for a, b in zip(cuts[:-1], cuts[1:]))
    opts = {"chunk_events": chunk} if chunk else {}
    got = run(GEO, gen(), outs=GEO_OUTS, cuts=cuts, device=device, **opts)
    for o in GEO_OUTS:
        assert_same_rows(got[o], want[o], "%s ragged" % o)
        assert len(got[o]) >= 200


def test_batch_without_stream_column():
    # only A's rows, sent as a plain A batch: the view gets a handle column of its own
    w = gen()
    a = w["stream"] == 0
    evs = [e for e in events() if e[0] == "A"]
    q = FILTER_Q + WLEN_Q.replace("into O;", "into W;")
    want, _ = chain_run([EV + M, DEF_M + q], evs)
    rt = fs.SiddhiAppRuntime(EV + M + q)
    for o in ("O", "W", "M"):
        rt.add_callback(o)
    rt.send("A", w["ts"][a], [w["k"][a], w["ts"][a], w["id"][a], w["price"][a]])
    rt.flush()
    for o in ("O", "W", "M"):
        got = engine_rows(rt.collect(o))
        assert_same_rows(got, want[o], o + " (no stream column)")
        assert len(got) >= 1000
    rt.shutdown()


# ---------------------------------------------------------------- event time --
def test_event_time_reorder():
    w0 = gen()
    rng = np.random.default_rng(11)
    arrival = np.argsort(np.arange(N) + rng.integers(0, 500, N), kind="stable")
    w = {c: w0[c][arrival] for c in ("k", "ts", "id", "price", "stream")}
    o = np.argsort(w["ts"], kind="stable")   # (ts, arrival): the order the engine sees
    srt = {c: w[c][o] for c in w}
    plan = EV + M + FILTER_Q + PAT3_Q.replace("into O;", "into P;")
    want, _ = chain_run([EV + M, DEF_M + DEF_B + FILTER_Q + PAT3_Q.replace("into O;", "into P;")],
                        workload_events(srt))
    rt = fs.SiddhiAppRuntime(plan)
    for out in ("O", "P"):
        rt.add_callback(out)
    cuts = np.linspace(0, N, 6).astype(int)
    suffix_min = np.minimum.accumulate(w["ts"][::-1])[::-1]
    for s, e in zip(cuts[:-1], cuts[1:]):
        rt.process_elements("A", w["ts"][s:e], cols(w, s, e), streams=w["stream"][s:e])
        if e < N:
            rt.process_watermark(int(suffix_min[e]) - 1)
    rt.process_watermark(int(w["ts"].max()))
    assert rt.buffered() == 0
    rt.flush()
    for out, least in (("O", 1000), ("P", 50)):
        got = engine_rows(rt.collect(out))
        assert_same_rows(got, want[out], "event time " + out)
        assert len(got) >= least
    rt.shutdown()


# --------------------------------------------------------- snapshot / restore --
@pytest.mark.parametrize("query,layer,opts", [
    (WLEN_Q, DEF_M + WLEN_Q, {}),
    (WTIME_Q, DEF_M + WTIME_Q, {"pending_slots": 16}),
    (PAT3_Q, DEF_M + DEF_B + PAT3_Q, {}),
], ids=["length", "time", "pattern"])
def test_snapshot_restore_mid_stream(query, layer, opts):
    plan = EV + DEF_M + M + query   # M defined and derived
    want, _ = model([EV + M, layer])
    w = gen()
    h = N // 2 + 1
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
    rt2.send("A", w["ts"][h:], cols(w, h, N), streams=w["stream"][h:])
    rt2.flush()
    second = engine_rows(rt2.collect("O"))
    rt2.shutdown()
    assert_same_rows(first + second, want["O"], "snapshot/restore " + query)
    assert len(first) >= 20 and len(second) >= 20
    # the plan hash covers the chain: the same text with the producer writing elsewhere compiles to
    # the same programs and state, but M is then fed from outside only, and the snapshot is refused
    unchained = EV + DEF_M + M.replace("insert into M;", "insert into MX;") + query
    rt3 = fs.SiddhiAppRuntime(unchained, **opts)
    with pytest.raises(fs.CepStateError):
        rt3.restore(snap)
    rt3.shutdown()


# ------------------------------------------------------- rows sent to M itself --
def test_external_rows_into_the_derived_stream():
    q = FILTER_Q + WLEN_Q.replace("into O;", "into W;")
    w = gen()
    ext = workload.generate(N, 6000, KEYS, rate=1)
    cuts = [0, 5001, 11111, N]
    ecuts = [0, 1999, 4000, 6000]
    evs = []
    sends = []
    for i in range(3):
        s, e = cuts[i], cuts[i + 1]
        part_w = {c: v[s:e] for c, v in w.items()}
        evs += workload_events(part_w)
        sends.append(("A", part_w))
        s, e = ecuts[i], ecuts[i + 1]
        x = {c: v[s:e] for c, v in ext.items()}
        evs += [("M", int(t), (int(k), int(t), int(i_), float(p)))
                for t, k, i_, p in zip(x["ts"], x["k"], x["id"], x["price"])]
        sends.append(("M", x))
    want, _ = chain_run([EV + M, DEF_M + q], evs)
    rt = fs.SiddhiAppRuntime(EV + M + q)
    for o in ("O", "W"):
        rt.add_callback(o)
    for sid, x in sends:
        if sid == "A":
            rt.send("A", x["ts"], [x["k"], x["ts"], x["id"], x["price"]], streams=x["stream"])
        else:
            rt.send("M", x["ts"], [x["k"], x["ts"], x["id"], x["price"]])
    rt.flush()
    for o in ("O", "W"):
        got = engine_rows(rt.collect(o))
        assert_same_rows(got, want[o], "external rows, " + o)
        assert len(got) >= 1000
    rt.shutdown()


# -------------------------------------------------------------- key shuffle ----
def test_route_batch_is_refused():
    import ctypes as C
    import torch
    w = gen()
    d = {c: torch.from_numpy(np.ascontiguousarray(w[c][:4096])).cuda() for c in ("k", "ts", "id", "price", "stream")}
    rt = fs.SiddhiAppRuntime(CFG3)
    ptrs = (C.c_void_p * 4)(*[d[c].data_ptr() for c in ("k", "ts", "id", "price")])
    b = L.cep_batch(n=4096, ts=C.c_void_p(d["ts"].data_ptr()), stream=C.c_void_p(d["stream"].data_ptr()),
                    input=rt.input_handle("A"), ncols=4, cols=ptrs, on_device=1)
    out = torch.empty((4096, 16), dtype=torch.int64, device="cuda")
    counts = (C.c_int64 * 2)()
    torch.cuda.synchronize()
    for fn in (rt._lib.cep_route_batch, rt._lib.cep_route_rows):
        rc = fn(rt._h, C.byref(b), 2, 0, C.c_void_p(out.data_ptr()), out.shape[0], counts)
        assert rc == L.CEP_E_UNSUPPORTED
        assert "query chaining" in rt._lib.cep_last_error(rt._h).decode()
    rt.shutdown()
