"""Logical pattern states on the device (`A -> B and C`, `A -> (B or C) -> D`:
the pattern branch of nfa_key) against tests/logic_model.py, row
for row and bit for bit: ts, arrival number, data.  The three-stream workload
of test_gpu_nfa.py with a STRING column; a capture of a side that never
matched is 0 (numeric) or dictionary id -1 (STRING) in an output row
(include/cep.h), the model's None maps to that as in test_gpu_seq_grammar.py.
Each model runs once per (plan, input) and is shared."""
import numpy as np
import pytest

import flink_siddhi as fs
from flink_siddhi import _lib as L
from flink_siddhi import workload
from helpers import assert_same_rows, engine_rows
from logic_model import LogicModel, model_run

pytestmark = pytest.mark.gpu

EV3 = "".join("define stream %s (k int, ts long, id int, price double, name string);" % s for s in "ABC")
STREAMS = ("A", "B", "C")
NAMES = ("zero", "one", "two", "three")
COLS = ("k", "ts", "id", "price", "name")
NULL_NUMERIC, NULL_STRING = 0, -1      # include/cep.h: a capture of a state that never matched
P3 = "partition with (k of A, k of B, k of C) begin "

_W, _MODEL = {}, {}


def three_streams(n=20000, keys=256, jitter=0):
    key = (n, keys, jitter)
    if key not in _W:
        w = workload.generate(0, n, keys, rate=1)
        w["stream"] = ((w["price"] * 1000).astype(np.int64) % 3).astype(np.uint8)
        if jitter:     # arrival order is not ts order
            w["ts"] = w["ts"] + np.random.default_rng(5).integers(-jitter, jitter + 1, n)
        w["name"] = ((w["id"] + w["k"]) % len(NAMES)).astype(np.int32)      # dictionary ids, interned in this order
        _W[key] = w
    return _W[key]


def events(w):
    k, ts, i, p, nm, st = (w[c].tolist() for c in ("k", "ts", "id", "price", "name", "stream"))
    return [(STREAMS[st[j]], ts[j], (k[j], ts[j], i[j], p[j], NAMES[nm[j]])) for j in range(len(ts))]


def model(plan, wkey):
    if (plan, wkey) not in _MODEL:
        _MODEL[(plan, wkey)] = model_run(plan, events(three_streams(*wkey)))
    return _MODEL[(plan, wkey)]


def expected(plan, rows, out="O"):
    """Model rows as the engine delivers them: names as dictionary ids, None as the null of the column's type."""
    types = [t for _, t in fs.plan_schema(plan, out)]

    def conv(v, t):
        if t == "string":
            return NULL_STRING if v is None else NAMES.index(v)
        return NULL_NUMERIC if v is None else v
    return [(ts, seq, tuple(conv(v, t) for v, t in zip(d, types))) for ts, seq, d in rows]


def make(plan, outs=("O",), **opts):
    rt = fs.SiddhiAppRuntime(plan, **opts)
    assert [rt.intern(nm) for nm in NAMES] == list(range(len(NAMES)))
    for o in outs:
        rt.add_callback(o)
    return rt


def send(rt, w, s, e, d=None):
    src = w if d is None else d
    rt.send("A", src["ts"][s:e], [src[c][s:e] for c in COLS], streams=src["stream"][s:e])
    rt.flush()


def run(plan, w, outs=("O",), cuts=None, device=False, **opts):
    rt = make(plan, outs, **opts)
    d = None
    if device:
        import torch
        d = {c: torch.from_numpy(np.ascontiguousarray(w[c])).cuda() for c in COLS + ("stream",)}
    cuts = [0, len(w["ts"])] if cuts is None else cuts
    try:
        for s, e in zip(cuts[:-1], cuts[1:]):
            send(rt, w, s, e, d)
        got = {o: engine_rows(rt.collect(o)) for o in outs}
        kl = list(rt.stats().kernel_launches)
    finally:
        rt.shutdown()
    return got, kl


def case(query, min_rows, wkey=(20000, 256, 0), **kw):
    plan = EV3 + query
    want, m = model(plan, wkey)
    got, kl = run(plan, three_streams(*wkey), **kw)
    assert kl[L.K_WALK] > 0 and kl[L.K_MQ_WALK] == 0 and kl[L.K_CF_WALK] == 0, kl
    assert len(want.get("O", [])) >= min_rows, len(want.get("O", []))
    assert_same_rows(got["O"], expected(plan, want.get("O", [])), query)
    return want["O"], m


def half_filled_at(plan, w, cut):
    """Partials with exactly one side filled after the first `cut` events."""
    m = LogicModel(plan)
    for sid, ts, row in events(w)[:cut]:
        m.send(sid, ts, row)
    return sum(len(p.filled) == 1 for d in m.instances for i in d.values() for p in i.partials)


SEL3 = (" select a.k as k, a.id as ai, b.price as bp, c.price as cp, b.name as bn, c.name as cn, c.ts as ct "
        "insert into O; end;")
AND_W = P3 + "from every a=A[price > 0.3] -> b=B[id % 3 == 0] and c=C[price < 0.6] within 5 sec" + SEL3
OR_W = P3 + "from every a=A[price > 0.3] -> b=B[id % 3 == 0] or c=C[price < 0.2] within 2 sec" + SEL3


# ---- a group at the end ------------------------------------------------------------------------
@pytest.mark.parametrize("ts_order", [0, 1])
def test_and_within(ts_order):
    rows, m = case(AND_W, 500, ts_order=ts_order)
    assert m.stat("half_filled_seen") > 500
    # some partials expired: the same plan without `within` matches more
    assert len(rows) < len(model(EV3 + AND_W.replace(" within 5 sec", ""), (20000, 256, 0))[0]["O"])


@pytest.mark.parametrize("ts_order", [0, 1])
def test_or_within(ts_order):
    rows, m = case(OR_W, 500, ts_order=ts_order)
    # both sides complete partials; the partner's captures are null: price 0, name id -1
    assert {(d[2] is None, d[3] is None) for _, _, d in rows} == {(True, False), (False, True)}
    assert {(d[4] is None, d[5] is None) for _, _, d in rows} == {(True, False), (False, True)}
    assert any(d[4] == NAMES[0] for _, _, d in rows)       # dictionary id 0 is a real string


def test_and_or_without_within_and_with_parentheses():
    case(P3 + "from every a=A[price > 0.6] -> (b=B[id % 3 == 0] and c=C[price < 0.6])" + SEL3, 500)
    case(P3 + "from every a=A[price > 0.6] -> (b=B[id % 5 == 0] or c=C[price < 0.1])" + SEL3, 500)


# ---- a group in the middle ---------------------------------------------------------------------
def test_or_group_in_the_middle():
    rows, m = case(P3 + "from every a=A[price > 0.4] -> (b=B[id % 3 == 0] or c=C[price < 0.3]) -> d=A[id > a.id] "
                   "within 8 sec select a.id as ai, b.id as bi, c.name as cn, d.id as di, d.ts as dt insert into O; end;",
                   300)
    assert {(d[1] is None, d[2] is None) for _, _, d in rows} == {(True, False), (False, True)}


def test_and_group_in_the_middle():
    case(P3 + "from every a=A[price > 0.4] -> (b=B[id % 2 == 0] and c=C[price < 0.7]) -> d=A "
         "within 8 sec select a.id as ai, b.name as bn, c.price as cp, d.id as di, d.ts as dt insert into O; end;", 300)


def test_two_groups_six_states():
    case(P3 + "from every a=A[price > 0.5] -> (b=B and c=C) -> d=A[id > 10] -> (e=B[price > b.price] or f=C[id < 25]) "
         "within 20 sec select a.id as ai, b.id as bi, c.id as ci, d.id as di, e.price as ep, f.name as fn "
         "insert into O; end;", 100, wkey=(20000, 64, 0))


# ---- conditions in the walk's interpreter and in the partition pass ----------------------------
def test_side_conditions_reading_the_start_capture():
    rows, m = case(P3 + "from every a=A[price > 0.2] -> b=B[id > a.id and price < a.price + 0.5] and "
                   "c=C[id % 7 != a.id % 7] within 6 sec" + SEL3, 300)
    assert m.stat("half_filled_seen") > 300
    case(P3 + "from every a=A[price > 0.2] -> b=B[id > a.id] or c=C[price > a.price] within 3 sec" + SEL3, 300)


def test_sides_without_conditions():
    case(P3 + "from every a=A -> b=B and c=C within 3 sec" + SEL3, 1000)
    case(P3 + "from every a=A -> b=B or c=C within 1 sec" + SEL3, 1000)


# ---- non-`every`, unpartitioned ----------------------------------------------------------------
def test_non_every_and_unpartitioned():
    sel = " select a.ts as at, b.ts as bt, c.ts as ct, b.name as bn insert into O;"
    rows, _ = case("from a=A[id == 3] -> b=B[id == 4] and c=C[id == 5]" + sel, 1, wkey=(20000, 16, 0))
    assert len(rows) == 1
    rows, _ = case("from a=A[id == 3] -> (b=B[id == 4] or c=C[id == 5]) -> d=A[id == 6]" + sel, 1, wkey=(20000, 16, 0))
    assert len(rows) == 1
    # `every`, one list for the whole stream
    case("from every a=A[id == 3] -> b=B[id > 40] and c=C[id < 9] within 50 milliseconds" + sel, 50,
         wkey=(20000, 16, 0))
    # non-`every` under a partition: one match per key
    rows, _ = case(P3 + "from a=A -> b=B[id > a.id] and c=C" + SEL3, 200)
    assert len(rows) == len({d[0] for _, _, d in rows})


# ---- lists longer than pending_slots -----------------------------------------------------------
PLONG = (P3 + "from every a=A[price > 0.1] -> b=B[id % 4 == 0] and c=C[id % 211 == 0] within 10 sec "
         "select a.k as k, a.price as ap, b.id as bi, c.ts as ct, b.name as bn insert into O; end;")


@pytest.mark.parametrize("batches,chunk", [(1, 1 << 22), (4, 4096)])
def test_pending_lists_beyond_slots_with_half_filled_partials(batches, chunk):
    # 16 keys at 1 event/ms: every key keeps far more live partials than its 16
    # inline slots, most of them half filled (b arrives long before the rare c);
    # the rest live in the pending pool across windows, chunks and batches
    wkey = (40000, 16, 0)
    cuts = np.linspace(0, wkey[0], batches + 1).astype(int).tolist()
    rows, m = case(PLONG, 1000, wkey=wkey, cuts=cuts, pending_slots=16, chunk_events=chunk)
    assert m.stat("max_live") >= 40 and m.stat("half_filled_seen") > 1000


def test_pending_lists_beyond_slots_or_group_in_the_middle():
    case(P3 + "from every a=A[price > 0.1] -> (b=B[id % 4 == 0] or c=C[id % 5 == 0]) -> d=A[id % 211 == 0] "
         "within 10 sec select a.k as k, b.id as bi, c.name as cn, d.ts as dt insert into O; end;",
         1000, wkey=(40000, 16, 0), pending_slots=16, chunk_events=4096)


# ---- chunks, batches, host and device input ----------------------------------------------------
@pytest.mark.parametrize("device", [False, True])
def test_chunks_and_batches_cut_between_the_two_sides(device):
    w = three_streams()
    cuts = [0, 6001, 13337, len(w["ts"])]
    for cut in cuts[1:-1]:
        assert half_filled_at(EV3 + AND_W, w, cut) > 50
    case(AND_W, 500, cuts=cuts, chunk_events=4096, device=device)
    case(OR_W, 500, cuts=cuts, chunk_events=4096, device=device)


# ---- snapshot / restore ------------------------------------------------------------------------
def test_snapshot_between_the_two_sides_restores_and_continues():
    w = three_streams()
    plan = EV3 + AND_W
    want, _ = model(plan, (20000, 256, 0))
    half = 9973
    assert half_filled_at(plan, w, half) > 50
    rt = make(plan, chunk_events=4096)
    send(rt, w, 0, half)
    first = engine_rows(rt.collect("O"))
    snap = rt.snapshot()
    rt.shutdown()
    rt2 = make(plan, chunk_events=4096)
    rt2.restore(snap)
    send(rt2, w, half, len(w["ts"]))
    second = engine_rows(rt2.collect("O"))
    rt2.shutdown()
    assert len(first) > 100 and len(second) > 100
    assert_same_rows(first + second, expected(plan, want["O"]), "snapshot between the sides")
    # `and` state is no `or` state: the plans differ in st_logic only
    rt3 = make(EV3 + AND_W.replace(" and c=C", " or c=C"), chunk_events=4096)
    try:
        with pytest.raises(L.CepStateError):
            rt3.restore(snap)
    finally:
        rt3.shutdown()


# ---- ts in any order ---------------------------------------------------------------------------
def test_ts_order_0_on_a_stream_with_arrival_jitter():
    wkey = (20000, 256, 1500)
    w = three_streams(*wkey)
    assert (np.diff(w["ts"]) < 0).sum() > 5000
    case(AND_W, 300, wkey=wkey, ts_order=0, chunk_events=4096)
    case(OR_W, 300, wkey=wkey, ts_order=0, chunk_events=4096)


# ---- delivery options --------------------------------------------------------------------------
def test_ordered_output_and_omit_seq():
    plan = EV3 + OR_W
    want = expected(plan, model(plan, (20000, 256, 0))[0]["O"])
    w = three_streams()
    rt = make(plan, ordered_output=1, omit_seq=1, chunk_events=4096)
    send(rt, w, 0, 7000)
    send(rt, w, 7000, len(w["ts"]))
    out = rt.collect("O")
    rt.shutdown()
    assert len(out.seq) == 0 and len(out.ts) == len(want) > 500
    assert out.ts.tolist() == [ts for ts, _, _ in want]
    for c, col in enumerate(out.cols):
        assert col.tolist() == [d[c] for _, _, d in want]
    got, _ = run(plan, w, ordered_output=0)      # the same rows in any order
    assert sorted(got["O"]) == sorted(want)


# ---- beside a multi-query group ----------------------------------------------------------------
def test_logical_query_beside_a_multi_query_group():
    plan = EV3 + (P3 +
                  "from every s1=A[price > 0.5], s2=B[id < 30]+, s3=C[id > 20] within 10 sec "
                  "select s1.k as k, s1.price as p1, s2[last].price as p2, s3.price as p3 insert into O1;"
                  "from every s1=A[price > 0.25], s2=B[id < 25]+, s3=C[id > 10] within 10 sec "
                  "select s1.k as k, s1.price as p1, s2[last].price as p2, s3.price as p3 insert into O2;"
                  "from every a=A[price > 0.3] -> b=B[id % 3 == 0] and c=C[price < 0.6] within 5 sec "
                  "select a.k as k, a.id as ai, b.price as bp, c.name as cn insert into O; end;")
    wkey = (20000, 64, 0)
    want, _ = model(plan, wkey)
    got, kl = run(plan, three_streams(*wkey), outs=("O", "O1", "O2"), key_capacity=64)
    assert kl[L.K_MQ_WALK] > 0 and kl[L.K_WALK] > 0, kl      # the group is formed, the logical query walks alone
    for o, least in (("O", 500), ("O1", 10), ("O2", 10)):
        assert len(want[o]) >= least, (o, len(want[o]))
        assert_same_rows(got[o], expected(plan, want[o], o), o)


# ---- the row shuffle ---------------------------------------------------------------------------
def test_row_shuffle_two_worlds():
    import torch
    world = 2
    plan = EV3 + AND_W
    wkey = (20000, 256, 0)
    w = three_streams(*wkey)
    want = expected(plan, model(plan, wkey)[0]["O"])
    sender = make(plan, outs=())
    owners = [make(plan, key_stride=world, key_offset=r, chunk_events=4096) for r in range(world)]
    n = len(w["ts"])
    m = n // (2 * world)
    try:
        for step in range(2):      # two shuffle steps: half-filled partials carry across them
            segs = [[] for _ in range(world)]
            for src in range(world):
                s = (step * world + src) * m
                d = {c: torch.from_numpy(np.ascontiguousarray(w[c][s:s + m])).cuda() for c in COLS + ("stream",)}
                rows, counts = sender.route_rows("A", d["ts"], [d[c] for c in COLS], world, seq0=int(s),
                                                 streams=d["stream"])
                off = np.concatenate([[0], np.cumsum(counts)])
                for r in range(world):
                    segs[r].append(rows[off[r]:off[r + 1]].clone())
            for r in range(world):
                recv = torch.cat(segs[r], dim=0)
                owners[r].send_rows(recv, recv.shape[0], 0)
        got = []
        for o in owners:
            o.flush()
            got += engine_rows(o.collect("O"))
    finally:
        for rt in owners + [sender]:
            rt.shutdown()
    got.sort(key=lambda t: t[1])      # rows of one arrival number come from one owner, in emission order
    assert len(want) > 500
    assert_same_rows(got, want, "row shuffle, world 2")


# ---- query chaining ----------------------------------------------------------------------------
def test_group_side_on_a_derived_stream():
    # a stateless producer folds into its reader by hand (test_gpu_chain.py): B1's filter joins b's condition
    chained = (EV3 + "from B[id % 7 != 0] select k, ts, id, price, name insert into B1;"
               "partition with (k of A, k of B1, k of C) begin "
               "from every a=A[price > 0.3] -> b=B1[id % 3 == 0] and c=C[price < 0.6] within 5 sec" + SEL3)
    twin = EV3 + P3 + ("from every a=A[price > 0.3] -> b=B[id % 7 != 0 and id % 3 == 0] and c=C[price < 0.6] "
                       "within 5 sec" + SEL3)
    wkey = (20000, 256, 0)
    want = expected(twin, model(twin, wkey)[0]["O"])
    got, kl = run(chained, three_streams(*wkey), chunk_events=4096)
    assert kl[L.K_WALK] > 0
    assert len(want) > 300
    assert_same_rows(got["O"], want, "group side on a derived stream")
