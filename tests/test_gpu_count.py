"""Count states in patterns on the device (`A -> B<m:n> -> C`: the third
instance of nfa_key) against tests/count_model.py, row for row and
bit for bit: ts, arrival number, data.  The three-stream workload of
test_gpu_logic.py with a STRING column; an index never collected is 0
(numeric) or dictionary id -1 (STRING) in an output row (include/cep.h).

No case passes vacuously: on the model's side every case has rows, has a row
whose b[last] is not its b[0], and differs from the same plan with every count
replaced by `<1>`.  Each model runs once per (plan, input) and is shared."""
import re

import numpy as np
import pytest

import flink_siddhi as fs
from flink_siddhi import _lib as L
from flink_siddhi import workload
from helpers import assert_same_rows, engine_rows
from count_model import CountModel, model_run

pytestmark = pytest.mark.gpu

EV3 = "".join("define stream %s (k int, ts long, id int, price double, name string);" % s for s in "ABC")
STREAMS = ("A", "B", "C")
NAMES = ("zero", "one", "two", "three")
COLS = ("k", "ts", "id", "price", "name")
NULL_NUMERIC, NULL_STRING = 0, -1      # include/cep.h: an index of a count state never collected
P3 = "partition with (k of A, k of B, k of C) begin "
COUNT = re.compile(r"<\d+(:\d*)?>")

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


def run(plan, w, outs=("O",), cuts=None, **opts):
    rt = make(plan, outs, **opts)
    cuts = [0, len(w["ts"])] if cuts is None else cuts
    try:
        for s, e in zip(cuts[:-1], cuts[1:]):
            send(rt, w, s, e)
        got = {o: engine_rows(rt.collect(o)) for o in outs}
        kl = list(rt.stats().kernel_launches)
    finally:
        rt.shutdown()
    return got, kl


def not_vacuous(plan, wkey, rows, first=2, last=3):
    """The three checks of the module's docstring, on the model's rows;
    `first` / `last`: the columns that hold b[0].id and b[last].id."""
    assert len(rows) > 0
    assert any(d[last] != d[first] for _, _, d in rows)
    ones = COUNT.sub("<1>", plan)
    assert ones != plan and model(ones, wkey)[0].get("O", []) != rows


def case(query, min_rows, wkey=(20000, 256, 0), first=2, last=3, **kw):
    plan = EV3 + query
    want, m = model(plan, wkey)
    assert len(want.get("O", [])) >= min_rows, len(want.get("O", []))
    not_vacuous(plan, wkey, want["O"], first, last)
    got, kl = run(plan, three_streams(*wkey), **kw)
    assert kl[L.K_WALK] > 0 and kl[L.K_MQ_WALK] == 0 and kl[L.K_CF_WALK] == 0, kl
    assert_same_rows(got["O"], expected(plan, want["O"]), query)
    return want["O"], m


def mid_count_at(plan, w, cut):
    """Partials that sit in a count state with more to collect after the first `cut` events."""
    m = CountModel(plan)
    for sid, ts, row in events(w)[:cut]:
        m.send(sid, ts, row)
    return m.mid_count()


# columns 2, 3: b[0].id, b[last].id
SELB = " select a.k as k, a.id as ai, b[0].id as b0, b[last].id as bl, b[1].id as b1, b[last].name as bn"
SELM = SELB + ", c.price as cp, c.ts as ct insert into O; end;"
MID = P3 + "from every a=A[price > 0.3] -> b=B[id % 3 != 0]<2:4> -> c=C[price < 0.6] within 5 sec" + SELM
LAST = P3 + "from every a=A[price > 0.3] -> c=C[price < 0.6] -> b=B[id % 3 != 0]<3:5> within 8 sec" + SELM
PAIR = P3 + "from every a=A[price > 0.3] -> b=B[id % 3 != 0]<2:3> within 5 sec" + SELB + " insert into O; end;"
OPEN = P3 + "from every a=A[price > 0.3] -> b=B[id % 3 != 0]<2:> -> c=C[price < 0.3] within 6 sec" + SELM


# ---- where the count state stands --------------------------------------------------------------
@pytest.mark.parametrize("ts_order", [0, 1])
def test_count_in_the_middle(ts_order):
    rows, m = case(MID, 500, ts_order=ts_order)
    assert m.stat("appended_past_min") > 500 and m.stat("shared_seen") > 500
    assert any(d[4] is not None and d[4] != d[3] for _, _, d in rows)       # b[1] is not b[last]
    # some partials expired: the same plan without `within` matches more
    assert len(rows) < len(model(EV3 + MID.replace(" within 5 sec", ""), (20000, 256, 0))[0]["O"])


def test_count_in_last_position():
    rows, _ = case(LAST, 300)
    w = three_streams()
    assert len(rows) <= ((w["stream"] == 0) & (w["price"] > 0.3)).sum()      # at most one row per start: it emits once


def test_two_positions():
    case(PAIR, 500)


def test_unbounded_count():
    rows, m = case(OPEN, 300)
    assert m.stat("appended_past_min") > 500


def test_two_consecutive_counts_in_six_states():
    case(P3 + "from every a=A[price > 0.5] -> b=B<2:3> -> c=C<1:2> -> d=A[id > 10] -> e=B[price > b[last].price] -> f=C "
         "within 20 sec select a.k as k, a.id as ai, b[0].id as b0, b[last].id as bl, c[last].name as cn, "
         "d.id as di, f.ts as ft insert into O; end;", 100, wkey=(20000, 64, 0))


def test_count_and_next_state_on_one_stream():
    rows, m = case(P3 + "from every a=A[price > 0.3] -> b=B[id % 3 != 0]<2:4> -> c=B[price < 0.3] within 5 sec" +
                   SELB + ", c.id as ci, c.ts as ct insert into O; end;", 300)
    # some closing B's passed b's condition too while b could still collect
    # (b[2] was free): the next state had them first
    assert any(d[6] % 3 != 0 and d[3] == d[4] for _, _, d in rows)


# ---- conditions in the walk's interpreter and in the partition pass ----------------------------
def test_condition_reading_its_own_last():
    # ids are positive, so a never-collected b[last].id (0 on the device, None
    # in the model) fails `>= id` on both sides; collected ids rise strictly
    rows, _ = case(P3 + "from every a=A[price > 0.2] -> b=B[id > a.id and not (b[last].id >= id)]<2:4> -> "
                   "c=C[price > a.price - 0.5 and id != b[1].id] within 6 sec" + SELM, 200)
    assert all(d[2] < d[3] for _, _, d in rows)


def test_conditions_over_the_events_own_columns():
    case(P3 + "from every a=A[id > 5] -> b=B[id % 2 == 0 and price > 0.1]<2:3> -> c=C[id < 45] within 6 sec" + SELM, 300)
    case(P3 + "from every a=A -> b=B<3:4> -> c=C within 3 sec" + SELM, 300)


# ---- non-`every`, unpartitioned ----------------------------------------------------------------
def test_non_every_and_unpartitioned():
    sel = SELB + ", c.ts as ct insert into O;"
    rows, _ = case("from a=A[id == 3] -> b=B[id > 40]<2:3> -> c=C[id == 5]" + sel, 1, wkey=(20000, 16, 0))
    assert len(rows) == 1
    # `every`, one list for the whole stream
    case("from every a=A[id == 3] -> b=B[id > 40]<2:4> -> c=C[id < 9] within 50 milliseconds" + sel, 50,
         wkey=(20000, 16, 0))
    # non-`every` under a partition: one match per key
    rows, _ = case(P3 + "from a=A -> b=B[id > a.id]<2:3> -> c=C" + SELM, 200)
    assert len(rows) == len({d[0] for _, _, d in rows})


# ---- lists longer than pending_slots -----------------------------------------------------------
PLONG = (P3 + "from every a=A[price > 0.1] -> b=B[id % 4 != 0]<2:6> -> c=C[id % 211 == 0] within 10 sec "
         "select a.k as k, a.price as ap, b[0].id as b0, b[last].id as bl, c.ts as ct, b[1].name as bn insert into O; end;")


@pytest.mark.parametrize("batches,chunk", [(1, 1 << 22), (4, 4096)])
def test_pending_lists_beyond_slots(batches, chunk):
    # 16 keys at 1 event/ms: every key keeps far more live partials than its 16
    # inline slots, most of them between min and max (the closing c is rare);
    # the rest live in the pending pool across windows, chunks and batches
    wkey = (40000, 16, 0)
    cuts = np.linspace(0, wkey[0], batches + 1).astype(int).tolist()
    rows, m = case(PLONG, 1000, wkey=wkey, cuts=cuts, pending_slots=16, chunk_events=chunk)
    assert m.stat("max_live") >= 40 and m.stat("appended_past_min") > 1000


# ---- chunks and batches ------------------------------------------------------------------------
def test_chunks_and_batches_cut_in_the_middle_of_a_count():
    w = three_streams()
    cuts = [0, 6001, 13337, len(w["ts"])]
    for cut in cuts[1:-1]:
        assert mid_count_at(EV3 + MID, w, cut) > 50
    case(MID, 500, cuts=cuts, chunk_events=4096)
    case(OPEN, 300, cuts=cuts, chunk_events=4096)


# ---- snapshot / restore ------------------------------------------------------------------------
def test_snapshot_in_the_middle_of_a_count_restores_and_continues():
    w = three_streams()
    plan = EV3 + MID
    want, _ = model(plan, (20000, 256, 0))
    not_vacuous(plan, (20000, 256, 0), want["O"])
    half = 9973
    assert mid_count_at(plan, w, half) > 50
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
    assert_same_rows(first + second, expected(plan, want["O"]), "snapshot in the middle of a count")
    # <2:4> is not <2:5>: the plans differ in st_max only
    rt3 = make(EV3 + MID.replace("<2:4>", "<2:5>"), chunk_events=4096)
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
    case(MID, 300, wkey=wkey, ts_order=0, chunk_events=4096)
    case(LAST, 200, wkey=wkey, ts_order=0, chunk_events=4096)


# ---- beside a multi-query group ----------------------------------------------------------------
def test_count_pattern_beside_a_multi_query_group():
    plan = EV3 + (P3 +
                  "from every s1=A[price > 0.5], s2=B[id < 30]+, s3=C[id > 20] within 10 sec "
                  "select s1.k as k, s1.price as p1, s2[last].price as p2, s3.price as p3 insert into O1;"
                  "from every s1=A[price > 0.25], s2=B[id < 25]+, s3=C[id > 10] within 10 sec "
                  "select s1.k as k, s1.price as p1, s2[last].price as p2, s3.price as p3 insert into O2;"
                  "from every a=A[price > 0.3] -> b=B[id % 3 != 0]<2:4> -> c=C[price < 0.6] within 5 sec" +
                  SELB + ", c.name as cn insert into O; end;")
    wkey = (20000, 64, 0)
    want, _ = model(plan, wkey)
    # (the sequences' `+` is no `<m:n>`: COUNT rewrites the pattern's count only)
    not_vacuous(plan, wkey, want["O"])
    got, kl = run(plan, three_streams(*wkey), outs=("O", "O1", "O2"), key_capacity=64)
    assert kl[L.K_MQ_WALK] > 0 and kl[L.K_WALK] > 0, kl      # the group is formed, the count pattern walks alone
    for o, least in (("O", 500), ("O1", 10), ("O2", 10)):
        assert len(want[o]) >= least, (o, len(want[o]))
        assert_same_rows(got[o], expected(plan, want[o], o), o)


# ---- the row shuffle ---------------------------------------------------------------------------
def test_row_shuffle_two_worlds():
    import torch
    world = 2
    plan = EV3 + MID
    wkey = (20000, 256, 0)
    w = three_streams(*wkey)
    rows = model(plan, wkey)[0]["O"]
    not_vacuous(plan, wkey, rows)
    want = expected(plan, rows)
    sender = make(plan, outs=())
    owners = [make(plan, key_stride=world, key_offset=r, chunk_events=4096) for r in range(world)]
    n = len(w["ts"])
    m = n // (2 * world)
    try:
        for step in range(2):      # two shuffle steps: counts carry across them
            segs = [[] for _ in range(world)]
            for src in range(world):
                s = (step * world + src) * m
                d = {c: torch.from_numpy(np.ascontiguousarray(w[c][s:s + m])).cuda() for c in COLS + ("stream",)}
                rws, counts = sender.route_rows("A", d["ts"], [d[c] for c in COLS], world, seq0=int(s),
                                                streams=d["stream"])
                off = np.concatenate([[0], np.cumsum(counts)])
                for r in range(world):
                    segs[r].append(rws[off[r]:off[r + 1]].clone())
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
def test_count_state_on_a_derived_stream():
    # a stateless producer folds into its reader by hand (test_gpu_chain.py): B1's filter joins b's condition
    chained = (EV3 + "from B[id % 7 != 0] select k, ts, id, price, name insert into B1;"
               "partition with (k of A, k of B1, k of C) begin "
               "from every a=A[price > 0.3] -> b=B1[id % 3 != 0]<2:4> -> c=C[price < 0.6] within 5 sec" + SELM)
    twin = EV3 + P3 + ("from every a=A[price > 0.3] -> b=B[id % 7 != 0 and id % 3 != 0]<2:4> -> c=C[price < 0.6] "
                       "within 5 sec" + SELM)
    wkey = (20000, 256, 0)
    rows = model(twin, wkey)[0]["O"]
    not_vacuous(twin, wkey, rows)
    want = expected(twin, rows)
    got, kl = run(chained, three_streams(*wkey), chunk_events=4096)
    assert kl[L.K_WALK] > 0
    assert len(want) > 300
    assert_same_rows(got["O"], want, "count state on a derived stream")
