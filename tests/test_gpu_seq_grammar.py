"""Count-state grammar parity of the three sequence engines.

The sequence grammar (`+ * ? <n> <n:m> <n:> <0:n>`, optional states, Kleene
tails, `every`, `within`, first / last / indexed captures, null captures) is
implemented three times on the device: the stand-alone N-state walk (nfa_key),
the generic multi-query unit (mq_seq: one partial per key, count and bounds
packed in words) and the bit-parallel multi-query unit (mq_seq_bp: one state
per key for a class of queries, an `allow` matrix instead of counts).  Every
shape of tests/seq_ref.gpu_shapes() runs on each engine that takes it, on one
skewed stream (130 keys in three 64-lane blocks, key 0 with 40 % of the rows,
a dozen keys with none, six uneven batches, one of a single row, one ending
inside a count run), bit for bit against the oracle and against the regex
reference; tests/test_seq_ref.py shows from the reference alone that every
shape reaches its maximum, is discarded at max + 1 / below min, skips and
takes its optional states, emits repeatedly from a Kleene tail and expires,
wherever its grammar allows.  The launch counters prove the engine: a plan of
bit-parallel shapes only (min <= 1, max 1 or unbounded: engine.cpp
mq_signature) with K_WALK == 0 ran on mq_seq_bp, a plan of bounded-count
shapes only with K_WALK == 0 on mq_seq, and CEP_NO_MQ=1 with K_MQ_WALK == 0 on
nfa_key.  A never-matched capture is 0 (numeric, bool) or dictionary id -1
(STRING) in an output row (include/cep.h); the oracle's None maps to that.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import flink_siddhi as fs  # noqa: E402
from flink_siddhi import _lib as L  # noqa: E402
import seq_ref as SR  # noqa: E402
from helpers import assert_same_rows, engine_rows, oracle_run  # noqa: E402

NK = 12
NULL_NUMERIC, NULL_STRING = 0, -1      # include/cep.h: a capture of a state that never matched
OPTS = dict(chunk_events=4096, key_capacity=256)


def null_mapped(rows, null=NULL_NUMERIC):
    return [(ts, seq, tuple(null if v is None else v for v in d)) for ts, seq, d in rows]


def run_engine(plan, w, sizes, outs, cols=("k", "ts", "id", "price"), snapshot_after=None, **opts):
    """Host batches of `sizes` rows through one runtime (snapshot_after = i:
    snapshot after batch i, restore into a fresh runtime) -> ({out: rows}, launches)."""
    def make():
        r = fs.SiddhiAppRuntime(plan, **opts)
        for o in outs:
            r.add_callback(o)
        return r
    got, kl, first = {o: [] for o in outs}, [0] * NK, 0
    rt = make()

    def drain():
        for o in outs:
            got[o] += engine_rows(rt.collect(o))
        st = rt.stats()
        for i in range(NK):
            kl[i] += st.kernel_launches[i]
    try:
        for i, n in enumerate(sizes):
            s, e = first, first + n
            rt.send("A", w["ts"][s:e], [w[c][s:e] for c in cols], streams=w["stream"][s:e])
            rt.flush()
            first = e
            if i == snapshot_after:
                drain()
                snap = rt.snapshot()
                rt.shutdown()
                rt = make()
                rt.restore(snap)
        drain()
    finally:
        rt.shutdown()
    return got, kl


# ---- the plans ----------------------------------------------------------------
def plans():
    """name -> shapes.  `bp`: the bit-parallel shapes, the two- and three-state
    ones a second time with the other thresholds (a class of two queries);
    `bounded0` / `bounded1`: the shapes with a bounded or a <2:> count."""
    shapes = SR.gpu_shapes()
    bp = [s for s in shapes if SR.is_bit_parallel(s)]
    bp += [s._replace(alt=True) for s in bp if len(s.quants) <= 2 and s.every and s.within is not None]
    rest = [s for s in shapes if not SR.is_bit_parallel(s)]
    out = {"bp": bp, "bounded0": rest[0::2], "bounded1": rest[1::2]}
    assert sum(len(v) for v in out.values()) == 120 + 20 and max(len(v) for v in out.values()) <= 64
    return out


PLANS = plans()
_want = {}


def wanted(plan_name):
    """(plan text, outs, oracle rows per out) of a plan on the GPU stream, once."""
    if plan_name not in _want:
        shapes = PLANS[plan_name]
        text = SR.plan_text(shapes)
        _want[plan_name] = (text, ["O%d" % i for i in range(len(shapes))], oracle_run(text, SR.events(SR.gpu_stream())))
    return _want[plan_name]


def run_plan(plan_name, path, monkeypatch, snapshot=False):
    shapes = PLANS[plan_name]
    text, outs, want = wanted(plan_name)
    opts = dict(OPTS)
    if path == "walk":
        monkeypatch.setenv("CEP_NO_MQ", "1")
        opts["pending_slots"] = 16
    else:
        monkeypatch.delenv("CEP_NO_MQ", raising=False)
    got, kl = run_engine(text, SR.gpu_stream(), SR.gpu_batches(), outs,
                         snapshot_after=SR.SNAPSHOT_AFTER if snapshot else None, **opts)
    if path == "walk":
        assert kl[L.K_WALK] > 0 and kl[L.K_MQ_WALK] == 0, kl
    else:
        assert kl[L.K_MQ_WALK] > 0 and kl[L.K_WALK] == 0, kl
    total = 0
    for i, sh in enumerate(shapes):
        ctx = "%s on %s (%s)" % (SR.name(sh), path, outs[i])
        ref, cn = SR.gpu_reference(sh)
        assert len(ref) > 0, ctx
        assert_same_rows(got[outs[i]], null_mapped(want.get(outs[i], [])), ctx + " vs oracle")
        assert_same_rows(got[outs[i]], null_mapped(ref), ctx + " vs reference")
        total += len(ref)
    print("%s on %s: %d shapes, %d rows" % (plan_name, path, len(shapes), total))


@pytest.mark.parametrize("plan_name", list(PLANS))
def test_multi_query_units(plan_name, monkeypatch):
    """bp: every query on mq_seq_bp; bounded0 / bounded1: every query on mq_seq."""
    for sh in PLANS[plan_name]:
        assert SR.is_bit_parallel(sh) == (plan_name == "bp")
    run_plan(plan_name, "mq", monkeypatch)


@pytest.mark.parametrize("plan_name", list(PLANS))
def test_stand_alone_walk(plan_name, monkeypatch):
    run_plan(plan_name, "walk", monkeypatch)


@pytest.mark.parametrize("plan_name,path", [("bp", "mq"), ("bounded0", "mq"), ("bounded1", "walk")])
def test_snapshot_inside_a_count_run(plan_name, path, monkeypatch):
    run_plan(plan_name, path, monkeypatch, snapshot=True)


# ---- stand-alone only: outside the disjoint-stream subset (oracle alone) -----------------
W6 = " within 6 milliseconds "
ALONE = [
    # sK[1] captures
    "from every s1=A[id < 8], s2=B[id < 7]+, s3=C[id < 8]" + W6 +
    "select s1.k as k, s2[1].id as b1, s2[last].id as bl, s3.id as c insert into O0;",
    "from every s1=A[id < 8], s2=B[id < 7]<2:3>, s3=C[id < 8]?" + W6 +
    "select s1.k as k, s2[0].id as b0, s2[1].id as b1, s3[1].id as c1 insert into O1;",
    "from every s1=A[id < 8], s2=B[id < 7]*, s3=C[id < 8]<2:> "
    "select s1.k as k, s2[1].id as b1, s3[1].id as c1, s3[last].id as cl insert into O2;",
    # conditions that read captures
    "from every s1=A[id < 8], s2=B[id >= s1.id]+, s3=C[id != s2[last].id]" + W6 +
    "select s1.k as k, s1.id as a, s2.id as b0, s2[last].id as bl, s3.id as c insert into O3;",
    # the start stream again as a later state: several partials per key
    "from every s1=A, s2=B[id < 7]+, s3=C[id < 8]?, s4=A[id > 4]" + W6 +
    "select s1.k as k, s1.id as a, s2[last].id as bl, s3.id as c, s4.id as d insert into O4;",
    # one stream in two adjacent states
    "from every s1=A[id < 8], s2=B[id < 5]+, s3=B[id >= 5]" + W6 +
    "select s1.k as k, s2.id as b0, s2[last].id as bl, s3.id as c insert into O5;",
    # a counted start state
    "from every s1=A[id < 8]<2:>, s2=B[id < 7]?" + W6 +
    "select s1.k as k, s1[0].id as a0, s1[1].id as a1, s1[last].id as al, s2.id as b insert into O6;",
    "from every s1=A[id < 8]+, s2=B[id < 7]" + W6 +
    "select s1.k as k, s1[0].id as a0, s1[last].id as al, s2.id as b insert into O7;",
]


def test_stand_alone_only_shapes(monkeypatch):
    monkeypatch.setenv("CEP_NO_MQ", "1")
    plan = SR.DEFS + SR.PARTITION + "".join(ALONE) + " end;"
    outs = ["O%d" % i for i in range(len(ALONE))]
    w = SR.gpu_stream()
    want = oracle_run(plan, SR.events(w))
    got, kl = run_engine(plan, w, SR.gpu_batches(), outs, pending_slots=16, **OPTS)
    assert kl[L.K_WALK] > 0 and kl[L.K_MQ_WALK] == 0, kl
    for o in outs:
        rows = want.get(o, [])
        assert len(rows) > 20, o
        assert_same_rows(got[o], null_mapped(rows), o)
    # the indexed captures are both present and absent, the later A state keeps two partials
    assert {r[2][1] is None for r in want["O0"]} == {True, False}
    assert {r[2][3] is None for r in want["O1"]} == {True}          # C? never has a second event
    assert {r[2][2] is None for r in want["O1"]} == {False}
    assert {r[2][1] is None for r in want["O2"]} == {True, False}
    assert any(r[2][3] is None for r in want["O4"]) and any(r[2][3] is not None for r in want["O4"])


# ---- count limits: the 8-bit count fields of the generic unit -----------------------------
RUNS = (253, 254, 255, 256)


def limit_stream():
    """One key: A, a run of B rows, C for every run length; 1 ms apart."""
    st = []
    for n in RUNS:
        st += [0] + [1] * n + [2]
    n = len(st)
    return {"k": np.full(n, 3, np.int32), "ts": 5_000 + np.arange(n, dtype=np.int64),
            "id": (np.arange(n) % 7).astype(np.int32), "price": np.full(n, 0.5), "stream": np.array(st, np.uint8)}


def limit_query(quant, out):
    return ("from every s1=A, s2=B%s, s3=C select s1.k as k, s1.ts as t1, s2[last].ts as tl, s3.ts as t3 "
            "insert into %s;" % (quant, out))


@pytest.mark.parametrize("path", ["mq", "walk"])
def test_count_limits(path, monkeypatch):
    """<254> and <2:254> fit the generic unit's 8-bit fields (0xff: unbounded)
    and stay in the group; <255> leaves it for the stand-alone walk; `+`
    matches all four runs on both."""
    monkeypatch.delenv("CEP_NO_MQ", raising=False)
    quants = ("<254>", "<2:254>", "+") if path == "mq" else ("<255>", "+")
    outs = ["O%d" % i for i in range(len(quants))]
    plan = SR.DEFS + SR.PARTITION + "".join(limit_query(q, o) for q, o in zip(quants, outs)) + " end;"
    w = limit_stream()
    n = len(w["ts"])
    want = oracle_run(plan, SR.events(w))
    got, kl = run_engine(plan, w, (400, n - 400), outs, pending_slots=16, **OPTS)
    if path == "mq":
        assert kl[L.K_MQ_WALK] > 0 and kl[L.K_WALK] == 0, kl
    else:
        assert kl[L.K_WALK] > 0, kl
    matched = {"<254>": [254], "<2:254>": [253, 254], "<255>": [255], "+": list(RUNS)}
    for q, o in zip(quants, outs):
        assert [r[2][2] - r[2][1] for r in want[o]] == matched[q], q       # last B - A = the run length
        assert_same_rows(got[o], want[o], "B%s on %s" % (q, path))


# ---- null captures ---------------------------------------------------------------------------
NAMED = "".join("define stream %s (k int, ts long, id int, name string);" % s for s in "ABC")
NAMES = ("zero", "one", "two", "three")


def test_null_captures_of_a_skipped_state(monkeypatch):
    """`A, B?, C` selecting s2.name and s2.id: rows that skipped B carry
    dictionary id -1 and 0, from a plan that forms a multi-query group and
    with CEP_NO_MQ=1.  (Dictionary id 0 is a real string, and it is what the
    group's units gave while they took such queries: they clear a new
    partial's captures to 0.  mq_candidate now leaves a query with a STRING
    capture of an optional state to the stand-alone walk; O4's STRING captures
    of states no match skips stay in the group with O2 and O3.)"""
    plan = (NAMED + "partition with (k of A, k of B, k of C) begin "
            "from every s1=A[id < 8], s2=B[id < 7]?, s3=C[id < 8] within 6 milliseconds "
            "select s1.k as k, s2.name as n, s2.id as i, s3.id as c insert into O0;"
            "from every s1=A[id < 8], s2=B[id < 7]*, s3=C[id < 8] within 6 milliseconds "
            "select s1.k as k, s2[last].name as n, s2.id as i, s3.name as c insert into O1;"
            "from every s1=A[id < 8], s2=B[id < 7]+, s3=C[id < 8] within 6 milliseconds "
            "select s1.k as k, s2[last].id as i, s3.id as c insert into O2;"
            "from every s1=A[id < 8], s2=B[id < 7]?, s3=C[id < 8] within 6 milliseconds "
            "select s1.k as k, s2.id as i, s3.id as c insert into O3;"
            "from every s1=A[id < 8], s2=B[id < 7]+, s3=C[id < 8] within 6 milliseconds "
            "select s1.k as k, s2[last].name as n, s2.id as i, s3.name as c insert into O4;"
            " end;")
    outs = ["O0", "O1", "O2", "O3", "O4"]
    w = SR.make_stream(3000, 40, 7, streams=3)
    names = np.array(NAMES)[(w["id"] + w["k"]) % len(NAMES)]
    ev = [("ABC"[s], t, (k, t, i, nm)) for k, t, i, nm, s in
          zip(w["k"].tolist(), w["ts"].tolist(), w["id"].tolist(), names.tolist(), w["stream"].tolist())]
    want = oracle_run(plan, ev)
    assert {r[2][1] is None for r in want["O0"]} == {True, False} and {r[2][1] is None for r in want["O1"]} == {True, False}
    assert any(r[2][1] == NAMES[0] for r in want["O0"])
    for path in ("mq", "walk"):
        if path == "walk":
            monkeypatch.setenv("CEP_NO_MQ", "1")
        else:
            monkeypatch.delenv("CEP_NO_MQ", raising=False)
        rt = fs.SiddhiAppRuntime(plan, pending_slots=16, **OPTS)
        try:
            ids = {nm: rt.intern(nm) for nm in NAMES}
            assert ids[NAMES[0]] == 0
            for o in outs:
                rt.add_callback(o)
            w["name"] = np.array([ids[nm] for nm in names.tolist()], np.int32)
            half = 1234
            for s, e in ((0, half), (half, len(names))):
                rt.send("A", w["ts"][s:e], [w[c][s:e] for c in ("k", "ts", "id", "name")], streams=w["stream"][s:e])
                rt.flush()
            got = {o: engine_rows(rt.collect(o)) for o in outs}
            kl = list(rt.stats().kernel_launches)
        finally:
            rt.shutdown()
        # the queries without a STRING capture of an optional state form the group
        assert (kl[L.K_MQ_WALK] > 0) == (path == "mq") and kl[L.K_WALK] > 0, kl
        for o in outs:
            rows = [(ts, seq, tuple(NULL_NUMERIC if v is None else v for v in d)) for ts, seq, d in want[o]]
            if o in ("O0", "O1", "O4"):     # column 1 is the string: None -> id -1, a name -> its id
                rows = [(ts, seq, (d[0], NULL_STRING if x[1] is None else ids[x[1]]) + d[2:])
                        for (ts, seq, d), (_, _, x) in zip(rows, want[o])]
            if o in ("O1", "O4"):
                rows = [(ts, seq, d[:3] + (ids[d[3]],)) for ts, seq, d in rows]
            assert len(rows) > 50, o
            assert_same_rows(got[o], rows, "%s on %s" % (o, path))
