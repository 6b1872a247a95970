"""The apps behind the snapshot fixtures under tests/golden/snapshots/, shared by
scripts/make_snapshot_fixtures.py (which writes the fixtures with the library
of the commit before a change) and tests/test_gpu_snapshot_compat.py (which
reads them with the current one).  One app per kind of snapshot state; every
app runs a deterministic stream in the smallest chunks the engine takes, so
the general partition / walk path (2048-row chunks), the join (1024) and the
table run more than one chunk before the snapshot is taken at row `split`; the
closed form (8192) and the multi-query group (16384) cannot within 4000 rows,
so every app is fed in batches of 700 rows, which cycle the chunk arenas too."""
import numpy as np

import flink_siddhi as fs
from flink_siddhi import workload
from helpers import engine_rows, oracle_run, workload_events
import config5_cases as C5

EV2 = ("define stream A (k int, ts long, id int, price double);"
       "define stream B (k int, ts long, id int, price double);")
P3 = "partition with (k of A, k of B, k of C) begin "
TABLE = ("@PrimaryKey('k') define table T (k int, id int, price double);"
         "from A[id % 3 == 0] select k, id, price update or insert into T on T.k == k;"
         "from T as t join B as b on b.k == t.k and b.price > t.price "
         "select b.k as k, b.price - t.price as d, t.id + b.id as n insert into O;")
MQ4 = (C5.EV3 + P3 +
       "from every s1=A[price > 0.0], s2=B[id % 10 == 0]+, s3=C[id % 10 == 1] within 10 sec "
       "select s1.k as k, s1.price as p1, s2[last].price as p2, s3.ts as t3 insert into Seq0;"
       "from every s1=A[price > 0.015625], s2=B[id % 10 == 1]+, s3=C[id % 10 == 2] within 10 sec "
       "select s1.k as k, s1.price as p1, s2[last].price as p2, s3.ts as t3 insert into Seq1; end;"
       "from A[id >= 0] select k, sum(price) as total, count() as n group by k having total > 6.0 insert into Agg0;"
       "from B[id >= 1] select k, sum(price) as total, count() as n group by k having total > 6.125 insert into Agg1;")

# name -> plan, runtime options, stream (n rows, keys), split row, outputs, reference
CASES = {
    # closed form: keys holding more than pending_slots partials (overflow
    # runs) and 200 rows still waiting for a watermark at the snapshot
    "cf_overflow_reorder": dict(plan=workload.PATTERN_PLAN, opts=dict(ts_order=1, pending_slots=2, key_capacity=64,
                                                                      buckets_log2=3, chunk_events=1),
                                n=2000, keys=24, split=1200, held=200, outs=["O"], ref="oracle"),
    "nfa3": dict(plan=C5.EV3 + P3 + "from every s1=A[price > 0.1] -> s2=B[id % 4 == 0] -> s3=C[id % 211 == 0] "
                 "within 1 sec select s1.k as k, s1.price as p1, s2.id as i2, s3.ts as t3 insert into O; end;",
                 opts=dict(pending_slots=16, key_capacity=64, chunk_events=1), n=4000, keys=16, split=2500,
                 streams=3, outs=["O"], ref="oracle"),
    "sparse": dict(plan=workload.PATTERN_PLAN.replace("(k int,", "(k long,"),
                   opts=dict(ts_order=1, sparse_keys=1, key_capacity=256, chunk_events=1),
                   n=2000, keys=100, split=1100, long_keys=True, outs=["O"], ref="oracle"),
    "mq4": dict(plan=MQ4, opts=dict(key_capacity=64, chunk_events=1), n=3000, keys=48, split=1517, streams=3,
                outs=["Seq0", "Seq1", "Agg0", "Agg1"], ref="oracle"),
    "win_length": dict(plan=EV2 + "partition with (k of A) begin from A#window.length(5) select k, sum(price) as s, "
                       "min(id) as mn, count() as c having s > 3.5 insert into O; end;",
                       opts=dict(key_capacity=256, chunk_events=1), n=4000, keys=64, split=2300, outs=["O"],
                       ref="window"),
    "win_time": dict(plan=EV2 + "partition with (k of A) begin from A#window.time(60) select k, sum(price) as s, "
                     "max(id) as mx, count() as c having s > 3.6 insert into O; end;",
                     opts=dict(key_capacity=64, pending_slots=32, chunk_events=1), n=4000, keys=8, split=2300,
                     outs=["O"], ref="window"),
    "join": dict(plan=EV2 + "from A#window.length(5) as a join B#window.time(200) as b on a.k == b.k "
                 "select a.id as x, b.price as p, a.price - b.price as d insert into O;",
                 opts=dict(ts_order=1, chunk_events=1), n=2600, keys=512, split=1300, outs=["O"], ref="join"),
    "table": dict(plan=EV2 + TABLE, opts=dict(key_capacity=256, buckets_log2=3, chunk_events=1),
                  n=4000, keys=256, split=2500, outs=["O"], ref="table"),
}


def stream(case):
    c = CASES[case]
    if c.get("streams") == 3:
        return C5.three_streams(c["n"], c["keys"])
    w = workload.generate(0, c["n"], c["keys"], rate=1)
    if c.get("long_keys"):
        vals = np.random.default_rng(7).integers(-(1 << 63), (1 << 63) - 1, c["keys"], dtype=np.int64)
        vals[:3] = [-1, 0, np.iinfo(np.int64).min]
        w["k"] = vals[w["k"]]
    return w


def reference(case):
    """{output: rows} of the whole stream, from the oracle or the naive model of the app's kind."""
    c = CASES[case]
    w = stream(case)
    ev = C5.events(w) if c.get("streams") == 3 else workload_events(w)
    if c["ref"] == "oracle":
        return oracle_run(c["plan"], ev)
    mod = __import__(c["ref"] + "_model")
    return mod.model_run(c["plan"], ev)[0]


def runtime(case):
    c = CASES[case]
    rt = fs.SiddhiAppRuntime(c["plan"], **c["opts"])
    for o in c["outs"]:
        rt.add_callback(o)
    return rt


def feed(rt, case, w, s, e, last):
    """Rows [s, e) of the stream -> {output: rows}.  A case with `held` rows goes
    through the reorder buffer; its last `held` rows stay there unless `last`."""
    c = CASES[case]
    for b in range(s, e, 700):
        t = min(b + 700, e)
        cols = [w["k"][b:t], w["ts"][b:t], w["id"][b:t], w["price"][b:t]]
        (rt.process_elements if "held" in c else rt.send)("A", w["ts"][b:t], cols, streams=w["stream"][b:t])
    if "held" in c:
        rt.process_watermark(int(w["ts"][e - 1] if last else w["ts"][e - 1 - c["held"]]))
    rt.flush()
    return {o: engine_rows(rt.collect(o)) for o in c["outs"]}


def first_part(case):
    """-> (snapshot bytes at the split, {output: rows} emitted before it)."""
    rt = runtime(case)
    rows = feed(rt, case, stream(case), 0, CASES[case]["split"], False)
    snap = rt.snapshot()
    rt.shutdown()
    return snap, rows
