"""Regenerates join_itcase.json: the input of SiddhiCEPITCase
testMultipleUnboundedPojoStreamUnionAndJoinWithWindow (SiddhiCEPITCase.java:306-327).

Two RandomEventSource(5) sources (RandomEventSource.java:56-66): id = n % 50
(0..4), name = "test_event", price = Random.nextDouble() (seeded here),
ts = T0 + 1000 n for both sources.  The two sources' rows of one n carry the
same ts, so the operator's priority queue may hand them to Siddhi in either
order: both interleavings are recorded (ties: inputStream1 first /
inputStream2 first).

Expected output: the 5 rows the ITCase counts (:326), written down directly,
not computed by any model: ids are distinct within a source, windows of 5
rows / 500 ms never drop the partner (the partner has the same ts), so row n
of one source joins row n of the other exactly once, whichever arrives
second: {t = T0 + 1000 n, n = "test_event", p1 = inputStream1's price,
p2 = inputStream2's price}.
"""
import json
import random
from pathlib import Path

PLAN = ("define stream inputStream1 (id int, name string, price double, timestamp long);"
        "define stream inputStream2 (id int, name string, price double, timestamp long);"
        "from inputStream1#window.length(5) as s1 "
        "join inputStream2#window.time(500) as s2 "
        "on s1.id == s2.id "
        "select s1.timestamp as t, s1.name as n, s1.price as p1, s2.price as p2 "
        "insert into JoinStream;")
T0 = 1_500_000_000_000
rnd = random.Random(306)
price = {sid: [rnd.random() for _ in range(5)] for sid in ("inputStream1", "inputStream2")}


def events(first, second):
    out = []
    for n in range(5):
        ts = T0 + 1000 * n
        for sid in (first, second):
            out.append([sid, ts, [n % 50, "test_event", price[sid][n], ts]])
    return out


expected = [[T0 + 1000 * n, "test_event", price["inputStream1"][n], price["inputStream2"][n]] for n in range(5)]
out = {"plan": PLAN,
       "events_stream1_first": events("inputStream1", "inputStream2"),
       "events_stream2_first": events("inputStream2", "inputStream1"),
       "expected": expected,
       "source": "SiddhiCEPITCase.java:306-327"}
(Path(__file__).parent / "join_itcase.json").write_text(json.dumps(out, indent=1))
