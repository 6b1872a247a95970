"""Sliding-window aggregates against the engine's own cumulative group-by:
the same partitioned query with no window (the yardstick: a strict subset of
the work, code this change does not touch), with `#window.length(5)` and with
`#window.time(T)`, T chosen from the generator's rate and key count so that a
key holds about 5 rows.  Device-resident generator input, 2^20 keys, default
chunks; one warm-up step (it also fills the windows), then timed steps.
Prints one JSON line per plan: events/s over the timed steps and the mean
time per launch of every kernel kind that ran (profile option: HIP events
around each launch; a chunk is one launch of each).

usage: python scripts/window_bench.py [log2 events per step] [steps]"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "flink-siddhi_amd"))
import torch  # noqa: E402

import flink_siddhi as fs  # noqa: E402
from flink_siddhi import workload  # noqa: E402

n = 1 << (int(sys.argv[1]) if len(sys.argv) > 1 else 24)
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 3
keys = 1 << 20
rate = 400                                   # rows per ms over both streams; half of them are A's
T = 5 * 2 * keys // rate                     # ms in which a key sees about 5 A rows
EV2 = ("define stream A (k int, ts long, id int, price double);"
       "define stream B (k int, ts long, id int, price double);")
QUERY = ("partition with (k of A) begin from A%s select k, sum(price) as s, avg(price) as a, count() as c "
         "insert into O; end;")
PLANS = [("group_by", ""), ("window_length_5", "#window.length(5)"), ("window_time", "#window.time(%d)" % T)]
KINDS = {0: "filter", 1: "partition", 2: "walk", 5: "agg", 6: "other", 10: "mq_partition", 11: "mq_walk"}

batches = []
for s in range(steps + 1):   # consecutive stream slices (ts ascending across steps)
    d = workload.generate_device(s * n, n, keys, rate=rate)
    batches.append((d, [d["k"], d["ts"], d["id"], d["price"]]))
torch.cuda.synchronize()

for name, clause in PLANS:
    # 32 ring entries: a key's occupancy is about Poisson(5)
    rt = fs.SiddhiAppRuntime(EV2 + QUERY % clause, ts_order=1, ordered_output=0, omit_seq=1, profile=1,
                             key_capacity=keys, pending_slots=32 if "time" in clause else 16)
    for s in range(steps + 1):
        if s == 1:
            torch.cuda.synchronize()
            st0 = rt.stats()
            t0 = time.perf_counter()
        d, cols = batches[s]
        rt.send("A", d["ts"], cols, streams=d["stream"])
        rt.flush()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    st1 = rt.stats()
    res = {"plan": name, "clause": clause, "events_per_step": n, "steps": steps, "keys": keys,
           "events_per_s": round(n * steps / dt), "us_per_launch": {}, "launches": {}}
    for k, kn in KINDS.items():
        timed = st1.kernel_timed[k] - st0.kernel_timed[k]
        if timed:
            res["us_per_launch"][kn] = round(1e3 * (st1.kernel_ms[k] - st0.kernel_ms[k]) / timed, 1)
            res["launches"][kn] = int(st1.kernel_launches[k] - st0.kernel_launches[k])
    rt.shutdown()
    print(json.dumps(res), flush=True)
