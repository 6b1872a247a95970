"""Tumbling-window aggregates against the sliding window they sit beside: the
same partitioned query with `#window.lengthBatch(5)`, with
`#window.externalTimeBatch(ts, T)`, T chosen from the generator's rate and key
count so that a batch holds about 5 rows, and, as the yardstick, with the
existing `#window.length(5)`.  Device-resident generator input, 2^20 keys,
default chunks; one warm-up step (it also opens every key's first batch), then
timed steps.  Every case runs in a child process of its own under its own time
limit (the parent never opens the GPU).  Prints one JSON line per plan:
events/s over the timed steps and the mean time per launch of
every kernel kind that ran (profile option: HIP events around each launch; a
chunk is one launch of each).

usage: python scripts/batch_window_bench.py [log2 events per step] [steps]"""
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
keys = 1 << 20
rate = 400                                   # rows per ms over both streams; half of them are A's
T = 5 * 2 * keys // rate                     # ms in which a key sees about 5 A rows
EV2 = ("define stream A (k int, ts long, id int, price double);"
       "define stream B (k int, ts long, id int, price double);")
QUERY = ("partition with (k of A) begin from A%s select k, sum(price) as s, avg(price) as a, count() as c "
         "insert into O; end;")
PLANS = {"length_batch_5": "#window.lengthBatch(5)",
         "external_time_batch": "#window.externalTimeBatch(ts, %d)" % T,
         "window_length_5": "#window.length(5)"}
KINDS = {0: "filter", 1: "partition", 2: "walk", 5: "agg", 6: "other", 10: "mq_partition", 11: "mq_walk"}
CASE_LIMIT_S = 240


def child(name, n, steps):
    sys.path.insert(0, os.path.join(HERE, "..", "flink-siddhi_amd"))
    import torch
    import flink_siddhi as fs
    from flink_siddhi import workload

    batches = []
    for s in range(steps + 1):   # consecutive stream slices (ts ascending across steps)
        d = workload.generate_device(s * n, n, keys, rate=rate)
        batches.append((d, [d["k"], d["ts"], d["id"], d["price"]]))
    torch.cuda.synchronize()
    clause = PLANS[name]
    rt = fs.SiddhiAppRuntime(EV2 + QUERY % clause, ts_order=1, ordered_output=0, omit_seq=1, profile=1,
                             key_capacity=keys, pending_slots=16)
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


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--case":
        return child(sys.argv[2], 1 << int(sys.argv[3]), int(sys.argv[4]))
    lg = int(sys.argv[1]) if len(sys.argv) > 1 else 24
    steps = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    for name in PLANS:
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", name, str(lg), str(steps)],
                               timeout=CASE_LIMIT_S)
        except subprocess.TimeoutExpired:
            print(json.dumps({"plan": name, "error": "time limit of %d s" % CASE_LIMIT_S}), flush=True)
            return 124      # nothing more is started after a case that hung
        if r.returncode:
            print(json.dumps({"plan": name, "error": "exit status %d" % r.returncode}), flush=True)
            return r.returncode
    return 0


if __name__ == "__main__":
    sys.exit(main())
