"""Event tables against the sliding-window walk (the context figure: code this
feature does not touch).  Plans:

  table_upsert_join   `from A select k, id, price update or insert into T on
                      T.k == k` + `from B as b join T as t on b.k == t.k
                      select ...` (k_partition + k_tabwalk<false>)
  table_vm            the same with a further `on` conjunct and a computed
                      item (k_tabwalk<true>)
  window_length_5     the partitioned `A#window.length(5)` plan of
                      scripts/window_bench.py, unchanged

Device-resident generator input, 2^20 keys, 2^24 events per step, default
chunks; one warm-up step, then timed steps; ordered_output = 0, omit_seq = 1,
profile = 1 (HIP events around each launch; a chunk is one launch of each
kernel kind).  Each case runs in its own child process under its own time
limit.  Prints one JSON line per case: events/s over the timed steps and the
mean time per launch (= per chunk) of the partition pass and the walk.

usage: python scripts/table_bench.py [log2 events per step] [steps]"""
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "flink-siddhi_amd"))

KEYS = 1 << 20
RATE = 400
EV2 = ("define stream A (k int, ts long, id int, price double);"
       "define stream B (k int, ts long, id int, price double);")
TAB = "@PrimaryKey('k') define table T (k int, id int, price double);"
UPSERT = "from A select k, id, price update or insert into T on T.k == k;"
PLANS = {
    "table_upsert_join": EV2 + TAB + UPSERT + ("from B as b join T as t on b.k == t.k "
                                               "select b.k as k, b.id as bid, t.id as tid, t.price as tp insert into O;"),
    "table_vm": EV2 + TAB + UPSERT + ("from B as b join T as t on b.k == t.k and b.price > t.price "
                                      "select b.k as k, b.price - t.price as d, t.id as tid insert into O;"),
    "window_length_5": EV2 + ("partition with (k of A) begin from A#window.length(5) select k, sum(price) as s, "
                              "avg(price) as a, count() as c insert into O; end;"),
}
KINDS = {1: "partition", 5: "window_walk", 15: "table_walk"}
CASE_LIMIT_S = 240


def child(name, log2n, steps):
    import torch
    import flink_siddhi as fs
    from flink_siddhi import workload

    n = 1 << log2n
    batches = []
    for s in range(steps + 1):   # consecutive stream slices
        d = workload.generate_device(s * n, n, KEYS, rate=RATE)
        batches.append((d, [d["k"], d["ts"], d["id"], d["price"]]))
    torch.cuda.synchronize()
    rt = fs.SiddhiAppRuntime(PLANS[name], ts_order=1, ordered_output=0, omit_seq=1, profile=1, key_capacity=KEYS)
    rows = 0
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
    rows = int(st1.matches_out - st0.matches_out)
    res = {"plan": name, "events_per_step": n, "steps": steps, "keys": KEYS, "events_per_s": round(n * steps / dt),
           "rows_out": rows, "table_dropped": int(st1.table_dropped), "us_per_launch": {}, "launches": {}}
    for k, kn in KINDS.items():
        timed = st1.kernel_timed[k] - st0.kernel_timed[k]
        if timed:
            res["us_per_launch"][kn] = round(1e3 * (st1.kernel_ms[k] - st0.kernel_ms[k]) / timed, 1)
            res["launches"][kn] = int(st1.kernel_launches[k] - st0.kernel_launches[k])
    rt.shutdown()
    print(json.dumps(res), flush=True)


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--case":
        return child(sys.argv[2], int(sys.argv[3]), int(sys.argv[4]))
    log2n = sys.argv[1] if len(sys.argv) > 1 else "24"
    steps = sys.argv[2] if len(sys.argv) > 2 else "3"
    for name in PLANS:
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", name, log2n, steps],
                               timeout=CASE_LIMIT_S)
        except subprocess.TimeoutExpired:
            print(json.dumps({"plan": name, "error": "time limit of %d s" % CASE_LIMIT_S}), flush=True)
            return 1   # a case that hangs: nothing more is started on the device
        if r.returncode != 0:
            print(json.dumps({"plan": name, "error": "exit status %d" % r.returncode}), flush=True)
            return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
