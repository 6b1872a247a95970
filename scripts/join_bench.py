"""Windowed stream joins: the ITCase-shaped plan

    from A#window.length(N) as s1 join B#window.time(T) as s2 on s1.k == s2.k
    select s1.ts as t, s1.id as n, s1.price as p1, s2.price as p2 insert into J;

on device-resident generator rows (65536 keys, 200 rows per ms over both
streams, so T ms hold about 100 T live B rows).  Sweeps N in {5, 255} and T in
{1, 100} (about 10^2 and 10^4 live rows).  One warm-up step (it also fills the
windows), then timed steps.  Each case runs in a child process of its own
under its own time limit and prints one JSON line: events/s over the timed
steps, and the time of all join kernels (CEP_K_JOIN, profile option: HIP
events around every launch) per chunk and per event.

There is no target: nothing exists to compare against but the CPU model, and
the probe cost is linear in the window size by design.

usage: python scripts/join_bench.py [log2 events per step] [steps]
       python scripts/join_bench.py --case N T [log2 events per step] [steps]   (one case, in this process)"""
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "flink-siddhi_amd"))

KEYS = 1 << 16
RATE = 200
CHUNK = 1 << 18                              # kJoinMaxChunk
CASE_LIMIT_S = 120
EV2 = ("define stream A (k int, ts long, id int, price double);"
       "define stream B (k int, ts long, id int, price double);")
QUERY = ("from A#window.length(%d) as s1 join B#window.time(%d) as s2 on s1.k == s2.k "
         "select s1.ts as t, s1.id as n, s1.price as p1, s2.price as p2 insert into J;")
K_JOIN = 13


def run_case(N, T, lg, steps):
    import torch

    import flink_siddhi as fs
    from flink_siddhi import workload

    n = 1 << lg
    batches = []
    for s in range(steps + 1):   # consecutive stream slices (ts ascending across steps)
        d = workload.generate_device(s * n, n, KEYS, rate=RATE)
        batches.append((d, [d["k"], d["ts"], d["id"], d["price"]]))
    torch.cuda.synchronize()
    rt = fs.SiddhiAppRuntime(EV2 + QUERY % (N, T), ts_order=1, ordered_output=0, omit_seq=1, profile=1)
    rows = 0
    for s in range(steps + 1):
        if s == 1:
            torch.cuda.synchronize()
            st0 = rt.stats()
            t0 = time.perf_counter()
        d, cols = batches[s]
        rt.send("A", d["ts"], cols, streams=d["stream"])
        rows += int(rt.output_device("J").n) if s >= 1 else 0
        rt.reset_output()
        rt.flush()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    st1 = rt.stats()
    ms = st1.kernel_ms[K_JOIN] - st0.kernel_ms[K_JOIN]
    chunks = steps * ((n + CHUNK - 1) // CHUNK)
    res = {"plan": "length(%d) join time(%d)" % (N, T), "live_time_rows": T * RATE // 2, "events_per_step": n,
           "steps": steps, "keys": KEYS, "events_per_s": round(n * steps / dt), "rows_out": rows,
           "join_kernel_us_per_chunk": round(1e3 * ms / chunks, 1),
           "join_kernel_ns_per_event": round(1e6 * ms / (n * steps), 2),
           "join_launches": int(st1.kernel_launches[K_JOIN] - st0.kernel_launches[K_JOIN]), "chunks": chunks}
    rt.shutdown()
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--case":
        run_case(int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]) if len(sys.argv) > 4 else 20,
                 int(sys.argv[5]) if len(sys.argv) > 5 else 3)
        sys.exit(0)
    lg = sys.argv[1] if len(sys.argv) > 1 else "20"
    steps = sys.argv[2] if len(sys.argv) > 2 else "3"
    for N in (5, 255):
        for T in (1, 100):
            # a fresh process per case; a case that fails or runs out of time ends the sweep
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", str(N), str(T), lg, steps],
                               timeout=CASE_LIMIT_S)
            if r.returncode != 0:
                sys.exit("case length(%d) / time(%d) ended with status %d" % (N, T, r.returncode))
