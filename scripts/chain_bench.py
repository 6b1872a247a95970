"""Query chaining at the bench geometry of config 3: the chained plan
(two cleaning producers feeding the partitioned `every s1=A1[f] -> s2=B1[g]
within 10 sec`) against its hand-inlined twin (config 3's shape with the
producers' filters as extra conjuncts), 2^20 keys, 2^28 events per step,
device-resident generator input, event-time order (ts_order = 1: the closed
form), unordered output without arrival numbers, 32 Mi-row chunks — bench.py's
options for the pattern workload.

(config 3's own g, `id % 7 == 0`, passes no row of B1 = B[id % 7 != 0]; the
reader's g here is `id % 5 == 0`, as in tests/test_gpu_chain.py.)

The driver holds no GPU: every measurement is a child process under its own
time limit, chained and twin alternating three times, then one profiled run
of each (HIP events around every launch) for k_derive's time, and one of a
plan with a computed select item (`price * 2.0 as p2` read by a filter) for
the interpreter instance of k_derive; it stops at the first child that fails
or overruns its limit.  One view is built per batch, so a step launches
k_derive once over its 2^28 rows; the time is reported per 32 Mi events.
Prints one JSON line.

usage: python scripts/chain_bench.py [log2 events per step] [timed steps]"""
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
EV = ("define stream A (k int, ts long, id int, price double);"
      "define stream B (k int, ts long, id int, price double);")
SEL = "select s1.k as k, s1.price as p1, s2.price as p2, s2.ts as t insert into O; end;"
PLANS = {
    "chained": EV + "from A[price > 0.1] select k, ts, id, price insert into A1;"
                    "from B[id % 7 != 0] select k, ts, id, price insert into B1;"
                    "partition with (k of A1, k of B1) begin "
                    "from every s1=A1[price > 0.5] -> s2=B1[id % 5 == 0] within 10 sec " + SEL,
    "twin": EV + "partition with (k of A, k of B) begin "
                 "from every s1=A[price > 0.1 and price > 0.5] -> s2=B[id % 7 != 0 and id % 5 == 0] "
                 "within 10 sec " + SEL,
    # a computed select item: the interpreter instance of k_derive, one materialised column
    "computed": EV + "from A[price > 0.1] select k, ts, id, price * 2.0 as p2 insert into M;"
                     "from M[p2 > 1.9] select k, p2 insert into O;",
}
# k_derive at this plan: reads price (8), id (4) and the handle (1) once, writes the handle (1);
# every select item is a same-position copy, so no column is materialised
DERIVE_BYTES = 8 + 4 + 1 + 1
# the computed plan: reads price (8) and the handle (1) once, writes the handle (1) and p2 (8)
DERIVE_VM_BYTES = 8 + 1 + 1 + 8
K_OTHER, K_CF_PART = 6, 7


def child(name, lg, steps, profile):
    sys.path.insert(0, os.path.join(HERE, "..", "flink-siddhi_amd"))
    import torch
    import flink_siddhi as fs
    from flink_siddhi import workload
    n, keys = 1 << lg, 1 << 20
    rt = fs.SiddhiAppRuntime(PLANS[name], key_capacity=keys, chunk_events=1 << 25, ts_order=1, ordered_output=0,
                             omit_seq=1, profile=profile)
    busy, o_rows = 0.0, 0
    for s in range(steps + 1):   # step 0 warms up; generation is off the clock
        d = workload.generate_device(s * n, n, keys, rate=400)
        torch.cuda.synchronize()
        if s == 1:
            st0 = rt.stats()
        t = time.perf_counter()
        rt.send("A", d["ts"], [d["k"], d["ts"], d["id"], d["price"]], streams=d["stream"])
        if profile and s >= 1:   # rows of O alone (the profiled runs are not the throughput runs)
            o_rows += int(rt.output_device("O").n)
        rt.flush()
        if s >= 1:
            busy += time.perf_counter() - t
        del d
    st1 = rt.stats()
    matches = int(st1.matches_out - st0.matches_out)
    # (every output stream's rows: the chained plan also emits A1 and B1 themselves)
    res = {"plan": name, "events_per_s": round(n * steps / busy), "output_rows_per_step": matches // steps,
           "cf_partition_launches": int(st1.kernel_launches[K_CF_PART] - st0.kernel_launches[K_CF_PART])}
    if profile:
        timed = int(st1.kernel_timed[K_OTHER] - st0.kernel_timed[K_OTHER])
        res["O_rows_per_step"] = o_rows // steps
        res["other_launches_per_step"] = int(st1.kernel_launches[K_OTHER] - st0.kernel_launches[K_OTHER]) // steps
        res["other_ms_per_step"] = (st1.kernel_ms[K_OTHER] - st0.kernel_ms[K_OTHER]) / steps if timed else 0.0
    rt.shutdown()
    print(json.dumps(res), flush=True)


def spawn(name, lg, steps, profile, limit):
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", name, str(lg), str(steps), str(profile)],
                       capture_output=True, text=True, timeout=limit)
    if p.returncode != 0:
        sys.stderr.write(p.stdout + p.stderr)
        raise SystemExit("chain_bench: %s failed (exit %d); stopping" % (name, p.returncode))
    return json.loads(p.stdout.strip().splitlines()[-1])


def main():
    lg = int(sys.argv[1]) if len(sys.argv) > 1 else 28
    steps = int(sys.argv[2]) if len(sys.argv) > 2 else 2
    limit = 240
    runs = {"chained": [], "twin": []}
    for _ in range(3):
        for name in ("chained", "twin"):
            runs[name].append(spawn(name, lg, steps, 0, limit))
    prof = {name: spawn(name, lg, steps, 1, limit) for name in ("chained", "twin", "computed")}
    vm32 = prof["computed"]["other_ms_per_step"] * 1e3 * (1 << 25) / (1 << lg)   # its K_OTHER launches are k_derive only
    n = 1 << lg
    # the twin's K_OTHER launches (none on this path) are subtracted, should it have any
    derive_ms = prof["chained"]["other_ms_per_step"] - prof["twin"]["other_ms_per_step"]
    per32 = derive_ms * 1e3 * (1 << 25) / n
    eps = {k: [r["events_per_s"] for r in v] for k, v in runs.items()}
    med = {k: sorted(v)[1] for k, v in eps.items()}
    print(json.dumps({
        "bench": "chain_bench", "events_per_step": n, "timed_steps": steps, "keys": 1 << 20,
        "chained_events_per_s": eps["chained"], "twin_events_per_s": eps["twin"],
        "chained_over_twin_median": round(med["chained"] / med["twin"], 4),
        "output_rows_per_step": {k: v[0]["output_rows_per_step"] for k, v in runs.items()},
        "O_rows_per_step": {k: prof[k]["O_rows_per_step"] for k in ("chained", "twin")},
        "cf_partition_launches": {k: v[0]["cf_partition_launches"] for k, v in runs.items()},
        "k_derive_launches_per_step": prof["chained"]["other_launches_per_step"] -
        prof["twin"]["other_launches_per_step"],
        "k_derive_us_per_32Mi_events": round(per32, 1),
        "k_derive_design_bytes_per_event": DERIVE_BYTES,
        "k_derive_TB_per_s": round(DERIVE_BYTES * (1 << 25) / (per32 * 1e-6) / 1e12, 3) if per32 > 0 else None,
        "k_derive_vm_launches_per_step": prof["computed"]["other_launches_per_step"],
        "k_derive_vm_us_per_32Mi_events": round(vm32, 1),
        "k_derive_vm_design_bytes_per_event": DERIVE_VM_BYTES,
        "k_derive_vm_TB_per_s": round(DERIVE_VM_BYTES * (1 << 25) / (vm32 * 1e-6) / 1e12, 3) if vm32 > 0 else None,
    }), flush=True)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        child(sys.argv[2], int(sys.argv[3]), int(sys.argv[4]), int(sys.argv[5]))
    else:
        main()
