"""Count states in patterns against the engine's own three-state chain: on one
stream, the same start state and the same conditions as

  chain  every a=A[f] -> b=B[g] -> c=C[h] within W          (the yardstick: code
         the count transition must not slow; runs on any commit)
  count  every a=A[f] -> b=B[g]<2:4> -> c=C[h] within W
  open   every a=A[f] -> b=B[g]<2:> within W                 (two positions, the
         count state last and unbounded)

Conditions as in scripts/logic_bench.py: device-resident generator input, 2^20
keys, three streams, default chunks; one warm-up step, then timed steps.  Each
case runs in a child process of its own under a time limit, one after the
other; the first child that fails, faults or runs out of time ends the run
(nothing more is started).  Prints one JSON line per run: events/s over the
timed steps, rows out, and the mean time per launch of every kernel kind that
ran.  CEP_LIB picks the library (the parent commit's for the yardstick).

usage: python scripts/count_bench.py [--cases chain,count,open] [--repeat N] [log2 events per step] [steps]"""
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
KEYS = 1 << 20
RATE = 400                                    # rows per ms over the three streams
W = "10 sec"                                  # a key sees a row every 2.6 s: about 4 rows in W
EV3 = "".join("define stream %s (k int, ts long, id int, price double);" % s for s in "ABC")
F, G, H = "a=A[price > 0.5]", "b=B[id % 3 == 0]", "c=C[id % 3 != 0]"
SHAPES = {"chain": ("%s -> %s -> %s" % (F, G, H), "b.price as bp, c.ts as ct"),
          "count": ("%s -> %s<2:4> -> %s" % (F, G, H), "b[last].price as bp, c.ts as ct"),
          "open": ("%s -> %s<2:>" % (F, G), "b[0].price as bp, b[last].ts as ct")}
KINDS = {1: "partition", 2: "walk", 6: "other"}
CHILD_LIMIT = 240                             # seconds per case


def plan(case):
    shape, sel = SHAPES[case]
    return (EV3 + "partition with (k of A, k of B, k of C) begin from every " + shape +
            " within " + W + " select a.k as k, a.price as ap, " + sel + " insert into O; end;")


def child(case, n, steps):
    sys.path.insert(0, os.path.join(HERE, "..", "flink-siddhi_amd"))
    import torch
    import flink_siddhi as fs
    from flink_siddhi import workload
    batches = []
    for s in range(steps + 1):   # consecutive stream slices (ts ascending across steps)
        d = workload.generate_device(s * n, n, KEYS, rate=RATE)
        d["stream"] = workload.config5_streams(d["price"]).to(torch.uint8)
        batches.append(d)
    torch.cuda.synchronize()
    rt = fs.SiddhiAppRuntime(plan(case), ts_order=1, ordered_output=0, omit_seq=1, profile=1, key_capacity=KEYS)
    for s in range(steps + 1):
        if s == 1:
            torch.cuda.synchronize()
            st0 = rt.stats()
            t0 = time.perf_counter()
        d = batches[s]
        rt.send("A", d["ts"], [d["k"], d["ts"], d["id"], d["price"]], streams=d["stream"])
        rt.flush()
        rt.reset_output()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    st1 = rt.stats()
    res = {"case": case, "events_per_step": n, "steps": steps, "keys": KEYS,
           "events_per_s": round(n * steps / dt), "rows_out": int(st1.matches_out - st0.matches_out),
           "us_per_launch": {}, "launches": {}}
    for k, kn in KINDS.items():
        timed = st1.kernel_timed[k] - st0.kernel_timed[k]
        if timed:
            res["us_per_launch"][kn] = round(1e3 * (st1.kernel_ms[k] - st0.kernel_ms[k]) / timed, 1)
            res["launches"][kn] = int(st1.kernel_launches[k] - st0.kernel_launches[k])
    rt.shutdown()
    print(json.dumps(res), flush=True)


def main(argv):
    cases, repeat, pos = ["chain", "count", "open"], 1, []
    it = iter(argv)
    for a in it:
        if a == "--cases":
            cases = next(it).split(",")
        elif a == "--repeat":
            repeat = int(next(it))
        elif a == "--child":
            case = next(it)
            return child(case, 1 << int(next(it)), int(next(it)))
        else:
            pos.append(a)
    lg = pos[0] if pos else "24"
    steps = pos[1] if len(pos) > 1 else "3"
    for _ in range(repeat):
        for case in cases:
            try:
                rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", case, lg, steps],
                                    timeout=CHILD_LIMIT).returncode
            except subprocess.TimeoutExpired:
                rc = 124
            if rc != 0:
                print("case %s ended with status %d: stopping" % (case, rc), flush=True)
                return rc
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]) or 0)
