#!/usr/bin/env python3
"""Write the snapshot fixtures of tests/test_gpu_snapshot_compat.py.

Run once on the GPU with the library of the commit BEFORE a change to the
snapshot code, so that the fixtures pin that commit's bytes:

    CEP_LIB=/path/to/parent/libcep.so python scripts/make_snapshot_fixtures.py

For every app of tests/snapshot_cases.py: tests/golden/snapshots/<name>.bin (the
snapshot at the split) and <name>.json (seed, options, split, the rows emitted
before the snapshot).  Each app runs twice and its snapshot is restored and
taken again; only when all three byte strings are equal does the JSON carry
"byte_exact": true, and the test then compares bytes.
"""
import argparse
import json
import struct
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
for p in ("flink-siddhi_amd", "oracle", "tests"):
    sys.path.insert(0, str(ROOT / p))

import flink_siddhi as fs  # noqa: E402
from flink_siddhi import _lib as L, workload  # noqa: E402
import snapshot_cases as SC  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "tests" / "golden" / "snapshots"))
    out = Path(ap.parse_args().out)
    out.mkdir(parents=True, exist_ok=True)
    print("library:", L.LIB_PATH)
    for name, c in SC.CASES.items():
        snap, rows = SC.first_part(name)
        again, _ = SC.first_part(name)
        rt = SC.runtime(name)
        rt.restore(snap)
        restored = rt.snapshot()
        rt.shutdown()
        exact = snap == again == restored
        why = None
        if not exact:
            why = "two runs of the parent differ" if snap != again else "the parent's restore -> snapshot differs"
            if c["opts"].get("sparse_keys"):
                why += " (dense ids are handed out by device atomics)"
        if name == "cf_overflow_reorder":   # the state the fixture is for is there
            kc, S, sw, live = struct.unpack_from("<qIII", snap, 28)
            off, over = 48, 0
            for _ in range(live):
                n = struct.unpack_from("<I", snap, off + 12)[0]
                over += n > S
                off += 16 + n * sw * 8
            held = struct.unpack_from("<q", snap, off + 5)[0]
            assert over > 0 and held == c["held"], (over, held)
        (out / (name + ".bin")).write_bytes(snap)
        doc = {"case": name, "seed": workload.SEED, "n": c["n"], "keys": c["keys"], "split": c["split"],
               "options": c["opts"], "byte_exact": exact, "rows": rows}
        if why:
            doc["comment"] = "bytes are not compared: " + why
        text = json.dumps(doc, separators=(",", ":"))
        (out / (name + ".json")).write_text(text + "\n")
        print("%-20s version %d, %6d bytes snapshot, %6d bytes json, rows %s, byte_exact %s" % (
            name, struct.unpack_from("<I", snap, 4)[0], len(snap), len(text),
            {o: len(r) for o, r in rows.items()}, exact))


if __name__ == "__main__":
    main()
