"""Static instruction-class counts per kernel from hipcc's device assembly
(-save-temps: *-hip-amdgcn-amd-amdhsa-gfx950.s).  usage:
  python3 scripts/isa_counts.py FILE.s [name filter]"""
import re
import sys

CLASSES = [
    ("readlane+writelane", re.compile(r"^v_(readlane|writelane)_")),
    ("s_load", re.compile(r"^s_load_")),
    ("s_waitcnt", re.compile(r"^s_waitcnt")),
    ("s_barrier", re.compile(r"^s_barrier")),
    ("global_atomic", re.compile(r"^global_atomic_")),
    ("scratch", re.compile(r"^scratch_")),
    ("salu", re.compile(r"^s_(?!load_|waitcnt|barrier|nop|endpgm|branch|cbranch)")),
    ("valu", re.compile(r"^v_")),
    ("lds", re.compile(r"^ds_")),
    ("vmem", re.compile(r"^(global|flat|buffer)_")),
]
INSN = re.compile(r"^\t([a-z][a-z0-9_]+)(\s|$)")


def main():
    path = sys.argv[1]
    flt = sys.argv[2] if len(sys.argv) > 2 else ""
    cur, rows = None, {}
    for line in open(path):
        m = re.match(r"^(_Z\w+):", line)
        if m:
            cur = m.group(1)
            rows[cur] = {"total": 0}
            continue
        if line.startswith(".Lfunc_end"):
            cur = None
            continue
        if cur is None:
            continue
        m = INSN.match(line)
        if not m or not re.match(r"^(s|v|ds|global|flat|buffer|scratch)_", m.group(1)):
            continue
        r = rows[cur]
        r["total"] += 1
        for name, rx in CLASSES:
            if rx.match(m.group(1)):
                r[name] = r.get(name, 0) + 1
    for name, r in rows.items():
        if flt in name and r["total"]:
            print(name)
            print("  total %d  " % r["total"] + "  ".join("%s %d" % (c, r.get(c, 0)) for c, _ in CLASSES))


main()
