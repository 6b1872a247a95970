"""An independent reference for the sequence grammar, and the shared streams
and plans of the grammar tests (no GPU, no engine or oracle state).

Scope: the disjoint-stream subset.  State j of a sequence reads stream j of
A, B, C, D and has one condition on its own `id` column; the first state
counts exactly one.  There the life of a partial is a property of a string,
so the reference is a regular expression and not a second automaton.  Per
partition key:

1. the key's events on the query's streams become a string: letter j in lower
   case for an event on state j's stream whose condition holds, in upper case
   when it fails (which breaks contiguity like any foreign letter);
2. R = (a{1,1})(b{m2,n2})(c{m3,n3})..., RL = R with the last state's minimum
   raised to at least 1, P = the prefixes of R's language;
3. for every start i (s[i] == 'a'; only the first one without `every`) the
   ends e >= i are walked: stop at the first e with |ts[e] - ts[i]| > within,
   or where s[i..e] is no prefix of a match (P); a row is emitted at e when
   R matches s[i..e] in full, and a start that has emitted goes on only while
   RL matched too (the partial sits in its last state and still grows);
4. captures are read from the group spans: sK / sK[0] the first event of
   group K, sK[last] the last, sK[n] event n, None when the group is shorter;
5. a row is (ts of event e, arrival number of e, data), in arrival order.

The walk also counts what makes a shape's run non-vacuous (Counters).
"""
from __future__ import annotations

import re
from collections import namedtuple
from typing import Dict, List, Optional

import numpy as np

STREAMS = ("A", "B", "C", "D", "E")           # E: defined, read by no query
LAYOUT = "(k int, ts long, id int, price double)"
DEFS = "".join("define stream %s %s;" % (s, LAYOUT) for s in STREAMS)
QUANTS = {"1": (1, 1), "+": (1, -1), "*": (0, -1), "?": (0, 1),
          "<2>": (2, 2), "<2:3>": (2, 3), "<2:>": (2, -1), "<0:2>": (0, 2)}
QUANT_NAMES = tuple(QUANTS)
BP_QUANTS = ("1", "+", "*", "?")              # min <= 1, max 1 or unbounded
ID_RANGE = 10
THRESH = (8, 7, 8, 7)                         # state j: id < THRESH[j]
THRESH_ALT = (7, 8, 7, 8)
WITHIN = 6

# quants: the quantifier names of states 1.. (state 0 counts one); caps: (state, index) with
# index 0 (written sK), "0" (written sK[0]), "last" or 1; alt: the other thresholds
Shape = namedtuple("Shape", "quants every within caps alt")


def shape(quants, every=True, within=WITHIN, caps=None, alt=False):
    quants = tuple(quants)
    if caps is None:
        caps = all_caps(len(quants) + 1)
    return Shape(quants, every, within, tuple(caps), alt)


def all_caps(n):
    """s1, then [0], [last] and [1] of every later state."""
    return [(0, 0)] + [(j, ix) for j in range(1, n) for ix in ("0", "last", 1)]


def name(sh: Shape) -> str:
    txt = "A" + "".join("," + STREAMS[j + 1] + ("" if q == "1" else q) for j, q in enumerate(sh.quants))
    return "%s%s%s%s" % (txt, " every" if sh.every else "", " w%d" % sh.within if sh.within is not None else "",
                         " alt" if sh.alt else "")


def bounds(sh: Shape):
    return [(1, 1)] + [QUANTS[q] for q in sh.quants]


def thresholds(sh: Shape):
    return THRESH_ALT if sh.alt else THRESH


def is_bit_parallel(sh: Shape) -> bool:
    return all(q in BP_QUANTS for q in sh.quants)


# ---- plans -------------------------------------------------------------------
def cap_text(j, ix, col="id"):
    return "s%d%s.%s" % (j + 1, "" if ix == 0 else "[%s]" % ix, col)


def query_text(sh: Shape, out: str) -> str:
    th = thresholds(sh)
    states = ["s%d=%s[id < %d]%s" % (j + 1, STREAMS[j], th[j], "" if j == 0 or sh.quants[j - 1] == "1" else sh.quants[j - 1])
              for j in range(len(sh.quants) + 1)]
    sel = ["s1.k as k"] + ["%s as c%d" % (cap_text(j, ix), i) for i, (j, ix) in enumerate(sh.caps)]
    return "from %s%s%s select %s insert into %s;" % (
        "every " if sh.every else "", ", ".join(states),
        " within %d milliseconds" % sh.within if sh.within is not None else "", ", ".join(sel), out)


PARTITION = "partition with (%s) begin " % ", ".join("k of %s" % s for s in STREAMS[:4])


def plan_text(shapes, prefix="O") -> str:
    """One app: every shape a query of one partition, output stream <prefix><i>."""
    return DEFS + PARTITION + "".join(query_text(sh, "%s%d" % (prefix, i)) for i, sh in enumerate(shapes)) + " end;"


# ---- streams -----------------------------------------------------------------
def make_stream(n, keys, seed, silent=0, hot_share=0.0, streams=5, burst=10.0):
    """n rows in arrival order, ts non-decreasing.  Rows come in bursts of one
    key (geometric length, mean `burst`); inside a key the stream follows a
    chain that favours staying and moving on to the next stream, so count runs
    and whole sequences occur; ts steps are drawn from {0, 1, 2, 7} (7 is
    beyond `within`).  Key 0 gets `hot_share` of the bursts, `silent` keys
    (5, 16, 27, ...) no row at all."""
    rng = np.random.default_rng(seed)
    k = np.zeros(n, np.int32)
    st = np.zeros(n, np.uint8)
    quiet = set(range(5, keys, 11)[:silent])
    live = np.array([x for x in range(keys) if x not in quiet])
    cur = rng.integers(0, streams, keys)
    i = 0
    while i < n:
        key = 0 if rng.random() < hot_share else int(live[rng.integers(0, len(live))])
        m = min(n - i, int(rng.geometric(1.0 / burst)))
        u = rng.random(m)
        jump = rng.integers(0, streams, m)
        for x in range(m):
            s = cur[key]
            s = s if u[x] < 0.44 else (s + 1) % streams if u[x] < 0.85 else (s + 2) % streams if u[x] < 0.93 else jump[x]
            cur[key] = s
            k[i + x], st[i + x] = key, s
        i += m
    dt = rng.choice(np.array([0, 1, 2, 7], np.int64), n, p=[0.60, 0.27, 0.08, 0.05])
    ts = 1_000_000 + np.cumsum(dt)
    return {"k": k, "ts": ts.astype(np.int64), "id": rng.integers(0, ID_RANGE, n).astype(np.int32),
            "price": rng.random(n), "stream": st}


def events(w):
    k, ts, i, p, st = (w[c].tolist() for c in ("k", "ts", "id", "price", "stream"))
    return [(STREAMS[st[j]], ts[j], (k[j], ts[j], i[j], p[j])) for j in range(len(ts))]


# ---- the reference -----------------------------------------------------------
def _rep(letter, lo, hi):
    return "%s{%d,%s}" % (letter, lo, "" if hi < 0 else hi)


def regexes(sh: Shape):
    b = bounds(sh)
    let = "abcd"
    groups = ["(%s)" % _rep(let[j], lo, hi) for j, (lo, hi) in enumerate(b)]
    last = "(%s)" % _rep(let[len(b) - 1], max(1, b[-1][0]), b[-1][1])
    prefix = "|".join("".join(_rep(let[i], *b[i]) for i in range(j)) + _rep(let[j], 0, b[j][1]) for j in range(len(b)))
    return re.compile("".join(groups)), re.compile("".join(groups[:-1]) + last), re.compile(prefix)


class Counters:
    """What a shape's run exercised, from the reference alone."""

    def __init__(self, n):
        self.rows = 0
        self.at_max = [0] * n       # matches with state j's count at its (finite) maximum
        self.over_max = [0] * n     # starts discarded by state j's event at max + 1
        self.below_min = [0] * n    # starts discarded by the next state's event while state j is below min
        self.skipped = [0] * n      # matches whose state j is empty
        self.took = [0] * n         # matches whose optional state j is not empty
        self.multi = 0              # starts that emitted more than once
        self.expired = 0            # starts ended by `within`


def key_strings(w, n_states, th):
    """Per key: (string, ts list, arrival numbers) of the events on streams < n_states."""
    out = {}
    sel = np.flatnonzero(w["stream"] < n_states)
    k, st, idv, ts = w["k"][sel], w["stream"][sel], w["id"][sel], w["ts"][sel]
    thr = np.array(th[:n_states])[st]
    code = np.where(idv < thr, ord("a") + st, ord("A") + st).astype(np.uint8)
    order = np.argsort(k, kind="stable")
    ks, first = np.unique(k[order], return_index=True)
    ends = list(first[1:]) + [len(order)]
    for key, f, e in zip(ks.tolist(), first.tolist(), ends):
        ix = order[f:e]
        out[key] = (code[ix].tobytes().decode("ascii"), ts[ix].tolist(), sel[ix].tolist())
    return out


def reference(sh: Shape, w, strings: Optional[dict] = None, col="id"):
    """-> (rows [(ts, arrival, (k, captures...))], Counters)."""
    b = bounds(sh)
    n = len(b)
    R, RL, P = regexes(sh)
    cn = Counters(n)
    rows = []
    vals = w[col].tolist()
    if strings is None:
        strings = key_strings(w, n, thresholds(sh))
    for key, (s, ts, arr) in strings.items():
        starts = [i for i, ch in enumerate(s) if ch == "a"]
        if not sh.every:
            starts = starts[:1]
        for i in starts:
            emitted = 0
            for e in range(i, len(s)):
                if sh.within is not None and abs(ts[e] - ts[i]) > sh.within:
                    cn.expired += 1
                    break
                if P.fullmatch(s, i, e + 1) is None:
                    # the partial s[i..e-1] was discarded by event e: why?
                    c = s[e - 1]
                    j = ord(c) - ord("a")
                    run = (e - i) - len(s[i:e].rstrip(c))
                    if 1 <= j < n - 1 and s[e] == c and run == b[j][1]:
                        cn.over_max[j] += 1
                    if j + 1 < n and s[e] == chr(ord(c) + 1) and run < b[j][0]:
                        cn.below_min[j] += 1
                    if j + 1 < n - 1 and s[e] == chr(ord(c) + 2) and b[j + 1][0] > 0:
                        cn.below_min[j + 1] += 1
                    break
                m = R.fullmatch(s, i, e + 1)
                if m is None:
                    continue
                data = [key]
                for j, ix in sh.caps:
                    g0, g1 = m.span(j + 1)
                    if ix == "last":
                        pos = g1 - 1 if g1 > g0 else None
                    else:
                        pos = g0 + int(ix) if g0 + int(ix) < g1 else None
                    data.append(None if pos is None else vals[arr[pos]])
                rows.append((ts[e], arr[e], tuple(data)))
                emitted += 1
                cn.rows += 1
                for j in range(1, n):
                    ln = m.end(j + 1) - m.start(j + 1)
                    cn.at_max[j] += ln == b[j][1]
                    cn.skipped[j] += ln == 0
                    cn.took[j] += b[j][0] == 0 and ln > 0
                if RL.fullmatch(s, i, e + 1) is None:
                    break
            cn.multi += emitted > 1
    rows.sort(key=lambda r: r[1])
    return rows, cn


# ---- what a shape cannot show, by arithmetic -----------------------------------
def requirements(sh: Shape) -> Dict[str, List[int]]:
    """Counter -> the states (or [0]) where it must be positive.  Left out,
    because the grammar rules them out:
    - took: an optional state whose followers are all optional is never taken:
      the partial emits as soon as the state before it is satisfied and is
      consumed (it is not in the last state);
    - at_max: states with a finite maximum of 2 or more only (a count of one
      is at its maximum in every match), and not the never-taken ones; nor a
      state before the last whose followers are all optional and whose
      minimum is below its maximum: the partial emits at the minimum and is
      consumed there;
    - discard: a count event discards a start only in a state between the
      first and the last: its own event at max + 1 (the last state's partial
      is consumed when it reaches max), or the next state's event while its
      minimum is not reached.  Two-state shapes have no such state;
    - discard, expired: where every state after the first is optional the
      start emits at once and is consumed: no partial lives to be discarded
      or to expire;
    - multi: a trailing state that is unbounded emits again only when its
      minimum is above zero (a trailing `*` is such an optional tail)."""
    b = bounds(sh)
    n = len(b)
    req = {"rows": [0]}
    opt = [j for j in range(1, n) if b[j][0] == 0]
    never = [j for j in opt if all(b[x][0] == 0 for x in range(j + 1, n))]
    stuck = [j for j in range(1, n - 1) if b[j][0] < b[j][1] and all(b[x][0] == 0 for x in range(j + 1, n))]
    req["at_max"] = [j for j in range(1, n) if b[j][1] >= 2 and j not in never and j not in stuck]
    lives = any(b[j][0] > 0 for j in range(1, n))
    if lives and any(b[j][1] > 0 or b[j][0] > 0 for j in range(1, n - 1)):
        req["discard"] = [0]
    req["skipped"] = opt
    req["took"] = [j for j in opt if j not in never]
    if b[-1][1] < 0 and b[-1][0] >= 1:
        req["multi"] = [0]
    if sh.within is not None and lives:
        req["expired"] = [0]
    return req


def missing(sh: Shape, cn: Counters) -> List[str]:
    """The required counters that stayed at zero."""
    req = requirements(sh)
    out = []
    for what, where in req.items():
        for j in where:
            if what == "rows":
                v = cn.rows
            elif what == "discard":
                v = sum(cn.over_max) + sum(cn.below_min)
            elif what in ("multi", "expired"):
                v = getattr(cn, what)
            else:
                v = getattr(cn, what)[j]
            if v <= 0:
                out.append("%s[%d]" % (what, j))
    return out


# ---- the grids ---------------------------------------------------------------
def cpu_grid(four_state_step=1):
    """{1, +, *, ?, <2>, <2:3>, <2:>, <0:2>} at every position after the
    first, 2 to 4 states, every on / off, within absent / 6 ms, all captures."""
    import itertools
    out = []
    for n in (2, 3, 4):
        combos = list(itertools.product(QUANT_NAMES, repeat=n - 1))
        if n == 4:
            combos = combos[::four_state_step]
        for q in combos:
            for every in (True, False):
                for within in (None, WITHIN):
                    out.append(shape(q, every, within))
    return out


def gpu_caps(quants, i):
    """At most four captures (a multi-query group carries four): s1, then of
    every later state the first or the last event by the bits of i; two- and
    three-state shapes take both of state 2."""
    n = len(quants) + 1
    if n == 2:
        return [(0, 0), (1, "0" if i & 1 else 0), (1, "last")]
    if n == 3:
        return [(0, 0), (1, 0), (1, "last"), (2, "last" if i & 1 else "0")]
    return [(0, 0)] + [(j, "last" if (i >> (j - 1)) & 1 else 0) for j in range(1, n)]


FOUR_STATE = (
    # two adjacent optional states; an optional tail behind a bounded count
    ("?", "?", "1"), ("?", "*", "+"), ("*", "?", "<2>"), ("<0:2>", "?", "1"), ("1", "<2:3>", "?"), ("+", "<2>", "*"),
    ("<2:3>", "?", "?"), ("?", "<0:2>", "<0:2>"),
    # trailing +, * and <2:>
    ("1", "1", "+"), ("+", "?", "+"), ("1", "+", "*"), ("<2>", "1", "*"), ("1", "?", "<2:>"), ("<2:3>", "+", "<2:>"),
    # <0:2> first after the start
    ("<0:2>", "1", "1"), ("<0:2>", "+", "?"), ("<0:2>", "<2:3>", "+"), ("<0:2>", "<2:>", "1"),
    # the rest of the quantifiers in the middle and at the end
    ("1", "1", "1"), ("+", "+", "1"), ("*", "*", "1"), ("<2:>", "1", "<2:3>"), ("1", "<2:>", "<0:2>"), ("*", "+", "<2>"),
)
# again without `every`, and again without `within`
AGAIN = (("+",), ("<2:3>",), ("?", "1"), ("+", "1"), ("*", "+"), ("<2>", "1"), ("<2:3>", "?"), ("<0:2>", "+"),
         ("1", "<2:>"), ("?", "?", "1"), ("1", "<2:3>", "?"), ("<0:2>", "1", "1"))


def gpu_shapes():
    """All 8 two-state and 64 three-state shapes and the 24 four-state ones
    with `every` and `within 6 milliseconds`; 12 of them again without
    `every`, 12 again without `within`."""
    import itertools
    base = [q for n in (2, 3) for q in itertools.product(QUANT_NAMES, repeat=n - 1)] + list(FOUR_STATE)
    out = [shape(q, True, WITHIN, gpu_caps(q, i)) for i, q in enumerate(base)]
    out += [shape(q, False, WITHIN, gpu_caps(q, i + 1)) for i, q in enumerate(AGAIN)]
    out += [shape(q, True, None, gpu_caps(q, i)) for i, q in enumerate(AGAIN)]
    assert len(out) == 8 + 64 + 24 + 12 + 12 and len(set(out)) == len(out)
    return out


GPU_N, GPU_KEYS, GPU_SILENT, GPU_SEED = 6000, 130, 12, 106
_gpu = {}


def gpu_stream():
    if "w" not in _gpu:
        _gpu["w"] = make_stream(GPU_N, GPU_KEYS, GPU_SEED, silent=GPU_SILENT, hot_share=0.4)
    return {c: v.copy() for c, v in _gpu["w"].items()}


def inside_count_run(w, r):
    """Rows r - 1 and r are consecutive condition-passing B rows of one key,
    right after a passing A row of that key: a batch that ends before row r
    ends inside the count run of every shape whose second state can take two."""
    k = int(w["k"][r])
    mine = np.flatnonzero((w["k"][:r] == k) & (w["stream"][:r] < 4))
    ok = lambda i, s: int(w["stream"][i]) == s and int(w["id"][i]) < min(THRESH[s], THRESH_ALT[s])  # noqa: E731
    return (len(mine) >= 2 and int(mine[-1]) == r - 1 and ok(r, 1) and ok(r - 1, 1) and ok(int(mine[-2]), 0)
            and int(w["ts"][r] - w["ts"][mine[-2]]) <= WITHIN)


def gpu_batches(w=None):
    """Six uneven batches; the second is a single row, the third ends inside a count run."""
    w = gpu_stream() if w is None else w
    cut = next(r for r in range(2800, len(w["ts"])) if inside_count_run(w, r))
    sizes = (1700, 1, cut - 1701, 1300, 900)
    sizes += (len(w["ts"]) - sum(sizes),)
    assert len(sizes) == 6 and min(sizes) > 0 and sum(sizes[:3]) == cut
    return sizes


SNAPSHOT_AFTER = 2      # the batch that ends inside the count run


def gpu_reference(sh: Shape):
    """(rows, Counters) of a GPU shape on the GPU stream, computed once."""
    if sh not in _gpu:
        w = _gpu.get("w")
        if w is None:
            gpu_stream()
            w = _gpu["w"]
        n = len(sh.quants) + 1
        sk = ("strings", n, sh.alt)
        if sk not in _gpu:
            _gpu[sk] = key_strings(w, n, thresholds(sh))
        _gpu[sh] = reference(sh, w, _gpu[sk])
    return _gpu[sh]
