"""A plain reference for running and sliding-window aggregates, in fixed-width
numpy scalars, and the edge-value stream the aggregate tests share.

Written from the stated semantics, independent of `siddhi_oracle._Agg` and
`window_model._Acc` (plain Python ints and floats): a mistake in either side's
arithmetic shows as a disagreement (tests/test_agg_ref.py).

  sum over int / long     np.int64, wrapping to 64 bits on every step;
  sum / avg over float /  sequential np.float64 additions; a float argument is
  double (avg: any type)  widened exactly, a long is converted with one rounding
                          (JLS 5.1.2);
  min / max               compared in the argument's own type; on a tie
                          (-0.0 / 0.0 included) the earlier row stays;
  count                   an int64;
  avg                     acc / float64(count).

Cumulative mode: one accumulator set per group.  Windowed mode: one queue of
kept rows per window instance, and per row the three steps of the
window_model docstring: expire (length N: the instance holds N rows -> the
oldest leaves; time T: rows leave from the front while front.ts + T <= ts),
remove each expired row from its group oldest first (count - 1, integer sums
subtract and wrap, float sums subtract float64(v), min / max are taken again
over the group's rows left), add the row.

NaN under min / max has no stated result (see tests/test_gpu_agg_edges.py);
the reference refuses it.
"""
from __future__ import annotations

from collections import deque
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

import expr_ref as X
import siddhi_oracle as O

_M64 = (1 << 64) - 1


def _wrap(x: int) -> np.int64:
    """A Python int -> the int64 with the same low 64 bits."""
    x &= _M64
    return np.int64(x - (1 << 64) if x >> 63 else x)


def _f64(v, t: str) -> np.float64:
    """The argument as a double: exact for int and float, one rounding for long."""
    assert isinstance(v, X.DTYPE[t]), (type(v), t)
    return np.float64(v)


class _Acc:
    def __init__(self, fn: str, t: Optional[str]):
        self.fn, self.t = fn, t
        self.isum = fn == "sum" and t in (O.INT, O.LONG)
        self.acc = 0 if fn == "xsum" else np.int64(0) if self.isum else np.float64(0.0)
        self.n = np.int64(0)
        self.ext = None                  # cumulative min / max
        self.twins = 0                   # windowed min / max: the extreme left, an equal value stayed
        self.live: deque = deque()       # windowed min / max: the group's rows, oldest first

    def _better(self, v, m) -> bool:
        assert v == v and m == m, "NaN under min / max"
        return bool(v < m) if self.fn == "min" else bool(m < v)

    def add(self, v, windowed: bool):
        self.n = self.n + np.int64(1)
        if self.fn == "xsum":
            self.acc += int(v)
        elif self.fn == "sum" and self.isum:
            self.acc = _wrap(int(self.acc) + int(v))
        elif self.fn in ("sum", "avg"):
            self.acc = self.acc + _f64(v, self.t)
        elif self.fn in ("min", "max"):
            if windowed:
                self.live.append(v)
            elif self.ext is None or self._better(v, self.ext):
                self.ext = v

    def remove(self, v):
        self.n = self.n - np.int64(1)
        if self.fn == "xsum":
            self.acc -= int(v)
        elif self.fn == "sum" and self.isum:
            self.acc = _wrap(int(self.acc) - int(v))
        elif self.fn in ("sum", "avg"):
            self.acc = self.acc - _f64(v, self.t)
        elif self.fn in ("min", "max"):
            gone = self.live.popleft()
            if gone == self._extreme(gone) and any(x == gone for x in self.live):
                self.twins += 1

    def value(self, windowed: bool):
        if self.fn == "count":
            return self.n.item()
        if self.fn == "xsum":
            return self.acc
        if self.fn == "sum":
            return self.acc.item()
        if self.fn == "avg":
            return (self.acc / np.float64(self.n)).item()
        return (self._extreme(self.live[0]) if windowed else self.ext).item()

    def _extreme(self, m):
        """The first of the live rows no other live row beats, starting from m."""
        for v in self.live:
            if self._better(v, m):
                m = v
        return m


# (function, argument type, argument column); "xsum": the exact sum of an int /
# long argument as a Python int (what a wrapped sum is told from)
Spec = Tuple[str, Optional[str], Optional[int]]


def _args(specs: Sequence[Spec], cols, r):
    out = []
    for fn, t, c in specs:
        if c is None:
            out.append(None)
        else:
            assert cols[c].dtype == X.DTYPE[t], (fn, t, cols[c].dtype)
            out.append(cols[c][r])
    return out


def cumulative(specs: Sequence[Spec], group, cols, keep=None) -> List[Optional[tuple]]:
    """Per input row the aggregates' values after the row joined its group
    (None for a row `keep` drops)."""
    groups: Dict[object, List[_Acc]] = {}
    out: List[Optional[tuple]] = []
    with np.errstate(all="ignore"):
        for r in range(len(group)):
            if keep is not None and not keep[r]:
                out.append(None)
                continue
            g = groups.get(group[r])
            if g is None:
                g = groups[group[r]] = [_Acc(fn, t) for fn, t, _ in specs]
            for a, v in zip(g, _args(specs, cols, r)):
                a.add(v, False)
            out.append(tuple(a.value(False) for a in g))
    return out


def windowed(specs: Sequence[Spec], group, cols, ts, kind: str, param: int, inst=None, keep=None):
    """-> (per row values as `cumulative`, the largest number of rows any
    window instance held, how often a min / max lost its extreme while an
    equal value, -0.0 / 0.0 twins included, stayed).  inst: per row the window
    instance (default: one instance for all rows); group: per row the
    aggregate group."""
    assert kind in ("length", "time")
    queues: Dict[object, deque] = {}
    groups: Dict[object, List[_Acc]] = {}
    out: List[Optional[tuple]] = []
    max_live = 0
    with np.errstate(all="ignore"):
        for r in range(len(group)):
            if keep is not None and not keep[r]:
                out.append(None)
                continue
            w = None if inst is None else inst[r]
            q = queues.get(w)
            if q is None:
                q = queues[w] = deque()
            gone = []
            if kind == "length":
                if len(q) == param:
                    gone.append(q.popleft())
            else:
                while q and q[0][0] + param <= ts[r]:
                    gone.append(q.popleft())
            for _, gk, vals in gone:
                for a, v in zip(groups[(w, gk)], vals):
                    a.remove(v)
            gk = group[r]
            g = groups.get((w, gk))
            if g is None:
                g = groups[(w, gk)] = [_Acc(fn, t) for fn, t, _ in specs]
            vals = _args(specs, cols, r)
            for a, v in zip(g, vals):
                a.add(v, True)
            q.append((ts[r], gk, vals))
            max_live = max(max_live, len(q))
            out.append(tuple(a.value(True) for a in g))
    return out, max_live, sum(a.twins for g in groups.values() for a in g)


def rows_of(ts, group, values) -> List[Tuple[int, int, tuple]]:
    """[(ts, arrival number, (group key, aggregate values...))] for the kept rows."""
    tl, gl = np.asarray(ts).tolist(), np.asarray(group).tolist()
    return [(tl[r], r, (gl[r],) + v) for r, v in enumerate(values) if v is not None]


# ------------------------------------------------------------ the edge data --
S_COLS = (("k", O.INT), ("a", O.INT), ("b", O.LONG), ("c", O.FLOAT), ("d", O.DOUBLE),
          ("c2", O.FLOAT), ("d2", O.DOUBLE))
COL = {name: i for i, (name, _) in enumerate(S_COLS)}
TYPE = dict(S_COLS)


def stream_def(name: str = "S", ktype: str = O.INT) -> str:
    cols = (("k", ktype),) + S_COLS[1:]
    return "define stream %s (%s);" % (name, ", ".join("%s %s" % ct for ct in cols))


N_ROWS = 6144 + 77
KEYS = 96                   # a full 64-lane key block and a ragged second one
T0 = 1_500_000_000_000
_DATA: Dict[int, tuple] = {}


def _wild(v: np.ndarray) -> np.ndarray:
    """Non-finite values and values of the type's largest magnitude."""
    return ~np.isfinite(v) | (np.abs(v) == np.finfo(v.dtype).max)


def edge_stream(seed: int = 7):
    """(ts, [k, a, b, c, d, c2, d2]) of stream S: N_ROWS rows over KEYS keys,
    one event per ms.  Every value column draws at random from
    expr_ref.EDGES of its type (b: and from +-2^53); non-finite values and +-FLT_MAX / +-DBL_MAX
    stay only in keys with k % 8 == 0 and are a random finite edge value
    elsewhere, so most keys exercise finite arithmetic and some reach +-inf
    and NaN.  c2 / d2: c / d with NaN replaced by -0.0 (the min / max
    arguments)."""
    if seed not in _DATA:
        rng = np.random.default_rng(seed)
        k = rng.integers(0, KEYS, N_ROWS).astype(np.int32)
        cols = [k]
        for t in (O.INT, O.LONG, O.FLOAT, O.DOUBLE):
            e = X.EDGES[t]
            if t == O.LONG:      # and the neighbours of +-(2^53 + 1) that a double cannot tell from them
                e = np.concatenate([e, np.array([1 << 53, -(1 << 53)], np.int64)])
            v = e[rng.integers(0, len(e), N_ROWS)]
            if t in (O.FLOAT, O.DOUBLE):
                tame = e[~_wild(e)]
                sub = tame[rng.integers(0, len(tame), N_ROWS)]
                v = np.where(_wild(v) & (k % 8 != 0), sub, v)
            cols.append(v)
        for v in cols[3:5]:
            cols.append(np.where(np.isnan(v), v.dtype.type(-0.0), v))
        for c in cols:
            c.setflags(write=False)
        ts = T0 + np.arange(N_ROWS, dtype=np.int64)
        ts.setflags(write=False)
        _DATA[seed] = (ts, cols)
    return _DATA[seed]


def events(ts, cols, name: str = "S"):
    """The oracle's / the window model's event list of one stream."""
    cl = [c.tolist() for c in cols]
    tl = ts.tolist()
    return [(name, tl[i], tuple(c[i] for c in cl)) for i in range(len(tl))]


def query_values(app, wspecs, qi: int, ts, cols):
    """The aggregate calls of the single-stream query qi of the bound app
    (siddhi_oracle.parse_app of the plan without its window clauses; wspecs:
    window_model.strip_windows' per-query window) over the stream (ts, cols), before select expressions and `having`:
    ([(function, argument name or None)], per input row the calls' values or
    None for a filtered row, group per row, largest window occupancy, twin
    count as `windowed`).  Every
    integer sum is followed by its "xsum".  Filters go through expr_ref, the
    window clause and the group / instance columns are read off the bound
    query; the arithmetic is this module's."""
    q = app.queries[qi]
    assert q.kind == "single"
    n = len(ts)
    env = lambda slot: cols[slot[1]]  # noqa: E731
    keep = np.ones(n, bool)
    for f in q.filters:
        v, vn = X.evaluate(f, env, n)
        keep &= v & ~vn
    calls: list = []
    for it in q.select:
        O._agg_walk(it.expr, calls)
    specs, names = [], []
    for ce in calls:
        if ce.args:
            arg = ce.args[0]
            assert arg.kind == "attr"
            specs.append((ce.name, arg.t, arg.slot[1]))
            names.append((ce.name, S_COLS[arg.slot[1]][0]))
        else:
            specs.append((ce.name, None, None))
            names.append((ce.name, None))
    for fn, t, c in list(specs):
        if fn == "sum" and t in (O.INT, O.LONG):
            specs.append(("xsum", t, c))
            names.append(("xsum", S_COLS[c][0]))
    inst = None
    if q.partition is not None:
        inst = cols[app.streams[q.stream].index(q.partition[q.stream])].tolist()
    if q.group_by:
        assert len(q.group_by) == 1 and q.group_by[0].kind == "attr"
        group = cols[q.group_by[0].slot[1]].tolist()
    else:
        group = inst if inst is not None else [0] * n
    if wspecs[qi] is None:
        return names, cumulative(specs, group, cols, keep), group, 0, 0
    vals, live, twins = windowed(specs, group, cols, ts.tolist(), wspecs[qi][0], wspecs[qi][1], inst, keep)
    return names, vals, group, live, twins
