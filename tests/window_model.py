"""A deliberately naive reference for `#window.length(N)` / `#window.time(T)`
aggregate queries (the oracle under oracle/ refuses `#`).

One deque per window instance, one accumulator set per group, and per kept
row the three steps in plain Python ints and floats:

  1. expire   length(N): the window holds N rows -> pop the oldest;
              time(T): pop from the front while front.ts + T <= e.ts, stop at
              the first row that stays;
  2. remove   each popped row leaves its group's aggregates, oldest first
              (count -= 1, long sums subtract and wrap to 64 bits, float sums
              do acc -= float(v), min / max are recomputed from the rows left);
  3. add e, evaluate having, emit.

The window instance is Siddhi's: one per partition key inside `partition
with`, otherwise one for the whole query, whatever the `group by` says.  The
engine keeps one window per group; for `group by` + `#window.time` outside a
partition this model therefore checks the engine's equivalence argument.

The plan is parsed by siddhi_oracle with the window clauses cut out, and
filters, select items and having are evaluated by its expression evaluator;
queries without a window run on the oracle's own instances.
"""
from __future__ import annotations

import re
from collections import deque
from typing import Dict, List, Optional, Sequence, Tuple

import siddhi_oracle as O

_UNITS = {"millisec": 1, "millisecond": 1, "milliseconds": 1, "millisecs": 1, "ms": 1,
          "sec": 1000, "secs": 1000, "second": 1000, "seconds": 1000,
          "min": 60000, "mins": 60000, "minute": 60000, "minutes": 60000,
          "hour": 3600000, "hours": 3600000, "day": 86400000, "days": 86400000}

_WINDOW = re.compile(r"#\s*window\s*\.\s*(length|time)\s*\(([^)]*)\)", re.I)
_FROM = re.compile(r"\bfrom\b", re.I)


def _time_ms(arg: str) -> int:
    arg = arg.strip()
    if re.fullmatch(r"\d+[lL]?", arg):
        return int(arg.rstrip("lL"))
    total = 0
    parts = re.findall(r"(\d+)\s*([A-Za-z]+)", arg)
    if not parts:
        raise ValueError("bad time constant " + arg)
    for n, u in parts:
        total += int(n) * _UNITS[u.lower()]
    return total


def strip_windows(plan: str):
    """-> (plan without window clauses, per query (kind, param) or None)."""
    starts = [m.start() for m in _FROM.finditer(plan)]
    specs: List[Optional[Tuple[str, int]]] = []
    for i, s in enumerate(starts):
        seg = plan[s:starts[i + 1] if i + 1 < len(starts) else len(plan)]
        m = _WINDOW.search(seg)
        if m is None:
            specs.append(None)
        elif m.group(1).lower() == "length":
            specs.append(("length", int(m.group(2).strip().rstrip("lL"))))
        else:
            specs.append(("time", _time_ms(m.group(2))))
    return _WINDOW.sub("", plan), specs


class _Acc:
    """One aggregate of one group: add / remove in the stated arithmetic."""

    def __init__(self, name: str, t: str):
        self.name, self.t = name, t
        self.n = 0
        self.s = 0 if t == O.LONG else 0.0
        self.live: deque = deque()      # min / max: the group's values in the window, oldest first

    def add(self, v):
        self.n += 1
        if self.name == "sum":
            self.s = O._wrap64(self.s + v) if self.t == O.LONG else self.s + float(v)
        elif self.name == "avg":
            self.s += float(v)
        elif self.name in ("min", "max"):
            self.live.append(v)

    def remove(self, v):
        self.n -= 1
        if self.name == "sum":
            self.s = O._wrap64(self.s - v) if self.t == O.LONG else self.s - float(v)
        elif self.name == "avg":
            self.s -= float(v)
        elif self.name in ("min", "max"):
            assert self.live[0] == v        # a group's rows leave in arrival order
            self.live.popleft()

    def value(self):
        if self.name == "count":
            return self.n
        if self.name == "sum":
            return self.s
        if self.name == "avg":
            return self.s / self.n
        return min(self.live) if self.name == "min" else max(self.live)


class _WindowInstance:
    """One window (deque of kept rows) and the groups it feeds."""

    def __init__(self, q, spec, agg_exprs):
        self.q, self.kind, self.param = q, spec[0], spec[1]
        self.agg_exprs = agg_exprs
        self.rows: deque = deque()      # (ts, group key, argument values)
        self.groups: Dict[Tuple, List[_Acc]] = {}
        self.max_live = 0

    def on_event(self, ts, row, stream, seq, out):
        q = self.q
        if stream != q.stream:
            return
        env = lambda slot: row[slot[1]]  # noqa: E731
        for f in q.filters:
            if not O.evaluate(f, env):
                return
        # 1. expire, 2. remove
        popped = []
        if self.kind == "length":
            if len(self.rows) == self.param:
                popped.append(self.rows.popleft())
        else:
            while self.rows and self.rows[0][0] + self.param <= ts:
                popped.append(self.rows.popleft())
        for _, g, vals in popped:
            for a, v in zip(self.groups[g], vals):
                a.remove(v)
        # 3. add and emit
        gkey = tuple(O.evaluate(g, env) for g in q.group_by)
        vals = tuple(O.evaluate(ae.args[0], env) if ae.args else None for ae in self.agg_exprs)
        st = self.groups.get(gkey)
        if st is None:
            st = [_Acc(ae.name, ae.t) for ae in self.agg_exprs]
            self.groups[gkey] = st
        for a, v in zip(st, vals):
            a.add(v)
        self.rows.append((ts, gkey, vals))
        self.max_live = max(self.max_live, len(self.rows))
        avals = {id(ae): a.value() for a, ae in zip(st, self.agg_exprs)}
        data = tuple(O._eval_with_aggs(it.expr, env, avals) for it in q.select)
        if q.having is not None:
            def envh(slot):
                if slot[0] == "out":
                    return data[slot[1]]
                return row[slot[1]]
            if not O.evaluate(q.having, envh):
                return
        out.append(O.OutEvent(q.out, ts, data, seq))


class WindowModel:
    """OracleRuntime with window queries: send(stream, ts, row) -> [OutEvent]."""

    def __init__(self, plan: str):
        stripped, specs = strip_windows(plan)
        self.app = O.parse_app(stripped)
        assert len(specs) == len(self.app.queries), "window clause / query mismatch"
        self.specs = specs
        self.aggs: List[list] = []
        for q in self.app.queries:
            found: list = []
            if q.kind == "single":
                for it in q.select:
                    O._agg_walk(it.expr, found)
            self.aggs.append(found)
        self.instances: List[dict] = [dict() for _ in self.app.queries]
        self.seq = 0

    def send(self, stream: str, ts: int, row):
        row = tuple(row)
        out: list = []
        seq = self.seq
        self.seq += 1
        for qi, q in enumerate(self.app.queries):
            if q.partition is not None:
                if stream not in q.partition:
                    continue
                kv = row[self.app.streams[stream].index(q.partition[stream])]
            else:
                kv = None
            inst = self.instances[qi].get(kv)
            if inst is None:
                if self.specs[qi] is not None and self.aggs[qi]:
                    inst = _WindowInstance(q, self.specs[qi], self.aggs[qi])
                elif q.kind == "single":
                    inst = O._SingleInstance(q)   # a window nobody aggregates over: current events only
                else:
                    inst = O._PatternInstance(q)
                self.instances[qi][kv] = inst
            inst.on_event(ts, row, stream, seq, out)
        return out

    def max_live(self) -> int:
        """Largest number of live rows any window instance reached."""
        m = 0
        for d in self.instances:
            for inst in d.values():
                if isinstance(inst, _WindowInstance):
                    m = max(m, inst.max_live)
        return m


def model_run(plan: str, events: Sequence[Tuple[str, int, tuple]]):
    """events: [(stream_id, ts, row)] in arrival order ->
    ({out: [(ts, seq, data)]} as helpers.oracle_run, largest live count)."""
    rt = WindowModel(plan)
    out: Dict[str, List] = {}
    for sid, ts, row in events:
        for ev in rt.send(sid, ts, row):
            out.setdefault(ev.stream, []).append((ev.ts, ev.seq, ev.data))
    return out, rt.max_live()
