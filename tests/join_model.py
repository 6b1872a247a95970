"""A deliberately naive reference for windowed stream joins

    from A[f]#window.wa [as a] join B[g]#window.wb [as b] on C
    select ... insert into O;

(the oracle under oracle/ refuses joins).  Two deques, one per side, and per
kept row e of side X, in arrival order over both streams:

  1. the other side Y's window as it stands when e arrives: of Y's kept rows
     that arrived before e, the last N (`length(N)`) or those with
     r.ts + T > e.ts (`time(T)`; a row with r.ts + T == e.ts has left);
  2. for each such r, oldest first, evaluate C with a.* bound to the A-side
     row and b.* to the B-side row, whichever of the two is e;
  3. where C holds, emit the select list with e's ts and arrival number;
  4. e enters X's own window.  It never joins rows of its own side.

A length side keeps its last N rows.  A time side applies the rule to every
row it still holds; the engine takes time-window joins with non-decreasing ts
only (ts_order = 1), the model asserts that, and a front row that has left
could then never return, so it is dropped to keep the model linear.

Filters, `on` and the select items are parsed and evaluated by
siddhi_oracle's expression parser, binder and evaluator, bound as the states
of a two-state pattern are (state 0 = the A side, state 1 = the B side).
Queries that are no join run on the oracle's own instances.
"""
from __future__ import annotations

import re
from collections import deque
from typing import Dict, List, Sequence, Tuple

import siddhi_oracle as O
from window_model import _time_ms

_SIDE = (r"(\w+)((?:\s*\[[^\]]*\])*)\s*#\s*window\s*\.\s*(length|time)\s*\(([^)]*)\)"
         r"(?:\s+as\s+(\w+))?")
_JOIN = re.compile(r"\bfrom\s+" + _SIDE + r"\s+(?:inner\s+)?join\s+" + _SIDE +
                   r"(?:\s+on\s+(.*?))?\s+select\s+(.*?)\s+insert\s+(?:current\s+events\s+)?into\s+(\w+)\s*;",
                   re.I | re.S)


def _expr(text: str) -> O.Expr:
    p = O.Parser(text)
    e = p.parse_expr()
    assert p.peek().kind == "eof", "trailing text in expression: " + text
    return e


def _select(text: str) -> List[O.SelectItem]:
    p = O.Parser(text)
    items = []
    while True:
        e = p.parse_expr()
        if p.accept("kw", "as"):
            name = p.ident()
        else:
            assert e.kind == "attr"
            name = e.name
        items.append(O.SelectItem(e, name))
        if not p.accept("op", ","):
            break
    assert p.peek().kind == "eof"
    return items


class _Side:
    def __init__(self, stream, filters, kind, arg, alias):
        self.stream = stream
        self.alias = alias or stream
        self.filters = [_expr(f) for f in re.findall(r"\[([^\]]*)\]", filters)]
        self.kind = kind.lower()
        self.param = int(arg.strip().rstrip("lL")) if self.kind == "length" else _time_ms(arg)
        self.rows: deque = deque()       # (ts, row), arrival order
        self.max_live = 0

    def window(self, ts):
        if self.kind == "length":
            return list(self.rows)
        while self.rows and self.rows[0][0] + self.param <= ts:
            self.rows.popleft()
        return [r for r in self.rows if r[0] + self.param > ts]

    def push(self, ts, row):
        self.rows.append((ts, row))
        if self.kind == "length":
            while len(self.rows) > self.param:
                self.rows.popleft()
            self.max_live = max(self.max_live, len(self.rows))
        else:
            self.max_live = max(self.max_live, len(self.window(ts)))


class _JoinInstance:
    def __init__(self, streams: Dict[str, O.StreamDef], m):
        g = m.groups()
        self.sides = [_Side(*g[0:5]), _Side(*g[5:10])]
        self.on = _expr(g[10]) if g[10] else None
        self.select = _select(g[11])
        self.out = g[12]
        q = O.Query(kind="pattern",
                    states=[O.PState(alias=s.alias, stream=s.stream, cond=None) for s in self.sides])
        b = O.Binder(streams, q)
        for k, s in enumerate(self.sides):
            for f in s.filters:
                assert b.bind(f, "filter", cur_state=k) == O.BOOL
        if self.on is not None:
            assert b.bind(self.on, "filter", cur_state=1) == O.BOOL
        self.out_attrs = [O.Attr(it.name, b.bind(it.expr, "select")) for it in self.select]
        self.triggered = [0, 0]          # rows emitted by arrivals of each side
        self.timed = any(s.kind == "time" for s in self.sides)
        self.last_ts = None

    def on_event(self, ts, row, stream, seq, out):
        if self.timed:
            assert self.last_ts is None or ts >= self.last_ts, "a time-window join needs non-decreasing ts"
            self.last_ts = ts
        for x, side in enumerate(self.sides):
            if side.stream != stream:
                continue
            own = lambda slot: row[slot[3]]  # noqa: E731
            if not all(O.evaluate(f, own) for f in side.filters):
                return
            other = self.sides[1 - x]
            for _, r in other.window(ts):
                pair = (row, r) if x == 0 else (r, row)
                env = lambda slot: pair[slot[1]][slot[3]]  # noqa: E731
                if self.on is not None and not O.evaluate(self.on, env):
                    continue
                out.append(O.OutEvent(self.out, ts, tuple(O.evaluate(it.expr, env) for it in self.select), seq))
                self.triggered[x] += 1
            side.push(ts, row)
            return


class JoinModel:
    """send(stream, ts, row) -> [OutEvent]; join queries here, the rest on the oracle."""

    def __init__(self, plan: str):
        joins = list(_JOIN.finditer(plan))
        rest = _JOIN.sub("", plan)
        assert " join " not in rest.lower(), "join query the model's pattern does not cover: " + rest
        self.app = O.parse_app(rest)
        self.joins = [_JoinInstance(self.app.streams, m) for m in joins]
        self.rest = O.OracleRuntime(rest) if self.app.queries else None
        self.seq = 0

    def send(self, stream: str, ts: int, row):
        row = tuple(row)
        out: list = []
        seq = self.seq
        self.seq += 1
        for j in self.joins:
            j.on_event(ts, row, stream, seq, out)
        if self.rest is not None:
            out.extend(self.rest.send(stream, ts, row))
        return out


def model_run(plan: str, events: Sequence[Tuple[str, int, tuple]]):
    """events: [(stream_id, ts, row)] in arrival order ->
    ({out: [(ts, seq, data)]} as helpers.oracle_run, the model)."""
    rt = JoinModel(plan)
    out: Dict[str, List] = {}
    for sid, ts, row in events:
        for ev in rt.send(sid, ts, row):
            out.setdefault(ev.stream, []).append((ev.ts, ev.seq, ev.data))
    return out, rt
