"""A deliberately naive reference for logical pattern states

    from [every] a=A[f] -> b=B[g] and c=C[h] [-> ...] [within W] select ... insert into O;
    from [every] a=A[f] -> (b=B[g] or c=C[h]) [-> ...] [within W] select ... insert into O;

(oracle/siddhi_oracle.py does not parse them).  A position after the first may
be a group of two sides; each side is an ordinary state.  One list of partials
per partition key, and per event e of a stream the query reads, in arrival
order, over the key's partials in list order ([U]):

  1. a partial waiting at a logical position reacts to e only if e's stream is
     the stream of a side that is not yet filled (the first matching event of
     a side is its capture; a filled side ignores later events);
  2. `within`: |e.ts - start.ts| > W drops the partial, exactly W stays;
  3. the side's condition fails: the partial stays as it is;
  4. `and`, condition holds: the side is captured and marked filled; with the
     partner filled too the position is complete, otherwise the partial keeps
     its place in the list and waits for the partner only;
  5. `or`, condition holds: the side is captured, the position is complete,
     the partner's captures stay null (None here);
  6. a complete position is a matched plain state: the last one emits a row
     with e's ts and arrival number and consumes the partial, any other moves
     the partial behind the partials that stayed;
  7. the rest is the plain pattern: an event never advances a partial it
     created, `every` on the start creates one partial per start event,
     matches of one event come out in list order.

Conditions and select items are parsed, bound and evaluated by siddhi_oracle's
expression parser, binder and evaluator; queries without a logical state run
on the oracle's own instances.
"""
from __future__ import annotations

from typing import Dict, List, Sequence, Tuple

import siddhi_oracle as O


class _Parser(O.Parser):
    """siddhi_oracle's parser with one more production: a pattern position may
    be `x=X[f] and y=Y[g]` / `x=X[f] or y=Y[g]`, in parentheses or not.  The
    two sides become consecutive states; the first carries `logic`."""

    def _position(self) -> List[O.PState]:
        paren = bool(self.accept("op", "("))
        s = self.parse_state()
        s.logic = None
        out = [s]
        t = self.peek()
        if t.kind == "kw" and t.val in ("and", "or"):
            self.next()
            s.logic = t.val
            y = self.parse_state()
            y.logic = None
            out.append(y)
        if paren:
            self.expect("op", ")")
        return out

    def _is_state_elem(self) -> bool:
        return super()._is_state_elem() or (self.peek().kind == "op" and self.peek().val == "(")

    def parse_input(self) -> O.Query:
        if not self._is_state_elem():
            return super().parse_input()
        states = self._position()
        sep = None
        while self.peek().kind == "op" and self.peek().val in ("->", ","):
            v = self.next().val
            assert sep in (None, v), "mixing -> and ,"
            sep = v
            states += self._position()
        q = O.Query(kind="pattern" if sep in (None, "->") else "sequence", states=states)
        if self.accept("kw", "within"):
            q.within = self.parse_time()
        logical = any(s.logic for s in states)
        assert not (logical and (q.kind == "sequence" or states[0].logic)), "logical group first / in a sequence"
        for k, s in enumerate(states):
            assert not (s.every and k != 0), "every on a non-start state"
            assert not logical or (s.min_count, s.max_count) == (1, 1), "count state in a logical pattern"
        return q


def parse_app(text: str) -> O.App:
    """siddhi_oracle.parse_app (definitions, binding, output schemas) over the
    parser above."""
    saved = O.Parser
    O.Parser = _Parser
    try:
        return O.parse_app(text)
    finally:
        O.Parser = saved


def is_logical(q: O.Query) -> bool:
    return q.kind == "pattern" and any(getattr(s, "logic", None) for s in q.states)


class _Partial:
    def __init__(self, j, filled, events, start_ts):
        self.j = j                 # elementary state awaited (first side of a logical position)
        self.filled = filled       # sides of that position already captured
        self.events = events       # per elementary state: [(ts, row)] (at most one)
        self.start_ts = start_ts


class _LogicInstance(O._PatternInstance):
    """One key's list of partials; conditions and emission are the oracle's
    (_cond, _emit), the transition is rules 1-7 above."""

    def __init__(self, q: O.Query):
        super().__init__(q)
        self.max_live = 0
        self.half_filled_seen = 0      # events that left an `and` partial half filled
        self.null_rows = 0

    def on_event(self, ts, row, stream, seq, out):
        if stream not in self.streams:
            return
        q = self.q
        n = len(q.states)
        keep: List[_Partial] = []
        moved: List[_Partial] = []
        for p in self.partials:
            first = q.states[p.j]
            sides = [p.j, p.j + 1] if first.logic else [p.j]
            # rule 1: the open side of e's stream, if any
            hit = [s for s in sides if q.states[s].stream == stream and s not in p.filled]
            if not hit:
                keep.append(p)
                continue
            s = hit[0]
            if q.within is not None and abs(ts - p.start_ts) > q.within:
                continue                                   # rule 2: dropped
            if not self._cond(s, ts, row, p):
                keep.append(p)                             # rule 3
                continue
            evs = [list(x) for x in p.events]
            evs[s].append((ts, row))
            filled = p.filled | {s}
            if first.logic == "and" and len(filled) < 2:
                keep.append(_Partial(p.j, filled, evs, p.start_ts))   # rule 4: keeps its place
                self.half_filled_seen += 1
                continue
            nxt = p.j + len(sides)                         # rules 4 (both filled), 5, and plain states
            done = _Partial(nxt, frozenset(), evs, p.start_ts)
            if nxt == n:
                self.null_rows += any(not e for e in evs)
                self._emit(done, ts, seq, out)             # rule 6: consumed
            else:
                moved.append(done)
        s0 = q.states[0]
        if s0.stream == stream and (s0.every or not self.started) and self._cond(0, ts, row, None):
            self.started = True
            evs = [[] for _ in range(n)]
            evs[0].append((ts, row))
            if n == 1:
                self._emit(_Partial(1, frozenset(), evs, ts), ts, seq, out)
            else:
                moved.append(_Partial(1, frozenset(), evs, ts))
        self.partials = keep + moved
        self.max_live = max(self.max_live, len(self.partials))


class LogicModel(O.OracleRuntime):
    """send(stream, ts, row) -> [OutEvent]: queries with a logical state on
    _LogicInstance, every other query on the oracle's own instances."""

    def __init__(self, plan: str):
        self.app = parse_app(plan)
        self.instances = [dict() for _ in self.app.queries]
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
                inst = (_LogicInstance(q) if is_logical(q) else
                        O._SingleInstance(q) if q.kind == "single" else O._PatternInstance(q))
                self.instances[qi][kv] = inst
            inst.on_event(ts, row, stream, seq, out)
        return out

    def stat(self, name: str) -> int:
        """max / sum over every logical instance of a counter (max_live:
        the longest list; half_filled_seen, null_rows: totals)."""
        vals = [getattr(i, name) for d in self.instances for i in d.values() if isinstance(i, _LogicInstance)]
        return (max if name == "max_live" else sum)(vals) if vals else 0


def model_run(plan: str, events: Sequence[Tuple[str, int, tuple]]):
    """events: [(stream_id, ts, row)] in arrival order ->
    ({out: [(ts, seq, data)]} as helpers.oracle_run, the model)."""
    rt = LogicModel(plan)
    out: Dict[str, List] = {}
    for sid, ts, row in events:
        for ev in rt.send(sid, ts, row):
            out.setdefault(ev.stream, []).append((ev.ts, ev.seq, ev.data))
    return out, rt
