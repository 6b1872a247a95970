"""A deliberately naive reference for count states in patterns

    from [every] a=A[f] -> b=B[g]<m:n> -> c=C[h] [within W] select b[0].v, b[last].v ... insert into O;

(oracle/siddhi_oracle.py parses `<m:n>` on a pattern state and then ignores
it).  It is written the way Siddhi is built, not the way the engine's walk is
([U]: CountPreStateProcessor / CountPostStateProcessor):

  * one pending list per state: pending[s] holds the partials that await an
    event of state s.  A partial that has collected between min and max events
    at a count state s sits in pending[s] (one more of s) and in pending[s + 1]
    (the first of s + 1) at once: the two lists share the object;
  * per event, the states are processed from the last to the first, each over
    the list it had when its turn came.  A partial a state hands on lands in a
    list that has had its turn, so an event never acts twice on one partial,
    nor on the partial it created; and where a count state and its successor
    read one stream the successor is tried first;
  * a partial whose next state is filled leaves the count state's list ("next
    state already filled"), so the count state collects no more;
  * `within`: |e.ts - start.ts| > W drops the partial from every list, checked
    when e is on the stream of a state the partial awaits; exactly W stays;
  * a failed condition leaves the partial where it is;
  * reaching `min` at state s is the moment the partial is added, at the end,
    to pending[s + 1]; at the last state it emits one row with e's ts and
    arrival number and is consumed.  Reaching `max` takes it off pending[s];
  * a plain state is `<1:1>`.

Conditions and select items are parsed, bound and evaluated by siddhi_oracle's
parser, binder and evaluator (`x[i]`, `x[last]`; an index not collected is
None), the binder with the one difference _Binder states; queries without a
count state run on the oracle's own instances.
"""
from __future__ import annotations

from typing import Dict, List, Sequence, Tuple

import siddhi_oracle as O


class _Binder(O.Binder):
    """siddhi_oracle's binder with one difference: in a pattern state's own
    condition `b[i]` / `b[last]` is the event b collected before, not the
    event under test (which plain `b.x` and an unqualified `x` stay).  The
    oracle binds every form to the event under test; with a count state that
    loses `b[last]`, whose whole use is a condition over the previous event."""

    def _resolve(self, e, ctx, cur_state):
        slot, t = super()._resolve(e, ctx, cur_state)
        if self.q.kind == "pattern" and slot[0] == "st" and slot[1] == cur_state and slot[2] == "cur" \
                and e.ref is not None and e.idx is not None:
            slot = ("st", slot[1], e.idx, slot[3])
        return slot, t


def parse_app(text: str) -> O.App:
    """siddhi_oracle.parse_app (definitions, binding, output schemas) over the binder above."""
    saved = O.Binder
    O.Binder = _Binder
    try:
        return O.parse_app(text)
    finally:
        O.Binder = saved


def has_count(q: O.Query) -> bool:
    return q.kind == "pattern" and any((s.min_count, s.max_count) != (1, 1) for s in q.states)


class _Partial:
    def __init__(self, n, start_ts):
        self.j = 0                             # the state that collected last
        self.events = [[] for _ in range(n)]   # per state: [(ts, row)]
        self.start_ts = start_ts
        self.lists = set()                     # the states whose pending list holds it


class _CountInstance(O._PatternInstance):
    """One key's pending lists; conditions and emission are the oracle's
    (_cond, _emit)."""

    def __init__(self, q: O.Query):
        super().__init__(q)
        n = len(q.states)
        assert q.states[0].min_count == 1 and q.states[0].max_count == 1
        assert all(1 <= s.min_count and (s.max_count == -1 or s.min_count <= s.max_count) for s in q.states)
        self.pending: List[List[_Partial]] = [[] for _ in range(n + 1)]
        self.max_live = 0
        self.shared_seen = 0      # (event, partial) pairs: the event left the partial in two lists
        self.appended_past_min = 0

    def _add(self, s: int, p: _Partial) -> None:
        self.pending[s].append(p)
        p.lists.add(s)

    def _drop(self, s: int, p: _Partial) -> None:
        if s in p.lists:
            p.lists.discard(s)
            lst = self.pending[s]
            for i, x in enumerate(lst):
                if x is p:
                    del lst[i]
                    return

    def live(self) -> List[_Partial]:
        seen: Dict[int, _Partial] = {}
        for lst in self.pending:
            for p in lst:
                seen[id(p)] = p
        return list(seen.values())

    def on_event(self, ts, row, stream, seq, out):
        if stream not in self.streams:
            return
        q = self.q
        n = len(q.states)
        for s in range(n - 1, 0, -1):
            st = q.states[s]
            if st.stream != stream:
                continue
            for p in list(self.pending[s]):
                if s not in p.lists:
                    continue                                 # dropped from this list since its turn began
                if q.within is not None and abs(ts - p.start_ts) > q.within:
                    for k in list(p.lists):
                        self._drop(k, p)
                    continue
                if not self._cond(s, ts, row, p):
                    continue
                if s == p.j + 1:
                    self._drop(p.j, p)                       # next state already filled
                    p.j = s
                p.events[s].append((ts, row))
                c = len(p.events[s])
                self.appended_past_min += c > st.min_count
                if c == st.max_count:
                    self._drop(s, p)
                if c == st.min_count:
                    if s == n - 1:
                        self._drop(s, p)
                        self._emit(p, ts, seq, out)
                    else:
                        self._add(s + 1, p)
        s0 = q.states[0]
        if s0.stream == stream and (s0.every or not self.started) and self._cond(0, ts, row, None):
            self.started = True
            p = _Partial(n, ts)
            p.events[0].append((ts, row))
            if n == 1:
                self._emit(p, ts, seq, out)
            else:
                self._add(1, p)
        live = self.live()
        self.max_live = max(self.max_live, len(live))
        self.shared_seen += sum(len(p.lists) > 1 for p in live)


class CountModel(O.OracleRuntime):
    """send(stream, ts, row) -> [OutEvent]: pattern queries with a count state
    on _CountInstance, every other query on the oracle's own instances
    (always=True: every pattern query on _CountInstance, a plain state being
    `<1:1>`)."""

    def __init__(self, plan: str, always: bool = False):
        self.app = parse_app(plan)
        self.instances = [dict() for _ in self.app.queries]
        self.seq = 0
        self.always = always

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
                inst = (_CountInstance(q) if has_count(q) or (self.always and q.kind == "pattern") else
                        O._SingleInstance(q) if q.kind == "single" else O._PatternInstance(q))
                self.instances[qi][kv] = inst
            inst.on_event(ts, row, stream, seq, out)
        return out

    def count_instances(self) -> List[_CountInstance]:
        return [i for d in self.instances for i in d.values() if isinstance(i, _CountInstance)]

    def stat(self, name: str) -> int:
        """max_live: the most live partials one key held; shared_seen,
        appended_past_min: totals."""
        vals = [getattr(i, name) for i in self.count_instances()]
        return (max if name == "max_live" else sum)(vals) if vals else 0

    def mid_count(self) -> int:
        """Live partials that have collected at a count state and can collect more there."""
        return sum(p.j in p.lists and p.j > 0
                   for i in self.count_instances() for p in i.live())


def model_run(plan: str, events: Sequence[Tuple[str, int, tuple]], always: bool = False):
    """events: [(stream_id, ts, row)] in arrival order ->
    ({out: [(ts, seq, data)]} as helpers.oracle_run, the model)."""
    rt = CountModel(plan, always)
    out: Dict[str, List] = {}
    for sid, ts, row in events:
        for ev in rt.send(sid, ts, row):
            out.setdefault(ev.stream, []).append((ev.ts, ev.seq, ev.data))
    return out, rt
