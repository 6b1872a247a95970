"""A deliberately naive reference for the tumbling windows
`#window.lengthBatch(N)` / `#window.externalTimeBatch(c, T)` in front of an
aggregate query inside a partition (the oracle under oracle/ refuses `#`).

Per window instance (one per partition key) a plain list of the open batch's
rows.  Per kept row e, in arrival order:

  lengthBatch(N)            e joins the batch; when it holds N rows it closes,
                            e being the trigger;
  externalTimeBatch(c, T)   x = e.c.  First row of the instance: start = x,
                            end = x + T.  Otherwise, if x >= end, the batch
                            closes (trigger e, not a member) and
                            end = x + (T - ((x - start) mod T)).  Then e joins.

A closing batch replays the selector's batch rule literally: fresh aggregates,
the rows folded oldest first (count from 0, long sums wrapping to 64 bits,
float sums `acc += float(v)` from +0.0, min / max from the first row), having
evaluated after each row on the running values; the batch emits the last row
for which having held (no having: the last row), with that row's attributes,
the aggregates as of that row, that row's ts and the trigger's arrival number.
A batch that never closes never emits.

The plan is parsed by siddhi_oracle with the window clauses cut out; filters,
select items and having go through its binder and evaluator.
"""
from __future__ import annotations

import re
from typing import Dict, List, Optional, Sequence, Tuple

import siddhi_oracle as O
from window_model import _time_ms

_WINDOW = re.compile(r"#\s*window\s*\.\s*(lengthBatch|externalTimeBatch)\s*\(([^)]*)\)")
_FROM = re.compile(r"\bfrom\b", re.I)


def strip_windows(plan: str):
    """-> (plan without batch-window clauses, per query (kind, param, attr) or None)."""
    starts = [m.start() for m in _FROM.finditer(plan)]
    specs: List[Optional[Tuple[str, int, Optional[str]]]] = []
    for i, s in enumerate(starts):
        seg = plan[s:starts[i + 1] if i + 1 < len(starts) else len(plan)]
        m = _WINDOW.search(seg)
        if m is None:
            specs.append(None)
        elif m.group(1) == "lengthBatch":
            specs.append(("length", int(m.group(2).strip().rstrip("lL")), None))
        else:
            attr, t = m.group(2).split(",")
            specs.append(("time", _time_ms(t), attr.strip().split(".")[-1]))
    return _WINDOW.sub("", plan), specs


class _Fold:
    """One aggregate of one closing batch."""

    def __init__(self, name: str, t: str):
        self.name, self.t = name, t
        self.n = 0
        self.s = 0 if t == O.LONG else 0.0
        self.ext = None

    def add(self, v):
        self.n += 1
        if self.name == "sum":
            self.s = O._wrap64(self.s + v) if self.t == O.LONG else self.s + float(v)
        elif self.name == "avg":
            self.s += float(v)
        elif self.name == "min":
            self.ext = v if self.n == 1 or v < self.ext else self.ext
        elif self.name == "max":
            self.ext = v if self.n == 1 or self.ext < v else self.ext

    def value(self):
        if self.name == "count":
            return self.n
        if self.name == "sum":
            return self.s
        if self.name == "avg":
            return self.s / self.n
        return self.ext


class _BatchInstance:
    """One tumbling window: the open batch as a list of (ts, row)."""

    def __init__(self, q, spec, agg_exprs, time_col):
        self.q, self.kind, self.param = q, spec[0], spec[1]
        self.agg_exprs = agg_exprs
        self.time_col = time_col
        self.rows: list = []
        self.start = self.end = None
        # what the tests assert about their own inputs
        self.closed = self.silent = self.early = 0

    def _close(self, seq, out):
        q = self.q
        folds = [_Fold(ae.name, ae.t) for ae in self.agg_exprs]
        best = None
        for i, (ts, row) in enumerate(self.rows):
            env = lambda slot, row=row: row[slot[1]]  # noqa: E731
            for f, ae in zip(folds, self.agg_exprs):
                f.add(O.evaluate(ae.args[0], env) if ae.args else None)
            avals = {id(ae): f.value() for f, ae in zip(folds, self.agg_exprs)}
            data = tuple(O._eval_with_aggs(it.expr, env, avals) for it in q.select)
            if q.having is not None:
                def envh(slot, row=row, data=data):
                    if slot[0] == "out":
                        return data[slot[1]]
                    return row[slot[1]]
                if not O.evaluate(q.having, envh):
                    continue
            best = (i, ts, data)
        self.closed += 1
        if best is None:
            self.silent += 1
        else:
            if best[0] != len(self.rows) - 1:
                self.early += 1
            out.append(O.OutEvent(q.out, best[1], best[2], seq))
        self.rows = []

    def on_event(self, ts, row, stream, seq, out):
        q = self.q
        if stream != q.stream:
            return
        env = lambda slot: row[slot[1]]  # noqa: E731
        for f in q.filters:
            if not O.evaluate(f, env):
                return
        if self.kind == "length":
            self.rows.append((ts, row))
            if len(self.rows) == self.param:
                self._close(seq, out)
            return
        x = row[self.time_col]
        if self.start is None:
            self.start, self.end = x, x + self.param
        elif x >= self.end:
            self._close(seq, out)
            self.end = x + (self.param - ((x - self.start) % self.param))
        self.rows.append((ts, row))


class BatchWindowModel:
    """OracleRuntime with batch-window queries: send(stream, ts, row) -> [OutEvent]."""

    def __init__(self, plan: str):
        stripped, specs = strip_windows(plan)
        self.app = O.parse_app(stripped)
        assert len(specs) == len(self.app.queries), "window clause / query mismatch"
        self.specs = specs
        self.aggs: List[list] = []
        for q, spec in zip(self.app.queries, specs):
            found: list = []
            if q.kind == "single":
                for it in q.select:
                    O._agg_walk(it.expr, found)
            if spec is not None:
                assert q.partition is not None and found, "batch windows: partitioned aggregate queries only"
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
                spec = self.specs[qi]
                if spec is not None:
                    tc = self.app.streams[q.stream].index(spec[2]) if spec[2] is not None else None
                    inst = _BatchInstance(q, spec, self.aggs[qi], tc)
                elif q.kind == "single":
                    inst = O._SingleInstance(q)
                else:
                    inst = O._PatternInstance(q)
                self.instances[qi][kv] = inst
            inst.on_event(ts, row, stream, seq, out)
        return out

    def stats(self) -> Dict[str, int]:
        """Closed batches, those that emitted nothing, those whose row was not their last."""
        s = {"closed": 0, "silent": 0, "early": 0}
        for d in self.instances:
            for inst in d.values():
                if isinstance(inst, _BatchInstance):
                    s["closed"] += inst.closed
                    s["silent"] += inst.silent
                    s["early"] += inst.early
        return s


def model_run(plan: str, events: Sequence[Tuple[str, int, tuple]]):
    """events: [(stream_id, ts, row)] in arrival order ->
    ({out: [(ts, seq, data)]} as helpers.oracle_run, stats())."""
    rt = BatchWindowModel(plan)
    out: Dict[str, List] = {}
    for sid, ts, row in events:
        for ev in rt.send(sid, ts, row):
            out.setdefault(ev.stream, []).append((ev.ts, ev.seq, ev.data))
    return out, rt.stats()


# ------------------------------------------------------ known answers -------
# Hand-made answers (tests/test_batch_window_model.py checks the model against
# them, tests/test_gpu_batch_window.py the engine).  One key, ts = 1000 + 10 *
# arrival number; rows as (ts, arrival number, data).
KAT_S = "define stream S (k int, v long, c long, p double);"


def kat_part(q):
    return KAT_S + "partition with (k of S) begin " + q + " end;"


def kat_events(vs=None, cs=None, ps=None):
    n = len(vs if vs is not None else cs if cs is not None else ps)
    vs = vs if vs is not None else [0] * n
    cs = cs if cs is not None else [0] * n
    ps = ps if ps is not None else [0.0] * n
    return [("S", 1000 + 10 * i, (7, vs[i], cs[i], ps[i])) for i in range(n)]


# 1: lengthBatch(3) over v = 1..7
KAT1_PLAN = kat_part("from S#window.lengthBatch(3) select sum(v) as s, count() as n, min(v) as mn, max(v) as mx "
                     "insert into O;")
KAT1_EVENTS = kat_events(vs=list(range(1, 8)))
KAT1_ROWS = [(1020, 2, (6, 3, 1, 3)), (1050, 5, (15, 3, 4, 6))]

# 2: having picks an earlier row of the batch, or none
KAT2_PLAN = kat_part("from S#window.lengthBatch(3) select v, sum(v) as s having s < 4 insert into O;")
KAT2_EVENTS = kat_events(vs=list(range(1, 7)))
KAT2_ROWS = [(1010, 2, (2, 3))]

# 3: externalTimeBatch(c, 10): ends 110, 120, 130, 140, 150; c = 140 stays pending
KAT3_PLAN = kat_part("from S#window.externalTimeBatch(c, 10) select c, count() as n insert into O;")
KAT3_EVENTS = kat_events(cs=[100, 105, 109, 110, 125, 103, 131, 140])
KAT3_ROWS = [(1020, 3, (109, 3)), (1030, 4, (110, 1)), (1050, 6, (103, 2)), (1060, 7, (131, 1))]

# 4: fp64 folds start at +0.0 and add in arrival order
KAT4_PLAN = kat_part("from S#window.lengthBatch(2) select sum(p) as s, avg(p) as a insert into O;")
KAT4_EVENTS = kat_events(ps=[0.1, 0.7, 0.3, 0.9])
KAT4_ROWS = [(1010, 1, ((0.0 + 0.1) + 0.7, ((0.0 + 0.1) + 0.7) / 2)), (1030, 3, ((0.0 + 0.3) + 0.9, ((0.0 + 0.3) + 0.9) / 2))]
KAT4Z_PLAN = kat_part("from S#window.lengthBatch(1) select sum(p) as s, min(p) as mn insert into O;")
KAT4Z_EVENTS = kat_events(ps=[-0.0])
KAT4Z_ROWS = [(1000, 0, (0.0, -0.0))]      # compared as bits: sum +0.0, min -0.0


def bits(rows):
    """Rows with every float as its IEEE-754 bit pattern."""
    import struct
    f = lambda v: struct.pack("<d", v) if isinstance(v, float) else v  # noqa: E731
    return [(t, s, tuple(f(v) for v in d)) for t, s, d in rows]
