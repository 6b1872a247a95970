"""A deliberately naive reference for event tables with a primary key

    @PrimaryKey('k') define table T (k int, ...);
    from U[f] select ... insert into T;
    from U[f] select ... update or insert into T [set ...] on T.k == k;
    from U[f] select ... update T [set ...] on T.k == k;
    from U[f] select ... delete T on T.k == k;
    from S[g] [as s] join T [as t] on s.k == t.k [and C] select ... insert into O;
    from S[g and (T.k == k) in T] select ... insert into O;

(the oracle under oracle/ refuses tables).  One dict per table, key -> row,
and per arriving row the plan's queries in plan order:

  insert            key absent: store the select row; present: drop it (the
                    first row stays) and count it in `dropped`;
  update or insert  key present: overwrite the `set` attributes (without
                    `set`: all); absent: store the select row;
  update            overwrite only when the key is present;
  delete            remove only when the key is present;
  lookup join       the table holds the stream row's key and `on` holds for
                    (stream row, that table row): one output row with the
                    stream row's ts and arrival number;
  in / not in       the conjunct is true iff the table holds the key (not).

So a reader sees the writes of earlier arrivals plus those of earlier queries
on the same row.  Filters, `on` and the select items are parsed and evaluated
by siddhi_oracle's expression parser, binder and evaluator (a join is bound as
the states of a two-state pattern are: state 0 = the stream row, state 1 = the
table row).  Every query that names no table runs on its own oracle runtime,
at its place in plan order.
"""
from __future__ import annotations

import re
from typing import Dict, List, Sequence, Tuple

import siddhi_oracle as O

_STMT = re.compile(r"\bpartition\b.*?\bend\s*;|[^;]+;", re.I | re.S)
_TABLE = re.compile(r"@\s*PrimaryKey\s*\(\s*'(\w+)'\s*\)\s*define\s+table\s+(\w+)\s*\(([^)]*)\)\s*;", re.I)
_FILTERS = r"((?:\s*\[[^\]]*\])*)"
_WRITER = re.compile(
    r"^\s*from\s+(\w+)" + _FILTERS + r"\s+select\s+(.*?)\s+"
    r"(?:(insert)\s+into\s+(\w+)|(update\s+or\s+insert)\s+into\s+(\w+)|(update)\s+(\w+)|(delete)\s+(\w+))"
    r"(?:\s+set\s+(.*?))?(?:\s+on\s+(.*?))?\s*;$", re.I | re.S)
_JOIN = re.compile(
    r"^\s*from\s+(\w+)" + _FILTERS + r"(?:\s+as\s+(\w+))?\s+(?:inner\s+)?join\s+(\w+)" + _FILTERS +
    r"(?:\s+as\s+(\w+))?\s+on\s+(.*?)\s+select\s+(.*?)\s+insert\s+(?:current\s+events\s+)?into\s+(\w+)\s*;$",
    re.I | re.S)
_SINGLE = re.compile(r"^\s*from\s+(\w+)" + _FILTERS + r"\s+select\s+(.*?)\s+insert\s+into\s+(\w+)\s*;$", re.I | re.S)


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


def _conjuncts(text: str) -> List[str]:
    """Top-level `and` conjuncts of a condition."""
    out, depth, start = [], 0, 0
    for m in re.finditer(r"[()]|\band\b", text, re.I):
        if m.group(0) == "(":
            depth += 1
        elif m.group(0) == ")":
            depth -= 1
        elif depth == 0:
            out.append(text[start:m.start()].strip())
            start = m.end()
    out.append(text[start:].strip())
    return out


class _Table:
    def __init__(self, name, pk, attrs):
        self.name, self.attrs = name, attrs          # attrs: [(name, type)]
        self.names = [a for a, _ in attrs]
        self.pk = self.names.index(pk)
        self.rows: Dict[int, list] = {}
        self.dropped = 0


class _Op:
    """One query that names a table."""

    def __init__(self, streams, tables, stmt):
        self.out = None
        m = _JOIN.match(stmt)
        if m and (m.group(1) in tables or m.group(4) in tables):
            g = m.groups()
            t_first = g[0] in tables
            sname, sfil, salias = (g[3], g[4], g[5]) if t_first else (g[0], g[1], g[2])
            tname, talias = (g[0], g[2]) if t_first else (g[3], g[5])
            self.kind, self.stream, self.table = "join", sname, tables[tname]
            self.filters = [_expr(f) for f in re.findall(r"\[([^\]]*)\]", sfil)]
            self.on = _expr(g[6])
            self.select = _select(g[7])
            self.out = g[8]
            q = O.Query(kind="pattern", states=[O.PState(alias=salias or sname, stream=sname, cond=None),
                                                O.PState(alias=talias or tname, stream=tname, cond=None)])
            b = O.Binder(streams, q)
            for f in self.filters:
                assert b.bind(f, "filter", cur_state=0) == O.BOOL
            assert b.bind(self.on, "filter", cur_state=1) == O.BOOL
            for it in self.select:
                b.bind(it.expr, "select")
            # the stream attribute that `on` equates with the primary key
            pk = self.table.names[self.table.pk]
            keys = []
            for c in _conjuncts(g[6]):
                mm = re.fullmatch(r"(\w+)\.(\w+)\s*==\s*(\w+)\.(\w+)", c)
                if not mm:
                    continue
                for (r1, a1, r2, a2) in (mm.groups(), mm.groups()[2:] + mm.groups()[:2]):
                    if r1 == (talias or tname) and a1 == pk and r2 == (salias or sname):
                        keys.append(a2)
            assert len(keys) == 1, "one key equality expected in: " + g[6]
            self.key = streams[sname].index(keys[0])
            return
        m = _WRITER.match(stmt)
        if m and any(x in tables for x in (m.group(5), m.group(7), m.group(9), m.group(11))):
            g = m.groups()
            self.stream = g[0]
            self.kind = "insert" if g[3] else "upsert" if g[5] else "update" if g[7] else "delete"
            self.table = tables[g[4] or g[6] or g[8] or g[10]]
            self.filters = [_expr(f) for f in re.findall(r"\[([^\]]*)\]", g[1])]
            self.select = _select(g[2])
            q = O.Query(kind="pattern", states=[O.PState(alias=self.stream, stream=self.stream, cond=None)])
            b = O.Binder(streams, q)
            for f in self.filters:
                assert b.bind(f, "filter", cur_state=0) == O.BOOL
            for it in self.select:
                b.bind(it.expr, "filter", cur_state=0)
            names = [it.name for it in self.select]
            T = self.table
            pk = T.names[T.pk]
            if self.kind == "insert":
                self.key = T.pk
            else:
                mm = re.fullmatch(r"\s*(?:%s\.%s\s*==\s*(\w+)|(\w+)\s*==\s*%s\.%s)\s*" % (T.name, pk, T.name, pk), g[12])
                assert mm, "`on` must be the key equality: " + str(g[12])
                self.key = names.index(mm.group(1) or mm.group(2))
            # table attribute -> select item, for a stored row and for an overwrite
            self.ins = [w for w in range(len(T.names))] if self.kind in ("insert", "upsert") else None
            if g[11]:
                self.set = {}
                for part in g[11].split(","):
                    mm = re.fullmatch(r"\s*(?:%s\.)?(\w+)\s*=\s*(\w+)\s*" % T.name, part)
                    self.set[T.names.index(mm.group(1))] = names.index(mm.group(2))
            elif self.kind in ("upsert", "update"):
                self.set = {w: names.index(n) for w, n in enumerate(T.names)}
            return
        m = _SINGLE.match(stmt)
        assert m, "table query the model does not cover: " + stmt
        g = m.groups()
        self.kind, self.stream, self.out = "in", g[0], g[3]
        conj = []
        for f in re.findall(r"\[([^\]]*)\]", g[1]):
            conj.extend(_conjuncts(f))
        own, found = [], []
        for c in conj:
            mm = re.fullmatch(r"(not\s*\(\s*)?\(\s*(\w+)\.(\w+)\s*==\s*(\w+)\s*\)\s*in\s+(\w+)\s*(\))?", c, re.I)
            if mm:
                assert bool(mm.group(1)) == bool(mm.group(6))
                found.append(mm)
            else:
                own.append(c)
        assert len(found) == 1, "one `in` conjunct expected: " + stmt
        mm = found[0]
        self.table = tables[mm.group(5)]
        assert mm.group(2) == self.table.name and mm.group(3) == self.table.names[self.table.pk]
        self.negate = bool(mm.group(1))
        self.key = streams[self.stream].index(mm.group(4))
        self.filters = [_expr(c) for c in own]
        if g[2].strip() == "*":
            self.select = _select(", ".join(a.name for a in streams[self.stream].attrs))
        else:
            self.select = _select(g[2])
        q = O.Query(kind="pattern", states=[O.PState(alias=self.stream, stream=self.stream, cond=None)])
        b = O.Binder(streams, q)
        for f in self.filters:
            assert b.bind(f, "filter", cur_state=0) == O.BOOL
        for it in self.select:
            b.bind(it.expr, "filter", cur_state=0)

    def on_event(self, ts, row, stream, seq, out):
        if stream != self.stream:
            return
        own = lambda slot: row[slot[3]]  # noqa: E731
        if not all(O.evaluate(f, own) for f in self.filters):
            return
        T = self.table
        if self.kind == "join":
            trow = T.rows.get(row[self.key])
            if trow is None:
                return
            pair = (row, tuple(trow))
            env = lambda slot: pair[slot[1]][slot[3]]  # noqa: E731
            if O.evaluate(self.on, env):
                out.append(O.OutEvent(self.out, ts, tuple(O.evaluate(it.expr, env) for it in self.select), seq))
            return
        if self.kind == "in":
            if (row[self.key] in T.rows) != self.negate:
                out.append(O.OutEvent(self.out, ts, tuple(O.evaluate(it.expr, own) for it in self.select), seq))
            return
        sel = [O.evaluate(it.expr, own) for it in self.select]
        key = sel[self.key]
        if self.kind == "delete":
            T.rows.pop(key, None)
        elif key in T.rows:
            if self.kind == "insert":
                T.dropped += 1
            else:
                for w, i in self.set.items():
                    T.rows[key][w] = sel[i]
        elif self.kind in ("insert", "upsert"):
            T.rows[key] = [sel[w] for w in self.ins]


class TableModel:
    """send(stream, ts, row) -> [OutEvent]; table_rows(T) -> rows by key."""

    def __init__(self, plan: str):
        stmts = [s.strip() for s in _STMT.findall(plan)]
        defs = [s for s in stmts if re.match(r"define\s+stream\b", s, re.I)]
        self.tables: Dict[str, _Table] = {}
        for s in stmts:
            m = _TABLE.match(s)
            if m:
                attrs = [tuple(a.split()) for a in m.group(3).split(",")]
                self.tables[m.group(2)] = _Table(m.group(2), m.group(1), attrs)
        # tables bind like streams of their attributes
        tdefs = ["define stream %s (%s);" % (t.name, ", ".join("%s %s" % a for a in t.attrs)) for t in self.tables.values()]
        streams = O.parse_app("".join(defs + tdefs)).streams
        self.queries = []            # plan order: _Op or an oracle runtime of one query
        for s in stmts:
            if s in defs or _TABLE.match(s):
                continue
            names = set(re.findall(r"\w+", s))
            if names & set(self.tables):
                self.queries.append(_Op(streams, self.tables, s))
            else:
                self.queries.append(O.OracleRuntime("".join(defs) + s))
        self.seq = 0

    def send(self, stream: str, ts: int, row):
        row = tuple(row)
        out: list = []
        seq = self.seq
        self.seq += 1
        for q in self.queries:
            if isinstance(q, _Op):
                q.on_event(ts, row, stream, seq, out)
            else:
                out.extend(q.send(stream, ts, row))
        return out

    def table_rows(self, name: str) -> List[tuple]:
        return [tuple(r) for _, r in sorted(self.tables[name].rows.items())]

    def dropped(self) -> int:
        return sum(t.dropped for t in self.tables.values())


def model_run(plan: str, events: Sequence[Tuple[str, int, tuple]]):
    """events: [(stream_id, ts, row)] in arrival order ->
    ({out: [(ts, seq, data)]} as helpers.oracle_run, the model)."""
    rt = TableModel(plan)
    out: Dict[str, List] = {}
    for sid, ts, row in events:
        for ev in rt.send(sid, ts, row):
            out.setdefault(ev.stream, []).append((ev.ts, ev.seq, ev.data))
    return out, rt
