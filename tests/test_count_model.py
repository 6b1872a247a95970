"""tests/count_model.py, the reference for count states in patterns (DESIGN
§14), checked three ways on the CPU: against oracle/siddhi_oracle.py where
every count is `<1>` / `<1:1>`, against a closed form that is no automaton for
`every a=A[f] -> b=B[g]<m:n> -> c=C[h]` (and, with `within`, against one
partial replayed on its own), and against answers worked out by hand."""
import random

import pytest

import siddhi_oracle as O
from count_model import CountModel, model_run

EV = "".join("define stream %s (k int, id int, v int);" % s for s in "ABCD")
P3 = "partition with (k of A, k of B, k of C) begin "


def gen(n=3000, keys=5, seed=7, step=3):
    rnd = random.Random(seed)
    ts, out = 1000, []
    for i in range(n):
        ts += rnd.randrange(0, step)
        out.append(("ABC"[rnd.randrange(3)], ts, (rnd.randrange(keys), i, rnd.randrange(10))))
    return out


def oracle_rows(plan, events):
    rt = O.OracleRuntime(plan)
    return [(e.ts, e.seq, e.data) for sid, ts, row in events for e in rt.send(sid, ts, row)]


# ---- against the oracle: `<1>` is a plain state ------------------------------------------------
ONES = [
    ("from every a=A[v > 2] -> b=B[v > a.v]%s -> c=C[v < b.v]%s within 40 milliseconds "
     "select a.id as ai, b.id as bi, b[last].id as bl, c.id as ci insert into O;"),
    ("from every a=A -> b=B%s -> c=B[v > b.v]%s -> d=C select a.id as ai, b.id as bi, c.id as ci, d.id as di "
     "insert into O;"),
    "from a=A[v == 4] -> b=B[v == 5]%s -> c=C%s select a.id as ai, b[0].id as bi, c[last].id as ci insert into O;",
    "from every a=A[v > 5] -> b=B[v < a.v]%s within 25 milliseconds select a.id as ai, b.id as bi insert into O;",
]


@pytest.mark.parametrize("partitioned", [False, True])
@pytest.mark.parametrize("q", ONES)
@pytest.mark.parametrize("one", [("<1>", "<1:1>"), ("<1:1>", "")])
def test_count_of_one_is_the_oracles_pattern(q, one, partitioned):
    wrap = (lambda s: EV + P3 + s + " end;") if partitioned else (lambda s: EV + s)
    events = gen()
    holes = q.count("%s")
    want = oracle_rows(wrap(q % ("", "")[:holes]), events)
    got, m = model_run(wrap(q % one[:holes]), events, always=True)
    assert m.count_instances() and len(want) > (0 if "from a=A" in q else 50)
    assert got.get("O", []) == want


# ---- against a closed form ---------------------------------------------------------------------
def f(row): return row[2] > 3           # a: v > 3
def g(row): return row[2] % 3 != 0      # b: v % 3 != 0
def h(row): return row[2] < 4           # c: v < 4


CF = ("from every a=A[v > 3] -> b=B[v %% 3 != 0]<%s> -> c=C[v < 4] %s"
      "select a.id as ai, b[0].id as b0, b[1].id as b1, b[2].id as b2, b[last].id as bl, c.id as ci insert into O;")


def closed_form(events, m, n, keyed, within=None):
    """Per start event: the closing c is the first h-passing C after the m-th
    g-passing B, the collected B's are the first min(n, .) g-passing B's before
    it.  Rows of one closing event come out in the order the partials reached
    m (the order they were handed to c's list), then in start order.  With
    `within` each partial is replayed on its own: an event of a stream it
    awaits (B while it holds fewer than n, C from the m-th B on) that is more
    than W from the start drops it."""
    rows = []
    for ia, (sid, ts0, ra) in enumerate(events):
        if sid != "A" or not f(ra):
            continue
        bs, close = [], None
        for i in range(ia + 1, len(events)):
            sid2, ts, r = events[i]
            if keyed and r[0] != ra[0]:
                continue
            wait_b = n < 0 or len(bs) < n
            wait_c = len(bs) >= m
            if within is not None and ((sid2 == "B" and wait_b) or (sid2 == "C" and wait_c)) and abs(ts - ts0) > within:
                break
            if sid2 == "C" and wait_c and h(r):
                close = i
                break
            if sid2 == "B" and wait_b and g(r):
                bs.append(i)
        if close is None:
            continue
        ids = [events[b][2][1] for b in bs]
        at = lambda x: ids[x] if x < len(ids) else None      # noqa: E731
        rows.append(((close, bs[m - 1], ia), (events[close][1], close, (ra[1], at(0), at(1), at(2), ids[-1], events[close][2][1]))))
    return [r for _, r in sorted(rows)]


@pytest.mark.parametrize("keyed", [False, True])
@pytest.mark.parametrize("m,n", [(1, 1), (2, 2), (2, 4), (1, 3), (3, -1), (2, -1), (4, 6)])
def test_against_the_closed_form(m, n, keyed):
    cnt = "%d:%s" % (m, "" if n < 0 else n) if m != n else str(m)
    q = CF % (cnt, "")
    plan = EV + (P3 + q + " end;" if keyed else q)
    events = gen(2500 if keyed else 700, keys=5)
    want = closed_form(events, m, n, keyed)
    got, mod = model_run(plan, events, always=True)
    assert len(want) > 100
    assert got["O"] == want
    if n != m:
        assert mod.stat("appended_past_min") > 0 and mod.stat("shared_seen") > 0
        assert any(d[4] != d[1] for _, _, d in want)


@pytest.mark.parametrize("keyed", [False, True])
@pytest.mark.parametrize("m,n,w", [(2, 4, 30), (2, -1, 60), (3, 3, 45), (1, 2, 12)])
def test_against_one_partial_replayed_with_expiry(m, n, w, keyed):
    cnt = "%d:%s" % (m, "" if n < 0 else n) if m != n else str(m)
    q = CF % (cnt, "within %d milliseconds " % w)
    plan = EV + (P3 + q + " end;" if keyed else q)
    events = gen(2500 if keyed else 700, keys=3 if keyed else 1, step=4)
    want = closed_form(events, m, n, keyed, within=w)
    got, _ = model_run(plan, events)
    assert 20 < len(want) < len(closed_form(events, m, n, keyed))      # some expired, some did not
    assert got["O"] == want


# ---- by hand -----------------------------------------------------------------------------------
def rows(plan, evs):
    """evs: [(stream, ts, id, v)], k = 0; -> [(ts, seq, data)]"""
    got, _ = model_run(EV + plan, [(s, ts, (0, i, v)) for s, ts, i, v in evs])
    return got.get("O", [])


def test_next_state_first_on_a_shared_stream():
    plan = ("from every a=A -> b=B[v > 0]<1:3> -> c=B[v > 5] "
            "select a.id as ai, b[0].id as b0, b[last].id as bl, c.id as ci insert into O;")
    # B 11 passes both conditions: it closes the match, it is not collected by b
    assert rows(plan, [("A", 1, 1, 0), ("B", 2, 10, 1), ("B", 3, 11, 9), ("B", 4, 12, 9)]) == [(3, 2, (1, 10, 10, 11))]
    # B 10 passes c's condition too, but c is not awaited before b has its min
    assert rows(plan, [("A", 1, 1, 0), ("B", 2, 10, 9), ("B", 3, 11, 1), ("B", 4, 12, 9)]) == [(4, 3, (1, 10, 11, 12))]


PLACE = ("from every a=A -> b=B[v >= a.v]<2:4> -> c=C "
         "select a.id as ai, b[0].id as b0, b[last].id as bl, c.id as ci insert into O;")


def test_a_partial_keeps_its_place_between_min_and_max():
    # list [P1, P2]; B 11 brings P1 to min: [P2, P1]; B 12 brings P2 to min
    # (it moves behind) and P1 to 3 (it keeps its place): [P1, P2]
    evs = [("A", 1, 1, 0), ("A", 2, 2, 5), ("B", 3, 10, 5), ("B", 4, 11, 0), ("B", 5, 12, 5), ("C", 6, 20, 0)]
    assert rows(PLACE, evs) == [(6, 5, (1, 10, 12, 20)), (6, 5, (2, 10, 12, 20))]


def test_a_partial_moves_behind_exactly_at_min():
    # P2 reaches min at B 11 and then collects to its max; P1 reaches min at
    # B 13 and moves behind P2, which keeps its place: [P2, P1]
    evs = [("A", 1, 1, 5), ("A", 2, 2, 0), ("B", 3, 10, 0), ("B", 4, 11, 0), ("B", 5, 12, 5), ("B", 6, 13, 5),
           ("B", 7, 14, 5), ("C", 8, 20, 0)]
    assert rows(PLACE, evs) == [(8, 7, (2, 10, 13, 20)), (8, 7, (1, 12, 14, 20))]


def test_a_last_count_state_emits_once_at_min():
    plan = "from every a=A -> b=B<2:4> select a.id as ai, b[0].id as b0, b[1].id as b1, b[last].id as bl insert into O;"
    evs = [("A", 1, 1, 0), ("B", 2, 10, 0), ("B", 3, 11, 0), ("B", 4, 12, 0), ("B", 5, 13, 0), ("B", 6, 14, 0)]
    assert rows(plan, evs) == [(3, 2, (1, 10, 11, 11))]
    # the two-position form with an unbounded count, two starts
    plan = "from every a=A -> b=B<3:> select a.id as ai, b[0].id as b0, b[2].id as b2, b[last].id as bl insert into O;"
    evs = [("A", 1, 1, 0), ("B", 2, 10, 0), ("A", 3, 2, 0), ("B", 4, 11, 0), ("B", 5, 12, 0), ("B", 6, 13, 0),
           ("B", 7, 14, 0)]
    assert rows(plan, evs) == [(5, 4, (1, 10, 12, 12)), (6, 5, (2, 11, 13, 13))]


def test_two_consecutive_count_states():
    plan = ("from every a=A -> b=B<2:3> -> c=C<2:2> -> d=D select a.id as ai, b[0].id as b0, b[last].id as bl, "
            "b[2].id as b2, c[0].id as c0, c[last].id as cl, d.id as di insert into O;")
    # C 20 fills c's first: b collects no more (B 12 is ignored); C 22 is past c's max
    evs = [("A", 1, 1, 0), ("B", 2, 10, 0), ("C", 3, 19, 0), ("B", 4, 11, 0), ("C", 5, 20, 0), ("B", 6, 12, 0),
           ("D", 7, 29, 0), ("C", 8, 21, 0), ("C", 9, 22, 0), ("D", 10, 30, 0), ("D", 11, 31, 0)]
    assert rows(plan, evs) == [(10, 9, (1, 10, 11, None, 20, 21, 30))]


def test_exactly_w_and_w_plus_one():
    plan = ("from every a=A -> b=B<2:3> -> c=C within 10 milliseconds "
            "select a.id as ai, b[last].id as bl, c.id as ci insert into O;")
    assert rows(plan, [("A", 100, 1, 0), ("B", 101, 10, 0), ("B", 102, 11, 0), ("C", 110, 20, 0)]) == \
        [(110, 3, (1, 11, 20))]
    # W + 1 drops the partial: the C at exactly W that arrives after it finds nothing
    assert rows(plan, [("A", 100, 1, 0), ("B", 101, 10, 0), ("B", 102, 11, 0), ("C", 111, 20, 0),
                       ("C", 110, 21, 0)]) == []
    # a B past W drops a partial that could still collect, whatever its condition says
    plan2 = plan.replace("b=B<2:3>", "b=B[v > 0]<2:3>")
    assert rows(plan2, [("A", 100, 1, 0), ("B", 101, 10, 1), ("B", 102, 11, 1), ("B", 111, 12, 0),
                        ("C", 105, 20, 0)]) == []
    # at its max the partial no longer awaits B: the late B leaves it alone
    assert rows(plan2.replace("<2:3>", "<2:2>"), [("A", 100, 1, 0), ("B", 101, 10, 1), ("B", 102, 11, 1),
                                                  ("B", 111, 12, 0), ("C", 105, 20, 0)]) == [(105, 4, (1, 11, 20))]


def test_a_condition_over_the_events_collected_before():
    plan = ("from every a=A -> b=B[not (b[last].v >= v) and not (v == b[0].v + 1)]<2:3> -> c=C "
            "select a.id as ai, b[0].id as b0, b[last].id as bl, c.id as ci insert into O;")
    # B 10: nothing collected, b[last] and b[0] are null, both comparisons fail: taken.  B 11 does not
    # rise, B 12 is b[0].v + 1, B 13 is taken
    evs = [("A", 1, 1, 0), ("B", 2, 10, 5), ("B", 3, 11, 3), ("B", 4, 12, 6), ("B", 5, 13, 8), ("C", 6, 20, 0)]
    assert rows(plan, evs) == [(6, 5, (1, 10, 13, 20))]


def test_model_runs_plain_queries_on_the_oracle():
    plan = EV + "from every a=A[v > 2] -> b=B[v > a.v] select a.id as ai, b.id as bi insert into O;"
    events = gen(500)
    m = CountModel(plan)
    got = [(e.ts, e.seq, e.data) for sid, ts, row in events for e in m.send(sid, ts, row)]
    assert not m.count_instances() and got == oracle_rows(plan, events) and len(got) > 20
