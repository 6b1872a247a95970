"""tests/logic_model.py (the reference of tests/test_gpu_logic.py) against
references that are no automata over partial lists, and against answers worked
out by hand.  The rules are [U] (upstream Siddhi 4.x, read from
LogicalPreStateProcessor / LogicalPostStateProcessor); each
hand-made case names the rule it assumes.

  or   relabel the g-passing B events and the h-passing C events as one stream
       M (everything else as a stream nobody reads, so arrival numbers stay):
       `every a=A[f] -> m=M` on siddhi_oracle gives the a.* columns, ts and
       arrival numbers of `every a=A[f] -> b=B[g] or c=C[h]`;
  and  per key, the partial of the A at index i completes at the first index
       t > i by which a g-passing B and an h-passing C have both occurred
       after i; its captures are the first such B and the first such C;
  and + within  the same, the expiry rule replayed event by event per partial.
"""
import numpy as np
import pytest

from flink_siddhi import workload
from helpers import oracle_run
from logic_model import model_run

DEFS = "".join("define stream %s (k int, ts long, id int, price double);" % s for s in "ABCMX")
P3 = "partition with (k of A, k of B, k of C) begin "
NAMES = ("A", "B", "C")


def three_streams(n, keys):
    w = workload.generate(0, n, keys, rate=1)
    w["stream"] = ((w["price"] * 1000).astype(np.int64) % 3).astype(np.uint8)
    return w


def events(w):
    k, ts, i, p, st = (w[c].tolist() for c in ("k", "ts", "id", "price", "stream"))
    return [(NAMES[st[j]], ts[j], (k[j], ts[j], i[j], p[j])) for j in range(len(ts))]


EV = events(three_streams(6000, 24))
F = lambda r: r[3] > 0.3          # noqa: E731  a=A[price > 0.3]
G = lambda r: r[2] % 3 == 0       # noqa: E731  b=B[id % 3 == 0]
H = lambda r: r[3] < 0.4          # noqa: E731  c=C[price < 0.4]
FGH = ("a=A[price > 0.3]", "b=B[id % 3 == 0]", "c=C[price < 0.4]")


# ---- or: one relabelled stream on the oracle ----------------------------------------------
@pytest.mark.parametrize("within", [None, 60, 200])
def test_or_equals_a_two_state_pattern_over_the_relabelled_stream(within):
    w = "" if within is None else " within %d milliseconds" % within
    got, rt = model_run(DEFS + P3 + "from every %s -> %s or %s%s select a.k as k, a.id as i, a.price as p "
                        "insert into O; end;" % (FGH + (w,)), EV)
    relabelled = [("M" if (s == "B" and G(r)) or (s == "C" and H(r)) else "A" if s == "A" else "X", ts, r)
                  for s, ts, r in EV]
    want = oracle_run(DEFS + "partition with (k of A, k of M) begin from every a=A[price > 0.3] -> m=M%s "
                      "select a.k as k, a.id as i, a.price as p insert into O; end;" % w, relabelled)
    assert len(want["O"]) > (50 if within == 60 else 500)
    assert got["O"] == want["O"]
    if within is not None:     # some partials did expire
        assert len(got["O"]) < len(model_run(DEFS + P3 + "from every %s -> %s or %s select a.k as k, a.id as i, "
                                             "a.price as p insert into O; end;" % FGH, EV)[0]["O"])


def test_or_null_side_and_captured_side():
    got, rt = model_run(DEFS + P3 + "from every %s -> %s or %s select a.id as i, b.id as bi, c.price as cp "
                        "insert into O; end;" % FGH, EV)
    rows = [d for _, _, d in got["O"]]
    assert all((bi is None) != (cp is None) for _, bi, cp in rows)
    assert any(bi is None for _, bi, _ in rows) and any(cp is None for _, _, cp in rows)
    assert all(bi is None or bi % 3 == 0 for _, bi, _ in rows) and all(cp is None or cp < 0.4 for _, _, cp in rows)


# ---- and: brute-force closed form per key ----------------------------------------------------
def closed_form_and(ev, within=None):
    """[(ts, seq, (a.id, b.id, b.ts, c.id, c.ts))] of `every a=A[F] -> b=B[G] and c=C[H]`
    from the definition above; with `within`, each partial replays the events
    of its key after its A: an event of a side's stream that is still open
    expires the partial when |ts - a.ts| > W and fills the side when the
    side's condition holds."""
    per_key = {}
    for seq, (s, ts, r) in enumerate(ev):
        per_key.setdefault(r[0], []).append((seq, s, ts, r))
    out = []
    for evs in per_key.values():
        for i, (aseq, s, ats, a) in enumerate(evs):
            if s != "A" or not F(a):
                continue
            b = c = None
            for seq, s2, ts, r in evs[i + 1:]:
                if (s2 == "B" and b is None) or (s2 == "C" and c is None):
                    if within is not None and abs(ts - ats) > within:
                        break
                    if s2 == "B" and G(r):
                        b = r
                    elif s2 == "C" and H(r):
                        c = r
                    if b is not None and c is not None:
                        out.append((seq, aseq, ts, (a[2], b[2], b[1], c[2], c[1])))
                        break
    out.sort()      # by completing event, then creation order: list order, since `and` partials keep their place
    return [(ts, seq, d) for seq, _, ts, d in out]


@pytest.mark.parametrize("within", [None, 100, 300])
def test_and_equals_the_closed_form(within):
    w = "" if within is None else " within %d milliseconds" % within
    got, rt = model_run(DEFS + P3 + "from every %s -> %s and %s%s select a.id as i, b.id as bi, b.ts as bt, "
                        "c.id as ci, c.ts as ct insert into O; end;" % (FGH + (w,)), EV)
    want = closed_form_and(EV, within)
    assert len(want) > (20 if within == 100 else 500)
    assert got["O"] == want
    assert rt.stat("half_filled_seen") > 500 and rt.stat("max_live") >= 3
    if within is not None:
        assert len(want) < len(closed_form_and(EV))


def test_parentheses_and_plain_queries():
    q = "from every %s -> %s and %s within 2 sec select a.id as i, b.id as bi, c.id as ci insert into O; end;"
    plain, _ = model_run(DEFS + P3 + q % FGH, EV)
    paren, _ = model_run(DEFS + P3 + q % (FGH[0], "(" + FGH[1], FGH[2] + ")"), EV)
    assert plain == paren and len(plain["O"]) > 20
    # a query without a logical state runs on the oracle's own instance
    chain = DEFS + P3 + "from every %s -> %s -> %s within 2 sec select a.id as i, c.id as ci insert into O; end;" % FGH
    assert model_run(chain, EV)[0] == oracle_run(chain, EV)


# ---- known answers -----------------------------------------------------------------------------
D3 = "".join("define stream %s (id int);" % s for s in "ABC")


def rows(plan, ev):
    return model_run(D3 + plan, [(s, ts, (i,)) for s, ts, i in ev])[0].get("O", [])


def test_U_rule1_first_matching_event_of_a_side_is_its_capture():
    sel = " select a.id as a, b.id as b, c.id as c insert into O;"
    ev = [("A", 0, 1), ("B", 1, 2), ("B", 2, 3), ("C", 3, 4), ("C", 4, 5), ("B", 5, 6)]
    # `and`: the second B finds its side filled; the row leaves with the first C, nothing is left for the rest
    assert rows("from every a=A -> b=B and c=C" + sel, ev) == [(3, 3, (1, 2, 4))]
    # `or`: the first event of either side completes it, the partner stays null
    assert rows("from every a=A -> b=B or c=C" + sel, ev) == [(1, 1, (1, 2, None))]
    assert rows("from every a=A -> b=B or c=C" + sel, [("A", 0, 1), ("C", 1, 9), ("B", 2, 8)]) == [(1, 1, (1, None, 9))]
    # a side whose condition fails leaves the partial as it is (rule 3)
    assert rows("from every a=A -> b=B[id > 2] and c=C" + sel, ev) == [(3, 3, (1, 3, 4))]


def test_U_rule4_half_filled_partial_keeps_its_place_in_the_list():
    plan = "from every a=A -> b=B[id > a.id] and c=C select a.id as a, b.id as b, c.id as c insert into O;"
    # partials P1 (a 5), P2 (a 1).  B 3 fills P2 only, B 9 then fills P1: were a
    # half-filled partial moved behind the ones that stayed, the list would be
    # [P2, P1] when C completes both; it keeps its place, so P1's row is first
    ev = [("A", 0, 5), ("A", 1, 1), ("B", 2, 3), ("B", 3, 9), ("C", 4, 0)]
    assert rows(plan, ev) == [(4, 4, (5, 9, 0)), (4, 4, (1, 3, 0))]


def test_U_rule6_completed_middle_position_moves_behind_the_partials_that_stayed():
    plan = ("from every a=A -> (b=B[id > a.id] or c=C[id > a.id]) -> d=A[id == 0] "
            "select a.id as a, b.id as b, c.id as c insert into O;")
    # P1 (a 5), P2 (a 1): C 3 completes P2's group only, so P2 moves behind P1;
    # B 9 completes P1's, which moves behind P2: the closing A finds [P2, P1]
    ev = [("A", 0, 5), ("A", 1, 1), ("C", 2, 3), ("B", 3, 9), ("A", 4, 0)]
    assert rows(plan, ev)[:2] == [(4, 4, (1, None, 3)), (4, 4, (5, 9, None))]


def test_U_rule2_within_exactly_W_stays_and_W_plus_1_drops():
    plan = "from every a=A -> b=B and c=C within 10 milliseconds select a.id as a, b.id as b, c.id as c insert into O;"
    assert rows(plan, [("A", 0, 1), ("B", 10, 2), ("C", 10, 3)]) == [(10, 2, (1, 2, 3))]
    assert rows(plan, [("A", 0, 1), ("B", 5, 2), ("C", 11, 3)]) == []
    # dropped, not left waiting: a late C inside the span finds nothing
    assert rows(plan, [("A", 0, 1), ("B", 5, 2), ("C", 11, 3), ("C", 9, 4)]) == []
    # checked only when an event of an open side arrives: B's side is filled, so the B at 50 expires nothing ...
    assert rows(plan, [("A", 0, 1), ("B", 5, 2), ("B", 50, 9), ("C", 9, 4)]) == [(9, 3, (1, 2, 4))]
    # ... and an event before the start counts by its distance too
    assert rows(plan, [("A", 100, 1), ("B", 89, 2), ("B", 90, 3), ("C", 100, 4)]) == []
    or_plan = plan.replace(" and ", " or ")
    assert rows(or_plan, [("A", 0, 1), ("C", 10, 3)]) == [(10, 1, (1, None, 3))]
    assert rows(or_plan, [("A", 0, 1), ("C", 11, 3), ("B", 5, 2)]) == []
