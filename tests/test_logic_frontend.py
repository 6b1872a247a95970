"""Logical pattern states in the front end (cep_validate / cep_plan_schema: no
device): `A -> B and C`, `A -> (B or C) -> D`.  Every accepted form, the
output schema of an `or` plan, every refusal with a message that names the
construct, and `not` at a state position as a named refusal instead of a
parse error."""
import pytest

import flink_siddhi as fs

ABC = "".join("define stream %s (k int, ts long, id int, price double, name string);" % s for s in "ABC")
SEL = " select a.id as x, b.price as y, c.price as z insert into O;"


def part(q):
    return "partition with (k of A, k of B, k of C) begin " + q + " end;"


ACCEPTED = [
    # a group at the end, with and without parentheses, with and without `within` / `every` / a partition
    "from every a=A[id > 3] -> b=B[price > 0.2] and c=C[price < 0.9] within 5 sec" + SEL,
    "from every a=A[id > 3] -> (b=B[price > 0.2] and c=C[price < 0.9]) within 5 sec" + SEL,
    "from every a=A -> b=B or c=C" + SEL,
    "from a=A -> (b=B or c=C) within 10 milliseconds" + SEL,
    part("from every a=A[id > 3] -> b=B and c=C[id != 4] within 5 sec" + SEL),
    # a group in the middle
    "from every a=A[id > 3] -> (b=B[price > 0.2] or c=C[price < 0.9]) -> d=A[id > a.id] "
    "select a.id as x, b.price as y, c.price as z, d.id as w insert into O;",
    "from every a=A -> b=B and c=C -> d=A[id > a.id and price > b.price] "
    "select a.id as x, b.price as y, c.price as z, d.id as w insert into O;",
    # two groups: six elementary states
    "from every a=A -> (b=B and c=C) -> d=A -> (e=B or f=C) "
    "select a.id as x, b.id as y, c.id as z, d.id as w, e.name as n, f.id as v insert into O;",
    # side conditions reading earlier captures; `and` / `or` inside [...] stay expression operators
    "from every a=A -> b=B[id > a.id and price > 0.1 or id == 0] and c=C[price < a.price or id == 1]" + SEL,
    "from every a=A -> b=B[price > a.price] or c=C[not (id > a.id)] within 1 sec" + SEL,
    # a STRING capture of an `or` side
    "from every a=A -> b=B or c=C select a.id as x, b.name as bn, c.name as cn insert into O;",
]


@pytest.mark.parametrize("plan", ACCEPTED)
def test_accepted(plan):
    fs.validate(ABC + plan)


def test_parentheses_change_nothing():
    """The two spellings of one group give the same output schema."""
    a, b = ACCEPTED[0], ACCEPTED[1]
    assert fs.plan_schema(ABC + a, "O") == fs.plan_schema(ABC + b, "O")


def test_or_plan_schema():
    plan = ABC + ("from every a=A -> b=B or c=C within 1 sec "
                  "select a.k as k, b.price as bp, c.price as cp, b.name as bn, c.id as ci insert into O;")
    assert fs.plan_schema(plan, "O") == [("k", "int"), ("bp", "double"), ("cp", "double"), ("bn", "string"),
                                        ("ci", "int")]


def test_plans_without_a_group_parse_as_before():
    for q in ("from every a=A[id > 3 and price < 0.5 or id == 0] -> b=B[not (id > a.id) and price > 0.1] "
              "select a.id as x, b.id as y insert into O;",
              "from every a=A, b=B[id > 1 or id < 0]+, c=C select a.id as x, b[last].id as y, c.id as z insert into O;"):
        fs.validate(ABC + q)


REFUSED = [
    # a logical group as the first position
    ("from a=A and b=B -> c=C" + SEL, "first pattern position"),
    ("from (a=A or b=B) -> c=C" + SEL, "first pattern position"),
    ("from every (a=A and b=B) -> c=C" + SEL, "first pattern position"),
    ("from a=A and b=B select a.id as x, b.id as y insert into O;", "first pattern position"),
    # in a sequence
    ("from every a=A, b=B and c=C" + SEL, "in a sequence"),
    ("from every a=A, (b=B or c=C)" + SEL, "in a sequence"),
    # more than two sides, mixed operators
    ("from every a=A -> b=B and c=C and d=A select a.id as x insert into O;", "more than two sides"),
    ("from every a=A -> (b=B or c=C or d=A) select a.id as x insert into O;", "more than two sides"),
    ("from every a=A -> b=B and c=C or d=A select a.id as x insert into O;", "mixing 'and' and 'or'"),
    # two sides on one stream
    ("from every a=A -> b=B[id > 1] and c=B[id < 1]" + SEL, "read the same stream"),
    ("from every a=A -> b=B or c=B" + SEL, "read the same stream"),
    # a side reading its partner
    ("from every a=A -> b=B and c=C[price > b.price]" + SEL, "partner's capture"),
    ("from every a=A -> b=B[price > c.price] and c=C" + SEL, "partner's capture"),
    ("from every a=A -> b=B or c=C[id == b.id]" + SEL, "partner's capture"),
    # a later condition reading an `or` side, which may be null
    ("from every a=A -> (b=B or c=C) -> d=A[id > b.id] select a.id as x, d.id as w insert into O;",
     "capture of an 'or' side"),
    ("from every a=A -> (b=B or c=C) -> d=A -> e=B[price > c.price] select a.id as x, e.id as w insert into O;",
     "capture of an 'or' side"),
    # a count suffix or `every` on a side
    ("from every a=A -> b=B<2:3> and c=C" + SEL, "count suffix on a side"),
    ("from every a=A -> b=B or c=C+" + SEL, "count suffix on a side"),
    ("from every a=A -> every b=B and c=C" + SEL, "'every' on a side"),
    ("from every a=A -> b=B or every c=C" + SEL, "'every' on a side"),
    ("from every a=A -> every (b=B and c=C)" + SEL, "'every' on a side"),
    # absent states
    ("from every a=A -> not B[id > 1] for 5 sec select a.id as x insert into O;", "absent pattern states"),
    ("from every a=A -> b=B and not C[id > 1] select a.id as x, b.id as y insert into O;", "absent pattern states"),
    ("from every a=A -> not C[id > 1] and b=B select a.id as x, b.id as y insert into O;", "absent pattern states"),
    ("from not A[id > 1] for 5 sec -> b=B select b.id as y insert into O;", "absent pattern states"),
    ("from every a=A -> (not B for 1 sec or c=C) select a.id as x insert into O;", "absent pattern states"),
    # more than six elementary states
    ("from every a=A -> (b=B and c=C) -> d=A -> (e=B or f=C) -> g=A select a.id as x insert into O;",
     "more than 6 states"),
]


@pytest.mark.parametrize("plan,word", REFUSED)
def test_refused(plan, word):
    with pytest.raises(fs.UnsupportedPlanException, match=word):
        fs.validate(ABC + plan)


def test_not_at_a_state_position_is_unsupported_not_a_parse_error():
    """A shim tells "fall back to Siddhi" (UnsupportedPlanException) from a
    typo (any other creation error) by the exception's type."""
    with pytest.raises(fs.UnsupportedPlanException, match=r"absent pattern states \(not \.\.\.\) are not supported"):
        fs.validate(ABC + "from every a=A -> not B for 1 sec select a.id as x insert into O;")
    # a typo stays a creation error that is no refusal
    with pytest.raises(fs.SiddhiAppCreationException) as e:
        fs.validate(ABC + "from every a=A -> b=B andd c=C" + SEL)
    assert not isinstance(e.value, fs.UnsupportedPlanException)
    with pytest.raises(fs.SiddhiAppCreationException) as e:
        fs.validate(ABC + "from every a=A -> (b=B) " + SEL)
    assert not isinstance(e.value, fs.UnsupportedPlanException)
