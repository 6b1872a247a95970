"""Front end of windowed stream joins (cep_validate / cep_plan_schema, no GPU):
what validates, the output schema, and every refusal by name."""
import json
from pathlib import Path

import pytest

import flink_siddhi as fs
from flink_siddhi.runtime import plan_schema

FIXTURE = json.loads((Path(__file__).parent / "golden" / "join_itcase.json").read_text())

EV = ("define stream A (k int, ts long, id int, price double);"
      "define stream B (k int, ts long, id int, price double);")
SEL = " select a.id as x, b.price as p insert into O;"


def test_reference_plan_validates_with_its_schema():
    # SiddhiCEPITCase.java:306-327
    fs.validate(FIXTURE["plan"])
    assert plan_schema(FIXTURE["plan"], "JoinStream") == [("t", "long"), ("n", "string"), ("p1", "double"),
                                                          ("p2", "double")]


ACCEPTED = [
    # both window kinds on either side
    "from A#window.length(5) as a join B#window.time(500) as b on a.k == b.k" + SEL,
    "from A#window.time(500) as a join B#window.length(5) as b on a.k == b.k" + SEL,
    "from A#window.length(1) as a join B#window.length(255) as b on a.k == b.k" + SEL,
    "from A#window.time(1) as a join B#window.time(7) as b on a.k == b.k" + SEL,
    # no alias: the stream name
    "from A#window.length(5) join B#window.length(5) on A.k == B.k select A.id as x, B.price as p insert into O;",
    "from A#window.length(5) as a join B#window.length(5) on a.k == B.k select a.id as x, B.price as p insert into O;",
    # filters before the window
    "from A[price > 0.5]#window.length(5) as a join B[id < 7][k > 1]#window.time(500) as b on a.k == b.k" + SEL,
    "from A[a.price > 0.5]#window.length(5) as a join B#window.length(2) as b on a.k == b.k" + SEL,
    # time units
    "from A#window.time(1 sec) as a join B#window.time(500 milliseconds) as b on a.k == b.k" + SEL,
    "from A#window.time(2 min) as a join B#window.time(1 hour) as b on a.k == b.k" + SEL,
    "from A#window.time(500L) as a join B#window.length(5) as b on a.k == b.k" + SEL,
    # `on`: any bool expression over both sides; none at all
    "from A#window.length(5) as a join B#window.length(5) as b on a.k == b.k and a.price < b.price" + SEL,
    "from A#window.length(5) as a join B#window.length(5) as b on a.id + b.id > 3 and a.k == b.k" + SEL,
    "from A#window.length(5) as a join B#window.length(5) as b on not (a.k == b.k) or a.ts < b.ts" + SEL,
    "from A#window.length(5) as a join B#window.length(5) as b" + SEL,
    # computed select items; `inner join`; `insert current events into`
    "from A#window.length(5) as a join B#window.length(5) as b on a.k == b.k "
    "select a.price - b.price as d, a.ts as t insert into O;",
    "from A#window.length(5) as a inner join B#window.length(5) as b on a.k == b.k" + SEL,
    "from A#window.length(5) as a join B#window.length(5) as b on a.k == b.k "
    "select a.id as x insert current events into O;",
]


@pytest.mark.parametrize("query", ACCEPTED)
def test_accepted(query):
    fs.validate(EV + query)


def test_output_types_follow_the_select_list():
    plan = EV + ("from A#window.length(5) as a join B#window.time(5) as b on a.k == b.k "
                 "select a.k as k, b.ts as t, a.price - b.price as d, a.id + b.ts as s insert into O;")
    assert plan_schema(plan, "O") == [("k", "int"), ("t", "long"), ("d", "double"), ("s", "long")]


J = "from A#window.length(5) as a join B#window.length(5) as b on a.k == b.k"
UNSUPPORTED = [
    # streams with different definitions
    ("define stream C (k int, w long);from A#window.length(5) as a join C#window.length(5) as c on a.k == c.k "
     "select a.id as x insert into O;"),
    ("define stream C (k int, ts long, id int, cost double);from A#window.length(5) as a join C#window.length(5) as c "
     "on a.k == c.k select a.id as x insert into O;"),
    # a side without a window
    "from A as a join B#window.length(5) as b on a.k == b.k" + SEL,
    "from A#window.length(5) as a join B as b on a.k == b.k" + SEL,
    "from A[id > 3] as a join B[id > 3] as b on a.k == b.k" + SEL,
    # a self-join
    "from A#window.length(5) as a join A#window.length(5) as b on a.k == b.k" + SEL,
    # outer and unidirectional joins
    "from A#window.length(5) as a left outer join B#window.length(5) as b on a.k == b.k" + SEL,
    "from A#window.length(5) as a right outer join B#window.length(5) as b on a.k == b.k" + SEL,
    "from A#window.length(5) as a full outer join B#window.length(5) as b on a.k == b.k" + SEL,
    "from A#window.length(5) as a outer join B#window.length(5) as b on a.k == b.k" + SEL,
    "from A#window.length(5) as a unidirectional join B#window.length(5) as b on a.k == b.k" + SEL,
    "from A#window.length(5) as a join B#window.length(5) as b unidirectional on a.k == b.k" + SEL,
    # within / per
    J + " within 1 sec" + SEL,
    J + " per 1 sec" + SEL,
    # aggregates, group by, having
    J + " select sum(a.price) as s insert into O;",
    J + " select a.k as k, count() as n insert into O;",
    J + " select a.k as k, b.price as p group by a.k insert into O;",
    J + " select a.k as k, b.price as p having p > 0.5 insert into O;",
    # inside partition with
    "partition with (k of A, k of B) begin " + J + SEL + " end;",
    # chaining: a join reading a derived stream, a join's output read by another query
    "from A[id > 3] select k, ts, id, price insert into M;"
    "from M#window.length(5) as a join B#window.length(5) as b on a.k == b.k" + SEL,
    J + " select a.k as k, b.price as p insert into M; from M[p > 0.5] select k insert into O;",
    # expired / all events
    J + " select a.id as x insert expired events into O;",
    J + " select a.id as x insert all events into O;",
    # more rows than a length side holds
    "from A#window.length(256) as a join B#window.length(5) as b on a.k == b.k" + SEL,
]


@pytest.mark.parametrize("query", UNSUPPORTED)
def test_refusals_name_the_join(query):
    with pytest.raises(fs.UnsupportedPlanException) as ei:
        fs.validate(EV + query)
    assert "join" in str(ei.value)


PARSE_ERRORS = [
    # bad window arguments stay parse errors
    "from A#window.length(0) as a join B#window.length(5) as b on a.k == b.k" + SEL,
    "from A#window.length(5) as a join B#window.length(0) as b on a.k == b.k" + SEL,
    "from A#window.length(5) as a join B#window.time(x) as b on a.k == b.k" + SEL,
    "from A#window.length(5) as a join B#window.length(2.5) as b on a.k == b.k" + SEL,
    "from A#window.length(5) as a join B#window.time(5 parsecs) as b on a.k == b.k" + SEL,
    "from A#window.length(5) as a join B#window.length() as b on a.k == b.k" + SEL,
    # select * (as for patterns), unqualified and unknown references, a non-bool `on`
    J + " select * insert into O;",
    J + " select id as x insert into O;",
    J + " select c.id as x insert into O;",
    "from A#window.length(5) as a join B#window.length(5) as b on a.k + b.k" + SEL,
    # a side's filter reads its own side only
    "from A#window.length(5) as a join B[a.id > 3]#window.length(5) as b on a.k == b.k" + SEL,
]


@pytest.mark.parametrize("query", PARSE_ERRORS)
def test_parse_errors(query):
    with pytest.raises(fs.SiddhiAppCreationException):
        fs.validate(EV + query)


def test_undefined_stream():
    with pytest.raises(fs.UndefinedStreamException):
        fs.validate(EV + "from A#window.length(5) as a join Z#window.length(5) as b on a.k == b.k" + SEL)
