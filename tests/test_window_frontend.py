"""`#window.length(N)` / `#window.time(T)` in the front end (cep_validate /
cep_plan_schema: no device): the accepted forms, the output types, and every
refusal with a message that names the construct."""
import pytest

import flink_siddhi as fs

S = "define stream S (k int, v long, p double, f float, name string);"


def part(q):
    return S + "partition with (k of S) begin " + q + " end;"


ACCEPTED = [
    # (a) inside a partition: no group by, or group by the partition key
    part("from S#window.length(5) select k, sum(v) as s insert into O;"),
    part("from S[v > 3]#window.length(1) select k, sum(v) as s, count() as c group by k insert into O;"),
    part("from S#window.time(500) select k, avg(p) as a insert into O;"),
    part("from S[p < 0.5 and v > 1]#window.time(1 sec) select k, min(p) as m group by k insert into O;"),
    # (b) one global window, one global group
    S + "from S#window.length(5) select sum(v) as s, count() as c insert into O;",
    S + "from S[v > 3]#window.time(10) select max(v) as m insert into O;",
    # (c) validates: its ts_order refusal is cep_create's
    S + "from S#window.time(10) select k, sum(v) as s group by k insert into O;",
    # unit spellings
    S + "from S#window.time(2 min 30 sec) select sum(v) as s insert into O;",
    S + "from S#window.time(100 milliseconds) select sum(v) as s insert into O;",
    S + "from S#window.time(1 hour) select sum(v) as s insert into O;",
    S + "from S#window.time(500L) select sum(v) as s insert into O;",
    # current events, having, current attributes next to aggregates, an alias
    S + "from S#window.length(5) select sum(v) as s insert current events into O;",
    part("from S#window.length(3) select k, v, sum(v) as s having s > 10 and v > 1 insert into O;"),
    S + "from S#window.length(5) as e select sum(e.v) as s insert into O;",
    # no aggregate: current events only, the plain projection
    S + "from S#window.length(5) select * insert into O;",
    S + "from S[v > 1]#window.time(1 sec) select k, v insert into O;",
]


@pytest.mark.parametrize("plan", ACCEPTED)
def test_accepted(plan):
    fs.validate(plan)


def test_output_schema_types():
    # (at most 8 aggregates per query, as for the plain group-by)
    plan = part("from S#window.length(4) select k, sum(k) as si, sum(v) as sl, sum(f) as sf, sum(p) as sd, "
                "avg(k) as ai, avg(p) as ad, count() as c insert into O;")
    assert fs.plan_schema(plan, "O") == [
        ("k", "int"), ("si", "long"), ("sl", "long"), ("sf", "double"), ("sd", "double"),
        ("ai", "double"), ("ad", "double"), ("c", "long")]
    plan = part("from S#window.time(4) select min(k) as mni, max(v) as mxl, min(f) as mnf, max(p) as mxd "
                "insert into O;")
    assert fs.plan_schema(plan, "O") == [("mni", "int"), ("mxl", "long"), ("mnf", "float"), ("mxd", "double")]
    with pytest.raises(fs.UnsupportedPlanException):
        fs.validate(part("from S#window.length(4) select sum(k) as a1, sum(v) as a2, sum(f) as a3, sum(p) as a4, "
                         "avg(k) as a5, avg(p) as a6, min(k) as a7, max(v) as a8, count() as a9 insert into O;"))


def test_select_star_schema_is_the_input():
    plan = S + "from S#window.time(1 sec) select * insert into O;"
    assert fs.plan_schema(plan, "O") == fs.plan_schema(plan, "S")


UNSUPPORTED = [
    (S + "from S#window.lengthBatch(5) select sum(v) as s insert into O;", "lengthBatch"),
    (S + "from S#window.timeBatch(1 sec) select sum(v) as s insert into O;", "timeBatch"),
    (S + "from S#window.externalTime(v, 1 sec) select sum(v) as s insert into O;", "externalTime"),
    (S + "from S#window.sort(5, v) select sum(v) as s insert into O;", "sort"),
    (S + "from S#str:tokenize(name, ',') select name insert into O;", "str:tokenize"),
    (S + "from S#log('x') select v insert into O;", "log"),
    (S + "from S#window.length(5)[v > 1] select sum(v) as s insert into O;", "filter after the window"),
    (S + "from S#window.length(5) select sum(v) as s insert expired events into O;", "expired events"),
    (S + "from S#window.time(5) select sum(v) as s insert all events into O;", "all events"),
    (S + "from S#window.length(5) select k, v insert all events into O;", "all events"),
    (S + "from every a=S[v > 1]#window.length(5) -> b=S[v > 2] select a.v as x insert into O;",
     "pattern or sequence state"),
    (S + "from a=S[v > 1], b=S[v > 2]#window.time(5) select a.v as x insert into O;",
     "pattern or sequence state"),
    (S + "define stream T (k int, w long);"
     "from S#window.length(5) join T#window.length(5) on S.k == T.k select S.v insert into O;", "join"),
    (S + "from S#window.length(5) select k, sum(v) as s group by k insert into O;",
     "length window shared by several groups"),
    (S + "from S#window.length(5)#window.time(5) select sum(v) as s insert into O;", "second window"),
]


@pytest.mark.parametrize("plan,names", UNSUPPORTED)
def test_unsupported(plan, names):
    with pytest.raises(fs.UnsupportedPlanException) as ei:
        fs.validate(plan)
    assert names in str(ei.value)


PARSE = [
    (S + "from S#window.length(0) select sum(v) as s insert into O;", "#window.length"),
    (S + "from S#window.time(0) select sum(v) as s insert into O;", "#window.time"),
    (S + "from S#window.time(0 sec) select sum(v) as s insert into O;", "#window.time"),
    (S + "from S#window.length(v) select sum(v) as s insert into O;", "#window.length"),
    (S + "from S#window.time(v) select sum(v) as s insert into O;", "#window.time"),
    (S + "from S#window.length(2.5) select sum(v) as s insert into O;", "#window.length"),
    (S + "from S#window.length(1 sec) select sum(v) as s insert into O;", "#window.length"),
    (S + "from S#window.length() select sum(v) as s insert into O;", "#window.length"),
]


@pytest.mark.parametrize("plan,names", PARSE)
def test_bad_argument_is_a_parse_error(plan, names):
    with pytest.raises(fs.SiddhiAppCreationException) as ei:
        fs.validate(plan)
    assert not isinstance(ei.value, fs.UnsupportedPlanException)
    assert names in str(ei.value)


def test_events_keyword_is_recorded_for_window_queries_only():
    with pytest.raises(fs.UnsupportedPlanException, match="expired events"):
        fs.validate(S + "from S[v > 1]#window.time(5) select v insert expired events into O;")
    # non-window queries stay as they are: the keyword is swallowed
    fs.validate(S + "from S[v > 1] select v insert expired events into O;")
