"""`#window.lengthBatch(N)` / `#window.externalTimeBatch(c, T)` in the front
end (cep_validate / cep_plan_schema: no device): the accepted forms, the
output types, and every refusal with a message that names the construct."""
import pytest

import flink_siddhi as fs

S = "define stream S (k int, v long, p double, f float, name string, t long);"
T2 = "define stream T (k int, v long, p double, f float, name string, t long);"
TAB = "@PrimaryKey('k') define table Tab (k int, v long);"


def part(q):
    return S + "partition with (k of S) begin " + q + " end;"


ACCEPTED = [
    part("from S#window.lengthBatch(5) select k, sum(v) as s insert into O;"),
    part("from S#window.lengthBatch(1) select sum(v) as s, count() as c insert into O;"),
    part("from S[v > 3]#window.lengthBatch(5) select k, sum(v) as s, count() as c group by k insert into O;"),
    part("from S#window.lengthBatch(2147483647) select k, max(p) as m insert into O;"),
    part("from S#window.lengthBatch(5L) select k, max(p) as m insert into O;"),
    part("from S#window.lengthBatch(5) as e select e.k, sum(e.v) as s insert into O;"),
    part("from S#window.lengthBatch(5) select k, sum(v) as s insert current events into O;"),
    part("from S#window.lengthBatch(3) select k, v, p * 2 as q, sum(v) as s having s > 10 and v > 1 insert into O;"),
    part("from S#window.externalTimeBatch(t, 500) select k, avg(p) as a insert into O;"),
    part("from S[p < 0.5 and v > 1]#window.externalTimeBatch(t, 1 sec) select k, min(p) as m group by k "
         "insert into O;"),
    part("from S#window.externalTimeBatch(t, 2 min 30 sec) select sum(v) as s insert into O;"),
    part("from S#window.externalTimeBatch(t, 100 milliseconds) select sum(v) as s insert into O;"),
    part("from S#window.externalTimeBatch(t, 1 hour) select sum(v) as s insert into O;"),
    part("from S#window.externalTimeBatch(t, 500L) select sum(v) as s insert into O;"),
    part("from S#window.externalTimeBatch(v, 1) select k, count() as c insert into O;"),
    part("from S#window.externalTimeBatch(t, 10) as e select e.k, e.v, sum(e.v) as s having s > 3 "
         "insert current events into O;"),
    part("from S#window.externalTimeBatch(S.t, 10) select k, count() as c insert into O;"),
    part("from S#window.externalTimeBatch(e.t, 10) as e select k, count() as c insert into O;"),
    part("from S#window.externalTimeBatch(S.t, 10) as e select k, count() as c insert into O;"),
]


@pytest.mark.parametrize("plan", ACCEPTED)
def test_accepted(plan):
    fs.validate(plan)


@pytest.mark.parametrize("win", ["lengthBatch(4)", "externalTimeBatch(t, 4)"])
def test_output_schema_types(win):
    # (at most 8 aggregates per query, as for the plain group-by)
    plan = part("from S#window.%s select k, sum(k) as si, sum(v) as sl, sum(f) as sf, sum(p) as sd, "
                "avg(k) as ai, avg(p) as ad, count() as c insert into O;" % win)
    assert fs.plan_schema(plan, "O") == [
        ("k", "int"), ("si", "long"), ("sl", "long"), ("sf", "double"), ("sd", "double"),
        ("ai", "double"), ("ad", "double"), ("c", "long")]
    plan = part("from S#window.%s select avg(v) as al, avg(f) as af, min(k) as mni, max(v) as mxl, min(f) as mnf, "
                "max(p) as mxd, max(k) as mxi, min(p) as mnd insert into O;" % win)
    assert fs.plan_schema(plan, "O") == [
        ("al", "double"), ("af", "double"), ("mni", "int"), ("mxl", "long"), ("mnf", "float"), ("mxd", "double"),
        ("mxi", "int"), ("mnd", "double")]
    with pytest.raises(fs.UnsupportedPlanException):
        fs.validate(part("from S#window.%s select sum(k) as a1, sum(v) as a2, sum(f) as a3, sum(p) as a4, "
                         "avg(k) as a5, avg(p) as a6, min(k) as a7, max(v) as a8, count() as a9 insert into O;" % win))


UNSUPPORTED = [
    # outside a partition
    (S + "from S#window.lengthBatch(5) select sum(v) as s insert into O;", "#window.lengthBatch outside a partition"),
    (S + "from S#window.externalTimeBatch(t, 5) select k, sum(v) as s group by k insert into O;",
     "#window.externalTimeBatch outside a partition"),
    # group by on anything but the partition key
    (part("from S#window.lengthBatch(5) select name, sum(v) as s group by name insert into O;"),
     "#window.lengthBatch with group by on anything but the partition key"),
    (part("from S#window.externalTimeBatch(t, 5) select v, count() as c group by v insert into O;"),
     "#window.externalTimeBatch with group by on anything but the partition key"),
    (part("from S#window.lengthBatch(5) select k, sum(v) as s group by k, name insert into O;"),
     "#window.lengthBatch with group by on anything but the partition key"),
    # no aggregate
    (part("from S#window.lengthBatch(5) select k, v insert into O;"), "#window.lengthBatch without an aggregate"),
    (part("from S#window.externalTimeBatch(t, 5) select * insert into O;"),
     "#window.externalTimeBatch without an aggregate"),
    # expired / all events
    (part("from S#window.lengthBatch(5) select k, sum(v) as s insert expired events into O;"),
     "insert expired events on a #window.lengthBatch query"),
    (part("from S#window.externalTimeBatch(t, 5) select k, sum(v) as s insert all events into O;"),
     "insert all events on a #window.externalTimeBatch query"),
    # the optional arguments of externalTimeBatch
    (part("from S#window.externalTimeBatch(t, 5, 0) select k, sum(v) as s insert into O;"), "more than two arguments"),
    (part("from S#window.externalTimeBatch(t, 5, 0, 1 sec) select k, sum(v) as s insert into O;"),
     "#window.externalTimeBatch with more than two arguments"),
    (part("from S#window.externalTimeBatch(t, 1 sec, 0, 1 sec, true) select k, sum(v) as s insert into O;"),
     "#window.externalTimeBatch with more than two arguments"),
    # join sides, pattern / sequence states, tables, `in`
    (S + T2 + "from S#window.lengthBatch(5) join T#window.length(5) on S.k == T.k select S.v insert into O;",
     "#window.lengthBatch on a join side"),
    (S + T2 + "from S#window.time(5) join T#window.externalTimeBatch(t, 5) on S.k == T.k select S.v insert into O;",
     "#window.externalTimeBatch on a join side"),
    (S + "from every a=S[v > 1]#window.lengthBatch(5) -> b=S[v > 2] select a.v as x insert into O;",
     "pattern or sequence state"),
    (S + "from a=S[v > 1], b=S[v > 2]#window.externalTimeBatch(t, 5) select a.v as x insert into O;",
     "pattern or sequence state"),
    (S + TAB + "from S#window.lengthBatch(5) select k, v insert into Tab;", "#window.lengthBatch on a query that names a table"),
    (S + TAB + "from S#window.externalTimeBatch(t, 5) select k, v update or insert into Tab on Tab.k == k;",
     "#window.externalTimeBatch on a query that names a table"),
    (S + TAB + "from S#window.lengthBatch(5) join Tab on S.k == Tab.k select S.v insert into O;",
     "#window.lengthBatch on a query that names a table"),
    (S + TAB + "from S[(Tab.k == k) in Tab]#window.lengthBatch(5) select k, sum(v) as s insert into O;",
     "#window.lengthBatch on a query that names a table"),
    # the windows that stay refused, and the list of supported ones
    (S + "from S#window.timeBatch(1 sec) select sum(v) as s insert into O;", "#window.timeBatch is not supported"),
    (S + "from S#window.externalTime(t, 1 sec) select sum(v) as s insert into O;",
     "#window.externalTime is not supported"),
    (S + "from S#window.sort(5, v) select sum(v) as s insert into O;",
     "only #window.length, #window.time, #window.lengthBatch and #window.externalTimeBatch"),
    # as for the sliding windows
    (part("from S#window.lengthBatch(5)[v > 1] select k, sum(v) as s insert into O;"), "filter after the window"),
    (part("from S#window.lengthBatch(5)#window.length(5) select k, sum(v) as s insert into O;"), "second window"),
]


@pytest.mark.parametrize("plan,names", UNSUPPORTED)
def test_unsupported(plan, names):
    with pytest.raises(fs.UnsupportedPlanException) as ei:
        fs.validate(plan)
    assert names in str(ei.value)


PARSE = [
    (part("from S#window.lengthBatch(0) select sum(v) as s insert into O;"), "#window.lengthBatch"),
    (part("from S#window.lengthBatch(2147483648) select sum(v) as s insert into O;"), "#window.lengthBatch"),
    (part("from S#window.lengthBatch(v) select sum(v) as s insert into O;"), "#window.lengthBatch"),
    (part("from S#window.lengthBatch(2.5) select sum(v) as s insert into O;"), "#window.lengthBatch"),
    (part("from S#window.lengthBatch(1 sec) select sum(v) as s insert into O;"), "#window.lengthBatch"),
    (part("from S#window.lengthBatch() select sum(v) as s insert into O;"), "#window.lengthBatch"),
    (part("from S#window.externalTimeBatch(t, 0) select sum(v) as s insert into O;"), "#window.externalTimeBatch"),
    (part("from S#window.externalTimeBatch(t, 0 sec) select sum(v) as s insert into O;"), "#window.externalTimeBatch"),
    (part("from S#window.externalTimeBatch(t, v) select sum(v) as s insert into O;"), "#window.externalTimeBatch"),
    (part("from S#window.externalTimeBatch(t, 2.5) select sum(v) as s insert into O;"), "#window.externalTimeBatch"),
    (part("from S#window.externalTimeBatch(t) select sum(v) as s insert into O;"), "#window.externalTimeBatch"),
    (part("from S#window.externalTimeBatch(5, 10) select sum(v) as s insert into O;"), "#window.externalTimeBatch"),
    (part("from S#window.externalTimeBatch(nosuch, 10) select sum(v) as s insert into O;"),
     "#window.externalTimeBatch: nosuch is not an attribute"),
    (part("from S#window.externalTimeBatch(p, 10) select sum(v) as s insert into O;"),
     "#window.externalTimeBatch: the time attribute p must be long"),
    (part("from S#window.externalTimeBatch(k, 10) select sum(v) as s insert into O;"),
     "#window.externalTimeBatch: the time attribute k must be long"),
    # a qualifier is bound against the stream and its alias
    (part("from S#window.externalTimeBatch(Nosuch.t, 10) select sum(v) as s insert into O;"),
     "#window.externalTimeBatch: Nosuch in Nosuch.t names neither the stream S"),
    (part("from S#window.externalTimeBatch(x.t, 10) as e select sum(v) as s insert into O;"),
     "#window.externalTimeBatch: x in x.t names neither the stream S nor its alias e"),
    (part("from S#window.externalTimeBatch(S.nosuch, 10) select sum(v) as s insert into O;"),
     "#window.externalTimeBatch: nosuch is not an attribute"),
    (part("from S#window.lengthBatch(99999999999999999999) select sum(v) as s insert into O;"), "#window.lengthBatch"),
]


@pytest.mark.parametrize("plan,names", PARSE)
def test_bad_argument_is_a_parse_error(plan, names):
    with pytest.raises(fs.SiddhiAppCreationException) as ei:
        fs.validate(plan)
    assert not isinstance(ei.value, fs.UnsupportedPlanException)
    assert names in str(ei.value)
