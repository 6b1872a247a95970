"""Query chaining in the front end (cep_validate / cep_plan_schema / the
planner calls: no device): a query may read a stream an earlier query inserts
into.  The accepted forms, the derived stream's schema, every refusal with a
message that names the construct, and what the planner calls report."""
import pytest

import flink_siddhi as fs
from flink_siddhi.operator import plan_input_streams, plan_partition_keys

AB = ("define stream A (k int, ts long, id int, price double);"
      "define stream B (k int, ts long, id int, price double);")
A1 = "from A[price > 0.1] select k, ts, id, price insert into A1;"
B1 = "from B[id % 7 != 0] select k, ts, id, price insert into B1;"
M = "from A[price > 0.1] select k, ts, id, price * 2.0 as p2 insert into M;"


def part(keys, q):
    return "partition with (" + keys + ") begin " + q + " end;"


ACCEPTED = [
    # the config-3 shape: two cleaning queries feed a partitioned pattern
    AB + A1 + B1 + part("k of A1, k of B1", "from every s1=A1[id > 3] -> s2=B1[price < 0.5] within 1 sec "
                                            "select s1.k as k, s1.id as a, s2.id as b insert into O;"),
    # computed column read by a filter, an aggregate, windows, a pattern, a sequence
    AB + M + "from M[p2 > 1.0] select k, p2 insert into O;",
    AB + M + "from M select k, sum(p2) as s, avg(p2) as a group by k having s > 1.0 insert into O;",
    AB + M + part("k of M", "from M#window.length(4) select k, sum(p2) as s insert into O;"),
    AB + M + part("k of M", "from M#window.time(50) select k, sum(p2) as s, count() as c insert into O;"),
    AB + M + part("k of M, k of B", "from every a=M[p2 > 1.0] -> b=B[id > 2] -> c=M[p2 < 1.5] "
                                    "select a.id as x, b.id as y, c.p2 as z insert into O;"),
    AB + M + part("k of M", "from every a=M[p2 > 1.0], b=M[p2 < 1.9]<1:3>, c=M[p2 > 0.3] "
                            "select a.id as x, b[last].p2 as y, c.id as z insert into O;"),
    # what the single-layer engine refuses: an aggregate of an expression, a computed key
    AB + "from A select k, price * id as notional insert into N;"
         "from N select k, sum(notional) as s group by k insert into O;",
    AB + "from A select id % 64 as g, ts, id, price insert into G;" +
    part("g of G", "from G#window.length(3) select g, sum(price) as s insert into O;"),
    # depth 2 and 3
    AB + M + "from M[p2 < 1.5] select k, ts, id, p2 + 1.0 as p3 insert into M2;"
             "from M2[p3 > 1.2] select k, p3 insert into O;",
    AB + M + "from M[p2 < 1.5] select k, ts, id, p2 + 1.0 as p3 insert into M2;"
             "from M2[p3 > 1.2] select k, ts, id, p3 * 2.0 as p4 insert into M3;"
             "from M3 select k, sum(p4) as s group by k insert into O;",
    # fan-out: one derived stream, three readers
    AB + M + "from M[p2 > 1.0] select k, p2 insert into O1;"
             "from M select k, count() as c group by k insert into O2;" +
    part("k of M", "from every a=M[p2 > 1.5] -> b=M[p2 < 0.5] select a.id as x, b.id as y insert into O3;"),
    # `define stream M` saying what the select list says
    AB + "define stream M (k int, ts long, id int, p2 double);" + M + "from M[p2 > 1.0] select k, p2 insert into O;",
    # ... and then the reader may stand before the producer
    AB + "define stream M (k int, ts long, id int, p2 double);"
         "from M[p2 > 1.0] select k, p2 insert into O;" + M,
    # select *
    AB + "from A[id > 2] select * insert into C; from C[price < 0.5] select k, id insert into O;",
    # a derived and a defined stream of identical definitions in one query
    AB + A1 + part("k of A1, k of B", "from every a=A1 -> b=B[id > 2] select a.id as x, b.id as y insert into O;"),
    # two producers of one stream
    AB + "from A[id > 5] select k, ts, id, price insert into C; from B[id < 3] select k, ts, id, price insert into C;"
         "from C select k, count() as c group by k insert into O;",
    # string passed through
    "define stream S (k int, name string, v long);"
    "from S[v > 1] select k, name, v * 2 as w insert into T; from T[name == 'x'] select k, name, w insert into O;",
]


@pytest.mark.parametrize("plan", ACCEPTED)
def test_accepted(plan):
    fs.validate(plan)


def test_derived_schema():
    plan = AB + M + "from M[p2 > 1.0] select k, p2 insert into O;"
    assert fs.plan_schema(plan, "M") == [("k", "int"), ("ts", "long"), ("id", "int"), ("p2", "double")]
    assert fs.plan_schema(plan, "O") == [("k", "int"), ("p2", "double")]
    plan = ("define stream S (k int, f float, name string, b bool);"
            "from S select k + 1L as kl, f * 2 as f2, name, b, k / 2.0 as d insert into T;"
            "from T[b] select kl, name insert into O;")
    assert fs.plan_schema(plan, "T") == [("kl", "long"), ("f2", "float"), ("name", "string"), ("b", "bool"),
                                        ("d", "double")]
    assert fs.plan_schema(plan, "O") == [("kl", "long"), ("name", "string")]


def test_output_only_streams_stay_outputs():
    # a defined stream that is inserted into and read by nobody is an output (it used to raise)
    plan = AB + "define stream O (k int, price double); from A[id > 1] select k, price insert into O;"
    fs.validate(plan)
    assert fs.plan_schema(plan, "O") == [("k", "int"), ("price", "double")]
    assert plan_input_streams(plan) == ["A"]


AGG = "from A select k, sum(price) as s group by k insert into M;"
REFUSED = [
    # producers that are not plain filter / projection queries
    (AB + part("k of A, k of B", "from every a=A -> b=B select a.k as k, b.id as id insert into M;") +
     "from M[id > 1] select k insert into O;", "pattern"),
    (AB + AGG + "from M[s > 1.0] select k insert into O;", "aggregate"),
    (AB + part("k of A", "from A#window.length(3) select k, sum(price) as s insert into M;") +
     "from M select k insert into O;", "window"),
    (AB + "from A#window.length(3) select sum(price) as s insert into M; from M select s insert into O;", "window"),
    (AB + "from A select k, price having price > 0.5 insert into M; from M select k insert into O;", "having"),
    # a producer inside a partition, inner streams
    (AB + part("k of A", "from A[id > 1] select k, id insert into M;") + "from M select k insert into O;",
     "partition"),
    (AB + part("k of A", "from A[id > 1] select k, id insert into #M; from #M select k insert into O;"),
     "inner streams"),
    # cycles
    (AB + "define stream M (k int, ts long, id int, price double);"
          "from M[id > 1] select k, ts, id, price insert into M;", "cycle"),
    (AB + "define stream X (k int, id int); define stream Y (k int, id int);"
          "from X[id > 1] select k, id insert into Y; from Y[id > 2] select k, id insert into X;", "cycle"),
    # depth 5
    (AB + "from A select k, id insert into D1; from D1 select k, id insert into D2;"
          "from D2 select k, id insert into D3; from D3 select k, id insert into D4;"
          "from D4 select k, id insert into D5; from D5 select k insert into O;", "deeper than 4"),
    # more than 8 derived streams
    (AB + "".join("from A[id == %d] select k, id insert into E%d;" % (i, i) for i in range(9)) +
     "".join("from E%d select k insert into O%d;" % (i, i) for i in range(9)), "more than 8 derived streams"),
    # handles are 8 in all: the defined streams count (two defined + seven derived)
    (AB + "".join("from A[id == %d] select k, id insert into E%d;" % (i, i) for i in range(7)) +
     "".join("from E%d select k insert into O%d;" % (i, i) for i in range(7)),
     "more than 8 defined and derived streams"),
    # a derived stream and a stream it derives from in one query
    (AB + A1 + part("k of A1, k of A", "from every a=A1 -> b=A select a.id as x, b.id as y insert into O;"),
     "derives from"),
    (AB + M + "from M select k, ts, id, p2 + 1.0 as p2 insert into M2;" +
     part("k of M, k of M2", "from every a=M -> b=M2 select a.id as x, b.id as y insert into O;"), "derives from"),
]


@pytest.mark.parametrize("plan,word", REFUSED)
def test_refused(plan, word):
    with pytest.raises(fs.UnsupportedPlanException, match=word):
        fs.validate(plan)


def test_incompatible_define_is_a_creation_error():
    for define in ("define stream M (k int, ts long, id int, p2 float);",      # type
                   "define stream M (k int, ts long, id int, price double);",  # name
                   "define stream M (k int, ts long, id int);"):               # count
        with pytest.raises(fs.SiddhiAppCreationException, match="incompatible definitions") as e:
            fs.validate(AB + define + M + "from M select k insert into O;")
        assert not isinstance(e.value, fs.UnsupportedPlanException)
    # two producers disagreeing about an undefined stream
    with pytest.raises(fs.SiddhiAppCreationException, match="incompatible definitions"):
        fs.validate(AB + M + "from B select k, ts, id insert into M; from M select k insert into O;")


def test_reading_before_the_producer_is_undefined():
    with pytest.raises(fs.UndefinedStreamException, match="M"):
        fs.validate(AB + "from M[p2 > 1.0] select k, p2 insert into O;" + M)
    # no define and no producer at all
    with pytest.raises(fs.UndefinedStreamException, match="Q"):
        fs.validate(AB + M + "from Q select k insert into O;")
    # an output nobody reads takes no input handle: its schema is known, but it is no input
    with pytest.raises(fs.UndefinedStreamException):
        plan_partition_keys(AB + "from A select k insert into O;", "O")


def test_plan_input_streams_leave_derived_streams_out():
    cfg3 = ACCEPTED[0]
    assert plan_input_streams(cfg3) == ["A", "B"]
    assert plan_input_streams(AB + M + "from M[p2 > 1.0] select k, p2 insert into O;") == ["A"]
    # a defined stream that a producer feeds is derived all the same
    assert plan_input_streams(ACCEPTED[12]) == ["A"]
    # mixed reader: B is fed from outside
    assert plan_input_streams(ACCEPTED[15]) == ["A", "B"]


def test_plan_partition_keys_follow_plain_copies():
    cfg3 = ACCEPTED[0]
    assert plan_partition_keys(cfg3, "A") == ["k"]
    assert plan_partition_keys(cfg3, "B") == ["k"]
    assert plan_partition_keys(cfg3, "A1") == ["k"]
    # a renamed and moved copy is followed back to the source's attribute
    plan = (AB + "from A select id, ts, k as key2, price insert into R;" +
            part("key2 of R", "from R#window.length(3) select key2, sum(price) as s insert into O;"))
    assert plan_partition_keys(plan, "A") == ["k"]
    assert plan_partition_keys(plan, "R") == ["key2"]
    # through two producers
    plan = (AB + "from A select id, ts, k as key2, price insert into R;"
                 "from R[price > 0.1] select key2 as key3, price insert into R2;"
                 "from R2 select key3, sum(price) as s group by key3 insert into O;")
    assert plan_partition_keys(plan, "A") == ["k"]
    # a computed key names no attribute of the source
    plan = ACCEPTED[8]
    assert plan_partition_keys(plan, "A") == []
    assert plan_partition_keys(plan, "G") == ["g"]
    # unkeyed readers
    assert plan_partition_keys(AB + M + "from M[p2 > 1.0] select k, p2 insert into O;", "A") == []
