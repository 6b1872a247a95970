"""Front end of event tables (cep_validate / cep_plan_schema, no GPU): what
validates, the output schema of a lookup join, the routing keys of a table
plan, and every refusal by name."""
import ctypes as C

import pytest

import flink_siddhi as fs
from flink_siddhi import _lib as L
from flink_siddhi.runtime import plan_schema

EV = ("define stream U (k int, ts long, id int, price double);"
      "define stream S (k int, ts long, id int, price double);")
TAB = "@PrimaryKey('k') define table T (k int, id int, price double);"
DEFS = EV + TAB
SEL = " select s.id as x, t.price as p insert into O;"

ACCEPTED = [
    # writers
    "from U select k, id, price insert into T;",
    "from U[price > 0.5] select k, id, price insert into T;",
    "from U select id as k, k as id, price insert into T;",
    "from U[price > 0.5][id < 7] select k, id, price insert into T;",
    "from U select k, id, price update or insert into T on T.k == k;",
    "from U select k, id, price update or insert into T on k == T.k;",
    "from U select k, id, price update or insert into T set T.price = price on T.k == k;",
    "from U select k, id, price update T on T.k == k;",
    "from U select k, price update T set T.price = price on T.k == k;",
    "from U select k, price, id update T set T.price = price, T.id = id on k == T.k;",
    "from U[id == 3] select k delete T on T.k == k;",
    "from U select k delete T on k == T.k;",
    # lookup join: both side orders, alias / no alias, a further condition, computed items
    "from S as s join T as t on s.k == t.k" + SEL,
    "from S as s join T as t on t.k == s.k" + SEL,
    "from T as t join S as s on s.k == t.k" + SEL,
    "from S join T on S.k == T.k select S.id as x, T.price as p insert into O;",
    "from T join S on T.k == S.k select S.id as x, T.price as p insert into O;",
    "from S as s join T on s.k == T.k select s.id as x, T.price as p insert into O;",
    "from S[price > 0.5][id < 9] as s join T as t on s.k == t.k" + SEL,
    "from S as s join T as t on s.k == t.k and s.price > t.price" + SEL,
    "from S as s join T as t on s.price > t.price and t.k == s.k and s.id != t.id" + SEL,
    "from S as s inner join T as t on s.k == t.k select s.price - t.price as d, s.ts as t0 insert into O;",
    "from S as s join T as t on s.k == t.k select s.id as x insert current events into O;",
    # in / not in
    "from S[(T.k == k) in T] select k, id insert into O;",
    "from S[(k == T.k) in T] select * insert into O;",
    "from S[id > 2 and (T.k == k) in T] select k, id insert into O;",
    "from S[id > 2][(T.k == k) in T and price < 0.5] select k, id + 1 as n insert into O;",
    "from S[not ((T.k == k) in T)] select k, id insert into O;",
    "from S[not ((T.k == k) in T) and id > 2] select k insert into O;",
    # several operations on one table in one plan
    "from U select k, id, price update or insert into T on T.k == k;from S as s join T as t on s.k == t.k" + SEL,
]


@pytest.mark.parametrize("query", ACCEPTED)
def test_accepted(query):
    fs.validate(DEFS + query)


def test_long_and_string_keys():
    fs.validate("define stream U (n string, v long);@PrimaryKey('n') define table T (n string, v long);"
                "from U select n, v insert into T;")
    fs.validate("define stream U (n long, v long);@PrimaryKey('n') define table T (n long, v long);"
                "from U select n, v update or insert into T on T.n == n;")


def test_other_annotations_are_still_skipped():
    fs.validate("@app:name('x') " + EV + "@info(name = 'q') from U select k insert into O;")


def test_join_schema_follows_the_select_list():
    plan = DEFS + ("from S as s join T as t on s.k == t.k "
                   "select s.k as k, t.id as i, s.price - t.price as d, s.id + s.ts as n, t.price as p insert into O;")
    assert plan_schema(plan, "O") == [("k", "int"), ("i", "int"), ("d", "double"), ("n", "long"), ("p", "double")]


def test_in_schema():
    assert plan_schema(DEFS + "from S[(T.k == k) in T] select * insert into O;", "O") == \
        [("k", "int"), ("ts", "long"), ("id", "int"), ("price", "double")]


def _plan_call(fn, *args):
    buf = C.create_string_buffer(1024)
    rc = fn(*[a.encode() for a in args], buf, len(buf))
    assert rc == L.CEP_OK, buf.value
    return buf.value.decode().split("\n") if buf.value else []


def test_input_streams_and_partition_keys_of_a_table_plan():
    plan = ("define stream U (id int, k int, price double);define stream S (a int, key int);define stream X (k int);"
            "@PrimaryKey('k') define table T (k int, price double);"
            "from U select k, price update or insert into T on T.k == k;"
            "from S as s join T as t on s.key == t.k select s.a as a, t.price as p insert into O;")
    lib = L.lib()
    assert _plan_call(lib.cep_plan_input_streams, plan) == ["U", "S"]
    assert _plan_call(lib.cep_plan_partition_keys, plan, "U") == ["k"]
    assert _plan_call(lib.cep_plan_partition_keys, plan, "S") == ["key"]


J = "from S as s join T as t on s.k == t.k"
W = "from U select k, id, price insert into T;"
UNSUPPORTED = [
    # no primary key, composite key, @Index, @Store
    EV + "define table T (k int, id int, price double);" + W,
    EV + "@PrimaryKey('k', 'id') define table T (k int, id int, price double);" + W,
    EV + "@PrimaryKey('k') @Index('id') define table T (k int, id int, price double);" + W,
    EV + "@Store(type='rdbms') @PrimaryKey('k') define table T (k int, id int, price double);" + W,
    # key type, object attribute, too many attributes
    EV + "@PrimaryKey('price') define table T (k int, id int, price double);" + W,
    EV + "@PrimaryKey('k') define table T (k int, o object);from U select k insert into T;",
    EV + "@PrimaryKey('k') define table T (k int, a int, b int, c int, d int, e int, f int, g int, h int);"
         "from U select k delete T on T.k == k;",
    # an `on` that is not the key equality
    DEFS + "from S as s join T as t on s.id == t.id" + SEL,
    DEFS + "from S as s join T as t on s.k == t.id" + SEL,
    DEFS + "from S as s join T as t on s.k > t.k" + SEL,
    DEFS + "from S as s join T as t on s.k == t.k or s.id == t.id" + SEL,
    DEFS + "from S as s join T as t on s.k == t.k and s.id == t.k" + SEL,
    DEFS + "from S as s join T as t" + SEL,
    DEFS + "from U select k, id, price update or insert into T on T.id == id;",
    DEFS + "from U select k, id, price update T on T.k == k and T.id == id;",
    DEFS + "from U select k, id delete T on T.id == id;",
    DEFS + "from U select k, id, price update or insert into T on T.k == id;",
    DEFS + "from S[(T.id == id) in T] select k insert into O;",
    DEFS + "from S[(T.k > k) in T] select k insert into O;",
    # outer and unidirectional joins with a table side
    DEFS + "from S as s left outer join T as t on s.k == t.k" + SEL,
    DEFS + "from S as s right outer join T as t on s.k == t.k" + SEL,
    DEFS + "from T as t full outer join S as s on s.k == t.k" + SEL,
    DEFS + "from S as s unidirectional join T as t on s.k == t.k" + SEL,
    DEFS + "from S as s join T as t unidirectional on s.k == t.k" + SEL,
    # windows, a filter on the table side
    DEFS + "from S#window.length(5) as s join T as t on s.k == t.k" + SEL,
    DEFS + "from S as s join T#window.length(5) as t on s.k == t.k" + SEL,
    DEFS + "from S as s join T[id > 3] as t on s.k == t.k" + SEL,
    # two tables
    DEFS + "@PrimaryKey('k') define table T2 (k int, id int, price double);"
           "from T as t join T2 as s on s.k == t.k" + SEL,
    DEFS + "@PrimaryKey('k') define table T2 (k int, id int, price double);"
           "from S[(T.k == k) in T] select k, id, price insert into T2;",
    DEFS + "@PrimaryKey('k') define table T2 (k int, id int, price double);"
           "from S[(T2.k == k) in T2] as s join T as t on s.k == t.k" + SEL,
    # a table read as a stream
    DEFS + "from T select k, id insert into O;",
    DEFS + "from T[id > 3] select k insert into O;",
    # pattern, sequence, window, aggregate queries that write a table; computed items
    DEFS + "from every a=U -> b=S[k == a.k] select a.k as k, b.id as id, b.price as price insert into T;",
    DEFS + "from every a=U, b=S select a.k as k, b.id as id, b.price as price insert into T;",
    DEFS + "from U#window.length(3) select k, id, price insert into T;",
    DEFS + "from U select k, count() as id, sum(price) as price group by k insert into T;",
    DEFS + "from U select k, id + 1 as id, price insert into T;",
    DEFS + "from U select k, price * 2 as price update T set T.price = price on T.k == k;",
    DEFS + "from every a=U -> b=T select a.k as k insert into O;",
    # inside partition with
    DEFS + "partition with (k of U) begin " + W + " end;",
    DEFS + "partition with (k of S) begin " + J + SEL + " end;",
    DEFS + "partition with (k of S) begin from S[(T.k == k) in T] select k insert into O; end;",
    # derived streams: an operation on one, one fed from a lookup join
    DEFS + "from U[id > 3] select k, id, price insert into M;from M select k, id, price insert into T;",
    DEFS + "from S[id > 3] select * insert into M;from M as s join T as t on s.k == t.k" + SEL,
    DEFS + J + " select s.k as k, t.price as p insert into M;from M[p > 0.5] select k insert into O;",
    # `in` anywhere but a top-level conjunct; two of them; in a writer
    DEFS + "from S[id > 3 or (T.k == k) in T] select k insert into O;",
    DEFS + "from S[(T.k == k) in T and (T.k == id) in T] select k insert into O;",
    DEFS + "from S select k, (T.k == k) in T as b insert into O;",
    DEFS + "from U[(T.k == k) in T] select k, id, price insert into T;",
    # insert with other attribute names; set of the key; more than 6 operations
    DEFS + "from U select k, id as n, price insert into T;",
    DEFS + "from U select k, id update T set T.k = id on T.k == k;",
    DEFS + W * 7,
    # more than 4 tables
    EV + "".join("@PrimaryKey('k') define table T%d (k int);" % i for i in range(5)) + "from U select k insert into T0;",
]


@pytest.mark.parametrize("plan", UNSUPPORTED)
def test_unsupported(plan):
    with pytest.raises(fs.UnsupportedPlanException, match="table"):
        fs.validate(plan)


PARSE = [
    # insert: count or type mismatch
    "from U select k, id insert into T;",
    "from U select k, id, price, ts insert into T;",
    "from U select k, price, id insert into T;",
    "from U select ts, id, price insert into T;",
    "from U select k, id, price, ts update or insert into T on T.k == k;",
    # update without set that lacks an attribute; a set of another type; an unknown attribute
    "from U select k, id update T on T.k == k;",
    "from U select k, price update T on T.k == k;",
    "from U select k, id update T set T.price = id on T.k == k;",
    "from U select k, id update T set T.nope = id on T.k == k;",
    # the key of another type
    "from U select ts delete T on T.k == ts;",
]


@pytest.mark.parametrize("query", PARSE)
def test_parse_errors(query):
    with pytest.raises(fs.SiddhiAppCreationException):
        fs.validate(DEFS + query)


def test_stream_join_refusals_keep_their_messages():
    # a side without a window is refused as before unless it is a defined table
    with pytest.raises(fs.UnsupportedPlanException, match="a join side without a window is not supported"):
        fs.validate(DEFS + "from S as s join U as u on s.k == u.k select s.id as x insert into O;")
    with pytest.raises(fs.UnsupportedPlanException, match=r"outer joins \(left ... join\) are not supported"):
        fs.validate(DEFS + "from S#window.length(2) as s left outer join U#window.length(2) as u on s.k == u.k "
                           "select s.id as x insert into O;")


def test_table_is_no_stream():
    plan = DEFS + W
    with pytest.raises(fs.UndefinedStreamException):
        plan_schema(plan, "T")
    with pytest.raises(fs.UndefinedStreamException):
        fs.validate(DEFS + "from U select k delete X on X.k == k;")
    with pytest.raises(fs.DuplicatedStreamException):
        fs.validate(DEFS + "define stream T (k int);" + W)
