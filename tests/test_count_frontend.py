"""Count states in patterns in the front end (cep_validate / cep_plan_schema:
no device): `A -> B<m:n> -> C`.  Every accepted form, the output schema of a
plan with b[0] / b[1] / b[last], every refusal with a message that names the
construct, and the malformed counts that stay parse errors."""
import pytest

import flink_siddhi as fs

ABC = "".join("define stream %s (k int, ts long, id int, price double, name string);" % s for s in "ABC")
SEL = " select a.id as x, b[0].price as y0, b[last].price as yl, c.price as z insert into O;"
SEL2 = " select a.id as x, b[0].price as y0, b[last].price as yl insert into O;"


def part(q):
    return "partition with (k of A, k of B, k of C) begin " + q + " end;"


ACCEPTED = [
    # <m:n>, <m:>, <n> in the middle, with and without `within` / `every` / a partition
    "from every a=A[id > 3] -> b=B[price > 0.2]<2:4> -> c=C[price < 0.9] within 5 sec" + SEL,
    "from every a=A -> b=B<2:> -> c=C" + SEL,
    "from a=A -> b=B<3> -> c=C within 10 milliseconds" + SEL,
    "from every a=A -> b=B<1:2> -> c=C" + SEL,
    part("from every a=A[id > 3] -> b=B[k == a.k]<2:> -> c=C[id != 4] within 5 sec" + SEL),
    # a count state in last position, the two-position form included
    "from every a=A -> b=B<2:3>" + SEL2,
    "from every a=A -> b=B[price > a.price]<2:> within 1 sec" + SEL2,
    "from every a=A -> c=C -> b=B<4>" + SEL,
    # consecutive count states; six states
    "from every a=A -> b=B<2:3> -> c=C<1:2>" + SEL,
    "from every a=A -> b=B<2> -> c=C<2:> -> d=A -> e=B<1:3> -> f=C "
    "select a.id as x, b[1].id as y, c[last].id as z, d.id as w, e[2].name as n, f.id as v insert into O;",
    # the same stream as its neighbour, on either side
    "from every a=A -> b=B[price > 0.1]<1:3> -> c=B[price > 0.5]" + SEL,
    "from every a=A -> b=A[id > a.id]<2:3> -> c=C" + SEL,
    # conditions reading the count state's own captures, and a later state reading them
    "from every a=A -> b=B[not (b[last].id >= id) and price > b[0].price / 2]<2:4> -> c=C[price > b[1].price]" + SEL,
    "from every a=A -> b=B<2:4> -> c=C[price > b.price and id > b[last].id]" + SEL,
]


@pytest.mark.parametrize("plan", ACCEPTED)
def test_accepted(plan):
    fs.validate(ABC + plan)


def test_plan_schema_of_indexed_captures():
    plan = ABC + ("from every a=A -> b=B<2:4> -> c=C within 1 sec select a.k as k, b[0].price as p0, b[1].id as i1, "
                  "b[last].name as nl, b.ts as t0, c.price as cp insert into O;")
    assert fs.plan_schema(plan, "O") == [("k", "int"), ("p0", "double"), ("i1", "int"), ("nl", "string"),
                                        ("t0", "long"), ("cp", "double")]


def test_a_count_of_one_is_a_plain_state():
    """`<1>` and `<1:1>` are the plain state: the same plan, the same schema."""
    plain = ABC + "from every a=A -> b=B[id > a.id] -> c=C select a.id as x, b.id as y, c.id as z insert into O;"
    for one in ("<1>", "<1:1>"):
        assert fs.plan_schema(plain.replace("b=B[id > a.id]", "b=B[id > a.id]" + one), "O") == fs.plan_schema(plain, "O")
    fs.validate(ABC + "from every a=A<1> -> b=B<1:1> select a.id as x, b.id as y insert into O;")


REFUSED = [
    # a count state as the first position
    ("from every a=A<2:3> -> b=B -> c=C" + SEL, "count state as the first pattern position"),
    ("from a=A<2> -> b=B select a.id as x, b.id as y insert into O;", "count state as the first pattern position"),
    ("from every a=A<2:> select a.id as x insert into O;", "count state as the first pattern position"),
    # a count state that may be empty
    ("from every a=A -> b=B<0:3> -> c=C" + SEL, r"may be empty \(<0:n>\)"),
    ("from every a=A -> b=B<0:> -> c=C" + SEL, r"may be empty \(<0:n>\)"),
    # sequence postfixes on a pattern state
    ("from every a=A -> b=B+ -> c=C" + SEL, r"postfix '\+' on a pattern state.*<m:n>"),
    ("from every a=A -> b=B[id > 1]* -> c=C" + SEL, r"postfix '\*' on a pattern state.*<m:n>"),
    ("from every a=A -> b=B? -> c=C" + SEL, r"postfix '\?' on a pattern state.*<m:n>"),
    ("from every a=A -> b=B+" + SEL2, r"postfix '\+' on a pattern state.*<m:n>"),
    # a logical group and a count state in one pattern
    ("from every a=A -> b=B<2:3> -> (c=C or d=A) select a.id as x, b[last].id as y insert into O;",
     "both a logical group .* and a count state"),
    ("from every a=A -> b=B and c=C -> d=A<2> select a.id as x, d[last].id as y insert into O;",
     "both a logical group .* and a count state"),
    # a count suffix on a side of a group: the message of DESIGN §12 stays
    ("from every a=A -> b=B<2:3> and c=C" + SEL, "count suffix on a side"),
    ("from every a=A -> (b=B or c=C<2:>)" + SEL, "count suffix on a side"),
    # a count state is one of the six states
    ("from every a=A -> b=B<2> -> c=C -> d=A -> e=B -> f=C -> g=A<2:3> select a.id as x insert into O;",
     "more than 6 states"),
]


@pytest.mark.parametrize("plan,word", REFUSED)
def test_refused(plan, word):
    with pytest.raises(fs.UnsupportedPlanException, match=word):
        fs.validate(ABC + plan)


MALFORMED = [
    "from every a=A -> b=B<:3> -> c=C" + SEL,
    "from every a=A -> b=B<3:2> -> c=C" + SEL,
    "from every a=A -> b=B<0> -> c=C" + SEL,
    "from every a=A -> b=B<0:0> -> c=C" + SEL,
    "from every a=A -> b=B<2:3 -> c=C" + SEL,       # a typo
    "from every a=A -> b=B<2;3> -> c=C" + SEL,
]


@pytest.mark.parametrize("plan", MALFORMED)
def test_malformed_counts_are_creation_errors_not_refusals(plan):
    """A shim tells "fall back to Siddhi" (UnsupportedPlanException) from a
    typo (any other creation error) by the exception's type."""
    with pytest.raises(fs.SiddhiAppCreationException) as e:
        fs.validate(ABC + plan)
    assert not isinstance(e.value, fs.UnsupportedPlanException)


def test_sequences_keep_their_postfixes():
    fs.validate(ABC + "from every a=A, b=B[id > 1]+, c=C select a.id as x, b[last].id as y, c.id as z insert into O;")
    fs.validate(ABC + "from every a=A, b=B<0:2>, c=C select a.id as x, b[last].id as y, c.id as z insert into O;")
