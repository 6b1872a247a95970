"""The naive event-table model (tests/table_model.py) reproduces the
hand-computed cases of tests/table_kats.py: output rows, table contents and
the number of inserts dropped."""
import pytest

import table_kats as K
from table_model import model_run


@pytest.mark.parametrize("name", sorted(K.KATS))
def test_model_reproduces_kat(name):
    plan, events, rows, tables, dropped = K.KATS[name]
    got, m = model_run(plan, events)
    assert got == rows
    for t, want in tables.items():
        assert m.table_rows(t) == want
    assert m.dropped() == dropped


def test_plan_order_includes_queries_without_a_table():
    # a filter query on the reader's output stream keeps its place in plan order
    plan = (K.DEFS + "from S[v > 100] select v as sv, k as tv insert into O;"
            "from U select k, v insert into T;" + K.JOIN)
    got, _ = model_run(plan, [("U", 1, (1, 10)), ("S", 2, (1, 101))])
    assert got == {"O": [(2, 1, (101, 1)), (2, 1, (101, 10))]}
