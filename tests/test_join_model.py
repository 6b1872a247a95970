"""The naive join model (tests/join_model.py) against the hand-computed cases
and the ITCase fixture: the GPU tests compare the engine with this model, so
the model itself is pinned here, without a GPU."""
import json
from pathlib import Path

import pytest

import join_kats as K
from join_model import model_run

FIXTURE = json.loads((Path(__file__).parent / "golden" / "join_itcase.json").read_text())


@pytest.mark.parametrize("name", sorted(K.KATS))
def test_model_matches_hand_computed_rows(name):
    plan, events, rows = K.KATS[name]
    got, _ = model_run(plan, events)
    assert got.get("O", []) == rows


def test_model_row_never_joins_its_own_side():
    plan, events, _ = K.KATS["length"]
    got, _ = model_run(plan, [e for e in events if e[0] == "A"])
    assert got == {}


@pytest.mark.parametrize("order", ["events_stream1_first", "events_stream2_first"])
def test_model_itcase_fixture(order):
    events = [(s, ts, tuple(row)) for s, ts, row in FIXTURE[order]]
    got, m = model_run(FIXTURE["plan"], events)
    rows = got["JoinStream"]
    assert len(rows) == 5                                   # SiddhiCEPITCase.java:326
    assert [list(d) for _, _, d in rows] == FIXTURE["expected"]
    assert [ts for ts, _, _ in rows] == [e[0] for e in FIXTURE["expected"]]
    # the second row of each pair triggers the match
    assert [s for _, s, _ in rows] == [1, 3, 5, 7, 9]
    assert m.joins[0].triggered == ([0, 5] if order == "events_stream1_first" else [5, 0])


def test_model_runs_other_queries_on_the_oracle():
    plan = K.KAT_L_PLAN + "from A[v > 10] select k, v insert into F;"
    got, _ = model_run(plan, K.KAT_L_EVENTS)
    assert got["O"] == K.KAT_L_ROWS
    assert got["F"] == [(11, 1, (1, 11)), (13, 3, (2, 12)), (16, 6, (1, 13))]
