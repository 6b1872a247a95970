"""Snapshots written by the commit before the host-runtime refactor
(tests/golden/snapshots/, scripts/make_snapshot_fixtures.py) against this build:

(a) a fixture restores into a fresh runtime, and the rows emitted before the
    snapshot plus the rows of the rest of the stream are the oracle's / the
    model's rows of the whole stream, bit for bit;
(b) right after the restore, snapshot() returns the fixture's bytes;
(c) this build, fed the first part itself, writes the fixture's bytes.

(b) and (c) hold for the fixtures whose bytes the writing commit itself
reproduces ("byte_exact" in the JSON, which says why where it is false).
"""
import json
from pathlib import Path

import pytest

import snapshot_cases as SC
from helpers import assert_same_rows

pytestmark = pytest.mark.gpu

DIR = Path(__file__).parent / "golden" / "snapshots"
_REF = {}


def fixture(case):
    doc = json.loads((DIR / (case + ".json")).read_text())
    c = SC.CASES[case]
    assert (doc["split"], doc["n"], doc["keys"], doc["options"]) == (c["split"], c["n"], c["keys"], c["opts"])
    rows = {o: [(ts, seq, tuple(data)) for ts, seq, data in r] for o, r in doc["rows"].items()}
    return (DIR / (case + ".bin")).read_bytes(), rows, doc["byte_exact"]


def reference(case):
    if case not in _REF:
        _REF[case] = SC.reference(case)
    return _REF[case]


def test_at_least_five_fixtures_pin_their_bytes():
    assert sorted(p.stem for p in DIR.glob("*.bin")) == sorted(SC.CASES)
    assert sum(fixture(c)[2] for c in SC.CASES) >= 5


@pytest.mark.parametrize("case", list(SC.CASES))
def test_fixture_restores_and_the_run_continues(case):
    snap, before, exact = fixture(case)
    c = SC.CASES[case]
    rt = SC.runtime(case)
    rt.restore(snap)
    again = rt.snapshot()
    after = SC.feed(rt, case, SC.stream(case), c["split"], c["n"], True)
    rt.shutdown()
    want = reference(case)
    for o in c["outs"]:
        assert_same_rows(before[o] + after[o], want.get(o, []), "%s %s" % (case, o))
    assert sum(len(after[o]) for o in c["outs"]) > 0
    if exact:
        assert again == snap, "snapshot() after restore differs from the fixture"


@pytest.mark.parametrize("case", list(SC.CASES))
def test_this_build_writes_the_fixture(case):
    snap, before, exact = fixture(case)
    mine, rows = SC.first_part(case)
    for o in SC.CASES[case]["outs"]:
        assert_same_rows(rows[o], before[o], "%s %s before the snapshot" % (case, o))
    if exact:
        assert mine == snap, "this build's snapshot differs from the fixture (%d vs %d bytes)" % (len(mine), len(snap))
