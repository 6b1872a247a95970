"""The sequence-grammar reference (tests/seq_ref.py: regular expressions over
a key's event string) against the oracle's automaton, bit-equal rows, on the
full quantifier grid; and, for every shape the GPU tests run, the counters
that show the GPU stream exercises what the shape can do."""
import itertools

import pytest

import seq_ref as SR
from helpers import assert_same_rows, oracle_run

GRID_N, GRID_KEYS = 1500, 3
_streams = {}


def grid_stream(n_states):
    """1500 rows, 3 keys, one more stream than the query reads."""
    if n_states not in _streams:
        w = SR.make_stream(GRID_N, GRID_KEYS, 100 + n_states, streams=n_states + 1)
        _streams[n_states] = (w, SR.events(w))
    return _streams[n_states]


def run_grid(n_states, quants_list):
    """every on / off x within absent / 6 ms of each shape, all captures;
    40 queries to an oracle app.  -> (cases, rows)."""
    w, ev = grid_stream(n_states)
    shapes = [SR.shape(q, every, within) for q in quants_list for every in (True, False) for within in (None, SR.WITHIN)]
    strings = SR.key_strings(w, n_states, SR.THRESH)
    rows = 0
    for lo in range(0, len(shapes), 40):
        part = shapes[lo:lo + 40]
        want = oracle_run(SR.plan_text(part), ev)
        for i, sh in enumerate(part):
            got, _ = SR.reference(sh, w, strings)
            assert_same_rows(got, want.get("O%d" % i, []), SR.name(sh))
            rows += len(got)
    return len(shapes), rows


@pytest.mark.parametrize("n_states", [2, 3])
def test_reference_equals_oracle_two_and_three_states(n_states):
    cases, rows = run_grid(n_states, list(itertools.product(SR.QUANT_NAMES, repeat=n_states - 1)))
    assert cases == 4 * 8 ** (n_states - 1) and rows > 100 * cases // 8


@pytest.mark.parametrize("second", SR.QUANT_NAMES)
def test_reference_equals_oracle_four_states(second):
    cases, rows = run_grid(4, [(second,) + q for q in itertools.product(SR.QUANT_NAMES, repeat=2)])
    assert cases == 4 * 64 and rows > 0


def test_gpu_shapes_are_the_issue_s_set():
    shapes = SR.gpu_shapes()
    base = [s for s in shapes if s.every and s.within is not None]
    assert sorted(len(s.quants) + 1 for s in base) == [2] * 8 + [3] * 64 + [4] * 24
    four = [s.quants for s in base if len(s.quants) == 3]
    opt = ("?", "*", "<0:2>")
    assert any(q[0] in opt and q[1] in opt for q in four) and any(q[1] in opt and q[2] in opt for q in four)
    assert any(q[1] in ("<2>", "<2:3>") and q[2] in opt for q in four)      # optional tail behind a bounded count
    assert {"+", "*", "<2:>"} <= {q[2] for q in four}
    assert sum(q[0] == "<0:2>" for q in four) >= 3
    assert sum(not s.every for s in shapes) == 12 and sum(s.within is None for s in shapes) == 12
    for s in shapes:
        assert len(s.caps) <= 4 and len(s.caps) + 1 <= 8


def test_gpu_stream_is_skewed_and_cut_inside_a_count_run():
    import numpy as np
    w = SR.gpu_stream()
    share = float((w["k"] == 0).mean())
    assert 0.35 < share < 0.45, share
    seen = len(np.unique(w["k"]))     # a dozen keys get no row (a few more by chance), in three 64-lane blocks
    assert SR.GPU_KEYS - SR.GPU_SILENT - 6 <= seen <= SR.GPU_KEYS - SR.GPU_SILENT and int(w["k"].max()) >= 2 * 64
    assert (np.diff(w["ts"]) >= 0).all() and (w["stream"] == 4).sum() > 500
    sizes = SR.gpu_batches()
    assert sizes[1] == 1 and SR.inside_count_run(w, sum(sizes[:SR.SNAPSHOT_AFTER + 1]))


# Counters a shape cannot raise, by arithmetic (seq_ref.requirements says why).
# Named here, so that a change of the rules shows up as a change of this list.
EXEMPT = {
    "discard": "two-state shapes; shapes whose states after the first are all optional; "
               "three- and four-state shapes with no finite maximum and no minimum above zero between first and last",
    "expired": "shapes whose states after the first are all optional",
    "took / at_max": "an optional state followed by optional states only",
    "at_max": "<2:3> before the last state when every later state is optional",
    "multi": "a trailing * (an optional tail)",
}


def test_exemptions_by_name():
    r = lambda q, **kw: SR.requirements(SR.shape(q, **kw))  # noqa: E731
    for q in SR.QUANT_NAMES:
        assert "discard" not in r((q,))                                   # A, B<2> has no "max + 1": consumed at max
    assert "discard" not in r(("*", "+")) and "discard" not in r(("?", "<0:2>")) and "discard" in r(("?", "+"))
    assert "expired" not in r(("*", "?")) and "expired" in r(("*", "+")) and "expired" not in r(("+",), within=None)
    assert r(("1", "<0:2>"))["at_max"] == [] and r(("1", "<0:2>"))["took"] == [] and r(("<0:2>", "1"))["took"] == [1]
    assert r(("<2:3>", "?"))["at_max"] == [] and r(("<2:3>", "1"))["at_max"] == [1] and r(("<2>", "?"))["at_max"] == [1]
    assert "multi" not in r(("1", "*")) and "multi" in r(("1", "+")) and "multi" in r(("<2:>",))
    assert r(("<2>",))["at_max"] == [1] and r(("?", "?"))["skipped"] == [1, 2]


@pytest.mark.parametrize("lo", range(0, 120, 24))
def test_gpu_shapes_are_not_vacuous_and_equal_the_oracle(lo):
    """Every shape of the GPU file, on the GPU stream: every counter its
    grammar allows is positive, and the reference equals the oracle."""
    part = SR.gpu_shapes()[lo:lo + 24]
    want = oracle_run(SR.plan_text(part), SR.events(SR.gpu_stream()))
    for i, sh in enumerate(part):
        rows, cn = SR.gpu_reference(sh)
        assert SR.missing(sh, cn) == [], SR.name(sh)
        assert_same_rows(rows, want.get("O%d" % i, []), SR.name(sh))
