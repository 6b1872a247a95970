"""The references of the time-edge tests, away from workload.T0 (no GPU).

tests/time_edges.py moves a seeded stream along the time axis and puts jumps
on tile, chunk and batch borders.  Before any kernel is compared with them,
the references are compared with each other at those values, where they have
never been run: oracle/siddhi_oracle.py and oracle/cep_oracle.c give the same
rows on every base and jump set, both are translation-invariant (the rows at
base B are the rows at T0 with every time shifted by B - T0), and so is
tests/window_model.py on the window plans.  The stream preconditions the GPU
cases rely on are asserted here from the oracle's output alone.
"""
import numpy as np
import pytest

import time_edges as TE
from helpers import oracle_run, workload_events
from window_model import model_run

BASE_NAMES = list(TE.BASES)
CASES = [("edge", TE.W, "10 sec"), ("wide", TE.W, "10 sec"),
         ("long_within", TE.LONG_WITHIN["30 days"], "30 days"),
         ("long_within", TE.LONG_WITHIN["1 year"], "1 year")]
IDS = ["edge", "wide", "long-30days", "long-1year"]

_py = {}


def python_rows(jump_set, base_name, text):
    key = (jump_set, base_name, text)
    if key not in _py:
        w, _, _ = TE.stream(jump_set, base_name)
        _py[key] = oracle_run(TE.plan_within(text), workload_events(w)).get("O", [])
    return _py[key]


def shift_rows(rows, d):
    """Pattern rows (ts, seq, (k, p1, p2, t)) with both times moved by d."""
    return [(ts + d, seq, (k, p1, p2, t + d)) for ts, seq, (k, p1, p2, t) in rows]


def test_bases_cross_the_lines_they_are_named_for():
    for name in BASE_NAMES:
        w, _, _ = TE.stream("edge", name)
        ts = w["ts"]
        assert (np.diff(ts) >= 0).all() and int(np.abs(ts).max()) <= TE.TS_LIMIT
        lo, hi = int(ts[0]), int(ts[-1])
        first_chunk_hi = int(ts[TE.CHUNK - 1])
        if name == "neg5000":
            assert lo < 0 < first_chunk_hi
        if name in ("2^31", "2^32"):
            line = 1 << (31 if name == "2^31" else 32)
            assert lo < line < first_chunk_hi
        if name in ("epoch_wrap", "neg2^32"):
            # the low 32 bits wrap inside the first chunk
            assert (lo >> 32) != (first_chunk_hi >> 32)
        if name == "zero":
            assert lo == 0
        assert hi > lo


@pytest.mark.parametrize("base_name", BASE_NAMES)
@pytest.mark.parametrize("jump_set,within,text", CASES, ids=IDS)
def test_python_and_c_oracle_agree(jump_set, within, text, base_name):
    w, sizes, want_c, _ = TE.pattern_want(jump_set, base_name, within)
    assert sum(sizes) == len(w["ts"])
    want_py = python_rows(jump_set, base_name, text)
    assert len(want_py) > 1000
    assert want_py == want_c


@pytest.mark.parametrize("base_name", BASE_NAMES[1:])
@pytest.mark.parametrize("jump_set,within,text", CASES, ids=IDS)
def test_pattern_oracles_are_translation_invariant(jump_set, within, text, base_name):
    d = TE.BASES[base_name] - TE.T0
    assert shift_rows(python_rows(jump_set, "T0", text), d) == python_rows(jump_set, base_name, text)
    assert shift_rows(TE.pattern_want(jump_set, "T0", within)[2], d) == TE.pattern_want(jump_set, base_name, within)[2]


def straddling(w, jump_row, within=TE.W):
    a, b = TE.c_pairs(w, within)
    return sorted((int(i), int(j)) for i, j in zip(a, b) if i < jump_row <= j)


@pytest.mark.parametrize("base_name", BASE_NAMES)
def test_edge_jumps_put_exactly_w_across_a_border(base_name):
    """One pair straddles each W-1 jump, exactly W apart (it matches); none
    straddles the W jump (the planted pair is W+1 apart)."""
    w, jumps, sizes = TE.stream("edge", base_name)
    starts = TE.chunk_starts(sizes)
    (mid, j_mid), (border, j_border), (batch, j_batch) = jumps
    assert mid not in starts and mid % TE.CHUNK not in (0, TE.CHUNK - 1)
    assert border in starts and border < sizes[0] and batch == sizes[0] and batch % 2 == 1
    assert (j_mid, j_border, j_batch) == (TE.W - 1, TE.W, TE.W - 1)
    for r, j in jumps:
        dt = int(w["ts"][r] - w["ts"][r - 1])
        assert dt == j + 1
        pairs = straddling(w, r)
        assert pairs == ([(r - 1, r)] if j == TE.W - 1 else []), (r, pairs)


@pytest.mark.parametrize("base_name", BASE_NAMES)
def test_wide_chunk_spans_exactly_the_accepted_maximum(base_name):
    w, jumps, sizes = TE.stream("wide", base_name)
    starts = TE.chunk_starts(sizes)
    c0, c1 = starts[1], starts[2]
    assert int(w["ts"][c1 - 1] - w["ts"][c0]) == TE.SPAN_MAX == (1 << 31) - 1
    assert jumps[1] == (c1, 1 << 40) and c0 < jumps[0][0] < c1
    # nothing survives the 2^40 jump: no pair straddles it
    assert straddling(w, c1) == []
    assert len(straddling(w, jumps[0][0])) == 0   # 2^31 ms is past `within 10 sec` too
    a, b = TE.c_pairs(w)
    assert ((a >= c0) & (b < c1)).sum() > 500     # the wide chunk itself matches on both sides of the jump


@pytest.mark.parametrize("base_name", BASE_NAMES)
def test_long_within_matches_lie_more_than_2_31_and_2_32_apart(base_name):
    w, jumps, sizes = TE.stream("long_within", base_name)
    starts = TE.chunk_starts(sizes)
    assert all(r in starts and j == (1 << 31) - 20000 for r, j in jumps)
    assert jumps[0][0] < sizes[0] < jumps[1][0]          # a batch border (a snapshot) lies between the jumps
    assert int(w["ts"][starts[-1]] - w["ts"][0]) > 1 << 32    # chunk bases more than 2^31 (and 2^32) apart
    far = {}
    for text, within in TE.LONG_WITHIN.items():
        a, b = TE.c_pairs(w, within)
        dt = w["ts"][b] - w["ts"][a]
        assert int(dt.max()) <= within
        far[text] = (int((dt > 1 << 31).sum()), int((dt > 1 << 32).sum()))
    assert (1 << 31) < TE.LONG_WITHIN["30 days"] < (1 << 32) < TE.LONG_WITHIN["1 year"]
    assert far["30 days"] == (3, 0)      # key 62's three partials; key 63's two expired
    assert far["1 year"] == (5, 2)       # and key 63's two, 2^32 + ~20000 ms old


# ---- the window model ----------------------------------------------------------
WINDOW_PLAN = ("define stream A (k int, ts long, id int, price double);"
               "define stream B (k int, ts long, id int, price double);"
               "partition with (k of A) begin from A#window.time(50) "
               "select k, sum(id) as si, avg(id) as ai, min(id) as mni, max(id) as mxi, sum(price) as sp, "
               "avg(price) as ap, min(price) as mnp, max(price) as mxp insert into O; end;")

_model = {}


def window_stream(jump_set, base_name, jitter=0):
    """The named stream, all rows on stream A and on 8 keys (several rows of a
    key inside 50 ms); jitter: ts moved by [-jitter, jitter]."""
    from flink_siddhi import workload
    w, _, sizes = TE.stream(jump_set, base_name)
    w["stream"] = np.zeros(len(w["ts"]), np.uint8)
    w["k"] = (w["k"] % 8).astype(np.int32)
    if jitter:
        n = len(w["ts"])
        j = (workload.splitmix64(np.arange(n, dtype=np.uint64)) % np.uint64(2 * jitter + 1)).astype(np.int64)
        w["ts"] = w["ts"] + j - jitter
    return w, sizes


def window_want(jump_set, base_name, jitter=0):
    key = (jump_set, base_name, jitter)
    if key not in _model:
        w, sizes = window_stream(jump_set, base_name, jitter)
        out, live = model_run(WINDOW_PLAN, workload_events(w))
        _model[key] = (w, sizes, out.get("O", []), live)
    return _model[key]


@pytest.mark.parametrize("jitter", [0, 15])
@pytest.mark.parametrize("base_name", ["neg5000", "epoch_wrap", "neg2^32", "2^62", "neg2^62"])
def test_window_model_is_translation_invariant(base_name, jitter):
    d = TE.BASES[base_name] - TE.T0
    at_t0 = window_want("edge", "T0", jitter)[2]
    moved = window_want("edge", base_name, jitter)[2]
    assert len(at_t0) == TE.N
    assert [(ts + d, seq, data) for ts, seq, data in at_t0] == moved
