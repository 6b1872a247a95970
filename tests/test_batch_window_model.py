"""The naive batch-window model (tests/batch_window_model.py) against hand-made
answers and against references that are not list automata: a numpy reshape
(`lengthBatch`), a floor-division grouping (`externalTimeBatch` on a
non-decreasing clock) and a brute force over batch prefixes (`having`)."""
import numpy as np

from flink_siddhi import workload
from helpers import workload_events
import batch_window_model as M

EV2 = ("define stream A (k int, ts long, id int, price double);"
       "define stream B (k int, ts long, id int, price double);")


def part(q):
    return "partition with (k of A) begin " + q + " end;"


def rows(plan, events):
    return M.model_run(plan, events)[0].get("O", [])


# ---------------------------------------------------------------- KATs ------
def test_kat1_length_batch():
    assert rows(M.KAT1_PLAN, M.KAT1_EVENTS) == M.KAT1_ROWS


def test_kat2_having_picks_an_earlier_row_or_none():
    out, st = M.model_run(M.KAT2_PLAN, M.KAT2_EVENTS)
    assert out["O"] == M.KAT2_ROWS
    assert st == {"closed": 2, "silent": 1, "early": 1}


def test_kat3_external_time_batch_is_positional():
    assert rows(M.KAT3_PLAN, M.KAT3_EVENTS) == M.KAT3_ROWS
    # the successive ends, and the pending last row
    rt = M.BatchWindowModel(M.KAT3_PLAN)
    ends = []
    for sid, ts, row in M.KAT3_EVENTS:
        rt.send(sid, ts, row)
        ends.append(rt.instances[0][7].end)
    assert ends == [110, 110, 110, 120, 130, 130, 140, 150]
    assert [r[2] for _, r in rt.instances[0][7].rows] == [140]


def test_kat4_fp64_left_fold_from_plus_zero():
    assert M.bits(rows(M.KAT4_PLAN, M.KAT4_EVENTS)) == M.bits(M.KAT4_ROWS)
    s = 0.0
    for v in (0.1, 0.7):
        s += v
    assert M.KAT4_ROWS[0][2] == (s, s / 2)
    assert M.bits(rows(M.KAT4Z_PLAN, M.KAT4Z_EVENTS)) == M.bits(M.KAT4Z_ROWS)
    assert M.bits(M.KAT4Z_ROWS) != M.bits([(1000, 0, (0.0, 0.0))])


# --------------------------------------------- independent references -------
N, KEYS = 20000, 512
_W = {}


def gen():
    if "w" not in _W:
        _W["w"] = workload.generate(0, N, KEYS, rate=1)
    return _W["w"]


def by_key(w, mask):
    """key -> arrival numbers of its kept rows, ascending."""
    idx = np.nonzero(mask)[0]
    order = np.argsort(w["k"][idx], kind="stable")
    idx = idx[order]
    ks, starts = np.unique(w["k"][idx], return_index=True)
    return {int(k): g for k, g in zip(ks, np.split(idx, starts[1:]))}


def test_length_batch_equals_a_reshape():
    n = 3
    w = gen()
    plan = EV2 + part("from A#window.lengthBatch(%d) select k, id, sum(id) as s, min(price) as mn, count() as c "
                      "insert into O;" % n)
    want = []
    for k, g in by_key(w, w["stream"] == 0).items():
        full = len(g) // n * n
        if not full:
            continue
        gi = g[:full].reshape(-1, n)
        ids = w["id"][gi].astype(np.int64)
        mn = w["price"][gi].min(axis=1)
        for b in range(gi.shape[0]):
            last = gi[b, -1]
            want.append((int(w["ts"][last]), int(last), (k, int(w["id"][last]), int(ids[b].sum()), float(mn[b]), n)))
    want.sort(key=lambda r: r[1])
    got = rows(plan, workload_events(w))
    assert got == want
    assert len(got) >= 1000


def test_external_time_batch_on_a_clock_equals_floor_division():
    t = 4000
    w = gen()
    assert (np.diff(w["ts"]) >= 0).all()
    plan = EV2 + part("from A#window.externalTimeBatch(ts, %d) select k, id, sum(price) as s, count() as c "
                      "insert into O;" % t)
    want = []
    for k, g in by_key(w, w["stream"] == 0).items():
        x = w["ts"][g]
        grp = (x - x[0]) // t
        cuts = np.nonzero(np.diff(grp))[0] + 1          # first row of every later group
        lo = 0
        for c in cuts:
            s = 0.0
            for v in w["price"][g[lo:c]].tolist():
                s += v
            last = g[c - 1]
            want.append((int(w["ts"][last]), int(g[c]), (k, int(w["id"][last]), s, int(c - lo))))
            lo = c
    want.sort(key=lambda r: r[1])
    got = rows(plan, workload_events(w))
    assert got == want
    assert len(got) >= 1000


def test_having_equals_brute_force_over_prefixes():
    n = 3
    w = gen()
    plan = EV2 + part("from A#window.lengthBatch(%d) select k, id, sum(id) as s having s < 60 and id > 5 "
                      "insert into O;" % n)
    want, silent, early = [], 0, 0
    for k, g in by_key(w, w["stream"] == 0).items():
        for b in range(len(g) // n):
            batch = g[b * n:(b + 1) * n]
            pick = None
            for m in range(1, n + 1):                   # prefix of m rows, judged at its last row
                s = int(w["id"][batch[:m]].astype(np.int64).sum())
                if s < 60 and int(w["id"][batch[m - 1]]) > 5:
                    pick = (m, s)
            if pick is None:
                silent += 1
                continue
            early += pick[0] != n
            row = batch[pick[0] - 1]
            want.append((int(w["ts"][row]), int(batch[-1]), (k, int(w["id"][row]), pick[1])))
    want.sort(key=lambda r: r[1])
    out, st = M.model_run(plan, workload_events(w))
    assert out["O"] == want
    assert (st["silent"], st["early"]) == (silent, early)
    assert silent > 0 and early > 0 and len(want) >= 1000
