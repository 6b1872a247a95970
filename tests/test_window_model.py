"""The window reference model (tests/window_model.py) against hand-derived
known answers and a brute-force recomputation over the window membership, so
the model is checked by something other than itself."""
import random

import window_kats as K
from window_model import model_run, strip_windows


def rows_of(out, name="O"):
    return [data for _, _, data in out.get(name, [])]


def test_kat_length():
    out, live = model_run(K.KAT_L_PLAN, K.KAT_L_EVENTS)
    assert rows_of(out) == K.KAT_L_ROWS
    assert live == 2


def test_kat_time_exact_boundary():
    out, live = model_run(K.KAT_T_PLAN, K.KAT_T_EVENTS)
    assert rows_of(out) == K.KAT_T_ROWS
    assert live == 4


def test_kat_time_any_order():
    for ts, vs, sums in K.KAT_O_CASES:
        out, _ = model_run(K.KAT_O_PLAN, K.kat_o_events(ts, vs))
        assert [d[0] for d in rows_of(out)] == sums, (ts, vs)


def test_kat_fp64_drift():
    out, _ = model_run(K.KAT_F_PLAN, K.KAT_F_EVENTS)
    got = rows_of(out)
    assert [d[0] for d in got] == K.KAT_F_SUMS
    assert K.KAT_F_SUMS[3] != 0.3 + 0.9          # the drift is part of the behaviour
    assert [d[1] for d in got] == K.KAT_F_AVGS


def test_strip_windows_units():
    plan = ("define stream S (k int, v long);"
            "from S#window.time(2 min 30 sec) select sum(v) as s insert into O;"
            "from S[v > 1] select v insert into P;"
            "from S[v > 1]#window.length(7) select count() as c insert into Q;")
    stripped, specs = strip_windows(plan)
    assert "#" not in stripped
    assert specs == [("time", 150000), None, ("length", 7)]


def _generated(n, keys, seed, jitter):
    rnd = random.Random(seed)
    ev = []
    t = 0
    for _ in range(n):
        t += rnd.choice((0, 0, 1, 1, 2, 5))
        ts = t + (rnd.randint(-6, 6) if jitter else 0)
        ev.append(("S", ts, (rnd.randrange(keys), rnd.randint(-(1 << 62), 1 << 62), rnd.random())))
    return ev


def _brute(events, members_of):
    """count, long sum (wrapped), min, max of v over each row's window membership."""
    want = []
    for i in range(len(events)):
        vs = [events[j][2][1] for j in members_of(i)]
        s = sum(vs)
        s = (s + (1 << 63)) % (1 << 64) - (1 << 63)
        want.append((len(vs), s, min(vs), max(vs)))
    return want


PLAN_GEN = ("define stream S (k int, v long, p double);"
            "partition with (k of S) begin from S#window.%s select count() as c, sum(v) as s, "
            "min(v) as mn, max(v) as mx insert into O; end;")


def test_length_membership_brute_force():
    ev = _generated(600, 3, 1, False)
    for n in (1, 2, 5, 16):
        out, live = model_run(PLAN_GEN % ("length(%d)" % n), ev)
        # membership: the last n kept rows of the key, by rank
        by_key = {}
        for i, e in enumerate(ev):
            by_key.setdefault(e[2][0], []).append(i)

        def members(i, n=n):
            r = by_key[ev[i][2][0]]
            pos = r.index(i)
            return r[max(0, pos - n + 1):pos + 1]

        assert rows_of(out) == _brute(ev, members), n
        assert live == n


def test_time_membership_brute_force_positional():
    for jitter in (False, True):
        ev = _generated(600, 3, 2, jitter)
        for t in (1, 4, 11):
            out, _ = model_run(PLAN_GEN % ("time(%d)" % t), ev)
            # replay the positional front-pop rule per key on indices only
            fronts = {}
            member = []
            for i, e in enumerate(ev):
                q = fronts.setdefault(e[2][0], [])
                while q and ev[q[0]][1] + t <= e[1]:
                    q.pop(0)
                q.append(i)
                member.append(list(q))
            assert rows_of(out) == _brute(ev, lambda i: member[i]), (jitter, t)


def test_global_window_group_by_differs_from_per_group_when_unordered():
    # group by + #window.time outside a partition: one window for all groups.
    # Key 1's row with ts 20 sits in front of key 0's row with ts 5 and blocks it.
    plan = ("define stream S (k int, v long, p double);"
            "from S#window.time(10) select k, sum(v) as s group by k insert into O;")
    ev = [("S", 20, (1, 1, 0.0)), ("S", 5, (0, 2, 0.0)), ("S", 16, (0, 4, 0.0))]
    out, live = model_run(plan, ev)
    assert rows_of(out) == [(1, 1), (0, 2), (0, 6)]      # a per-key window would give (0, 4) last
    assert live == 3
