"""Known answers for the sliding-window aggregates, derived by hand from the
semantics (expire -> remove -> add per kept row); shared by the model's and the
engine's tests."""

S_DEF = "define stream S (k int, v long, p double);"

# KAT-L: length(2) under a partition; (k, sum, count, min, max)
KAT_L_PLAN = (S_DEF + "partition with (k of S) begin "
              "from S#window.length(2) select k, sum(v) as s, count() as c, min(v) as mn, max(v) as mx "
              "insert into O; end;")
KAT_L_EVENTS = [("S", 1, (0, 5, 0.0)), ("S", 2, (0, 3, 0.0)), ("S", 3, (1, 10, 0.0)),
                ("S", 4, (0, 7, 0.0)), ("S", 5, (0, 1, 0.0))]
KAT_L_ROWS = [(0, 5, 1, 5, 5), (0, 8, 2, 3, 5), (1, 10, 1, 10, 10), (0, 10, 2, 3, 7), (0, 8, 2, 1, 7)]

# KAT-T: one global time(10) window; a row with ts exactly e.ts - 10 has left
KAT_T_PLAN = S_DEF + "from S#window.time(10) select sum(v) as s, count() as c insert into O;"
KAT_T_EVENTS = [("S", 0, (0, 1, 0.0)), ("S", 5, (0, 2, 0.0)), ("S", 10, (0, 4, 0.0)),
                ("S", 10, (0, 8, 0.0)), ("S", 14, (0, 16, 0.0)), ("S", 15, (0, 32, 0.0))]
KAT_T_ROWS = [(1, 1), (3, 2), (6, 2), (14, 3), (30, 4), (60, 4)]

# KAT-O: partitioned time(10), one key, ts in any order: the expiry is
# positional (in the last case the ts 20 row blocks the front, the ts 5 row stays)
KAT_O_PLAN = (S_DEF + "partition with (k of S) begin "
              "from S#window.time(10) select sum(v) as s insert into O; end;")
KAT_O_CASES = [([20, 5, 31], [1, 2, 4], [1, 3, 4]),
               ([5, 20, 12], [1, 2, 4], [1, 2, 6]),
               ([20, 5, 16], [1, 2, 4], [1, 3, 7])]


def kat_o_events(ts, vs):
    return [("S", t, (0, v, 0.0)) for t, v in zip(ts, vs)]


# KAT-F: fp64 sums are the sequence of += and -=, not a fresh sum
KAT_F_PLAN = (S_DEF + "partition with (k of S) begin "
              "from S#window.length(2) select sum(p) as s, avg(p) as a insert into O; end;")
KAT_F_EVENTS = [("S", i + 1, (0, 0, p)) for i, p in enumerate((0.1, 0.7, 0.3, 0.9))]
KAT_F_SUMS = [0.1, 0.7999999999999999, 1.0, 1.2000000000000002]
KAT_F_AVGS = [0.1, 0.7999999999999999 / 2, 1.0 / 2, 1.2000000000000002 / 2]
