"""Hand-computed windowed-join cases (no model, no engine): events are
(stream, ts, (k, v)), rows are (ts, arrival number, data)."""

DEFS = "define stream A (k int, v int);define stream B (k int, v int);"

# ---- length + length: a row never joins rows of its own side; a window of 2
# forgets its oldest row.
#   0 A(1,10)  B's window is empty                        A: [a0]
#   1 A(1,11)  B's window is empty (a0 is A's own side)   A: [a0 a1]
#   2 B(1,20)  A: a0, a1 match, oldest first              B: [b2]
#   3 A(2,12)  B: b2 has k 1                              A: [a1 a3]
#   4 B(2,21)  A: a1 (k 1) no, a3 yes                     B: [b2 b4]
#   5 B(1,22)  A: a1 yes, a3 no                           B: [b4 b5]
#   6 A(1,13)  B: b4 (k 2) no, b5 yes; b2 has left
KAT_L_PLAN = DEFS + ("from A#window.length(2) as a join B#window.length(2) as b on a.k == b.k "
                     "select a.v as av, b.v as bv insert into O;")
KAT_L_EVENTS = [("A", 10, (1, 10)), ("A", 11, (1, 11)), ("B", 12, (1, 20)), ("A", 13, (2, 12)),
                ("B", 14, (2, 21)), ("B", 15, (1, 22)), ("A", 16, (1, 13))]
KAT_L_ROWS = [(12, 2, (10, 20)), (12, 2, (11, 20)), (14, 4, (12, 21)), (15, 5, (11, 22)), (16, 6, (13, 22))]

# ---- the exact time boundary: a row r of a time(100) side joins e while
# r.ts + 100 > e.ts.
#   0 A ts 1000 (1,1)
#   1 A ts 1001 (1,2)
#   2 B ts 1100 (1,50)  a0: 1100 > 1100 no (r.ts + T == e.ts has left); a1: 1101 > 1100 yes
#   3 B ts 1100 (1,51)  the same
#   4 B ts 1101 (1,52)  a1: 1101 > 1101 no
#   5 A ts 1101 (1,3)   B's last 3 rows: b2 b3 b4
#   6 B ts 1200 (1,53)  a5: 1201 > 1200 yes (r.ts + T == e.ts + 1 stays)
#   7 B ts 1201 (1,54)  a5: 1201 > 1201 no
KAT_T_PLAN = DEFS + ("from A#window.time(100) as a join B#window.length(3) as b on a.k == b.k "
                     "select a.v as av, b.v as bv insert into O;")
KAT_T_EVENTS = [("A", 1000, (1, 1)), ("A", 1001, (1, 2)), ("B", 1100, (1, 50)), ("B", 1100, (1, 51)),
                ("B", 1101, (1, 52)), ("A", 1101, (1, 3)), ("B", 1200, (1, 53)), ("B", 1201, (1, 54))]
KAT_T_ROWS = [(1100, 2, (2, 50)), (1100, 3, (2, 51)), (1101, 5, (3, 50)), (1101, 5, (3, 51)), (1101, 5, (3, 52)),
              (1200, 6, (3, 53))]

# ---- a filter in front of the window, no aliases, two `on` terms, a computed
# select item, time units.
#   0 A ts 0    (1,-5)  fails [v > 0]: neither probes nor enters
#   1 A ts 1    (1,5)
#   2 B ts 2    (1,3)   A: [a1]: 5 < 3 no
#   3 B ts 3    (1,7)   5 < 7: 12
#   4 A ts 4    (1,6)   B: b2 6 < 3 no, b3 6 < 7: 13; A: [a4] (length 1)
#   5 B ts 1002 (1,9)   A: [a4] 6 < 9: 15
#   6 A ts 1003 (1,1)   B: b2 1002 > 1003 no, b3 1003 > 1003 no, b5 1 < 9: 10
KAT_F_PLAN = DEFS + ("from A[v > 0]#window.length(1) join B#window.time(1 sec) on A.k == B.k and A.v < B.v "
                     "select A.v + B.v as s insert into O;")
KAT_F_EVENTS = [("A", 0, (1, -5)), ("A", 1, (1, 5)), ("B", 2, (1, 3)), ("B", 3, (1, 7)), ("A", 4, (1, 6)),
                ("B", 1002, (1, 9)), ("A", 1003, (1, 1))]
KAT_F_ROWS = [(3, 3, (12,)), (4, 4, (13,)), (1002, 5, (15,)), (1003, 6, (10,))]

KATS = {"length": (KAT_L_PLAN, KAT_L_EVENTS, KAT_L_ROWS),
        "time_boundary": (KAT_T_PLAN, KAT_T_EVENTS, KAT_T_ROWS),
        "filter_terms_computed": (KAT_F_PLAN, KAT_F_EVENTS, KAT_F_ROWS)}
