"""Hand-computed event-table cases (no model, no engine): events are
(stream, ts, row), output rows are (ts, arrival number, data), table rows are
ordered by primary key.  Event i has ts 1000 + i."""

DEFS = ("define stream U (k int, v int);define stream S (k int, v int);"
        "@PrimaryKey('k') define table T (k int, v int);")
JOIN = "from S as s join T as t on s.k == t.k select s.v as sv, t.v as tv insert into O;"


def _ev(rows):
    return [(s, 1000 + i, r) for i, (s, r) in enumerate(rows)]


# ---- insert, duplicate insert (the first row stays), delete, re-insert
#   0 U(1,10)   T: {1: 10}
#   1 S(1,100)  joins 10
#   2 U(1,11)   key 1 is present: dropped, 10 stays
#   3 S(1,101)  joins 10
#   4 U(1,-1)   delete key 1
#   5 S(1,102)  nothing
#   6 U(1,12)   T: {1: 12}
#   7 S(1,103)  joins 12
#   8 S(2,104)  key 2 was never stored
#   9 U(3,-1)   delete of an absent key: nothing
_ROWS = [("U", (1, 10)), ("S", (1, 100)), ("U", (1, 11)), ("S", (1, 101)), ("U", (1, -1)), ("S", (1, 102)),
         ("U", (1, 12)), ("S", (1, 103)), ("S", (2, 104)), ("U", (3, -1))]
INSERT = (DEFS + "from U[v > 0] select k, v insert into T;from U[v < 0] select k delete T on T.k == k;" + JOIN,
          _ev(_ROWS),
          {"O": [(1001, 1, (100, 10)), (1003, 3, (101, 10)), (1007, 7, (103, 12))]},
          {"T": [(1, 12)]}, 1)

# ---- the same events under update or insert: the last row wins
#   3 S(1,101)  joins 11
UPSERT = (DEFS + "from U[v > 0] select k, v update or insert into T on T.k == k;"
          "from U[v < 0] select k delete T on k == T.k;" + JOIN,
          _ev(_ROWS),
          {"O": [(1001, 1, (100, 10)), (1003, 3, (101, 11)), (1007, 7, (103, 12))]},
          {"T": [(1, 12)]}, 0)

# ---- update of an absent key (no effect), update ... set of one attribute,
# update without set (every attribute), the table side first in the join
#   0 U(5,1,1)   update set: key 5 is absent
#   1 S(5,0,0)   nothing
#   2 U(5,10,0)  insert (5,10,0)
#   3 U(5,20,1)  set v = 20: (5,20,0)
#   4 S(5,7,0)   joins (20,0)
#   5 U(5,30,2)  update all: (5,30,2)
#   6 S(5,8,0)   joins (30,2)
#   7 U(6,40,2)  update all: key 6 is absent
#   8 S(6,9,0)   nothing
DEFS3 = ("define stream U (k int, v int, w int);define stream S (k int, v int, w int);"
         "@PrimaryKey('k') define table T (k int, v int, w int);")
UPDATE = (DEFS3 + "from U[w == 0] select k, v, w insert into T;"
          "from U[w == 1] select k, v update T set T.v = v on T.k == k;"
          "from U[w == 2] select k, v, w update T on T.k == k;"
          "from T join S on S.k == T.k select S.v as sv, T.v as tv, T.w as tw insert into O;",
          _ev([("U", (5, 1, 1)), ("S", (5, 0, 0)), ("U", (5, 10, 0)), ("U", (5, 20, 1)), ("S", (5, 7, 0)),
               ("U", (5, 30, 2)), ("S", (5, 8, 0)), ("U", (6, 40, 2)), ("S", (6, 9, 0))]),
          {"O": [(1004, 4, (7, 20, 0)), (1006, 6, (8, 30, 2))]},
          {"T": [(5, 30, 2)]}, 0)

# ---- one stream writes and reads T.  Writer first: every row joins its own
# write.  Reader first: a row sees the writes of earlier rows only.
#   0 U(1,10)  1 U(1,11)  2 U(2,12)
_SELF = _ev([("U", (1, 10)), ("U", (1, 11)), ("U", (2, 12))])
_W = "from U select k, v update or insert into T on T.k == k;"
_R = "from U as u join T as t on u.k == t.k select u.v as uv, t.v as tv insert into O;"
WRITE_READ = (DEFS + _W + _R, _SELF,
              {"O": [(1000, 0, (10, 10)), (1001, 1, (11, 11)), (1002, 2, (12, 12))]}, {"T": [(1, 11), (2, 12)]}, 0)
READ_WRITE = (DEFS + _R + _W, _SELF, {"O": [(1001, 1, (11, 10))]}, {"T": [(1, 11), (2, 12)]}, 0)

# ---- in / not in
#   0 S(1,5)   T is empty: N
#   1 U(1,10)  T: {1: 10}
#   2 S(1,6)   in T and v > 0: O
#   3 S(1,-6)  in T, v > 0 fails: neither
#   4 S(2,7)   not in T: N
IN = (DEFS + "from U select k, v insert into T;"
      "from S[v > 0 and (T.k == k) in T] select k, v insert into O;"
      "from S[not ((T.k == k) in T)] select k, v insert into N;",
      _ev([("S", (1, 5)), ("U", (1, 10)), ("S", (1, 6)), ("S", (1, -6)), ("S", (2, 7))]),
      {"O": [(1002, 2, (1, 6))], "N": [(1000, 0, (1, 5)), (1004, 4, (2, 7))]},
      {"T": [(1, 10)]}, 0)

# name -> (plan, events, {output stream: rows}, {table: rows}, inserts dropped)
KATS = {"insert_delete": INSERT, "upsert_delete": UPSERT, "update": UPDATE, "write_then_read": WRITE_READ,
        "read_then_write": READ_WRITE, "in_not_in": IN}
