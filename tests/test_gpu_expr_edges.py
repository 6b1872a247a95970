"""Edge-value parity of every device expression evaluator (not only the
interpreter): the edge table of expr_ref.EDGES (INT_MIN, LONG_MIN, negative
dividends and divisors, constant zero divisors, NaN, +-inf, -0.0, denormals,
long -> float, float column against a double constant) through

  A  the three filter paths: k_filterc's register term list, k_filter's term
     list with its own loads, the interpreter;
  B  int division / remainder by a constant (div32_magic / div32_apply);
  C  the keyed pattern paths: closed form, fast partition pass, interpreter
     partition pass, and walk conditions / select items over captures;
  D  a multi-query group: k_mqpart condition bits and both `having` units;
  E  derived streams: k_derive's streaming instances, its row-by-row
     fallback, and a term-list producer of plain copies.

Expected rows: expr_ref (numpy, column-wise) for filters and projections,
the Python oracle for keyed / aggregate / chained apps; compared with
expr_ref.same_rows_bits (float / double by bit pattern, any NaN = any NaN, a
reference null = the engine's stand-in 0).

Which kernel instance runs is not visible in stats() beyond one launch
counter per family, so each case is built from the engine's own selection
rule, cited where the case is built.  Every literal in plan text is exact in
its type.  Every case selects >= 16 and rejects >= 16 rows in the reference
(`_nonvacuous`), except where the expression is constant by arithmetic (said
at the case).
"""
import numpy as np
import pytest

import expr_ref as X
import flink_siddhi as fs
import siddhi_oracle as O
from flink_siddhi import _lib as L
from helpers import engine_rows, oracle_run

pytestmark = pytest.mark.gpu

S_DEF = "define stream S (a int, b long, c float, d double, e bool, s string);"
NAMES = ("x", "y", "z")
ABSENT = "zz"                       # interned, never in a row
# Column i cycles through its edge table, padded with full-range random
# values (fresh ones every cycle) to a prime period; the periods are pairwise
# coprime, so every pair of edge values of two columns shares a row within
# the first 29 * 31 rows and every edge value meets every per-lane row
# position of the register paths.
PERIOD = {"a": 29, "b": 23, "c": 19, "d": 31, "e": 2, "s": 3}


def _random(t, n, rng):
    if t == O.INT:
        return rng.integers(X.INT_MIN, X.INT_MAX, n, dtype=np.int64, endpoint=True).astype(np.int32)
    if t == O.LONG:
        return rng.integers(X.LONG_MIN, X.LONG_MAX, n, dtype=np.int64, endpoint=True)
    if t == O.FLOAT:     # any bit pattern: NaNs with payloads, denormals
        return rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32).view(np.float32)
    return rng.integers(0, 1 << 64, n, dtype=np.uint64).view(np.float64)


def edge_cycle(edges, n, period, rng, t):
    assert len(edges) <= period
    out = _random(t, n, rng)
    i = np.arange(n) % period
    m = i < len(edges)
    out[m] = np.asarray(edges)[i[m]]
    return out


def s_columns(n, ids, seed=1):
    """The six columns of S; `ids`: name -> dictionary id of the string column."""
    rng = np.random.default_rng(seed)
    cols = [edge_cycle(X.EDGES[t], n, PERIOD[c], rng, t)
            for c, t in zip("abcd", (O.INT, O.LONG, O.FLOAT, O.DOUBLE))]
    i = np.arange(n)
    cols.append((i % 2).astype(np.uint8))
    cols.append(np.array([ids[nm] for nm in NAMES], np.int32)[i % 3])
    return cols


def _input_row(cols):
    return lambda r: tuple(c[r].item() for c in cols)


def _nonvacuous(nsel, n, ctx):
    assert nsel >= 16 and n - nsel >= 16, "%s: reference selects %d of %d rows" % (ctx, nsel, n)


def run_filter(plan, n, path="host", seed=1, cols_fn=s_columns):
    """One filter app over n rows -> (engine rows, columns, ids, stats).
    path "host": one host batch; "odd": a device batch whose columns start
    at an odd element of their allocations."""
    rt = fs.SiddhiAppRuntime(plan)
    rt.add_callback("O")
    ids = {nm: rt.intern(nm) for nm in NAMES + (ABSENT,)}
    cols = cols_fn(n, ids, seed)
    ts = np.arange(n, dtype=np.int64) * 3 + 5
    if path == "host":
        rt.send("S", ts, cols)
    else:
        import torch

        def odd(x):
            t = torch.empty(len(x) + 1, dtype=torch.from_numpy(x[:1]).dtype, device="cuda")
            t[1:] = torch.from_numpy(x)
            return t[1:]
        rt.send("S", odd(ts), [odd(c) for c in cols])
    rt.flush()
    got = engine_rows(rt.collect("O"))
    st = rt.stats()
    rt.shutdown()
    return got, cols, ts, ids, st


def check_filter(plan, n, path="host", seed=1, cols_fn=s_columns, vacuous_ok=False, ctx=""):
    got, cols, ts, ids, st = run_filter(plan, n, path, seed, cols_fn)
    assert st.kernel_launches[L.K_FILTER] > 0
    idx, outs, nulls, types = X.filter_project(plan, cols, strings=ids)
    if not vacuous_ok:
        _nonvacuous(len(idx), n, ctx or plan)
    want = X.rows_of(ts[idx], idx, outs, nulls)
    X.same_rows_bits(got, want, types, ctx or plan, inputs=_input_row(cols))
    return len(idx)


# ---------------------------------------------------------------- group A --
FLT_MAX_LIT = "340282346638528859811704183484516925440.0f"
F01_LIT = "0.100000001490116119384765625f"          # float(0.1f), exactly
# (predicate, "and" | "or": how further terms join it)
PREDICATES = [
    # comparisons: every column type against a constant of every numeric
    # type, all six operators, both operand orders
    ("a > 7", "and"), ("65537L >= a", "and"), ("a == 16777216.0f", "and"), ("a != 16777217.0", "and"),
    ("b < 2", "and"), ("4294967297L <= b", "and"),
    ("b > 4611686018427387904.0f", "and"),            # long -> float: 2^62 + 2^38 + 1 rounds up, once
    ("-4611686018427387904.0f >= b", "and"),
    ("b == 9007199254740992.0", "and"),               # 2^53 + 1 -> 2^53
    ("c <= 1", "and"), ("c < 16777217L", "and"), ("0.375f == c", "and"), ("c <= 0.0f", "and"),
    ("c > 1.0000001", "and"),                         # float column widened, not the constant narrowed
    ("d >= 1", "and"), ("d < 9007199254740993L", "and"), ("d == " + F01_LIT, "and"),
    ("0.30000000000000004 == d", "and"), ("d != 0.0", "and"), ("0.0 > d", "and"),
    # column op constant, five operators in four types
    ("a + 2147483647 < 0", "and"), ("a - 7 > 2147483640", "and"), ("a * 65536 == 0", "and"),
    ("a / -7 <= -9362", "and"), ("a % -7 == -1", "and"),
    ("b + 9223372036854775807L < 0", "and"), ("b - 2 >= 9223372036854775806L", "and"),
    ("b * 4294967297L > 0", "and"), ("b / -1L < 0", "and"), ("b % -4294967297L == -1", "and"),
    ("b % 2 == -1", "and"),
    ("c + 1.0f == 1.0f", "and"), ("c - 1.0f < -1.0f", "and"), ("c * 0.0f != 0.0f", "and"),
    ("c / 0.0f > " + FLT_MAX_LIT, "and"), ("c % 1.5f == 1.0f", "and"), ("c % 0.0f != 1.0f and a > 5", "and"),
    ("d + 0.1 > 0.30000000000000004", "and"), ("d - 1.5 <= -0.5", "and"), ("d * 0 != 0", "and"),
    ("d / 0.0 > 1.0e300", "and"), ("d % 1.5 < 0.0", "and"), ("d % 0.0 != 1.0 and 0 > a", "and"),
    # long -> float arithmetic
    ("b * 1.0f > 4611686018427387904.0f", "and"), ("a * 1.0f == 16777216.0f", "and"),
    # bool and string
    ("e == true", "and"), ("false != e", "and"), ("e", "and"), ("s == 'x'", "and"), ("'y' != s", "and"),
    # null terms in an OR and in an AND list
    ("a / 0 == 0 or a > 5", "or"), ("b % 0 == 0 or b < 0 or b / 0L != 1L", "or"),
    ("a % -7 == -1 or d < 0.0", "or"),
]
# identically null: no row, alone; the OR forms above are their non-vacuous twins
NULL_EVERYWHERE = ["a / 0 == 0", "a % 0 == 0 and a > 5", "b / 0L != 1L", "0 <= b % 0"]
# true (and-ed on) / false (or-ed on) for every value of the column
FILL = {"a": ("a * 0 == 0", "a * 0 == 1"), "b": ("b * 0 == 0", "b * 0 == 1"),
        "c": ("c * 0.0f != 1.0f", "c * 0.0f == 1.0f"), "d": ("d * 0.0 != 1.0", "d * 0.0 == 1.0"),
        "s": ("s != '%s'" % ABSENT, "s == '%s'" % ABSENT)}
N_A = 8192 + 77          # crosses k_filter's 8192-row tile and k_filterc's 2048-row tiles, ragged


def _columns_of(pred):
    e = O.parse_app(S_DEF + "from S[%s] select * insert into O;" % pred).queries[0].filters[0]
    names, out = "abcdes", []

    def walk(x):
        if x.kind == "attr" and names[x.slot[1]] not in out:
            out.append(names[x.slot[1]])
        for y in x.args:
            walk(y)
    walk(e)
    nterms = 1 + pred.count(" and ") + pred.count(" or ")
    return out, nterms


def filter_plan(pred, join, path):
    """A1: <= 3 distinct columns, plain projection, host batch: k_filterc
    (run_filter in engine.cpp: `fc`).
    A2: the same term list padded to 4 terms over 4 distinct columns, which
    k_filterc refuses (npref == 3 -> fc = false): k_filter<false>,
    eval_terms_run; a list that cannot reach 4 columns within kMaxTerms = 4
    terms goes in as a device batch whose columns are not aligned for pair
    loads instead (`al(...)` fails -> fc = false).
    A3: not (not (p)): lower_atom takes BIN comparisons and bare bool
    attributes only (frontend.cpp: `if (e->k != Expr::BIN) return false`), so
    the filter compiles to a VM program: k_filter<true>."""
    how = "host"
    if path == "A2":
        used, nterms = _columns_of(pred)
        free = [c for c in "abcds" if c not in used]
        add = 4 - len(used)
        if nterms + add <= 4:
            pred = (" %s " % join).join([pred] + [FILL[c][0 if join == "and" else 1] for c in free[:add]])
        else:
            how = "odd"
    elif path == "A3":
        pred = "not (not (%s))" % pred
    return S_DEF + "from S[%s] select * insert into O;" % pred, how


@pytest.mark.parametrize("path", ["A1", "A2", "A3"])
@pytest.mark.parametrize("pred,join", PREDICATES, ids=[p for p, _ in PREDICATES])
def test_filter_paths(pred, join, path):
    plan, how = filter_plan(pred, join, path)
    check_filter(plan, N_A, how, ctx="%s %s" % (path, pred))


@pytest.mark.parametrize("path", ["A1", "A2", "A3"])
@pytest.mark.parametrize("pred", NULL_EVERYWHERE)
def test_null_everywhere_selects_nothing(pred, path):
    plan, how = filter_plan(pred, "and", path)
    assert check_filter(plan, N_A, how, vacuous_ok=True, ctx="%s %s" % (path, pred)) == 0


# an edge value of each column, written as a constant of each numeric type
CMP_CONST = {"a": ("7", "7L", "7.0f", "7.0"), "b": ("1", "2147483648L", "2147483648.0f", "2147483648.0"),
             "c": ("1", "1L", "1.0f", "1.0"), "d": ("1", "1L", "1.0f", "1.0")}


@pytest.mark.parametrize("path", ["A1", "A2", "A3"])
@pytest.mark.parametrize("ktype", range(4), ids=["int", "long", "float", "double"])
@pytest.mark.parametrize("col", "abcd")
def test_comparison_matrix(col, ktype, path):
    """All six operators, both operand orders, for every (column type,
    constant type) pair; PREDICATES holds the pairs' rounding edges."""
    k = CMP_CONST[col][ktype]
    for op in ("==", "!=", "<", "<=", ">", ">="):
        for pred in ("%s %s %s" % (col, op, k), "%s %s %s" % (k, op, col)):
            plan, how = filter_plan(pred, "and", path)
            check_filter(plan, N_A, how, ctx="%s %s" % (path, pred))


@pytest.mark.parametrize("items", [
    "-c as nc, c * 0.0f as cz, c - 0.0f as cs, 0.0f - c as sc, c % 1.5f as cm, c / 0.0f as ci, c * 2.5f as y, "
    "d % 1.0 as dm, -d as nd, d * 0 as dz, d - (-0.0) as dn, d / 0.0 as di",
    "a % -7 as r, a / -1 as q1, -a as na, a * 65537 as m, b % -1L as r1, -b as nb, b * 1.0f as bf, b + c as bc, "
    "a * 1.0f as af, b / a as q, a % (a / 65536) as rq, b - d as bd"], ids=["float", "int"])
def test_projection_signs_and_nulls(items):
    """Computed select items (the interpreter): the sign of a zero result,
    NaN / inf results, wraps and nulls are visible here, bit for bit."""
    plan = S_DEF + "from S[a != 7] select %s insert into O;" % items
    check_filter(plan, N_A, ctx="projection")


# ---------------------------------------------------------------- group B --
DIV_K = [1, -1, 2, -2, 3, 7, -7, 10, 641, 65536, 65537, -65537, 2147483647, -2147483647]
N_B = 65536 + 77
S1_DEF = "define stream S (a int);"


def div_column(K):
    """The edge table plus m K + {-1, 0, 1} for m in {0, +-1, +-2,
    +-(2^31 / |K|)} clipped to int, cycled with fresh full-range random
    values to the prime period 53."""
    special = [m * K + o for m in (0, 1, -1, 2, -2, (1 << 31) // abs(K), -((1 << 31) // abs(K)))
               for o in (-1, 0, 1)] if K else []
    vals = np.concatenate([X.EDGES[O.INT].astype(np.int64), np.clip(special, X.INT_MIN, X.INT_MAX)])
    vals = vals.astype(np.int32)

    def cols(n, ids, seed):
        return [edge_cycle(vals, n, 53, np.random.default_rng(seed), O.INT)]
    return cols


def _lit(v):
    assert v != X.INT_MIN       # has no literal
    return str(int(v))


@pytest.mark.parametrize("op", ["/", "%"])
@pytest.mark.parametrize("K", DIV_K)
def test_int_division_by_constant(K, op):
    """`a op K cmp const` on k_filterc (one column, host batch): arith_run's
    magic-number division.  The constants come from the reference on this
    data: == its most frequent result, < and >= its median result."""
    cols_fn = div_column(K)
    a = cols_fn(N_B, None, 2)[0]
    e = O.parse_app(S1_DEF + "from S select a %s %s as r insert into O;" % (op, _lit(K))).queries[0].select[0].expr
    r, null = X.evaluate(e, lambda slot: a, N_B)
    assert not null.any()
    u, cnt = np.unique(r, return_counts=True)
    mode, med = u[np.argmax(cnt)], np.sort(r)[N_B // 2]
    constant = len(u) == 1          # a % 1, a % -1: 0 whatever a is
    assert constant == (op == "%" and abs(K) == 1)
    for cmp_, k in (("==", mode), ("<", med), (">=", med)):
        plan = S1_DEF + "from S[a %s %s %s %s] select a insert into O;" % (op, _lit(K), cmp_, _lit(k))
        check_filter(plan, N_B, seed=2, cols_fn=cols_fn, vacuous_ok=constant)


@pytest.mark.parametrize("op", ["/", "%"])
def test_int_division_by_constant_zero(op):
    cols_fn = div_column(0)
    for cmp_ in ("==", "!=", "<", ">="):
        plan = S1_DEF + "from S[a %s 0 %s 0] select a insert into O;" % (op, cmp_)
        assert check_filter(plan, N_B, seed=2, cols_fn=cols_fn, vacuous_ok=True) == 0
    plan = S1_DEF + "from S[a %s 0 == 0 or a > 5] select a insert into O;" % op
    check_filter(plan, N_B, seed=2, cols_fn=cols_fn)


# ------------------------------------------------- keyed / multi-stream apps --
def run_app(plan, names, ts, cols, streams, outs, cuts=None, device=False, **opts):
    """A batch that mixes identically-defined streams (`streams`: per-row
    index into `names`) -> ({out: engine rows}, stats).  cuts: slice bounds;
    device=True sends slices of one device allocation (odd first rows)."""
    rt = fs.SiddhiAppRuntime(plan, **opts)
    for o in outs:
        rt.add_callback(o)
    n = len(ts)
    cuts = [0, n] if cuts is None else cuts
    if device:
        import torch
        dts = torch.from_numpy(ts).cuda()
        dst = None if streams is None else torch.from_numpy(streams).cuda()
        dcols = [torch.from_numpy(np.ascontiguousarray(c)).cuda() for c in cols]
    for s, e in zip(cuts[:-1], cuts[1:]):
        if device:
            rt.send(names[0], dts[s:e], [c[s:e] for c in dcols], streams=None if dst is None else dst[s:e])
        else:
            rt.send(names[0], ts[s:e], [c[s:e] for c in cols], streams=None if streams is None else streams[s:e])
        rt.flush()
    got = {o: engine_rows(rt.collect(o)) for o in outs}
    st = rt.stats()
    rt.shutdown()
    return got, st


def events_of(names, ts, cols, streams):
    cl = [c.astype(bool).tolist() if c.dtype == np.uint8 else c.tolist() for c in cols]
    tl, sl = ts.tolist(), streams.tolist()
    return [(names[sl[i]], tl[i], tuple(c[i] for c in cl)) for i in range(len(tl))]


def out_types(plan, out):
    return [a.type for a in O.parse_app(plan).out_streams[out].attrs]


_ORACLE = {}


def oracle_cached(plan, key, make_events):
    if (plan, key) not in _ORACLE:
        _ORACLE[(plan, key)] = oracle_run(plan, make_events())
    return _ORACLE[(plan, key)]


# ---------------------------------------------------------------- group C --
KEYS = 64
T0 = 1_500_000_000_000
AB_DEF = ("define stream A (k int, a int, b long, c float, d double);"
          "define stream B (k int, a int, b long, c float, d double);")
N_C = 2 * 8192 + 77          # two closed-form tiles (8192 rows; 8 partition-pass tiles of 2048) and a ragged tail
_KEYED = {}


def keyed_data(n, nstreams=2, seed=3):
    """(ts, [k, a, b, c, d], stream): the edge columns of S behind a key
    column of 64 keys, one event per ms, streams drawn at random."""
    if (n, nstreams, seed) not in _KEYED:
        rng = np.random.default_rng(seed)
        k = rng.integers(0, KEYS, n).astype(np.int32)
        st = rng.integers(0, nstreams, n).astype(np.uint8)
        cols = s_columns(n, {nm: 0 for nm in NAMES}, seed)[:4]
        _KEYED[(n, nstreams, seed)] = (T0 + np.arange(n, dtype=np.int64), [k] + cols, st)
    return _KEYED[(n, nstreams, seed)]


def pattern_plan(f, g, x, computed):
    sel = "s1.k as k, s1.%s as x1, s2.%s as x2" % (x, x)
    if computed:
        sel += ", s2.%s - s1.%s as dx" % (x, x)
    return AB_DEF + ("partition with (k of A, k of B) begin from every s1=A[%s] -> s2=B[%s] within 10 sec "
                     "select %s insert into O; end;" % (f, g, sel))


# (predicate as f and as g, the column the select list carries)
KEYED_PREDICATES = [("a % -7 == -1", "a"),                       # negative constant, negative data
                    ("c <= 0.0f", "c"),                          # NaN is not, -0.0 is
                    ("b > 4611686018427387904.0f", "b"),         # long -> float
                    ("a / 0 == 0 or a > 5", "a")]                # a null term


@pytest.mark.parametrize("path", ["closed_form", "fast_partition", "vm_partition"])
@pytest.mark.parametrize("pred,x", KEYED_PREDICATES, ids=[p for p, _ in KEYED_PREDICATES])
def test_keyed_pattern_paths(pred, x, path):
    """closed_form: f / g term lists on own columns, plain-copy items,
    ts_order=1 (engine.cpp, "closed-form fast path").
    fast_partition: a computed select item makes the walk a VM walk, which
    the closed form refuses (`!rt.walk_vm`); f and g are still term lists, so
    the partition pass is the prefetching one (`!rt.part_vm`: rt.pref).
    vm_partition: g = not (not (p)) does not lower (`rt.part_vm`)."""
    ts, cols, st = keyed_data(N_C)
    full = pattern_plan(pred, pred, x, True)
    want_full = oracle_cached(full, N_C, lambda: events_of("AB", ts, cols, st)).get("O", [])
    _nonvacuous(len(want_full), int((st == 1).sum()), path + " " + pred)
    if path == "fast_partition":
        plan, want, opts = full, want_full, {}
    else:
        g = pred if path == "closed_form" else "not (not (%s))" % pred
        plan = pattern_plan(pred, g, x, False)
        want = [(t, s, d[:3]) for t, s, d in want_full]
        opts = {"ts_order": 1} if path == "closed_form" else {}
    got, stats = run_app(plan, "AB", ts, cols, st, ["O"], **opts)
    if path == "closed_form":
        assert stats.kernel_launches[L.K_CF_PARTITION] > 0
    else:
        assert stats.kernel_launches[L.K_PARTITION] > 0 and stats.kernel_launches[L.K_CF_PARTITION] == 0
    X.same_rows_bits(got["O"], want, out_types(plan, "O"), path + " " + pred)


def test_walk_condition_and_items_over_captures():
    """OP_LDCAP: a captured int (negative, INT_MIN) sign-extends, a captured
    float word (NaN, -0.0) compares as a float; s1.a / s2.a is null when s2.a
    is 0."""
    n = 2 * 2048 + 77
    ts, cols, st = keyed_data(n)
    plan = AB_DEF + ("partition with (k of A, k of B) begin "
                     "from every s1=A[a < 0] -> s2=B[c < s1.c and a == s1.a % -7] within 10 sec "
                     "select s1.a as a1, s1.c as c1, s2.a as a2, s1.a / s2.a as q, s2.c - s1.c as dc "
                     "insert into O; end;")
    want = oracle_cached(plan, n, lambda: events_of("AB", ts, cols, st)).get("O", [])
    _nonvacuous(len(want), int((st == 1).sum()), "walk over captures")
    assert sum(1 for _, _, d in want if d[3] is None) >= 4 and sum(1 for _, _, d in want if d[3]) >= 4
    assert any(d[0] == X.INT_MIN for _, _, d in want)
    got, stats = run_app(plan, "AB", ts, cols, st, ["O"])
    assert stats.kernel_launches[L.K_PARTITION] > 0
    X.same_rows_bits(got["O"], want, out_types(plan, "O"), "walk over captures")


# ---------------------------------------------------------------- group D --
ABC_DEF = "".join("define stream %s (k int, a int, c float, d double);" % s for s in "ABC")
N_D = 16384 + 77          # k_mqpart's 16384-row tile and a ragged tail
MQ_SEQ = [("a % -7 <= -1", "c <= 0.0", "a % -7 != -1"),      # negative modulus; float column, double constant
          ("a % -7 != -1", "c > 1.0000001", "a % -7 <= -1")]
MQ_AGG = [("A", "", "count() as n", "n != 3"),
          ("B", "", "count() as n", "n > 2.5"),
          ("C", "", "count() as n", "n > 2.5f"),            # a float constant: the generic unit
          ("A", "[c <= 0.0]", "sum(a) as s", "s <= -1"),     # int argument, long sum, negative sums
          ("B", "", "sum(d) as t", "t != 0.0"),              # through 0.0 and +-inf
          ("C", "", "count() as n", "5 >= k")]               # operands flipped


def mq_plan():
    seq = ["partition with (k of A, k of B, k of C) begin "]
    for q, (f1, f2, f3) in enumerate(MQ_SEQ):
        seq.append("from every s1=A[%s], s2=B[%s]+, s3=C[%s] within 10 sec select s1.k as k, s1.a as a1, "
                   "s2[last].c as c2, s3.d as d3 insert into Seq%d;" % (f1, f2, f3, q))
    seq.append(" end;")
    agg = ["from %s%s select k, %s group by k having %s insert into Agg%d;" % (s, f, item, hav, q)
           for q, (s, f, item, hav) in enumerate(MQ_AGG)]
    return ABC_DEF + "".join(seq) + "".join(agg)


def mq_data():
    ts, cols, st = keyed_data(N_D, nstreams=3, seed=4)
    rng = np.random.default_rng(9)
    # no NaN in an aggregate argument; sums return to 0.0 often and overflow
    # to +-inf in some keys
    vals = np.array([1.5, -1.5, 0.0, -0.0, 1.5, -1.5, 0.1 + 0.2, -(0.1 + 0.2), X.DBL_MAX, -X.DBL_MAX, 2.0 ** -1074])
    d = vals[rng.integers(0, len(vals), N_D)]
    d[rng.integers(0, N_D, 6)] = np.inf
    d[rng.integers(0, N_D, 6)] = -np.inf
    return ts, [cols[0], cols[1], cols[3], d], st


def test_multi_query_group():
    ts, cols, st = mq_data()
    plan = mq_plan()
    outs = ["Seq%d" % q for q in range(len(MQ_SEQ))] + ["Agg%d" % q for q in range(len(MQ_AGG))]
    want = oracle_cached(plan, "mq", lambda: events_of("ABC", ts, cols, st))
    per_stream = {s: int((st == i).sum()) for i, s in enumerate("ABC")}
    for q in range(len(MQ_SEQ)):
        _nonvacuous(len(want.get("Seq%d" % q, [])), per_stream["C"], "Seq%d" % q)
    for q, (s, _, _, _) in enumerate(MQ_AGG):
        _nonvacuous(len(want.get("Agg%d" % q, [])), per_stream[s], "Agg%d" % q)
    t = [d[1] for _, _, d in want["Agg4"]]
    assert any(v == np.inf for v in t) and any(v == -np.inf for v in t)
    assert any(d[1] < -1 for _, _, d in want["Agg3"])
    got, stats = run_app(plan, "ABC", ts, cols, st, outs)
    assert stats.kernel_launches[L.K_MQ_PARTITION] > 0
    for o in outs:
        X.same_rows_bits(got[o], want.get(o, []), out_types(plan, o), o)


# ---------------------------------------------------------------- group E --
N_E = 4096 + 77
M_COMPUTED = ("from S[a / 0 == 0 or a % -7 != -3] select a, b, c, d, a % -7 as r, c * 2.5f as y, b / a as q "
              "insert into M;", "from M[r == -1 or q > 0] select * insert into O;")
M_COPIES = ("from S[b * 1.0f > 4611686018427387904.0f or c <= 0.0f] select a, b, c, d insert into M;",
            "from M[a % -7 == -1 or b > 4611686018427387904.0f] select * insert into O;")


def chain_expected(producer, reader, cols, ts):
    """M = the producer's rows with a null written as 0 (the engine's columns
    hold no null); O = the reader over those columns."""
    idx, outs, nulls, mt = X.filter_project(S_DEF + producer, cols)
    m_cols = [np.where(nm, o.dtype.type(0), o) for o, nm in zip(outs, nulls)]
    m_def = "define stream M (%s);" % ", ".join(
        "%s %s" % (a.name, a.type) for a in O.parse_app(S_DEF + producer).out_streams["M"].attrs)
    j, o2, n2, ot = X.filter_project(m_def + reader, m_cols)
    return (X.rows_of(ts[idx], idx, outs, nulls), mt), (X.rows_of(ts[idx][j], idx[j], o2, n2), ot), len(idx)


@pytest.mark.parametrize("how", ["host", "odd_device_slices"])
@pytest.mark.parametrize("chain", [M_COMPUTED, M_COPIES], ids=["computed", "copies"])
def test_derived_stream(chain, how):
    """host: an aligned slice, k_derive_vec (computed items: the interpreter
    over prefetched registers; copies: eval_terms_regs only).
    odd_device_slices: slices of one device allocation that start at odd rows
    are not aligned for the vector accesses (build_view: `da.vec`): k_derive
    row by row, terms_row and the per-row interpreter."""
    producer, reader = chain
    plan = S_DEF + producer + reader
    ids = {nm: i for i, nm in enumerate(NAMES)}
    cols = s_columns(N_E, ids, 5)
    ts = np.arange(N_E, dtype=np.int64) * 2 + 1
    (want_m, mt), (want_o, ot), nm = chain_expected(producer, reader, cols, ts)
    _nonvacuous(nm, N_E, "producer " + producer)
    _nonvacuous(len(want_o), nm, "reader " + reader)
    if chain is M_COMPUTED:
        assert sum(1 for _, _, d in want_m if d[6] is None) >= 16       # b / 0
    cuts = None if how == "host" else [0, 1, 2050, 2051, N_E]
    got, stats = run_app(plan, ["S"], ts, cols, None, ["M", "O"], cuts=cuts, device=how != "host")
    assert stats.kernel_launches[L.K_OTHER] > 0          # k_derive
    X.same_rows_bits(got["M"], want_m, mt, "M " + how, inputs=_input_row(cols))
    X.same_rows_bits(got["O"], want_o, ot, "O " + how, inputs=_input_row(cols))
