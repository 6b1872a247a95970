"""expr_ref (vectorised numpy, tests/expr_ref.py) against siddhi_oracle.evaluate
(row-at-a-time pure Python): every operator over every ordered pair of operand
types, on all pairs of the edge values of expr_ref.EDGES.  The two evaluators
share the oracle's parser and binder and nothing else, so a disagreement is a
value-semantics mistake in one of them; which one is decided from the Java
rules (JLS 5.1.2, 15.17, 15.20, 15.21)."""
import math
import struct

import numpy as np
import pytest

import expr_ref as X
import siddhi_oracle as O

NUM = [O.INT, O.LONG, O.FLOAT, O.DOUBLE]
ARITH = ["+", "-", "*", "/", "%"]
CMP = ["==", "!=", "<", "<=", ">", ">="]


def _grid(ta, tb):
    a, b = X.EDGES[ta], X.EDGES[tb]
    x = np.repeat(a, len(b))
    y = np.tile(b, len(a))
    return x, y


def _py(v, t):
    if t in (O.INT, O.LONG):
        return int(v)
    if t == O.BOOL:
        return bool(v)
    return float(v)


def _bits(v, t):
    if v is None:
        return None
    if t in (O.FLOAT, O.DOUBLE):
        f = float(v)
        if f != f:
            return "NaN"
        return struct.pack("<f" if t == O.FLOAT else "<d", f)
    return v


def _check(expr_text, types, cols, select=False):
    """Evaluate `expr_text` over stream S(x, y) both ways; compare every row."""
    sdef = "define stream S (%s);" % ", ".join("%s %s" % (nm, t) for nm, t in zip("xy", types))
    if select:
        plan = sdef + "from S select %s as r insert into O;" % expr_text
        e = O.parse_app(plan).queries[0].select[0].expr
    else:
        plan = sdef + "from S[%s] select x insert into O;" % expr_text
        e = O.parse_app(plan).queries[0].filters[0]
    n = len(cols[0])
    val, null = X.evaluate(e, lambda slot: cols[slot[1]], n)
    rows = [tuple(_py(c[i], t) for c, t in zip(cols, types)) for i in range(n)]
    bad = []
    for i, row in enumerate(rows):
        want = O.evaluate(e, lambda slot: row[slot[1]])
        got = None if null[i] else val[i].item()
        if _bits(got, e.t) != _bits(want, e.t):
            bad.append((row, got, want))
    assert not bad, "%s over (%s): %d of %d rows differ; first (inputs, expr_ref, oracle): %r" % (
        expr_text, ", ".join(types), len(bad), n, bad[:3])
    return val, null


@pytest.mark.parametrize("tb", NUM)
@pytest.mark.parametrize("ta", NUM)
@pytest.mark.parametrize("op", ARITH)
def test_arithmetic(op, ta, tb):
    x, y = _grid(ta, tb)
    val, null = _check("x %s y" % op, (ta, tb), (x, y), select=True)
    ints = ta in (O.INT, O.LONG) and tb in (O.INT, O.LONG)
    # null exactly at an integer division / remainder by zero
    assert np.array_equal(null, (y == 0) if ints and op in "/%" else np.zeros(len(x), bool))


@pytest.mark.parametrize("tb", NUM)
@pytest.mark.parametrize("ta", NUM)
@pytest.mark.parametrize("op", CMP)
def test_comparison(op, ta, tb):
    x, y = _grid(ta, tb)
    val, _ = _check("x %s y" % op, (ta, tb), (x, y))
    assert val.any() and not val.all()


@pytest.mark.parametrize("tb", NUM)
@pytest.mark.parametrize("ta", NUM)
def test_comparison_of_null_is_false(ta, tb):
    # x / 0 is null for int / long (App. A.2), +-inf / NaN for float / double
    x, y = _grid(ta, tb)
    for op in CMP:
        val, _ = _check("x / 0 %s y" % op, (ta, tb), (x, y))
        if ta in (O.INT, O.LONG):
            assert not val.any()
        _check("not (x %% 0 %s y)" % op, (ta, tb), (x, y))


@pytest.mark.parametrize("t", NUM)
def test_negation(t):
    x = X.EDGES[t]
    _check("-x", (t, t), (x, x), select=True)
    _check("-(x * 0)", (t, t), (x, x), select=True)       # sign of a zero result
    _check("0 - x == -x", (t, t), (x, x))


def test_logic():
    x, y = _grid(O.BOOL, O.BOOL)
    for e in ("x and y", "x or y", "not x", "not (x and not y) or y", "x == y", "x != y",
              "x == true", "false != y"):
        _check(e, (O.BOOL, O.BOOL), (x, y))
    # null terms: a comparison of null is false, so `and` / `or` / `not` see false
    x, y = _grid(O.INT, O.INT)
    for e in ("x / y == 0 or x > 5", "x % y == 0 and x > 5", "not (x / y == x / y)",
              "not (x % y < 1) and not (y / x > 0)"):
        _check(e, (O.INT, O.INT), (x, y))


def test_long_to_float_rounds_once():
    """(float) long rounds once (JLS 5.1.2); through binary64 it rounds twice
    and 2^62 + 2^38 + 1 lands on 2^62 instead of the float above it."""
    v = (1 << 62) + (1 << 38) + 1
    up = float(np.nextafter(np.float32(2.0 ** 62), np.float32(np.inf)))
    assert float(np.int64(v).astype(np.float32)) == up
    assert O._convert(v, O.LONG, O.FLOAT) == up
    assert O._convert(-v, O.LONG, O.FLOAT) == -up
    # ties to even, and a carry into the next binade
    assert O._convert((1 << 24) + 1, O.LONG, O.FLOAT) == 2.0 ** 24
    assert O._convert((1 << 24) + 3, O.LONG, O.FLOAT) == 2.0 ** 24 + 4
    assert O._convert((1 << 63) - 1, O.LONG, O.FLOAT) == 2.0 ** 63
    rng = np.random.default_rng(5)
    for x in rng.integers(-(1 << 63), (1 << 63) - 1, 2000, dtype=np.int64, endpoint=True):
        assert O._convert(int(x), O.LONG, O.FLOAT) == float(x.astype(np.float32))


def test_select_list_past_the_kernels_column_limit_is_refused():
    """The kernels' output descriptors hold 16 columns.  A 21-item select list
    (the first form of test_gpu_expr_edges.test_projection_signs_and_nulls)
    was accepted, overran them and delivered unrelated values."""
    import flink_siddhi as fs
    sdef = "define stream S (a int);"
    items = lambda n: ", ".join("a + %d as x%d" % (i, i) for i in range(n))  # noqa: E731
    fs.validate(sdef + "from S select %s insert into O;" % items(16))
    for tail in ("insert into O;", "insert into M; from M[x0 > 1] select x0 insert into O;"):
        with pytest.raises(fs.UnsupportedPlanException, match="more than 16 attributes"):
            fs.validate(sdef + "from S select %s %s" % (items(17), tail))


def test_same_rows_bits():
    T = [O.INT, O.FLOAT, O.DOUBLE, O.BOOL]
    a = [(1, 0, (3, 0.5, -0.0, True)), (2, 1, (4, math.nan, 1.0, False))]
    X.same_rows_bits(a, a, T)
    # any NaN equals any NaN; a reference null is the engine's 0
    X.same_rows_bits([(2, 1, (0, -math.nan, 0.0, 0))], [(2, 1, (None, math.nan, None, False))], T)
    # float narrows to binary32 before the bits are compared
    X.same_rows_bits([(0, 0, (0, 0.1, 0.0, 0))], [(0, 0, (0, float(np.float32(0.1)), 0.0, 0))], T)
    for bad in ((1, 0, (3, 0.5, 0.0, True)),        # -0.0 vs 0.0 (double)
                (1, 0, (3, -0.5, -0.0, True)),
                (1, 0, (3, 0.5, -0.0, False)),
                (1, 1, (3, 0.5, -0.0, True))):
        with pytest.raises(AssertionError, match="first difference at row 0"):
            X.same_rows_bits([bad], a[:1], T)
    with pytest.raises(AssertionError, match="-0.0"):
        X.same_rows_bits([(1, 0, (3, -0.0, -0.0, True))], [(1, 0, (3, 0.0, -0.0, True))], T)
    with pytest.raises(AssertionError, match="engine 1 rows, reference 2 rows"):
        X.same_rows_bits(a[:1], a, T)
    with pytest.raises(AssertionError, match=r"input row 1: \('in', 1\)"):
        X.same_rows_bits(a[:1], a, T, inputs=lambda s: ("in", s))
