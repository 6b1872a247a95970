"""Column-wise numpy reference for the SiddhiQL expression subset, and a
bit-exact row comparison.

Independent of `siddhi_oracle.evaluate` (the row-at-a-time pure-Python
evaluator): the oracle's parser and binder supply the typed expression tree,
the evaluation here is vectorised numpy in the operand types themselves
(np.int32 / np.int64 with explicit wrap, np.float32 / np.float64), so a
mistake in either evaluator's value semantics shows as a disagreement
(tests/test_expr_ref.py).  Java rules: JLS 5.1.2 (widening conversions round
once), 15.17 (integer division truncates, % takes the dividend's sign, float
% is fmod), 15.20 / 15.21 (NaN compares false, != true; -0.0 == 0.0);
Siddhi: int / long division or remainder by zero is null, a comparison with a
null operand is false.
"""
from __future__ import annotations

import struct
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np

import siddhi_oracle as O

DTYPE = {O.INT: np.int32, O.LONG: np.int64, O.FLOAT: np.float32, O.DOUBLE: np.float64,
         O.BOOL: np.bool_, O.STRING: np.int32}

INT_MIN, INT_MAX = -(1 << 31), (1 << 31) - 1
LONG_MIN, LONG_MAX = -(1 << 63), (1 << 63) - 1
FLT_MIN, FLT_MAX = float(np.finfo(np.float32).tiny), float(np.finfo(np.float32).max)
DBL_MIN, DBL_MAX = float(np.finfo(np.float64).tiny), float(np.finfo(np.float64).max)


def _pm(vals):
    out = []
    for v in vals:
        out += [v, -v]
    return out


# every value is exactly representable in its type
EDGES = {
    O.INT: np.array([0] + _pm([1, 2, 7]) + [INT_MAX, INT_MAX - 1, INT_MIN, INT_MIN + 1]
                    + _pm([46341, (1 << 24) + 1, 65536, 65537]), np.int32),
    O.LONG: np.array([0] + _pm([1, 1 << 31, (1 << 32) + 1, (1 << 24) + 1, (1 << 53) + 1,
                                (1 << 62) + (1 << 38) + 1])
                     + [LONG_MAX, LONG_MIN, LONG_MIN + 1], np.int64),
    O.FLOAT: np.array(_pm([0.0, 1.0]) + [float(np.nextafter(np.float32(1), np.float32(2))), 0.375]
                      + _pm([2.0 ** -149, FLT_MIN, FLT_MAX, float("inf")])
                      + [float("nan"), 2.0 ** 24, 2.0 ** 62], np.float32),
    O.DOUBLE: np.array(_pm([0.0, 1.0]) + [1.5, 0.1 + 0.2]
                       + _pm([2.0 ** -1074, DBL_MIN, DBL_MAX, float("inf")])
                       + [float("nan"), 2.0 ** 53, float(np.float32(0.1))], np.float64),
    O.BOOL: np.array([0, 1], np.uint8),
}


# -------------------------------------------------------------- evaluation --
def _convert(v: np.ndarray, frm: str, to: str) -> np.ndarray:
    """A single numpy cast (one rounding: JLS 5.1.2)."""
    return v if frm == to else v.astype(DTYPE[to])


def _int_divmod(a: np.ndarray, b: np.ndarray, op: str):
    """Truncating division / dividend-signed remainder in a's own integer
    type; x / -1 and x % -1 wrap; a zero divisor is null."""
    dt = a.dtype.type
    null = b == 0
    m1 = b == -1
    safe = np.where(null | m1, dt(1), b)
    q = a // safe                                       # floor
    r = a - q * safe
    q = q + ((r != 0) & ((a < 0) != (safe < 0))).astype(dt)   # -> truncation
    q = np.where(m1, dt(0) - a, q)                      # MIN / -1 wraps to MIN
    if op == "/":
        out = q
    else:
        out = np.where(m1, dt(0), a - q * safe)
    return np.where(null, dt(0), out).astype(dt), null


def evaluate(e: O.Expr, env: Callable[[object], np.ndarray], n: int,
             strings: Optional[Dict[str, int]] = None) -> Tuple[np.ndarray, np.ndarray]:
    """(values, null mask) of the bound expression `e` over n rows;
    env(slot) -> the typed column.  `strings` maps string constants to the
    ids the string columns hold."""
    with np.errstate(all="ignore"):
        return _ev(e, env, n, strings or {})


def _ev(e, env, n, strings):
    no = np.zeros(n, bool)
    k = e.kind
    if k == "const":
        if e.vtype == O.STRING:
            return np.full(n, strings[e.value], np.int32), no
        return np.full(n, e.value, DTYPE[e.vtype]), no
    if k == "attr":
        col = np.asarray(env(e.slot))
        if e.t == O.BOOL:
            col = col != 0
        assert col.dtype == DTYPE[e.t], (e.name, col.dtype, e.t)
        return col, no
    if k == "not":
        v, vn = _ev(e.args[0], env, n, strings)
        return ~(v & ~vn), no
    if k == "neg":
        v, vn = _ev(e.args[0], env, n, strings)
        if e.t in (O.INT, O.LONG):
            return (v.dtype.type(0) - v), vn
        return -v, vn
    assert k == "bin", k
    op = e.op
    a, an = _ev(e.args[0], env, n, strings)
    b, bn = _ev(e.args[1], env, n, strings)
    ta, tb = e.args[0].t, e.args[1].t
    if op == "and":
        return (a & ~an) & (b & ~bn), no
    if op == "or":
        return (a & ~an) | (b & ~bn), no
    if op in ("==", "!=", "<", "<=", ">", ">="):
        if ta in O.NUMERIC_RANK and tb in O.NUMERIC_RANK:
            ct = ta if O.NUMERIC_RANK[ta] >= O.NUMERIC_RANK[tb] else tb
            a, b = _convert(a, ta, ct), _convert(b, tb, ct)
        r = {"==": np.equal, "!=": np.not_equal, "<": np.less, "<=": np.less_equal,
             ">": np.greater, ">=": np.greater_equal}[op](a, b)
        return r & ~(an | bn), no
    t = e.t
    a, b = _convert(a, ta, t), _convert(b, tb, t)
    null = an | bn
    if t in (O.INT, O.LONG):
        if op == "+":
            r = a + b
        elif op == "-":
            r = a - b
        elif op == "*":
            r = a * b
        else:
            r, z = _int_divmod(a, b, op)
            null = null | z
    else:
        r = {"+": np.add, "-": np.subtract, "*": np.multiply, "/": np.divide,
             "%": np.fmod}[op](a, b)
    assert r.dtype == DTYPE[t], (op, r.dtype, t)
    return r, null


# ------------------------------------------------ plans over typed columns --
def bound_query(plan: str, qi: int = 0) -> Tuple[O.App, O.Query]:
    app = O.parse_app(plan)
    return app, app.queries[qi]


def filter_project(plan: str, cols: Sequence[np.ndarray], strings=None, qi: int = 0):
    """A single-stream `from S[f] select items` query over typed columns:
    (selected row indices, [output columns at those rows], [null masks],
    [output types])."""
    app, q = bound_query(plan, qi)
    assert q.kind == "single" and q.having is None and not q.group_by
    n = len(cols[0])
    env = lambda slot: cols[slot[1]]  # noqa: E731
    sel = np.ones(n, bool)
    for f in q.filters:
        v, vn = evaluate(f, env, n, strings)
        sel &= v & ~vn
    idx = np.nonzero(sel)[0]
    outs, nulls, types = [], [], []
    for it in q.select:
        v, vn = evaluate(it.expr, env, n, strings)
        if it.expr.t == O.BOOL:
            v = v.astype(np.uint8)
        outs.append(v[idx])
        nulls.append(vn[idx])
        types.append(it.expr.t)
    return idx, outs, nulls, types


def rows_of(ts, seq, outs, nulls) -> List[Tuple[int, int, tuple]]:
    """[(ts, seq, data)] with Python scalars; a null is None."""
    cs = [[None if m else v for v, m in zip(o.tolist(), nm.tolist())] for o, nm in zip(outs, nulls)]
    ts, seq = np.asarray(ts).tolist(), np.asarray(seq).tolist()
    return [(ts[i], seq[i], tuple(c[i] for c in cs)) for i in range(len(ts))]


# ------------------------------------------------------- bit-exact compare --
_NAN = "NaN"


def value_key(v, t: str):
    """The comparison key of one value of declared type t: float / double by
    bit pattern after narrowing to t (-0.0 != 0.0), any NaN equal to any NaN
    (sign and payload of a generated NaN differ between processors), null as
    the engine's stand-in 0, everything else by value."""
    if v is None:
        v = 0
    if t == O.FLOAT:
        f = np.float32(v)
        return _NAN if f != f else struct.pack("<f", f)
    if t == O.DOUBLE:
        f = float(v)
        return _NAN if f != f else struct.pack("<d", f)
    if t == O.BOOL:
        return int(bool(v))
    return v


def same_rows_bits(got, want, types: Sequence[str], ctx: str = "", inputs=None):
    """got / want: [(ts, seq, data)].  Raises on the first differing row,
    naming it and (with `inputs`: seq -> input row) the input values."""
    def key(row):
        t, s, d = row
        assert len(d) == len(types), (len(d), len(types))
        return (t, s, tuple(value_key(v, ty) for v, ty in zip(d, types)))

    for i in range(min(len(got), len(want))):
        if key(got[i]) != key(want[i]):
            src = ""
            if inputs is not None:
                src = " input row %d: %r" % (want[i][1], inputs(want[i][1]))
            raise AssertionError("%s: first difference at row %d: engine %r reference %r%s "
                                 "(engine %d rows, reference %d rows)"
                                 % (ctx, i, got[i], want[i], src, len(got), len(want)))
    if len(got) != len(want):
        i = min(len(got), len(want))
        extra = (got if len(got) > len(want) else want)[i]
        src = ""
        if inputs is not None:
            src = " input row %d: %r" % (extra[1], inputs(extra[1]))
        raise AssertionError("%s: engine %d rows, reference %d rows; first unmatched %r%s"
                             % (ctx, len(got), len(want), extra, src))
