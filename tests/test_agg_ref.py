"""agg_ref (fixed-width numpy scalars) against the Python oracle (cumulative
aggregates) and the window model (sliding windows) on the edge-value stream
of agg_ref.edge_stream, bit for bit: function x argument type.  The three
are written independently, so a wrong wrap, widening, tie rule or removal
order in one of them shows here, without a device."""
import numpy as np
import pytest

import agg_ref as R
import expr_ref as X
import siddhi_oracle as O
from helpers import oracle_run
from window_model import model_run

FNS = ("sum", "avg", "min", "max", "count")
TYPES = (O.INT, O.LONG, O.FLOAT, O.DOUBLE)
# the argument of each type; min / max take the columns without NaN
ARG = {fn: dict(zip(TYPES, "abcd")) for fn in ("sum", "avg", "count")}
ARG.update({fn: dict(zip(TYPES, ("a", "b", "c2", "d2"))) for fn in ("min", "max")})
TIME_T = 300
MODES = {
    "cumulative": "from S select k, %s group by k insert into O;",
    "length": "partition with (k of S) begin from S#window.length(5) select k, %s insert into O; end;",
    "time": "partition with (k of S) begin from S#window.time(%d) select k, %%s insert into O; end;" % TIME_T,
    # Siddhi's one window for all groups: rows of other groups push a group's rows out
    "global_time": "from S#window.time(20) select k, %s group by k insert into O;",
}
_WANT = {}


def _call(fn, t):
    return "count()" if fn == "count" else "%s(%s)" % (fn, ARG[fn][t])


def expected(fn, mode):
    """The oracle's / the model's rows of the four argument types at once."""
    if (fn, mode) not in _WANT:
        ts, cols = R.edge_stream()
        plan = R.stream_def() + MODES[mode] % ", ".join("%s as v%d" % (_call(fn, t), i) for i, t in enumerate(TYPES))
        ev = R.events(ts, cols)
        _WANT[(fn, mode)] = (oracle_run(plan, ev) if mode == "cumulative" else model_run(plan, ev)[0])["O"]
    return _WANT[(fn, mode)]


def out_type(fn, t):
    if fn == "count":
        return O.LONG
    if fn == "avg":
        return O.DOUBLE
    if fn == "sum":
        return O.LONG if t in (O.INT, O.LONG) else O.DOUBLE
    return t


@pytest.mark.parametrize("t", TYPES)
@pytest.mark.parametrize("fn", FNS)
def test_reference_agrees(fn, t):
    ts, cols = R.edge_stream()
    k = cols[0]
    spec = [(fn, None, None) if fn == "count" else (fn, t, R.COL[ARG[fn][t]])]
    i = TYPES.index(t)
    types = [O.INT, out_type(fn, t)]
    for mode in MODES:
        if mode == "cumulative":
            vals = R.cumulative(spec, k, cols)
        elif mode == "length":
            vals, _, _ = R.windowed(spec, k, cols, ts, "length", 5, inst=k)
        elif mode == "time":
            vals, live, _ = R.windowed(spec, k, cols, ts, "time", TIME_T, inst=k)
            assert 4 <= live <= 16
        else:
            vals, _, _ = R.windowed(spec, k, cols, ts, "time", 20)
        want = [(tt, s, (d[0], d[1 + i])) for tt, s, d in expected(fn, mode)]
        X.same_rows_bits(R.rows_of(ts, k, vals), want, types, "%s(%s) %s" % (fn, t, mode))


def test_edge_stream_reaches_the_edges():
    """What the device tests rely on, on the reference alone: wrapped long
    sums, int sums beyond 32 bits and negative, double sums finite, infinite
    and NaN, both zeros as a float minimum."""
    ts, cols = R.edge_stream()
    k = cols[0]
    n = len(ts)
    spec = [("sum", O.LONG, R.COL["b"]), ("sum", O.INT, R.COL["a"]), ("sum", O.DOUBLE, R.COL["d"]),
            ("sum", O.FLOAT, R.COL["c"]), ("min", O.FLOAT, R.COL["c2"])]
    vals = R.cumulative(spec, k, cols)
    exact = {}
    wrapped = 0
    for r in range(n):
        exact[k[r]] = exact.get(k[r], 0) + int(cols[R.COL["b"]][r])
        wrapped += vals[r][0] != exact[k[r]]
    assert wrapped >= 256
    sa = [v[1] for v in vals]
    assert sum(1 for v in sa if not X.INT_MIN <= v <= X.INT_MAX) >= 256 and sum(1 for v in sa if v < 0) >= 256
    sd = np.array([v[2] for v in vals])
    assert (np.isfinite(sd) & (sd != 0)).sum() >= n // 2
    assert np.isinf(sd).sum() >= 16 and np.isnan(sd).sum() >= 16
    sc = np.array([v[3] for v in vals])
    with np.errstate(all="ignore"):
        assert (np.isfinite(sc) & (sc.astype(np.float32).astype(np.float64) != sc)).sum() >= 16
    mc = np.array([v[4] for v in vals])
    assert ((mc == 0) & np.signbit(mc)).sum() >= 16 and ((mc == 0) & ~np.signbit(mc)).sum() >= 16
    # finite arithmetic outside the keys k % 8 == 0
    for c in ("c", "d"):
        v = cols[R.COL[c]]
        assert not R._wild(v[k % 8 != 0]).any() and np.isnan(v).sum() >= 16
    assert not np.isnan(cols[R.COL["c2"]]).any() and not np.isnan(cols[R.COL["d2"]]).any()


def test_fixed_width_rules():
    """The reference's own arithmetic on hand-made rows."""
    g = np.zeros(4, np.int32)
    b = np.array([X.LONG_MAX, 1, X.LONG_MIN, -1], np.int64)
    assert [v[0] for v in R.cumulative([("sum", O.LONG, 0)], g, [b])] == [X.LONG_MAX, X.LONG_MIN, 0, -1]
    a = np.array([X.INT_MIN, X.INT_MIN, -1, 7], np.int32)
    assert [v[0] for v in R.cumulative([("sum", O.INT, 0)], g, [a])] == [-(1 << 31), -(1 << 32), -(1 << 32) - 1,
                                                                         -(1 << 32) + 6]
    c = np.array([0.0, -0.0, 0.0, -0.0], np.float32)
    mn = [v[0] for v in R.cumulative([("min", O.FLOAT, 0)], g, [c])]
    assert [np.signbit(v) for v in mn] == [False] * 4          # the earlier row stays
    w, live, twins = R.windowed([("min", O.FLOAT, 0)], g, [c], np.arange(4), "length", 2)
    assert [np.signbit(v[0]) for v in w] == [False, False, True, False] and live == 2 and twins == 2
    big = np.array([(1 << 53) + 1, 1], np.int64)
    assert [v[0] for v in R.cumulative([("avg", O.LONG, 0)], g[:2], [big])] == [2.0 ** 53, (2.0 ** 53 + 1.0) / 2.0]
    f = np.array([16777216.0, 1.0, 1.0], np.float32)
    assert [v[0] for v in R.cumulative([("sum", O.FLOAT, 0)], g[:3], [f])][-1] == 16777218.0   # not summed in float
    d = np.array([np.inf, 1.0, 2.0], np.float64)
    w, _, _ = R.windowed([("sum", O.DOUBLE, 0)], g[:3], [d], np.arange(3), "length", 1)
    assert w[0][0] == np.inf and np.isnan(w[1][0]) and np.isnan(w[2][0])      # inf - inf stays
