"""Edge-value parity of the four hand-written copies of the aggregate
arithmetic: the stand-alone walk (agg_update / AggEnv::agg / agg_key), the
multi-query group's mq_agg_fast and mq_agg_unit, and the sliding windows
(win_key), on the stream of agg_ref.edge_stream: int and long sums that wrap
and leave 32 bits, float arguments summed in double, double sums through
+-inf into NaN, min / max over INT_MIN, LONG_MIN, 2^53 / 2^53 + 1, denormals
and -0.0 / 0.0, groups that start above (min) or below (max) zero.

Expected rows: the Python oracle (cumulative) and the window model
(windows), both checked against agg_ref on this very stream by
tests/test_agg_ref.py; compared with expr_ref.same_rows_bits.  No tolerance:
the device adds in the reference's order.  Every number below is a condition
on the reference (`conditions`), asserted before the engine is started.

NaN under min / max is left out on purpose (the min / max arguments are c2 /
d2: c / d with NaN replaced by -0.0).  Siddhi's ordering of NaN cannot be
established here, and the naive model and the device legitimately differ:
after the window [1, NaN, 0] loses the 1 the model's min() gives NaN, the
ring's recomputation gives 0.  NaN under sum / avg is in.

Every case is cut into the batches CUTS, so accumulators travel through
per-key state, and runs with chunk_events = 2048 where a chunk can be that
small (a multi-query group's chunk is at least its 16384-row tile), so they
also cross chunks inside a batch.  Which kernel instance runs shows in
stats() as one launch counter per family only, so each case is built from
the engine's own selection rule, cited at the case.
"""
import numpy as np
import pytest

import agg_ref as R
import expr_ref as X
import flink_siddhi as fs
import siddhi_oracle as O
from flink_siddhi import _lib as L
from chain_model import chain_run
from helpers import engine_rows, oracle_run
from window_model import model_run, strip_windows

pytestmark = pytest.mark.gpu

SEED = 7
N = R.N_ROWS
CUTS = [0, 1, 2050, 4099, N]
CHUNK = 2048
_REF = {}


def data():
    return R.edge_stream(SEED)


def reference(body, windows=False):
    """{out: rows} of the oracle / (rows, largest occupancy) of the model,
    once per plan."""
    if body not in _REF:
        ts, cols = data()
        run = model_run if windows else oracle_run
        _REF[body] = run(R.stream_def() + body, R.events(ts, cols))
    return _REF[body]


def _count(xs, pred):
    return sum(1 for x in xs if pred(x))


def conditions(body, want, skip=()):
    """Non-vacuity of one case, on the reference alone.  `skip` names the
    conditions a case cannot meet by arithmetic (said at the case)."""
    ts, cols = data()
    plan = R.stream_def() + body
    stripped, wspecs = strip_windows(plan)
    app = O.parse_app(stripped)
    zneg = zpos = 0
    zeros = False
    live = twins = 0
    for qi, q in enumerate(app.queries):
        names, vals, group, lv, tw = R.query_values(app, wspecs, qi, ts, cols)
        live, twins = max(live, lv), twins + tw
        rows = [r for r, v in enumerate(vals) if v is not None]
        ctx = "query %d of %s" % (qi, body)
        if q.having is not None:
            npass = len(want.get(q.out, []))
            assert npass >= 16 and len(rows) - npass >= 16, "%s: having passes %d of %d" % (ctx, npass, len(rows))
        first = {}
        for r in rows:
            first.setdefault(group[r], r)
        for j, (fn, col) in enumerate(names):
            x = [vals[r][j] for r in rows]
            if fn == "sum" and col == "b" and "wrap" not in skip:
                exact = [vals[r][names.index(("xsum", "b"))] for r in rows]
                assert _count(zip(x, exact), lambda p: p[0] != p[1]) >= 256, ctx
            if fn == "sum" and col == "a":
                if "int32" not in skip:
                    assert _count(x, lambda v: not X.INT_MIN <= v <= X.INT_MAX) >= 256, ctx
                assert _count(x, lambda v: v < 0) >= 256, ctx
            if fn == "sum" and col == "c" and "float32" not in skip:
                with np.errstate(all="ignore"):
                    xa = np.array(x)
                    assert (np.isfinite(xa) & (xa.astype(np.float32).astype(np.float64) != xa)).sum() >= 16, ctx
            if fn == "sum" and col == "d":
                xa = np.array(x)
                assert (np.isfinite(xa) & (xa != 0)).sum() * 2 >= len(rows), ctx
                assert np.isinf(xa).sum() >= (0 if "inf" in skip else 16) and np.isnan(xa).sum() >= 16, ctx
            if fn in ("min", "max") and col in ("c2", "d2"):
                zeros = True
                xa = np.array(x)
                zneg += int(((xa == 0) & np.signbit(xa)).sum())
                zpos += int(((xa == 0) & ~np.signbit(xa)).sum())
            if fn in ("min", "max") and "keys" not in skip:
                arg = cols[R.COL[col]]
                starts = _count(first.values(), lambda r: arg[r] > 0 if fn == "min" else arg[r] < 0)
                assert starts >= 4, "%s: %s(%s) starts beyond zero in %d groups" % (ctx, fn, col, starts)
            if fn in ("min", "max") and col == "b":
                seen = {}
                for r in rows:
                    seen.setdefault(group[r], set()).add(int(cols[R.COL["b"]][r]))
                assert any({1 << 53, (1 << 53) + 1} <= s for s in seen.values()), ctx
    if zeros and "zeros" not in skip:
        assert zneg >= 16 and zpos >= 16, "%s: min / max is -0.0 in %d rows, +0.0 in %d" % (body, zneg, zpos)
    return live, twins


def run_cuts(plan, outs, snapshot_at=None, key=None, **opts):
    """The stream in the batches CUTS -> ({out: rows}, stats).  snapshot_at:
    the cut at which the state moves into a fresh runtime.  key: runtime ->
    the key column (long values, dictionary ids)."""
    ts, cols = data()
    cols = list(cols)

    def start():
        rt = fs.SiddhiAppRuntime(plan, **opts)
        for o in outs:
            rt.add_callback(o)
        return rt
    rt = start()
    if key is not None:
        cols[0] = key(rt)
    got = {o: [] for o in outs}
    for s, e in zip(CUTS[:-1], CUTS[1:]):
        if s == snapshot_at:
            snap = rt.snapshot()
            rt.shutdown()
            rt = start()
            rt.restore(snap)
        rt.send("S", ts[s:e], [c[s:e] for c in cols])
        rt.flush()
        for o in outs:
            got[o] += engine_rows(rt.collect(o))
    st = rt.stats()
    rt.shutdown()
    return got, st


def out_types(plan, out):
    return [a.type for a in O.parse_app(strip_windows(plan)[0]).out_streams[out].attrs]


def same(got, want, plan, outs, ctx):
    for o in outs:
        X.same_rows_bits(got[o], want.get(o, []), out_types(plan, o), "%s %s" % (ctx, o))


# ------------------------------------------------------- stand-alone walk --
# A single aggregate query in the app: a multi-query group of one query is
# dissolved (build_mq_groups in engine.cpp: "a group of one query stays on its
# own PatternRT"), so the query runs k_walk's agg_key, always with the
# interpreter's environment (AggEnv).  8 aggregates = kMaxAggs.
SUMS8 = ("sum(a) as sa, sum(b) as sb, sum(c) as sc, sum(d) as sd, avg(a) as aa, avg(b) as ab, avg(c) as ac, "
         "avg(d) as ad")
EXTS8 = ("min(a) as m1, min(b) as m2, min(c2) as m3, min(d2) as m4, max(a) as x1, max(b) as x2, max(c2) as x3, "
         "max(d2) as x4")
COMPUTED = "sum(a) + max(b) as x, avg(c) * 2.0 as y, min(d2) as m, sum(d) as sd"


def grouped(items, having=None):
    return "from S select k, %s group by k %sinsert into O;" % (items, "having %s " % having if having else "")


def partitioned(items, having=None, window=""):
    return ("partition with (k of S) begin from S%s select k, %s %sinsert into O; end;"
            % (window, items, "having %s " % having if having else ""))


WALK = {
    "sums": (grouped(SUMS8), ()),
    "extremes": (grouped(EXTS8), ()),
    # having on an aggregate of each output type, the constant at an edge
    "having_long": (grouped("sum(b) as sb, count() as n", "sb < 0"), ()),
    "having_double": (grouped("avg(d) as ad, sum(a) as sa", "ad >= 0.0"), ()),        # NaN is not
    "having_float": (grouped("min(c2) as m5, max(a) as x", "m5 <= 0.0"), ()),         # -0.0 is; float widened
    "computed": (grouped(COMPUTED, "y != 0.0"), ()),
    "partition_sums": (partitioned(SUMS8), ()),
    "partition_extremes": (partitioned(EXTS8), ()),
    "partition_computed": (partitioned(COMPUTED, "m <= 0.0"), ()),
    # no filter: every 2048-row tile of the partition pass lands in one bucket,
    # two LDS windows of 1024 records each (k_walk splits the tile's segment by
    # arrival number); avg(c) is NaN once the group has met inf and -inf
    "global_dense": ("from S select sum(a) as sa, sum(b) as sb, avg(c) as ac, min(c2) as m, max(b) as x2, "
                     "count() as n insert into O;", ("keys", "zeros")),
    # one group: no second group to start beyond zero; and a single double sum
    # that has met inf and -inf is NaN for good, so the group is made of the
    # keys of finite values and takes no sum(d); its one running minimum is a
    # zero only until the first negative value arrives
    "global": ("from S[k % 8 != 0] select sum(a) as sa, sum(b) as sb, sum(c) as sc, avg(d) as ad, min(d2) as m, "
               "max(c2) as x, count() as n insert into O;", ("keys", "zeros")),
}


def walk_case(body, skip, ktype=O.INT, key=None, key_map=None, snapshot_at=None):
    want = reference(body)
    conditions(body, want, skip)
    plan = R.stream_def(ktype=ktype) + body
    got, st = run_cuts(plan, ["O"], snapshot_at=snapshot_at, key=key, chunk_events=CHUNK)
    assert st.kernel_launches[L.K_WALK] > 0 and st.kernel_launches[L.K_MQ_PARTITION] == 0
    if key_map is not None:
        want = {"O": [(t, s, (key_map(d[0]),) + d[1:]) for t, s, d in want["O"]]}
    same(got, want, plan, ["O"], body)


@pytest.mark.parametrize("name", list(WALK))
def test_stand_alone_walk(name):
    walk_case(*WALK[name])


KEYED4 = grouped("sum(a) as sa, min(b) as m, avg(c) as ac, max(d2) as x, min(c2) as m3")


def test_stand_alone_walk_long_key():
    walk_case(KEYED4, (), ktype=O.LONG, key=lambda rt: data()[1][0].astype(np.int64))


def test_stand_alone_walk_string_key():
    ids = {}

    def key(rt):
        for i in range(R.KEYS):
            ids[i] = rt.intern("key%d" % i)
        return np.array([ids[i] for i in range(R.KEYS)], np.int32)[data()[1][0]]
    walk_case(KEYED4, (), ktype=O.STRING, key=key, key_map=lambda k: ids[k])


def test_stand_alone_walk_snapshot_restore():
    walk_case(grouped("sum(a) as sa, sum(b) as sb, sum(c) as sc, avg(d) as ad, min(c2) as m3, max(b) as x2, "
                      "min(a) as m1, count() as n"), (), snapshot_at=2050)


# ----------------------------------------------------- multi-query groups --
# Apps of several candidate queries (mq_candidate in engine.cpp: int / long
# key, <= kMqMaxAggs = 4 aggregates, <= kMqMaxSel = 8 items that are the key,
# an aggregate or a carried column, a filter that lowers to a term list,
# having = `item op constant`).  Queries of one signature (mq_signature:
# select layout, aggregates, having item, operator and comparison type) form
# one class = one walk unit per nu queries; every
# shape comes twice, with another filter and another constant, so a unit's
# query 1 is exercised.  The unit: build_mq_groups, "mq_agg_fast: at most one
# non-count accumulator, having compared as a double or an integer (not a
# float)"; otherwise mq_agg_unit<8,1>, <4,2>, <2,4> by the number of non-count
# aggregates (nu = na <= 1 ? 8 : na == 2 ? 4 : 2).
# A group also prefetches at most kPref = 4 columns, the key among them
# (`fits` in build_mq_groups), so each app reads three columns beside k,
# filters included: a class that fits no group would quietly take the general
# path, which the launch counters below rule out.
# (filter, select items after k, having)
MQ = {
    # mq_agg_fast AOP 0 (sum / avg in double) over double, float and int arguments
    "fast_double": [("", "sum(d) as s", "s > 0.0"), ("[a < 0]", "sum(d) as s", "s > 1.5"),
                    ("", "sum(d) as s, count() as n", None),
                    ("", "avg(c) as v, count() as n", "v < 0.0"), ("[a > 0]", "avg(c) as v, count() as n", "v < 1.0"),
                    ("", "avg(a) as v", "v < 0"), ("[d != 0.0]", "avg(a) as v", "v < -65536"),
                    ("", "sum(c) as s, d", None)],
    # mq_agg_fast AOP 0 over a long argument, AOP 1 (integer sums), AOP 4 (count only)
    "fast_long": [("", "sum(a) as s", "s < 0"), ("[c <= 0.0f]", "sum(a) as s", "s < -4294967296L"),
                  ("", "sum(b) as s", "s >= 4294967296L"), ("[a < 0]", "sum(b) as s", "s >= 0L"),
                  ("", "avg(b) as v", "v >= 0.0"), ("[c <= 0.0f]", "avg(b) as v", "v >= 4294967296.0"),
                  ("", "a, sum(b) as s, count() as n", None),
                  ("", "count() as n", "n != 3")],
    # mq_agg_unit<8,1>: one min / max per query in compare domain 0 (int,
    # long); an integer sum whose having constant is a float
    "unit81_int": [("", "min(a) as m", "m < 0"), ("[b > 0]", "min(a) as m", "m < -7"),
                   ("", "max(a) as m", None),
                   ("", "max(b) as m", "m > 9007199254740992L"), ("[a < 0]", "max(b) as m", "m > 4294967297L"),
                   ("", "min(b) as m, a", None),
                   ("", "sum(a) as s", "s > 2.5f"), ("[b > 0]", "sum(a) as s", "s > -16777217.0f")],
    # compare domains 1 (float) and 2 (double)
    "unit81_float": [("", "min(c2) as m", "m <= 0.0f"), ("[a < 0]", "min(c2) as m", "m <= -1.0f"),
                     ("", "max(c2) as m", "m > 1.0000001"),       # float widened, not the constant narrowed
                     ("", "max(d2) as m", "m > 0.0"), ("[c2 <= 0.0f]", "max(d2) as m", "m > 1.5"),
                     ("", "a, min(d2) as m, c2", None)],
    # mq_agg_unit<4,2>: two accumulators of different operations and types
    "unit42_long": [("", "max(b) as m, sum(c) as s", "s > 0.0"), ("[a < 0]", "max(b) as m, sum(c) as s", "s > 1.5"),
                    ("", "sum(a) as s, c, min(b) as m, count() as n", None),
                    ("[c <= 0.0f]", "sum(a) as s, c, min(b) as m, count() as n", None)],
    "unit42_float": [("", "min(c2) as m, avg(a) as v", "m <= 0.0f"),
                     ("[b > 0]", "min(c2) as m, avg(a) as v", "m <= -1.0f"),
                     ("", "min(a) as m, max(c2) as x", None), ("[b > 0]", "min(a) as m, max(c2) as x", None)],
    # mq_agg_unit<2,4>: four accumulators; three and count() (kMqMaxAggs = 4)
    "unit24": [("", "sum(a) as s, min(d2) as m, max(b) as x, avg(a) as v", "s < 0"),
               ("[a < 0]", "sum(a) as s, min(d2) as m, max(b) as x, avg(a) as v", "s < -65536"),
               ("", "count() as n, sum(b) as s, min(a) as m, max(d2) as x, a", "n > 3"),
               ("[b > 0]", "count() as n, sum(b) as s, min(a) as m, max(d2) as x, a", "n > 1")],
}


def mq_body(name):
    return "".join("from S%s select k, %s group by k %sinsert into O%d;"
                   % (f, items, "having %s " % h if h else "", i) for i, (f, items, h) in enumerate(MQ[name]))


def mq_case(name, snapshot_at=None):
    body = mq_body(name)
    outs = ["O%d" % i for i in range(len(MQ[name]))]
    want = reference(body)
    conditions(body, want)
    plan = R.stream_def() + body
    got, st = run_cuts(plan, outs, snapshot_at=snapshot_at, chunk_events=CHUNK)
    # every query is in a group: none took the general partition pass / walk
    assert st.kernel_launches[L.K_MQ_PARTITION] > 0 and st.kernel_launches[L.K_MQ_WALK] > 0
    assert st.kernel_launches[L.K_PARTITION] == 0 and st.kernel_launches[L.K_WALK] == 0
    same(got, want, plan, outs, name)


@pytest.mark.parametrize("name", list(MQ))
def test_multi_query_group(name):
    mq_case(name)


def test_multi_query_group_snapshot_restore():
    mq_case("unit24", snapshot_at=2050)


# -------------------------------------------------------- sliding windows --
# `partition with (k of S)`: one ring per key, k_winwalk's win_key
# (run_pattern in engine.cpp: `rt.win.kind != WIN_NONE` -> launch_winwalk,
# counted as K_AGG).  No having and only key / aggregate / carried items:
# k_winwalk<false>, the build without the interpreter; otherwise <true>.
W_SUMS = "sum(a) as sa, sum(b) as sb, sum(c) as sc, sum(d) as sd, avg(a) as aa, avg(b) as ab, avg(c) as ac, count() as n"
TIME_T = 120          # a key's rows are 96 ms apart on average: windows hold 0 to 8 rows
SLOTS = 16
WINDOWS = {
    # a window of one value is that value: its sums neither wrap, leave int32
    # nor need more than a float, and its double sum is +-inf only in the one
    # row where a key first meets inf (12 keys have any), NaN from then on
    "length1_sums": (partitioned(W_SUMS, window="#window.length(1)"), ("wrap", "int32", "float32", "inf"), {}),
    "length2_sums": (partitioned(W_SUMS, window="#window.length(2)"), (), {}),
    "length5_sums": (partitioned(W_SUMS, window="#window.length(5)"), (), {}),
    "length1_extremes": (partitioned(EXTS8, window="#window.length(1)"), (), {}),
    "length2_extremes": (partitioned(EXTS8, window="#window.length(2)"), (), {}),
    "length5_extremes": (partitioned(EXTS8, window="#window.length(5)"), (), {}),
    "time_sums": (partitioned(W_SUMS, window="#window.time(%d)" % TIME_T), (), {"pending_slots": SLOTS}),
    "time_extremes": (partitioned(EXTS8, window="#window.time(%d)" % TIME_T), (), {"pending_slots": SLOTS}),
    "length5_computed": (partitioned(COMPUTED + ", min(c2) as m3", "m3 <= 0.0", "#window.length(5)"), (), {}),
    "time_computed": (partitioned(COMPUTED + ", min(c2) as m3", "y != 0.0", "#window.time(%d)" % TIME_T), (),
                      {"pending_slots": SLOTS}),
    # one window for the whole stream: one group, as the stand-alone "global"
    "global_length5": ("from S[k % 8 != 0]#window.length(5) select sum(b) as sb, min(c2) as m, max(a) as x, "
                       "sum(c) as sc, avg(d) as ad, max(d2) as x4, sum(a) as sa insert into O;", ("keys",), {}),
}


def window_case(name, snapshot_at=None):
    body, skip, opts = WINDOWS[name]
    want, live = reference(body, windows=True)
    ref_live, twins = conditions(body, want, skip)
    assert live == ref_live and live <= opts.get("pending_slots", 255)
    if "time" in name:
        assert live <= 8
    if "extremes" in name and "length1" not in name:
        # the extreme leaves while an equal value (or its -0.0 / 0.0 twin) stays
        assert twins >= 16, "%s: %d" % (name, twins)
    plan = R.stream_def() + body
    got, st = run_cuts(plan, ["O"], snapshot_at=snapshot_at, chunk_events=CHUNK, **opts)
    assert st.kernel_launches[L.K_AGG] > 0
    same(got, want, plan, ["O"], name)


@pytest.mark.parametrize("name", list(WINDOWS))
def test_sliding_window(name):
    window_case(name)


def test_length_window_snapshot_restore():
    window_case("length5_sums", snapshot_at=2050)


def test_time_window_snapshot_restore():
    window_case("time_extremes", snapshot_at=4099)


# --------------------------------------------------------- derived stream --
def test_aggregates_over_a_derived_stream():
    """A producer computes a float and a long column (k_derive); a grouped
    reader, the only aggregate query of the app and so on the stand-alone
    walk, sums the float in double and takes the minimum of the long.
    Expected rows: chain_model over the two layers."""
    producer = "from S select k, c * 2.5f as y, b / 3 as q insert into M;"
    reader = "from M select k, sum(y) as sy, min(q) as mq, avg(y) as ay group by k insert into O;"
    ts, cols = data()
    layers = [R.stream_def() + producer, "define stream M (k int, y float, q long);" + reader]
    key = ("chain", producer, reader)
    if key not in _REF:
        _REF[key] = chain_run(layers, R.events(ts, cols))[0]
    want = _REF[key]
    sy = np.array([d[1] for _, _, d in want["O"]])
    with np.errstate(all="ignore"):
        assert (np.isfinite(sy) & (sy.astype(np.float32).astype(np.float64) != sy)).sum() >= 16
    assert np.isnan(sy).sum() >= 16 and np.isinf(sy).sum() >= 16
    mq = [d[2] for _, _, d in want["O"]]
    assert _count(mq, lambda v: v < X.INT_MIN) >= 256 and _count(mq, lambda v: v > 0) >= 16
    plan = R.stream_def() + producer + reader
    got, st = run_cuts(plan, ["M", "O"], chunk_events=CHUNK)
    assert st.kernel_launches[L.K_OTHER] > 0 and st.kernel_launches[L.K_WALK] > 0          # k_derive, k_walk
    assert st.kernel_launches[L.K_MQ_PARTITION] == 0
    X.same_rows_bits(got["M"], want["M"], [O.INT, O.FLOAT, O.LONG], "derived stream M")
    X.same_rows_bits(got["O"], want["O"], [O.INT, O.DOUBLE, O.LONG, O.DOUBLE], "derived stream O")
