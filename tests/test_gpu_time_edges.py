"""Time-edge parity of every path that stores a 32-bit event time.

Every pattern, window and multi-query kernel stores an event's time as a
32-bit offset from its chunk's first row and rebuilds the 64-bit value when it
compares against `within` or a window length; the encodings differ (unsigned:
closed form in event time; biased by 2^31: order-tolerant / adaptive closed
form and the hot-key scans; signed: general path, windows, multi-query groups,
received shuffle records).  tests/time_edges.py moves the seeded stream to
bases where a wrong decode shows (zero crossing, 2^31, 2^32, a wrapping low
word, the far ends of int64) and puts jumps of W - 1 / W on tile, chunk and
batch borders (`edge`), stretches one chunk to the widest accepted span of
2^31 - 1 ms (`wide`), and keeps partials alive across chunks whose bases lie
more than 2^31 ms apart under `within 30 days` / `within 1 year`
(`long_within`).  tests/test_time_edges.py checks the references against each
other at these values; here every path is bit-exact against them (rows, ts,
seq, global and per-key order), and each case proves from the launch counters
that the intended path ran.

The span contract (test_span_*): a chunk whose rows lie up to 2^31 - 1 ms
after its first row is exact on every path; one that reaches 2^32 ms is
refused with the "2^31 ms" message (never with "not in event-time order": the
stream is in order).  In between (2^31 + 5 ms) the paths differ, as observed
on an MI355X: the closed form in event time and its adaptive build (ts_order
0, chunk in order) store the offset unsigned and are exact up to 2^32 - 1 ms;
the general two-state and N-state walks, the window walk (signed field,
k_partition) and the multi-query group (signed field, k_mqpart) refuse it, and
so does the order-tolerant closed form (biased field) for rows 2^31 ms or more
after, or more than 2^31 ms before, the chunk's first row.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import flink_siddhi as fs  # noqa: E402
from flink_siddhi import _lib as L  # noqa: E402
from flink_siddhi import workload  # noqa: E402
import time_edges as TE  # noqa: E402
from helpers import assert_same_rows, engine_rows, oracle_run, workload_events  # noqa: E402
from test_gpu_atol import adaptive_ran  # noqa: E402
from test_gpu_nfa import EV3, P3, events as events3  # noqa: E402
from test_gpu_ooo_cf import assert_same_per_key  # noqa: E402
from test_time_edges import WINDOW_PLAN, window_want  # noqa: E402

NK = 12   # kernel launch counters


class Stats:
    """Launch counters and hot-key sightings summed over the runtimes of one case."""

    def __init__(self):
        self.kernel_launches = [0] * NK
        self.hot_seen = 0

    def add(self, st):
        for i in range(NK):
            self.kernel_launches[i] += st.kernel_launches[i]
        self.hot_seen += st.hot_keys


def run_host(plan, w, sizes, outs=("O",), snapshot_after=None, key=None, chunk=TE.CHUNK, **opts):
    """Host batches of `sizes` rows through one runtime (snapshot_after = i:
    snapshot after batch i, restore into a fresh runtime) -> ({out: rows}, Stats)."""
    def make():
        r = fs.SiddhiAppRuntime(plan, chunk_events=chunk, **opts)
        for o in outs:
            r.add_callback(o)
        return r
    k = w["k"] if key is None else key
    got, st, first = {o: [] for o in outs}, Stats(), 0
    rt = make()
    try:
        for i, n in enumerate(sizes):
            s, e = first, first + n
            rt.send("A", w["ts"][s:e], [k[s:e], w["ts"][s:e], w["id"][s:e], w["price"][s:e]],
                    streams=w["stream"][s:e])
            rt.flush()
            st.hot_seen += rt.stats().hot_keys
            first = e
            if i == snapshot_after:
                for o in outs:
                    got[o] += engine_rows(rt.collect(o))
                st.add(rt.stats())
                snap = rt.snapshot()
                rt.shutdown()
                rt = make()
                rt.restore(snap)
        for o in outs:
            got[o] += engine_rows(rt.collect(o))
        st.add(rt.stats())
    finally:
        rt.shutdown()
    return got, st


# ---- two-state paths: a closed form, b general, c adaptive, d order-tolerant,
# ---- e hot keys (event time and order-tolerant scans), f sparse keys ---------
TWO_STATE = ("cf", "general", "adaptive", "tolerant", "hot", "hot_tol", "sparse")
SPARSE_BASE, SPARSE_MUL = 1 << 40, 7919
_cases = {}


def split3(sizes):
    """The same rows in three batches with the same chunk borders (the first
    chunk alone, then the rest of the first batch): diversion of hot keys
    starts with the batch after the one that found them."""
    assert sizes[0] > TE.CHUNK
    return (TE.CHUNK, sizes[0] - TE.CHUNK) + tuple(sizes[1:])


def two_state_case(path, jump_set, base_name, within):
    """(rows, batch sizes, reference rows) of a path's stream: the shared one,
    or the path's variant of it with the oracle run again on that variant."""
    variant = {"tolerant": "late", "hot": "hot", "hot_tol": "hot", "general": "short"}.get(path, "")
    key = (variant, jump_set, base_name, within)
    if key not in _cases:
        w, sizes, rows, _ = TE.pattern_want(jump_set, base_name, within)
        if variant == "late":
            w = TE.late_blocks(w, sizes)
            for c0 in TE.chunk_starts(sizes)[:-1]:
                assert (np.diff(w["ts"][c0:c0 + TE.CHUNK]) < 0).any()
        elif variant == "hot":
            w = TE.hot_key(w, key=TE.EDGE_KEY)
            keep = ((w["stream"] == 0) & (w["price"] > 0.5)) | ((w["stream"] == 1) & (w["id"] % 7 == 0))
            per_chunk = [int((keep[c:c + TE.CHUNK] & (w["k"][c:c + TE.CHUNK] == TE.EDGE_KEY)).sum())
                         for c in TE.chunk_starts(sizes)[:2]]
            assert min(per_chunk) > 2 * 256, per_chunk      # the hot-key threshold is 256 kept records
        if variant == "short":      # the general walk has no overflow pool: TE.SHORT_PLAN
            a, b = TE.c_pairs(w, within, f_above=TE.SHORT_F, g_mod=TE.SHORT_G)
            rows = TE.pair_rows(w, a, b)
        elif variant:
            a, b = TE.c_pairs(w, within)
            rows = TE.pair_rows(w, a, b)
        _cases[key] = (w, sizes, rows)
    return _cases[key]


def run_two_state(path, jump_set, base_name, monkeypatch, within_text="10 sec", within=TE.W, snapshot=False):
    w, sizes, want = two_state_case(path, jump_set, base_name, within)
    plan = TE.plan_within(within_text, TE.SHORT_PLAN if path == "general" else workload.PATTERN_PLAN)
    opts = {"key_capacity": 4096, "buckets_log2": 4}
    key = None
    if path == "general":
        monkeypatch.setenv("CEP_NO_CF", "1")
    else:
        monkeypatch.delenv("CEP_NO_CF", raising=False)
    opts["ts_order"] = 1 if path in ("cf", "general", "hot", "sparse") else 0
    if path in ("hot", "hot_tol"):
        sizes = split3(sizes)
    if path == "sparse":
        plan = plan.replace("k int", "k long")
        opts["sparse_keys"] = 1
        key = w["k"].astype(np.int64) * SPARSE_MUL + SPARSE_BASE
        want = [(ts, seq, (k * SPARSE_MUL + SPARSE_BASE, p1, p2, t)) for ts, seq, (k, p1, p2, t) in want]
    snap_at = None
    if snapshot:
        snap_at = len(sizes) - 2
    got, st = run_host(plan, w, sizes, key=key, snapshot_after=snap_at, **opts)
    got = got["O"]
    kl = st.kernel_launches
    if path == "general":
        assert kl[L.K_WALK] > 0 and kl[L.K_CF_WALK] == 0, kl
    else:
        assert kl[L.K_CF_WALK] > 0 and kl[L.K_WALK] == 0, kl
    if path == "adaptive":
        assert adaptive_ran(st) and kl[L.K_HOT] == 0, kl
    if path in ("hot", "hot_tol"):
        assert kl[L.K_HOT] > 0 and st.hot_seen > 0, kl
    elif path != "tolerant":
        assert kl[L.K_HOT] == 0, kl
    ctx = "%s %s %s within %s" % (path, jump_set, base_name, within_text)
    assert len(want) > 1000
    assert_same_rows(got, want, ctx)
    assert_same_per_key(TE.rows_columns(got), TE.rows_columns(want))
    return len(want)


@pytest.mark.parametrize("base_name", TE.GPU_BASES)
@pytest.mark.parametrize("path", TWO_STATE)
def test_two_state_edge(path, base_name, monkeypatch):
    run_two_state(path, "edge", base_name, monkeypatch)


@pytest.mark.parametrize("base_name", TE.WIDE_BASES)
@pytest.mark.parametrize("path", TWO_STATE)
def test_two_state_wide(path, base_name, monkeypatch):
    run_two_state(path, "wide", base_name, monkeypatch)


LONG_CASES = [("30 days", "epoch_wrap"), ("30 days", "neg2^32"), ("1 year", "neg5000"), ("1 year", "2^62")]


@pytest.mark.parametrize("within_text,base_name", LONG_CASES)
@pytest.mark.parametrize("path", ("cf", "general", "adaptive", "hot", "hot_tol"))
def test_two_state_long_within(path, within_text, base_name, monkeypatch):
    run_two_state(path, "long_within", base_name, monkeypatch, within_text, TE.LONG_WITHIN[within_text])


@pytest.mark.parametrize("within_text,base_name", [("30 days", "neg2^32"), ("1 year", "epoch_wrap")])
def test_closed_form_snapshot_between_the_long_jumps(within_text, base_name, monkeypatch):
    # key 63's partials (and under `1 year` every older one) are pending in
    # the snapshot, 2^31 - 20000 ms and more before the rows that follow
    run_two_state("cf", "long_within", base_name, monkeypatch, within_text, TE.LONG_WITHIN[within_text],
                  snapshot=True)


@pytest.mark.parametrize("base_name", ["T0", "epoch_wrap"])
def test_tolerant_late_row_at_the_far_end_of_the_biased_field(base_name, monkeypatch):
    """Order-tolerant closed form: one row of the second chunk moved back by
    2^31 - 1 ms, so it lies 2^31 - 1 - (its offset) before the chunk's first
    row: the lowest values of the biased 32-bit field."""
    monkeypatch.delenv("CEP_NO_CF", raising=False)
    w, sizes, _, _ = TE.pattern_want("edge", base_name)
    w = TE.late_blocks(w, sizes)
    off = 100
    r = TE.CHUNK + off
    w["ts"][r] -= TE.SPAN_MAX
    assert int(w["ts"][TE.CHUNK] - w["ts"][r]) == TE.SPAN_MAX - off
    a, b = TE.c_pairs(w)
    want = TE.pair_rows(w, a, b)
    got, st = run_host(workload.PATTERN_PLAN, w, sizes, ts_order=0, key_capacity=4096, buckets_log2=4)
    assert st.kernel_launches[L.K_CF_WALK] > 0 and st.kernel_launches[L.K_WALK] == 0
    assert len(want) > 1000
    assert_same_rows(got["O"], want, "late row 2^31 - 1 ms back, base %s" % base_name)
    assert_same_per_key(TE.rows_columns(got["O"]), TE.rows_columns(want))


# ---- g: N-state patterns and sequences on k_walk -----------------------------------
NFA = {
    "pattern": "from every s1=A -> s2=B -> s3=C within %s "
               "select s1.k as k, s1.ts as t1, s2.ts as t2, s3.ts as t3 insert into O;",
    "kleene": "from every s1=A, s2=B+, s3=C within %s "
              "select s1.k as k, s1.ts as t1, s2[last].ts as t2, s3.ts as t3 insert into O;",
}
_nfa = {}


def nfa_case(query, jump_set, base_name, within_text):
    key = (query, jump_set, base_name, within_text)
    if key not in _nfa:
        w, _, sizes = TE.stream(jump_set, base_name)
        w = TE.three_streams(w)
        plan = EV3 + P3 + NFA[query] % within_text + " end;"
        _nfa[key] = (plan, w, sizes, oracle_run(plan, events3(w)).get("O", []))
    return _nfa[key]


def run_nfa(query, jump_set, base_name, within_text="10 sec", snapshot=False):
    plan, w, sizes, want = nfa_case(query, jump_set, base_name, within_text)
    got, st = run_host(plan, w, sizes, snapshot_after=0 if snapshot else None, ts_order=1, key_capacity=4096,
                       pending_slots=16)
    assert st.kernel_launches[L.K_WALK] > 0 and st.kernel_launches[L.K_CF_WALK] == 0
    assert st.kernel_launches[L.K_MQ_WALK] == 0
    assert len(want) > 1000
    assert_same_rows(got["O"], want, "%s %s %s" % (query, jump_set, base_name))
    return want


@pytest.mark.parametrize("base_name", TE.GPU_BASES)
@pytest.mark.parametrize("query", list(NFA))
def test_nfa_edge(query, base_name):
    run_nfa(query, "edge", base_name)


@pytest.mark.parametrize("base_name", TE.WIDE_BASES)
@pytest.mark.parametrize("query", list(NFA))
def test_nfa_wide(query, base_name):
    run_nfa(query, "wide", base_name)


def far_apart(want, bits):
    return sum(1 for _, _, d in want if d[3] - d[1] > 1 << bits)


@pytest.mark.parametrize("snapshot", [False, True], ids=["straight", "snapshot"])
@pytest.mark.parametrize("within_text,base_name", [("30 days", "neg2^32"), ("1 year", "epoch_wrap")])
def test_nfa_pattern_long_within(within_text, base_name, snapshot):
    want = run_nfa("pattern", "long_within", base_name, within_text, snapshot=snapshot)
    # the planted keys: A's in the first chunk, their B and C 2^31 (2^32) ms later
    assert far_apart(want, 31) >= 3
    assert (far_apart(want, 32) >= 2) == (within_text == "1 year")


# ---- h: a multi-query group (k_mqpart / k_mqwalk; chunks of 16384 rows) ------------
MQ_OUTS = ("Seq0", "Seq1", "Seq2", "Agg0")
_mq = {}


def mq_plan(within_text):
    return (EV3 + P3 +
            "from every s1=A[price > 0.5], s2=B[id %% 7 == 0] within %s "
            "select s1.k as k, s1.price as p1, s2.price as p2, s2.ts as t insert into Seq0;"
            "from every s1=A[price > 0.25], s2=B+, s3=C within %s "
            "select s1.k as k, s1.ts as t1, s2[last].price as p2, s3.ts as t3 insert into Seq1;"
            # a bounded count: not bit-parallel, the generic sequence unit (mq_seq)
            "from every s1=A[price > 0.25], s2=B<2:3>, s3=C within %s "
            "select s1.k as k, s1.ts as t1, s2[last].ts as t2, s3.ts as t3 insert into Seq2;"
            " end;"
            "from A[id >= 3] select k, sum(price) as total, count() as n group by k having total > 1.0 "
            "insert into Agg0;") % (within_text, within_text, within_text)


def run_mq(jump_set, base_name, within_text="10 sec", late=False):
    """late: ts_order 0 and a block of rows in every 16384-row chunk that lie
    before the chunk's first row (negative values of the signed field)."""
    key = (jump_set, base_name, within_text, late)
    if key not in _mq:
        w, _, sizes = TE.stream(jump_set, base_name)
        w = TE.three_streams(w)
        if late:
            w = TE.late_blocks(w, sizes, chunk=2 * TE.CHUNK)
        _mq[key] = (w, sizes, oracle_run(mq_plan(within_text), events3(w)))
    w, sizes, want = _mq[key]
    got, st = run_host(mq_plan(within_text), w, sizes, outs=MQ_OUTS, key_capacity=64, ts_order=0 if late else 1)
    assert st.kernel_launches[L.K_MQ_WALK] > 0 and st.kernel_launches[L.K_WALK] == 0, list(st.kernel_launches)
    for o in MQ_OUTS:
        assert len(want.get(o, [])) > {"Seq0": 400, "Seq1": 1000, "Seq2": 100, "Agg0": 1000}[o], o
        assert_same_rows(got[o], want.get(o, []), "%s %s %s" % (o, jump_set, base_name))
    return want


@pytest.mark.parametrize("base_name", TE.GPU_BASES)
def test_mq_edge(base_name):
    want = run_mq("edge", base_name)
    # the pairs planted across the W - 1 jumps are contiguous in their key:
    # Seq0 matches them exactly W apart
    w, jumps, _ = TE.stream("edge", base_name)
    seqs = {seq for _, seq, _ in want["Seq0"]}
    for r, j in jumps:
        assert (r in seqs) == (j == TE.W - 1), (r, j)


@pytest.mark.parametrize("base_name", TE.GPU_BASES)
def test_mq_edge_with_rows_before_the_chunk(base_name):
    run_mq("edge", base_name, late=True)


@pytest.mark.parametrize("base_name", TE.WIDE_BASES)
def test_mq_wide(base_name):
    run_mq("wide16k", base_name)


@pytest.mark.parametrize("within_text,base_name", [("30 days", "neg2^32"), ("1 year", "epoch_wrap")])
def test_mq_long_within(within_text, base_name):
    run_mq("long_within", base_name, within_text)


# ---- i: #window.time(50), partitioned, all aggregates (k_partition / k_winwalk) ----
def run_window(jump_set, base_name, jitter, ts_order):
    w, sizes, want, live = window_want(jump_set, base_name, jitter)
    assert 4 < live <= 32, live
    got, st = run_host(WINDOW_PLAN, w, sizes, ts_order=ts_order, pending_slots=32, key_capacity=64)
    kl = st.kernel_launches
    assert kl[L.K_PARTITION] > 0 and kl[L.K_AGG] > 0 and kl[L.K_WALK] == 0, list(kl)
    assert len(want) == len(w["ts"])
    assert_same_rows(got["O"], want, "window %s %s jitter %d" % (jump_set, base_name, jitter))


@pytest.mark.parametrize("base_name", TE.GPU_BASES)
@pytest.mark.parametrize("jitter,ts_order", [(0, 1), (15, 0)], ids=["in_order", "jitter15"])
def test_window_time_edge(jitter, ts_order, base_name):
    run_window("edge", base_name, jitter, ts_order)


@pytest.mark.parametrize("base_name", TE.WIDE_BASES)
def test_window_time_wide(base_name):
    run_window("wide", base_name, 0, 1)


# ---- j: received shuffle records (two ranks) -----------------------------------------
@pytest.mark.parametrize("path", ["cf", "general"])
def test_received_records_wide(path, monkeypatch):
    """Two simulated shuffle ranks (route -> send_records): the owner of key 4
    receives step 0's first and last row in one chunk, 2^31 - 1 ms apart (the
    signed field of a received record, kernels.hip from_records), then records
    2^40 ms later."""
    import torch
    if path == "general":
        monkeypatch.setenv("CEP_NO_CF", "1")
    else:
        monkeypatch.delenv("CEP_NO_CF", raising=False)
    world, n_per, steps = 2, TE.CHUNK, 2
    w, _ = TE.records_wide_stream(TE.BASES["epoch_wrap"], n_per, world, steps)
    plan = TE.SHORT_PLAN if path == "general" else workload.PATTERN_PLAN
    a, b = TE.c_pairs(w, f_above=TE.SHORT_F, g_mod=TE.SHORT_G) if path == "general" else TE.c_pairs(w)
    want = TE.pair_columns(w, a, b)
    assert len(a) > 1000 and ((a < world * n_per) & (b >= world * n_per)).sum() == 0
    rts = [fs.SiddhiAppRuntime(plan, ts_order=1, key_stride=world, key_offset=r,
                               chunk_events=TE.CHUNK, key_capacity=TE.KEYS // world, buckets_log2=2,
                               ordered_output=0) for r in range(world)]
    parts = []
    try:
        for s in range(steps):
            segs = [[] for _ in range(world)]
            for src in range(world):
                first = (s * world + src) * n_per
                d = {c: torch.from_numpy(np.ascontiguousarray(w[c][first:first + n_per])).cuda()
                     for c in ("k", "ts", "id", "price", "stream")}
                recs, counts = rts[src].route("A", d["ts"], [d["k"], d["ts"], d["id"], d["price"]], world,
                                              seq0=first, streams=d["stream"])
                off = np.concatenate([[0], np.cumsum(counts)])
                for r in range(world):
                    segs[r].append(recs[off[r]:off[r + 1]].clone())
            for r in range(world):
                recv = torch.cat(segs[r], dim=0)
                assert 0 < recv.shape[0] <= TE.CHUNK      # one chunk per owner and step
                rts[r].send_records(recv, recv.shape[0], n_per)
                parts.append(rts[r].output_tensors("O", copy=True))
                rts[r].flush()
        torch.cuda.synchronize()
        kl = [sum(rt.stats().kernel_launches[i] for rt in rts) for i in range(NK)]
    finally:
        for rt in rts:
            rt.shutdown()
    if path == "cf":
        assert kl[L.K_CF_WALK] >= world * steps and kl[L.K_WALK] == 0, kl
    else:
        assert kl[L.K_WALK] >= world * steps and kl[L.K_CF_WALK] == 0, kl
    got = {c: torch.cat([p[2][i] for p in parts]).cpu().numpy() for i, c in enumerate(("k", "p1", "p2", "t"))}
    got["ts"] = torch.cat([p[0] for p in parts]).cpu().numpy()
    got["seq"] = torch.cat([p[1] for p in parts]).cpu().numpy()
    assert_same_per_key(got, want)


# ---- the span contract -------------------------------------------------------------------
SPAN_PATHS = ("cf", "general", "adaptive", "nfa", "mq", "window")
SPAN_MSG = r"2\^31 ms"
_small = {}


def span_setup(path, monkeypatch):
    """(plan, outs, chunk rows, runtime options, stream transform, path check) of a span-contract path."""
    monkeypatch.delenv("CEP_NO_CF", raising=False)
    two = {"key_capacity": 4096, "buckets_log2": 4}
    ident = lambda w: w  # noqa: E731
    if path == "cf":
        return workload.PATTERN_PLAN, ("O",), TE.CHUNK, dict(two, ts_order=1), ident
    if path == "general":
        monkeypatch.setenv("CEP_NO_CF", "1")
        return TE.SHORT_PLAN, ("O",), TE.CHUNK, dict(two, ts_order=1), ident
    if path == "adaptive":
        return workload.PATTERN_PLAN, ("O",), TE.CHUNK, dict(two, ts_order=0), ident
    if path == "nfa":
        return (EV3 + P3 + NFA["pattern"] % "10 sec" + " end;", ("O",), TE.CHUNK,
                dict(ts_order=1, key_capacity=4096, pending_slots=16), TE.three_streams)
    if path == "mq":
        return mq_plan("10 sec"), MQ_OUTS, 2 * TE.CHUNK, dict(ts_order=1, key_capacity=64), TE.three_streams

    def all_a(w):
        w = {c: v.copy() for c, v in w.items()}
        w["stream"] = np.zeros(len(w["ts"]), np.uint8)
        return w
    return WINDOW_PLAN, ("O",), TE.CHUNK, dict(ts_order=1, pending_slots=32, key_capacity=64), all_a


def reference(path, plan, w):
    if path == "window":
        from window_model import model_run
        return model_run(plan, workload_events(w))[0]
    if path in ("nfa", "mq"):
        return oracle_run(plan, events3(w))
    a, b = TE.c_pairs(w, f_above=TE.SHORT_F, g_mod=TE.SHORT_G) if path == "general" else TE.c_pairs(w)
    return {"O": TE.pair_rows(w, a, b)}


def fresh_runtime_works(path, plan, outs, chunk, opts, prep):
    """A short run at T0 on a new runtime, exact."""
    if path not in _small:
        w = prep({c: v[:6000] for c, v in TE.generated().items()})
        _small[path] = (w, reference(path, plan, w))
    w, want = _small[path]
    got, _ = run_host(plan, w, (len(w["ts"]),), outs=outs, chunk=chunk, **opts)
    for o in outs:
        assert len(want.get(o, [])) > 0
        assert_same_rows(got[o], want.get(o, []), "fresh runtime after a refused chunk (%s)" % o)


@pytest.mark.parametrize("path", SPAN_PATHS)
def test_span_of_2_32_ms_is_refused_as_a_span(path, monkeypatch):
    plan, outs, chunk, opts, prep = span_setup(path, monkeypatch)
    w = prep(TE.span_stream(TE.BASES["epoch_wrap"], 1 << 32, chunk=chunk))
    with pytest.raises(ValueError, match=SPAN_MSG) as ei:
        run_host(plan, w, (len(w["ts"]),), outs=outs, chunk=chunk, **opts)
    assert "not in event-time order" not in str(ei.value)
    fresh_runtime_works(path, plan, outs, chunk, opts, prep)


# observed: the closed form in event time and its adaptive build (unsigned
# field, up to 2^32 - 1 ms) accept 2^31 + 5 ms and are exact; the rest refuse it
SPAN_JUST_OVER_ACCEPTED = ("cf", "adaptive")


@pytest.mark.parametrize("path", SPAN_PATHS)
def test_span_just_over_2_31_ms_is_exact_or_refused(path, monkeypatch):
    """Observed on an MI355X: cf and adaptive accept the chunk and are exact;
    general, nfa, mq and window refuse it with the span message."""
    plan, outs, chunk, opts, prep = span_setup(path, monkeypatch)
    w = prep(TE.span_stream(TE.BASES["neg5000"], (1 << 31) + 5, chunk=chunk))
    try:
        got, _ = run_host(plan, w, (len(w["ts"]),), outs=outs, chunk=chunk, **opts)
    except ValueError as e:
        assert "2^31 ms" in str(e) and "not in event-time order" not in str(e), str(e)
        print("span 2^31 + 5 ms on %s: refused" % path)
        assert path not in SPAN_JUST_OVER_ACCEPTED
        return
    print("span 2^31 + 5 ms on %s: accepted" % path)
    want = reference(path, plan, w)
    for o in outs:
        assert_same_rows(got[o], want.get(o, []), "span 2^31 + 5 ms, %s %s" % (path, o))
    assert path in SPAN_JUST_OVER_ACCEPTED


@pytest.mark.parametrize("path", ["closed_form", "window"])
def test_row_more_than_2_31_ms_before_its_chunk_is_refused(path, monkeypatch):
    """ts_order 0: a row more than 2^31 ms before its chunk's first row."""
    monkeypatch.delenv("CEP_NO_CF", raising=False)
    w, sizes, _, _ = TE.pattern_want("edge", "epoch_wrap")
    w = {c: v.copy() for c, v in w.items()}
    r = TE.CHUNK + 100
    w["ts"][r] = w["ts"][TE.CHUNK] - (1 << 31) - 1000
    if path == "window":
        w["stream"] = np.zeros(len(w["ts"]), np.uint8)
        plan, opts = WINDOW_PLAN, dict(pending_slots=32, key_capacity=64)
    else:
        plan, opts = workload.PATTERN_PLAN, dict(key_capacity=4096, buckets_log2=4)
    with pytest.raises(ValueError, match=SPAN_MSG) as ei:
        run_host(plan, w, sizes, ts_order=0, **opts)
    assert "not in event-time order" not in str(ei.value)


# ---- the reorder buffer ------------------------------------------------------------------
RO_PLAN = ("define stream S (k int, ts long, id int, price double);"
           "from S[id >= 0] select k, ts, id, price insert into O;")
RO_VALUES = (-(1 << 62), -1, 0, 1, 1 << 31, 1 << 32, 1 << 62)


def ro_stream(n=700, seed=5):
    """Arrivals whose ts are drawn from RO_VALUES (many ties) and their neighbours."""
    rng = np.random.default_rng(seed)
    ts = np.array(RO_VALUES, np.int64)[rng.integers(0, len(RO_VALUES), n)] + rng.integers(-1, 2, n)
    return {"k": rng.integers(0, 50, n).astype(np.int32), "ts": ts.astype(np.int64),
            "id": np.arange(n, dtype=np.int32), "price": rng.random(n)}


def ro_cols(w, idx):
    return [np.ascontiguousarray(w[c][idx]) for c in ("k", "ts", "id", "price")]


def ro_events(w, order):
    return [("S", int(w["ts"][i]), (int(w["k"][i]), int(w["ts"][i]), int(w["id"][i]), float(w["price"][i])))
            for i in order]


def ro_send(rt, w, idx):
    rt.process_elements("S", np.ascontiguousarray(w["ts"][idx]), ro_cols(w, idx))


def test_reorder_buffer_across_zero_and_the_far_ends():
    """Buffered ts from -2^62 to 2^62 with ties; watermarks on a tied value,
    on -1 and on 0.  Every release is the stable (ts, arrival) prefix; a
    genuine ts of 0 and a negative latest-released ts are not taken for "none"."""
    w = ro_stream()
    n = len(w["ts"])
    rt = fs.SiddhiAppRuntime(RO_PLAN)
    rt.add_callback("O")
    try:
        ro_send(rt, w, np.arange(n))
        assert rt.buffered() == n
        released = []
        held = np.arange(n)
        for mark in (-(1 << 62) - 2, -(1 << 62), -1, -1, 0, 1 << 31, (1 << 62) + 1):
            rt.process_watermark(int(mark))
            out = held[w["ts"][held] <= mark]
            released += sorted(out.tolist(), key=lambda i: (int(w["ts"][i]), i))
            held = held[w["ts"][held] > mark]
            assert rt.buffered() == len(held), mark
        assert len(held) == 0
        rt.flush()
        got = engine_rows(rt.collect("O"))
    finally:
        rt.shutdown()
    assert released == sorted(range(n), key=lambda i: (int(w["ts"][i]), i))     # a stable sort by ts
    assert_same_rows(got, oracle_run(RO_PLAN, ro_events(w, released))["O"], "reorder across zero")
    assert {0, -1, -(1 << 62)} <= {t for t, _, _ in got}


@pytest.mark.parametrize("released_to", [-1, 0])
def test_late_row_below_a_negative_or_zero_release(released_to):
    """late_policy 0: after rows up to ts = released_to were released, an older
    row is late (dropped and counted); one at released_to itself is not."""
    ts = np.array([-(1 << 62), -7, released_to, 5], np.int64)
    w = {"k": np.arange(4, dtype=np.int32), "ts": ts, "id": np.arange(4, dtype=np.int32), "price": np.full(4, 0.5)}
    more = {"k": np.array([9, 8, 7], np.int32), "ts": np.array([released_to - 1, released_to, 6], np.int64),
            "id": np.array([10, 11, 12], np.int32), "price": np.full(3, 0.25)}
    rt = fs.SiddhiAppRuntime(RO_PLAN, late_policy=0)
    rt.add_callback("O")
    try:
        ro_send(rt, w, np.arange(4))
        rt.process_watermark(released_to)
        assert rt.buffered() == 1 and rt.stats().late_events == 0
        ro_send(rt, more, np.arange(3))
        rt.process_watermark(released_to)          # releases the row at released_to, drops the older one
        assert rt.stats().late_events == 1 and rt.buffered() == 2
        rt.process_watermark(1 << 62)
        assert rt.buffered() == 0 and rt.stats().late_events == 1
        rt.flush()
        got = engine_rows(rt.collect("O"))
    finally:
        rt.shutdown()
    ev = ro_events(w, [0, 1, 2]) + ro_events(more, [1]) + ro_events(w, [3]) + ro_events(more, [2])
    assert_same_rows(got, oracle_run(RO_PLAN, ev)["O"], "late row below released_max = %d" % released_to)


def test_reorder_snapshot_holds_negative_ts():
    w = ro_stream(n=300, seed=8)
    n = len(w["ts"])
    order = sorted(range(n), key=lambda i: (int(w["ts"][i]), i))
    mark = -(1 << 62)
    rt = fs.SiddhiAppRuntime(RO_PLAN)
    rt.add_callback("O")
    rt2 = None
    try:
        ro_send(rt, w, np.arange(n))
        rt.process_watermark(mark)
        held = int((w["ts"] > mark).sum())
        assert 0 < held < n and rt.buffered() == held and int((w["ts"][w["ts"] > mark] < 0).sum()) > 10
        rt.flush()
        first = engine_rows(rt.collect("O"))
        snap = rt.snapshot()
        rt.shutdown()
        rt2 = fs.SiddhiAppRuntime(RO_PLAN)
        rt2.add_callback("O")
        rt2.restore(snap)
        assert rt2.buffered() == held
        rt2.process_watermark(-1)
        assert rt2.buffered() == int((w["ts"] > -1).sum())
        rt2.process_watermark(1 << 62 | 1)
        assert rt2.buffered() == 0
        rt2.flush()
        second = engine_rows(rt2.collect("O"))
    finally:
        rt.shutdown()
        if rt2 is not None:
            rt2.shutdown()
    assert_same_rows(first + second, oracle_run(RO_PLAN, ro_events(w, order))["O"], "reorder snapshot, negative ts")
