"""GPU parity of k_cfpart2 (csrc/cf_kernels.hip): the event-time partition of
local rows without hot-key diversion as two 512-lane workgroups per CU, a
tile's rows taken in two halves of 8 per lane and kept rows parked in an LDS
pending area.  Every output row is compared with the CPU oracle.

Every case runs twice in one process: with the default kernel selection and
with CEP_CF_PART=1, which keeps k_cfpart (the variable is read when a runtime
is created).  kernel_launches[K_CF_PARTITION_2WG] counts the launches that
ran k_cfpart2: > 0 in the first run, 0 in the second.

The sizes sit on the edges of the new kernel: below, at and above one 64-row
load segment, the 4096-row half boundary and the 8192-row tile; batches cut
off the segment grid (the previous-row ts of a half comes from another tile,
chunk or batch); plans with no carried word (NW = 0) and one (config 3);
every column type of the decode; tiles that keep every row, more than the
pending area holds (the redo that stores straight to HBM); the order check at
the first row of a tile's second half; and a diverted Zipf stream and a
ts_order = 0 run, which stay on the unchanged kernels.
"""
import numpy as np
import pytest

from helpers import assert_same_rows, engine_rows, oracle_run, workload_events

pytestmark = pytest.mark.gpu

import flink_siddhi as fs  # noqa: E402
from flink_siddhi import _lib as L  # noqa: E402
from flink_siddhi import workload  # noqa: E402
from test_gpu_cfpart_loads import COLS, TYPED_PLANS, send, typed_stream  # noqa: E402

TILE = 8192
HALF = TILE // 2
LAST = 2 * TILE + 777
SIZES = [1, 63, 64, 65, HALF - 1, HALF, HALF + 1, TILE - 1, TILE, TILE + 1, LAST]
KEYS = {1: 64, 63: 64, 64: 64, 65: 64, HALF - 1: 128, HALF: 128, HALF + 1: 128,
        TILE - 1: 256, TILE: 256, TILE + 1: 512, LAST: 1024}
KERNELS = [("k_cfpart2", None), ("k_cfpart", "1")]   # (name, CEP_CF_PART)

# a select with no captured column: records are one word (NW = 0)
PLAN_NW0 = (workload.PATTERN_PLAN
            .replace("select s1.k as k, s1.price as p1, s2.price as p2, s2.ts as t", "select s1.k as k"))
# predicates that keep every row: every full tile exceeds the pending area
PLAN_KEEP_ALL = (workload.PATTERN_PLAN.replace("price > 0.5", "price > -1.0").replace("id % 7 == 0", "id % 1 == 0"))

_want = {}


def stream_of(n, keys):
    return workload.generate(0, n, keys, rate=2)


def want_rows(plan, n, keys):
    """Oracle rows of `plan` over stream_of(n, keys), computed once."""
    if (plan, n, keys) not in _want:
        _want[(plan, n, keys)] = oracle_run(plan, workload_events(stream_of(n, keys))).get("O", [])
    return _want[(plan, n, keys)]


def both_kernels(monkeypatch, body, expect_2wg=True):
    """body() -> stats, once per kernel; checks which partition ran."""
    for name, env in KERNELS:
        if env is None:
            monkeypatch.delenv("CEP_CF_PART", raising=False)
        else:
            monkeypatch.setenv("CEP_CF_PART", env)
        st = body(name)
        assert st.kernel_launches[L.K_CF_PARTITION] > 0 and st.kernel_launches[L.K_WALK] == 0, name
        if env is None and expect_2wg:
            assert st.kernel_launches[L.K_CF_PARTITION_2WG] > 0, "k_cfpart2 was not selected"
            assert st.kernel_launches[L.K_CF_PARTITION_2WG] <= st.kernel_launches[L.K_CF_PARTITION]
        else:
            assert st.kernel_launches[L.K_CF_PARTITION_2WG] == 0, name


def run(plan, w, cuts, device, **opts):
    rt = fs.SiddhiAppRuntime(plan, **opts)
    rt.add_callback("O")
    for s, e in zip(cuts[:-1], cuts[1:]):
        send(rt, w, s, e, device)
    got = engine_rows(rt.collect("O"))
    st = rt.stats()
    rt.shutdown()
    return got, st


@pytest.mark.parametrize("chunk", [TILE, 2 * TILE])
@pytest.mark.parametrize("plan", [workload.PATTERN_PLAN, PLAN_NW0], ids=["nw1", "nw0"])
def test_batch_sizes(plan, chunk, monkeypatch):
    def body(name):
        tot = None
        for n in SIZES:
            got, st = run(plan, stream_of(n, KEYS[n]), [0, n], False, ts_order=1, chunk_events=chunk)
            assert_same_rows(got, want_rows(plan, n, KEYS[n]), "%s n=%d chunk=%d" % (name, n, chunk))
            if tot is None:
                tot = st
            else:
                for i in range(16):
                    tot.kernel_launches[i] += st.kernel_launches[i]
        return tot
    both_kernels(monkeypatch, body)
    assert len(want_rows(plan, LAST, KEYS[LAST])) > 50


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("chunk", [TILE, 2 * TILE])
def test_three_batches_cut_off_the_segment_grid(chunk, device, monkeypatch):
    w = stream_of(LAST, KEYS[LAST])

    def body(name):
        got, st = run(workload.PATTERN_PLAN, w, [0, TILE + 37, 2 * TILE + 101, LAST], device,
                      ts_order=1, chunk_events=chunk)
        assert_same_rows(got, want_rows(workload.PATTERN_PLAN, LAST, KEYS[LAST]), "%s 3 batches chunk=%d" % (name, chunk))
        return st
    both_kernels(monkeypatch, body)


@pytest.mark.parametrize("which", [0, 1], ids=["int-long-bool", "float-double-bool"])
def test_every_type_arm_decodes(which, monkeypatch):
    n, keys = LAST, 512
    w = typed_stream(n, keys)
    plan = TYPED_PLANS[which]
    names = ("k", "a", "b", "c", "d", "e")
    want = oracle_run(plan, workload_events(w, cols=names)).get("O", [])
    assert len(want) > 100
    if which == 1:   # the engine hands float columns back as float32
        want = [(t, s, (k, float(np.float32(c)), d)) for t, s, (k, c, d) in want]

    def body(name):
        rt = fs.SiddhiAppRuntime(plan, ts_order=1, chunk_events=TILE)
        rt.add_callback("O")
        rt.send("A", w["ts"], [w[c].astype(np.uint8) if c == "e" else w[c] for c in names], streams=w["stream"])
        rt.flush()
        got = engine_rows(rt.collect("O"))
        st = rt.stats()
        rt.shutdown()
        if which == 1:
            got = [(t, s, (k, float(np.float32(c)), d)) for t, s, (k, c, d) in got]
        assert_same_rows(got, want, "%s typed plan %d" % (name, which))
        return st
    both_kernels(monkeypatch, body)


def test_tiles_that_keep_more_than_the_pending_area(monkeypatch):
    # every row is kept: both full tiles overflow (8192 > pending records) and
    # are redone; the ragged one (1 row past the half boundary) keeps 4097
    n, keys = TILE + HALF + 1, 512
    w = stream_of(n, keys)
    want = want_rows(PLAN_KEEP_ALL, n, keys)
    assert len(want) > 1000

    def body(name):
        got, st = run(PLAN_KEEP_ALL, w, [0, n], False, ts_order=1, chunk_events=2 * TILE)
        assert_same_rows(got, want, "%s keep-all" % name)
        return st
    both_kernels(monkeypatch, body)


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_descent_at_the_first_row_of_the_second_half(device, monkeypatch):
    n = 2 * TILE + 777
    w = stream_of(n, 256)
    w["ts"] = w["ts"].copy()
    pos = TILE + HALF   # row 4096 of tile 1
    w["ts"][pos] = w["ts"][pos - 1] - 1

    def body(name):
        rt = fs.SiddhiAppRuntime(workload.PATTERN_PLAN, ts_order=1, chunk_events=2 * TILE)
        rt.add_callback("O")
        with pytest.raises(ValueError, match="event-time order"):
            send(rt, w, 0, n, device)
        st = rt.stats()
        rt.shutdown()
        return st
    both_kernels(monkeypatch, body)


def test_equal_timestamp_at_the_first_row_of_the_second_half(monkeypatch):
    n = 2 * TILE + 777
    w = stream_of(n, 256)
    w["ts"] = w["ts"].copy()
    for pos in (HALF, TILE + HALF):
        w["ts"][pos] = w["ts"][pos - 1]
    want = oracle_run(workload.PATTERN_PLAN, workload_events(w)).get("O", [])

    def body(name):
        got, st = run(workload.PATTERN_PLAN, w, [0, n], True, ts_order=1, chunk_events=2 * TILE)
        assert_same_rows(got, want, "%s equal ts at half starts" % name)
        return st
    both_kernels(monkeypatch, body)


def test_ts_order_0_keeps_its_kernels(monkeypatch):
    n, keys = LAST, KEYS[LAST]
    w = stream_of(n, keys)

    def body(name):
        got, st = run(workload.PATTERN_PLAN, w, [0, n], False, ts_order=0, chunk_events=TILE)
        assert_same_rows(got, want_rows(workload.PATTERN_PLAN, n, keys), "%s ts_order=0" % name)
        return st
    both_kernels(monkeypatch, body, expect_2wg=False)


def test_diverted_zipf_stream_keeps_k_cfpart(monkeypatch):
    # the small skewed setup of test_gpu_cfpart_loads: once keys are hot the
    # partition diverts them (nhot > 0), which k_cfpart2 does not take.  Only
    # the probe chunk, the first of the twelve, runs before any key is hot:
    # it is the one launch without diversion, so the one k_cfpart2 launch
    from test_gpu_geometry import assert_same_per_key
    from test_gpu_hot import oracle_batches, run_batches
    import cep_oracle as CO
    monkeypatch.setenv("CEP_HOT_THRESH", "16")
    monkeypatch.delenv("CEP_CF_PART", raising=False)
    keys, rate, n = 4096, 50, 1 << 16
    z = workload.zipf_map(keys, seed=13)
    batches = [(i * n, n, z) for i in range(3)]
    want, _ = oracle_batches(batches, keys, rate, CO.cond(("id", 7, "==", 0)), 10000)
    got, st = run_batches(batches, keys, rate, workload.PATTERN_PLAN, 2 * TILE)
    assert st.kernel_launches[L.K_HOT] > 0, "hot-key path never engaged"
    assert_same_per_key(got, want)
    assert st.kernel_launches[L.K_CF_PARTITION] == 12
    assert st.kernel_launches[L.K_CF_PARTITION_2WG] == 1   # every diverted launch is k_cfpart's
    assert len(want["k"]) > 5000
