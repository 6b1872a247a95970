"""GPU parity of k_cfpart's two load paths (csrc/dev_common.h): a full tile
issues every column load of its rows, and the ts of the row before them, as
one group (cf_load_cols_full); a ragged last tile keeps the conditional loads
(cf_load_cols).  Every row is compared with the CPU oracle.

The sizes sit on the edges between the two: batches below, at and just above
one 8192-row tile, chunks that start at row0 > 0 and end in a ragged tile,
batches cut at rows that are no multiple of the 64-row load segment (the
previous-row ts crosses tiles, chunks and batches), device batches whose `ts`
attribute is the event-ts buffer (its prefetch slot is dropped: one carried
word) and host batches where it is not (two), every column type of the
decode, the order check at each place the previous row comes from, and a
skewed stream with hot-key diversion on (grouped hot_id lookups).

The closed form prefetches at most four columns (kPref), the key included,
so the int / long / float / double / bool predicates are spread over two
plans with a `long` key rather than one.
"""
import numpy as np
import pytest

from helpers import assert_same_rows, engine_rows, oracle_run, workload_events

pytestmark = pytest.mark.gpu

import flink_siddhi as fs  # noqa: E402
from flink_siddhi import _lib as L  # noqa: E402
from flink_siddhi import workload  # noqa: E402

TILE = 8192
SIZES = [1, 63, 64, 65, TILE - 1, TILE, TILE + 1, 2 * TILE + 777]
KEYS = {1: 64, 63: 64, 64: 64, 65: 64, TILE - 1: 256, TILE: 256, TILE + 1: 512, 2 * TILE + 777: 1024}
COLS = ("k", "ts", "id", "price", "stream")

_want = {}


def stream_of(n, keys):
    return workload.generate(0, n, keys, rate=2)


def want_rows(n, keys):
    """Oracle rows of the config-3 plan over stream_of(n, keys), computed once."""
    if (n, keys) not in _want:
        _want[(n, keys)] = oracle_run(workload.PATTERN_PLAN, workload_events(stream_of(n, keys))).get("O", [])
    return _want[(n, keys)]


def send(rt, w, s, e, device):
    cols = {c: np.ascontiguousarray(w[c][s:e]) for c in COLS}
    if device:
        import torch
        cols = {c: torch.from_numpy(v).cuda() for c, v in cols.items()}
    rt.send("A", cols["ts"], [cols["k"], cols["ts"], cols["id"], cols["price"]], streams=cols["stream"])
    rt.flush()


def run(plan, w, cuts, device, **opts):
    rt = fs.SiddhiAppRuntime(plan, **opts)
    rt.add_callback("O")
    for s, e in zip(cuts[:-1], cuts[1:]):
        send(rt, w, s, e, device)
    got = engine_rows(rt.collect("O"))
    st = rt.stats()
    rt.shutdown()
    assert st.kernel_launches[L.K_CF_PARTITION] > 0 and st.kernel_launches[L.K_WALK] == 0
    return got


@pytest.mark.parametrize("ts_order", [1, 0])
@pytest.mark.parametrize("chunk", [TILE, 2 * TILE])
def test_batch_sizes(chunk, ts_order):
    for n in SIZES:
        w = stream_of(n, KEYS[n])
        got = run(workload.PATTERN_PLAN, w, [0, n], False, ts_order=ts_order, chunk_events=chunk)
        assert_same_rows(got, want_rows(n, KEYS[n]), "n=%d chunk=%d ts_order=%d" % (n, chunk, ts_order))
    assert len(want_rows(SIZES[-1], KEYS[SIZES[-1]])) > 50


@pytest.mark.parametrize("ts_order", [1, 0])
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("chunk", [TILE, 2 * TILE])
def test_three_batches_cut_off_the_segment_grid(chunk, device, ts_order):
    # cuts at rows that are no multiple of 64: the row before a lane's first
    # row lies in another tile, another chunk or the batch before
    n = SIZES[-1]
    w = stream_of(n, KEYS[n])
    got = run(workload.PATTERN_PLAN, w, [0, TILE + 37, 2 * TILE + 101, n], device,
              ts_order=ts_order, chunk_events=chunk)
    assert_same_rows(got, want_rows(n, KEYS[n]), "3 batches chunk=%d" % chunk)


TYPED = ("define stream A (k long, a int, b long, c float, d double, e bool);"
         "define stream B (k long, a int, b long, c float, d double, e bool);"
         "partition with (k of A, k of B) begin "
         "from every s1=A[%s] -> s2=B[%s] within 1 sec "
         "select s1.k as k, %s insert into O; end;")
TYPED_PLANS = [
    # key long + int, long, bool
    TYPED % ("a % 3 == 0 and b > 100", "e", "s1.a as a1, s2.b as b2"),
    # key long + float, double, bool
    TYPED % ("c < 0.25 and d < 0.75", "e", "s1.c as c1, s2.d as d2"),
]


def typed_stream(n, keys):
    base = workload.generate(0, n, keys, rate=2)
    rng = np.random.default_rng(5)
    return {"ts": base["ts"], "stream": base["stream"],
            "k": base["k"].astype(np.int64),
            "a": rng.integers(-1000, 1000, n).astype(np.int32),
            "b": rng.integers(-1000, 1000, n).astype(np.int64) * (1 << 33),   # needs its high word
            "c": rng.standard_normal(n).astype(np.float32),
            "d": rng.random(n),
            "e": rng.random(n) < 0.3}


@pytest.mark.parametrize("ts_order", [1, 0])
@pytest.mark.parametrize("which", [0, 1], ids=["int-long-bool", "float-double-bool"])
def test_every_type_arm_decodes(which, ts_order):
    n, keys = 2 * TILE + 777, 512
    w = typed_stream(n, keys)
    plan = TYPED_PLANS[which]
    names = ("k", "a", "b", "c", "d", "e")
    ev = workload_events(w, cols=names)
    want = oracle_run(plan, ev).get("O", [])
    assert len(want) > 100
    rt = fs.SiddhiAppRuntime(plan, ts_order=ts_order, chunk_events=TILE)
    rt.add_callback("O")
    rt.send("A", w["ts"], [w[c].astype(np.uint8) if c == "e" else w[c] for c in names], streams=w["stream"])
    rt.flush()
    got = engine_rows(rt.collect("O"))
    st = rt.stats()
    rt.shutdown()
    assert st.kernel_launches[L.K_CF_PARTITION] > 0 and st.kernel_launches[L.K_WALK] == 0
    if which == 1:   # the engine hands float columns back as float32
        want = [(t, s, (k, float(np.float32(c)), d)) for t, s, (k, c, d) in want]
        got = [(t, s, (k, float(np.float32(c)), d)) for t, s, (k, c, d) in got]
    assert_same_rows(got, want, "typed plan %d ts_order=%d" % (which, ts_order))


N_DESC = 4 * TILE + 777
DESCENTS = {
    "tile-first-row": (TILE, None),            # tile 1 of chunk 0: the row before is in tile 0
    "chunk-first-row": (2 * TILE, None),       # chunk 1: the row before is in chunk 0
    "second-batch-first-row": (20000, 20000),  # the row before is the batch before's last
    "ragged-last-tile": (4 * TILE + 300, None),
}


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("where", list(DESCENTS))
def test_one_descending_timestamp_is_reported(where, device):
    pos, cut = DESCENTS[where]
    w = stream_of(N_DESC, 256)
    w["ts"] = w["ts"].copy()
    w["ts"][pos] = w["ts"][pos - 1] - 1
    rt = fs.SiddhiAppRuntime(workload.PATTERN_PLAN, ts_order=1, chunk_events=2 * TILE)
    rt.add_callback("O")
    cuts = [0, N_DESC] if cut is None else [0, cut, N_DESC]
    with pytest.raises(ValueError, match="event-time order"):
        for s, e in zip(cuts[:-1], cuts[1:]):
            send(rt, w, s, e, device)
    rt.shutdown()


def test_equal_timestamps_across_tiles_are_in_order():
    # the check is `<`: a row equal to the one before it, at the first row of
    # a tile and of a chunk, is in order
    w = stream_of(N_DESC, 256)
    w["ts"] = w["ts"].copy()
    for pos in (TILE, 2 * TILE):
        w["ts"][pos] = w["ts"][pos - 1]
    want = oracle_run(workload.PATTERN_PLAN, workload_events(w)).get("O", [])
    got = run(workload.PATTERN_PLAN, w, [0, N_DESC], True, ts_order=1, chunk_events=2 * TILE)
    assert_same_rows(got, want, "equal ts at tile / chunk starts")


def test_diversion_on_a_small_skewed_stream(monkeypatch):
    # Zipf keys, 16 Ki-row chunks, keys with >= 16 records per chunk hot: the
    # first chunk probes, the later ones divert (hot_id looked up per row)
    from test_gpu_geometry import assert_same_per_key
    from test_gpu_hot import oracle_batches, run_batches
    import cep_oracle as CO
    monkeypatch.setenv("CEP_HOT_THRESH", "16")
    keys, rate, n = 4096, 50, 1 << 16
    z = workload.zipf_map(keys, seed=13)
    batches = [(i * n, n, z) for i in range(3)]
    got, st = run_batches(batches, keys, rate, workload.PATTERN_PLAN, 2 * TILE)
    want, _ = oracle_batches(batches, keys, rate, CO.cond(("id", 7, "==", 0)), 10000)
    assert st.kernel_launches[L.K_HOT] > 0, "hot-key path never engaged"
    assert st.kernel_launches[L.K_CF_WALK] > 0
    assert_same_per_key(got, want)
    assert len(want["k"]) > 5000
