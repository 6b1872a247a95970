"""Event tables on the device (tab_kernels.hip) against the naive table model
(tests/table_model.py): the same output rows, bit for bit and in the same
order, the same table contents and the same number of dropped inserts.  Every
value is copied or computed by one interpreter program per row, so there is
no tolerance to choose."""
import numpy as np
import pytest

import flink_siddhi as fs
from flink_siddhi import _lib as L
from flink_siddhi import workload
from helpers import assert_same_rows, engine_rows, workload_events
from table_model import model_run
import table_kats as K

pytestmark = pytest.mark.gpu

EV2 = ("define stream A (k int, ts long, id int, price double);"
       "define stream B (k int, ts long, id int, price double);"
       "@PrimaryKey('k') define table T (k int, id int, price double);")
# stream A writes, stream B reads
INSERT = "from A[price > 0.5] select k, id, price insert into T;"
DELETE = "from A[price < 0.1] select k delete T on T.k == k;"
# no interpreter in the walk: the key equality alone, plain items of either row
PLAIN = (INSERT + DELETE + "from B as b join T as t on b.k == t.k "
         "select b.k as k, b.id as bid, t.id as tid, t.price as tp insert into O;")
# the interpreter build: a further `on` conjunct and a computed item
VM = ("from A[id % 3 == 0] select k, id, price update or insert into T on T.k == k;"
      "from T as t join B as b on b.k == t.k and b.price > t.price "
      "select b.k as k, b.price - t.price as d, t.id + b.id as n insert into O;")
IN = (INSERT + DELETE + "from B[id > 5 and (T.k == k) in T] select k, id insert into O;"
      "from B[not ((T.k == k) in T)] select k, price insert into N;")
UPDATE = (INSERT + "from A[id == 7] select k, price update T set T.price = price on T.k == k;"
          "from B as b join T as t on b.k == t.k select b.id as bid, t.id as tid, t.price as tp insert into O;")
# 512 keys in 8 buckets of 64; chunks of 4096 rows: 5 chunks per 20 000 rows
GEOM = dict(key_capacity=512, buckets_log2=3, chunk_events=4096)

_W = {}
_MODEL = {}


def gen(n, keys):
    if (n, keys) not in _W:
        _W[(n, keys)] = workload.generate(0, n, keys, rate=1)
    return _W[(n, keys)]


def model(plan, wkey):
    """Reference rows and the model (table contents, dropped inserts), once per (plan, input)."""
    if (plan, wkey) not in _MODEL:
        _MODEL[(plan, wkey)] = model_run(plan, workload_events(gen(*wkey)))
    return _MODEL[(plan, wkey)]


def cols(w, s, e):
    return [w["k"][s:e], w["ts"][s:e], w["id"][s:e], w["price"][s:e]]


def run(plan, w, batches=1, outs=("O",), after_batch=None, rt=None, first=0, device=False, **opts):
    """-> ({out: rows}, table rows, stats); batches [first, batches) of the input."""
    rt = rt or fs.SiddhiAppRuntime(plan, **opts)
    for o in outs:
        rt.add_callback(o)
    n = len(w["ts"])
    cuts = np.linspace(0, n, batches + 1).astype(int)
    for i, (s, e) in enumerate(zip(cuts[:-1], cuts[1:])):
        if i < first:
            continue
        c, ts, st = cols(w, s, e), w["ts"][s:e], w["stream"][s:e]
        if device:
            import torch
            c = [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in c]
            ts, st = c[1], torch.from_numpy(np.ascontiguousarray(st)).cuda()
        rt.send("A", ts, c, streams=st)
        rt.flush()
        if after_batch is not None and after_batch(rt, i) is False:
            break
    got = {o: engine_rows(rt.collect(o)) for o in outs}
    rows, st = rt.table_rows("T"), rt.stats()
    rt.shutdown()
    return got, rows, st


def check(plan, wkey, got, rows, st, outs, vm, min_rows, drops):
    want, m = model(plan, wkey)
    # the shape exercises the feature (checked on the CPU, from the model alone)
    for o in outs:
        assert len(want.get(o, [])) >= min_rows, (o, len(want.get(o, [])))
    assert len(m.table_rows("T")) >= 100 or wkey[1] < 100
    assert (m.dropped() >= 1) == drops
    for o in outs:
        assert_same_rows(got[o], want.get(o, []), o)
    assert rows == m.table_rows("T")
    assert st.table_dropped == m.dropped()
    assert st.kernel_launches[L.K_TABLE] > 0
    assert (st.table_vm_launches > 0) == vm
    if vm:
        assert st.table_vm_launches == st.kernel_launches[L.K_TABLE]


CASES = {"plain": (PLAIN, ("O",), False, 2000, True), "vm": (VM, ("O",), True, 1000, False),
         "in": (IN, ("O", "N"), False, 500, True), "update_set": (UPDATE, ("O",), False, 2000, True)}


# ------------------------------------------------------------------- small --
def run_kat(plan, events, outs, **opts):
    rt = fs.SiddhiAppRuntime(plan, key_capacity=64, **opts)
    for o in outs:
        rt.add_callback(o)
    h = {s: rt.input_handle(s) for s in ("U", "S")}
    ts = np.array([e[1] for e in events], np.int64)
    c = [np.array([e[2][i] for e in events], np.int32) for i in range(len(events[0][2]))]
    rt.send("U", ts, c, streams=np.array([h[e[0]] for e in events], np.uint8))
    rt.flush()
    got = {o: engine_rows(rt.collect(o)) for o in outs}
    rows, st = rt.table_rows("T"), rt.stats()
    rt.shutdown()
    return got, rows, st


@pytest.mark.parametrize("name", sorted(K.KATS))
def test_kats(name):
    plan, events, rows, tables, dropped = K.KATS[name]
    got, trows, st = run_kat(plan, events, sorted(rows))
    assert got == rows
    assert trows == tables["T"]
    assert st.table_dropped == dropped
    assert st.kernel_launches[L.K_TABLE] == 1 and st.table_vm_launches == 0


# --------------------------------------------------------------- generated --
@pytest.mark.parametrize("batches", [1, 3])
@pytest.mark.parametrize("name", sorted(CASES))
def test_generated(name, batches):
    plan, outs, vm, min_rows, drops = CASES[name]
    wkey = (20000, 512)
    got, rows, st = run(EV2 + plan, gen(*wkey), batches=batches, outs=outs, **GEOM)
    check(EV2 + plan, wkey, got, rows, st, outs, vm, min_rows, drops)
    assert st.kernel_launches[L.K_TABLE] >= 5      # several chunks


@pytest.mark.parametrize("name", ["plain", "vm"])
def test_a_key_run_spans_lds_windows(name):
    # 4 keys in 2 buckets, one chunk: 10 000 records per bucket, 2048 per LDS
    # window, so a key's row is handed from window to window through its state
    plan, outs, vm, _, drops = CASES[name]
    wkey = (20000, 4)
    got, rows, st = run(EV2 + plan, gen(*wkey), outs=outs, key_capacity=4, buckets_log2=1, chunk_events=32768)
    check(EV2 + plan, wkey, got, rows, st, outs, vm, 2000, drops)
    assert st.kernel_launches[L.K_TABLE] == 1


def test_device_input_and_default_geometry():
    wkey = (20000, 512)
    got, rows, st = run(EV2 + PLAIN, gen(*wkey), batches=2, device=True)
    check(EV2 + PLAIN, wkey, got, rows, st, ("O",), False, 2000, True)


def test_ordered_output_with_a_filter_query_on_the_same_stream():
    # rows of one arrival come in plan order: the filter query's row before
    # (F1) or after (F2) the join's
    f1 = "from B[id == 7] select k, id as bid, id as tid, price as tp insert into O;"
    f2 = "from B[id == 9] select k, id as bid, k as tid, price as tp insert into O;"
    plan = EV2 + f1 + PLAIN + f2
    wkey = (20000, 512)
    want, _ = model(plan, wkey)
    both = [r for r in want["O"] if r[2][1] in (7, 9)]
    assert len(want["O"]) >= 2000 and len(both) >= 200
    got, rows, st = run(plan, gen(*wkey), batches=3, ordered_output=1, **GEOM)
    assert_same_rows(got["O"], want["O"], "ordered")


def test_unordered_output_without_arrival_numbers():
    wkey = (20000, 512)
    want, m = model(EV2 + VM, wkey)
    rt = fs.SiddhiAppRuntime(EV2 + VM, ordered_output=0, omit_seq=1, **GEOM)
    rt.add_callback("O")
    w = gen(*wkey)
    rt.send("A", w["ts"], cols(w, 0, len(w["ts"])), streams=w["stream"])
    rt.flush()
    out = rt.collect("O")
    assert len(out.seq) == 0
    got = sorted(zip(out.ts.tolist(), *[c.tolist() for c in out.cols]))
    assert got == sorted((ts,) + data for ts, _, data in want["O"])
    assert rt.table_rows("T") == m.table_rows("T")
    rt.shutdown()


def test_two_shards_equal_one():
    # key_stride = 2: each shard gets the rows of the keys it owns (the
    # operator routes by cep_plan_partition_keys) and holds their table rows
    wkey = (20000, 512)
    w = gen(*wkey)
    want, m = model(EV2 + PLAIN, wkey)
    merged, trows = [], []
    for r in range(2):
        idx = np.nonzero(w["k"] % 2 == r)[0]
        part = {c: np.ascontiguousarray(v[idx]) for c, v in w.items()}
        got, rows, st = run(EV2 + PLAIN, part, batches=2, key_stride=2, key_offset=r, **GEOM)
        assert st.kernel_launches[L.K_TABLE] > 0 and len(rows) >= 50
        assert all(row[0] % 2 == r for row in rows)
        # shard-local arrival numbers -> the batch's
        merged += [(ts, int(idx[seq]), data) for ts, seq, data in got["O"]]
        trows += rows
    merged.sort(key=lambda x: x[1])
    assert_same_rows(merged, want["O"], "two shards")
    assert sorted(trows) == m.table_rows("T")


def test_snapshot_restore_continues_the_run():
    wkey = (20000, 512)
    plan = EV2 + VM
    want, m = model(plan, wkey)
    snap = []

    def take(rt, i):
        snap.append(rt.snapshot())
        return False

    first, _, _ = run(plan, gen(*wkey), batches=3, after_batch=take, **GEOM)
    rt = fs.SiddhiAppRuntime(plan, **GEOM)
    rt.restore(snap[0])
    rest, rows, st = run(plan, gen(*wkey), batches=3, rt=rt, first=1)
    assert len(first["O"]) >= 100 and len(rest["O"]) >= 100
    assert_same_rows(first["O"] + rest["O"], want["O"], "restored")
    assert rows == m.table_rows("T")
    # another table definition: another plan's snapshot
    other = EV2.replace("define table T (k int, id int, price double)", "define table T (k int, id long, price double)")
    other += ("from A[id % 3 == 0] select k, ts as id, price update or insert into T on T.k == k;"
              "from T as t join B as b on b.k == t.k and b.price > t.price "
              "select b.k as k, b.price - t.price as d, t.id + b.id as n insert into O;")
    rt2 = fs.SiddhiAppRuntime(other, **GEOM)
    with pytest.raises(fs.CepStateError):
        rt2.restore(snap[0])
    rt2.shutdown()


def test_dropped_inserts_survive_a_snapshot():
    plan, events, _, _, dropped = K.KATS["insert_delete"]
    assert dropped == 1
    rt = fs.SiddhiAppRuntime(plan, key_capacity=64)
    h = {s: rt.input_handle(s) for s in ("U", "S")}
    ts = np.array([e[1] for e in events], np.int64)
    c = [np.array([e[2][i] for e in events], np.int32) for i in range(2)]
    rt.send("U", ts, c, streams=np.array([h[e[0]] for e in events], np.uint8))
    rt.flush()
    snap = rt.snapshot()
    rt.shutdown()
    rt = fs.SiddhiAppRuntime(plan, key_capacity=64)
    rt.restore(snap)
    assert rt.table_rows("T") == [(1, 12)] and rt.stats().table_dropped == 1
    rt.shutdown()


# ---------------------------------------------------------------- refusals --
def test_refusals_at_create_and_at_the_call():
    import torch
    with pytest.raises(fs.UnsupportedPlanException, match="table"):
        fs.SiddhiAppRuntime(EV2 + PLAIN, sparse_keys=1)
    rt = fs.SiddhiAppRuntime(EV2 + PLAIN, **GEOM)
    with pytest.raises(fs.UndefinedStreamException):
        rt.add_callback("T")
    w = gen(20000, 512)
    d = [torch.from_numpy(np.ascontiguousarray(x[:64])).cuda() for x in cols(w, 0, 64)]
    for call in (rt.record_words, rt.row_words,
                 lambda: rt.route_rows("A", d[1], d, 2, 0), lambda: rt.route("A", d[1], d, 2, 0)):
        with pytest.raises(fs.UnsupportedPlanException, match="table"):
            call()
    with pytest.raises(fs.UndefinedStreamException):
        rt.table_rows("O")
    assert rt.table_rows("T") == []
    rt.shutdown()


def test_a_key_out_of_range_fails_the_flush_as_for_partition_keys():
    rt = fs.SiddhiAppRuntime(EV2 + PLAIN, key_capacity=16)
    w = gen(20000, 512)
    rt.send("A", w["ts"][:256], cols(w, 0, 256), streams=w["stream"][:256])
    with pytest.raises(fs.CepCapacityError):
        rt.flush()
    rt.shutdown()
