"""A runtime owns what it allocates: destroying an app, or a creation that
fails after allocations have begun, gives every byte of device memory back.

For one app of each runtime kind: create, send one 4096-row batch, flush,
destroy.  One cycle warms the HIP runtime; the free device memory is then read
with and without a live app (the difference is the app's footprint), and after
50 more cycles it must be no lower than the warm reading minus one footprint:
a leak of one app's worth spread over the 50 cycles fails.
"""
import os
import subprocess
import sys

import pytest
import torch

import flink_siddhi as fs
from flink_siddhi import workload
import snapshot_cases as SC

pytestmark = pytest.mark.gpu

CYCLES = 50
LONG_PLAN = workload.PATTERN_PLAN.replace("(k int,", "(k long,")
CHAIN = (SC.EV2 + "define stream M (k int, ts long, id int, p2 double);"
         "from A[price > 0.1] select k, ts, id, price * 2.0 as p2 insert into M;"
         "from M[id > 4] select k, sum(p2) as s, count() as c group by k having s > 3.0 insert into O;")
# kind -> (plan, options, outputs, rows through the reorder buffer)
APPS = {
    "filter": (SC.EV2 + "from A[price > 0.5 and id % 7 == 0] select k, id, price insert into O;", {}, ["O"], False),
    # closed form, hot-key candidates and the sparse key map; event time: the reorder buffers exist
    "closed_form_sparse_hot": (LONG_PLAN, dict(ts_order=1, sparse_keys=1, key_capacity=4096), ["O"], True),
    "group": (SC.MQ4, dict(key_capacity=4096), ["Seq0", "Agg0"], False),
    "window": (SC.CASES["win_time"]["plan"], dict(key_capacity=4096, pending_slots=32), ["O"], True),
    "join": (SC.CASES["join"]["plan"], dict(ts_order=1), ["O"], False),
    "table": (SC.EV2 + SC.TABLE, dict(key_capacity=4096), ["O"], False),
    "chain_view": (CHAIN, dict(key_capacity=4096), ["O"], False),
}
_W = {}


def rows():
    if not _W:
        _W.update(workload.generate(0, 4096, 1000, rate=1))
    return _W


def create(kind):
    plan, opts, outs, _ = APPS[kind]
    rt = fs.SiddhiAppRuntime(plan, **opts)
    for o in outs:
        rt.add_callback(o)
    return rt


def cycle(kind):
    """create, one batch, flush, destroy -> the free device memory while the app was alive."""
    w = rows()
    rt = create(kind)
    cols = [w["k"].astype("int64") if "k long" in APPS[kind][0] else w["k"], w["ts"], w["id"], w["price"]]
    if APPS[kind][3]:
        rt.process_elements("A", w["ts"], cols, streams=w["stream"])
        rt.process_watermark(int(w["ts"][-100]))
    else:
        rt.send("A", w["ts"], cols, streams=w["stream"])
    rt.flush()
    for o in APPS[kind][2]:
        rt.collect(o)
    alive = torch.cuda.mem_get_info()[0]
    rt.shutdown()
    return alive


def free_now():
    torch.cuda.synchronize()
    return torch.cuda.mem_get_info()[0]


@pytest.mark.parametrize("kind", list(APPS))
def test_destroy_returns_all_device_memory(kind):
    cycle(kind)                      # warm: code objects, the runtime's own pools
    warm = free_now()
    footprint = warm - cycle(kind)
    assert footprint > 0, "a live app must hold device memory"
    for _ in range(CYCLES):
        cycle(kind)
    after = free_now()
    print("%s: footprint %d bytes, free %d -> %d" % (kind, footprint, warm, after))
    assert after >= warm - footprint, "%d bytes lost over %d cycles (one app: %d)" % (warm - after, CYCLES, footprint)


def test_failed_creation_returns_all_device_memory():
    # refused late and cleanly: sparse_keys on a sharded runtime is rejected
    # after the pattern's state, arenas, pending pools and hot-key lists are
    # allocated.  The footprint is the same app's without the shard option.
    plan, opts, _, _ = APPS["closed_form_sparse_hot"]

    def refused():
        with pytest.raises(fs.SiddhiError, match="sparse_keys needs"):
            fs.SiddhiAppRuntime(plan, key_stride=2, **opts)

    cycle("closed_form_sparse_hot")
    refused()
    warm = free_now()
    footprint = warm - cycle("closed_form_sparse_hot")
    assert footprint > 0
    for _ in range(CYCLES):
        refused()
    after = free_now()
    print("failed creation: footprint %d bytes, free %d -> %d" % (footprint, warm, after))
    assert after >= warm - footprint, "%d bytes lost over %d failed creations" % (warm - after, CYCLES)


def test_stamp_diagnostics_buffer_is_freed_and_the_process_exits_cleanly():
    # CEP_STAMPS=1 is read at creation: a child process with the variable set
    code = ("import sys; sys.path[:0] = %r\n"
            "import test_gpu_lifecycle as T\n"
            "for _ in range(3): T.cycle('closed_form_sparse_hot')\n"
            "T.cycle('group')\n" % [p for p in sys.path if p])
    env = dict(os.environ, CEP_STAMPS="1")
    run = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr[-3000:]
    assert "[cep stamps]" in run.stderr
