"""bench.py --dump-outputs / --full.

CPU: dump_sample's row order is independent of the order the rows arrive in,
a large output is cut to a seeded sample within the byte budget, write_dump's
files are float64.  GPU: a small config-3 run of bench.main() writes the last
timed step's rows exactly as oracle/cep_oracle.c gives them for that step, two
runs over the same stream write identical files whether all input batches are
resident at once or one at a time (--resident-mb), a plain run carries no
parity / CPU-baseline leg and a --full run carries both.
"""
import json
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

import bench  # noqa: E402


def test_dump_sample_is_sorted_and_order_independent():
    import torch
    rng = np.random.default_rng(1)
    m = 5000
    ts = torch.from_numpy(rng.integers(1_700_000_000_000, 1_700_000_000_050, m))
    k = torch.from_numpy(rng.integers(0, 7, m).astype(np.int32))
    p = torch.from_numpy(rng.random(m))
    rows, n = bench.dump_sample(ts, [k, p], 1 << 20)
    assert n == m and rows.shape == (m, 3) and rows.dtype == np.float64
    want = np.stack([ts.numpy().astype(np.float64), k.numpy().astype(np.float64), p.numpy()], axis=1)
    want = want[np.lexsort((want[:, 2], want[:, 1], want[:, 0]))]
    assert np.array_equal(rows, want)
    perm = torch.from_numpy(rng.permutation(m))
    rows2, _ = bench.dump_sample(ts[perm], [k[perm], p[perm]], 1 << 20)
    assert np.array_equal(rows, rows2)


def test_dump_sample_budget_and_files(tmp_path):
    import torch
    m = 4096
    ts = torch.arange(m, dtype=torch.int64)
    c = torch.arange(m, dtype=torch.int32)
    budget = 100 * 16
    a, n = bench.dump_sample(ts, [c], budget)
    b, _ = bench.dump_sample(ts.flip(0), [c.flip(0)], budget)
    assert n == m and a.shape == (100, 2) and a.nbytes <= budget
    assert np.array_equal(a, b)                      # the same seeded rows every time
    assert (np.diff(a[:, 0]) > 0).all()              # rows of the sorted order, in that order
    e, n0 = bench.dump_sample(ts[:0], [c[:0]], budget)
    assert n0 == 0 and e.shape == (0, 2)
    bench.write_dump(str(tmp_path / "d"), {"O": (a, n), "P": (e, n0)})
    got = np.load(tmp_path / "d" / "O.npy")
    assert got.dtype == np.float64 and np.array_equal(got, a)
    assert np.load(tmp_path / "d" / "P.npy").shape == (0, 2)
    assert np.array_equal(np.load(tmp_path / "d" / "row_counts.npy"), np.array([m, 0], dtype=np.float64))


def _bench_line(monkeypatch, capsys, argv):
    monkeypatch.setattr(sys, "argv", ["bench.py"] + argv)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.delenv("RANK", raising=False)
    monkeypatch.delenv("LOCAL_RANK", raising=False)
    bench.main()
    lines = [l for l in capsys.readouterr().out.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


@pytest.mark.gpu
def test_dump_outputs_last_step_vs_oracle(tmp_path, monkeypatch, capsys):
    import cep_oracle as CO
    n, keys, warm, steps = 1 << 18, 1 << 12, 1, 2
    argv = ["--gpus", "1", "--steps", str(steps), "--warmup", str(warm), "--events", str(n), "--keys", str(keys)]
    plain = _bench_line(monkeypatch, capsys, argv + ["--dump-outputs", str(tmp_path / "a")])
    # 8 MiB of resident input: one 6.25 MiB batch per window, so every step's
    # batch is generated after the step before it has run
    full = _bench_line(monkeypatch, capsys, argv + ["--full", "--resident-mb", "8",
                                                    "--dump-outputs", str(tmp_path / "b")])
    assert plain["steps"] == steps and plain["ms_per_step"] > 0
    assert plain["parity"] is None and plain["cpu_baseline"] is None
    assert full["parity"]["parity"] == "ok" and full["cpu_baseline"]["value"] > 0
    a = np.load(tmp_path / "a" / "O.npy")
    assert a.dtype == np.float64
    assert np.array_equal(a, np.load(tmp_path / "b" / "O.npy"))
    assert np.array_equal(np.load(tmp_path / "a" / "row_counts.npy"), np.load(tmp_path / "b" / "row_counts.npy"))

    # the oracle over the whole stream; the last step's rows are those whose
    # completing event arrived in it
    w = CO.generate(0, (warm + steps) * n, keys, rate=400)
    po = CO.PatternOracle(keys, CO.cond(("price", 0, ">", 0.5)), CO.cond(("id", 7, "==", 0)), every=True, within=10000)
    ia, ib, _ = po.run(w)
    last = ib >= (warm + steps - 1) * n
    ia, ib = ia[last], ib[last]
    want = np.stack([w["ts"][ib], w["k"][ia], w["price"][ia], w["price"][ib], w["ts"][ib]], axis=1).astype(np.float64)
    want = want[np.lexsort(tuple(want[:, c] for c in reversed(range(want.shape[1]))))]
    assert len(want) > 1000
    assert np.load(tmp_path / "a" / "row_counts.npy").tolist() == [float(len(want))]
    assert np.array_equal(a, want)
