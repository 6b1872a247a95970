"""An explicit model of query chaining (synchronous, depth-first delivery).

A chained plan is given as layers.  Layer 0 holds the `define stream`s of the
outside inputs and the first producers; every later layer is a plan of its
own that `define`s the derived streams it reads (and any outside stream it
reads beside them) followed by its queries.  One source event is pushed
through window_model.WindowModel (siddhi_oracle's instances plus the naive
windows) of every layer that defines its stream; each row a layer emits is
recorded and, before the next source event is looked at, handed on to the
later layers that define its stream, carrying the ts it was emitted with and
the arrival number of the source event.  Nothing else: no inlining, no
views.

Events may name a derived stream directly (rows sent to it from outside):
they enter at the layers that define it, like any other event.
"""
from __future__ import annotations

from typing import Dict, List, Sequence, Tuple

from window_model import WindowModel


class ChainModel:
    def __init__(self, layers: Sequence[str]):
        self.rts = [WindowModel(p) for p in layers]
        self.seq = 0

    def send(self, stream: str, ts: int, row) -> list:
        out: list = []
        seq = self.seq
        self.seq += 1
        self._deliver(0, stream, ts, tuple(row), seq, out)
        return out

    def _deliver(self, first: int, stream: str, ts: int, row, seq: int, out: list):
        for li in range(first, len(self.rts)):
            rt = self.rts[li]
            if stream not in rt.app.streams:
                continue
            rt.seq = seq            # the source row's arrival number
            for ev in rt.send(stream, ts, row):
                out.append(ev)
                self._deliver(li + 1, ev.stream, ev.ts, ev.data, seq, out)

    def max_live(self) -> int:
        return max(rt.max_live() for rt in self.rts)


def chain_run(layers: Sequence[str], events: Sequence[Tuple[str, int, tuple]]):
    """events: [(stream_id, ts, row)] in arrival order ->
    ({stream: [(ts, seq, data)]} for every stream any layer inserts into, largest live count)."""
    m = ChainModel(layers)
    out: Dict[str, List] = {}
    for sid, ts, row in events:
        for ev in m.send(sid, ts, row):
            out.setdefault(ev.stream, []).append((ev.ts, ev.seq, ev.data))
    return out, m.max_live()
