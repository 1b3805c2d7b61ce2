"""CPU: what one TrainStep iteration enqueues, and where, pinned against a recorded table.

The real step() and the real capture code run with recorders in place of the GPU: torch.cuda's graphs, streams and synchronisation,
the collectives, and the TrainStep pieces that enqueue kernels (PIECES, plus the plan's backward / run_late).  For a captured step
(use_graph=True) and an eager one, and every combination of skip_nonfinite, max_grad_norm, a distributed run (one-rank stand-in for
the collectives) and update_interval 1 and 3 -- the latter followed by a flush (last_of_epoch on the first iteration of a window:
the (True, True) variant, captured on demand) -- the table holds

  * graphs: per captured graph, labelled <variant>.<n-th graph of that variant>, the stream it was captured on and its pieces in
    order, each with its bucket key;
  * steps: per step() call its variant and everything it did in order: pieces called eagerly (the warm-up iteration of a capture;
    an eager step) with their stream, graph replays with their stream, wait_stream edges (waiter, waited-on), all_reduce calls with
    what they reduce, GradSync.wait, TrainStep._agree.

tests/trainstep_order.json was recorded at commit 89a78d6 -- before the iteration had one description; there the norm / commit
pieces were spelled _norm_gated, _norm_clip / _commit_gated, _commit_clip in PIECES, the only difference of this file -- with

    python -m tests.test_trainstep_order_cpu > tests/trainstep_order.json

and is never regenerated from the code it checks."""
import contextlib
import itertools
import json
import os

import pytest
import torch
import torch.distributed as dist

from tests.trainstep_stub import stub_model, stub_trainstep

TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "trainstep_order.json")
PIECES = {"_forward_and_loss_partials": "forward", "_loss_backward": "loss_backward", "_optimizer": "optimizer", "_norm": "norm",
          "_commit": "commit"}
CONFIGS = ["%s-skip%d-clip%d-dist%d-k%d" % c for c in itertools.product(("late", "eager"), (0, 1), (0, 1), (0, 1), (1, 3))]


def _key(key):
    return None if key is None else "+".join(key)


class Recorder:
    """State shared by the stand-ins; Stream and CUDAGraph are classes made per recorder, as the trainer constructs them bare."""

    def __init__(self):
        rec = self
        self.log, self.graphs, self.capturing, self.ts = [], {}, None, None

        class Stream:
            count = 0

            def __init__(self):
                self.name = "s%d" % Stream.count if Stream.count else "main"
                Stream.count += 1

            def wait_stream(self, other):
                rec.log.append(["wait", self.name, other.name])

        class CUDAGraph:
            def __init__(self):
                variant = "".join("FT"[bool(f)] for f in (rec.ts._zero, rec.ts._opt))
                self.label = "%s.%d" % (variant, sum(1 for g in rec.graphs if g.startswith(variant)))
                rec.graphs[self.label] = self.record = {"stream": None, "pieces": []}

            def replay(self):
                rec.log.append(["replay", self.label, rec.streams[-1].name])
        self.Stream, self.CUDAGraph = Stream, CUDAGraph
        self.streams = [Stream()]                      # the stack of current streams; [0]: the default stream

    @contextlib.contextmanager
    def on_stream(self, stream):
        self.streams.append(stream if stream is not None else self.streams[-1])
        try:
            yield
        finally:
            self.streams.pop()

    @contextlib.contextmanager
    def capture(self, graph, stream=None):
        with self.on_stream(stream):
            graph.record["stream"] = self.streams[-1].name
            self.capturing = graph
            try:
                yield
            finally:
                self.capturing = None

    def piece(self, name, key=None):
        if self.capturing is not None:
            self.capturing.record["pieces"].append([name, _key(key)])
        else:
            self.log.append(["call", name, _key(key), self.streams[-1].name])

    def all_reduce(self, t, op=dist.ReduceOp.SUM, group=None, async_op=False):
        ts = self.ts
        if t is ts.acc:
            what = "acc"
        elif ts.gate is not None and t.data_ptr() == ts.gate.data_ptr() and t.numel() == 2:
            what = "gate[:2]"
        else:
            what = next("bucket:" + _key(k) for k in ts.sync.ranges
                        if ts.sync.bucket(k).data_ptr() == t.data_ptr() and ts.sync.bucket(k).numel() == t.numel())
        self.log.append(["all_reduce", what, "max" if op == dist.ReduceOp.MAX else "sum", "async" if async_op else "sync"])
        return self                                    # (the work handle of an async call)

    def wait(self):
        pass


@contextlib.contextmanager
def patched(rec):
    names = [(torch.cuda, "CUDAGraph", rec.CUDAGraph), (torch.cuda, "graph", rec.capture), (torch.cuda, "Stream", rec.Stream),
             (torch.cuda, "stream", rec.on_stream), (torch.cuda, "current_stream", lambda: rec.streams[-1]),
             (torch.cuda, "synchronize", lambda: None), (dist, "all_reduce", rec.all_reduce)]
    saved = [(o, n, getattr(o, n)) for o, n, _ in names]
    for o, n, v in names:
        setattr(o, n, v)
    try:
        yield
    finally:
        for o, n, v in saved:
            setattr(o, n, v)


def record(config):
    mode, skip, clip, dist_active, k = config.split("-")
    ts = stub_trainstep(stub_model(), skip=skip == "skip1", clip=1.0 if clip == "clip1" else None, dist_active=dist_active == "dist1",
                        k=int(k[1:]), late=mode == "late")
    rec = Recorder()
    rec.ts = ts
    for attr, name in PIECES.items():
        setattr(ts, attr, lambda key=None, name=name: rec.piece(name, key))
    ts._capture_flags = lambda window: rec.piece("capture_flags:" + ("window" if window else "start"))
    ts.plan.backward = lambda tags=None: rec.piece("backward", tags)
    ts.plan.run_late = lambda key: rec.piece("run_late", key)
    agree, wait = ts._agree, ts.sync.wait
    ts._agree = lambda: (rec.log.append(["agree"]), agree())
    ts.sync.wait = lambda: (rec.log.append(["sync.wait"]), wait())
    steps = []
    with patched(rec):
        # update_interval 1: the capturing step and a plain replay; 3: one window, then a flush on the first iteration of the next
        for last in (False, False) if ts.update_interval == 1 else (False, False, False, True):
            rec.log = []
            ts.step(last_of_epoch=last)
            steps.append({"variant": "".join("FT"[f] for f in (ts._zero, ts._opt)), "events": rec.log})
    return {"graphs": rec.graphs, "steps": steps}


@pytest.mark.parametrize("config", CONFIGS)
def test_iteration_order_matches_the_recorded_table(config):
    with open(TABLE) as f:
        want = json.load(f)
    assert sorted(want) == sorted(CONFIGS)
    got = json.loads(json.dumps(record(config)))
    assert got["graphs"] == want[config]["graphs"]
    for g, w in zip(got["steps"], want[config]["steps"]):
        assert g == w, (config, g["variant"])
    assert len(got["steps"]) == len(want[config]["steps"])


if __name__ == "__main__":
    print(json.dumps({c: record(c) for c in CONFIGS}, indent=1))
