"""Call trace of the Python `split_epoch` loop (vanilla and U-shape, look-ahead and §3.2
overlap order): every call the loop makes on Bob's tail engine, the Alice's front and head
engines, the point-to-point calls of the communicator and `ops.softmax_ce`, in order, with the
shapes of the tensors it passes.  Pins the schedule itself — which call follows which, with
which batch — where tests/test_split_order_cpu.py pins the parameters it produces.

One epoch of 37 samples at B = 16: three batches, the last of 5 rows.  On CPU the tail has no
fused or grouped kernels, so this file pins the unfused branches; tests/test_split_trace_gpu.py
pins the fused and look-ahead ones with the same recorder.

The expected traces are tests/data/split_epoch_trace.json (and split_epoch_trace_gpu.json).
They are regenerated only by hand, from the repository root:

    python -m tests.test_split_trace_cpu          # tests/data/split_epoch_trace.json
    python -m tests.test_split_trace_cpu --gpu    # tests/data/split_epoch_trace_gpu.json
"""
import json
import os

import pytest
import torch

from splitlearning_amd.config import parse_args
from splitlearning_amd.data.mnist import write_shards
from splitlearning_amd.engine.slots import OptSlot
from splitlearning_amd.parallel.dist import Comm, Placement

DATA = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data")
CASES = [(kind, ahead) for kind in ("vanilla", "ushape") for ahead in (True, False)]
N, B = 37, 16
KWARGS = ("train", "pre", "defer", "premasked", "need_dx", "prefix", "mask_input")
COMM = ("multicast", "send_recv", "reduce_to", "reduce_to_async")


def case_id(kind, ahead):
    return f"{kind}-{'lookahead' if ahead else 'overlap'}"


def _session(kind, tmp_path, dev, extra=()):
    from splitlearning_amd.protocols import UShapeSession, VanillaSession
    flags = (["--vanilla"] if kind == "vanilla" else []) + list(extra)
    args = parse_args(flags + ["--world_size", "2", "--seed", "7", "--num_samples", "300", "--no_tqdm",
                               "--batch_size", str(B), "--datapath", str(tmp_path / "d"),
                               "--log_dir", str(tmp_path / "logs")])
    if not (tmp_path / "d").exists():
        write_shards(args, verbose=False)
    cls = VanillaSession if kind == "vanilla" else UShapeSession
    return cls(args, Comm(0, 1, dev, Placement.make(2, 1, 1)), dev)


def _public_methods(obj):
    for name in dir(type(obj)):
        if not name.startswith("_") and not isinstance(getattr(type(obj), name), property) \
                and callable(getattr(obj, name)):
            yield name


def record_trace(kind, ahead, tmp_path, dev, extra=()):
    """The calls of one `split_epoch(1, order, 37)` as [name, args, kwargs] entries: a tensor is
    its shape, None stays None, an OptSlot is "alice" or "bob", every other positional argument
    is left out; of the keyword arguments the tensors, Nones and slots, and the flags in KWARGS."""
    sess = _session(kind, tmp_path, dev, extra)
    sess.split_lookahead = lambda cid: ahead
    a = sess.alices[1]
    trace = []

    def enc(v):
        if isinstance(v, torch.Tensor):
            return list(v.shape)
        return "alice" if v is a.slot else "bob"

    def seen(v):
        return v is None or isinstance(v, (torch.Tensor, OptSlot))

    def proxy(label, fn):
        def call(*args, **kw):
            trace.append([label, [v if v is None else enc(v) for v in args if seen(v)],
                          {k: (enc(v) if seen(v) and v is not None else v) for k, v in sorted(kw.items())
                           if seen(v) or k in KWARGS}])
            return fn(*args, **kw)
        return call

    targets = [("tail", sess.tail, None), ("front", a.front, None), ("comm", sess.comm, COMM),
               ("ops", sess.ops, ("softmax_ce",))]
    if a.head is not None:
        targets.append(("head", a.head, None))
    order = a.train.shuffled_order(torch.Generator().manual_seed(4))[:N].to(dev)
    with pytest.MonkeyPatch.context() as mp:       # undone on exit: `sess.ops` outlives the session
        for label, obj, names in targets:
            for name in (names or _public_methods(obj)):
                mp.setattr(obj, name, proxy(f"{label}.{name}", getattr(obj, name)))
        sess.split_epoch(1, order, N)
    return trace


@pytest.mark.parametrize("kind,ahead", CASES)
def test_split_epoch_call_trace(kind, ahead, tmp_path):
    with open(os.path.join(DATA, "split_epoch_trace.json")) as f:
        want = json.load(f)[case_id(kind, ahead)]
    got = json.loads(json.dumps(record_trace(kind, ahead, tmp_path, torch.device("cpu"))))
    assert len(got) > 20
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, (i, g, w)
    assert len(got) == len(want)


if __name__ == "__main__":
    import pathlib
    import sys
    import tempfile
    gpu = "--gpu" in sys.argv[1:]
    if gpu:
        from splitlearning_amd import _native
        _native.load()
    dev = torch.device("cuda", 0) if gpu else torch.device("cpu")
    extra = ("--python_epoch", "--split_persist", "off") if gpu else ()
    out = {}
    for kind, ahead in CASES:
        with tempfile.TemporaryDirectory() as d:
            out[case_id(kind, ahead)] = record_trace(kind, ahead, pathlib.Path(d), dev, extra)
    path = os.path.join(DATA, "split_epoch_trace_gpu.json" if gpu else "split_epoch_trace.json")
    with open(path, "w") as f:
        f.write("{\n" + ",\n".join(f' "{k}": [\n' + ",\n".join("  " + json.dumps(e) for e in v) + "\n ]"
                                    for k, v in out.items()) + "\n}\n")
    print(path, {k: len(v) for k, v in out.items()})
