"""One optimizer step over a whole model's parameters: FusedAdam / FusedSGD (one launch,
csrc/optim.hip) against a loop of hip_ops.apply_update_ (one scalar launch per tensor, the
path before them) and torch.optim with foreach=True and, where this torch build has it,
fused=True; gradient-norm clipping on and off.

    python scripts/optim_bench.py [--rounds 9] [--iters 20] [--limit_s 120]

Shapes: model2_sisa's six parameter tensors (32.1 M elements) and the U-shape model2's four
(5.5 M).  Every candidate owns its parameters, gradients and state; the candidates of a shape
are timed in interleaved rounds (device events around `iters` steps) and the median round is
reported, with the bytes the algorithm has to move (Adam 28 B, SGD with momentum 20 B per
parameter; the norm's extra 4 B read is not counted, so a clipped row shows the price of the
clip).  One process; each shape runs under its own time limit (--limit_s) and the process
ends there if the limit passes.
"""
import argparse
import faulthandler
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from splitlearning_amd.config import OptimCfg  # noqa: E402
from splitlearning_amd.ops import hip_ops  # noqa: E402
from splitlearning_amd.optim import FusedAdam, FusedSGD  # noqa: E402

SHAPES = {
    "model2_sisa": [(5000, 5408), (5000,), (1000, 5000), (1000,), (100, 1000), (100,)],
    "model2 (U-shape)": [(1000, 5408), (1000,), (100, 1000), (100,)],
}
LR, WD, MOM, CLIP = 1e-4, 1e-5, 0.9, 1.0
BYTES = {"adam": 28, "sgd": 20}


def _params(dev, shapes, seed=0):
    g = torch.Generator().manual_seed(seed)
    ps = [torch.nn.Parameter((torch.randn(s, generator=g) * 0.05).to(dev)) for s in shapes]
    for p in ps:
        p.grad = (torch.randn(p.shape, generator=g) * 0.01).to(dev)
    return ps


def _torch_opt(kind, ps, **kw):
    if kind == "adam":
        return torch.optim.Adam(ps, lr=LR, weight_decay=WD, **kw)
    return torch.optim.SGD(ps, lr=LR, momentum=MOM, weight_decay=WD, **kw)


def _loop_step(kind, ps):
    """Today's path: one opt_flat launch per tensor."""
    cfg = OptimCfg(kind, LR, weight_decay=WD, momentum=MOM if kind == "sgd" else 0.0)
    sts = [({"m": torch.zeros_like(p), "v": torch.zeros_like(p)} if kind == "adam" else {"buf": torch.zeros_like(p)})
           for p in ps]
    t = [0]

    def step():
        t[0] += 1
        for p, st in zip(ps, sts):
            hip_ops.apply_update_(p, p.grad, st, cfg, t[0])
    return step


def candidates(dev, shapes, kind):
    """[(label, step function)]; a candidate this torch build cannot construct or run is
    reported as unavailable, not replaced."""
    out, skipped = [], []
    fused_cls = FusedAdam if kind == "adam" else FusedSGD
    fkw = {"weight_decay": WD} if kind == "adam" else {"weight_decay": WD, "momentum": MOM}
    out.append((f"Fused{kind.upper() if kind == 'sgd' else 'Adam'}", fused_cls(_params(dev, shapes), lr=LR, **fkw).step))
    out.append((f"  + max_grad_norm={CLIP}", fused_cls(_params(dev, shapes), lr=LR, max_grad_norm=CLIP, **fkw).step))
    out.append(("loop of hip_ops.apply_update_", _loop_step(kind, _params(dev, shapes))))
    for label, kw in (("foreach=True", {"foreach": True}), ("fused=True", {"fused": True})):
        name = f"torch.optim.{'Adam' if kind == 'adam' else 'SGD'}({label})"
        try:
            ps = _params(dev, shapes)
            opt = _torch_opt(kind, ps, **kw)
            opt.step()
            torch.cuda.synchronize()
        except Exception as e:      # noqa: BLE001 (reported below)
            skipped.append((name, f"{type(e).__name__}: {e}".splitlines()[0][:100]))
            continue
        out.append((name, opt.step))
        if label == "foreach=True":
            def clipped(ps=ps, opt=opt):
                torch.nn.utils.clip_grad_norm_(ps, CLIP, foreach=True)
                opt.step()
            out.append(("  + clip_grad_norm_", clipped))
    return out, skipped


def time_rounds(cands, rounds, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _, fn in cands:
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    us = {label: [] for label, _ in cands}
    for _ in range(rounds):
        for label, fn in cands:
            s.record()
            for _ in range(iters):
                fn()
            e.record()
            torch.cuda.synchronize()
            us[label].append(s.elapsed_time(e) * 1000.0 / iters)
    return us


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--limit_s", type=float, default=120.0, help="time limit of each shape's measurement")
    ap.add_argument("--json", type=str, default="", help="also write the results to this file")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("optim_bench.py measures on the GPU: none found")
    dev = torch.device("cuda", 0)
    results = []
    print(f"{torch.cuda.get_device_name(0)}, torch {torch.__version__}; median of {a.rounds} interleaved rounds "
          f"x {a.iters} steps, us per step (min .. max), bytes per parameter / time")
    for model, shapes in SHAPES.items():
        n = sum(torch.Size(s).numel() for s in shapes)
        for kind in ("adam", "sgd"):
            faulthandler.dump_traceback_later(a.limit_s, exit=True)     # this step's time limit
            cands, skipped = candidates(dev, shapes, kind)
            us = time_rounds(cands, a.rounds, a.iters)
            faulthandler.cancel_dump_traceback_later()
            print(f"\n### {model}: {len(shapes)} tensors, {n / 1e6:.2f} M parameters, {kind} "
                  f"({BYTES[kind]} B per parameter)\n")
            print("| optimizer step | us | min .. max | TB/s |\n|---|---|---|---|")
            for label, _ in cands:
                med = statistics.median(us[label])
                print(f"| {label} | {med:.1f} | {min(us[label]):.1f} .. {max(us[label]):.1f} | "
                      f"{n * BYTES[kind] / med / 1e6:.2f} |", flush=True)
                results.append({"model": model, "kind": kind, "step": label.strip(), "us": med,
                                "us_min": min(us[label]), "us_max": max(us[label]),
                                "tb_per_s": n * BYTES[kind] / med / 1e6})
            for name, why in skipped:
                print(f"| {name} | not available | {why} | |")
            del cands, us
            torch.cuda.empty_cache()
    if a.json:
        with open(a.json, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
