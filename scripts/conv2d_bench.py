"""FusedConv2d(relu=True, pool=2) (csrc/conv2d.hip: one kernel forward, dgrad + wgrad backward)
against nn.Conv2d + F.relu + F.max_pool2d (MIOpen plus separate ReLU and pool kernels), forward
and forward + backward, and at the MNIST front's shape also against FusedConvFront.

    python scripts/conv2d_bench.py [--rounds 9] [--iters 50] [--limit_s 120]

Shapes (B, Cin -> Cout, H x W, padding): (16, 32 -> 64, 13 x 13, 1), (128, 32 -> 64, 13 x 13, 1)
and (16, 1 -> 32, 28 x 28, 0).  The input requires a gradient at the first two (a conv behind
another layer) and not at the last (a front), so forward + backward includes the data gradient
only there; FusedConvFront never computes one.  Every candidate owns its parameters and inputs;
the candidates of a shape are timed in interleaved rounds (device events around `iters` calls)
after a warm-up that also takes MIOpen's first-call algorithm search out of the timing, and the
median round is reported.  One process; each shape runs under its own time limit (--limit_s)
and the process ends there if the limit passes.
"""
import argparse
import faulthandler
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F
from torch import nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from splitlearning_amd import nn as snn  # noqa: E402

# (B, Cin, Cout, H, W, pad, the input requires a gradient)
SHAPES = [(16, 32, 64, 13, 13, 1, True), (128, 32, 64, 13, 13, 1, True), (16, 1, 32, 28, 28, 0, False)]


class TorchConv(nn.Module):
    def __init__(self, cin, cout, pad):
        super().__init__()
        self.conv = nn.Conv2d(cin, cout, 3, padding=pad)

    def forward(self, x):
        return F.max_pool2d(F.relu(self.conv(x)), 2, 2)


def candidates(dev, shape):
    B, cin, cout, H, W, pad, xgrad = shape
    torch.manual_seed(0)
    mods = [("FusedConv2d", snn.FusedConv2d(cin, cout, padding=pad, relu=True, pool=2)),
            ("nn.Conv2d + relu + max_pool2d", TorchConv(cin, cout, pad))]
    if (cin, cout, H, W, pad) == (1, 32, 28, 28, 0):
        mods.append(("FusedConvFront", snn.FusedConvFront()))
    out = []
    for label, mod in mods:
        mod = mod.to(dev)
        x = torch.randn(B, cin, H, W, device=dev, requires_grad=xgrad)
        with torch.no_grad():
            g = torch.randn_like(mod(x))

        def fwd(mod=mod, x=x):
            with torch.no_grad():
                mod(x)

        def fwd_bwd(mod=mod, x=x, g=g):
            mod.zero_grad(set_to_none=True)
            x.grad = None
            mod(x).backward(g)
        out.append((label + ", forward", fwd))
        out.append((label + ", forward + backward", fwd_bwd))
    return out


def time_rounds(cands, rounds, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _, fn in cands:
        for _ in range(5):
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
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--limit_s", type=float, default=120.0, help="time limit of each shape's measurement")
    ap.add_argument("--json", type=str, default="", help="also write the results to this file")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("conv2d_bench.py measures on the GPU: none found")
    dev = torch.device("cuda", 0)
    print(f"{torch.cuda.get_device_name(0)}, torch {torch.__version__}; median of {a.rounds} interleaved rounds "
          f"x {a.iters} calls, us per call (min .. max)")
    print("MIOpen: MIOPEN_FIND_MODE=" + os.environ.get("MIOPEN_FIND_MODE", "(unset)") +
          ", MIOPEN_USER_DB_PATH=" + os.environ.get("MIOPEN_USER_DB_PATH", "(unset)") +
          ", torch.backends.cudnn.benchmark=" + str(torch.backends.cudnn.benchmark))
    results = []
    for shape in SHAPES:
        B, cin, cout, H, W, pad, xgrad = shape
        faulthandler.dump_traceback_later(a.limit_s, exit=True)     # this shape's time limit
        cands = candidates(dev, shape)
        us = time_rounds(cands, a.rounds, a.iters)
        faulthandler.cancel_dump_traceback_later()
        print(f"\n### B = {B}, {cin} -> {cout}, {H} x {W}, padding {pad}, "
              f"{'input gradient' if xgrad else 'no input gradient'}\n")
        print("| layer, pass | us | min .. max | torch / this |\n|---|---|---|---|")
        med = {label: statistics.median(v) for label, v in us.items()}
        for label, _ in cands:
            base = med["nn.Conv2d + relu + max_pool2d, " + label.split(", ", 1)[1]]
            print(f"| {label} | {med[label]:.1f} | {min(us[label]):.1f} .. {max(us[label]):.1f} | "
                  f"{base / med[label]:.2f} |", flush=True)
            results.append({"shape": shape[:6], "input_grad": xgrad, "case": label, "us": med[label],
                            "us_min": min(us[label]), "us_max": max(us[label]), "torch_over_this": base / med[label]})
        del cands, us
        torch.cuda.empty_cache()
    if a.json:
        with open(a.json, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
