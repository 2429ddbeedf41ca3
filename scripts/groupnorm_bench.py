"""FusedGroupNorm(relu=True, pool=2) (csrc/groupnorm.hip: one kernel forward, one kernel plus the
parameter-gradient sum backward) against nn.GroupNorm + F.relu + F.max_pool2d, forward and
forward + backward, and the block conv -> norm -> ReLU -> pool both ways (FusedConv2d +
FusedGroupNorm against nn.Conv2d + nn.GroupNorm + F.relu + F.max_pool2d).

    python scripts/groupnorm_bench.py [--rounds 9] [--iters 50] [--limit_s 120]

Shapes (B, C, G, H x W) of the norm's input: (16, 32, 8, 26 x 26), (128, 32, 8, 26 x 26),
(16, 64, 8, 32 x 32) and (128, 64, 8, 32 x 32).  The block's conv is Conv2d(1, 32, 3) on 28 x 28
for the first two (model1_sisa's front: its input gets no gradient) and Conv2d(32, 64, 3,
padding=1) on 32 x 32 for the last two (a conv behind another layer: its input gets one).  The
norm's own input always requires a gradient.  Every candidate owns its parameters and inputs; the
candidates of a shape are timed in interleaved rounds (device events around `iters` calls) after
a warm-up that also takes MIOpen's first-call algorithm search out of the timing, and the median
round is reported.  Beside the time of the fused norm stands the rate at which it moves the
least traffic the pass needs: x once plus y forward, and x, dy and dx more for the backward.
One process; each shape runs under its own time limit (--limit_s) and the process ends there if
the limit passes.
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

# (B, C, G, H, W, the block's conv: (Cin, padding, its input requires a gradient))
SHAPES = [(16, 32, 8, 26, 26, (1, 0, False)), (128, 32, 8, 26, 26, (1, 0, False)),
          (16, 64, 8, 32, 32, (32, 1, True)), (128, 64, 8, 32, 32, (32, 1, True))]
NORM, BLOCK = "norm + relu + pool", "conv + norm + relu + pool"


class TorchNorm(nn.Module):
    def __init__(self, groups, channels, conv=None):
        super().__init__()
        self.conv = conv
        self.norm = nn.GroupNorm(groups, channels)

    def forward(self, x):
        x = self.conv(x) if self.conv is not None else x
        return F.max_pool2d(F.relu(self.norm(x)), 2, 2)


def min_bytes(shape):
    """(forward, backward) bytes of the norm's least traffic: x + y, and x + dy + dx."""
    B, C, G, H, W, _ = shape
    nx, ny = B * C * H * W, B * C * (H // 2) * (W // 2)
    return 4 * (nx + ny), 4 * (2 * nx + ny)


def candidates(dev, shape):
    B, C, G, H, W, (cin, pad, cgrad) = shape
    torch.manual_seed(0)
    hin, win = H + 2 - 2 * pad, W + 2 - 2 * pad
    mods = [("fused", NORM, snn.FusedGroupNorm(G, C, relu=True, pool=2), (B, C, H, W), True),
            ("torch", NORM, TorchNorm(G, C), (B, C, H, W), True),
            ("fused", BLOCK, nn.Sequential(snn.FusedConv2d(cin, C, padding=pad), snn.FusedGroupNorm(G, C, relu=True, pool=2)),
             (B, cin, hin, win), cgrad),
            ("torch", BLOCK, TorchNorm(G, C, nn.Conv2d(cin, C, 3, padding=pad)), (B, cin, hin, win), cgrad)]
    out = []
    for side, what, mod, xshape, xgrad in mods:
        mod = mod.to(dev)
        x = torch.randn(xshape, device=dev, requires_grad=xgrad)
        with torch.no_grad():
            g = torch.randn_like(mod(x))

        def fwd(mod=mod, x=x):
            with torch.no_grad():
                mod(x)

        def fwd_bwd(mod=mod, x=x, g=g):
            mod.zero_grad(set_to_none=True)
            x.grad = None
            mod(x).backward(g)
        out.append(((side, what, "forward"), fwd))
        out.append(((side, what, "forward + backward"), fwd_bwd))
    return out


def time_rounds(cands, rounds, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _, fn in cands:
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    us = {key: [] for key, _ in cands}
    for _ in range(rounds):
        for key, fn in cands:
            s.record()
            for _ in range(iters):
                fn()
            e.record()
            torch.cuda.synchronize()
            us[key].append(s.elapsed_time(e) * 1000.0 / iters)
    return us


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--limit_s", type=float, default=120.0, help="time limit of each shape's measurement")
    ap.add_argument("--json", type=str, default="", help="also write the results to this file")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("groupnorm_bench.py measures on the GPU: none found")
    dev = torch.device("cuda", 0)
    print(f"{torch.cuda.get_device_name(0)}, torch {torch.__version__}; median of {a.rounds} interleaved rounds "
          f"x {a.iters} calls, us per call (min .. max)")
    print("MIOpen: MIOPEN_FIND_MODE=" + os.environ.get("MIOPEN_FIND_MODE", "(unset)") +
          ", torch.backends.cudnn.benchmark=" + str(torch.backends.cudnn.benchmark))
    results = []
    for shape in SHAPES:
        B, C, G, H, W, (cin, pad, cgrad) = shape
        faulthandler.dump_traceback_later(a.limit_s, exit=True)     # this shape's time limit
        cands = candidates(dev, shape)
        us = time_rounds(cands, a.rounds, a.iters)
        faulthandler.cancel_dump_traceback_later()
        bf, bb = min_bytes(shape)
        print(f"\n### B = {B}, C = {C}, G = {G}, {H} x {W} ({B * G} workgroups; block conv {cin} -> {C}, padding {pad}, "
              f"{'input gradient' if cgrad else 'no input gradient'})\n")
        print("| layers, pass | fused us | min .. max | torch us | min .. max | torch / fused | fused GB/s of least traffic |")
        print("|---|---|---|---|---|---|---|")
        med = {key: statistics.median(v) for key, v in us.items()}
        for what in (NORM, BLOCK):
            for pas in ("forward", "forward + backward"):
                f, t = ("fused", what, pas), ("torch", what, pas)
                nbytes = bf if pas == "forward" else bf + bb
                rate = f"{nbytes / med[f] / 1e3:.0f}" if what == NORM else ""
                print(f"| {what}, {pas} | {med[f]:.1f} | {min(us[f]):.1f} .. {max(us[f]):.1f} | {med[t]:.1f} | "
                      f"{min(us[t]):.1f} .. {max(us[t]):.1f} | {med[t] / med[f]:.2f} | {rate} |", flush=True)
                results.append({"shape": shape[:5], "layers": what, "pass": pas, "fused_us": med[f], "torch_us": med[t],
                                "fused_us_min": min(us[f]), "fused_us_max": max(us[f]), "torch_us_min": min(us[t]),
                                "torch_us_max": max(us[t]), "torch_over_fused": med[t] / med[f],
                                "least_bytes": nbytes if what == NORM else None})
        del cands, us
        torch.cuda.empty_cache()
    if a.json:
        with open(a.json, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
