"""The cut sparsifier's kernels (csrc/cuttopk.hip: cut_topk_dense, cut_topk, cut_scatter, cut_mask)
against the eager composition a user would otherwise write on the same GPU tensors, in the same
process: abs, topk, sort, gather, zeros, scatter.

    python scripts/cuttopk_bench.py [--rounds 9] [--iters 50] [--limit_s 120] [--json FILE]

Shapes [16, 5408] (one batch at model1_sisa's cut) at k = 338 (1 / 16) and k = 2704 (1 / 2), and
[256, 65536] at k = 4096.  The eager baseline takes `torch.topk` as it is, so its tie order is
whatever the backend gives: it is timed, not compared.  The bytes of an op are the least it can
move: topk_dense reads x and writes y + indices, topk reads x and writes values + indices, scatter
reads values + indices and writes y, mask reads dy at the support + indices and writes dx.  The
candidates of a case are timed in interleaved rounds (device events around `iters` calls) after a
warm-up, and the median round is reported with its spread.  The 64 MB input of the large shape is
smaller than the 256 MB last-level cache: the rates are not HBM rates.  Kernel launches per call are
counted with torch.profiler in a pass of its own, after the timing.  One process; each case runs
under its own time limit (--limit_s) and the process ends there if the limit passes.
"""
import argparse
import faulthandler
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from splitlearning_amd.ops import hip_ops  # noqa: E402

CASES = [(16, 5408, 338), (16, 5408, 2704), (256, 65536, 4096)]
OPS = ("topk_dense", "topk", "scatter", "mask")


def op_bytes(R, K, k):
    """Least bytes each op moves (read + written)."""
    x, wire = 4 * R * K, 4 * R * k
    return {"topk_dense": 2 * x + wire, "topk": x + 2 * wire, "scatter": 2 * wire + x, "mask": 2 * wire + x}


# ---- the eager composition
def eager_topk(x, k):
    idx = torch.topk(x.abs(), k, dim=1).indices.sort(dim=1).values
    return x.gather(1, idx), idx


def eager_scatter(values, idx, K):
    return torch.zeros(values.shape[0], K, device=values.device).scatter_(1, idx, values)


def eager_topk_dense(x, k):
    values, idx = eager_topk(x, k)
    return eager_scatter(values, idx, x.shape[1]), idx


def eager_mask(d, idx):
    return eager_scatter(d.gather(1, idx), idx, d.shape[1])


def candidates(dev, R, K, k):
    gen = torch.Generator(dev).manual_seed(0)
    x = torch.randn(R, K, device=dev, generator=gen)
    d = torch.randn(R, K, device=dev, generator=gen)
    values, indices = hip_ops.cut_topk(x, k)
    idx64 = indices.long()
    return [(("hip", "topk_dense"), lambda: hip_ops.cut_topk_dense(x, k)),
            (("hip", "topk"), lambda: hip_ops.cut_topk(x, k)),
            (("hip", "scatter"), lambda: hip_ops.cut_scatter(values, indices, K)),
            (("hip", "mask"), lambda: hip_ops.cut_mask(d, indices)),
            (("eager", "topk_dense"), lambda: eager_topk_dense(x, k)),
            (("eager", "topk"), lambda: eager_topk(x, k)),
            (("eager", "scatter"), lambda: eager_scatter(values, idx64, K)),
            (("eager", "mask"), lambda: eager_mask(d, idx64))]


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


def count_launches(cands):
    """Kernels per call of every candidate, or None where the profiler gives no device events."""
    from torch.profiler import ProfilerActivity, profile
    n = {}
    for key, fn in cands:
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        k = sum(1 for ev in prof.events() if ev.device_type == torch.autograd.DeviceType.CUDA)
        n[key] = k or None
    return n


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--limit_s", type=float, default=120.0, help="time limit of each case's measurement")
    ap.add_argument("--json", type=str, default="", help="also write the results to this file")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("cuttopk_bench.py measures on the GPU: none found")
    dev = torch.device("cuda", 0)
    print(f"{torch.cuda.get_device_name(0)}, torch {torch.__version__}; median of {a.rounds} interleaved rounds x "
          f"{a.iters} calls, us per call (min .. max); GB/s = least bytes of the op / time")
    results = []
    for R, K, k in CASES:
        faulthandler.dump_traceback_later(a.limit_s, exit=True)     # this case's time limit
        cands = candidates(dev, R, K, k)
        us = time_rounds(cands, a.rounds, a.iters)
        try:
            launches = count_launches(cands)
        except Exception as ex:                                     # the table stands without the counts
            print(f"(launch counts not measured: {type(ex).__name__}: {ex})")
            launches = {}
        faulthandler.cancel_dump_traceback_later()
        nb = op_bytes(R, K, k)
        med = {key: statistics.median(v) for key, v in us.items()}
        print(f"\n### [{R}, {K}], k = {k}\n")
        print("| op | MB | hip us | min .. max | hip GB/s | hip launches | eager us | min .. max | eager launches | "
              "eager / hip |")
        print("|---|---|---|---|---|---|---|---|---|---|")
        for op in OPS:
            h, t = ("hip", op), ("eager", op)
            print(f"| {op} | {nb[op] / 1e6:.2f} | {med[h]:.1f} | {min(us[h]):.1f} .. {max(us[h]):.1f} | "
                  f"{nb[op] / med[h] / 1e3:.0f} | {launches.get(h) or 'not measured'} | {med[t]:.1f} | "
                  f"{min(us[t]):.1f} .. {max(us[t]):.1f} | {launches.get(t) or 'not measured'} | "
                  f"{med[t] / med[h]:.2f} |", flush=True)
            results.append({"shape": [R, K], "k": k, "op": op, "bytes": nb[op], "hip_us": med[h],
                            "hip_us_min": min(us[h]), "hip_us_max": max(us[h]), "eager_us": med[t],
                            "eager_us_min": min(us[t]), "eager_us_max": max(us[t]),
                            "hip_launches": launches.get(h), "eager_launches": launches.get(t),
                            "hip_GBps": nb[op] / med[h] / 1e3, "eager_over_hip": med[t] / med[h]})
        del cands, us
        torch.cuda.empty_cache()
    if a.json:
        with open(a.json, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
