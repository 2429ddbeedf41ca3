"""The cut codec's kernels (csrc/cutcodec.hip: pack, unpack and the one-pass roundtrip) against the
torch twin on the same GPU tensors (ops/torch_ops.py, the eager code a user would otherwise write)
and against a `copy_` that moves the same number of bytes.

    python scripts/cutcodec_bench.py [--rounds 9] [--iters 50] [--limit_s 120] [--json FILE]

Shapes [16, 5408] (one batch at model1_sisa's cut) and [4096, 5408], bits 8 and 4, group 64.  The
bytes of an op are the least it can move: pack reads x and writes payload + scales, unpack the
reverse, roundtrip reads x and writes x^.  The copy baseline copies half that many bytes from one
uint8 buffer to another, so it reads and writes the same total.  The candidates of a shape are timed
in interleaved rounds (device events around `iters` calls) after a warm-up, and the median round is
reported with its spread.  The 88 MB input of the large shape is smaller than the 256 MB last-level
cache, for the kernels and for the copy alike: the rates compare the two, they are not HBM rates.
Kernel launches per call are counted with torch.profiler in a pass of its own, after the timing.
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

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from splitlearning_amd.ops import hip_ops, torch_ops  # noqa: E402

SHAPES = [(16, 5408), (4096, 5408)]
GROUP = 64
SEED = 0x1234_5678_9ABC_DEF0
OPS = ("pack", "unpack", "roundtrip", "roundtrip, stochastic")


def op_bytes(R, K, bits):
    """Least bytes each op moves (read + written)."""
    x = 4 * R * K
    wire = (R * K if bits == 8 else R * ((K + 1) // 2)) + 4 * R * (-(-K // GROUP))
    return {"pack": x + wire, "unpack": wire + x, "roundtrip": 2 * x, "roundtrip, stochastic": 2 * x}


def candidates(dev, R, K, bits):
    x = torch.randn(R, K, device=dev, generator=torch.Generator(dev).manual_seed(0))
    payload, scales = hip_ops.cut_pack(x, bits, GROUP)
    out = []
    for side, K_ in (("hip", hip_ops), ("twin", torch_ops)):
        out.append(((side, "pack"), lambda K_=K_: K_.cut_pack(x, bits, GROUP)))
        out.append(((side, "unpack"), lambda K_=K_: K_.cut_unpack(payload, scales, K, bits, GROUP)))
        out.append(((side, "roundtrip"), lambda K_=K_: K_.cut_roundtrip(x, bits, GROUP)))
        out.append(((side, "roundtrip, stochastic"), lambda K_=K_: K_.cut_roundtrip(x, bits, GROUP, SEED)))
    for op, nbytes in op_bytes(R, K, bits).items():
        if op == "roundtrip, stochastic":
            continue
        src = torch.zeros(nbytes // 2, device=dev, dtype=torch.uint8)
        dst = torch.empty_like(src)
        out.append((("copy", op), lambda src=src, dst=dst: dst.copy_(src)))
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
    ap.add_argument("--limit_s", type=float, default=120.0, help="time limit of each shape's measurement")
    ap.add_argument("--json", type=str, default="", help="also write the results to this file")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("cutcodec_bench.py measures on the GPU: none found")
    dev = torch.device("cuda", 0)
    print(f"{torch.cuda.get_device_name(0)}, torch {torch.__version__}; group {GROUP}; median of {a.rounds} interleaved "
          f"rounds x {a.iters} calls, us per call (min .. max); GB/s = least bytes of the op / time")
    results = []
    for R, K in SHAPES:
        for bits in (8, 4):
            faulthandler.dump_traceback_later(a.limit_s, exit=True)     # this shape's time limit
            cands = candidates(dev, R, K, bits)
            us = time_rounds(cands, a.rounds, a.iters)
            try:
                launches = count_launches(cands)
            except Exception as ex:                                     # the table stands without the counts
                print(f"(launch counts not measured: {type(ex).__name__}: {ex})")
                launches = {}
            faulthandler.cancel_dump_traceback_later()
            nb = op_bytes(R, K, bits)
            med = {key: statistics.median(v) for key, v in us.items()}
            print(f"\n### [{R}, {K}], {bits} bits\n")
            print("| op | MB | hip us | min .. max | hip GB/s | hip launches | twin us | twin launches | twin / hip | "
                  "copy us | min .. max | copy GB/s | hip rate / copy rate |")
            print("|---|---|---|---|---|---|---|---|---|---|---|---|---|")
            for op in OPS:
                h, t, c = ("hip", op), ("twin", op), ("copy", op.split(",")[0])
                rate, crate = nb[op] / med[h] / 1e3, nb[op] / med[c] / 1e3
                print(f"| {op} | {nb[op] / 1e6:.2f} | {med[h]:.1f} | {min(us[h]):.1f} .. {max(us[h]):.1f} | {rate:.0f} | "
                      f"{launches.get(h) or 'not measured'} | {med[t]:.1f} | {launches.get(t) or 'not measured'} | "
                      f"{med[t] / med[h]:.1f} | {med[c]:.1f} | {min(us[c]):.1f} .. {max(us[c]):.1f} | {crate:.0f} | "
                      f"{rate / crate:.2f} |", flush=True)
                results.append({"shape": [R, K], "bits": bits, "op": op, "bytes": nb[op], "hip_us": med[h],
                                "hip_us_min": min(us[h]), "hip_us_max": max(us[h]), "twin_us": med[t], "copy_us": med[c],
                                "hip_launches": launches.get(h), "twin_launches": launches.get(t),
                                "hip_GBps": rate, "copy_GBps": crate, "hip_over_copy_rate": rate / crate})
            del cands, us
            torch.cuda.empty_cache()
    if a.json:
        with open(a.json, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
