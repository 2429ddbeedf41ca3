"""The Python-visible surface of `_C` and its host-side refusals, without a GPU.

1. Every function's pybind signature, every class's public methods and every attribute's value
   are compared with tests/data/native_surface.json (recorded once; regenerate only when the
   surface is meant to change: `python tests/test_native_surface_cpu.py --record`).
2. Every tensor-taking function refuses a CPU tensor as its first tensor operand (of otherwise
   valid shape and dtype) with a RuntimeError, before anything reaches a GPU.
"""
import inspect
import json
import os
import re
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))   # for --record

C = pytest.importorskip("splitlearning_amd._C")

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data", "native_surface.json")


def _sig_lines(obj):
    """The pybind signature line(s) of a function's docstring: `name(args) -> ret`, one per
    overload, without the free text."""
    name = obj.__name__
    doc = obj.__doc__ or ""
    pat = re.compile(r"^\s*(?:\d+\.\s+)?(" + re.escape(name) + r"\(.*\)\s*->\s*.+?)\s*$")
    out = [m.group(1) for m in map(pat.match, doc.splitlines()) if m]
    assert out, f"{name}: no pybind signature in its docstring"
    return out


def surface():
    funcs, classes, attrs = {}, {}, {}
    for name in sorted(dir(C)):
        if name.startswith("__"):
            continue
        obj = getattr(C, name)
        if inspect.isclass(obj):
            methods = {}
            for m in sorted(dir(obj)):
                if m.startswith("_") and m != "__init__":
                    continue
                mo = getattr(obj, m)
                if callable(mo):
                    methods[m] = _sig_lines(mo)
                else:
                    methods[m] = f"<{type(mo).__name__}>"
            classes[name] = methods
        elif callable(obj):
            funcs[name] = _sig_lines(obj)
        else:
            attrs[name] = obj
    return {"functions": funcs, "classes": classes, "attributes": attrs}


def test_surface_matches_fixture():
    with open(FIXTURE) as f:
        want = json.load(f)
    got = surface()
    for kind in ("functions", "classes", "attributes"):
        assert sorted(got[kind]) == sorted(want[kind]), f"{kind}: names differ"
        for name in want[kind]:
            assert got[kind][name] == want[kind][name], f"{kind}: {name}"


# ---------------------------------------------------------------- CPU operands are refused
def f32(*shape):
    return torch.zeros(*shape)


def i64(*shape):
    return torch.zeros(*shape, dtype=torch.long)


def u8(*shape):
    return torch.zeros(*shape, dtype=torch.uint8)


OPT = (2, 1e-3, 0.9, 0.999, 1e-8, 0.0, 0.0, 1, 0)   # kind, lr, beta1, beta2, eps, wd, momentum, t, dyn
B = 2
X, IDX, LAB = (lambda: u8(4, 784)), (lambda: i64(B)), (lambda: i64(4))
CW, CB = (lambda: f32(288)), (lambda: f32(32))
CUT, AM, SLAB = (lambda: f32(B, 5408)), (lambda: u8(B, 5408)), (lambda: f32(B, 320))

# name -> a call whose operands are all valid in shape and dtype, all on the CPU
CPU_CALLS = {
    "conv_fwd": lambda: C.conv_fwd(X(), IDX(), B, CW(), CB(), CUT(), AM(), None, None),
    "conv_fwd_pending": lambda: C.conv_fwd_pending(X(), IDX(), B, CW(), CB(), CUT(), AM(), LAB(), i64(B), SLAB(), B,
                                                   CW(), CW(), CB(), CB(), *OPT),
    "conv_local_step": lambda: C.conv_local_step(X(), IDX(), LAB(), B, CW(), CB(), SLAB(), f32(B), CW(), CW(), CB(),
                                                 CB(), *OPT),
    "conv_local_epoch": lambda: C.conv_local_epoch(X(), i64(4), LAB(), B, CW(), CB(), SLAB(), f32(4), CW(), CW(), CB(),
                                                   CB(), *OPT[:7], 0, f32(4096)),
    "conv_local_epoch_multi": lambda: C.conv_local_epoch_multi(
        [(X(), i64(4), LAB(), CW(), CB(), CW(), CW(), CB(), CB(), f32(2 * B * 320 + 2 * 960), f32(4), 0)], B,
        *OPT[:7], u8(4096)),
    "conv_fwd_multi": lambda: C.conv_fwd_multi([(X(), None, 2, CW(), CB(), CUT())], 2),
    "conv_bwd_step": lambda: C.conv_bwd_step(CUT(), CUT(), AM(), X(), IDX(), B, CW(), CB(), SLAB(), CW(), CW(), CB(),
                                             CB(), *OPT),
    "conv_bwd_defer": lambda: C.conv_bwd_defer(CUT(), CUT(), AM(), X(), IDX(), B, CW(), CB(), SLAB(), None, 0, CW(),
                                               CW(), CB(), CB(), *OPT),
    "conv_apply": lambda: C.conv_apply(SLAB(), B, CW(), CB(), CW(), CW(), CB(), CB(), *OPT),
    "head_step": lambda: C.head_step(f32(2, 8), f32(3, 8), f32(3), i64(2), -100, 0.5, False, f32(2), f32(2, 8),
                                     f32(3, 8), f32(3, 8), f32(3), f32(3), *OPT),
    "linear_fwd": lambda: C.linear_fwd(f32(2, 8), f32(3, 8), f32(3), f32(2, 3), True, 0.0, 0, 0, 0, None),
    "linear_epilogue": lambda: C.linear_epilogue(f32(2, 3), f32(3), f32(2, 3), True, 0.0, 0, 0, 0),
    "linear_dgrad": lambda: C.linear_dgrad(f32(2, 4), f32(4, 8), None, 1.0, f32(2, 8), None),
    "gemm_nn_dgrad": lambda: C.gemm_nn_dgrad(f32(2, 4), f32(4, 8), None, 1.0, f32(2, 8), None),
    "linear_wgrad_opt": lambda: C.linear_wgrad_opt(f32(2, 4), f32(2, 8), f32(4, 8), f32(4, 8), f32(4, 8), f32(4),
                                                   f32(4), f32(4), *OPT),
    "linear_fwd_partial": lambda: C.linear_fwd_partial(f32(2, 8), f32(4, 8), f32(1024), 4),
    "opt_flat": lambda: C.opt_flat(f32(8), f32(8), f32(8), f32(8), *OPT),
    "multi_opt": lambda: C.multi_opt([f32(8)], [f32(8)], [f32(8)], [f32(8)], *OPT, None),
    "grad_norm": lambda: C.grad_norm([f32(8)], 1.0, f32(3), f32(4)),
    "conv3x3_fwd": lambda: C.conv3x3_fwd(f32(1, 2, 4, 4), f32(3, 2, 3, 3), f32(3), f32(1, 3, 4, 4), None, 1, True, 0),
    "conv3x3_dgrad": lambda: C.conv3x3_dgrad(f32(1, 3, 4, 4), f32(1, 3, 4, 4), None, f32(3, 2, 3, 3), f32(1, 2, 4, 4),
                                             1, True, 0),
    "conv3x3_wgrad": lambda: C.conv3x3_wgrad(f32(1, 3, 4, 4), f32(1, 3, 4, 4), None, f32(1, 2, 4, 4), f32(4096),
                                             f32(3, 2, 3, 3), f32(3), 1, True, 0),
    "group_norm_fwd": lambda: C.group_norm_fwd(f32(1, 4, 3), f32(4), f32(4), f32(1, 4, 3), f32(1, 2), f32(1, 2), None,
                                               2, 1e-5, False, 0),
    "group_norm_bwd": lambda: C.group_norm_bwd(f32(1, 4, 3), f32(1, 4, 3), f32(1, 2), f32(1, 2), f32(4), f32(4), None,
                                               f32(1, 4, 3), f32(1, 4, 2), f32(4), f32(4), 2, False, 0),
    "cut_pack": lambda: C.cut_pack(f32(2, 16), torch.zeros(2, 16, dtype=torch.int8), f32(2, 1), 8, 16, 0, False),
    "cut_unpack": lambda: C.cut_unpack(torch.zeros(2, 16, dtype=torch.int8), f32(2, 1), f32(2, 16), 8, 16),
    "cut_roundtrip": lambda: C.cut_roundtrip(f32(2, 16), f32(2, 16), 8, 16, 0, False),
    "softmax_ce": lambda: C.softmax_ce(f32(2, 4), i64(2), -100, 0.5, f32(2), f32(2, 4)),
    "relu_mask": lambda: C.relu_mask(f32(8), f32(8), 1.0, f32(8)),
    "eval_counters": lambda: C.eval_counters(f32(2, 4), i64(2), -1, i64(6)),
    "server_head3": lambda: C.server_head3(f32(2, 8), f32(8), True, 0.0, 0, 0, f32(4, 8), f32(4), i64(2), -100, 0.5,
                                           f32(2, 8), f32(2, 4), f32(2, 8), f32(2), f32(4096), 1, None),
    "wgrad_group": lambda: C.wgrad_group([(f32(2, 4), f32(2, 8), f32(4, 8), f32(4, 8), f32(4, 8), f32(4), f32(4),
                                           f32(4))], 2, None, None, *OPT),
}


def _takes_tensor(fn):
    return any("Tensor" in s.split("->")[0] or "list" in s.split("->")[0] or "tuple" in s.split("->")[0]
               for s in _sig_lines(fn))


def test_every_tensor_function_has_a_cpu_case():
    """A new tensor-taking binding gets its CPU-operand refusal here too."""
    # collectives and the executors' free functions take a communicator / executor first
    other_first = {"allreduce_sum", "broadcast", "all_gather", "send", "recv", "tp_emulate_epoch"}
    names = {n for n in dir(C) if not n.startswith("_") and not inspect.isclass(getattr(C, n))
             and callable(getattr(C, n)) and _takes_tensor(getattr(C, n))}
    assert names - other_first - set(CPU_CALLS) == set()


# multi_opt asks for the current stream before it looks at its lists, which a host without a GPU
# already refuses; its CPU-operand refusal is in tests/test_native_checks_gpu.py (mo_cpu_param)
STREAM_FIRST = {"multi_opt": "GPU tensor|ROCm-capable device"}


@pytest.mark.parametrize("name", sorted(CPU_CALLS))
def test_cpu_operand_is_refused(name):
    with pytest.raises(RuntimeError, match=STREAM_FIRST.get(name, "must be a GPU tensor")):
        CPU_CALLS[name]()


if __name__ == "__main__":
    if sys.argv[1:] == ["--record"]:
        os.makedirs(os.path.dirname(FIXTURE), exist_ok=True)
        with open(FIXTURE, "w") as f:
            json.dump(surface(), f, indent=1, sort_keys=True)
            f.write("\n")
        print(FIXTURE)
