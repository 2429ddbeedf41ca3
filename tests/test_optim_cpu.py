"""FusedSGD / FusedAdam (splitlearning_amd/optim.py) on CPU tensors against torch.optim, and the
tensor lists the CPU and GPU optimizer tests share."""
import copy

import pytest
import torch
from torch.nn import Parameter
from torch.nn.utils import clip_grad_norm_

from splitlearning_amd.ops.hip_ops import MULTI_OPT_CHUNK as CHUNK
from splitlearning_amd.ops.hip_ops import MULTI_OPT_MAX as CAPACITY
from splitlearning_amd.optim import FusedAdam, FusedSGD

# Where a chunked f32x4 kernel can go wrong: below / at / above the vector width and the chunk,
# several chunks plus a tail, a 2-D tensor.
SHAPES = [(1,), (3,), (4,), (5,), (CHUNK - 1,), (CHUNK,), (CHUNK + 1,), (2 * CHUNK + 7,), (7, 33)]
UNALIGNED = 1027            # a slice starting one element into a buffer: 4- but not 16-byte aligned
RTOL, ATOL = 1e-5, 1e-6     # tests/test_kernels_gpu.py::test_opt_flat's bounds


def make_params(dev, many=False, seed=0):
    """The shared size list as leaf parameters on `dev` (the last one never gets a gradient),
    or with `many` more tensors than one launch's table holds: CAPACITY + 6 of 5 .. 40 elements."""
    g = torch.Generator().manual_seed(seed)
    if many:
        return [Parameter(torch.randn(5 + (7 * i) % 36, generator=g).to(dev)) for i in range(CAPACITY + 6)]
    ps = [Parameter(torch.randn(s, generator=g).to(dev)) for s in SHAPES]
    ps.append(Parameter(torch.randn(UNALIGNED + 1, generator=g).to(dev)[1:]))
    assert ps[-1].is_contiguous() and (torch.device(dev).type == "cpu" or ps[-1].data_ptr() % 16 == 4)
    ps.append(Parameter(torch.empty(0).to(dev)))
    ps.append(Parameter(torch.randn(6, generator=g).to(dev)))       # grad stays None
    return ps


def has_grad(ps, many):
    return ps if many else ps[:-1]


def set_grads(ps, many, seed, scale=1.0):
    g = torch.Generator().manual_seed(1000 + seed)
    for p in has_grad(ps, many):
        p.grad = (torch.randn(p.shape, generator=g) * scale).to(p.device)


def clones(ps):
    return [Parameter(p.detach().clone()) for p in ps]


def copy_grads(src, dst):
    for a, b in zip(src, dst):
        b.grad = None if a.grad is None else a.grad.clone()


def assert_params_close(ps, rs, rtol=RTOL, atol=ATOL):
    for i, (p, r) in enumerate(zip(ps, rs)):
        torch.testing.assert_close(p.detach().cpu(), r.detach().cpu(), rtol=rtol, atol=atol, msg=lambda m: f"param {i}: {m}")


def make_pair(kind, ps, rs, max_grad_norm=None):
    """(fused optimizer over ps, torch optimizer over rs) with the issue's hyper-parameters."""
    if kind == "adam":
        return (FusedAdam(ps, lr=1e-3, weight_decay=1e-5, max_grad_norm=max_grad_norm),
                torch.optim.Adam(rs, lr=1e-3, weight_decay=1e-5))
    return (FusedSGD(ps, lr=1e-2, momentum=0.9, weight_decay=1e-5, max_grad_norm=max_grad_norm),
            torch.optim.SGD(rs, lr=1e-2, momentum=0.9, weight_decay=1e-5))


def run_against_torch(dev, kind, many, steps, max_grad_norm=None, grad_scale=1.0):
    ps = make_params(dev, many)
    rs = clones(ps)
    opt, ref = make_pair(kind, ps, rs, max_grad_norm)
    for s in range(steps):
        set_grads(ps, many, s, grad_scale)
        copy_grads(ps, rs)
        opt.step()
        if max_grad_norm is not None:
            total = clip_grad_norm_(rs, max_grad_norm)
            torch.testing.assert_close(opt.last_grad_norm[1].cpu(), total.cpu(), rtol=1e-5, atol=0.0)
            assert opt.last_grad_norm[2].item() < 0.1       # the clip is far from a no-op
        ref.step()
        assert_params_close(ps, rs)
    assert ps[-1].grad is not None or ps[-1] not in opt.state   # the grad-less parameter has no state
    return ps, rs, opt, ref


@pytest.mark.parametrize("many", [False, True], ids=["sizes", "many"])
@pytest.mark.parametrize("kind", ["adam", "sgd"])
def test_matches_torch_optim(kind, many):
    run_against_torch("cpu", kind, many, steps=5)


@pytest.mark.parametrize("kind", ["adam", "sgd"])
def test_clipping_matches_clip_grad_norm(kind):
    # ~10 k gradient elements of std 3: a norm near 300 against max_grad_norm = 0.5
    run_against_torch("cpu", kind, False, steps=5, max_grad_norm=0.5, grad_scale=3.0)


@pytest.mark.parametrize("kind", ["adam", "sgd"])
def test_clipping_above_the_norm_is_the_plain_step(kind):
    ps = make_params("cpu")
    qs = clones(ps)
    clipped = make_pair(kind, ps, clones(ps), max_grad_norm=1e6)[0]
    plain = make_pair(kind, qs, clones(qs))[0]
    for s in range(2):
        set_grads(ps, False, s)
        copy_grads(ps, qs)
        clipped.step()
        plain.step()
        assert clipped.last_grad_norm[2].item() == 1.0
    for p, q in zip(ps, qs):
        assert torch.equal(p, q)


@pytest.mark.parametrize("direction", ["fused_to_torch", "torch_to_fused"])
@pytest.mark.parametrize("kind", ["adam", "sgd"])
def test_state_dict_round_trip(kind, direction):
    ps = make_params("cpu")
    rs = clones(ps)
    opt, ref = make_pair(kind, ps, rs)
    src_p, src, dst_p, dst = (ps, opt, rs, ref) if direction == "fused_to_torch" else (rs, ref, ps, opt)
    for s in range(2):
        set_grads(src_p, False, s)
        src.step()
    with torch.no_grad():
        for a, b in zip(src_p, dst_p):
            b.copy_(a)
    dst.load_state_dict(copy.deepcopy(src.state_dict()))    # load_state_dict keeps the tensors it is given
    if kind == "adam":
        assert set(dst.state[dst_p[0]]) == {"step", "exp_avg", "exp_avg_sq"} and int(dst.state[dst_p[0]]["step"]) == 2
    else:
        assert set(dst.state[dst_p[0]]) == {"momentum_buffer"}
    for s in range(2, 4):
        set_grads(ps, False, s)
        copy_grads(ps, rs)
        opt.step()
        ref.step()
    assert_params_close(ps, rs)


def test_param_groups_with_their_own_lr():
    ps = make_params("cpu")
    rs = clones(ps)
    half = len(ps) // 2
    for fused, torch_cls, kw in [(FusedAdam, torch.optim.Adam, {}), (FusedSGD, torch.optim.SGD, {"momentum": 0.9})]:
        opt = fused([{"params": ps[:half]}, {"params": ps[half:], "lr": 0.05}], lr=1e-3, **kw)
        ref = torch_cls([{"params": rs[:half]}, {"params": rs[half:], "lr": 0.05}], lr=1e-3, **kw)
        for s in range(3):
            set_grads(ps, False, s)
            copy_grads(ps, rs)
            opt.step()
            ref.step()
        assert_params_close(ps, rs)


def test_strided_gradient_is_gathered():
    ps = make_params("cpu")
    rs = clones(ps)
    opt, ref = make_pair("adam", ps, rs)
    set_grads(ps, False, 0)
    ps[8].grad = torch.randn(33, 7).t()         # the (7, 33) parameter
    assert not ps[8].grad.is_contiguous()
    copy_grads(ps, rs)
    opt.step()
    ref.step()
    assert_params_close(ps, rs)


def test_sgd_without_momentum_keeps_no_buffer():
    ps = make_params("cpu")
    rs = clones(ps)
    opt, ref = FusedSGD(ps, lr=0.1), torch.optim.SGD(rs, lr=0.1)
    set_grads(ps, False, 0)
    copy_grads(ps, rs)
    opt.step()
    ref.step()
    assert_params_close(ps, rs)
    assert all(not st or st.get("momentum_buffer") is None for st in opt.state.values())


@pytest.mark.parametrize("cls,kw", [
    (FusedSGD, {"nesterov": True, "momentum": 0.9}), (FusedSGD, {"dampening": 0.1}), (FusedSGD, {"maximize": True}),
    (FusedAdam, {"amsgrad": True}), (FusedAdam, {"maximize": True})])
def test_unsupported_options_raise(cls, kw):
    with pytest.raises(ValueError):
        cls([Parameter(torch.zeros(4))], lr=0.1, **kw)


def test_unsupported_options_raise_when_loaded():
    p = Parameter(torch.zeros(4))
    sd = torch.optim.Adam([p], amsgrad=True).state_dict()
    with pytest.raises(ValueError):
        FusedAdam([p]).load_state_dict(sd)


@pytest.mark.parametrize("cls", [FusedSGD, FusedAdam])
def test_bf16_or_strided_parameter_raises(cls):
    with pytest.raises(ValueError):
        cls([Parameter(torch.zeros(4, dtype=torch.bfloat16))], lr=0.1)
    with pytest.raises(ValueError):
        cls([Parameter(torch.zeros(4, 6).t())], lr=0.1)
