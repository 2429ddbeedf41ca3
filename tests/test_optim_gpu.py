"""The multi-tensor optimizer and gradient-norm kernels (csrc/optim.hip) on the GPU: bitwise
against the per-tensor kernel, the norm against float64, and FusedSGD / FusedAdam against
torch.optim, alone and under a FusedLinear model."""
import pytest
import torch
from torch.nn.utils import clip_grad_norm_

from splitlearning_amd import nn as snn
from splitlearning_amd.config import OptimCfg
from splitlearning_amd.ops import hip_ops
from splitlearning_amd.optim import FusedAdam
from test_optim_cpu import assert_params_close, clones, has_grad, make_params, run_against_torch, set_grads

pytestmark = pytest.mark.gpu

CFGS = {"adam": OptimCfg("adam", 1e-3), "adam_wd": OptimCfg("adam", 1e-3, weight_decay=1e-5),
        "sgd": OptimCfg("sgd", 1e-2, momentum=0.9), "sgd_wd": OptimCfg("sgd", 1e-2, momentum=0.9, weight_decay=1e-5)}


def _states(ps, cfg):
    if cfg.kind == "adam":
        return [{"m": torch.zeros_like(p), "v": torch.zeros_like(p)} for p in ps]
    return [{"buf": torch.zeros_like(p)} for p in ps]


def _with_grads(dev, many, seed, scale=1.0):
    """(the shared list's parameters that get a gradient, their random gradients).  Outside the
    many-tensor list one gradient (CHUNK + 1 elements) starts one element into its buffer, so
    the gradient pointer alone is not 16-byte aligned."""
    allp = make_params(dev, many)
    set_grads(allp, many, seed, scale)
    if not many:
        g = allp[6].grad
        allp[6].grad = torch.cat([g.new_zeros(1), g])[1:]
        assert allp[6].grad.data_ptr() % 16 == 4 and allp[6].grad.is_contiguous()
    ps = has_grad(allp, many)
    return ps, [p.grad for p in ps]


@pytest.mark.parametrize("many", [False, True], ids=["sizes", "many"])
@pytest.mark.parametrize("cfg", list(CFGS))
def test_multi_update_is_bitwise_the_per_tensor_update(cuda, cfg, many):
    cfg = CFGS[cfg]
    ps, _ = _with_grads(cuda, many, 0)
    qs = clones(ps)
    sp, sq = _states(ps, cfg), _states(qs, cfg)
    for t in range(1, 4):
        gs = _with_grads(cuda, many, t)[1]
        hip_ops.multi_update_(ps, gs, sp, cfg, t)
        for q, g, st in zip(qs, gs, sq):
            if q.numel():
                hip_ops.apply_update_(q, g, st, cfg, t)
    for i, (p, q, a, b) in enumerate(zip(ps, qs, sp, sq)):
        assert torch.equal(p, q), f"param {i}"
        for k in a:
            assert torch.equal(a[k], b[k]), f"state {k} of param {i}"
    assert not torch.equal(ps[0], make_params(cuda, many)[0])       # and it did step


def test_sgd_without_momentum_takes_no_buffer(cuda):
    cfg = OptimCfg("sgd", 1e-2, weight_decay=1e-5)
    ps, gs = _with_grads(cuda, False, 0)
    qs = clones(ps)
    hip_ops.multi_update_(ps, gs, [{"buf": None} for _ in ps], cfg, 1)
    for q, g in zip(qs, gs):
        if q.numel():
            hip_ops.apply_update_(q, g, {"buf": torch.zeros_like(q)}, cfg, 1)
    for p, q in zip(ps, qs):
        assert torch.equal(p, q)


@pytest.mark.parametrize("many", [False, True], ids=["sizes", "many"])
def test_grad_norm(cuda, many):
    gs = _with_grads(cuda, many, 0, scale=3.0)[1]
    out = hip_ops.grad_norm(gs, 0.5)
    again = hip_ops.grad_norm(gs, 0.5)
    ref = torch.linalg.vector_norm(torch.cat([g.flatten().double() for g in gs]))
    # per-lane sums of at most a few dozen non-negative terms, then tree reductions: a few
    # 1e-6 relative in the sum of squares, halved by the square root
    torch.testing.assert_close(out[1].double(), ref, rtol=1e-5, atol=0.0)
    torch.testing.assert_close(out[0].double(), ref * ref, rtol=2e-5, atol=0.0)
    assert out[2].item() < 0.1
    torch.testing.assert_close(out[2], 0.5 / (out[1] + 1e-6), rtol=1e-6, atol=0.0)
    assert torch.equal(out, again)                                  # deterministic: the same bits
    assert hip_ops.grad_norm(gs, 1e6)[2].item() == 1.0


@pytest.mark.parametrize("cfg", ["adam_wd", "sgd_wd"])
def test_gscale_is_bitwise_a_prescaled_gradient(cuda, cfg):
    cfg = CFGS[cfg]
    ps, gs = _with_grads(cuda, False, 0, scale=3.0)
    qs = clones(ps)
    sp, sq = _states(ps, cfg), _states(qs, cfg)
    out = hip_ops.grad_norm(gs, 0.5)
    coef = out[2].item()                        # read back: the same float the kernel reads
    assert 0.0 < coef < 0.1
    hip_ops.multi_update_(ps, gs, sp, cfg, 1, gscale=out[2:3])
    hip_ops.multi_update_(qs, [g * coef for g in gs], sq, cfg, 1)
    for i, (p, q, a, b) in enumerate(zip(ps, qs, sp, sq)):
        assert torch.equal(p, q), f"param {i}"
        for k in a:
            assert torch.equal(a[k], b[k]), f"state {k} of param {i}"


@pytest.mark.parametrize("clip", [None, 0.5], ids=["plain", "clipped"])
@pytest.mark.parametrize("kind", ["adam", "sgd"])
def test_fused_optimizers_match_torch_optim(cuda, kind, clip):
    _, _, opt, _ = run_against_torch(cuda, kind, False, steps=1, max_grad_norm=clip, grad_scale=3.0 if clip else 1.0)
    assert all(st[k].is_cuda for st in opt.state.values() for k in st if k != "step")


def _tail(dev):
    torch.manual_seed(0)
    return torch.nn.Sequential(snn.FusedLinear(64, 40, relu=True), snn.FusedLinear(40, 24, relu=True),
                               snn.FusedLinear(24, 12)).to(dev)


def test_fused_linear_tail_trains_like_clip_and_torch_adam(cuda):
    model, ref = _tail(cuda), _tail(cuda)
    opt = FusedAdam(model.parameters(), lr=1e-3, weight_decay=1e-5, max_grad_norm=1.0)
    ropt = torch.optim.Adam(ref.parameters(), lr=1e-3, weight_decay=1e-5)
    g = torch.Generator().manual_seed(1)
    for _ in range(3):
        x = (torch.randn(5, 64, generator=g) * 4).to(cuda)
        y = torch.randint(0, 12, (5,), generator=g).to(cuda)
        opt.zero_grad()
        snn.softmax_cross_entropy(model(x), y).backward()
        opt.step()
        ropt.zero_grad()
        snn.softmax_cross_entropy(ref(x), y).backward()
        total = clip_grad_norm_(ref.parameters(), 1.0)
        ropt.step()
        torch.testing.assert_close(opt.last_grad_norm[1], total, rtol=1e-4, atol=1e-4)
    assert_params_close(list(model.parameters()), list(ref.parameters()), rtol=1e-4, atol=1e-4)
