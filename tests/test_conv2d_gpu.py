"""FusedConv2d on an MI355X: the implicit-GEMM kernels of csrc/conv2d.hip against torch.
SHAPES[8:] exist for the launch geometry past one 64 x 64 tile: blockIdx.y > 0 in the forward (Cout > 64) and
in dgrad (Cin > 64), blockIdx.x > 0 and more than three N tiles in wgrad; keep them in any edit of the table."""
import pytest
import torch
import torch.nn.functional as F
from torch import nn

from splitlearning_amd import nn as snn
from splitlearning_amd.ops import hip_ops, torch_ops
from splitlearning_amd.optim import FusedAdam
from test_conv2d_cpu import (INT_CASES, NO_BIAS_CASES, SHAPES, assert_case_equal, int_case, make_layer, run_layer,
                             torch_ref)
from test_optim_cpu import assert_params_close

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------- 1. integer-exact
@pytest.mark.parametrize("i,relu", INT_CASES)
def test_integer_exact_against_torch_cpu(cuda, i, relu):
    c = int_case(i, relu)
    for name in ("y", "dx", "dw", "db"):
        assert c[name].abs().max() > 0, name
    assert_case_equal(run_layer(c, cuda), c)


@pytest.mark.parametrize("i", [i for i, s in enumerate(SHAPES) if s[6]])
def test_argmax_positions_match_torch(cuda, i):
    c = int_case(i, True)
    y, am = hip_ops.conv3x3_fwd(c["x"].to(cuda), c["w"].to(cuda), c["b"].to(cuda), c["pad"], True, 2)
    ry, ram = torch_ops.conv3x3_fwd(c["x"], c["w"], c["b"], c["pad"], True, 2)
    assert am.dtype == torch.uint8 and am.shape == y.shape
    assert torch.equal(y.cpu(), ry) and torch.equal(am.cpu(), ram)


@pytest.mark.parametrize("i,relu", NO_BIAS_CASES)
def test_integer_exact_without_bias(cuda, i, relu):
    """bias=False: the null bias of the forward epilogue through the layer, and the null db of
    conv_wgrad_sum_kernel through the binding (the layer's op always passes a db buffer)."""
    c = int_case(i, relu, bias=False)
    assert c["b"] is None and c["db"] is None
    for name in ("y", "dx", "dw"):
        assert c[name].abs().max() > 0, name
    assert make_layer(c, cuda).bias is None
    got = run_layer(c, cuda)
    assert got[3] is None
    assert_case_equal(got, c)
    # the same weight gradient with no db to write
    x, g, w = c["x"].to(cuda), c["g"].to(cuda), c["w"].to(cuda)
    pool = int(c["pool"] or 0)
    y, am = hip_ops.conv3x3_fwd(x, w, None, c["pad"], relu, c["pool"])
    assert torch.equal(y.cpu(), c["y"])
    n = hip_ops.C().conv3x3_wgrad_ws(list(x.shape), list(w.shape), c["pad"], pool)
    ws = torch.empty(n, device=cuda)
    dw = torch.full_like(w, float("nan"))
    hip_ops.C().conv3x3_wgrad(g, y, am, x, ws, dw, None, c["pad"], relu, pool)
    assert torch.equal(dw.cpu(), c["dw"])


def test_all_equal_windows_route_to_position_zero(cuda):
    x = torch.arange(2 * 2 * 6 * 6, dtype=torch.float32, device=cuda).reshape(2, 2, 6, 6)
    w, b = torch.zeros(3, 2, 3, 3, device=cuda), torch.ones(3, device=cuda)
    y, am = hip_ops.conv3x3_fwd(x, w, b, 0, True, 2)
    assert torch.equal(y.cpu(), torch.ones(2, 3, 2, 2)) and not am.any()
    dy = torch.full_like(y, 2.0)
    w1 = torch.zeros(3, 2, 3, 3, device=cuda)
    w1[:, :, 0, 0] = 1.0                     # dx[h, w] = sum over co of dz[h, w]
    dx = hip_ops.conv3x3_dgrad(dy, y, am, w1, 0, True, 2, x.shape)
    ref = torch.zeros(2, 2, 6, 6)
    ref[:, :, 0:4:2, 0:4:2] = 6.0
    assert torch.equal(dx.cpu(), ref)


def test_mnist_front_matches_fused_conv_front(cuda):
    c = int_case(6, True)
    front = snn.FusedConvFront().to(cuda)
    with torch.no_grad():
        front.conv_layers[0].weight.copy_(c["w"])
        front.conv_layers[0].bias.copy_(c["b"])
    with torch.no_grad():
        y = make_layer(c, cuda)(c["x"].to(cuda))
        yf = front(c["x"].to(cuda))
    assert y.shape == (16, 32, 13, 13)
    assert torch.equal(y.reshape(16, -1), yf)


# ---------------------------------------------------------------- 2. random floats
def _twin(layer):
    conv = nn.Conv2d(layer.in_channels, layer.out_channels, 3, padding=layer.padding).to(layer.weight.device)
    conv.load_state_dict(layer.state_dict())
    return conv


def _float_run(mod, x, g, relu, pool):
    x = x.detach().clone().requires_grad_(True)
    y = mod(x)
    if isinstance(mod, nn.Conv2d):
        y = F.relu(y) if relu else y
        y = F.max_pool2d(y, 2, 2) if pool else y
    y.backward(g)
    return y.detach(), x.grad, mod.weight.grad, mod.bias.grad


@pytest.mark.parametrize("i", [3, 4, 5, 10])
def test_random_floats_match_nn_conv2d(cuda, i):
    B, cin, cout, H, W, pad, pool = SHAPES[i]
    torch.manual_seed(10 + i)
    layer = snn.FusedConv2d(cin, cout, padding=pad, relu=True, pool=pool).to(cuda)
    conv = _twin(layer)
    x = torch.randn(B, cin, H, W, device=cuda)
    with torch.no_grad():
        g = torch.randn_like(layer(x))
    got = _float_run(layer, x, g, True, pool)
    ref = _float_run(conv, x, g, True, pool)
    bad = []
    for name, a, r in zip(("y", "dx", "dw", "db"), got, ref):
        print(f"shape {i + 1} {name}: max |fused - torch| {(a - r).abs().max().item():.3e}")
        if not torch.allclose(a, r, rtol=1e-4, atol=1e-4):
            bad.append(name)
    if bad:
        # which side is off: both against float64 on the CPU
        r64 = torch_ref(x.cpu().double(), layer.weight.detach().cpu().double(), layer.bias.detach().cpu().double(),
                        g.cpu().double(), pad, True, pool)
        msg = [f"{n}: fused off fp64 by {(a.cpu().double() - e).abs().max().item():.3e}, "
               f"torch by {(r.cpu().double() - e).abs().max().item():.3e}"
               for n, a, r, e in zip(("y", "dx", "dw", "db"), got, ref, r64) if n in bad]
        pytest.fail("beyond rtol = atol = 1e-4: " + "; ".join(msg))


# ---------------------------------------------------------------- 3. determinism
def test_backward_is_bitwise_reproducible(cuda):
    c = int_case(7, True)
    torch.manual_seed(0)
    shape = c["x"].shape
    x = torch.randn(shape, device=cuda)
    layer = snn.FusedConv2d(shape[1], c["w"].shape[0], padding=c["pad"], relu=True, pool=c["pool"]).to(cuda)
    g = torch.randn(c["g"].shape, device=cuda)
    assert hip_ops.C().conv3x3_wgrad_ws(list(shape), list(layer.weight.shape), c["pad"], 0) > layer.weight.numel() + 16
    runs = []
    for _ in range(2):
        layer.zero_grad()
        xr = x.clone().requires_grad_(True)
        layer(xr).backward(g)
        runs.append((layer.weight.grad.clone(), layer.bias.grad.clone(), xr.grad.clone()))
    for a, b in zip(*runs):
        assert a.abs().max() > 0 and torch.equal(a, b)


# ---------------------------------------------------------------- 4. leaf input
def test_leaf_input_gets_no_gradient(cuda):
    c = int_case(3, True)
    y, dx, dw, db = run_layer(c, cuda, x_grad=False)
    assert dx is None
    assert torch.equal(dw, c["dw"]) and torch.equal(db, c["db"])


# ---------------------------------------------------------------- 5. non-contiguous input
def test_non_contiguous_input(cuda):
    c = int_case(3, True)
    x = c["x"].to(cuda)
    cl = x.to(memory_format=torch.channels_last)
    assert not cl.is_contiguous()
    assert_case_equal(run_layer(c, cuda, x=cl), c)
    wide = torch.zeros(x.shape[0], x.shape[1], x.shape[2], x.shape[3] + 3, device=cuda)
    wide[..., 1:-2] = x
    sl = wide[..., 1:-2]
    assert not sl.is_contiguous()
    assert_case_equal(run_layer(c, cuda, x=sl), c)


# ---------------------------------------------------------------- 6. a stacked model
def _stacked(dev):
    torch.manual_seed(0)
    return nn.Sequential(snn.FusedConv2d(1, 8, relu=True, pool=2), snn.FusedConv2d(8, 16, padding=1, relu=True, pool=2),
                         nn.Flatten(), snn.FusedLinear(16 * 6 * 6, 32, relu=True), snn.FusedLinear(32, 10)).to(dev)


def _stacked_torch(dev):
    return nn.Sequential(nn.Conv2d(1, 8, 3), nn.ReLU(), nn.MaxPool2d(2, 2), nn.Conv2d(8, 16, 3, padding=1), nn.ReLU(),
                         nn.MaxPool2d(2, 2), nn.Flatten(), nn.Linear(16 * 6 * 6, 32), nn.ReLU(), nn.Linear(32, 10)).to(dev)


def test_stacked_model_trains_like_torch(cuda):
    model, ref = _stacked(cuda), _stacked_torch(cuda)
    with torch.no_grad():
        for p, r in zip(model.parameters(), ref.parameters()):
            r.copy_(p)
    opt = FusedAdam(model.parameters(), lr=1e-3, weight_decay=1e-5)
    ropt = torch.optim.Adam(ref.parameters(), lr=1e-3, weight_decay=1e-5)
    g = torch.Generator().manual_seed(1)
    x = torch.rand(16, 1, 28, 28, generator=g).to(cuda)
    y = torch.randint(0, 10, (16,), generator=g).to(cuda)
    first = [p.detach().clone() for p in model.parameters()]
    for _ in range(3):
        opt.zero_grad()
        snn.softmax_cross_entropy(model(x), y).backward()
        opt.step()
        ropt.zero_grad()
        F.cross_entropy(ref(x), y).backward()
        ropt.step()
    assert all(not torch.equal(p, f) for p, f in zip(model.parameters(), first))     # the first conv included
    assert_params_close(list(model.parameters()), list(ref.parameters()), rtol=1e-4, atol=1e-4)
