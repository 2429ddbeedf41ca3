"""FusedConv2d on the CPU (the eager op set in ops/torch_ops.py): constructor and shape
checks, state-dict compatibility with nn.Conv2d, and the integer-exact cases that
tests/test_conv2d_gpu.py runs again on the HIP kernels (the helpers here are shared)."""
import functools

import pytest
import torch
import torch.nn.functional as F
from torch import nn

from splitlearning_amd import nn as snn
from splitlearning_amd.ops import torch_ops

# (B, Cin, Cout, H, W, pad, pool)
SHAPES = [
    (1, 1, 1, 3, 3, 0, None),       # one output pixel, K = 9
    (1, 2, 3, 4, 4, 1, None),       # padding on all sides
    (2, 4, 4, 5, 5, 0, 2),          # odd conv output 3x3: last row and column unpooled
    (2, 3, 5, 7, 6, 1, 2),          # non-square, odd and even mixed
    (2, 17, 33, 9, 9, 0, 2),        # K = 153; Cout one past a 32 tile
    (3, 8, 64, 16, 16, 1, 2),       # several M tiles
    (16, 1, 32, 28, 28, 0, 2),      # the MNIST front
    (64, 8, 16, 12, 12, 1, None),   # 9216 pixels to reduce: several wgrad slabs
    # past one 64 x 64 tile of csrc/conv2d.hip (blockIdx.y > 0 in fwd / dgrad, blockIdx.x > 0 in wgrad)
    (1, 2, 65, 4, 4, 1, 2),         # fwd second N tile holding one channel; wgrad second M tile
    (1, 65, 3, 5, 5, 0, None),      # dgrad second N tile holding one channel; fwd K = 585; wgrad 10 N tiles
    (2, 70, 130, 6, 6, 1, 2),       # both at once: three fwd N tiles, three wgrad M tiles, padding, pooling
    (1, 3, 129, 3, 3, 0, None),     # one output pixel per sample under three N tiles
]
# (index into SHAPES, relu): every shape with ReLU, shapes 2, 4, 9 and 11 (1-based) also without
INT_CASES = [(i, True) for i in range(len(SHAPES))] + [(1, False), (3, False), (8, False), (10, False)]
# (index into SHAPES, relu) run again with bias=False: one pooled and one un-pooled shape past one tile
NO_BIAS_CASES = [(10, True), (9, True)]
SEED = 0


def torch_ref(x, w, b, g, pad, relu, pool):
    """nn.Conv2d [+ ReLU] [+ MaxPool2d(2, 2)] and its autograd -> (y, dx, dw, db)."""
    x = x.detach().clone().requires_grad_(True)
    w = w.detach().clone().requires_grad_(True)
    b = None if b is None else b.detach().clone().requires_grad_(True)
    y = F.conv2d(x, w, b, padding=pad)
    if relu:
        y = F.relu(y)
    if pool:
        y = F.max_pool2d(y, 2, 2)
    y.backward(g)
    return y.detach(), x.grad, w.grad, None if b is None else b.grad


@functools.lru_cache(maxsize=None)
def int_case(i, relu, bias=True):
    """Small-integer inputs (every partial sum is an integer far below 2^24, so the result does
    not depend on the summation order) and torch's CPU result, computed once and shared.
    `bias=False` draws the same x, w and g and drops b (b and db are None)."""
    B, cin, cout, H, W, pad, pool = SHAPES[i]
    gen = torch.Generator().manual_seed(SEED + i)
    x = torch.randint(0, 4, (B, cin, H, W), generator=gen).float()
    w = torch.randint(-1, 2, (cout, cin, 3, 3), generator=gen).float()
    b = torch.randint(-2, 3, (cout,), generator=gen).float()
    ho, wo = H + 2 * pad - 2, W + 2 * pad - 2
    yshape = (B, cout, ho // 2, wo // 2) if pool else (B, cout, ho, wo)
    g = torch.randint(-2, 3, yshape, generator=gen).float()
    b = b if bias else None
    y, dx, dw, db = torch_ref(x, w, b, g, pad, relu, pool)
    return dict(x=x, w=w, b=b, g=g, y=y, dx=dx, dw=dw, db=db, pad=pad, relu=relu, pool=pool)


def make_layer(c, device):
    layer = snn.FusedConv2d(c["w"].shape[1], c["w"].shape[0], padding=c["pad"], bias=c["b"] is not None,
                            relu=c["relu"], pool=c["pool"])
    with torch.no_grad():
        layer.weight.copy_(c["w"])
        if c["b"] is not None:
            layer.bias.copy_(c["b"])
    return layer.to(device)


def run_layer(c, device, x=None, x_grad=True):
    """(y, dx, dw, db) of FusedConv2d on `device` for the case's inputs, moved to the CPU; db is
    None for a case without bias."""
    layer = make_layer(c, device)
    x = (c["x"].to(device) if x is None else x).detach().clone().requires_grad_(x_grad)
    y = layer(x)
    y.backward(c["g"].to(device))
    cpu = lambda t: None if t is None else t.detach().cpu()
    return cpu(y), cpu(x.grad), cpu(layer.weight.grad), cpu(None if layer.bias is None else layer.bias.grad)


def assert_case_equal(got, c):
    for name, t in zip(("y", "dx", "dw", "db"), got):
        if c[name] is None:
            assert t is None, name
            continue
        assert torch.equal(t, c[name]), f"{name} differs: max |diff| {(t - c[name]).abs().max().item()}"


@pytest.mark.parametrize("i,relu", INT_CASES)
def test_integer_cases_are_exact_in_fp32_and_not_trivial(i, relu):
    c = int_case(i, relu)
    ref64 = torch_ref(c["x"].double(), c["w"].double(), c["b"].double(), c["g"].double(), c["pad"], relu, c["pool"])
    for name, t64 in zip(("y", "dx", "dw", "db"), ref64):
        assert torch.equal(c[name].double(), t64), name
        assert c[name].abs().max() > 0, f"{name} is all zero: pick another seed"


@pytest.mark.parametrize("i,relu", INT_CASES)
def test_integer_exact_on_torch_ops(i, relu):
    c = int_case(i, relu)
    assert_case_equal(run_layer(c, "cpu"), c)


@pytest.mark.parametrize("i,relu", NO_BIAS_CASES)
def test_integer_exact_without_bias(i, relu):
    c, cb = int_case(i, relu, bias=False), int_case(i, relu)
    assert c["b"] is None and c["db"] is None
    assert all(torch.equal(c[k], cb[k]) for k in ("x", "w", "g"))          # the draw order is the biased case's
    ref64 = torch_ref(c["x"].double(), c["w"].double(), None, c["g"].double(), c["pad"], relu, c["pool"])
    for name, t64 in zip(("y", "dx", "dw"), ref64):
        assert torch.equal(c[name].double(), t64), name
        assert c[name].abs().max() > 0, f"{name} is all zero: pick another seed"
    assert not torch.equal(c["y"], cb["y"])                                 # the bias mattered
    assert make_layer(c, "cpu").bias is None
    assert_case_equal(run_layer(c, "cpu"), c)


@pytest.mark.parametrize("pad", [0, 1])
@pytest.mark.parametrize("bias", [True, False])
def test_state_dict_round_trip_with_nn_conv2d(pad, bias):
    torch.manual_seed(0)
    conv = nn.Conv2d(3, 5, 3, padding=pad, bias=bias)
    fused = snn.FusedConv2d(3, 5, padding=pad, bias=bias)
    assert set(fused.state_dict()) == set(conv.state_dict())
    fused.load_state_dict(conv.state_dict())
    x = torch.randn(2, 3, 6, 7)
    torch.testing.assert_close(fused(x), conv(x), rtol=1e-5, atol=1e-5)
    back = nn.Conv2d(3, 5, 3, padding=pad, bias=bias)
    back.load_state_dict(fused.state_dict())
    assert all(torch.equal(back.state_dict()[k], conv.state_dict()[k]) for k in conv.state_dict())


def test_default_init_is_nn_conv2d():
    torch.manual_seed(3)
    conv = nn.Conv2d(4, 6, 3)
    torch.manual_seed(3)
    fused = snn.FusedConv2d(4, 6)
    assert torch.equal(fused.weight, conv.weight) and torch.equal(fused.bias, conv.bias)


@pytest.mark.parametrize("kwargs", [dict(kernel_size=5), dict(stride=2), dict(padding=2), dict(pool=3)])
def test_unsupported_arguments_raise(kwargs):
    with pytest.raises(ValueError):
        snn.FusedConv2d(1, 4, **kwargs)


def test_accepted_argument_forms():
    layer = snn.FusedConv2d(2, 4, kernel_size=(3, 3), stride=1, padding=1, relu=True, pool=2)
    assert "in_channels=2, out_channels=4" in repr(layer) and "relu=True, pool=2" in repr(layer)
    assert layer(torch.zeros(1, 2, 5, 4)).shape == (1, 4, 2, 2)
    assert "FusedConv2d" in snn.__all__


def test_too_small_inputs_raise_in_forward():
    with pytest.raises(ValueError):
        snn.FusedConv2d(1, 4)(torch.zeros(1, 1, 2, 2))
    with pytest.raises(ValueError):
        snn.FusedConv2d(1, 4, pool=2)(torch.zeros(1, 1, 3, 3))      # conv output 1x1 < 2x2
    with pytest.raises(ValueError):
        snn.FusedConv2d(1, 4, pool=2)(torch.zeros(1, 1, 4, 3))      # conv output 2x1


def test_tie_goes_to_position_zero():
    # w = 0 and b = 1: every conv output is 1, so all four values of every window tie
    x = torch.arange(2 * 2 * 6 * 6, dtype=torch.float32).reshape(2, 2, 6, 6)
    w, b = torch.zeros(3, 2, 3, 3), torch.ones(3)
    y, am = torch_ops.conv3x3_fwd(x, w, b, 0, True, 2)
    assert torch.equal(y, torch.ones(2, 3, 2, 2)) and am.dtype == torch.uint8 and not am.any()
    dy = torch.full_like(y, 2.0)
    dz = torch_ops._conv3x3_dz(dy, y, am, True, 2, 4, 4)
    assert torch.equal(dz[:, :, ::2, ::2], dy) and dz.sum() == dy.sum()      # all of it at (0, 0)
    _, db = torch_ops.conv3x3_wgrad(dy, y, am, x, 0, True, 2)
    assert torch.equal(db, torch.full((3,), 16.0))


def test_am_is_the_window_position():
    c = int_case(3, True)
    y, am = torch_ops.conv3x3_fwd(c["x"], c["w"], c["b"], c["pad"], True, 2)
    z = F.relu(F.conv2d(c["x"], c["w"], c["b"], padding=c["pad"]))
    hp, wp = y.shape[2:]
    win = torch.stack([z[:, :, dy:2 * hp:2, dx:2 * wp:2] for dy in (0, 1) for dx in (0, 1)], dim=-1)
    assert torch.equal(win.gather(-1, am.long().unsqueeze(-1)).squeeze(-1), y)
    # the lowest position among equals
    first = (win == y.unsqueeze(-1)).float().argmax(dim=-1)
    assert torch.equal(first, am.long())


def test_leaf_input_gets_no_gradient():
    c = int_case(3, True)
    y, dx, dw, db = run_layer(c, "cpu", x_grad=False)
    assert dx is None
    assert torch.equal(dw, c["dw"]) and torch.equal(db, c["db"])
