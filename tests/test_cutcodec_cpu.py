"""The cut codec on the CPU: the torch twin in ops/torch_ops.py (the definition of the format) and
splitlearning_amd.nn.CutCodec / cut_pack / cut_unpack over it.  tests/test_cutcodec_gpu.py runs the
shapes and cases built here on the HIP kernels of csrc/cutcodec.hip (the helpers are shared).

Bounds.  Nearest rounding leaves |x^ - x| <= 0.5 scale and stochastic rounding < 1 scale in exact
arithmetic; the 1e-3 on top covers the fp32 rounding of x * inv and of q * scale (each below 2e-5
steps at |q| <= 127).  The unbiasedness bound is 6 sigma of a mean of 256 draws of variance at most
scale^2 / 4: 6 * 0.5 / 16 = 0.1875 -> 0.19 scale."""
import functools
import math

import pytest
import torch
from torch import nn

from splitlearning_amd import nn as snn
from splitlearning_amd.ops import rng, torch_ops
from splitlearning_amd.ops.rng import step_seed

# (input shape, group, bits)
SHAPES = [
    ((2, 5408), 64, 8),             # S1 the project's cut; short last group of 32
    ((3, 5408), 64, 4),             # S2 same, nibbles
    ((1, 1), 64, 8),                # S3 one element
    ((5, 63), 64, 4),               # S4 K < group, odd K, lone last nibble
    ((4, 65), 64, 8),               # S5 a last group of one; rows at every 4-byte phase
    ((2, 129), 32, 4),              # S6 odd K, several groups, row 1 misaligned
    ((300, 200), 256, 8),           # S7 K < group, more rows than a workgroup has waves
    ((4096, 96), 16, 8),            # S8 24576 groups = 1536 waves of 16 groups: 384 workgroups
    ((2, 8, 13, 13), 128, 4),       # S9 4-D input, K = 1352 = 10 x 128 + 72
    ((16, 27040), 64, 8),           # S10 a long row (concat of 5 fronts)
    # csrc/cutcodec.hip caps its grid at 2048 workgroups = 8192 waves; at group 16 and 8 bits a wave
    # holds 16 groups, so 4100 x 33 = 135300 groups are 8457 waves: the grid-stride loop's second pass
    ((4100, 520), 16, 8),           # S11 past one grid pass, a short last group of 8
]
QMAX = {8: 127, 4: 7}
SEED = 0x1234_5678_9ABC_DEF0        # the stochastic cases' 64-bit seed


@functools.lru_cache(maxsize=None)
def case(i):
    """Inputs of shape i, computed once and shared: x (the shape's own dims), x2d = [R, K], and where
    the planted values are.  randn, with one group of exact zeros and, in another group, the first
    element at +absmax and the last at -absmax of that group, so both ends of the clamp are met."""
    shape, group, bits = SHAPES[i]
    gen = torch.Generator().manual_seed(100 + i)
    x = torch.randn(shape, generator=gen)
    x2d = x.view(shape[0], -1)
    R, K = x2d.shape
    ng = -(-K // group)
    zr, zg = R - 1, ng // 2                                  # the zero group
    x2d[zr, zg * group:(zg + 1) * group] = 0.0
    pr, pg = 0, (ng - 1 if ng > 1 and (R > 1 or zg != ng - 1) else 0)       # the planted -absmax
    if (pr, pg) != (zr, zg):
        seg = x2d[pr, pg * group:(pg + 1) * group]
        m = seg.abs().max().item()
        seg[0], seg[-1] = m, -m                              # a group of one keeps -m
    return dict(x=x, x2d=x2d, R=R, K=K, ng=ng, group=group, bits=bits, zero=(zr, zg), planted=(pr, pg))


@functools.lru_cache(maxsize=None)
def twin(i, stochastic):
    """(payload, scales, x^) of the torch twin on the CPU for case i, computed once."""
    c = case(i)
    seed = SEED if stochastic else None
    payload, scales = torch_ops.cut_pack(c["x2d"], c["bits"], c["group"], seed)
    return payload, scales, torch_ops.cut_unpack(payload, scales, c["K"], c["bits"], c["group"])


def per_element(scales, K, group):
    return scales.repeat_interleave(group, dim=1)[:, :K]


def ints(payload, K, bits):
    """The integers q [R, K] a payload holds (written independently of torch_ops.cut_unpack)."""
    if bits == 8:
        return payload.to(torch.int64)
    p = payload.to(torch.int64)
    q = torch.stack((p % 16, p // 16), dim=2).view(p.shape[0], -1)[:, :K]
    return torch.where(q >= 8, q - 16, q)


ALL = range(len(SHAPES))


# ---------------------------------------------------------------- 1. hand-written examples
def test_hand_written_row_8_bits():
    x = torch.tensor([[0.5, -1.0, 0.25, 0.0, 1.0]])
    payload, scales = torch_ops.cut_pack(x, 8, 16)
    assert payload.dtype == torch.int8 and scales.dtype == torch.float32
    assert payload.tolist() == [[64, -127, 32, 0, 127]]        # 63.5 -> 64 (even), 31.75 -> 32
    assert scales.shape == (1, 1) and scales[0, 0].item() == torch.tensor(1.0).div(torch.tensor(127.0)).item()
    xh = torch_ops.cut_unpack(payload, scales, 5, 8, 16)
    assert torch.equal(xh, payload.float() * scales[0, 0])


def test_hand_written_row_4_bits():
    x = torch.tensor([[1.0, -1.0, 0.5]])                        # q = 7, -7, 4 (3.5 -> 4, even)
    payload, scales = torch_ops.cut_pack(x, 4, 16)
    assert payload.dtype == torch.uint8 and payload.shape == (1, 2)
    assert payload.tolist() == [[0x7 | (0x9 << 4), 0x4]]        # -7 = 0b1001; the lone high nibble is 0
    assert ints(payload, 3, 4).tolist() == [[7, -7, 4]]
    xh = torch_ops.cut_unpack(payload, scales, 3, 4, 16)
    s = scales[0, 0]
    assert torch.equal(xh, torch.stack((7 * s, -7 * s, 4 * s)).view(1, 3))


def test_hash32_is_what_keep_mask_thresholds():
    h = rng.hash32(SEED, 7, 300)
    assert h.dtype == torch.int64 and h.shape == (7, 300) and h.min() >= 0 and h.max() < 2 ** 32
    for p in (0.1, 0.5):
        assert torch.equal(h >= int(p * 4294967296.0), rng.keep_mask(SEED, 7, 300, p))


# ---------------------------------------------------------------- 2. / 3. error bounds
@pytest.mark.parametrize("i", ALL)
def test_nearest_error_bound(i):
    c = case(i)
    _, scales, xh = twin(i, False)
    err = (xh.double() - c["x2d"].double()).abs()
    bound = (0.5 + 1e-3) * per_element(scales, c["K"], c["group"]).double()
    print(f"S{i + 1} nearest: max |x^ - x| / scale {(err / bound.clamp_min(1e-300)).max().item() * (0.5 + 1e-3):.6f}")
    assert (err <= bound).all()


@pytest.mark.parametrize("i", ALL)
def test_stochastic_error_bound(i):
    c = case(i)
    _, scales, xh = twin(i, True)
    err = (xh.double() - c["x2d"].double()).abs()
    bound = (1 + 1e-3) * per_element(scales, c["K"], c["group"]).double()
    print(f"S{i + 1} stochastic: max |x^ - x| / scale {(err / bound.clamp_min(1e-300)).max().item() * (1 + 1e-3):.6f}")
    assert (err <= bound).all()
    assert not torch.equal(xh, twin(i, False)[2]) or c["K"] == 1


# ---------------------------------------------------------------- 4. unbiasedness
def test_stochastic_rounding_is_unbiased():
    """Over 256 seeds (step_seed(SEED, 0, 1 .. 256), the schedule CutCodec uses) on S1's first row:
    |mean(x^) - x| <= 0.19 scale on every element, 6 sigma of such a mean, while nearest rounding is
    off by more than that on some element.  Seen on the CPU: the largest such mean error is 0.103
    scale, nearest rounding's largest error 0.4999 scale, so the hash passes at 6 sigma as it is."""
    c = case(0)
    x = c["x2d"][:1]
    scale = per_element(torch_ops.cut_pack(x, 8, 64)[1], c["K"], 64).double()
    acc = torch.zeros_like(x, dtype=torch.float64)
    n = 256
    for k in range(1, n + 1):
        acc += torch_ops.cut_roundtrip(x, 8, 64, step_seed(SEED, 0, k)).double()
    bias = (acc / n - x.double()).abs() / scale.clamp_min(1e-300)
    near = (torch_ops.cut_roundtrip(x, 8, 64).double() - x.double()).abs() / scale.clamp_min(1e-300)
    print(f"max |mean(x^) - x| / scale over {n} seeds: {bias.max().item():.4f}; nearest: {near.max().item():.4f}")
    assert (bias <= 0.19).all()
    assert (near > 0.19).any()


# ---------------------------------------------------------------- 5. roundtrip identity
@pytest.mark.parametrize("stochastic", [False, True])
@pytest.mark.parametrize("i", ALL)
def test_roundtrip_is_unpack_of_pack(i, stochastic):
    c = case(i)
    R, K, ng, group, bits = c["R"], c["K"], c["ng"], c["group"], c["bits"]
    payload, scales, xh = twin(i, stochastic)
    assert torch.equal(torch_ops.cut_roundtrip(c["x2d"], bits, group, SEED if stochastic else None), xh)
    assert xh.shape == (R, K) and xh.dtype == torch.float32 and scales.shape == (R, ng) and scales.dtype == torch.float32
    if bits == 8:
        assert payload.dtype == torch.int8 and payload.shape == (R, K)
    else:
        assert payload.dtype == torch.uint8 and payload.shape == (R, (K + 1) // 2)
        if K % 2:
            assert not (payload[:, -1] >> 4).any()              # the lone high nibble
    q = ints(payload, K, bits)
    assert q.abs().max() <= QMAX[bits]
    assert torch.isfinite(xh).all() and torch.isfinite(scales).all()
    zr, zg = c["zero"]
    assert scales[zr, zg] == 0 and not q[zr, zg * group:(zg + 1) * group].any()
    assert not xh[zr, zg * group:(zg + 1) * group].any()
    if c["planted"] != c["zero"]:                               # both ends of the clamp
        pr, pg = c["planted"]
        seg = q[pr, pg * group:(pg + 1) * group]
        assert seg.min() == -QMAX[bits] and (seg.max() == QMAX[bits] or seg.numel() == 1)


# ---------------------------------------------------------------- 6. the module
def _module_case(i):
    c = case(i)
    dy = torch.randn(c["x"].shape, generator=torch.Generator().manual_seed(500 + i))
    return c, dy


@pytest.mark.parametrize("i", [0, 1, 8])
def test_module_forward_and_backward_are_the_twin(i):
    c, dy = _module_case(i)
    group, bits = c["group"], c["bits"]
    grad_bits = 12 - bits                                       # the other width on the way back
    layer = snn.CutCodec(bits, grad_bits, group, seed=7)
    grads = []
    for call in (1, 2):
        x = c["x"].clone().requires_grad_(True)
        y = layer(x)
        assert y.shape == x.shape and torch.equal(y.view(c["R"], -1), twin(i, False)[2])
        y.backward(dy)
        ref = torch_ops.cut_roundtrip(dy.view(c["R"], -1), grad_bits, group, step_seed(7, 0, call))
        assert x.grad.shape == x.shape and torch.equal(x.grad.view(c["R"], -1), ref)
        grads.append(x.grad)
    assert layer.calls == 2 and not torch.equal(grads[0], grads[1])          # a new seed per call
    again = snn.CutCodec(bits, grad_bits, group, seed=7)
    for g in grads:                                             # the same seed repeats the sequence
        x = c["x"].clone().requires_grad_(True)
        again(x).backward(dy)
        assert torch.equal(x.grad, g)
    other = snn.CutCodec(bits, grad_bits, group, seed=8)
    x = c["x"].clone().requires_grad_(True)
    other(x).backward(dy)
    assert not torch.equal(x.grad, grads[0])


def test_module_pass_through_settings():
    c, dy = _module_case(8)
    x = c["x"].clone().requires_grad_(True)
    snn.CutCodec(4, None, 128)(x).backward(dy)
    assert torch.equal(x.grad, dy)                              # grad_bits=None: dy itself
    x = c["x"].clone().requires_grad_(True)
    y = snn.CutCodec(None, 4, 128, seed=3)(x)
    assert torch.equal(y, c["x"])                               # bits=None: the activation untouched
    y.backward(dy)
    assert torch.equal(x.grad.view(2, -1), torch_ops.cut_roundtrip(dy.view(2, -1), 4, 128, step_seed(3, 0, 1)))
    x = c["x"].clone().requires_grad_(True)
    y = snn.CutCodec(None, None)(x)
    y.backward(dy)
    assert torch.equal(y, c["x"]) and torch.equal(x.grad, dy)


def test_module_train_and_eval_compute_the_same():
    c, _ = _module_case(1)
    layer = snn.CutCodec(4, 8, 64)
    a = layer.train()(c["x"])
    b = layer.eval()(c["x"])
    assert torch.equal(a, b) and not torch.equal(a, c["x"])
    with torch.no_grad():
        assert torch.equal(layer(c["x"]), a)


def test_module_has_no_state():
    layer = snn.CutCodec()
    assert not list(layer.parameters()) and not list(layer.buffers()) and not layer.state_dict()
    torch.manual_seed(0)
    plain = nn.Sequential(nn.Flatten(), snn.FusedLinear(24, 8, relu=True), nn.Identity(), snn.FusedLinear(8, 3))
    cut = nn.Sequential(nn.Flatten(), snn.FusedLinear(24, 8, relu=True), snn.CutCodec(8, 4, 16), snn.FusedLinear(8, 3))
    assert list(cut.state_dict().keys()) == list(plain.state_dict().keys())
    cut.load_state_dict(plain.state_dict())
    x = torch.randn(5, 2, 12, generator=torch.Generator().manual_seed(1))
    cut(x).sum().backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in cut.parameters())


def test_module_errors():
    for bad in (2, 16, "8", True):
        with pytest.raises(ValueError, match="bits"):
            snn.CutCodec(bits=bad)
        with pytest.raises(ValueError, match="grad_bits"):
            snn.CutCodec(grad_bits=bad)
    for bad in (0, 8, 48, 512):
        with pytest.raises(ValueError, match="group"):
            snn.CutCodec(group=bad)
        with pytest.raises(ValueError, match="group"):
            snn.cut_pack(torch.zeros(2, 4), group=bad)
    layer = snn.CutCodec()
    with pytest.raises(ValueError, match="float32"):
        layer(torch.zeros(2, 4, dtype=torch.float64))
    with pytest.raises(ValueError, match="dimensions"):
        layer(torch.zeros(4))
    with pytest.raises(ValueError, match="float32"):
        snn.cut_pack(torch.zeros(2, 4, dtype=torch.float16))
    with pytest.raises(ValueError, match="bits"):
        snn.cut_pack(torch.zeros(2, 4), bits=None)
    with pytest.raises(ValueError, match="bits"):
        torch_ops.cut_pack(torch.zeros(2, 4), 5, 64)
    with pytest.raises(ValueError, match="group"):
        torch_ops.cut_roundtrip(torch.zeros(2, 4), 8, 24)


def test_module_accepts_non_contiguous_input():
    c, dy = _module_case(8)
    layer = snn.CutCodec(4, 4, 128, seed=1)
    cl = c["x"].to(memory_format=torch.channels_last)
    assert not cl.is_contiguous()
    x = cl.clone(memory_format=torch.preserve_format).requires_grad_(True)
    assert not x.is_contiguous()
    y = layer(x)
    y.backward(dy.to(memory_format=torch.channels_last))
    assert torch.equal(y.view(2, -1), twin(8, False)[2])
    assert torch.equal(x.grad.contiguous().view(2, -1), torch_ops.cut_roundtrip(dy.view(2, -1), 4, 128, step_seed(1, 0, 1)))


# ---------------------------------------------------------------- 7. the packet
@pytest.mark.parametrize("i", [0, 1, 3, 8])
def test_packet(i):
    c = case(i)
    R, K, ng, group, bits = c["R"], c["K"], c["ng"], c["group"], c["bits"]
    pk = snn.cut_pack(c["x"], bits, group)
    assert isinstance(pk, snn.CutPacket) and pk.shape == tuple(c["x"].shape) and (pk.bits, pk.group) == (bits, group)
    assert torch.equal(pk.payload, twin(i, False)[0]) and torch.equal(pk.scales, twin(i, False)[1])
    assert pk.tensors()[0] is pk.payload and pk.tensors()[1] is pk.scales
    assert pk.nbytes == (R * K if bits == 8 else R * math.ceil(K / 2)) + 4 * R * ng
    y = snn.cut_unpack(pk)
    assert y.shape == c["x"].shape and torch.equal(y.view(R, -1), twin(i, False)[2])
    st = snn.cut_pack(c["x"], bits, group, seed=SEED)
    assert torch.equal(st.payload, twin(i, True)[0])
    assert not snn.cut_pack(c["x"].clone().requires_grad_(True), bits, group).scales.requires_grad
    if group == 64 and K >= 64:                                 # bytes per element of the full groups
        full = K // 64 * 64
        per = (full if bits == 8 else full // 2) + 4 * (full // 64)
        assert per / full == (1.0625 if bits == 8 else 0.5625)
