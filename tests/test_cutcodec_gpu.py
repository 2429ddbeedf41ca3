"""The cut codec on an MI355X: the kernels of csrc/cutcodec.hip against the torch twin on the CPU.

Every comparison is torch.equal.  The format is integers plus two IEEE divisions per group, the
group maximum does not depend on the order it is taken in, and the kernels round x * inv and the
sum with u separately, as the twin's separate torch ops do: there is nothing for a tolerance to
cover, and a value near a rounding boundary would be off by a whole step anyway."""
import pytest
import torch
from torch import nn

from splitlearning_amd import nn as snn
from splitlearning_amd.ops import hip_ops, torch_ops
from splitlearning_amd.ops.rng import step_seed
from splitlearning_amd.optim import FusedAdam
from test_cutcodec_cpu import SEED, SHAPES, case, twin

pytestmark = pytest.mark.gpu


def _hip(c, x2d, stochastic):
    """(payload, scales, x^ of unpack, x^ of roundtrip) of the HIP kernels on the device tensor x2d."""
    seed = SEED if stochastic else None
    payload, scales = hip_ops.cut_pack(x2d, c["bits"], c["group"], seed)
    xh = hip_ops.cut_unpack(payload, scales, c["K"], c["bits"], c["group"])
    return payload, scales, xh, hip_ops.cut_roundtrip(x2d, c["bits"], c["group"], seed)


def _same(a, r):
    return a.shape == r.shape and a.dtype == r.dtype and torch.equal(a.cpu(), r.cpu())


# ---------------------------------------------------------------- 1. equality with the twin
@pytest.mark.parametrize("stochastic", [False, True])
@pytest.mark.parametrize("i", range(len(SHAPES)))
def test_kernels_equal_the_twin(cuda, i, stochastic):
    c = case(i)
    payload, scales, xh = twin(i, stochastic)
    got = _hip(c, c["x2d"].to(cuda), stochastic)
    for name, a, r in zip(("payload", "scales", "unpack", "roundtrip"), got, (payload, scales, xh, xh)):
        if not _same(a, r):
            bad = (a.cpu() != r).nonzero()
            pytest.fail(f"S{i + 1} {name}: {tuple(a.shape)} {a.dtype} against {tuple(r.shape)} {r.dtype}, "
                        f"{bad.shape[0]} elements differ, the first at {bad[0].tolist() if bad.numel() else None}")


# ---------------------------------------------------------------- 2. misaligned base pointers
def _at_offset(t, off, dev):
    """A contiguous device copy of t that starts `off` elements into a larger, 16-byte aligned buffer."""
    buf = torch.empty(t.numel() + 4, device=dev, dtype=t.dtype)
    assert buf.data_ptr() % 16 == 0
    v = buf[off:off + t.numel()].view(t.shape)
    v.copy_(t)
    return v


@pytest.mark.parametrize("stochastic", [False, True])
@pytest.mark.parametrize("i", [0, 4, 5])
def test_misaligned_base_pointers(cuda, i, stochastic):
    """x one float and three floats into its storage: bitwise the aligned run (and with that the
    twin), since no result depends on which lanes take the float4 path."""
    c = case(i)
    x0 = c["x2d"].to(cuda)
    assert x0.data_ptr() % 16 == 0
    ref = _hip(c, x0, stochastic)
    assert _same(ref[0], twin(i, stochastic)[0])
    for off in (1, 3):
        xo = _at_offset(c["x2d"], off, cuda)
        assert xo.data_ptr() % 16 == 4 * off and xo.is_contiguous()
        got = _hip(c, xo, stochastic)
        assert all(_same(a, r) for a, r in zip(got, ref)), f"S{i + 1} at offset {off}"
        # the wire tensors too: the payload one and three bytes, the scales one float, into their storage
        po, so = _at_offset(ref[0], off, cuda), _at_offset(ref[1], 1, cuda)
        assert _same(hip_ops.cut_unpack(po, so, c["K"], c["bits"], c["group"]), ref[2])


# ---------------------------------------------------------------- 3. non-contiguous input
@pytest.mark.parametrize("stochastic", [False, True])
def test_channels_last_and_sliced_inputs(cuda, stochastic):
    c = case(8)
    seed = SEED if stochastic else None
    x = c["x"].to(cuda)
    R = x.shape[0]
    cl = x.to(memory_format=torch.channels_last)
    wide = torch.zeros(x.shape[0], x.shape[1], x.shape[2], x.shape[3] + 3, device=cuda)
    wide[..., 1:-2] = x
    sl = wide[..., 1:-2]
    assert not cl.is_contiguous() and not sl.is_contiguous()
    for v in (cl, sl):
        v2 = v.reshape(R, -1)
        got = hip_ops.cut_pack(v2, 4, 128, seed) + (hip_ops.cut_roundtrip(v2, 4, 128, seed),)
        assert all(_same(a, r) for a, r in zip(got, twin(8, stochastic)))
        pk = snn.cut_pack(v, 4, 128, seed)
        assert _same(pk.payload, twin(8, stochastic)[0]) and _same(snn.cut_unpack(pk).view(R, -1), twin(8, stochastic)[2])


# ---------------------------------------------------------------- 4. the module
def _run_module(c, dy, dev, x_grad=True, calls=2):
    layer = snn.CutCodec(c["bits"], 12 - c["bits"], c["group"], seed=11).to(dev)
    out = []
    for _ in range(calls):
        x = c["x"].clone().to(dev).requires_grad_(x_grad)       # a leaf of its own, never the shared case
        y = layer(x)
        if y.requires_grad:
            y.backward(dy.to(dev))
        out.append((y.detach().cpu(), None if x.grad is None else x.grad.cpu()))
    return out


@pytest.mark.parametrize("i", [0, 1, 8])
def test_module_matches_the_cpu(cuda, i, monkeypatch):
    c = case(i)
    dy = torch.randn(c["x"].shape, generator=torch.Generator().manual_seed(500 + i))
    launches = []
    real = hip_ops.cut_roundtrip
    monkeypatch.setattr(hip_ops, "cut_roundtrip", lambda *a, **k: launches.append(a[1:]) or real(*a, **k))
    ref, got = _run_module(c, dy, "cpu"), _run_module(c, dy, cuda)
    assert len(launches) == 4                                   # a forward and a backward kernel per call
    for (y, dx), (ry, rdx) in zip(got, ref):
        assert _same(y, ry) and _same(dx, rdx) and y.shape == c["x"].shape
    assert not torch.equal(got[0][1], got[1][1])
    del launches[:]
    leaf = _run_module(c, dy, cuda, x_grad=False)
    assert len(launches) == 2                                   # no backward kernel
    assert all(dx is None and _same(y, ry) for (y, dx), (ry, _) in zip(leaf, ref))


# ---------------------------------------------------------------- 5. determinism
def test_pack_is_bitwise_reproducible(cuda):
    c = case(7)
    x = c["x2d"].to(cuda)
    for seed in (None, SEED):
        a, b = hip_ops.cut_pack(x, 8, 16, seed), hip_ops.cut_pack(x, 8, 16, seed)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and a[0].any()


# ---------------------------------------------------------------- 6. a split-shaped model
class _TwinFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, bits, grad_bits, group, seed):
        ctx.cfg = (grad_bits, group, seed)
        return torch_ops.cut_roundtrip(x.reshape(x.shape[0], -1), bits, group).view(x.shape)

    @staticmethod
    def backward(ctx, dy):
        grad_bits, group, seed = ctx.cfg
        return torch_ops.cut_roundtrip(dy.reshape(dy.shape[0], -1), grad_bits, group, seed).view(dy.shape), None, None, None, None


class _TwinCodec(nn.Module):
    """CutCodec's seed schedule over the torch twin, on whatever device the tensors are on."""

    def __init__(self, bits, grad_bits, group=64, seed=0):
        super().__init__()
        self.cfg, self.seed, self.calls = (bits, grad_bits, group), seed, 0

    def forward(self, x):
        self.calls += 1
        return _TwinFn.apply(x, *self.cfg, step_seed(self.seed, 0, self.calls))


def _split_model(codec, dev):
    torch.manual_seed(0)
    return nn.Sequential(snn.FusedConv2d(1, 8), snn.FusedGroupNorm(4, 8, relu=True, pool=2), nn.Flatten(), codec,
                         snn.FusedLinear(8 * 13 * 13, 32, relu=True), snn.FusedLinear(32, 10)).to(dev)


def _train(codec, dev, steps=3):
    model = _split_model(codec, dev)
    first = [p.detach().clone() for p in model.parameters()]
    opt = FusedAdam(model.parameters(), lr=1e-3)
    g = torch.Generator().manual_seed(1)
    x = torch.rand(16, 1, 28, 28, generator=g).to(dev)
    y = torch.randint(0, 10, (16,), generator=g).to(dev)
    for _ in range(steps):
        opt.zero_grad()
        snn.softmax_cross_entropy(model(x), y).backward()
        opt.step()
    return first, [p.detach().clone() for p in model.parameters()]


def test_split_model_trains_like_the_twin(cuda):
    _, ref = _train(_TwinCodec(8, 8), cuda)
    _, ref2 = _train(_TwinCodec(8, 8), cuda)
    # the precondition: everything but the codec under test repeats itself bit for bit
    assert all(torch.equal(a, b) for a, b in zip(ref, ref2)), "the reference model does not repeat itself"
    first, got = _train(snn.CutCodec(8, 8), cuda)
    assert len(got) == len(ref) == 8
    assert all(not torch.equal(p, f) for p, f in zip(got, first))
    for n, (p, r) in enumerate(zip(got, ref)):
        assert torch.equal(p, r), f"parameter {n}: max difference {(p - r).abs().max().item():.3e}"
