"""FusedGroupNorm on an MI355X: the kernels of csrc/groupnorm.hip against float64 on the CPU.

Tolerances.  rtol = atol = 1e-4 is the project's bound for FusedConv2d against torch; eager fp32
and a two-pass fp32 formula are within 5e-7 of float64 (relative to the tensor's maximum) on
these shapes.  The large-mean bound of 1e-3 (max |a - ref| / max |ref|) lies between what a
two-pass fp32 variance gives on x = 1000 + randn (at most 2.9e-4, worst on dweight, over 3
seeds on the CPU) and what the one-pass E[x^2] - mean^2 form gives (at least 2.6e-2 on y).

SHAPES[8:] exist for the launch geometry: the re-read form under pooling and at odd span phases, both sides
of the LDS bound (n + 3 <= 16000 floats), and a wave's second channel in pass A; keep them in any edit of the table."""
import pytest
import torch
import torch.nn.functional as F
from torch import nn

from splitlearning_amd import nn as snn
from splitlearning_amd.ops import hip_ops, torch_ops
from splitlearning_amd.optim import FusedAdam
from test_groupnorm_cpu import (EPS, SHAPES, VARIANTS, assert_decision_margins, float_case, make_layer, run_layer, stats64,
                                torch_ref)
from test_optim_cpu import assert_params_close

pytestmark = pytest.mark.gpu

NAMES = ("y", "dx", "dw", "db", "mean", "rstd")


def _fused(c, dev):
    """(y, dx, dw, db, mean, rstd) of the HIP kernels for a case, on the CPU."""
    y, dx, dw, db = run_layer(c, dev)
    w, b = (None, None) if c["w"] is None else (c["w"].to(dev), c["b"].to(dev))
    _, mean, rstd, _ = hip_ops.group_norm_fwd(c["x"].to(dev), w, b, c["groups"], EPS, c["relu"], c["pool"])
    return y, dx, dw, db, mean.cpu(), rstd.cpu()


def _torch_fp32(c, dev):
    """(y, dx, dw, db) of eager fp32 torch on the GPU, for the failure message."""
    x = c["x"].to(dev).requires_grad_(True)
    w, b = (None, None) if c["w"] is None else (c["w"].to(dev).requires_grad_(True), c["b"].to(dev).requires_grad_(True))
    y = F.group_norm(x, c["groups"], w, b, EPS)
    y = F.relu(y) if c["relu"] else y
    y = F.max_pool2d(y, 2, 2) if c["pool"] else y
    y.backward(c["g"].to(dev))
    return y.detach().cpu(), x.grad.cpu(), None if w is None else w.grad.cpu(), None if w is None else b.grad.cpu()


def _check_close(c, dev, label):
    got = _fused(c, dev)
    bad = []
    for name, a in zip(NAMES, got):
        r = c[name]
        if r is None:
            assert a is None, name
            continue
        assert a.shape == r.shape and a.dtype == torch.float32, name
        err = (a.double() - r).abs().max().item()
        print(f"{label} {name}: max |fused - fp64| {err:.3e} (max |fp64| {r.abs().max().item():.3e})")
        if not torch.allclose(a.double(), r, rtol=1e-4, atol=1e-4):
            bad.append(name)
    if bad:
        ref32 = dict(zip(NAMES, _torch_fp32(c, dev)))
        msg = [f"{n}: fused off fp64 by {(dict(zip(NAMES, got))[n].double() - c[n]).abs().max().item():.3e}"
               + (f", torch fp32 by {(ref32[n].double() - c[n]).abs().max().item():.3e}" if n in ref32 else "")
               for n in bad]
        pytest.fail(f"{label} beyond rtol = atol = 1e-4: " + "; ".join(msg))


# ---------------------------------------------------------------- 1. random floats
@pytest.mark.parametrize("i", range(len(SHAPES)))
def test_random_floats_match_float64(cuda, i):
    c = float_case(i)
    assert_decision_margins(c, f"S{i + 1}")
    _check_close(c, cuda, f"S{i + 1}")


# ---------------------------------------------------------------- 2. variants
@pytest.mark.parametrize("i,relu,affine", VARIANTS)
def test_variants_match_float64(cuda, i, relu, affine):
    c = float_case(i, relu, affine)
    assert_decision_margins(c, f"S{i + 1}")
    _check_close(c, cuda, f"S{i + 1} relu={relu} affine={affine}")


# ---------------------------------------------------------------- 2a. the LDS bound
def test_lds_bound_forms_agree(cuda):
    """Both sides of the bound between the two span forms, each against its own float64 reference
    (mean and rstd included): the same x, one float per channel shorter, moves from one to the other."""
    # csrc/groupnorm.h: kGroupNormLdsFloats = 16000, and a span of n floats stays in LDS while n + 3 <= 16000.
    # If that constant changes, these shapes no longer straddle the bound: change them (and S10, S11) with it.
    lds_floats = 16000
    B, C, G = 2, 4, 2
    cpg = C // G
    L = (lds_floats - 3) // cpg + 1                       # 7999: n = 15998 is re-read, L - 1 gives n = 15996 in LDS
    assert cpg * (L - 1) + 3 <= lds_floats < cpg * L + 3
    assert SHAPES[10] == (B, C, G, (L,), None)
    above = float_case(10)
    cut = lambda t: t[..., :L - 1].contiguous()
    x, g = cut(above["x"]), cut(above["g"])
    y, dx, dw, db = torch_ref(x.double(), above["w"].double(), above["b"].double(), g.double(), G, True, None)
    mean, rstd = stats64(x, G)
    below = dict(above, x=x, g=g, y=y, dx=dx, dw=dw, db=db, mean=mean, rstd=rstd)
    for label, c in ((f"n = {cpg * L}, re-read", above), (f"n = {cpg * (L - 1)}, in LDS", below)):
        assert c["x"].shape == (B, C, c["x"].shape[2]) and c["x"].is_contiguous()
        assert_decision_margins(c, label)
        _check_close(c, cuda, label)


# ---------------------------------------------------------------- 2b. misaligned base pointers
def _at_offset(t, off, dev):
    """A contiguous device copy of t that starts `off` elements into a larger, 16-byte aligned buffer."""
    buf = torch.empty(t.numel() + 4, device=dev, dtype=t.dtype)
    assert buf.data_ptr() % 16 == 0
    v = buf[off:off + t.numel()].view(t.shape)
    v.copy_(t)
    return v


@pytest.mark.parametrize("i", [0, 11])
def test_misaligned_base_pointers(cuda, i):
    """x one float and dy three floats into their storage (hip_ops hands such contiguous views to the
    kernels as they are: no copy), against float64 at the tolerance of the other tests.

    Not bitwise against the run on ordinarily allocated copies: gn_sweep's split into head, float4s
    and tail follows the pointer's phase, so which elements a thread adds up, and with that the
    rounding of every sum, follows it too.  Seen on an MI355X: y, mean, dx, dw and db differ from the
    aligned run by at most 4.8e-7 (dw and db of S1, one unit in the last place), rstd and am not at
    all; the offset run is within 1.4e-6 of float64.  The difference from the aligned run is printed."""
    c = float_case(i)
    assert_decision_margins(c, f"S{i + 1}")
    G, pool = c["groups"], c["pool"]
    w, b = c["w"].to(cuda), c["b"].to(cuda)

    def run(x, dy):
        y, mean, rstd, am = hip_ops.group_norm_fwd(x, w, b, G, EPS, True, pool)
        dx, dw, db = hip_ops.group_norm_bwd(dy, x, mean, rstd, w, b, am, G, True, pool, True)
        return dict(y=y, am=am, mean=mean, rstd=rstd, dx=dx, dw=dw, db=db)

    x1, dy3 = _at_offset(c["x"], 1, cuda), _at_offset(c["g"], 3, cuda)
    assert x1.data_ptr() % 16 == 4 and dy3.data_ptr() % 16 == 12
    assert x1.is_contiguous() and dy3.is_contiguous()
    x0, dy0 = c["x"].to(cuda), c["g"].to(cuda)
    assert x0.data_ptr() % 16 == 0 and dy0.data_ptr() % 16 == 0
    ref, got = run(x0, dy0), run(x1, dy3)
    assert (got["am"] is None) == (pool is None)
    bad = []
    for name in ("y", "am", "mean", "rstd", "dx", "dw", "db"):
        if got[name] is None:
            continue
        a, r = got[name].cpu(), ref[name].cpu()
        assert a.shape == r.shape and a.dtype == r.dtype, name
        if name == "am":
            assert torch.equal(a, r) and torch.equal(a, torch_ops.group_norm_fwd(c["x"], c["w"], c["b"], G, EPS, True, pool)[3])
            continue
        print(f"S{i + 1} {name}: max |offset - aligned| {(a - r).abs().max().item():.3e}, "
              f"max |offset - fp64| {(a.double() - c[name]).abs().max().item():.3e}")
        if not torch.allclose(a.double(), c[name], rtol=1e-4, atol=1e-4):
            bad.append(name)
    assert not bad, f"beyond rtol = atol = 1e-4 of float64: {bad}"


# ---------------------------------------------------------------- 3. large mean
@pytest.mark.parametrize("i", [0, 1, 2, 3])
def test_large_mean_input(cuda, i):
    c = float_case(i, relu=False, affine=True, pooled=False, offset=1000.0)
    assert c["pool"] is None and c["x"].mean() > 990
    got = dict(zip(NAMES, _fused(c, cuda)))
    errs = {n: ((got[n].double() - c[n]).abs().max() / c[n].abs().max()).item() for n in ("y", "dx", "dw", "db")}
    print(f"S{i + 1} x = 1000 + randn: max |a - fp64| / max |fp64| = " + ", ".join(f"{n} {e:.3e}" for n, e in errs.items()))
    assert all(e <= 1e-3 for e in errs.values()), errs


# ---------------------------------------------------------------- 4. argmax and ties
@pytest.mark.parametrize("i", [1, 4, 8, 11])
def test_argmax_positions_match_torch_ops(cuda, i):
    c = float_case(i)
    assert_decision_margins(c, f"S{i + 1}")
    y, mean, rstd, am = hip_ops.group_norm_fwd(c["x"].to(cuda), c["w"].to(cuda), c["b"].to(cuda), c["groups"], EPS, True, 2)
    ry, _, _, ram = torch_ops.group_norm_fwd(c["x"], c["w"], c["b"], c["groups"], EPS, True, 2)
    assert am.dtype == torch.uint8 and am.shape == y.shape == ry.shape
    assert torch.equal(am.cpu(), ram)
    torch.testing.assert_close(y.cpu(), ry, rtol=1e-4, atol=1e-4)


def test_all_equal_windows_route_to_position_zero(cuda):
    # sums of the integer 2 are exact: mean = 2 and xh = 0 bitwise, so z = bias = 1 everywhere
    x = torch.full((2, 4, 6, 6), 2.0, device=cuda)
    layer = snn.FusedGroupNorm(2, 4, relu=True, pool=2).to(cuda)
    with torch.no_grad():
        layer.weight.zero_()
        layer.bias.fill_(1.0)
    y, mean, rstd, am = hip_ops.group_norm_fwd(x, layer.weight, layer.bias, 2, EPS, True, 2)
    assert torch.equal(y.cpu(), torch.ones(2, 4, 3, 3)) and torch.equal(layer(x), y) and not am.any()
    assert torch.equal(mean.cpu(), torch.full((2, 2), 2.0))
    # weight = 1 in the backward shows where dz landed: dx = rstd * (dz - mean(dz)), dz = 2 on a quarter
    dy, one = torch.full_like(y, 2.0), torch.ones(4, device=cuda)
    dx, dw, db = hip_ops.group_norm_bwd(dy, x, mean, rstd, one, one, am, 2, True, 2, True)
    rs = rstd.cpu().reshape(2, 2, 1, 1, 1)
    ref = torch.full((2, 2, 2, 6, 6), -0.5) * rs
    ref[..., ::2, ::2] = 1.5 * rs
    torch.testing.assert_close(dx.cpu(), ref.reshape(2, 4, 6, 6), rtol=1e-6, atol=0)
    assert torch.equal(db.cpu(), torch.full((4,), 36.0)) and not dw.any()
    rdx, rdw, rdb = torch_ops.group_norm_bwd(dy.cpu(), x.cpu(), mean.cpu(), rstd.cpu(), one.cpu(), one.cpu(), am.cpu(),
                                             2, True, 2, True)
    torch.testing.assert_close(dx.cpu(), rdx, rtol=1e-4, atol=1e-4)
    assert torch.equal(db.cpu(), rdb)


# ---------------------------------------------------------------- 5. dropped pixels
def test_dropped_column_counts_in_the_statistics(cuda):
    c = float_case(1)                           # 7 x 9: row 6 and column 8 are in no window
    args = (c["w"].to(cuda), c["b"].to(cuda), c["groups"], EPS, True, 2)
    x = c["x"].to(cuda)
    y, mean, rstd, _ = hip_ops.group_norm_fwd(x, *args)
    x2 = x.clone()
    x2[..., -1] += 3.0
    y2, mean2, rstd2, _ = hip_ops.group_norm_fwd(x2, *args)
    assert (mean2 - mean).abs().min() > 1e-3 and (rstd2 - rstd).abs().min() > 1e-4
    assert (y2 - y).abs().max() > 1e-3
    _, dx, _, _ = run_layer(c, cuda)
    assert (dx[..., -1] != 0).all() and (dx[:, :, -1, :] != 0).all()
    torch.testing.assert_close(dx[..., -1].double(), c["dx"][..., -1], rtol=1e-4, atol=1e-4)


# ---------------------------------------------------------------- 6. determinism
def test_backward_is_bitwise_reproducible(cuda):
    c = float_case(4)
    layer = make_layer(c, cuda)
    x, g = c["x"].to(cuda), c["g"].to(cuda)
    runs = []
    for _ in range(2):
        layer.zero_grad()
        xr = x.clone().requires_grad_(True)
        layer(xr).backward(g)
        runs.append((xr.grad.clone(), layer.weight.grad.clone(), layer.bias.grad.clone()))
    for a, b in zip(*runs):
        assert a.abs().max() > 0 and torch.equal(a, b)


# ---------------------------------------------------------------- 7. leaf input
def test_leaf_input_gets_no_gradient(cuda):
    c = float_case(4)
    y, dx, dw, db = run_layer(c, cuda, x_grad=False)
    y2, dx2, dw2, db2 = run_layer(c, cuda)
    assert dx is None and dx2 is not None
    assert torch.equal(y, y2) and torch.equal(dw, dw2) and torch.equal(db, db2)


# ---------------------------------------------------------------- 8. non-contiguous input
def test_non_contiguous_input(cuda):
    c = float_case(1)
    ref = run_layer(c, cuda)
    x = c["x"].to(cuda)
    cl = x.to(memory_format=torch.channels_last)
    assert not cl.is_contiguous()
    assert all(torch.equal(a, r) for a, r in zip(run_layer(c, cuda, x=cl), ref))
    wide = torch.zeros(x.shape[0], x.shape[1], x.shape[2], x.shape[3] + 3, device=cuda)
    wide[..., 1:-2] = x
    sl = wide[..., 1:-2]
    assert not sl.is_contiguous()
    assert all(torch.equal(a, r) for a, r in zip(run_layer(c, cuda, x=sl), ref))


# ---------------------------------------------------------------- 9. a stacked model
def _stacked(dev):
    torch.manual_seed(0)
    return nn.Sequential(snn.FusedConv2d(1, 8), snn.FusedGroupNorm(4, 8, relu=True, pool=2),
                         snn.FusedConv2d(8, 16, padding=1), snn.FusedGroupNorm(4, 16, relu=True, pool=2),
                         nn.Flatten(), snn.FusedLinear(16 * 6 * 6, 32, relu=True), snn.FusedLinear(32, 10)).to(dev)


def _stacked_torch(dev):
    return nn.Sequential(nn.Conv2d(1, 8, 3), nn.GroupNorm(4, 8), nn.ReLU(), nn.MaxPool2d(2, 2),
                         nn.Conv2d(8, 16, 3, padding=1), nn.GroupNorm(4, 16), nn.ReLU(), nn.MaxPool2d(2, 2),
                         nn.Flatten(), nn.Linear(16 * 6 * 6, 32), nn.ReLU(), nn.Linear(32, 10)).to(dev)


def test_stacked_model_trains_like_torch(cuda):
    model, ref = _stacked(cuda), _stacked_torch(cuda)
    assert len(list(model.parameters())) == len(list(ref.parameters())) == 12
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
    assert all(not torch.equal(p, f) for p, f in zip(model.parameters(), first))
    assert_params_close(list(model.parameters()), list(ref.parameters()), rtol=1e-4, atol=1e-4)
