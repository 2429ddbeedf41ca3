"""The cut sparsifier on an MI355X: the kernels of csrc/cuttopk.hip (extension module `_C2`) against
the torch twin on the same GPU tensors.

Every comparison is exact, and on bit patterns where a signed zero could hide a difference: the
kernels select and copy, they compute nothing.  Shapes and inputs come from
tests/test_cuttopk_cpu.py, where the twin itself is checked against a brute-force selection."""
import pytest
import torch
from torch import nn

from splitlearning_amd import nn as snn
from splitlearning_amd.ops import hip_ops, torch_ops
from splitlearning_amd.optim import FusedAdam
from test_cuttopk_cpu import CASES, L, SHAPES, bits, make_dy, make_input

pytestmark = pytest.mark.gpu


def _same(a, r):
    if a.shape != r.shape or a.dtype != r.dtype:
        return False
    return torch.equal(bits(a), bits(r)) if a.dtype == torch.float32 else torch.equal(a, r)


def _all_ops(K_, x, d, k):
    """Every entry of the op set K_ (hip_ops or torch_ops) on the device tensors x and d."""
    values, indices = K_.cut_topk(x, k)
    y, indices2 = K_.cut_topk_dense(x, k)
    return dict(values=values, indices=indices, dense=y, dense_indices=indices2,
                scatter=K_.cut_scatter(values, indices, x.shape[1]), gather=K_.cut_gather(d, indices),
                mask=K_.cut_mask(d, indices))


def _check(x, d, k, what):
    got, ref = _all_ops(hip_ops, x, d, k), _all_ops(torch_ops, x, d, k)
    assert got["indices"].dtype == torch.int32
    for name in ref:
        if not _same(got[name], ref[name]):
            bad = (got[name] != ref[name]).nonzero() if got[name].shape == ref[name].shape else None
            pytest.fail(f"{what} {name}: {tuple(got[name].shape)} {got[name].dtype} against {tuple(ref[name].shape)} "
                        f"{ref[name].dtype}; {0 if bad is None else bad.shape[0]} elements differ, the first at "
                        f"{bad[0].tolist() if bad is not None and bad.numel() else None}")
    return got


def _at_offset(t, off, dev):
    """A contiguous device copy of t that starts `off` elements into a larger, 16-byte aligned buffer."""
    buf = torch.empty(t.numel() + 4, device=dev, dtype=t.dtype)
    assert buf.data_ptr() % 16 == 0
    v = buf[off:off + t.numel()].view(t.shape)
    v.copy_(t)
    return v


# ---------------------------------------------------------------- 1. equality with the twin
def test_the_second_module(cuda):
    c2 = hip_ops.C2()
    assert c2.arch == "gfx950" and c2.cut_topk_lds_floats == L == hip_ops.CUT_TOPK_LDS_FLOATS


@pytest.mark.parametrize("i,name", CASES)
def test_kernels_equal_the_twin(cuda, i, name):
    x = make_input(i, name).to(cuda)
    assert x.data_ptr() % 16 == 0
    _check(x, make_dy(i).to(cuda), SHAPES[i][2], f"{SHAPES[i]} {name}")


@pytest.mark.parametrize("i,name", CASES)
def test_views_inside_their_storage(cuda, i, name):
    """x and dy 1, 2 and 3 floats into their storage: every row phase moves, the results do not."""
    x, d, k = make_input(i, name), make_dy(i), SHAPES[i][2]
    for off in (1, 2, 3):
        xo, do = _at_offset(x, off, cuda), _at_offset(d, 4 - off, cuda)
        assert xo.data_ptr() % 16 == 4 * off and xo.is_contiguous()
        got = _check(xo, do, k, f"{SHAPES[i]} {name} at offset {off}")
        # the wire tensors inside their storage too
        vo, io = _at_offset(got["values"], off, cuda), _at_offset(got["indices"], off, cuda)
        assert _same(hip_ops.cut_scatter(vo, io, x.shape[1]), got["scatter"])
        assert _same(hip_ops.cut_mask(do, io), got["mask"]) and _same(hip_ops.cut_gather(do, io), got["gather"])


# ---------------------------------------------------------------- 2. determinism
@pytest.mark.parametrize("i,name", [(11, "normal"), (11, "ints"), (14, "lowbyte"), (13, "zeros")])
def test_two_runs_agree_bitwise(cuda, i, name):
    x, d, k = make_input(i, name).to(cuda), make_dy(i).to(cuda), SHAPES[i][2]
    a, b = _all_ops(hip_ops, x, d, k), _all_ops(hip_ops, x, d, k)
    assert all(_same(a[n], b[n]) for n in a) and bool(a["mask"].any())


# ---------------------------------------------------------------- 3. the module
def _run_module(x, dy, k, dev, grad_mask=True):
    layer = snn.CutTopK(k=k, grad_mask=grad_mask).to(dev)
    x = x.clone().to(dev).requires_grad_(True)                  # a leaf of its own, never the shared input
    y = layer(x)
    y.backward(dy.to(dev))
    return y.detach().cpu(), x.grad.cpu()


@pytest.mark.parametrize("i,name", [(3, "normal"), (9, "ints"), (11, "normal"), (11, "zeros"), (13, "lowbyte")])
def test_module_matches_the_cpu(cuda, i, name, monkeypatch):
    R, K, k = SHAPES[i]
    shape = (R, 2, K // 2) if K % 2 == 0 else (R, K)
    x, dy = make_input(i, name).view(shape), make_dy(i).view(shape)
    launches = []
    for fn in ("cut_topk_dense", "cut_mask"):
        real = getattr(hip_ops, fn)
        monkeypatch.setattr(hip_ops, fn, lambda *a, _fn=fn, _real=real, **kw: launches.append(_fn) or _real(*a, **kw))
    ref, got = _run_module(x, dy, k, "cpu"), _run_module(x, dy, k, cuda)
    assert launches == ["cut_topk_dense", "cut_mask"]           # one kernel forward, one backward
    assert got[0].shape == shape and _same(got[0], ref[0]) and _same(got[1], ref[1])
    del launches[:]
    passed = _run_module(x, dy, k, cuda, grad_mask=False)
    assert launches == ["cut_topk_dense"] and _same(passed[0], ref[0]) and torch.equal(passed[1], dy)


def test_wire_functions(cuda):
    i = 11
    R, K, k = SHAPES[i]
    x, dy = make_input(i, "normal").view(R, 32, 13, 13), make_dy(i).view(R, 32, 13, 13)
    ref = snn.cut_sparsify(x, k)
    pk = snn.cut_sparsify(x.to(cuda), k)
    assert pk.values.is_cuda and pk.nbytes == 8 * R * k and pk.shape == x.shape
    assert _same(pk.values.cpu(), ref.values) and _same(pk.indices.cpu(), ref.indices)
    assert _same(snn.cut_densify(pk).cpu(), snn.cut_densify(ref))
    assert _same(snn.cut_sparse_grad(dy.to(cuda), pk).cpu(), snn.cut_sparse_grad(dy, ref))
    # a channels-last input reaches the kernel as the contiguous tensor it stands for
    cl = x.to(cuda).to(memory_format=torch.channels_last)
    assert not cl.is_contiguous() and _same(snn.cut_sparsify(cl, k).indices.cpu(), ref.indices)


# ---------------------------------------------------------------- 4. a split-shaped model
class _TwinFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, k):
        y, ctx.indices = torch_ops.cut_topk_dense(x, k)
        return y

    @staticmethod
    def backward(ctx, dy):
        return torch_ops.cut_mask(dy, ctx.indices), None


class _TwinTopK(nn.Module):
    """CutTopK over the torch twin, on whatever device the tensors are on."""

    def __init__(self, k):
        super().__init__()
        self.k = k

    def forward(self, x):
        return _TwinFn.apply(x, self.k)


def _train(cut, dev, steps=3):
    torch.manual_seed(0)
    model = nn.Sequential(snn.FusedLinear(64, 96, relu=True), cut, snn.FusedLinear(96, 10)).to(dev)
    first = [p.detach().clone() for p in model.parameters()]
    opt = FusedAdam(model.parameters(), lr=1e-2)
    g = torch.Generator().manual_seed(1)
    x = torch.randn(16, 64, generator=g).to(dev)
    y = torch.randint(0, 10, (16,), generator=g).to(dev)
    for _ in range(steps):
        opt.zero_grad()
        snn.softmax_cross_entropy(model(x), y).backward()
        opt.step()
    return first, [p.detach().clone() for p in model.parameters()]


def test_split_model_trains_like_the_twin(cuda):
    """FusedLinear, CutTopK, FusedLinear against the same model with the twin at the cut, to the
    same bits.  The twin model keeps the fused linear kernels, as
    test_cutcodec_gpu.py::test_split_model_trains_like_the_twin does and for its reason: the eager
    linear of set_backend("torch") sums in another order than the split-K kernels, and a selection
    downstream of a last-bit difference has no tolerance that would mean anything.  After the ReLU
    about half of a row's 96 entries are 0.0, so k = 24 cuts into the non-zero ones."""
    _, ref = _train(_TwinTopK(24), cuda)
    _, ref2 = _train(_TwinTopK(24), cuda)
    assert all(torch.equal(a, b) for a, b in zip(ref, ref2)), "the reference model does not repeat itself"
    first, got = _train(snn.CutTopK(k=24), cuda)
    assert len(got) == len(ref) == 4
    assert all(not torch.equal(p, f) for p, f in zip(got, first))
    for n, (p, r) in enumerate(zip(got, ref)):
        assert torch.equal(p, r), f"parameter {n}: max difference {(p - r).abs().max().item():.3e}"
    _, dense = _train(nn.Identity(), cuda)
    assert not torch.equal(dense[0], got[0])                    # the cut is not a pass-through


# ---------------------------------------------------------------- 5. a packet with bad indices
def test_indices_outside_the_row_are_never_stored_through(cuda):
    """A hand-made packet with indices -1 and K: y lies inside a larger buffer whose guard zones,
    before and behind, stay as they were, and the rows of y hold the valid entries only (an index
    one past a row would otherwise land in the next row).  All memory touched is allocated."""
    R, K, k, G = 3, 37, 4, 64
    c2 = hip_ops.C2()
    indices = torch.tensor([[-1, 0, 5, K], [K, 36, -1, 2], [7, -1, K, 8]], dtype=torch.int32, device=cuda)
    values = torch.arange(1.0, R * k + 1, device=cuda).view(R, k)
    d = torch.arange(100.0, 100.0 + R * K, device=cuda).view(R, K)
    want_s, want_m = torch.zeros(R, K), torch.zeros(R, K)
    for r in range(R):
        for j in range(k):
            c = int(indices[r, j])
            if 0 <= c < K:
                want_s[r, c], want_m[r, c] = float(values[r, j]), float(d[r, c])
    for fn, src, want in ((c2.cut_scatter, values, want_s), (c2.cut_mask, d, want_m)):
        buf = torch.full((G + R * K + G,), 7.0, device=cuda)
        y = buf[G:G + R * K].view(R, K)
        fn(src, indices, y)
        torch.cuda.synchronize()
        assert torch.equal(y.cpu(), want)
        assert bool((buf[:G] == 7.0).all()) and bool((buf[G + R * K:] == 7.0).all())
    out = torch.full((R, k), 7.0, device=cuda)
    c2.cut_gather(d, indices, out)
    assert torch.equal(out.cpu(), torch.where((indices.cpu() >= 0) & (indices.cpu() < K),
                                              d.cpu().gather(1, indices.cpu().long().clamp(0, K - 1)), torch.tensor(0.0)))


# ---------------------------------------------------------------- 6. refusals before a launch
def test_refusals(cuda):
    c2 = hip_ops.C2()
    R, K, k = 2, 8, 3
    x = torch.zeros(R, K, device=cuda)
    values, indices = torch.zeros(R, k, device=cuda), torch.zeros(R, k, device=cuda, dtype=torch.int32)
    y = torch.zeros(R, K, device=cuda)
    with pytest.raises(RuntimeError, match="must be a GPU tensor"):
        c2.cut_topk(x.cpu(), values, indices)
    with pytest.raises(RuntimeError, match="must be a GPU tensor"):
        c2.cut_scatter(values, indices.cpu(), y)
    with pytest.raises(RuntimeError, match="must be float32"):
        c2.cut_topk(x.double(), values, indices)
    with pytest.raises(RuntimeError, match="must be int32"):
        c2.cut_topk(x, values, indices.long())
    with pytest.raises(RuntimeError, match="1 <= k <= K"):
        c2.cut_topk(x, torch.zeros(R, K + 1, device=cuda), torch.zeros(R, K + 1, device=cuda, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="1 <= k <= K"):
        c2.cut_gather(x, torch.zeros(R, 0, device=cuda, dtype=torch.int32), torch.zeros(R, 0, device=cuda))
    with pytest.raises(RuntimeError, match="contiguous"):
        c2.cut_topk(torch.zeros(K, R, device=cuda).t(), values, indices)
    with pytest.raises(RuntimeError, match=r"\[R, k\]"):
        c2.cut_topk(x, torch.zeros(R + 1, k, device=cuda), indices)
    with pytest.raises(RuntimeError, match="shape"):
        c2.cut_topk_dense(x, torch.zeros(R, K + 1, device=cuda), values, indices)
    with pytest.raises(RuntimeError, match="2-D"):
        c2.cut_mask(x.view(-1), indices, y)
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        snn.CutTopK(k=K + 1)(x)
