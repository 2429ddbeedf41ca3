"""The cut sparsifier on the CPU: the torch twin in ops/torch_ops.py (the definition: per-row
magnitude top-k, the lowest columns winning ties at the threshold) against a brute-force selection,
and splitlearning_amd.nn.CutTopK / cut_sparsify / cut_densify / cut_sparse_grad over it.
tests/test_cuttopk_gpu.py runs the shapes and inputs built here on the HIP kernels of
csrc/cuttopk.hip (the helpers are shared).

Everything is a selection or a copy, so every comparison is exact."""
import functools
import math

import numpy as np
import pytest
import torch

from splitlearning_amd import nn as snn
from splitlearning_amd.ops import hip_ops, torch_ops

L = hip_ops.CUT_TOPK_LDS_FLOATS       # the longest row csrc/cuttopk.hip keeps in LDS

# (R, K, k)
SHAPES = [
    (1, 1, 1),                # the smallest possible input
    (2, 5, 5),                # k == K
    (3, 7, 1),                # k == 1
    (2, 64, 8),               # one wave
    (4, 255, 17),             # around the thread count
    (4, 256, 256),
    (3, 257, 100),
    (2, 1024, 1),             # a second chunk of the ordered prefix (a chunk is 256 quads = 1024 columns)
    (2, 1031, 1030),          # odd K: rows at all four 16-byte phases
    (5, 1031, 64),
    (2, 4099, 2050),          # several chunks
    (16, 5408, 338),          # the project's own cut at 1 / 16
    (2, L, 1000),             # both sides of the LDS bound
    (2, L + 1, 1000),
    (1, 40000, 39999),        # far past the LDS bound
]
GENERATORS = ("normal", "ints", "const", "lowbyte", "exponents", "zeros", "denorm")
CASES = [(i, g) for i in range(len(SHAPES)) for g in GENERATORS]


def _signs(shape, gen):
    return torch.randint(0, 2, shape, generator=gen).bool()


@functools.lru_cache(maxsize=None)
def make_input(i, name):
    """x [R, K] fp32 of shape i from generator `name`, computed once and shared (never written to)."""
    R, K, _ = SHAPES[i]
    gen = torch.Generator().manual_seed(1000 * GENERATORS.index(name) + i)
    col = torch.arange(K).expand(R, K)
    if name == "normal":                      # the general case
        return torch.randn(R, K, generator=gen)
    if name == "ints":                        # heavy ties, both signed zeros
        x = torch.randint(-3, 4, (R, K), generator=gen).float()
        return torch.where((x == 0) & _signs((R, K), gen), torch.tensor(-0.0), x)
    if name == "const":                       # one magnitude: the lowest columns win
        return torch.where(col % 2 == 0, torch.tensor(1.5), torch.tensor(-1.5)).contiguous()
    if name == "lowbyte":                     # keys differ only in the last radix pass
        j = torch.stack([torch.randperm(K, generator=gen) % 256 for _ in range(R)])
        x = 1.0 + j.float() * 2.0 ** -23
        return torch.where(_signs((R, K), gen), -x, x)
    if name == "exponents":                   # keys differ only in the first passes
        x = torch.pow(2.0, torch.randint(-60, 61, (R, K), generator=gen).float())
        return torch.where(_signs((R, K), gen), -x, x)
    if name == "zeros":                       # every key equal
        return torch.where(_signs((R, K), gen), torch.tensor(-0.0), torch.tensor(0.0)).contiguous()
    if name == "denorm":                      # the smallest keys
        x = torch.randint(0, 1 << 20, (R, K), generator=gen).to(torch.int32).view(torch.float32)
        return torch.where(_signs((R, K), gen), -x, x)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def make_dy(i):
    """A gradient of shape i, nowhere zero."""
    R, K, _ = SHAPES[i]
    d = torch.randn(R, K, generator=torch.Generator().manual_seed(77 + i))
    return torch.where(d == 0, torch.tensor(1.0), d)


@functools.lru_cache(maxsize=None)
def brute(i, name):
    """indices int64 [R, k] of an independent selection: per row, a sort on (-|x|, column)."""
    R, K, k = SHAPES[i]
    a = np.abs(make_input(i, name).numpy())
    cols = np.arange(K)
    return torch.from_numpy(np.stack([np.sort(np.lexsort((cols, -a[r]))[:k]) for r in range(R)]))


@functools.lru_cache(maxsize=None)
def twin(i, name):
    """(values, indices) of the torch twin on the CPU, computed once."""
    return torch_ops.cut_topk(make_input(i, name), SHAPES[i][2])


def bits(t):
    """The bit patterns of a float tensor: equality that tells -0.0 from 0.0."""
    return t.contiguous().view(torch.int32)


def support(i, name):
    R, K, _ = SHAPES[i]
    return torch.zeros(R, K, dtype=torch.bool).scatter_(1, brute(i, name), True)


# ---------------------------------------------------------------- 1. hand-written examples
def test_hand_written_rows():
    x = torch.tensor([[0.5, -2.0, 2.0, 0.25, -2.0], [-0.0, 0.0, -0.0, 0.0, 0.0]])
    values, indices = torch_ops.cut_topk(x, 2)
    assert indices.dtype == torch.int32 and indices.tolist() == [[1, 2], [0, 1]]       # the third |2| loses to lower columns
    assert bits(values).tolist() == bits(torch.tensor([[-2.0, 2.0], [-0.0, 0.0]])).tolist()
    y = torch_ops.cut_scatter(values, indices, 5)
    assert y.tolist() == [[0.0, -2.0, 2.0, 0.0, 0.0], [0.0] * 5]
    d = torch.arange(10.0).view(2, 5) + 1
    assert torch_ops.cut_gather(d, indices).tolist() == [[2.0, 3.0], [6.0, 7.0]]
    assert torch_ops.cut_mask(d, indices).tolist() == [[0.0, 2.0, 3.0, 0.0, 0.0], [6.0, 7.0, 0.0, 0.0, 0.0]]


def test_a_row_of_equal_keys_selects_the_first_columns():
    x = torch.where(torch.arange(40) % 3 == 0, torch.tensor(-7.0), torch.tensor(7.0)).view(1, 40)
    assert torch_ops.cut_topk(x, 13)[1].tolist() == [list(range(13))]


# ---------------------------------------------------------------- 2. the twin against brute force
@pytest.mark.parametrize("i,name", CASES)
def test_twin_equals_brute_force(i, name):
    R, K, k = SHAPES[i]
    x = make_input(i, name)
    values, indices = twin(i, name)
    assert values.shape == (R, k) and values.dtype == torch.float32
    assert indices.shape == (R, k) and indices.dtype == torch.int32
    ref = brute(i, name)
    assert torch.equal(indices.long(), ref)
    assert k == 1 or bool((indices[:, 1:] > indices[:, :-1]).all())                     # strictly ascending
    assert torch.equal(bits(values), bits(x.gather(1, ref)))                             # signs kept, zeros too


@pytest.mark.parametrize("i,name", CASES)
def test_dense_forms_agree(i, name):
    R, K, k = SHAPES[i]
    x = make_input(i, name)
    want = torch.where(support(i, name), x, torch.tensor(0.0))
    y, indices = torch_ops.cut_topk_dense(x, k)
    assert torch.equal(indices, twin(i, name)[1]) and torch.equal(bits(y), bits(want))
    pk = snn.cut_sparsify(x, k)
    assert torch.equal(bits(snn.cut_densify(pk)), bits(want))
    assert pk.nbytes == 8 * R * k and pk.shape == (R, K) and pk.k == k
    assert pk.tensors()[0] is pk.values and pk.tensors()[1] is pk.indices


@pytest.mark.parametrize("i,name", CASES)
def test_mask_is_dy_on_the_support(i, name):
    """A selected entry passes its gradient whatever its value: with `ints` and `zeros` many
    selected entries are 0.0 or -0.0, and dy is nowhere zero."""
    d = make_dy(i)
    _, indices = twin(i, name)
    sup = support(i, name)
    dx = torch_ops.cut_mask(d, indices)
    assert torch.equal(bits(dx), bits(torch.where(sup, d, torch.tensor(0.0))))
    assert int((dx != 0).sum()) == SHAPES[i][0] * SHAPES[i][2]
    assert torch.equal(torch_ops.cut_gather(d, indices), d[sup].view(indices.shape))
    pk = snn.cut_sparsify(make_input(i, name), SHAPES[i][2])
    assert torch.equal(snn.cut_sparse_grad(d, pk), d[sup].view(indices.shape))


# ---------------------------------------------------------------- 3. the module
@pytest.mark.parametrize("i,name", [(3, "normal"), (9, "ints"), (11, "normal"), (11, "zeros"), (13, "lowbyte")])
def test_module_gradients(i, name):
    R, K, k = SHAPES[i]
    d, sup = make_dy(i), support(i, name)
    for grad_mask in (True, False):
        layer = snn.CutTopK(k=k, grad_mask=grad_mask)
        x = make_input(i, name).clone().requires_grad_(True)
        y = layer(x)
        y.backward(d)
        assert torch.equal(bits(y.detach()), bits(torch.where(sup, x.detach(), torch.tensor(0.0))))
        assert torch.equal(x.grad, torch.where(sup, d, torch.tensor(0.0)) if grad_mask else d)


def test_module_on_a_4d_input_in_train_and_eval():
    x = torch.randn(3, 2, 5, 4, generator=torch.Generator().manual_seed(5))
    layer = snn.CutTopK(ratio=0.25)
    y = layer(x)
    assert y.shape == x.shape and layer.k_for(40) == 10
    want, _ = torch_ops.cut_topk_dense(x.view(3, -1), 10)
    assert torch.equal(y.view(3, -1), want) and int((y != 0).sum()) == 30
    assert torch.equal(layer.eval()(x), y) and torch.equal(layer.train()(x), y)
    assert not y.requires_grad and layer(x.requires_grad_(True)).requires_grad


def test_ratio_to_k():
    assert [snn.CutTopK(ratio=r).k_for(K) for r, K in
            [(1.0, 7), (0.5, 7), (1 / 16, 5408), (1e-9, 100), (0.125, 8), (0.126, 8), (1, 3)]] == [7, 4, 338, 1, 1, 2, 3]
    assert snn.CutTopK(k=5).k_for(5) == 5 and snn.CutTopK(k=5).k_for(5408) == 5
    for r, K in [(0.3, 10), (0.7, 33), (1 / 3, 3)]:
        assert snn.CutTopK(ratio=r).k_for(K) == max(1, math.ceil(r * K))


@pytest.mark.parametrize("kw", [dict(), dict(k=3, ratio=0.5), dict(k=0), dict(k=-1), dict(k=2.0), dict(k=True),
                                dict(ratio=0.0), dict(ratio=1.5), dict(ratio=-0.1), dict(ratio="half"),
                                dict(ratio=True)])
def test_constructor_refusals(kw):
    with pytest.raises(ValueError):
        snn.CutTopK(**kw)


def test_call_refusals():
    x = torch.zeros(2, 6)
    with pytest.raises(ValueError):
        snn.CutTopK(k=7)(x)                                   # k > K, known at forward only
    with pytest.raises(ValueError):
        snn.CutTopK(k=1)(torch.zeros(6))                      # at least 2 dimensions
    with pytest.raises(ValueError):
        snn.CutTopK(k=1)(x.double())
    for k in (0, 7, 1.0, True):
        with pytest.raises(ValueError):
            snn.cut_sparsify(x, k)
    with pytest.raises(ValueError):
        snn.cut_sparsify(x.half(), 1)
    with pytest.raises(ValueError):
        snn.cut_sparse_grad(torch.zeros(2, 5), snn.cut_sparsify(x, 2))
    with pytest.raises(ValueError):
        torch_ops.cut_topk(x, 7)
    with pytest.raises(ValueError):
        torch_ops.cut_topk(x.view(2, 3, 2), 1)


def test_no_parameters_no_buffers():
    layer = snn.CutTopK(k=4)
    assert list(layer.parameters()) == [] and list(layer.buffers()) == [] and layer.state_dict() == {}
    model = torch.nn.Sequential(torch.nn.Linear(4, 8), layer, torch.nn.Linear(8, 2))
    assert sorted(model.state_dict()) == ["0.bias", "0.weight", "2.bias", "2.weight"]
    assert "k=4" in repr(layer) and "ratio=0.5" in repr(snn.CutTopK(ratio=0.5))


def test_public_names():
    for n in ("CutTopK", "CutSparsePacket", "cut_sparsify", "cut_densify", "cut_sparse_grad"):
        assert n in snn.__all__ and hasattr(snn, n)
    assert "CutTopK" in snn.__doc__ and "cut_sparsify" in snn.__doc__
    for n in ("cut_topk", "cut_scatter", "cut_gather", "cut_topk_dense", "cut_mask", "C2"):
        assert hasattr(hip_ops, n) and (n == "C2" or hasattr(torch_ops, n))


def test_wire_functions_do_not_differentiate():
    x = torch.randn(2, 9, generator=torch.Generator().manual_seed(3)).requires_grad_(True)
    pk = snn.cut_sparsify(x, 3)
    assert not pk.values.requires_grad and not snn.cut_densify(pk).requires_grad
    assert not snn.cut_sparse_grad(torch.ones(2, 9, requires_grad=True), pk).requires_grad


# ---------------------------------------------------------------- 4. composition with the codec
def test_the_values_of_a_packet_go_through_the_codec():
    """The [B, k] values are an ordinary fp32 tensor: cut_pack quantises them as they are, and the
    round trip is within half a step of each group (1e-3 of a step for the fp32 roundings, as in
    tests/test_cutcodec_cpu.py).  At k = K / 8 the two together are 0.63 bytes per element."""
    i = 11
    R, K, k = SHAPES[i]
    pk = snn.cut_sparsify(make_input(i, "normal").view(R, 2, 52, 52), k * 2)
    q = snn.cut_pack(pk.values, 8, 64)
    assert q.shape == (R, 2 * k) and q.payload.dtype == torch.int8
    back = snn.cut_unpack(q)
    step = q.scales.repeat_interleave(64, dim=1)[:, :2 * k]
    assert bool(((back - pk.values).abs() <= (0.5 + 1e-3) * step).all())
    y = snn.cut_densify(snn.CutSparsePacket(back, pk.indices, pk.shape, pk.k))
    assert y.shape == (R, 2, 52, 52) and int((y != 0).sum()) <= R * 2 * k
    assert 2 * k == K // 8 and 0.63 <= (q.nbytes + pk.indices.numel() * 4) / (R * K) < 0.64
