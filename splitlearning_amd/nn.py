"""Autograd-aware modules over the framework's kernels, for user-written models.

The engines (engine/) drive the reference architectures without autograd: they know
the whole step and fuse it. A user who builds a different split model out of ordinary
`nn.Module`s and trains it with `loss.backward()` and an optimizer can use these layers
instead, and still gets the fused kernels on an MI355X; `splitlearning_amd.optim.FusedSGD`
/ `FusedAdam` are the matching optimizers (one launch per parameter group, optional global
gradient-norm clipping), and any `torch.optim` optimizer works too:

* `FusedLinear`: Linear + optional ReLU + optional dropout in one forward kernel
  (the skinny split-K MFMA GEMM for batches <= 128, hipBLASLt + fused epilogue above).
  Backward is the dgrad kernel plus the wgrad kernel. Dropout masks come from a
  counter hash, so they are regenerated in backward instead of stored.
* `FusedConvFront`: `model1_sisa`'s Conv2d(1,32,3) + ReLU + MaxPool(2) + flatten, with
  the uint8 gather fused into the forward (models.py:16-30).
* `FusedConv2d`: `nn.Conv2d(in, out, 3, padding=0|1)` + optional ReLU + optional
  MaxPool2d(2, 2) for any channel count and image size, as implicit-GEMM MFMA kernels.  The
  output stays 4-D and the input gets a gradient when it requires one, so the layer can be
  stacked or start a server part.  The un-pooled activation is never stored.
* `FusedGroupNorm`: `nn.GroupNorm(groups, channels)` + optional ReLU + optional MaxPool2d(2, 2)
  as one kernel per pass, for any [B, C, *] input.  After a `FusedConv2d` it makes conv, norm,
  ReLU and pool two kernels per direction with no un-pooled activation stored.  It keeps no
  buffers, so weight relay, snapshots and unlearning carry a model that uses it as they are.
* `softmax_cross_entropy`: mean CrossEntropyLoss as one fused forward+backward kernel.
* `CutCodec`: the cut itself.  What crosses it is block-quantised to int8 or int4 with one fp32
  scale per group of a row: the activation to the nearest step, its gradient with stochastic
  (unbiased) rounding, one streaming kernel each.  `cut_pack` / `cut_unpack` produce and read the
  wire tensors (`CutPacket`) for a transport.  No parameters and no buffers.
* `CutTopK`: the cut, sparsified.  Only the k largest-magnitude entries of each sample cross it
  (ties at the threshold: the lowest positions, so runs repeat bit for bit) and the gradient comes
  back on the same support: one radix-select kernel forward, one masking kernel backward.
  `cut_sparsify` / `cut_densify` / `cut_sparse_grad` produce and read the wire tensors
  (`CutSparsePacket`: values + int32 positions); the values are an ordinary tensor that `cut_pack`
  quantises further.  No parameters and no buffers.

On CPU tensors the same layers run the eager torch implementations (ops/torch_ops.py),
so a model is written once. State-dict keys match `nn.Linear` / `nn.Conv2d` / `nn.GroupNorm` /
`model1_sisa`.
"""
from __future__ import annotations

import math
from dataclasses import dataclass

import torch
from torch import nn

from . import ops
from .ops.rng import step_seed


def _keep_scale(drop: float) -> float:
    return 1.0 / (1.0 - drop) if drop else 1.0


def _linear_impl(x):
    """The skinny kernels stream float4 rows: K % 4 == 0. Other widths use the eager path."""
    if x.shape[-1] % 4:
        return ops.torch_ops
    return ops.impl(x.device)


class _LinearFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, relu: bool, drop: float, seed: int):
        K = _linear_impl(x)
        x = x.contiguous()
        y = K.linear_fwd(x, weight.detach(), bias.detach() if bias is not None else None, relu, drop, seed, 0)
        ctx.save_for_backward(x, weight, y)
        ctx.relu, ctx.drop, ctx.has_bias = relu, drop, bias is not None
        return y

    @staticmethod
    def backward(ctx, dy):
        x, weight, y = ctx.saved_tensors
        K = _linear_impl(x)
        dz = dy.contiguous()
        if ctx.relu or ctx.drop:
            # y > 0 <=> (kept by dropout) and (ReLU active, when there is a ReLU)
            mask = (y > 0) if ctx.relu else (y != 0)
            dz = dz * mask * _keep_scale(ctx.drop)
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            dx = K.linear_dgrad(dz, weight.detach())
        if ctx.needs_input_grad[1] or (ctx.has_bias and ctx.needs_input_grad[2]):
            dw, db = K.linear_wgrad(dz.contiguous(), x)
        return dx, dw, (db if ctx.has_bias else None), None, None, None


class FusedLinear(nn.Module):
    """`nn.Linear(in, out)` [+ ReLU] [+ Dropout(p)] as one kernel per pass."""

    def __init__(self, in_features: int, out_features: int, bias: bool = True, relu: bool = False,
                 dropout: float = 0.0, seed: int = 0):
        super().__init__()
        self.in_features, self.out_features = in_features, out_features
        self.relu, self.dropout, self.seed = relu, float(dropout), seed
        self.weight = nn.Parameter(torch.empty(out_features, in_features))
        self.bias = nn.Parameter(torch.empty(out_features)) if bias else None
        self.calls = 0
        self.reset_parameters()

    def reset_parameters(self):
        # nn.Linear's default init (kaiming-uniform a=sqrt(5), uniform bias)
        nn.init.kaiming_uniform_(self.weight, a=math.sqrt(5))
        if self.bias is not None:
            bound = 1.0 / math.sqrt(self.in_features) if self.in_features > 0 else 0.0
            nn.init.uniform_(self.bias, -bound, bound)

    def forward(self, x):
        drop = self.dropout if self.training else 0.0
        self.calls += 1
        seed = step_seed(self.seed, 0, self.calls) if drop else 0
        shape = x.shape
        y = _LinearFn.apply(x.reshape(-1, shape[-1]), self.weight, self.bias, self.relu, drop, seed)
        return y.reshape(*shape[:-1], self.out_features)

    def extra_repr(self):
        return (f"in_features={self.in_features}, out_features={self.out_features}, "
                f"relu={self.relu}, dropout={self.dropout}")


class _Conv2dFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, pad: int, relu: bool, pool):
        K = ops.impl(x.device)
        x = x.contiguous()
        y, am = K.conv3x3_fwd(x, weight.detach(), bias.detach() if bias is not None else None, pad, relu, pool)
        ctx.save_for_backward(x, weight, y, am)
        ctx.pad, ctx.relu, ctx.pool, ctx.has_bias = pad, relu, pool, bias is not None
        return y

    @staticmethod
    def backward(ctx, dy):
        x, weight, y, am = ctx.saved_tensors
        K = ops.impl(dy.device)
        dy = dy.contiguous()
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            dx = K.conv3x3_dgrad(dy, y, am, weight.detach(), ctx.pad, ctx.relu, ctx.pool, x.shape)
        if ctx.needs_input_grad[1] or (ctx.has_bias and ctx.needs_input_grad[2]):
            dw, db = K.conv3x3_wgrad(dy, y, am, x, ctx.pad, ctx.relu, ctx.pool)
        return dx, dw, (db if ctx.has_bias else None), None, None, None


class FusedConv2d(nn.Module):
    """`nn.Conv2d(in, out, 3, padding=padding)` [+ ReLU] [+ MaxPool2d(2, 2) with `pool=2`] as one
    kernel per pass.  Input [B, Cin, H, W] float32, output [B, Cout, H', W'] (never flattened).
    Parameters are named and initialised like `nn.Conv2d`'s.  Supported: kernel_size 3,
    stride 1, padding 0 or 1, pool None or 2; anything else raises ValueError."""

    def __init__(self, in_channels: int, out_channels: int, kernel_size=3, stride=1, padding=0,
                 bias: bool = True, relu: bool = False, pool=None):
        super().__init__()
        if kernel_size not in (3, (3, 3), [3, 3]):
            raise ValueError(f"FusedConv2d: kernel_size must be 3, got {kernel_size!r}")
        if stride not in (1, (1, 1), [1, 1]):
            raise ValueError(f"FusedConv2d: stride must be 1, got {stride!r}")
        if padding not in (0, 1, (0, 0), (1, 1), [0, 0], [1, 1]):
            raise ValueError(f"FusedConv2d: padding must be 0 or 1, got {padding!r}")
        if pool not in (None, 2, (2, 2), [2, 2]):
            raise ValueError(f"FusedConv2d: pool must be None or 2, got {pool!r}")
        if in_channels < 1 or out_channels < 1:
            raise ValueError("FusedConv2d: in_channels and out_channels must be >= 1")
        self.in_channels, self.out_channels = in_channels, out_channels
        self.padding = padding if isinstance(padding, int) else int(padding[0])
        self.relu, self.pool = bool(relu), (None if pool is None else 2)
        self.weight = nn.Parameter(torch.empty(out_channels, in_channels, 3, 3))
        self.bias = nn.Parameter(torch.empty(out_channels)) if bias else None
        self.reset_parameters()

    def reset_parameters(self):
        # nn.Conv2d's default init (kaiming-uniform a=sqrt(5), uniform bias over fan_in = Cin * 9)
        nn.init.kaiming_uniform_(self.weight, a=math.sqrt(5))
        if self.bias is not None:
            bound = 1.0 / math.sqrt(self.in_channels * 9)
            nn.init.uniform_(self.bias, -bound, bound)

    def forward(self, x):
        if x.dim() != 4 or x.shape[1] != self.in_channels:
            raise ValueError(f"FusedConv2d: expected [B, {self.in_channels}, H, W], got {tuple(x.shape)}")
        if x.dtype != torch.float32:
            raise ValueError(f"FusedConv2d: input must be float32, got {x.dtype}")
        ho, wo = x.shape[2] + 2 * self.padding - 2, x.shape[3] + 2 * self.padding - 2
        if x.shape[2] < 3 or x.shape[3] < 3:
            raise ValueError(f"FusedConv2d: input {tuple(x.shape[2:])} is smaller than the 3x3 kernel")
        if self.pool and (ho < 2 or wo < 2):
            raise ValueError(f"FusedConv2d: conv output {ho}x{wo} is smaller than the 2x2 pooling window")
        return _Conv2dFn.apply(x, self.weight, self.bias, self.padding, self.relu, self.pool)

    def extra_repr(self):
        return (f"in_channels={self.in_channels}, out_channels={self.out_channels}, kernel_size=3, "
                f"padding={self.padding}, relu={self.relu}, pool={self.pool}")


class _GroupNormFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, groups: int, eps: float, relu: bool, pool):
        K = ops.impl(x.device)
        x = x.contiguous()
        affine = weight is not None
        y, mean, rstd, am = K.group_norm_fwd(x, weight.detach() if affine else None, bias.detach() if affine else None,
                                             groups, eps, relu, pool)
        # y is not saved: the backward recomputes the pre-activation from x, mean and rstd
        ctx.save_for_backward(x, mean, rstd, am, weight, bias)
        ctx.groups, ctx.relu, ctx.pool = groups, relu, pool
        return y

    @staticmethod
    def backward(ctx, dy):
        x, mean, rstd, am, weight, bias = ctx.saved_tensors
        K = ops.impl(dy.device)
        affine = weight is not None
        dx, dw, db = K.group_norm_bwd(dy.contiguous(), x, mean, rstd, weight.detach() if affine else None,
                                      bias.detach() if affine else None, am, ctx.groups, ctx.relu, ctx.pool,
                                      ctx.needs_input_grad[0])
        return dx, dw, db, None, None, None, None


class FusedGroupNorm(nn.Module):
    """`nn.GroupNorm(num_groups, num_channels, eps, affine)` [+ ReLU] [+ MaxPool2d(2, 2) with
    `pool=2`] as one kernel per pass (plus the per-channel sum of the parameter gradients).
    Input [B, C, *] float32; output [B, C, *], or [B, C, H // 2, W // 2] with pooling, which needs
    a 4-D input with H, W >= 2 (an odd last row or column is left out of the output and still
    counts in the statistics).  Parameters are named and initialised like `nn.GroupNorm`'s; there
    are no buffers, and `train()` and `eval()` compute the same."""

    def __init__(self, num_groups: int, num_channels: int, eps: float = 1e-5, affine: bool = True,
                 relu: bool = False, pool=None):
        super().__init__()
        if num_groups < 1 or num_channels < 1 or num_channels % num_groups != 0:
            raise ValueError(f"FusedGroupNorm: num_channels ({num_channels}) must be a positive multiple of "
                             f"num_groups ({num_groups})")
        if pool not in (None, 2):
            raise ValueError(f"FusedGroupNorm: pool must be None or 2, got {pool!r}")
        self.num_groups, self.num_channels, self.eps, self.affine = num_groups, num_channels, float(eps), bool(affine)
        self.relu, self.pool = bool(relu), pool
        if self.affine:
            self.weight = nn.Parameter(torch.empty(num_channels))
            self.bias = nn.Parameter(torch.empty(num_channels))
        else:
            self.register_parameter("weight", None)
            self.register_parameter("bias", None)
        self.reset_parameters()

    def reset_parameters(self):
        if self.affine:
            nn.init.ones_(self.weight)
            nn.init.zeros_(self.bias)

    def forward(self, x):
        if x.dim() < 2 or x.shape[1] != self.num_channels:
            raise ValueError(f"FusedGroupNorm: expected [B, {self.num_channels}, *], got {tuple(x.shape)}")
        if x.dtype != torch.float32:
            raise ValueError(f"FusedGroupNorm: input must be float32, got {x.dtype}")
        if self.pool and (x.dim() != 4 or x.shape[2] < 2 or x.shape[3] < 2):
            raise ValueError(f"FusedGroupNorm: pool=2 needs [B, C, H, W] with H, W >= 2, got {tuple(x.shape)}")
        return _GroupNormFn.apply(x, self.weight, self.bias, self.num_groups, self.eps, self.relu, self.pool)

    def extra_repr(self):
        return (f"{self.num_groups}, {self.num_channels}, eps={self.eps}, affine={self.affine}, "
                f"relu={self.relu}, pool={self.pool}")


class _ConvFrontFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias):
        K = ops.impl(x.device)
        B = x.shape[0]
        xf = x.reshape(B, 784).contiguous()
        idx = torch.arange(B, device=x.device)
        y, am = K.conv_front_fwd(xf, idx, weight.detach(), bias.detach())
        ctx.save_for_backward(xf, idx, weight, bias, y, am)
        return y

    @staticmethod
    def backward(ctx, dy):
        xf, idx, weight, bias, y, am = ctx.saved_tensors
        K = ops.impl(dy.device)
        dw, db = K.conv_front_bwd(dy.contiguous(), y, am, xf, idx, weight.detach(), bias.detach())
        return None, dw.view_as(weight), db.view_as(bias)


class FusedConvFront(nn.Module):
    """`model1_sisa` (Conv2d(1,32,3) -> ReLU -> MaxPool(2,2) -> Flatten) as one kernel.
    Input: [B,1,28,28] or [B,784], float32 or uint8 (raw 0-255 pixels, like the
    reference's unnormalised MNIST). Output: [B,5408]. The input gets no gradient."""

    def __init__(self):
        super().__init__()
        conv = nn.Conv2d(1, 32, 3)
        self.conv_layers = nn.Sequential(conv)      # state_dict: conv_layers.0.{weight,bias}

    def forward(self, x):
        c = self.conv_layers[0]
        return _ConvFrontFn.apply(x, c.weight, c.bias)


class _SoftmaxCEFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, labels, ignore_index: int):
        K = ops.impl(logits.device)
        n_valid = int((labels != ignore_index).sum().item())
        scale = 1.0 / max(n_valid, 1)
        loss_rows, d = K.softmax_ce(logits.contiguous(), labels.contiguous(), scale, ignore_index)
        ctx.save_for_backward(d)
        return loss_rows.sum() * scale

    @staticmethod
    def backward(ctx, g):
        (d,) = ctx.saved_tensors
        return d * g, None, None


def softmax_cross_entropy(logits, labels, ignore_index: int = -100):
    """`nn.CrossEntropyLoss()(logits, labels)` (mean over non-ignored rows)."""
    return _SoftmaxCEFn.apply(logits, labels, ignore_index)


# ------------------------------------------------------------------ the cut
_CUT_BITS = (None, 4, 8)


def _cut_args(name, bits, group, what="bits"):
    if bits not in _CUT_BITS or isinstance(bits, bool):
        raise ValueError(f"{name}: {what} must be None, 4 or 8, got {bits!r}")
    if group not in ops.torch_ops.CUT_GROUPS:
        raise ValueError(f"{name}: group must be one of {ops.torch_ops.CUT_GROUPS}, got {group!r}")


def _cut_input(name, x):
    if x.dim() < 2:
        raise ValueError(f"{name}: expected [B, *] with at least 2 dimensions, got {tuple(x.shape)}")
    if x.dtype != torch.float32:
        raise ValueError(f"{name}: input must be float32, got {x.dtype}")


class _CutFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, bits, grad_bits, group: int, seed: int):
        ctx.grad_bits, ctx.group, ctx.seed = grad_bits, group, seed
        if bits is None:
            return x.view_as(x)
        y = ops.impl(x.device).cut_roundtrip(x.reshape(x.shape[0], -1), bits, group)
        return y.view(x.shape)

    @staticmethod
    def backward(ctx, dy):
        if ctx.grad_bits is None:
            return dy, None, None, None, None
        dx = ops.impl(dy.device).cut_roundtrip(dy.reshape(dy.shape[0], -1), ctx.grad_bits, ctx.group, ctx.seed)
        return dx.view(dy.shape), None, None, None, None


class CutCodec(nn.Module):
    """The cut of a split model: what the other side receives after int8 / int4 block quantisation.

    x [B, *] float32 is read as [B, K]; each row is cut into groups of `group` (16, 32, 64, 128 or
    256) consecutive elements, the last of a row possibly short, and a group is sent as integers in
    [-qmax, qmax] (qmax = 127 at 8 bits, 7 at 4) with one fp32 scale = max |x| / qmax.  At
    group = 64 that is 1.0625 bytes per element at 8 bits and 0.5625 at 4, against 4.

    Forward: y = the dequantised activation, rounded to the nearest step (half to even); the same
    in `train()` and `eval()`, since the wire is there at inference too.  Backward: dx = the
    gradient quantised to `grad_bits` with stochastic rounding, which is unbiased; its seed is
    `step_seed(seed, 0, calls)`, `calls` counting forward calls.  `grad_bits=None` passes the
    gradient through, `bits=None` the activation.  No parameters and no buffers, so state dicts,
    weight relay, snapshots and unlearning carry a model that contains it unchanged."""

    def __init__(self, bits=8, grad_bits=8, group: int = 64, seed: int = 0):
        super().__init__()
        _cut_args("CutCodec", bits, group)
        _cut_args("CutCodec", grad_bits, group, "grad_bits")
        self.bits, self.grad_bits, self.group, self.seed = bits, grad_bits, group, seed
        self.calls = 0

    def forward(self, x):
        _cut_input("CutCodec", x)
        self.calls += 1
        if self.bits is None and self.grad_bits is None:
            return x
        return _CutFn.apply(x, self.bits, self.grad_bits, self.group, step_seed(self.seed, 0, self.calls))

    def extra_repr(self):
        return f"bits={self.bits}, grad_bits={self.grad_bits}, group={self.group}"


@dataclass
class CutPacket:
    """What `cut_pack` makes and a transport ships: `payload` (int8 [R, K] at 8 bits; uint8
    [R, ceil(K / 2)] at 4 bits, the even column in the low nibble) and `scales` (fp32
    [R, ceil(K / group)]), with the `shape` of the tensor they came from."""
    payload: torch.Tensor
    scales: torch.Tensor
    shape: tuple
    bits: int
    group: int

    @property
    def nbytes(self) -> int:
        return sum(t.numel() * t.element_size() for t in self.tensors())

    def tensors(self):
        return self.payload, self.scales


def cut_pack(x, bits: int = 8, group: int = 64, seed=None) -> CutPacket:
    """Quantise x [B, *] float32 for the wire: nearest rounding, or stochastic with a 64-bit
    `seed`.  Not differentiable (the result is integers): inside a model use `CutCodec`."""
    _cut_args("cut_pack", bits, group)
    if bits is None:
        raise ValueError("cut_pack: bits must be 4 or 8, got None")
    _cut_input("cut_pack", x)
    x = x.detach()
    payload, scales = ops.impl(x.device).cut_pack(x.reshape(x.shape[0], -1), bits, group, seed)
    return CutPacket(payload, scales, tuple(x.shape), bits, group)


def cut_unpack(packet: CutPacket) -> torch.Tensor:
    """The float32 tensor of `packet.shape` the packet stands for."""
    K = math.prod(packet.shape[1:])
    y = ops.impl(packet.payload.device).cut_unpack(packet.payload, packet.scales, K, packet.bits, packet.group)
    return y.view(packet.shape)


# ------------------------------------------------------------------ the cut, sparsified
def _topk_k(name, k, K: int) -> int:
    if k > K:
        raise ValueError(f"{name}: k = {k} exceeds the {K} elements of a sample")
    return k


class _TopKFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, k: int, grad_mask: bool):
        y, indices = ops.impl(x.device).cut_topk_dense(x.reshape(x.shape[0], -1), k)
        ctx.indices = indices if grad_mask else None
        return y.view(x.shape)

    @staticmethod
    def backward(ctx, dy):
        if ctx.indices is None:
            return dy, None, None
        dx = ops.impl(dy.device).cut_mask(dy.reshape(dy.shape[0], -1), ctx.indices)
        return dx.view(dy.shape), None, None


class CutTopK(nn.Module):
    """The cut of a split model, sparsified: only the `k` entries of largest magnitude of each
    sample cross it, and the other side sees zeros elsewhere.

    x [B, *] float32 is read as [B, K].  A sample's support is the k columns with the largest |x|;
    among equal magnitudes at the threshold the lowest columns win, so a run repeats bit for bit
    on every backend.  On the wire that is k values + k int32 positions, 8 k / K bytes per element
    against 4 (`cut_sparsify`); the values are an ordinary [B, k] tensor, so `cut_pack` quantises
    them further.  Give exactly one of `k` (an int >= 1) and `ratio` (in (0, 1]: k = max(1,
    ceil(ratio * K)) for the K of each call).

    Forward: y = x on the support and 0 elsewhere, one kernel; the same in `train()` and `eval()`,
    since the wire is there at inference too.  Backward: dx = dy on the support and 0 elsewhere, one
    kernel (what comes back over the wire is `dy` at the k positions, `cut_sparse_grad`);
    `grad_mask=False` passes the gradient through.  No parameters and no buffers, so state dicts,
    weight relay, snapshots and unlearning carry a model that contains it unchanged."""

    def __init__(self, k=None, ratio=None, grad_mask: bool = True):
        super().__init__()
        if (k is None) == (ratio is None):
            raise ValueError("CutTopK: give exactly one of k and ratio")
        if k is not None and (isinstance(k, bool) or not isinstance(k, int) or k < 1):
            raise ValueError(f"CutTopK: k must be an int >= 1, got {k!r}")
        if ratio is not None and (isinstance(ratio, bool) or not isinstance(ratio, (int, float)) or not 0 < ratio <= 1):
            raise ValueError(f"CutTopK: ratio must be in (0, 1], got {ratio!r}")
        self.k, self.ratio, self.grad_mask = k, ratio, bool(grad_mask)

    def k_for(self, K: int) -> int:
        """The k of a sample of K elements."""
        if self.k is not None:
            return _topk_k("CutTopK", self.k, K)
        return max(1, math.ceil(self.ratio * K))

    def forward(self, x):
        _cut_input("CutTopK", x)
        return _TopKFn.apply(x, self.k_for(math.prod(x.shape[1:])), self.grad_mask)

    def extra_repr(self):
        return (f"k={self.k}" if self.k is not None else f"ratio={self.ratio}") + f", grad_mask={self.grad_mask}"


@dataclass
class CutSparsePacket:
    """What `cut_sparsify` makes and a transport ships: `values` (fp32 [B, k]) and `indices` (int32
    [B, k], ascending in a row: positions in the flattened sample), with the `shape` of the tensor
    they came from."""
    values: torch.Tensor
    indices: torch.Tensor
    shape: tuple
    k: int

    @property
    def nbytes(self) -> int:
        return sum(t.numel() * t.element_size() for t in self.tensors())

    def tensors(self):
        return self.values, self.indices


def cut_sparsify(x, k: int) -> CutSparsePacket:
    """The k largest-magnitude entries of each sample of x [B, *] float32, for the wire.  Not
    differentiable: inside a model use `CutTopK`."""
    _cut_input("cut_sparsify", x)
    if isinstance(k, bool) or not isinstance(k, int) or k < 1:
        raise ValueError(f"cut_sparsify: k must be an int >= 1, got {k!r}")
    x = x.detach()
    x2d = x.reshape(x.shape[0], -1)
    values, indices = ops.impl(x.device).cut_topk(x2d, _topk_k("cut_sparsify", k, x2d.shape[1]))
    return CutSparsePacket(values, indices, tuple(x.shape), k)


def cut_densify(packet: CutSparsePacket) -> torch.Tensor:
    """The float32 tensor of `packet.shape` the packet stands for: zeros off the support."""
    K = math.prod(packet.shape[1:])
    values = packet.values.detach()
    return ops.impl(values.device).cut_scatter(values, packet.indices, K).view(packet.shape)


def cut_sparse_grad(dy, packet: CutSparsePacket) -> torch.Tensor:
    """The return message: dy [B, *] at the packet's positions, fp32 [B, k].  The side that made
    the packet holds the indices, and `cut_densify` of these values is its gradient."""
    _cut_input("cut_sparse_grad", dy)
    if tuple(dy.shape) != tuple(packet.shape):
        raise ValueError(f"cut_sparse_grad: dy is {tuple(dy.shape)}, the packet's tensor {tuple(packet.shape)}")
    dy = dy.detach()
    return ops.impl(dy.device).cut_gather(dy.reshape(dy.shape[0], -1), packet.indices)


__all__ = ["FusedLinear", "FusedConv2d", "FusedGroupNorm", "FusedConvFront", "softmax_cross_entropy", "CutCodec",
           "CutPacket", "cut_pack", "cut_unpack", "CutTopK", "CutSparsePacket", "cut_sparsify", "cut_densify",
           "cut_sparse_grad"]
