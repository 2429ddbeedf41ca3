"""Eager PyTorch implementations of every framework op.

These are (a) the CPU execution path (gloo multi-process tests, CPU runs of
`split_nn.py`) and (b) the fp32 ground truth the HIP kernels are tested
against.  Signatures are identical to `ops.hip_ops`; `ops.__init__` picks one
per call by device.
"""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

from .rng import hash32, keep_mask

CUT = 5408


# ---------------------------------------------------------------- conv front
def conv_front_fwd(x_u8: torch.Tensor, idx: torch.Tensor, w: torch.Tensor, b: torch.Tensor, labels=None):
    """Gather rows `idx` of the uint8 shard, conv3x3(1->32)+bias, ReLU, maxpool2x2.

    Returns (y [B,5408] fp32 NCHW-flattened, am uint8 [B,5408] argmax-in-window 0..3),
    plus `labels[idx]` when the shard's labels are given.
    """
    if labels is not None:
        return conv_front_fwd(x_u8, idx, w, b) + (labels.index_select(0, idx),)
    x = x_u8.index_select(0, idx).to(torch.float32).reshape(-1, 1, 28, 28)
    z = F.relu(F.conv2d(x, w, b))
    y, ind = F.max_pool2d(z, 2, 2, return_indices=True)
    # ind is the flat index into 26x26; convert to 2-bit window position
    r = ind // 26
    c = ind % 26
    am = ((r % 2) * 2 + (c % 2)).to(torch.uint8)
    return y.reshape(-1, CUT).contiguous(), am.reshape(-1, CUT).contiguous()


def conv_front_bwd(dy, y, am, x_u8, idx, w, b):
    """Gradients of conv weight/bias given dL/dy for the pooled, flattened output."""
    B = dy.shape[0]
    x = x_u8.index_select(0, idx).to(torch.float32).reshape(B, 1, 28, 28)
    g = (dy * (y > 0)).reshape(B, 32, 13, 13)
    amr = am.reshape(B, 32, 13, 13).long()
    dz = torch.zeros(B, 32, 26, 26, dtype=dy.dtype, device=dy.device)
    ph = torch.arange(13, device=dy.device).view(1, 1, 13, 1)
    pw = torch.arange(13, device=dy.device).view(1, 1, 1, 13)
    rr = 2 * ph + amr // 2
    cc = 2 * pw + amr % 2
    dz.view(B, 32, -1).scatter_(2, (rr * 26 + cc).reshape(B, 32, -1), g.reshape(B, 32, -1))
    dw = torch.nn.grad.conv2d_weight(x, w.shape, dz)
    db = dz.sum(dim=(0, 2, 3))
    return dw, db


# ---------------------------------------------------------------- general 3x3 conv
def conv3x3_fwd(x, w, b, pad: int, relu: bool, pool):
    """Conv2d(3x3, stride 1, padding `pad`) [+ ReLU] [+ MaxPool2d(2, 2) when `pool` == 2].

    Returns (y [B,Cout,Hy,Wy], am): am is uint8 like y, the window position 2*dy + dx of the
    maximum (a tie goes to the lowest position), or None without pooling."""
    z = F.conv2d(x, w, b, padding=pad)
    if relu:
        z = F.relu(z)
    if not pool:
        return z, None
    y, ind = F.max_pool2d(z, 2, 2, return_indices=True)
    wo = z.shape[-1]           # ind is the flat index into the Ho x Wo plane
    am = (((ind // wo) % 2) * 2 + (ind % wo) % 2).to(torch.uint8)
    return y, am


def _conv3x3_dz(dy, y, am, relu: bool, pool, ho: int, wo: int):
    """The gradient at conv resolution: dy routed to each window's maximum, masked by the ReLU;
    0 in the row / column the floor rule leaves out of every window."""
    g = dy * (y > 0) if relu else dy
    if not pool:
        return g
    B, C, hp, wp = dy.shape
    a = am.long()
    rr = 2 * torch.arange(hp, device=dy.device).view(1, 1, hp, 1) + a // 2
    cc = 2 * torch.arange(wp, device=dy.device).view(1, 1, 1, wp) + a % 2
    dz = torch.zeros(B, C, ho * wo, dtype=dy.dtype, device=dy.device)
    dz.scatter_(2, (rr * wo + cc).reshape(B, C, -1), g.reshape(B, C, -1))
    return dz.view(B, C, ho, wo)


def conv3x3_dgrad(dy, y, am, w, pad: int, relu: bool, pool, x_shape):
    ho, wo = x_shape[2] + 2 * pad - 2, x_shape[3] + 2 * pad - 2
    dz = _conv3x3_dz(dy, y, am, relu, pool, ho, wo)
    return torch.nn.grad.conv2d_input(tuple(x_shape), w, dz, padding=pad)


def conv3x3_wgrad(dy, y, am, x, pad: int, relu: bool, pool):
    """(dw [Cout,Cin,3,3], db [Cout])."""
    ho, wo = x.shape[2] + 2 * pad - 2, x.shape[3] + 2 * pad - 2
    dz = _conv3x3_dz(dy, y, am, relu, pool, ho, wo)
    dw = torch.nn.grad.conv2d_weight(x, (dy.shape[1], x.shape[1], 3, 3), dz, padding=pad)
    return dw, dz.sum(dim=(0, 2, 3))


# ---------------------------------------------------------------- GroupNorm
def _gn_pre(x, mean, rstd, weight, bias, groups: int):
    """(xh, z): xh = (x - mean) * rstd per (sample, group), z = xh * weight[c] + bias[c]."""
    B, C = x.shape[:2]
    xh = ((x.reshape(B, groups, -1) - mean.unsqueeze(-1)) * rstd.unsqueeze(-1)).reshape(x.shape)
    if weight is None:
        return xh, xh
    cshape = (1, C) + (1,) * (x.dim() - 2)
    return xh, xh * weight.reshape(cshape) + bias.reshape(cshape)


def group_norm_fwd(x, weight, bias, groups: int, eps: float, relu: bool, pool):
    """GroupNorm(groups, C, eps) [+ ReLU] [+ MaxPool2d(2, 2) when `pool` == 2] of x [B, C, *].

    Returns (y, mean [B, G], rstd [B, G], am): the variance is the mean squared deviation from
    the mean (two passes); am is uint8 like y, the window position 2*dy + dx of the maximum (a
    tie goes to the lowest position), or None without pooling."""
    B = x.shape[0]
    xg = x.reshape(B, groups, -1)
    mean = xg.mean(dim=2)
    var = (xg - mean.unsqueeze(-1)).square().mean(dim=2)
    rstd = 1.0 / torch.sqrt(var + eps)
    z = _gn_pre(x, mean, rstd, weight, bias, groups)[1]
    if relu:
        z = F.relu(z)
    if not pool:
        return z, mean, rstd, None
    y, ind = F.max_pool2d(z, 2, 2, return_indices=True)
    wo = z.shape[-1]           # ind is the flat index into the H x W plane
    am = (((ind // wo) % 2) * 2 + (ind % wo) % 2).to(torch.uint8)
    return y, mean, rstd, am


def group_norm_bwd(dy, x, mean, rstd, weight, bias, am, groups: int, relu: bool, pool, need_dx: bool = True):
    """(dx, dweight, dbias) by the explicit formula: dz = dy routed back through the pool and
    the ReLU, xh = (x - mean) * rstd, dweight[c] = sum dz * xh, dbias[c] = sum dz, and per
    (sample, group) of n elements dx = rstd * (w dz - mean_n(w dz) - xh * mean_n(w dz xh)).
    dx is None when `need_dx` is false; dweight and dbias are None without the affine."""
    B, C = x.shape[:2]
    xh, z = _gn_pre(x, mean, rstd, weight, bias, groups)
    dz = _conv3x3_dz(dy, None, am, False, pool, x.shape[2], x.shape[3]) if pool else dy
    if relu:
        dz = dz * (z > 0)
    dweight = dbias = dx = None
    red = (0,) + tuple(range(2, x.dim()))
    if weight is not None:
        dweight, dbias = (dz * xh).sum(dim=red), dz.sum(dim=red)
    if need_dx:
        wdz = dz if weight is None else dz * weight.reshape((1, C) + (1,) * (x.dim() - 2))
        wg, xg = wdz.reshape(B, groups, -1), xh.reshape(B, groups, -1)
        m1, m2 = wg.mean(dim=2, keepdim=True), (wg * xg).mean(dim=2, keepdim=True)
        dx = (rstd.unsqueeze(-1) * (wg - m1 - xg * m2)).reshape(x.shape)
    return dx, dweight, dbias


# ---------------------------------------------------------------- cut codec
# The definition of the cut-layer format (csrc/cutcodec.hip matches it bit for bit).  x2d [R, K]
# fp32 is cut into ng = ceil(K / group) groups of `group` consecutive elements of a row (the last
# may be short).  Per group, in fp32: absmax = max |x|, scale = absmax / qmax, inv = qmax / absmax
# (0 for a zero group), q = clamp(rint(x * inv)) or, with a seed, clamp(floor((x * inv) + u)) with
# u = (hash32(seed, row, column) >> 8) * 2^-24; x^ = float(q) * scale.  Every step is its own torch
# op, so nothing is contracted into an FMA, and the divisions are tensor / tensor (a GPU division
# by a Python scalar multiplies by its reciprocal, which rounds differently).
CUT_GROUPS = (16, 32, 64, 128, 256)
CUT_QMAX = {8: 127.0, 4: 7.0}


def _cut_check(t, bits, group):
    if bits not in CUT_QMAX:
        raise ValueError(f"cut codec: bits must be 8 or 4, got {bits!r}")
    if group not in CUT_GROUPS:
        raise ValueError(f"cut codec: group must be one of {CUT_GROUPS}, got {group!r}")
    if t.dim() != 2:
        raise ValueError(f"cut codec: expected a 2-D tensor, got {tuple(t.shape)}")


def _cut_per_element(scales, K: int, group: int):
    """[R, ng] -> [R, K]: each group's value at its elements."""
    return scales.repeat_interleave(group, dim=1)[:, :K]


def cut_pack(x2d, bits: int, group: int, seed=None):
    """(payload, scales): payload int8 [R, K] at 8 bits; uint8 [R, ceil(K / 2)] at 4 bits, column
    2j in the low nibble of byte j and 2j + 1 in the high one (two's complement, 0 past an odd K);
    scales fp32 [R, ng].  Nearest (half to even) without a seed, stochastic with one."""
    _cut_check(x2d, bits, group)
    if x2d.dtype != torch.float32:
        raise ValueError(f"cut codec: input must be float32, got {x2d.dtype}")
    R, K = x2d.shape
    ng = -(-K // group)
    absmax = F.pad(x2d.abs(), (0, ng * group - K)).view(R, ng, group).amax(dim=2)
    qmax = torch.full_like(absmax, CUT_QMAX[bits])
    scales = absmax / qmax
    inv = torch.where(absmax > 0, qmax / absmax, torch.zeros_like(absmax))
    t = x2d * _cut_per_element(inv, K, group)
    if seed is None:
        q = torch.round(t)
    else:
        u = (hash32(seed, R, K, x2d.device) >> 8).to(torch.float32) * 2.0 ** -24
        q = torch.floor(t + u)
    q = q.clamp(-CUT_QMAX[bits], CUT_QMAX[bits])
    if bits == 8:
        return q.to(torch.int8), scales
    nib = F.pad(q.to(torch.int32) & 0xF, (0, K % 2))
    return (nib[:, 0::2] | (nib[:, 1::2] << 4)).to(torch.uint8), scales


def cut_unpack(payload, scales, K: int, bits: int, group: int):
    """x^ [R, K] fp32 = float(q) * scale of its group."""
    _cut_check(payload, bits, group)
    if bits == 8:
        q = payload.to(torch.float32)
    else:
        p = payload.to(torch.int32)
        nib = torch.stack((p & 0xF, p >> 4), dim=2).view(p.shape[0], -1)[:, :K]
        q = ((nib ^ 8) - 8).to(torch.float32)
    return q * _cut_per_element(scales, K, group)


def cut_roundtrip(x2d, bits: int, group: int, seed=None):
    """cut_unpack(*cut_pack(x2d, ...)): what the other side of the cut receives."""
    payload, scales = cut_pack(x2d, bits, group, seed)
    return cut_unpack(payload, scales, x2d.shape[1], bits, group)


# ---------------------------------------------------------------- cut sparsifier
# The definition of the top-k form of the cut (nn.CutTopK / cut_sparsify / cut_densify /
# cut_sparse_grad).  x [R, K] fp32, 1 <= k <= K.  The key of an element is |x| (so -0.0 and 0.0 are
# equal); a row's support is the k columns with the largest keys, and among equal keys at the
# threshold the lowest columns win: a stable descending sort keeps equal keys in column order, so
# its first k entries are exactly that.  The wire is values fp32 [R, k] (signs kept) + indices int32
# [R, k], ascending in a row.  The gradient is dy on the support and 0 elsewhere.
def _topk_check(x2d, k):
    if x2d.dim() != 2:
        raise ValueError(f"cut top-k: expected a 2-D tensor, got {tuple(x2d.shape)}")
    if x2d.dtype != torch.float32:
        raise ValueError(f"cut top-k: input must be float32, got {x2d.dtype}")
    if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= x2d.shape[1]:
        raise ValueError(f"cut top-k: need an integer 1 <= k <= K = {x2d.shape[1]}, got {k!r}")


def cut_topk(x2d, k: int):
    """(values fp32 [R, k], indices int32 [R, k] ascending): the k largest |x| of each row."""
    _topk_check(x2d, k)
    order = torch.sort(x2d.abs(), dim=1, descending=True, stable=True).indices[:, :k]
    idx = order.sort(dim=1).values
    return x2d.gather(1, idx), idx.to(torch.int32)


def cut_scatter(values, indices, K: int):
    """y [R, K]: 0 everywhere but y[r, indices[r, j]] = values[r, j]."""
    y = torch.zeros(values.shape[0], K, device=values.device, dtype=values.dtype)
    return y.scatter_(1, indices.to(torch.int64), values)


def cut_gather(d2d, indices):
    """[R, k]: d2d at the support, the wire form of the gradient."""
    return d2d.gather(1, indices.to(torch.int64))


def cut_topk_dense(x2d, k: int):
    """(y, indices): what the other side holds after densifying the packet of x2d."""
    values, indices = cut_topk(x2d, k)
    return cut_scatter(values, indices, x2d.shape[1]), indices


def cut_mask(d2d, indices):
    """d2d on the support, 0 elsewhere."""
    return cut_scatter(cut_gather(d2d, indices), indices, d2d.shape[1])


# ---------------------------------------------------------------- linear
# `--dtype bf16`: GEMM operands rounded to bf16, fp32 accumulation (the HIP kernels' rule,
# csrc/common.h bfr); parameters and optimizer state stay fp32
_BF16 = False


def set_compute_dtype(dtype: str):
    global _BF16
    if dtype not in ("fp32", "bf16"):
        raise ValueError(dtype)
    _BF16 = dtype == "bf16"


def _r(t: torch.Tensor) -> torch.Tensor:
    return t.to(torch.bfloat16).to(t.dtype) if _BF16 else t


def linear_fwd(x, w, b, relu: bool, drop_p: float, seed: int, col_offset: int = 0,
               out: torch.Tensor | None = None):
    y = _r(x) @ _r(w).t()
    if b is not None:
        y = y + b
    if relu:
        y = F.relu(y)
    if drop_p > 0:
        keep = keep_mask(seed, y.shape[0], y.shape[1], drop_p, col_offset, device=y.device)
        y = y * keep * (1.0 / (1.0 - drop_p))
    if out is not None:
        out.copy_(y)
        return out
    return y


def linear_epilogue(P, b, relu: bool, drop_p: float, seed: int, col_offset: int = 0):
    """bias + ReLU + dropout applied to an already-reduced GEMM result (row-parallel layers)."""
    y = P if b is None else P + b
    if relu:
        y = F.relu(y)
    if drop_p > 0:
        keep = keep_mask(seed, y.shape[0], y.shape[1], drop_p, col_offset, device=y.device)
        y = y * keep * (1.0 / (1.0 - drop_p))
    return y


def linear_dgrad(dz, w, h_prev=None, scale: float = 1.0):
    """dx = dz @ w; if h_prev is given, also back-propagate through the previous
    layer's ReLU(+dropout): dx *= scale * [h_prev > 0]."""
    dx = _r(dz) @ _r(w)
    if h_prev is not None:
        dx = dx * (h_prev > 0) * scale
    return dx


def linear_wgrad(dz, a):
    return _r(dz).t() @ _r(a), _r(dz).sum(0)


# ---------------------------------------------------------------- optimizers
def adam_update_(p, g, m, v, t, lr, beta1, beta2, eps, wd):
    if wd:
        g = g.add(p, alpha=wd)
    m.mul_(beta1).add_(g, alpha=1 - beta1)
    v.mul_(beta2).addcmul_(g, g, value=1 - beta2)
    bc1 = 1 - beta1 ** t
    bc2 = 1 - beta2 ** t
    denom = (v.sqrt() / math.sqrt(bc2)).add_(eps)
    p.addcdiv_(m, denom, value=-lr / bc1)


def sgd_update_(p, g, buf, lr, momentum, wd):
    if wd:
        g = g.add(p, alpha=wd)
    if momentum:
        buf.mul_(momentum).add_(g)
        p.add_(buf, alpha=-lr)
    else:
        p.add_(g, alpha=-lr)


def apply_update_(p, g, st: dict, cfg, t: int):
    if cfg.kind == "adam":
        adam_update_(p, g, st["m"], st["v"], t, cfg.lr, cfg.beta1, cfg.beta2, cfg.eps,
                     cfg.weight_decay)
    elif cfg.kind == "sgd":
        sgd_update_(p, g, st["buf"], cfg.lr, cfg.momentum, cfg.weight_decay)
    else:
        raise ValueError(cfg.kind)


def multi_update_(ps, gs, sts, cfg, t: int, gscale=None):
    """`apply_update_` over lists of tensors; `gscale` (a one-float tensor) multiplies every
    gradient first."""
    with torch.no_grad():
        for p, g, st in zip(ps, gs, sts):
            apply_update_(p, g if gscale is None else g * gscale, st, cfg, t)


def grad_norm(gs, max_norm: float):
    """{sum of squares, L2 norm, min(1, max_norm / (norm + 1e-6))} over all of `gs`
    (torch.nn.utils.clip_grad_norm_'s rule) as a 3-float tensor."""
    norm = torch.linalg.vector_norm(torch.stack([torch.linalg.vector_norm(g) for g in gs]))
    coef = torch.clamp(max_norm / (norm + 1e-6), max=1.0)
    return torch.stack([norm * norm, norm, coef])


def linear_wgrad_step_(dz, a, w, b, cfg, st_w: dict, st_b: dict, t: int):
    with torch.no_grad():
        dw, db = linear_wgrad(dz, a)
        apply_update_(w, dw, st_w, cfg, t)
        if b is not None:
            apply_update_(b, db, st_b, cfg, t)


def conv_front_bwd_step_(dy, y, am, x_u8, idx, w, b, cfg, st_w, st_b, t):
    with torch.no_grad():
        dw, db = conv_front_bwd(dy, y, am, x_u8, idx, w, b)
        apply_update_(w, dw, st_w, cfg, t)
        apply_update_(b, db, st_b, cfg, t)


def conv_local_step_(x_u8, y_all, idx, w, b, cfg, st_w, st_b, t, loss_rows=None):
    """SISA client step: CE over the 5408-wide activation (Q5), backward, optimizer."""
    with torch.no_grad():
        act, am = conv_front_fwd(x_u8, idx, w, b)
        loss, d = softmax_ce(act, y_all[idx], 1.0 / idx.numel())
        conv_front_bwd_step_(d, act, am, x_u8, idx, w, b, cfg, st_w, st_b, t)
    return loss


def conv_local_epoch_(x_u8, y_all, order, B: int, w, b, cfg, st_w, st_b, t0: int):
    """ceil(n/B) client steps over `order` (steps t0, t0+1, ...); per-sample losses [n]."""
    out = []
    for i, s in enumerate(range(0, order.numel(), B)):
        out.append(conv_local_step_(x_u8, y_all, order[s:s + B], w, b, cfg, st_w, st_b, t0 + i))
    return torch.cat(out) if out else torch.empty(0, device=x_u8.device)


# ---------------------------------------------------------------- loss / metrics
def softmax_ce(logits, labels, scale: float, ignore_index: int = -100):
    """Row-wise cross-entropy. Returns (per-row loss [M] (0 for ignored rows),
    dlogits = scale * (softmax - onehot) (0 rows for ignored))."""
    lse = torch.logsumexp(logits, dim=1)
    valid = labels != ignore_index
    safe = torch.where(valid, labels, torch.zeros_like(labels))
    picked = logits.gather(1, safe.view(-1, 1)).squeeze(1)
    loss = torch.where(valid, lse - picked, torch.zeros_like(lse))
    p = torch.softmax(logits, dim=1)
    p.scatter_add_(1, safe.view(-1, 1), -torch.ones_like(picked).view(-1, 1))
    d = p * scale * valid.view(-1, 1)
    return loss, d


def relu_mask(d, h, scale: float = 1.0):
    """d * scale * [h > 0] (a layer's own ReLU/dropout backward)."""
    return d * (h > 0) * scale


def eval_counters(logits, labels, omit_label: int):
    """[correct, total, correct_unlearned, total_unlearned, correct_remaining, total_remaining]
    (reference `eval_breakdown`, data_entities_vanilla.py:159-202)."""
    pred = logits.argmax(dim=1)
    ok = pred == labels
    unl = labels == omit_label
    rem = ~unl
    return torch.stack([ok.sum(), torch.tensor(labels.numel(), device=labels.device),
                        (ok & unl).sum(), unl.sum(), (ok & rem).sum(), rem.sum()]).to(torch.int64)
