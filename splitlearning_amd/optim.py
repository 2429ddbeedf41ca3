"""Fused multi-tensor optimizers for user-written models (the optimizer step of `nn.py`'s
autograd path).

The engines fuse the optimizer update into their weight-gradient kernels. A model trained
with `loss.backward()` has its gradients materialised by autograd, so what can still be
fused is the pass over them: `FusedSGD` and `FusedAdam` update every parameter of a
parameter group in one launch (`csrc/optim.hip`: 16-byte streaming loads and stores, the
engines' own update rule `sl_opt_update`), instead of one launch, or several, per tensor.

* Semantics are `torch.optim.SGD` (dampening 0, no Nesterov) and `torch.optim.Adam`
  (coupled L2 weight decay, no amsgrad). Options the kernel does not implement raise
  `ValueError`; fp32 contiguous parameters only.
* `max_grad_norm` clips the global gradient norm over all groups, as
  `torch.nn.utils.clip_grad_norm_(all parameters, max_grad_norm)` before the step would:
  two deterministic kernels leave {sum of squares, norm, coefficient} on the device
  (`opt.last_grad_norm`) and the step kernels read the coefficient from there, so the host
  never waits. Reading `last_grad_norm` is the caller's synchronisation.
* State layout is torch's (`step` / `exp_avg` / `exp_avg_sq`, `momentum_buffer`), and the
  parameter groups carry torch's option keys, so a `state_dict()` loads into the
  `torch.optim` class over the same parameters and back.

On CPU tensors the same classes run the eager implementations (`ops/torch_ops.py`).
"""
from __future__ import annotations

import torch

from . import ops
from .config import OptimCfg


class _FusedOptimizer(torch.optim.Optimizer):
    # torch's option keys this implementation cannot honour -> the one value it accepts
    _FIXED: dict = {}

    def __init__(self, params, defaults, max_grad_norm):
        if max_grad_norm is not None and not max_grad_norm > 0.0:
            raise ValueError(f"max_grad_norm must be positive, got {max_grad_norm}")
        self.max_grad_norm = max_grad_norm
        self.last_grad_norm = None
        super().__init__(params, defaults)

    def _check_group(self, group):
        for key, only in self._FIXED.items():
            if group.get(key, only) != only:
                raise ValueError(f"{type(self).__name__} does not implement {key}={group[key]!r}")
        for p in group["params"]:
            if p.dtype != torch.float32 or not p.is_contiguous():
                raise ValueError(f"{type(self).__name__} needs contiguous float32 parameters, got "
                                 f"{p.dtype} with strides {tuple(p.stride())}")

    def add_param_group(self, param_group):
        super().add_param_group(param_group)
        self._check_group(self.param_groups[-1])

    def __setstate__(self, state):     # load_state_dict and unpickling end here
        super().__setstate__(state)
        for group in self.param_groups:
            for key, value in self.defaults.items():
                group.setdefault(key, value)
            self._check_group(group)

    def _cfg(self, group) -> OptimCfg:
        raise NotImplementedError

    def _slot(self, p, group):
        """(kernel state dict of p, creating torch-layout state on first use; step count)."""
        raise NotImplementedError

    def _advance(self, p):
        pass

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        # one launch list per (group, device, step count): a launch shares its hyper-parameters
        work = []
        for group in self.param_groups:
            buckets: dict = {}
            for p in group["params"]:
                if p.grad is None:
                    continue
                if p.grad.is_sparse:
                    raise RuntimeError(f"{type(self).__name__} does not support sparse gradients")
                st, t = self._slot(p, group)
                ps, gs, sts = buckets.setdefault((p.device, t), ([], [], []))
                ps.append(p)
                gs.append(p.grad if p.grad.is_contiguous() else p.grad.contiguous())
                sts.append(st)
            work += [(self._cfg(group), dev, t, *b) for (dev, t), b in buckets.items()]
        gscale = None
        if self.max_grad_norm is not None and work:
            devs = {dev for _, dev, *_ in work}
            if len(devs) != 1:
                raise ValueError("max_grad_norm needs all parameters on one device")
            dev = devs.pop()
            self.last_grad_norm = ops.impl(dev).grad_norm([g for w in work for g in w[4]], self.max_grad_norm)
            gscale = self.last_grad_norm[2:3]
        for cfg, dev, t, ps, gs, sts in work:
            ops.impl(dev).multi_update_(ps, gs, sts, cfg, t, gscale)
            for p in ps:
                self._advance(p)
        return loss


class FusedSGD(_FusedOptimizer):
    """`torch.optim.SGD(params, lr, momentum, weight_decay=...)` as one launch per parameter
    group, with optional global gradient-norm clipping (`max_grad_norm`)."""

    _FIXED = {"dampening": 0, "nesterov": False, "maximize": False, "differentiable": False}

    def __init__(self, params, lr, momentum=0, weight_decay=0, max_grad_norm=None, *, dampening=0,
                 nesterov=False, maximize=False):
        if lr < 0.0 or momentum < 0.0 or weight_decay < 0.0:
            raise ValueError("lr, momentum and weight_decay must be non-negative")
        defaults = dict(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay,
                        nesterov=nesterov, maximize=maximize, foreach=None, differentiable=False, fused=None)
        super().__init__(params, defaults, max_grad_norm)

    def _cfg(self, group):
        return OptimCfg("sgd", float(group["lr"]), weight_decay=float(group["weight_decay"]),
                        momentum=float(group["momentum"]))

    def _slot(self, p, group):
        buf = None
        if group["momentum"] != 0:
            state = self.state[p]
            buf = state.get("momentum_buffer")
            if buf is None:     # torch starts from the first gradient: 0 * momentum + g is the same
                buf = state["momentum_buffer"] = torch.zeros_like(p, memory_format=torch.preserve_format)
        return {"buf": buf}, 1


class FusedAdam(_FusedOptimizer):
    """`torch.optim.Adam(params, lr, betas, eps, weight_decay)` as one launch per parameter
    group, with optional global gradient-norm clipping (`max_grad_norm`)."""

    _FIXED = {"amsgrad": False, "maximize": False, "capturable": False, "differentiable": False,
              "decoupled_weight_decay": False}

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, max_grad_norm=None, *,
                 amsgrad=False, maximize=False):
        if lr < 0.0 or eps < 0.0 or weight_decay < 0.0 or not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0):
            raise ValueError("lr, eps and weight_decay must be non-negative and betas in [0, 1)")
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad,
                        maximize=maximize, foreach=None, capturable=False, differentiable=False, fused=None,
                        decoupled_weight_decay=False)
        super().__init__(params, defaults, max_grad_norm)

    def _cfg(self, group):
        b1, b2 = group["betas"]
        return OptimCfg("adam", float(group["lr"]), beta1=float(b1), beta2=float(b2), eps=float(group["eps"]),
                        weight_decay=float(group["weight_decay"]))

    def _slot(self, p, group):
        state = self.state[p]
        if len(state) == 0:
            state["step"] = torch.tensor(0.0, dtype=torch.float32)
            state["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            state["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
        # parameters that have always stepped together share t and therefore a launch
        return {"m": state["exp_avg"], "v": state["exp_avg_sq"]}, int(state["step"]) + 1

    def _advance(self, p):
        self.state[p]["step"] += 1


__all__ = ["FusedSGD", "FusedAdam"]
