"""Native split-mode epochs: a vanilla / U-shape `split_epoch` issued from C++
(`_C.SplitEpoch`, csrc/split.cpp) when the Alice and the whole Bob (TP = 1) live in this
process — the one-GPU BASELINE point (ws = 2) and every co-located placement — and, for an
Alice remote from a one-shard Bob (BASELINE config 2, U-shape ws = 2 on 2 GPUs; vanilla
with `--bob_tp 1`), each side's half of the same loop with the per-batch messages on the
split channel (csrc/ipc_p2p.h peer-mapped messages, or RCCL).

The executor issues the same launches, with the same arguments, dropout seeds, workspaces
and optimizer step counts, as the Python loop of `SplitSession.split_epoch`
(protocols/split.py) in its look-ahead order, so the parameters it produces are bit-identical
to that loop's (tests/test_split_native_gpu.py); the Python loop stays the path for every
other placement and for `--python_epoch`.

The persistent one-launch epochs (`_C.VanillaEpoch`, `_C.UShapeEpoch`) share one gate, one
cfg per side and one fail-safe runner here; `_Vanilla` / `_UShape` hold what differs.

Reference hot loops: data_entities_vanilla.py:66-76 and data_entities.py:65-81.
"""
from __future__ import annotations

import os

import torch

_KIND = {"sgd": 1, "adam": 2}
# rows per batch `_C.SplitEpoch` accepts on every role (csrc/split.cpp, the constructor's check)
SPLIT_MIN_B, SPLIT_MAX_B = 1, 64


def _opt(cfg, adam_only: bool = False) -> dict:
    """An optimizer's settings as the executors read them (`_C.UShapeEpoch` is Adam only)."""
    d = {"lr": cfg.lr, "beta1": cfg.beta1, "beta2": cfg.beta2, "eps": cfg.eps, "wd": cfg.weight_decay}
    return d if adam_only else {"kind": _KIND[cfg.kind], "momentum": cfg.momentum, **d}


def _param(slot, name: str, p: torch.Tensor) -> dict:
    st = slot.state(name, p)
    return {"p": p, "s0": st["m"] if "m" in st else st["buf"], "s1": st.get("v")}


def native_split_ok(sess, cid: int, mode: str) -> bool:
    """Whether `run_native_split_epoch` can drive this epoch: Alice_cid hosted here, Bob a
    single shard in this process, the HIP kernels, the look-ahead order and its batch bound."""
    a = sess.alices.get(cid)
    if a is None or not getattr(sess.args, "native_epoch", True) or not sess.is_bob:
        return False
    if list(sess.bob_ranks) != [sess.rank] or sess.tail.tp_size != 1 or sess.device.type != "cuda":
        return False
    if not hasattr(sess.ops, "C") or a.front.frozen or a.train.x.dtype != torch.uint8:
        return False
    if not sess.split_lookahead(cid):
        return False
    B = sess.B
    if mode == "vanilla":
        return sess.tail.fused3_ok() and sess.tail.lookahead_ok(B)
    return (sess.tail.grouped_ok(B) and len(sess.tail.layers) == 2 and sess.head_fused(B)
            and a.head.head_step_ok(B))


def _alice_cfg(sess, cid: int, mode: str) -> dict:
    a = sess.alices[cid]
    a.front.flush()
    w, b = a.front.params
    pre = "front." if mode == "ushape" else ""
    cfg = {"x": a.train.x, "y": a.train.y,
           "front": {"w": _param(a.slot, pre + "conv.weight", w), "b": _param(a.slot, pre + "conv.bias", b)},
           "front_opt": _opt(a.slot.cfg)}
    if mode == "ushape":
        H = a.head.layers[0]
        cfg["head"] = {"w": _param(a.slot, f"head.{H.spec.name}.weight", H.W),
                       "b": _param(a.slot, f"head.{H.spec.name}.bias", H.b)}
    return cfg


def _bob_cfg(sess, cid: int, mode: str) -> dict:
    tail, ops, dev, B = sess.tail, sess.ops, sess.device, sess.B
    bslot = sess.bob_slot(cid)
    layers = []
    for L in tail.layers:
        layers.append({"w": _param(bslot, f"{L.spec.name}.weight", L.W),
                       "b": _param(bslot, f"{L.spec.name}.bias", L.b)})
    N2 = tail.layers[1].W.shape[0]
    nmax = max(L.W.shape[0] for L in tail.layers)
    kmax = max(L.W.shape[1] for L in tail.layers)
    cfg = {"bob_opt": _opt(bslot.cfg), "tail": layers,
           "p1": tail.layers[0].spec.dropout, "p2": tail.layers[1].spec.dropout,
           # the Python path's own workspaces (ops/hip_ops.py), so every split factor matches
           "fwdws": ops._workspace(dev, 16 * B * nmax, "fwd"),
           "dgws": ops._workspace(dev, 16 * B * kmax, "dgrad")}
    if mode == "vanilla":
        C3 = tail.layers[2].W.shape[0]
        cfg["p2ws"] = ops._workspace(dev, 16 * B * N2, "fc2p")
        cfg["headws"] = ops._workspace(dev, ops.C().head3_slices(N2) * B * C3, "head")
    return cfg


def _bob_done(sess, cid: int, t_b: int, fc: int):
    tail = sess.tail
    sess.bob_slot(cid).t, tail.fwd_count = int(t_b), int(fc)
    tail._pre = None
    tail.acts, tail.dz, tail._wg = [], [], []


def _count(sess, kind: str):
    """Per-session tally of native split epochs by kind (bench.py reports it)."""
    c = sess.native_split_epochs
    c[kind] = c.get(kind, 0) + 1


def run_native_split_epoch(sess, cid: int, order: torch.Tensor, mode: str):
    """One split epoch of Alice_cid over `order` through `_C.SplitEpoch`."""
    _count(sess, "colocated")
    a = sess.alices[cid]
    B = sess.B
    cfg = {"mode": 1 if mode == "vanilla" else 2, "B": B}
    cfg.update(_alice_cfg(sess, cid, mode))
    cfg.update(_bob_cfg(sess, cid, mode))
    ex = sess.ops.C().SplitEpoch(cfg)
    order = order.to(sess.device, torch.int64).contiguous()
    sess.tail._pre = None
    t_a, t_b, fc = ex.run(order, a.slot.t, sess.bob_slot(cid).t, sess.tail.fwd_count, sess.tail.seed_base)
    nb = -(-int(order.numel()) // B)
    a.slot.t = int(t_a)
    _bob_done(sess, cid, t_b, fc)
    if a.head is not None:
        a.head.fwd_count += nb
    return ex


# ---------------------------------------------------------------------- persistent epochs
def _rows(slot, L) -> dict:
    pw, pb = _param(slot, f"{L.spec.name}.weight", L.W), _param(slot, f"{L.spec.name}.bias", L.b)
    return {"W": pw["p"], "b": pb["p"], "s0": pw["s0"], "sb0": pb["s0"]}


def _six(slot, name: str, W: torch.Tensor, b: torch.Tensor) -> dict:
    sw, sb = slot.state(name + ".weight", W), slot.state(name + ".bias", b)
    return {"W": W, "m": sw["m"], "v": sw["v"], "b": b, "mb": sb["m"], "vb": sb["v"]}


def _loss_buf(sess, nb: int) -> torch.Tensor:
    return torch.empty(max(nb, 1) * sess.B, dtype=torch.float32, device=sess.device)


class _Vanilla:
    """`_C.VanillaEpoch` (csrc/vanilla.hip): fp32 SGD-momentum, three tail layers."""
    executor, opt_kind, n_layers, remote_env = "VanillaEpoch", "sgd", 3, "SL_VA_REMOTE_G"

    @staticmethod
    def dtype_reason(dt: str, cdt: str):
        # vanilla.hip computes in exact fp32 only: a bf16 run (fp32 master weights, bf16 operands
        # through the global compute-dtype switch) stays on the per-batch executor, whose kernels
        # honour it, instead of silently running fp32
        return None if dt == cdt == "fp32" else f"dtype {dt if dt != 'fp32' else cdt}: fp32 only"

    @staticmethod
    def bob_cfg(sess, cid: int) -> dict:
        bslot, tail = sess.bob_slot(cid), sess.tail
        bo = bslot.cfg
        return {"layers": [_rows(bslot, L) for L in tail.layers], "lr": bo.lr, "momentum": bo.momentum,
                "wd": bo.weight_decay, "p1": tail.layers[0].spec.dropout, "p2": tail.layers[1].spec.dropout}

    @staticmethod
    def alice_cfg(sess, cid: int) -> dict:
        a = sess.alices[cid]
        a.front.flush()
        w, b = a.front.params
        aw, ab, ao = _param(a.slot, "conv.weight", w), _param(a.slot, "conv.bias", b), a.slot.cfg
        return {"alice": {"w": aw["p"], "b": ab["p"], "s0w": aw["s0"], "s0b": ab["s0"]},
                "alice_lr": ao.lr, "alice_momentum": ao.momentum, "alice_wd": ao.weight_decay,
                "x": a.train.x, "y": a.train.y}

    @staticmethod
    def state(cfg: dict) -> list:
        """Everything the launch writes: what the fail-safe copies and restores."""
        return [t for g in cfg["layers"] + [cfg["alice"]] for t in g.values()]

    @staticmethod
    def run(ex, sess, cid: int, order, loss, nb: int):
        tail = sess.tail
        return ex.run(order, loss, sess.alices[cid].slot.t, sess.bob_slot(cid).t, tail.fwd_count, tail.seed_base)

    @staticmethod
    def run_remote(ex, sess, cid: int, n: int, nb: int):
        loss, tail = _loss_buf(sess, nb), sess.tail
        t_b, fc = ex.run_remote(n, loss, sess.bob_slot(cid).t, tail.fwd_count, tail.seed_base)
        return t_b, fc, loss


class _UShape:
    """`_C.UShapeEpoch` (csrc/ushape.hip): Adam, two tail layers, fp32 or bf16 compute as --dtype;
    it draws no dropout seeds, so the host advances `fwd_count` by the batches run."""
    executor, opt_kind, n_layers, remote_env = "UShapeEpoch", "adam", 2, "SL_US_REMOTE_G"

    @staticmethod
    def dtype_reason(dt: str, cdt: str):
        # bf16 runs the kernel's bf16 instantiation (bf16 operands, fp32 state), but only when the
        # compute dtype the per-batch kernels use agrees with --dtype
        return None if dt in ("fp32", "bf16") and cdt == dt else f"dtype {dt} with compute dtype {cdt}"

    @staticmethod
    def bob_cfg(sess, cid: int) -> dict:
        bslot = sess.bob_slot(cid)
        L1, L2 = sess.tail.layers
        return {"fc1": _six(bslot, L1.spec.name, L1.W, L1.b), "fc2": _six(bslot, L2.spec.name, L2.W, L2.b),
                "bob_opt": _opt(bslot.cfg, adam_only=True), "bf16": getattr(sess.args, "dtype", "fp32") == "bf16"}

    @staticmethod
    def alice_cfg(sess, cid: int) -> dict:
        a = sess.alices[cid]
        a.front.flush()
        w, b = a.front.params
        H = a.head.layers[0]
        return {"conv": _six(a.slot, "front.conv", w, b), "head": _six(a.slot, f"head.{H.spec.name}", H.W, H.b),
                "alice_opt": _opt(a.slot.cfg, adam_only=True), "x": a.train.x, "y": a.train.y}

    @staticmethod
    def state(cfg: dict) -> list:
        return [t for k in ("fc1", "fc2", "conv", "head") for t in cfg[k].values()]

    @staticmethod
    def run(ex, sess, cid: int, order, loss, nb: int):
        t_a, t_b = ex.run(order, loss, sess.alices[cid].slot.t, sess.bob_slot(cid).t)
        return t_a, t_b, sess.tail.fwd_count + nb

    @staticmethod
    def run_remote(ex, sess, cid: int, n: int, nb: int):
        return ex.run_remote(n, sess.bob_slot(cid).t), sess.tail.fwd_count + nb, None


_MODES = {"vanilla": _Vanilla, "ushape": _UShape}


def _dtypes(sess):
    C = sess.ops.C()
    return getattr(sess.args, "dtype", "fp32"), C.get_compute_dtype() if hasattr(C, "get_compute_dtype") else "fp32"


def persistent_ok(sess, cid: int, mode: str) -> bool:
    """Whether `run_persistent_epoch` may drive this epoch: the co-located native conditions,
    the mode's optimizer on both sides and its compute dtype, batches of at most 16 rows, the
    flag, and no earlier failure of the persistent executor in this session."""
    m = _MODES[mode]
    if getattr(sess.args, "split_persist", "auto") == "off" or sess.persist_off:
        return False
    if getattr(sess.comm, "host_staging", False):
        return False   # ranks share this GPU (--ranks_share_gpu): 256 co-resident workgroups are not assured
    if not native_split_ok(sess, cid, mode) or not hasattr(sess.ops.C(), m.executor):
        return False
    reason = m.dtype_reason(*_dtypes(sess))
    if reason is None and not 1 <= sess.B <= 16:
        # every product's MFMA row block is the batch (csrc/vanilla.hip): larger batches run per batch
        reason = f"batch {sess.B} > 16: per-batch executor"
    if reason is not None:
        sess.split_persist_reason = reason
        return False
    return (sess.alices[cid].slot.cfg.kind == m.opt_kind and sess.bob_slot(cid).cfg.kind == m.opt_kind
            and len(sess.tail.layers) == m.n_layers and all(L.W.dtype == torch.float32 for L in sess.tail.layers))


def _shared_cfg(sess) -> dict:
    return {"B": sess.B, "timeout_s": float(getattr(sess.args, "persist_timeout_s", 30.0)),
            # a plain (non-cooperative) launch of the same grid for rocprofv3, whose process dies at
            # exit after any cooperative launch (docs/PERF.md, tools/coop_repro.hip)
            "workgroups": int(os.environ.get("SL_PERSIST_WORKGROUPS", "0"))}


def persist_cfg(sess, cid: int, mode: str) -> dict:
    """What the co-located persistent executor is built from: Bob's half (the whole cfg of the
    remote executor's side), the Alice's half and the shared scalars."""
    m = _MODES[mode]
    return {**m.alice_cfg(sess, cid), **m.bob_cfg(sess, cid), **_shared_cfg(sess)}


def run_persistent_epoch(sess, cid: int, order: torch.Tensor, mode: str) -> bool:
    """One epoch of a co-located Alice_cid as ONE launch (`_C.VanillaEpoch`, csrc/vanilla.hip;
    `_C.UShapeEpoch`, csrc/ushape.hip: every parameter and Adam moment of model1 / model2 /
    model3 on-chip).  Fail-safe: the Alice's and Bob's parameters and optimizer states are
    copied first; if the launch fails they are restored, the persistent executor is switched
    off for the session (`split_persist_fallback`) and False is returned, so the caller runs
    the epoch on the per-batch executor instead."""
    m = _MODES[mode]
    cfg = persist_cfg(sess, cid, mode)
    ex = getattr(sess.ops.C(), m.executor)(cfg)
    if not ex.ok():
        sess.persist_off = True
        sess.split_persist_reason = ex.why()
        return False
    a = sess.alices[cid]
    order = order.to(sess.device, torch.int64).contiguous()
    state = m.state(cfg)
    snap = [t.clone() for t in state] if getattr(sess.args, "persistent_failsafe", "on") != "off" else None
    nb = -(-int(order.numel()) // sess.B)
    loss = _loss_buf(sess, nb)
    sess.tail._pre = None
    if sess.persist_max_steps:
        ex.set_max_steps(int(sess.persist_max_steps))
    fault, sess.persist_fault_step = sess.persist_fault_step, None
    if fault is not None:
        ex.set_fault_step(int(fault))
    try:
        t_a, t_b, fc = m.run(ex, sess, cid, order, loss, nb)
    except RuntimeError as e:
        if snap is None:
            raise
        for t, s in zip(state, snap):
            t.copy_(s)
        sess.persist_off = True
        sess.split_persist_fallback = str(e).splitlines()[0][:200]
        return False
    _count(sess, "persistent")
    a.slot.t = int(t_a)
    _bob_done(sess, cid, t_b, fc)
    if a.head is not None:
        a.head.fwd_count += nb
    sess.last_split_losses = loss[:order.numel()]
    return True


# ---------------------------------------------------------------------- remote placements
def _remote_placement_ok(sess, cid: int) -> bool:
    """Conditions every rank evaluates identically (placement, flags, the link): the Alice
    remote from a one-shard Bob, an fp32 wire, the native kernels, a split channel."""
    return (getattr(sess.args, "native_epoch", True) and sess.device.type == "cuda"
            and getattr(sess, "split_channel", None) is not None and sess.pl.bob_tp == 1
            and sess.host(cid) != sess.pl.bob_root and sess.act_dtype == torch.float32
            and hasattr(sess.ops, "C"))


def _remote_side_ok(sess, cid: int, mode: str) -> bool:
    """This rank's side of the pair can run natively (the same per-side rules as
    `native_split_ok`), including `_C.SplitEpoch`'s batch bound (csrc/split.cpp: 1..64 rows on
    every role), so a larger `--batch_size` keeps the Python loop instead of raising."""
    B = sess.B
    if not SPLIT_MIN_B <= B <= SPLIT_MAX_B:
        return False
    if sess.hosts(cid):
        a = sess.alices[cid]
        if a.front.frozen or a.train.x.dtype != torch.uint8:
            return False
        return mode == "vanilla" or (sess.head_fused(B) and a.head.head_step_ok(B))
    t = sess.tail
    if mode == "vanilla":
        return t.fused3_ok()
    return t.grouped_ok(B) and len(t.layers) == 2 and sess.head_fused(B)


def native_remote_role(sess, cid: int, mode: str):
    """Collective over the pair (the Alice's rank, Bob's): whether this epoch of a remote
    Alice runs on the native split executor.  Returns "alice" / "bob" on the pair's ranks
    when both sides agree, "skip" on every other rank (it moves nothing in this epoch either
    way), None when the Python loop runs it."""
    if not _remote_placement_ok(sess, cid):
        return None
    host, bob = sess.host(cid), sess.pl.bob_root
    if sess.rank not in (host, bob):
        return "skip"
    peer = bob if sess.rank == host else host
    mine = torch.tensor([1 if _remote_side_ok(sess, cid, mode) else 0], dtype=torch.int32, device=sess.device)
    theirs = torch.empty_like(mine)
    sess.comm.exchange([(mine, peer)], [(theirs, peer)])
    if int(mine.item()) and int(theirs.item()):
        return "alice" if sess.rank == host else "bob"
    return None


def persistent_remote_ok(sess, cid: int, mode: str) -> bool:
    """Bob's side only (the Alice's side is the same run_alice either way): whether Bob serves
    this remote Alice's epoch with ONE persistent launch that speaks the peer-mapped channel
    itself (`_C.VanillaEpoch.run_remote` / `_C.UShapeEpoch.run_remote`, csrc/vanilla.hip and
    csrc/ushape.hip REM).  Needs the peer-mapped channel (not RCCL), B <= 16, the flag, no
    earlier decline, vanilla: fp32 SGD-momentum; U-shape: Adam, fp32 or bf16 as the compute
    dtype; and a GPU of its own: with ranks sharing one GPU the Alice's kernels need CUs the
    launch would hold, so only an explicit reduced grid (SL_VA_REMOTE_G / SL_US_REMOTE_G, the
    one-GPU tests) runs there."""
    m = _MODES.get(mode)
    if m is None or getattr(sess.args, "split_persist", "auto") == "off" or sess.persist_remote_off:
        return False
    ch = getattr(sess, "split_channel", None)
    if ch is None or not hasattr(ch, "host_error") or not hasattr(sess.ops.C(), m.executor):
        return False
    if getattr(sess.comm, "host_staging", False) and not os.environ.get(m.remote_env):
        return False
    t = sess.tail
    if not (1 <= sess.B <= 16 and t.tp_size == 1 and all(L.W.dtype == torch.float32 for L in t.layers)):
        return False
    return (m.dtype_reason(*_dtypes(sess)) is None and sess.bob_slot(cid).cfg.kind == m.opt_kind
            and len(t.layers) == m.n_layers)


def _run_remote_persistent(sess, cid: int, n: int, peer: int, mode: str):
    """Bob's half of a remote epoch as one persistent launch; None when the executor declines
    this configuration (the caller then runs run_bob, which Alice cannot tell apart).  A launch
    that fails mid-epoch raises: the Alice is then stopped at a message of this epoch and times
    out on her side, so there is no state both sides could roll back to (fail-stop,
    docs/DEVIATIONS.md)."""
    m = _MODES[mode]
    cfg = {**m.bob_cfg(sess, cid), **_shared_cfg(sess), "channel": sess.split_channel, "peer": int(peer),
           "G": int(os.environ.get(m.remote_env, "256"))}
    ex = getattr(sess.ops.C(), m.executor)(cfg)
    if not ex.ok():
        sess.persist_remote_off = True
        sess.split_persist_reason = "remote: " + ex.why()
        return None
    sess.tail._pre = None
    t_b, fc, loss = m.run_remote(ex, sess, cid, int(n), -(-int(n) // sess.B))
    _bob_done(sess, cid, t_b, fc)
    if loss is not None:
        sess.last_split_losses = loss[:int(n)]
    _count(sess, "remote_persistent")
    return ex


def run_native_remote_epoch(sess, cid: int, order, n: int, mode: str, role: str):
    """This rank's half of one split epoch of a remote Alice_cid (`_C.SplitEpoch` roles 1 / 2,
    csrc/split.cpp run_alice / run_bob): the per-batch messages go over `sess.split_channel`
    on the compute stream.  Same launches and step counts as the Python loop of this
    placement (the §3.2 overlap order: no look-ahead).  Bob's side of a vanilla epoch runs as
    ONE persistent launch when `persistent_remote_ok` (the same messages, from inside it)."""
    if role == "skip":
        return None
    _count(sess, "remote_" + role)
    C = sess.ops.C()
    host, bob = sess.host(cid), sess.pl.bob_root
    cfg = {"mode": 1 if mode == "vanilla" else 2, "B": sess.B, "channel": sess.split_channel}
    comm = sess.comm
    comm.progress()
    ex = _run_remote_persistent(sess, cid, n, host, mode) if role == "bob" and persistent_remote_ok(sess, cid, mode) else None
    if ex is not None:
        pass                      # Bob's side ran as one persistent launch
    elif role == "alice":
        a = sess.alices[cid]
        cfg.update(_alice_cfg(sess, cid, mode))
        cfg.update({"role": 1, "peer": bob})
        ex = C.SplitEpoch(cfg)
        order = order.to(sess.device, torch.int64).contiguous()
        a.slot.t = int(ex.run_alice(order, a.slot.t))
        if a.head is not None:
            a.head.fwd_count += -(-int(order.numel()) // sess.B)
    else:
        cfg.update(_bob_cfg(sess, cid, mode))
        cfg.update({"role": 2, "peer": host})
        ex = C.SplitEpoch(cfg)
        sess.tail._pre = None
        t_b, fc = ex.run_bob(int(n), sess.bob_slot(cid).t, sess.tail.fwd_count, sess.tail.seed_base)
        _bob_done(sess, cid, t_b, fc)
    for op, peer, nb in ex.messages():
        if op == "send":
            comm.bytes_sent += nb
            comm.msgs_sent += 1
            if comm.msg_log is not None:
                comm.msg_log.append(("native_send", comm.rank, peer, nb))
    comm.progress()
    return ex
