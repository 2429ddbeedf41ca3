"""One refused call per distinct host-side operand check of `_C`, on the smallest tensors that
express it.  Every bad operand is chosen so that a launch would stay inside every buffer even
if its check were absent: a wider dtype, a larger tensor, a mismatched but larger dimension, a
non-contiguous view of a larger buffer.  No case is expected to reach a kernel, and refusals
that only an undersized buffer can show (`y too small`, short workspaces, `rows beyond the
shard`) are left out on purpose.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

OPT = (2, 1e-3, 0.9, 0.999, 1e-8, 0.0, 0.0, 1, 0)   # kind, lr, beta1, beta2, eps, wd, momentum, t, dyn
SGD = (1,) + OPT[1:]
B = 2


@pytest.fixture(scope="module")
def k(cuda):
    import splitlearning_amd._C as C

    class K:
        pass

    o = K()
    o.C = C
    o.dev = cuda
    o.f = lambda *s: torch.zeros(*s, device=cuda)
    o.d = lambda *s: torch.zeros(*s, device=cuda, dtype=torch.float64)
    o.l = lambda *s: torch.zeros(*s, device=cuda, dtype=torch.long)
    o.i = lambda *s: torch.zeros(*s, device=cuda, dtype=torch.int32)
    o.u = lambda *s: torch.zeros(*s, device=cuda, dtype=torch.uint8)
    # [rows, cols] with row stride `ld` inside a buffer that holds it
    o.strided = lambda rows, cols, ld: torch.zeros(rows * ld + 16, device=cuda).as_strided((rows, cols), (ld, 1))
    return o


def front(k, **over):
    """Valid operands of the front-conv bindings (batch B of a 4-row uint8 shard)."""
    a = dict(x=k.u(4, 784), idx=k.l(B), labels=k.l(4), w=k.f(288), b=k.f(32), y=k.f(B, 5408), dy=k.f(B, 5408),
             am=k.u(B, 5408), slab=k.f(B, 320), loss=k.f(B), s0w=k.f(288), s1w=k.f(288), s0b=k.f(32), s1b=k.f(32),
             lab_out=k.l(B), B=B)
    a.update(over)
    return a


def conv_fwd(k, lab_in=None, lab_out=None, **o):
    a = front(k, **o)
    k.C.conv_fwd(a["x"], a["idx"], a["B"], a["w"], a["b"], a["y"], a["am"], lab_in, lab_out)


def conv_fwd_pending(k, pslab=None, pB=B, **o):
    a = front(k, **o)
    k.C.conv_fwd_pending(a["x"], a["idx"], a["B"], a["w"], a["b"], a["y"], a["am"], a["labels"], a["lab_out"],
                         k.f(B, 320) if pslab is None else pslab, pB, a["s0w"], a["s1w"], a["s0b"], a["s1b"], *OPT)


def conv_local_step(k, **o):
    a = front(k, **o)
    k.C.conv_local_step(a["x"], a["idx"], a["labels"], a["B"], a["w"], a["b"], a["slab"], a["loss"], a["s0w"],
                        a["s1w"], a["s0b"], a["s1b"], *OPT)


def conv_local_epoch(k, order=None, kind=2, ws=None, **o):
    a = front(k, loss=k.f(4), **o)
    k.C.conv_local_epoch(a["x"], k.l(4) if order is None else order, a["labels"], a["B"], a["w"], a["b"], a["slab"],
                         a["loss"], a["s0w"], a["s1w"], a["s0b"], a["s1b"], kind, *OPT[1:7], 0,
                         k.f(8192) if ws is None else ws)


def alice12(k, **o):
    a = front(k, loss=k.f(4), **o)
    return (a["x"], k.l(4), a["labels"], a["w"], a["b"], a["s0w"], a["s1w"], a["s0b"], a["s1b"],
            k.f(2 * B * 320 + 2 * 960), a["loss"], 0)


def epoch_multi(k, alices, Bm=B, kind=2, table=None):
    k.C.conv_local_epoch_multi(alices, Bm, kind, *OPT[1:7], k.u(1 << 16) if table is None else table)


def conv_bwd_step(k, **o):
    a = front(k, **o)
    k.C.conv_bwd_step(a["dy"], a["y"], a["am"], a["x"], a["idx"], a["B"], a["w"], a["b"], a["slab"], a["s0w"],
                      a["s1w"], a["s0b"], a["s1b"], *OPT)


def conv_bwd_defer(k, pslab=None, pB=0, **o):
    a = front(k, **o)
    k.C.conv_bwd_defer(a["dy"], a["y"], a["am"], a["x"], a["idx"], a["B"], a["w"], a["b"], a["slab"],
                       a["slab"] if pslab == "same" else pslab, pB, a["s0w"], a["s1w"], a["s0b"], a["s1b"], *OPT)


def head_step(k, X=None, W=None, b="d", y=None, dX=None, s0w=None, s0b="d"):
    X = k.f(2, 8) if X is None else X
    W = k.f(3, 8) if W is None else W
    M, C = X.size(0), W.size(0)
    k.C.head_step(X, W, k.f(C) if isinstance(b, str) else b, k.l(M) if y is None else y, -100, 0.5, False, k.f(M),
                  k.f(M, 8) if dX is None else dX, k.f(C, 8) if s0w is None else s0w, k.f(C, 8),
                  k.f(C) if isinstance(s0b, str) else s0b, k.f(C), *OPT)


def linear_fwd(k, X=None, W=None, bias=None, Y=None, ws=None):
    k.C.linear_fwd(k.f(2, 8) if X is None else X, k.f(3, 8) if W is None else W, bias,
                   k.f(2, 3) if Y is None else Y, True, 0.0, 0, 0, 0, ws)


def dgrad(k, fn, dZ=None, W=None, hprev=None, dX=None, ws=None):
    getattr(k.C, fn)(k.f(2, 4) if dZ is None else dZ, k.f(4, 8) if W is None else W, hprev, 1.0,
                     k.f(2, 8) if dX is None else dX, ws)


def wgrad_opt(k, kind=2, A=None, s0=None, s1="d", bias=None, sb0=None):
    k.C.linear_wgrad_opt(k.f(2, 4), k.f(2, 8) if A is None else A, k.f(4, 8), k.f(4, 8) if s0 is None else s0,
                         k.f(4, 8) if isinstance(s1, str) else s1, bias, sb0, None, kind, *OPT[1:])


def multi_opt(k, ps=None, gs=None, s0s=None, s1s=None, opt=OPT, gscale=None):
    one = lambda v: [k.f(8)] if v is None else v
    k.C.multi_opt(one(ps), one(gs), one(s0s), one(s1s), *opt, gscale)


def conv3(k, x=None, w=None, bias=None, y=None, am=None, pad=1, pool=0):
    k.C.conv3x3_fwd(k.f(1, 2, 4, 4) if x is None else x, k.f(3, 2, 3, 3) if w is None else w, bias,
                    k.f(1, 3, 4, 4) if y is None else y, am, pad, True, pool)


def gn_fwd(k, x=None, w="d", b="d", y=None, mean=None, am=None, groups=2, pool=0):
    x = k.f(1, 4, 3) if x is None else x
    k.C.group_norm_fwd(x, k.f(4) if isinstance(w, str) else w, k.f(4) if isinstance(b, str) else b,
                       k.f(*x.shape) if y is None else y, k.f(1, 2) if mean is None else mean, k.f(1, 2), am, groups,
                       1e-5, False, pool)


def gn_bwd(k, affine=True, dy=None, dx="d", ws="d", dw="d", am=None):
    v = lambda: k.f(4) if affine else None
    k.C.group_norm_bwd(k.f(1, 4, 3) if dy is None else dy, k.f(1, 4, 3), k.f(1, 2), k.f(1, 2), v(), v(), am,
                       k.f(1, 4, 3) if isinstance(dx, str) else dx, (k.f(1, 4, 2) if affine else None) if
                       isinstance(ws, str) else ws, v() if isinstance(dw, str) else dw, v(), 2, False, 0)


def cut_pack(k, x=None, payload=None, scales=None, bits=8, group=16):
    k.C.cut_pack(k.f(2, 16) if x is None else x,
                 torch.zeros(2, 16, device=k.dev, dtype=torch.int8) if payload is None else payload,
                 k.f(2, 1) if scales is None else scales, bits, group, 0, False)


def softmax_ce(k, x=None, y=None, loss=None, d=None):
    k.C.softmax_ce(k.f(2, 4) if x is None else x, k.l(2) if y is None else y, -100, 0.5,
                   k.f(2) if loss is None else loss, d)


def head3(k, P2=None, W3=None, y=None, h2=None, dlog=None, G=1, gscale=None):
    k.C.server_head3(k.f(2, 8) if P2 is None else P2, k.f(8), True, 0.0, 0, 0, k.f(4, 8) if W3 is None else W3,
                     k.f(4), k.l(2) if y is None else y, -100, 0.5, k.f(2, 8) if h2 is None else h2,
                     k.f(2, 4) if dlog is None else dlog, k.f(2, 8), k.f(2), k.f(8192), G, gscale)


def layer8(k, dz=None, A=None, s0=None, s1="d", bias="d", sb0="d"):
    d = lambda v, mk: mk() if isinstance(v, str) else v
    return (k.f(2, 4) if dz is None else dz, k.f(2, 8) if A is None else A, k.f(4, 8),
            k.f(4, 8) if s0 is None else s0, d(s1, lambda: k.f(4, 8)), d(bias, lambda: k.f(4)),
            d(sb0, lambda: k.f(4)), k.f(4))


def wgrad_group(k, layers, xn=None, pn=None):
    k.C.wgrad_group(layers, 2, xn, pn, *OPT)


def tail_layers(k, kind=2, **over):
    """Valid {W, b, s0, s1, sb0, sb1} dicts of a 3-layer tail 8 -> 8 -> 4 -> 4."""
    out = []
    for n, kk in ((8, 8), (4, 8), (4, 4)):
        d = dict(W=k.f(n, kk), b=k.f(n), s0=k.f(n, kk), sb0=k.f(n))
        if kind == 2:
            d.update(s1=k.f(n, kk), sb1=k.f(n))
        out.append(d)
    for key, v in over.items():
        if v is None:
            del out[0][key]
        else:
            out[0][key] = v
    return out


def tail_cfg(k, kind=2, layers=None, **over):
    cfg = dict(layers=tail_layers(k, kind) if layers is None else layers, kind=kind, lr=1e-3, beta1=0.9, beta2=0.999,
               eps=1e-8, wd=0.0, momentum=0.0, p1=0.0, p2=0.0, col_off1=0, row2=False, comm=None, ipc=None, B=2,
               **{w: k.f(8192) for w in ("pn", "p2ws", "fwdws", "dgws", "headws", "h1", "h2", "dz1", "dz2", "dlog")})
    cfg.update(over)
    return cfg


def split_cfg(k, **over):
    p = lambda *s: dict(p=k.f(*s), s0=k.f(*s), s1=k.f(*s))
    cfg = dict(mode=1, B=2, x=k.u(4, 784), y=k.l(4), front=dict(w=p(288), b=p(32)),
               front_opt=dict(kind=2, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, wd=0.0, momentum=0.0),
               bob_opt=dict(kind=2, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, wd=0.0, momentum=0.0),
               tail=[dict(w=p(8, 5408), b=p(8)), dict(w=p(4, 8), b=p(4)), dict(w=p(4, 4), b=p(4))], p1=0.0, p2=0.0)
    cfg.update(over)
    return cfg


def six(k, *shape, **over):
    n = shape[0]
    d = dict(W=k.f(*shape), m=k.f(*shape), v=k.f(*shape), b=k.f(n), mb=k.f(n), vb=k.f(n))
    d.update(over)
    return d


# (id, call taking k, a word of the refusal)
CASES = [
    # ---- the shared tensor checks
    ("f32_dtype", lambda k: linear_fwd(k, X=k.d(2, 8)), "float32"),
    ("col_stride", lambda k: linear_fwd(k, X=k.f(2, 16)[:, ::2]), "unit column stride"),
    ("row_stride_5", lambda k: linear_fwd(k, X=k.strided(2, 4, 5), W=k.f(3, 4)), "16-byte aligned"),
    # ---- linear
    ("fwd_W_K", lambda k: linear_fwd(k, W=k.f(3, 12)), "W must be"),
    ("fwd_K_6", lambda k: linear_fwd(k, X=k.f(2, 8)[:, :6], W=k.f(3, 8)[:, :6]), "K % 4"),
    ("fwd_Y_shape", lambda k: linear_fwd(k, Y=k.f(3, 3)), "Y must be"),
    ("fwd_bias", lambda k: linear_fwd(k, bias=k.f(4)), "bias"),
    ("fwd_ws_strided", lambda k: linear_fwd(k, ws=k.f(8192)[::2]), "ws contiguous"),
    ("epi_P3", lambda k: k.C.linear_epilogue(k.f(2, 3, 3), None, k.f(2, 3), True, 0.0, 0, 0, 0), r"P \[S,M,N\]"),
    ("epi_P2", lambda k: k.C.linear_epilogue(k.f(3, 3), None, k.f(2, 3), True, 0.0, 0, 0, 0), "P/Y"),
    ("epi_bias", lambda k: k.C.linear_epilogue(k.f(2, 3), k.f(4), k.f(2, 3), True, 0.0, 0, 0, 0), "bias"),
    ("dgrad_W", lambda k: dgrad(k, "linear_dgrad", W=k.f(8, 8)), "W must be"),
    ("dgrad_dX", lambda k: dgrad(k, "linear_dgrad", dX=k.f(3, 8)), "dX must be"),
    ("dgrad_hprev", lambda k: dgrad(k, "linear_dgrad", hprev=k.f(3, 8)), "hprev"),
    ("dgrad_ws_strided", lambda k: dgrad(k, "linear_dgrad", ws=k.f(8192)[::2]), "ws contiguous"),
    ("nn_dgrad_W", lambda k: dgrad(k, "gemm_nn_dgrad", W=k.f(8, 8)), "W must be"),
    ("nn_dgrad_N_6", lambda k: dgrad(k, "gemm_nn_dgrad", dZ=k.f(2, 8)[:, :6], W=k.f(6, 8)), "% 4"),
    ("nn_dgrad_rows", lambda k: dgrad(k, "gemm_nn_dgrad", dZ=k.strided(2, 4, 5)), "16-B aligned"),
    ("nn_dgrad_dX", lambda k: dgrad(k, "gemm_nn_dgrad", dX=k.f(3, 8)), "dX must be"),
    ("nn_dgrad_hprev", lambda k: dgrad(k, "gemm_nn_dgrad", hprev=k.f(3, 8)), "hprev"),
    ("wgrad_shapes", lambda k: wgrad_opt(k, A=k.f(3, 8)), "shapes"),
    ("wgrad_s0_stride", lambda k: wgrad_opt(k, s0=k.f(4, 12)[:, :8]), "s0 like W"),
    ("wgrad_s1_shape", lambda k: wgrad_opt(k, s1=k.f(5, 8)), "s1"),
    ("wgrad_adam_no_s1", lambda k: wgrad_opt(k, s1=None), "Adam needs s1"),
    ("wgrad_bias_state", lambda k: wgrad_opt(k, bias=k.f(4)), "bias state"),
    ("partial_W", lambda k: k.C.linear_fwd_partial(k.f(2, 8), k.f(4, 12), k.f(8192), 4), "W must be"),
    ("partial_ws", lambda k: k.C.linear_fwd_partial(k.f(2, 8), k.f(4, 8), k.f(8192)[::2], 4), "ws contiguous"),
    ("opt_flat_sizes", lambda k: k.C.opt_flat(k.f(8), k.f(16), k.f(8), None, *SGD), "sizes"),
    ("opt_flat_strided", lambda k: k.C.opt_flat(k.f(8), k.f(16)[::2], k.f(8), None, *SGD), "contiguous"),
    ("adam_t0", lambda k: k.C.opt_flat(k.f(8), k.f(8), k.f(8), k.f(8), *OPT[:7], 0, 0), "step count"),
    # ---- multi-tensor optimizer
    ("mo_kind", lambda k: multi_opt(k, opt=(0,) + OPT[1:]), "kind"),
    ("mo_grads", lambda k: multi_opt(k, gs=[k.f(8), k.f(8)]), "one gradient"),
    ("mo_s0", lambda k: multi_opt(k, s0s=[k.f(8), k.f(8)]), "one s0"),
    ("mo_s1", lambda k: multi_opt(k, s1s=[]), "Adam needs"),
    ("mo_grad_numel", lambda k: multi_opt(k, gs=[k.f(16)]), "grad must be"),
    ("mo_param_strided", lambda k: multi_opt(k, ps=[k.f(16)[::2]]), "params"),
    ("mo_gscale", lambda k: multi_opt(k, gscale=k.d(1)), "gscale"),
    ("mo_cpu_param", lambda k: multi_opt(k, ps=[torch.zeros(8)]), "GPU tensor"),
    ("gn_grads_strided", lambda k: k.C.grad_norm([k.f(16)[::2]], 1.0, k.f(3), k.f(64)), "grads"),
    ("gn_out3_dtype", lambda k: k.C.grad_norm([k.f(8)], 1.0, k.d(3), k.f(64)), "out3"),
    # ---- the front conv
    ("x_dtype", lambda k: conv_fwd(k, x=k.l(4, 784)), "uint8 or float32"),
    ("x_numel", lambda k: conv_fwd(k, x=k.u(4, 785)), r"\[N,784\]"),
    ("conv_params", lambda k: conv_fwd(k, w=k.f(300)), "conv params"),
    ("idx_int32", lambda k: conv_fwd(k, idx=k.i(2 * B)), "idx int64"),
    ("y_dtype", lambda k: conv_fwd(k, y=k.d(B, 5408)), "float32"),
    ("am_dtype", lambda k: conv_fwd(k, am=k.f(B, 5408)), "am"),
    ("lab_pair", lambda k: conv_fwd(k, lab_in=k.l(4)), "go together"),
    ("lab_in_N", lambda k: conv_fwd(k, lab_in=k.l(8), lab_out=k.l(B)), "lab_in"),
    ("lab_out_int32", lambda k: conv_fwd(k, lab_in=k.l(4), lab_out=k.i(2 * B)), "lab_out"),
    ("pending_lab_in", lambda k: conv_fwd_pending(k, labels=k.l(8)), "lab_in"),
    ("pending_batch", lambda k: conv_fwd_pending(k, pB=0), "pending batch"),
    ("pending_state", lambda k: conv_fwd_pending(k, s0w=k.f(300)), "optimizer state"),
    ("pending_slab_dtype", lambda k: conv_fwd_pending(k, pslab=k.d(B, 320)), "slab"),
    ("step_labels_int32", lambda k: conv_local_step(k, labels=k.i(8)), "labels int64"),
    ("step_loss_dtype", lambda k: conv_local_step(k, loss=k.d(B)), "loss_rows"),
    ("step_state", lambda k: conv_local_step(k, s0b=k.f(64)), "optimizer state"),
    ("step_slab_strided", lambda k: conv_local_step(k, slab=k.f(B, 640)[:, ::2]), "slab"),
    ("epoch_batch", lambda k: conv_local_epoch(k, B=5000, slab=k.f(5000, 320)), "batch size"),
    ("epoch_order_2d", lambda k: conv_local_epoch(k, order=k.l(2, 2)), "order"),
    ("epoch_kind", lambda k: conv_local_epoch(k, kind=0), "SGD-momentum or Adam"),
    ("epoch_labels", lambda k: conv_local_epoch(k, labels=k.l(8)), "labels"),
    ("epoch_ws_strided", lambda k: conv_local_epoch(k, ws=k.f(16384)[::2]), "ws contiguous"),
    ("multi_65", lambda k: epoch_multi(k, [alice12(k)] * 65), "Alices"),
    ("multi_batch", lambda k: epoch_multi(k, [alice12(k)], Bm=2000), "batch size"),
    ("multi_kind", lambda k: epoch_multi(k, [alice12(k)], kind=0), "SGD-momentum or Adam"),
    ("multi_table", lambda k: epoch_multi(k, [alice12(k)], table=k.i(1 << 14)), "table"),
    ("multi_tuple", lambda k: epoch_multi(k, [alice12(k)[:11]]), "alice tuple"),
    ("multi_f32_shard", lambda k: epoch_multi(k, [alice12(k, x=k.f(4, 784))]), "uint8"),
    ("multi_labels_strided", lambda k: epoch_multi(k, [alice12(k, labels=k.l(8)[::2])]), "labels"),
    ("multi_adam_no_s1", lambda k: epoch_multi(k, [alice12(k, s1w=None)]), "Adam second moments"),
    ("fwd_multi_17", lambda k: k.C.conv_fwd_multi([(k.u(4, 784), None, 2, k.f(288), k.f(32), k.f(2, 5408))] * 17, 2),
     "16 Alices"),
    ("fwd_multi_chunk", lambda k: k.C.conv_fwd_multi([(k.u(4, 784), None, 2, k.f(288), k.f(32), k.f(2, 5408))], 70000),
     "chunk"),
    ("fwd_multi_n", lambda k: k.C.conv_fwd_multi([(k.u(4, 784), None, -1, k.f(288), k.f(32), k.f(2, 5408))], 2), "n"),
    ("fwd_multi_f32", lambda k: k.C.conv_fwd_multi([(k.f(4, 784), None, 2, k.f(288), k.f(32), k.f(2, 5408))], 2),
     "uint8"),
    ("fwd_multi_tuple", lambda k: k.C.conv_fwd_multi([(k.u(4, 784), None, 2, k.f(288), k.f(32))], 2), "alice tuple"),
    ("bwd_dy_strided", lambda k: conv_bwd_step(k, dy=k.f(B, 10816)[:, ::2]), "dy/y"),
    ("bwd_am_dtype", lambda k: conv_bwd_step(k, am=k.f(B, 5408)), "am"),
    ("bwd_state", lambda k: conv_bwd_step(k, s0w=k.f(300)), "optimizer state"),
    ("defer_same_slab", lambda k: conv_bwd_defer(k, pslab="same", pB=B), "differ"),
    ("defer_pending_batch", lambda k: conv_bwd_defer(k, pslab=k.f(B, 320), pB=0), "pending batch"),
    ("apply_batch", lambda k: k.C.conv_apply(k.f(B, 320), 0, k.f(288), k.f(32), k.f(288), None, k.f(32), None, *SGD),
     "pending batch"),
    ("apply_params", lambda k: k.C.conv_apply(k.f(B, 320), B, k.f(300), k.f(32), k.f(288), None, k.f(32), None, *SGD),
     "conv params"),
    # ---- U-shape head
    ("head_1025", lambda k: head_step(k, X=k.f(41, 8), W=k.f(25, 8)), "too large"),
    ("head_W_K", lambda k: head_step(k, W=k.f(3, 12), s0w=k.f(3, 12)), "contiguous"),
    ("head_labels_int32", lambda k: head_step(k, y=k.i(4)), "labels int64"),
    ("head_dX", lambda k: head_step(k, dX=k.f(3, 8)), "outputs"),
    ("head_state", lambda k: head_step(k, s0w=k.f(4, 8)), "state"),
    ("head_bias_state", lambda k: head_step(k, s0b=None), "bias state"),
    # ---- general 3x3 conv
    ("c3_w_cin", lambda k: conv3(k, w=k.f(3, 4, 3, 3)), "w must be"),
    ("c3_pad", lambda k: conv3(k, pad=2), "padding"),
    ("c3_pool", lambda k: conv3(k, pool=3), "pool"),
    ("c3_small", lambda k: conv3(k, x=k.f(1, 2, 2, 4), y=k.f(1, 3, 2, 4)), "too small"),
    ("c3_am_without_pool", lambda k: conv3(k, am=k.u(1, 3, 4, 4)), "am goes with pooling"),
    ("c3_pool_without_am", lambda k: conv3(k, pool=2, y=k.f(1, 3, 2, 2)), "am goes with pooling"),
    ("c3_am_dtype", lambda k: conv3(k, pool=2, y=k.f(1, 3, 2, 2), am=k.f(1, 3, 2, 2)), "uint8"),
    ("c3_y_shape", lambda k: conv3(k, y=k.f(1, 3, 5, 5)), "y must be"),
    ("c3_x_dtype", lambda k: conv3(k, x=k.d(1, 2, 4, 4)), "float32"),
    ("c3_x_strided", lambda k: conv3(k, x=k.f(1, 2, 4, 8)[..., ::2]), "contiguous"),
    ("c3_bias", lambda k: conv3(k, bias=k.f(4)), "bias"),
    ("c3_dgrad_dy", lambda k: k.C.conv3x3_dgrad(k.f(1, 3, 5, 5), k.f(1, 3, 4, 4), None, k.f(3, 2, 3, 3),
                                                 k.f(1, 2, 4, 4), 1, True, 0), "dy must be"),
    ("c3_wgrad_db", lambda k: k.C.conv3x3_wgrad(k.f(1, 3, 4, 4), k.f(1, 3, 4, 4), None, k.f(1, 2, 4, 4), k.f(8192),
                                                 k.f(3, 2, 3, 3), k.f(4), 1, True, 0), "db"),
    # ---- GroupNorm
    ("gn_groups", lambda k: gn_fwd(k, groups=3), "multiple of the groups"),
    ("gn_pool_3d", lambda k: gn_fwd(k, pool=2), "pooling needs"),
    ("gn_pool_value", lambda k: gn_fwd(k, pool=3), "pool"),
    ("gn_y_shape", lambda k: gn_fwd(k, y=k.f(1, 4, 4)), "x's shape"),
    ("gn_mean", lambda k: gn_fwd(k, mean=k.f(1, 3)), "mean"),
    ("gn_affine_pair", lambda k: gn_fwd(k, b=None), "go together"),
    ("gn_weight", lambda k: gn_fwd(k, w=k.f(5), b=k.f(5)), "weight"),
    ("gn_am_without_pool", lambda k: gn_fwd(k, am=k.u(1, 4, 3)), "am goes with pooling"),
    ("gn_pooled_y", lambda k: gn_fwd(k, x=k.f(1, 4, 4, 4), pool=2, y=k.f(1, 4, 4, 4), am=k.u(1, 4, 2, 2)), "H / 2"),
    ("gn_bwd_dw", lambda k: gn_bwd(k, affine=False, dw=k.f(4)), "go together"),
    ("gn_bwd_ws", lambda k: gn_bwd(k, affine=False, ws=k.f(1, 4, 2)), "workspace goes with"),
    ("gn_bwd_dx", lambda k: gn_bwd(k, dx=k.f(1, 4, 4)), "dx must have"),
    ("gn_bwd_dy", lambda k: gn_bwd(k, dy=k.f(1, 4, 4)), "x's shape"),
    # ---- cut codec
    ("cut_group_24", lambda k: cut_pack(k, group=24), "group"),
    ("cut_bits", lambda k: cut_pack(k, bits=5), "bits"),
    ("cut_payload_dtype", lambda k: cut_pack(k, payload=k.u(2, 16)), "int8"),
    ("cut_payload_shape", lambda k: cut_pack(k, payload=torch.zeros(2, 32, device=k.dev, dtype=torch.int8)),
     "payload must be"),
    ("cut_scales_shape", lambda k: cut_pack(k, scales=k.f(2, 2)), "scales must be"),
    ("cut_x_3d", lambda k: cut_pack(k, x=k.f(2, 4, 4)), "2-D"),
    ("cut_roundtrip_y", lambda k: k.C.cut_roundtrip(k.f(2, 16), k.f(2, 32), 8, 16, 0, False), "y must have"),
    # ---- loss / metrics
    ("ce_labels_int32", lambda k: softmax_ce(k, y=k.i(4)), "labels"),
    ("ce_dlogits", lambda k: softmax_ce(k, d=k.f(3, 4)), "dlogits"),
    ("ce_loss_dtype", lambda k: softmax_ce(k, loss=k.d(2)), "loss_rows"),
    ("relu_mask_sizes", lambda k: k.C.relu_mask(k.f(8), k.f(16), 1.0, k.f(8)), "one size"),
    ("eval_labels_int32", lambda k: k.C.eval_counters(k.f(2, 4), k.i(4), -1, k.l(6)), "labels"),
    ("eval_counters_int32", lambda k: k.C.eval_counters(k.f(2, 4), k.l(2), -1, k.i(12)), "counters"),
    # ---- fused server step
    ("h3_P2_dim", lambda k: head3(k, P2=k.f(16)), "P2"),
    ("h3_W3", lambda k: head3(k, W3=k.f(4, 12)), "W3"),
    ("h3_groups", lambda k: head3(k, G=3), "groups"),
    ("h3_labels", lambda k: head3(k, y=k.l(4)), "labels"),
    ("h3_gscale", lambda k: head3(k, gscale=k.f(4)), "gscale"),
    ("h3_h2", lambda k: head3(k, h2=k.f(3, 8)), "h2/dz2"),
    ("h3_dlog", lambda k: head3(k, dlog=k.f(3, 4)), "dlog"),
    ("wg_4_layers", lambda k: wgrad_group(k, [layer8(k)] * 4), "1..3 layers"),
    ("wg_tuple", lambda k: wgrad_group(k, [layer8(k)[:7]]), "layer tuple"),
    ("wg_A", lambda k: wgrad_group(k, [layer8(k, A=k.f(3, 8))]), r"A \[M,K\]"),
    ("wg_s0", lambda k: wgrad_group(k, [layer8(k, s0=k.f(4, 12)[:, :8])]), "s0 like W"),
    ("wg_adam_no_s1", lambda k: wgrad_group(k, [layer8(k, s1=None)]), "s1"),
    ("wg_bias_state", lambda k: wgrad_group(k, [layer8(k, sb0=None)]), "bias state"),
    ("wg_dz", lambda k: wgrad_group(k, [layer8(k, dz=k.f(3, 4))]), r"dz \[M,N\]"),
    ("wg_xn_without_pn", lambda k: wgrad_group(k, [layer8(k)], xn=k.f(2, 8)), "pn needed"),
    ("wg_xn_rows", lambda k: wgrad_group(k, [layer8(k)], xn=k.f(65, 8), pn=k.f(8192)), "xn"),
    # ---- module switches and the hand-off stress entry
    ("variant_slot", lambda k: k.C.set_variant(24, 0), "variant slot"),
    ("compute_dtype", lambda k: k.C.set_compute_dtype("fp16"), "compute dtype"),
    ("handoff_workgroups", lambda k: k.C.handoff_stress(12, 64, 1, 1, 1, 0, 0.0, 1.0), "workgroups"),
    ("handoff_mode", lambda k: k.C.handoff_stress(8, 64, 1, 1, 1, 9, 0.0, 1.0), "mode"),
    # ---- executors: constructors and the operands of run()
    ("server_2_layers", lambda k: k.C.ServerEpoch(tail_cfg(k, layers=tail_layers(k)[:2])), "3-layer"),
    ("server_missing_W", lambda k: k.C.ServerEpoch(tail_cfg(k, layers=tail_layers(k, W=None))), "missing 'W'"),
    ("server_f64", lambda k: k.C.ServerEpoch(tail_cfg(k, layers=tail_layers(k, b=k.d(8)))), "f32 GPU"),
    ("server_K_6", lambda k: k.C.ServerEpoch(tail_cfg(k, layers=tail_layers(k, W=k.f(8, 6), s0=k.f(8, 6)))), "K % 4"),
    ("server_state", lambda k: k.C.ServerEpoch(tail_cfg(k, layers=tail_layers(k, sb0=k.f(9)))), "layer state shapes"),
    ("server_chain", lambda k: k.C.ServerEpoch(tail_cfg(k, layers=tail_layers(k, W=k.f(12, 8), s0=k.f(12, 8),
                                                                              s1=k.f(12, 8), b=k.f(12), sb0=k.f(12)))),
     "chain"),
    ("server_kind", lambda k: k.C.ServerEpoch(tail_cfg(k, kind=0)), "SGD-momentum or Adam"),
    ("server_adam_no_s1", lambda k: k.C.ServerEpoch(tail_cfg(k, layers=tail_layers(k, s1=None))), "Adam v"),
    ("server_row2", lambda k: k.C.ServerEpoch(tail_cfg(k, row2=True)), "communicator"),
    ("server_groups", lambda k: k.C.ServerEpoch(tail_cfg(k, groups=3)), "groups"),
    ("server_batch", lambda k: k.C.ServerEpoch(tail_cfg(k, B=65)), "batch 1..64"),
    ("server_run_acts", lambda k: k.C.ServerEpoch(tail_cfg(k)).run(k.f(2, 12), k.l(2), k.f(2), 0, 0, 0, False, True),
     "acts"),
    ("server_run_labels", lambda k: k.C.ServerEpoch(tail_cfg(k)).run(k.f(2, 8), k.i(4), k.f(2), 0, 0, 0, False, True),
     "labels int64"),
    ("server_run_loss", lambda k: k.C.ServerEpoch(tail_cfg(k)).run(k.f(2, 8), k.l(2), k.d(2), 0, 0, 0, False, True),
     "loss"),
    ("server_run_gscale", lambda k: k.C.ServerEpoch(tail_cfg(k, groups=2)).run(k.f(2, 8), k.l(2, 2), k.f(2, 2), 0, 0, 0,
                                                                              False, True, None), "gscale"),
    ("server_emulate", lambda k: k.C.ServerEpoch(tail_cfg(k, emulate_tp=True)).run(k.f(2, 8), k.l(2), k.f(2), 0, 0, 0,
                                                                                  False, True), "tp_emulate_epoch"),
    ("emulate_losses", lambda k: k.C.tp_emulate_epoch([k.C.ServerEpoch(tail_cfg(k, emulate_tp=True))], k.f(2, 8),
                                                      k.l(2), [], 0, 0, 0, False, True), "one loss buffer"),
    ("resident_missing_s1", lambda k: k.C.ResidentEpoch(tail_cfg(k, layers=tail_layers(k, s1=None))), "missing 's1'"),
    ("resident_none", lambda k: k.C.ResidentEpoch(tail_cfg(k, layers=tail_layers(k)[:2] + [dict(tail_layers(k)[2],
                                                                                                  b=None)])),
     "missing 'b'"),
    ("resident_kind", lambda k: k.C.ResidentEpoch(tail_cfg(k, kind=3)), "SGD-momentum or Adam"),
    ("resident_f64", lambda k: k.C.ResidentEpoch(tail_cfg(k, layers=tail_layers(k, sb1=k.d(8)))), "f32 GPU"),
    ("resident_shapes", lambda k: k.C.ResidentEpoch(tail_cfg(k, layers=tail_layers(k, b=k.f(9)))), "layer shapes"),
    ("hybrid_2_layers", lambda k: k.C.HybridEpoch(tail_cfg(k, layers=tail_layers(k)[:2])), "3-layer"),
    ("hybrid_missing", lambda k: k.C.HybridEpoch(tail_cfg(k, layers=tail_layers(k, sb0=None))), "missing 'sb0'"),
    ("hybrid_strided", lambda k: k.C.HybridEpoch(tail_cfg(k, layers=tail_layers(k, b=k.f(16)[::2]))), "f32 GPU"),
    ("hybrid_chain", lambda k: k.C.HybridEpoch(tail_cfg(k, layers=tail_layers(k, W=k.f(12, 8), s0=k.f(12, 8),
                                                                              b=k.f(12)))), "chain"),
    ("vanilla_layer_shapes", lambda k: k.C.VanillaEpoch(tail_cfg(k, kind=1, layers=tail_layers(k, 1, sb0=k.f(9)))),
     "layer shapes"),
    ("vanilla_conv", lambda k: k.C.VanillaEpoch(tail_cfg(k, kind=1, layers=tail_layers(k, 1), alice=dict(
        w=k.f(300), b=k.f(32), s0w=k.f(300), s0b=k.f(32)))), "conv 32"),
    ("vanilla_x", lambda k: k.C.VanillaEpoch(tail_cfg(k, kind=1, layers=tail_layers(k, 1), x=k.f(4, 784), y=k.l(4),
                                                      alice=dict(w=k.f(288), b=k.f(32), s0w=k.f(288), s0b=k.f(32)))),
     "shard pixels"),
    ("vanilla_y", lambda k: k.C.VanillaEpoch(tail_cfg(k, kind=1, layers=tail_layers(k, 1), x=k.u(4, 784), y=k.l(8),
                                                      alice=dict(w=k.f(288), b=k.f(32), s0w=k.f(288), s0b=k.f(32)))),
     "labels int64"),
    ("vanilla_channel", lambda k: k.C.VanillaEpoch(tail_cfg(k, kind=1, layers=tail_layers(k, 1), channel=object())),
     "IpcChannel"),
    ("ushape_f64", lambda k: k.C.UShapeEpoch(dict(fc1=six(k, 8, 5408, b=k.d(8)))), "f32 GPU"),
    ("ushape_missing", lambda k: k.C.UShapeEpoch(dict(fc1=six(k, 8, 5408, vb=None))), "missing 'vb'"),
    ("ushape_moments", lambda k: k.C.UShapeEpoch(dict(fc1=six(k, 8, 5408, mb=k.f(9)))), "moment shapes"),
    ("split_mode", lambda k: k.C.SplitEpoch(split_cfg(k, mode=3)), "mode"),
    ("split_batch", lambda k: k.C.SplitEpoch(split_cfg(k, B=65)), "batch"),
    ("split_role", lambda k: k.C.SplitEpoch(split_cfg(k, role=3)), "role"),
    ("split_missing_x", lambda k: k.C.SplitEpoch({kk: v for kk, v in split_cfg(k).items() if kk != "x"}), "missing 'x'"),
    ("split_x", lambda k: k.C.SplitEpoch(split_cfg(k, x=k.f(4, 784))), "shard pixels"),
    ("split_y_strided", lambda k: k.C.SplitEpoch(split_cfg(k, y=k.l(8)[::2])), "shard labels"),
    ("split_param_dtype", lambda k: k.C.SplitEpoch(split_cfg(k, front=dict(
        w=dict(p=k.d(288), s0=k.f(288), s1=k.f(288)), b=dict(p=k.f(32), s0=k.f(32), s1=k.f(32))))), "contiguous f32"),
    ("split_state", lambda k: k.C.SplitEpoch(split_cfg(k, front=dict(
        w=dict(p=k.f(288), s0=None, s1=None), b=dict(p=k.f(32), s0=k.f(32), s1=k.f(32))))), "optimizer state"),
    ("split_front", lambda k: k.C.SplitEpoch(split_cfg(k, front=dict(
        w=dict(p=k.f(300), s0=k.f(300), s1=k.f(300)), b=dict(p=k.f(32), s0=k.f(32), s1=k.f(32))))), "conv front"),
    ("split_opt_kind", lambda k: k.C.SplitEpoch(split_cfg(k, front_opt=dict(split_cfg(k)["front_opt"], kind=0))),
     "SGD-momentum or Adam"),
    ("split_tail_count", lambda k: k.C.SplitEpoch(split_cfg(k, tail=split_cfg(k)["tail"][:2])), "3 layers"),
    ("split_cut_width", lambda k: k.C.SplitEpoch(split_cfg(k, tail=[
        dict(w=dict(p=k.f(8, 5412), s0=k.f(8, 5412), s1=None), b=dict(p=k.f(8), s0=k.f(8), s1=None))] +
        split_cfg(k)["tail"][1:])), "5408"),
    ("split_chain", lambda k: k.C.SplitEpoch(split_cfg(k, tail=split_cfg(k)["tail"][:2] + [
        dict(w=dict(p=k.f(4, 8), s0=k.f(4, 8), s1=None), b=dict(p=k.f(4), s0=k.f(4), s1=None))])), "chain"),
    ("split_workspace", lambda k: k.C.SplitEpoch(split_cfg(k, fwdws=k.d(1 << 16))), "contiguous f32"),
]


@pytest.mark.parametrize("call,word", [pytest.param(c, w, id=i) for i, c, w in CASES])
def test_refused(k, call, word):
    with pytest.raises(RuntimeError, match=word):
        call(k)
