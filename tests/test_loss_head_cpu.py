"""The loss and head kernels' cases on the CPU: softmax cross-entropy, the one-launch head step, the
evaluation counters, the softmax of server_head3 and relu_mask (csrc/loss.hip, csrc/fused.hip).

This file owns the inputs and the float64 references; tests/test_loss_head_gpu.py runs the same
cases on the HIP kernels.  Here the fp32 torch twin (ops/torch_ops.py) is held to the very bounds
the kernels are held to, which shows that a correct fp32 implementation can meet them, and the
twin's eval_counters is pinned on hand-written rows, since torch.argmax is the counters' definition.

Inputs.  Every builder is seeded with a torch.Generator on the CPU and returns fp32 tensors.  Where
a case is about large logits, the logits are exact in fp32 (multiples of 0.25, or sums of small
integers), so `x - max` is exact and the only error left is the softmax's own.

Bounds.
  loss   |loss - ref| <= 4 * 2^-23 * max|x_row| + 1e-5: `mx + log(s) - x[lab]` rounds twice at the
         magnitude of the row's largest logit (2 * 2^-24 * max|x| each way), doubled, plus the
         atol the project's loss tests already use.  max|x_row| is over the row's finite entries.
  d      rtol 1e-5, atol 1e-6 (tests/test_kernels_gpu.py test_softmax_ce).
  head   rtol 1e-5; atol 1e-5 loss, 1e-6 dX / W / b, 1e-7 optimizer state (_head_step_check); the
         large-logit variant's loss as `loss` above, with no relative part.
  head3  rtol 1e-4; atol 1e-6 dlogits / dz2, 1e-4 h2 (test_server_head3); the loss as above."""
import functools

import pytest
import torch

from splitlearning_amd.config import OptimCfg
from splitlearning_amd.ops import torch_ops

U = 2.0 ** -23
IGN = -100


def loss_atol(xmax):
    """The loss bound's absolute part per row, from that row's largest finite |logit| (float64)."""
    return 4 * U * xmax + 1e-5


def row_max(x):
    a = x.double().abs()
    return torch.where(torch.isfinite(a), a, torch.zeros_like(a)).amax(dim=1)


def worst(got, ref, rtol, atol):
    """max |got - ref| / (atol + rtol |ref|) in float64 (atol a number or a tensor broadcast over ref):
    <= 1 passes.  Both non-finite and different, or either alone, counts as infinitely wrong."""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    if got.numel() == 0:
        return 0.0
    if not (torch.isfinite(got).all() and torch.isfinite(ref).all()):
        return float("inf")
    return ((got - ref).abs() / (atol + rtol * ref.abs())).max().item()


# ---------------------------------------------------------------- 1. softmax cross-entropy
CE_C = [1, 63, 64, 65, 100, 512, 513, 1030]     # 64: the lane stride; 512 / 513: narrow -> wide kernel
CE_SHAPES = [(9, c) for c in CE_C] + [(1, 100), (1, 513)]
CE_INF_C = (100, 1030)                          # these get a tenth, hand-written row with one -inf


def ce64(x, y, scale):
    """(loss rows, dlogits) in float64 from the fp32 logits: logsumexp - x[lab]; scale (softmax - onehot)."""
    x = x.double()
    valid = y != IGN
    safe = torch.where(valid, y, torch.zeros_like(y)).view(-1, 1)
    loss = torch.where(valid, torch.logsumexp(x, dim=1) - x.gather(1, safe).squeeze(1), torch.zeros(x.shape[0], dtype=torch.float64))
    d = torch.softmax(x, dim=1)
    d.scatter_add_(1, safe, -torch.ones_like(safe, dtype=torch.float64))
    return loss, d * scale * valid.view(-1, 1)


@functools.lru_cache(maxsize=None)
def ce_case(M, C):
    """Logits that are multiples of 0.25.  M = 9: row 0 ignored, row 1 moderate (|x| <= 100), row 2
    all 7.0, row 3 labelled with the last column, the rest uniform in +-30000; at C = 100 and 1030 a
    tenth row with one -inf that the label is not on.  M = 1: one +-30000 row with a real label (an
    ignored one would leave the kernel nothing to compute)."""
    g = torch.Generator().manual_seed(1000 * M + C)
    x = torch.randint(-120000, 120001, (M, C), generator=g).float() * 0.25
    y = torch.randint(0, C, (M,), generator=g)
    if M > 1:
        y[0] = IGN
        x[1] = torch.randint(-400, 401, (C,), generator=g).float() * 0.25
        x[2] = 7.0
        y[3] = C - 1
        if C in CE_INF_C:
            r = torch.randint(-400, 401, (1, C), generator=g).float() * 0.25
            r[0, 17] = float("-inf")
            x, y = torch.cat([x, r]), torch.cat([y, torch.tensor([C - 2])])
    scale = 1.0 / x.shape[0]
    loss, d = ce64(x, y, scale)
    return dict(x=x, y=y, scale=scale, loss=loss, d=d, atol=loss_atol(row_max(x)))


def ce_check(c, loss, d, name):
    """The bounds of section 1 on a (loss, d) computed from case c; prints the figures first."""
    wl, wd = worst(loss, c["loss"], 0.0, c["atol"]), worst(d, c["d"], 1e-5, 1e-6)
    print(f"{name}: loss error / bound {wl:.3f}, d error / bound {wd:.3f}")
    assert wl <= 1 and wd <= 1
    ign = (c["y"] == IGN).nonzero().view(-1)
    assert not loss.cpu()[ign].any() and not d.cpu()[ign].any()     # ignored rows: exactly 0


@pytest.mark.parametrize("M,C", CE_SHAPES)
def test_twin_softmax_ce_meets_the_bounds(M, C):
    c = ce_case(M, C)
    assert torch.equal(c["x"] * 4, (c["x"] * 4).round()) or C in CE_INF_C
    if M > 1 and C > 1:
        assert row_max(c["x"])[4:9].min() > 10000
        if C in CE_INF_C:
            assert c["d"][9, 17] == 0 and c["d"][9].abs().sum() > 0 and torch.isfinite(c["loss"][9])
    loss, d = torch_ops.softmax_ce(c["x"], c["y"], c["scale"])
    ce_check(c, loss, d, f"twin softmax_ce {M}x{C}")


# ---------------------------------------------------------------- 2. the head step
# (M, K, C): which kernel csrc/loss.hip's launcher takes, and what the shape is there for
HEAD_SHAPES = [
    (16, 128, 16),      # MFMA: every bound at once, C K = 2048: all eight prefetch slots
    (1, 4, 1),          # MFMA: the smallest
    (7, 100, 10),       # MFMA: the shipped head at a short batch
    (17, 100, 10),      # FMA: the first M past the MFMA form
    (16, 100, 17),      # FMA: C > 16
    (8, 132, 8),        # FMA: K > 128; C K = 1056 takes the remainder loop past 4 x 256 state elements
    (25, 100, 40),      # FMA: C K = 4000, M C = 1000
    (64, 64, 16),       # FMA: M C = 1024 exactly
    (300, 12, 3),       # FMA: more rows than the workgroup has threads
    (3, 4, 300),        # FMA: more classes than the workgroup has threads (the bias step)
]
HEAD_LARGE = [(7, 100, 10), (17, 100, 10)]      # the large-logit variant, one shape per kernel
HEAD_MASKED = [(17, 100, 10), (300, 12, 3)]
HEAD_T = 3
HEAD_TOL = dict(loss=1e-5, dx=1e-6, W=1e-6, b=1e-6, state=1e-7)     # atol; rtol 1e-5 throughout
HEAD_RTOL = 1e-5


def head_cfg(kind):
    return (OptimCfg("adam", 1e-3, weight_decay=1e-5) if kind == "adam"
            else OptimCfg("sgd", 1e-2, momentum=0.9, weight_decay=1e-5))


def head_state(kind, p, g):
    """A non-trivial optimizer state for p: momenta around 0.01, second moments in [0.001, 0.021]."""
    m = torch.randn(p.shape, generator=g) * 0.01
    if kind == "adam":
        return {"m": m, "v": torch.rand(p.shape, generator=g) * 0.02 + 0.001}
    return {"buf": m}


def clone_state(st, dtype=None, device=None):
    return {k: v.clone().to(dtype=dtype, device=device) for k, v in st.items()}


def head_labels(M, C, g, ignore_only_row):
    y = torch.randint(0, C, (M,), generator=g)
    if M >= 2:
        y[0] = y[M - 1] = IGN
    elif ignore_only_row:
        y[0] = IGN
    return y


def head_reference(x, W, b, y, kind, sw, sb, masked, dtype):
    """The step in `dtype` from the fp32 inputs: logits, cross-entropy, dX = dlog @ W (with the
    [x > 0] mask), dW, db and torch_ops.apply_update_.  float64 gives the reference; float32 through
    the twin's own ops (linear_fwd, softmax_ce, linear_dgrad, linear_wgrad_step_) the precondition."""
    cfg, scale = head_cfg(kind), 1.0 / x.shape[0]
    X, Wn = x.to(dtype), W.to(dtype).clone()
    bn = None if b is None else b.to(dtype).clone()
    sw = clone_state(sw, dtype)
    sb = None if b is None else clone_state(sb, dtype)
    if dtype == torch.float64:
        logits = X @ Wn.t() if bn is None else X @ Wn.t() + bn
        loss, dlog = ce64(logits, y, scale)
        dx = dlog @ Wn
        if masked:
            dx = torch.where(X > 0, dx, torch.zeros_like(dx))
        torch_ops.apply_update_(Wn, dlog.t() @ X, sw, cfg, HEAD_T)
        if bn is not None:
            torch_ops.apply_update_(bn, dlog.sum(0), sb, cfg, HEAD_T)
    else:
        logits = torch_ops.linear_fwd(X, Wn, bn, False, 0.0, 0)
        loss, dlog = torch_ops.softmax_ce(logits, y, scale)
        dx = torch_ops.linear_dgrad(dlog, Wn, X if masked else None)
        torch_ops.linear_wgrad_step_(dlog, X, Wn, bn, cfg, sw, sb, HEAD_T)
    return dict(loss=loss, dx=dx, W=Wn, b=bn, sw=sw, sb=sb, logit_max=row_max(logits))


@functools.lru_cache(maxsize=None)
def head_case(M, K, C, kind, bias=True, large=False, ignore_only_row=False):
    """Inputs and the float64 result of one head step.  large: X, W and b are small integers, so the
    logits (up to about +-2000) are exact in fp32 in any order of summation."""
    g = torch.Generator().manual_seed(7919 * M + 31 * K + C + (1 if large else 0))
    if large:
        x = torch.randint(-16, 17, (M, K), generator=g).float()
        W = torch.randint(-16, 17, (C, K), generator=g).float()
        b = torch.randint(-3, 4, (C,), generator=g).float()
    else:
        x = torch.rand(M, K, generator=g)
        W, b = torch.randn(C, K, generator=g) * 0.1, torch.randn(C, generator=g) * 0.1
    y = head_labels(M, C, g, ignore_only_row)
    sw, sb = head_state(kind, W, g), head_state(kind, b, g)
    if not bias:
        b = sb = None
    ref = head_reference(x, W, b, y, kind, sw, sb, False, torch.float64)
    return dict(x=x, W=W, b=b, y=y, sw=sw, sb=sb, ref=ref, kind=kind, large=large)


def head_variants(M):
    """(bias, ignore_only_row): with and without a bias, and at M = 1 the lone row ignored too."""
    v = [(True, False), (False, False)]
    return v + [(True, True), (False, True)] if M == 1 else v


def head_check(c, got, name):
    """The bounds of section 2 on `got` (loss, dx, W, b, sw, sb as the kernel or the twin left them)
    against case c's float64 result; prints every figure, then asserts.  The large-logit variant's
    loss bound is section 1's, from the reference's own largest logit of each row."""
    ref = c["ref"]
    if c["large"]:          # section 1's bound has no relative part
        figs = {"loss": worst(got["loss"], ref["loss"], 0.0, loss_atol(ref["logit_max"]))}
    else:
        figs = {"loss": worst(got["loss"], ref["loss"], HEAD_RTOL, HEAD_TOL["loss"])}
    for k in ("dx", "W") + (("b",) if c["b"] is not None else ()):
        figs[k] = worst(got[k], ref[k], HEAD_RTOL, HEAD_TOL[k])
    for s in ("sw",) + (("sb",) if c["b"] is not None else ()):
        assert set(got[s]) == set(ref[s])
        for k in ref[s]:
            figs[f"{s}.{k}"] = worst(got[s][k], ref[s][k], HEAD_RTOL, HEAD_TOL["state"])
    print(f"{name}: error / bound " + ", ".join(f"{k} {v:.3f}" for k, v in figs.items()))
    bad = {k: v for k, v in figs.items() if not v <= 1}
    assert not bad, f"{name}: past the bound by the factor {bad}"
    ign = (c["y"] == IGN).nonzero().view(-1)
    assert not got["loss"].cpu()[ign].any() and not got["dx"].cpu()[ign].any()
    assert not torch.equal(got["W"].cpu().double(), c["W"].double())           # the step moved the weights


def _twin_head(c):
    return head_reference(c["x"], c["W"], c["b"], c["y"], c["kind"], c["sw"], c["sb"], False, torch.float32)


@pytest.mark.parametrize("kind", ["sgd", "adam"])
@pytest.mark.parametrize("M,K,C", HEAD_SHAPES)
def test_twin_head_step_meets_the_bounds(M, K, C, kind):
    for bias, only in head_variants(M):
        c = head_case(M, K, C, kind, bias, False, only)
        if M >= 2:
            assert c["y"][0] == IGN and c["y"][-1] == IGN and (c["y"][1:-1] != IGN).all()
        head_check(c, _twin_head(c), f"twin head {kind} {M}x{K}->{C} bias={bias} ignored_only={only}")


@pytest.mark.parametrize("kind", ["sgd", "adam"])
@pytest.mark.parametrize("M,K,C", HEAD_LARGE)
def test_twin_head_step_large_logits_meet_the_bounds(M, K, C, kind):
    c = head_case(M, K, C, kind, True, True)
    assert c["ref"]["logit_max"].max() > 1000
    twin = _twin_head(c)
    # the case's premise: fp32 computes these logits exactly
    assert torch.equal(torch_ops.linear_fwd(c["x"], c["W"], c["b"], False, 0.0, 0).double(),
                       c["x"].double() @ c["W"].double().t() + c["b"].double())
    head_check(c, twin, f"twin head large {kind} {M}x{K}->{C}")


def head_masked_inputs(M, K, C):
    """X with exact zeros, -0.0 and negatives for mask_by_input."""
    g = torch.Generator().manual_seed(5 * M + K)
    x = torch.randn(M, K, generator=g)
    x.view(-1)[::5] = 0.0
    x.view(-1)[2::35] = -0.0
    return x


# ---------------------------------------------------------------- 3. evaluation counters
EVAL_C = [1, 10, 63, 64, 65, 130]
EVAL_M = 77


@functools.lru_cache(maxsize=None)
def eval_case(C):
    """77 rows of logits on a grid of 13 values, so most rows hold their maximum several times
    (lowest index wins), in different lanes and in the same lane; half the rows labelled correctly."""
    g = torch.Generator().manual_seed(300 + C)
    x = torch.randint(-6, 7, (EVAL_M, C), generator=g).float() * 0.5
    y = torch.randint(0, min(C, 10), (EVAL_M,), generator=g)
    y[::2] = x[::2].argmax(dim=1)
    omit = min(C - 1, 9)
    return dict(x=x, y=y, omit=omit, counts=torch_ops.eval_counters(x, y, omit).tolist())


NAN, INF = float("nan"), float("inf")
# the hand-written rows at C = 130: ({column: planted value} over a base in [-1, 1] or a base value,
# label, the column argmax must give).  Rows 5, 6, 7, 9, 10 and 13 are the ones a kernel that skips
# NaNs or leaves "no column" on an all -inf row gets wrong; rows 8 and 11 it counts as wrong for
# another reason, which is the expected count too, and rows 0 to 4 hold the lowest-index rule.
EVAL_HAND = [
    ({5: 50.0, 69: 50.0}, 5, 5),             # the maximum twice in lane 5 (columns 5 and 5 + 64)
    ({5: 50.0, 69: 50.0}, 69, 5),
    ({64: 50.0, 3: 50.0}, 3, 3),             # twice, lanes 0 and 3: the merge takes the lower column
    ({64: 50.0, 3: 50.0}, 64, 3),
    ({129: 50.0}, 129, 129),                 # the last column
    ({40: NAN}, 40, 40),                     # a NaN is the maximum
    ({40: NAN, 7: 50.0}, 7, 40),
    ({100: NAN, 20: NAN}, 20, 20),           # two NaNs in different lanes: the first one
    ({100: NAN, 20: NAN}, 100, 20),
    ({84: NAN, 20: NAN}, 20, 20),            # two NaNs in lane 20
    (-INF, 0, 0),                            # all -inf: column 0
    (-INF, 1, 0),
    ({77: INF}, 77, 77),
    ({77: INF, 90: NAN}, 90, 90),            # a NaN beats +inf
    ({9: 50.0}, 20, 9),                      # a wrong row with the omitted label
]
EVAL_HAND_OMIT = 20
# correct: rows 0 2 4 5 7 9 10 12 13 = 9 of 15; label 20: rows 7 9 14, two of them correct
EVAL_HAND_COUNTS = [9, 15, 2, 3, 7, 12]


@functools.lru_cache(maxsize=None)
def eval_hand():
    g = torch.Generator().manual_seed(9)
    x = torch.rand(len(EVAL_HAND), 130, generator=g) * 2 - 1
    for r, (plant, _, _) in enumerate(EVAL_HAND):
        if isinstance(plant, dict):
            for col, v in plant.items():
                x[r, col] = v
        else:
            x[r] = plant
    return x, torch.tensor([lab for _, lab, _ in EVAL_HAND]), torch.tensor([p for _, _, p in EVAL_HAND])


def test_twin_eval_counters_on_the_hand_written_rows():
    """torch.argmax is the definition: the first NaN, else the first maximum, and column 0 of a row
    of nothing but -inf."""
    x, y, pred = eval_hand()
    assert torch.equal(x.argmax(dim=1), pred)
    assert torch_ops.eval_counters(x, y, EVAL_HAND_OMIT).tolist() == EVAL_HAND_COUNTS
    assert all(v > 0 for v in EVAL_HAND_COUNTS) and EVAL_HAND_COUNTS[2] < EVAL_HAND_COUNTS[3]


@pytest.mark.parametrize("C", EVAL_C)
def test_twin_eval_counters_cases_have_ties(C):
    c = eval_case(C)
    x = c["x"]
    ties = ((x == x.amax(dim=1, keepdim=True)).sum(dim=1) > 1).sum().item()
    assert ties > 20 or C == 1
    n_ok, n, _, n_unl, _, n_rem = c["counts"]
    assert n == EVAL_M and n_unl + n_rem == n and EVAL_M // 2 <= n_ok and (n_ok < n or C == 1)


# ---------------------------------------------------------------- 4. server_head3 at large logits
HEAD3 = dict(M=16, S2=4, N2=1000, C=100, seed=1234567)


@functools.lru_cache(maxsize=None)
def head3_case(G):
    """(M, S2, N2, C) = (16, 4, 1000, 100 G) with small-integer P2, b2, W3 and b3: h2 (ReLU, dropout
    0.5 and its factor 2) and the logits, up to about +-300, are exact in fp32 in any order of
    summation.  G = 1: one label per row, row 0 ignored.  G = 4: labels and scales per (row, group),
    two pairs ignored.  The float64 result composes the same ops, torch_ops.linear_epilogue giving
    the dropout mask both share."""
    M, S2, N2 = HEAD3["M"], HEAD3["S2"], HEAD3["N2"]
    C = 100 * G
    g = torch.Generator().manual_seed(40 + G)
    P2 = torch.randint(-2, 3, (S2, M, N2), generator=g).float()
    b2 = torch.randint(-1, 2, (N2,), generator=g).float()
    W3 = torch.randint(-1, 2, (C, N2), generator=g).float()
    b3 = torch.randint(-2, 3, (C,), generator=g).float()
    if G == 1:
        y = torch.randint(0, 100, (M,), generator=g)
        y[0] = IGN
        sc = None
    else:
        y = torch.randint(0, 100, (M, G), generator=g)
        y[M - 1, 0] = y[0, G - 1] = IGN
        sc = 1.0 / torch.randint(1, M + 1, (M, G), generator=g).float()
    h2 = torch_ops.linear_epilogue(P2.double().sum(0), b2.double(), True, 0.5, HEAD3["seed"])
    logits = (h2 @ W3.double().t() + b3.double()).view(M * G, 100)
    loss, d = ce64(logits, y.view(-1), 1.0 if G > 1 else 1.0 / M)
    if G > 1:
        d = d * sc.double().view(-1, 1)
    d = d.view(M, C)
    dz2 = (d @ W3.double()) * (h2 > 0) * 2.0
    return dict(P2=P2, b2=b2, W3=W3, b3=b3, y=y, sc=sc, G=G, h2=h2, loss=loss, dlog=d, dz2=dz2,
                logit_max=row_max(logits), logits=logits)


def head3_check(c, h2, dlog, dz2, loss, name):
    figs = dict(h2=worst(h2, c["h2"], 1e-4, 1e-4), loss=worst(loss.reshape(-1), c["loss"], 1e-4, loss_atol(c["logit_max"])),
                dlog=worst(dlog, c["dlog"], 1e-4, 1e-6), dz2=worst(dz2, c["dz2"], 1e-4, 1e-6))
    print(f"{name}: error / bound " + ", ".join(f"{k} {v:.3f}" for k, v in figs.items()))
    assert all(v <= 1 for v in figs.values()), figs
    ign = (c["y"].view(-1) == IGN).nonzero().view(-1)
    assert ign.numel() and not loss.cpu().reshape(-1)[ign].any() and not dlog.cpu().reshape(-1, 100)[ign].any()


@pytest.mark.parametrize("G", [1, 4])
def test_twin_server_head3_meets_the_bounds(G):
    c = head3_case(G)
    assert 200 < c["logit_max"].max() < 600
    M = HEAD3["M"]
    h2 = torch_ops.linear_epilogue(c["P2"].sum(0), c["b2"], True, 0.5, HEAD3["seed"])
    logits = h2 @ c["W3"].t() + c["b3"]
    assert torch.equal(logits.double().view(-1, 100), c["logits"])          # the premise: exact in fp32
    loss, d = torch_ops.softmax_ce(logits.view(-1, 100), c["y"].view(-1), 1.0 if G > 1 else 1.0 / M)
    if G > 1:
        d = d * c["sc"].view(-1, 1)
    d = d.view(M, -1)
    head3_check(c, h2, d, (d @ c["W3"]) * (h2 > 0) * 2.0, loss, f"twin server_head3 G={G}")


# ---------------------------------------------------------------- 5. relu_mask
RELU_N = [1, 255, 257, 16 * 100 + 3]
RELU_SPECIALS = [0.0, -0.0, 1e-40, -1e-40, -INF, INF, NAN]       # 1e-40: a denormal


@functools.lru_cache(maxsize=None)
def bits(t):
    """The fp32 tensor's bit patterns, so that 0.0 and -0.0 differ and equal NaNs compare equal."""
    return t.detach().cpu().contiguous().view(torch.int32)


def relu_where(d, h, scale):
    """relu_mask written as a select, as ReLU's backward is: d * scale where h > 0, else +0.0.  The
    twin's product form d * (h > 0) * scale has the same values but leaves -0.0 where it masks a
    negative d; bit for bit the kernels are held to this form."""
    return torch.where(h > 0, d * scale, torch.zeros_like(d))


@functools.lru_cache(maxsize=None)
def relu_case(n, lone=None):
    """(d, h, scale, the twin's result).  d is finite and non-zero; h is randn with the specials
    planted every 13 elements (n = 1: `lone`, one of them, is the whole of h)."""
    g = torch.Generator().manual_seed(60 + n)
    d = torch.randn(n, generator=g)
    d = torch.where(d == 0, torch.ones_like(d), d)
    h = torch.randn(n, generator=g)
    if lone is not None:
        h[0] = RELU_SPECIALS[lone]
    else:
        for j in range(0, n, 13):
            h[j] = RELU_SPECIALS[(j // 13) % len(RELU_SPECIALS)]
    return d, h, 2.0, torch_ops.relu_mask(d, h, 2.0)


def relu_cases():
    return [(n, None) for n in RELU_N if n > 1] + [(1, k) for k in range(len(RELU_SPECIALS))]


@pytest.mark.parametrize("n,lone", relu_cases())
def test_twin_relu_mask_is_where(n, lone):
    """The twin's product form lets only h > 0 through: a positive denormal and +inf pass, both
    zeros, -inf and NaN do not, and no NaN of h reaches the result."""
    d, h, scale, out = relu_case(n, lone)
    sel = relu_where(d, h, scale)
    assert torch.equal(out, sel) and torch.isfinite(out).all()
    # bit for bit the two differ only in the sign of the zeros the twin leaves for a masked negative d
    assert torch.equal(bits(out)[sel != 0], bits(sel)[sel != 0]) and not bits(sel)[sel == 0].any()
    if lone is not None:
        assert (out[0] != 0) == (RELU_SPECIALS[lone] in (1e-40, INF))
