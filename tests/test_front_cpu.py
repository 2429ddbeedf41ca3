"""The client-front kernels' cases on the CPU: conv3x3(1->32) + bias + ReLU + max-pool 2x2 with its
2-bit argmax, its backward, the optimizer step, the deferred forward and the fused SISA local step
(csrc/conv.hip).

This file owns the images, the parameters, the float64 references, the bounds and the checks;
tests/test_front_gpu.py runs the same cases on the HIP kernels.  Here the fp32 torch twin
(ops/torch_ops.py) is held to the same checks, which shows that a correct fp32 implementation meets
them, and every premise of a case (exactness, populated tie classes, the near-tie cap) is asserted
on the reference alone.

Images (a shard of N = 40 rows, seeded torch.Generator on the CPU).
  stroke  MNIST-like: a zero border 4 wide, bars of saturated 255 at least 4 x 8 (whole constant 4x4
          patches) and a few grey ramps.
  edge    random pixels; rows and columns 0, 26 and 27 nonzero and distinct along the line.
  forms   u8; dyadic (x - 33) / 4 (negative, non-integer, granule 2^-2); real
          (x / 255 - 0.1307) / 0.3081 in fp32 (not exact).

Parameters.  w and b are multiples of 2^-10 with |w| <= 2^-4.  Channels 0..29 cycle through a
positive, a zero and a slightly negative bias; channel 30 (NEG) has only negative weights; channel
31 (DEAD) has the bias -2^8, so its y is 0 everywhere.

Exactness.  `fwd_exact` finds the granules 2^-kx, 2^-kw, 2^-kb of x, w, b and asserts
(9 max|x| max|w| + max|b|) 2^max(kx + kw, kb) < 2^24: every product and partial sum of the nine-tap
conv is then an fp32 number, so y and am must equal float64 bit for bit, true ties (lowest position
wins) included.  `bwd_exact` does the same for the backward: with dy on the granule 2^-kd, the
largest sum over all terms of |dy x| 2^(kd + kx) stays below 2^24, so dW and db are the same in
every summation order.

Bounds for what is not exact (U = 2^-23).
  sum     n fp32 terms (fma products included) in any order err by at most n U sum|terms|; the sum
          of |terms| is computed in float64 beside each reference.
  y       10 U (sum_k |w_k x_k| + |b|), the largest of the window's four positions (max and ReLU are
          1-Lipschitz); after an optimizer step plus sum_k |x_k| dw_k + db for parameters known to dw, db.
  am      compared wherever the reference y > 0 and the float64 gap from the winner to the best
          position *with a different 3x3 input window* exceeds twice the y bound.  Positions with the
          same window (constant patches, bars' straight edges) get identical values from any
          implementation that computes the four positions alike, so the lowest of them must win and
          they are compared, not left out.  What is left out is at most 1 % of the positive positions.
  loss    loss_atol(max y of the row) of test_loss_head_cpu.py, plus twice the row's y bound.
  g       the local step's softmax gradient g_i = (p_i - [i == label]) / B.  p_i = e_i / se with
          e_i = expf(y_i - mx): the subtraction (0 <= mx - y_i <= mx) costs mx U / 2 relative in e_i,
          expf U; se sums 5408 positive terms (5408 U) of such e_j; the reciprocal and the product U
          together; a y known to dy moves e_i / se by at most 2 dy.  So
          |dp_i| <= p_i ((5408 + 4 + mx) U + 2 dy) and |dg_i| <= |dp_i| / B + U |g_i|.
  dW, db  sum_i |dg_i| |x_i| (db: sum |dg_i|) + 169 B U sum_i |g_i x_i|.  Where the forward is not
          exact, a position whose gap (as under `am`) is within twice the y bound, or whose
          pre-ReLU value is within the y bound of 0, may take another window or gate: it adds
          |g_i| (|x_i| + the largest |x| of that tap over the four windows) (db: |g_i|).
  params  the float64 update (torch_ops.apply_update_ on float64 tensors) evaluated at the reference
          gradient +- its bound, the larger deviation, plus rtol 1e-5 and atol 1e-6 (test_opt_flat);
          the same form for both optimizer states, plus a term for the hyper-parameters: the
          kernels take beta (beta1, beta2, the momentum; all in [0.5, 1)) as an fp32 number, which
          is beta to 2^-25, and form 1.f - beta from it, which is then 1 - beta to the same 2^-25
          (the subtraction is exact): 1.f - float(0.999) is 1.3e-8 below 0.001, 1.3e-5 relative,
          more than rtol.  In s' = beta s + (1 - beta) q (q = g, or g^2 for v) both factors move by
          2^-25, so s' moves by at most 2^-25 (|s| + |q|).  (The tightest figure of the file, 0.96
          of the bound on the momentum of `local stroke real B=5`, is not this term: the twin and
          the kernel both resolve one near-tie unlike float64 there and use its allowance.)  Adam cases start from m around 0.01 and v in
          [0.001, 0.021], where the update is Lipschitz in the gradient.  The zero-state case is the
          DEAD channel at weight decay 0: its gradient is exactly 0, so SGD and Adam leave its
          parameters bitwise unchanged.
Consecutive steps of conv_local_step_ are compared step by step: each step's float64 reference
starts from the fp32 parameters and states the implementation under test holds at that point, so no
bound has to be carried across steps.
  epoch   conv_local_epoch_ shows no parameters between its steps, so its reference is the float64
          chain of local steps and the bounds are carried: a step that starts from w, b and states
          known to dw, db, ds has the y bound above with dw, db (so its loss, g and near-tie terms
          grow with them), and its update is evaluated at every corner of the intervals of g, p and
          the states (the update is smooth and the intervals are short), the largest deviation
          plus rtol, atol and the hyper-parameter term being what the next step starts from."""
import functools
import itertools

import pytest
import torch
import torch.nn.functional as F

from splitlearning_amd.config import OptimCfg
from splitlearning_amd.ops import torch_ops
from test_loss_head_cpu import U, loss_atol

N = 40
CUT = 5408
NEG, DEAD = 30, 31
KINDS = ("stroke", "edge")
EXACT_FORMS = ("u8", "dyadic")
NEAR_TIE_CAP = 0.01
OPT_RTOL, OPT_ATOL = 1e-5, 1e-6


# ---------------------------------------------------------------- images and parameters
@functools.lru_cache(maxsize=None)
def images(kind):
    """[N, 28, 28] int64 pixels 0..255."""
    g = torch.Generator().manual_seed({"stroke": 11, "edge": 12}[kind])
    ri = lambda lo, hi: int(torch.randint(lo, hi, (1,), generator=g))      # noqa: E731
    if kind == "edge":
        x = torch.randint(0, 256, (N, 28, 28), generator=g)
        n, c = torch.arange(N).view(N, 1), torch.arange(28).view(1, 28)
        for r in (0, 26, 27):
            x[:, r, :] = 1 + (37 * c + 11 * r + n) % 255
        for cc in (0, 26, 27):
            x[:, :, cc] = 1 + (53 * c + 29 * cc + 3 * n) % 255
        return x
    x = torch.zeros(N, 28, 28, dtype=torch.int64)
    for i in range(N):
        for _ in range(3):
            t, ln = ri(4, 7), ri(8, 17)
            h, w = (t, ln) if ri(0, 2) else (ln, t)
            r0, c0 = ri(4, 24 - h + 1), ri(4, 24 - w + 1)
            x[i, r0:r0 + h, c0:c0 + w] = 255
        for _ in range(2):
            r0, c0, k = ri(4, 24), ri(4, 16), ri(8, 32)
            x[i, r0, c0:c0 + 8] = (torch.arange(8) + 1) * k
    return x


@functools.lru_cache(maxsize=None)
def shard(kind, form):
    """[N, 784]: uint8, or fp32 in the dyadic or the real normalisation."""
    x = images(kind).reshape(N, 784)
    if form == "u8":
        return x.to(torch.uint8)
    if form == "dyadic":
        return (x.float() - 33) / 4
    assert form == "real"
    return (x.float() / 255 - 0.1307) / 0.3081


@functools.lru_cache(maxsize=None)
def params():
    g = torch.Generator().manual_seed(21)
    w = torch.randint(-64, 65, (32, 1, 3, 3), generator=g).float() / 1024
    b = torch.zeros(32)
    for c in range(30):
        if c % 3 == 0:
            b[c] = torch.randint(1, 129, (1,), generator=g).item() / 1024
        elif c % 3 == 2:
            b[c] = -torch.randint(1, 9, (1,), generator=g).item() / 1024
    w[NEG] = -torch.randint(1, 65, (1, 3, 3), generator=g).float() / 1024
    b[NEG] = 32 / 1024
    b[DEAD] = -256.0
    return w, b


def bias_class():
    """Per channel: 1 positive, 0 zero, -1 negative bias."""
    return torch.sign(params()[1]).long()


def granule(t):
    """The smallest k with t 2^k all integers (k <= 30), or None."""
    t = t.double()
    for k in range(31):
        s = t * 2.0 ** k
        if torch.equal(s, s.round()):
            return k
    return None


def fwd_exact(xs, w, b):
    """True if fp32 computes the nine-tap conv of these operands exactly in any order (see above)."""
    kx, kw, kb = granule(xs), granule(w), granule(b)
    if kx is None or kw is None or kb is None:
        return False
    k = max(kx + kw, kb)
    return bool((9 * xs.double().abs().max() * w.double().abs().max() + b.double().abs().max()) * 2.0 ** k < 2 ** 24)


# ---------------------------------------------------------------- float64 references
def _win(t):
    """[B, C, 26, 26] -> [B, C, 13, 13, 4], position dy * 2 + dx last."""
    B, C = t.shape[:2]
    return t.reshape(B, C, 13, 2, 13, 2).permute(0, 1, 2, 4, 3, 5).reshape(B, C, 13, 13, 4)


def fwd64(xs, w, b, dw=None, db=None):
    """The forward of rows xs [B, 784] in float64.  y, am (first maximum of the pre-pool values),
    pre [B, 32, 13, 13, 4], yerr (the y bound; 0 where fwd_exact holds and dw is None) and gap (from
    the winner to the best position with a different input window; inf if there is none)."""
    B = xs.shape[0]
    x = xs.double().view(B, 1, 28, 28)
    w64, b64 = w.double().view(32, 1, 3, 3), b.double().view(32)
    pre = _win(F.conv2d(x, w64, b64))
    best, am = pre[..., 0].clone(), torch.zeros(pre.shape[:-1], dtype=torch.int64)
    for p in (1, 2, 3):
        m = pre[..., p] > best
        best, am = torch.where(m, pre[..., p], best), torch.where(m, torch.full_like(am, p), am)
    if dw is None and fwd_exact(xs, w, b):
        yerr = torch.zeros_like(best)
    else:
        yerr = 10 * U * _win(F.conv2d(x.abs(), w64.abs(), b64.abs())).amax(-1)
        if dw is not None:
            yerr = yerr + _win(F.conv2d(x.abs(), dw.double().view(32, 1, 3, 3), db.double().view(32))).amax(-1)
    # windows of the four positions, [B, 13, 13, 4, 9], and which of them are equal
    xu = xs.float().view(B, 28, 28).unfold(1, 3, 1).unfold(2, 3, 1).reshape(B, 1, 26, 26, 9)
    wins = xu.reshape(B, 13, 2, 13, 2, 9).permute(0, 1, 3, 2, 4, 5).reshape(B, 13, 13, 4, 9)
    eq = (wins.unsqueeze(4) == wins.unsqueeze(3)).all(-1)                  # [B, 13, 13, 4, 4]
    same = eq.unsqueeze(1).expand(B, 32, 13, 13, 4, 4).gather(
        4, am.view(B, 32, 13, 13, 1, 1).expand(B, 32, 13, 13, 1, 4)).squeeze(4)
    # equal windows have equal values, but a float64 convolution may sum two of them in different
    # orders and differ in the last bit: the winner is the lowest position of its window's class
    am = same.int().argmax(-1)
    gap = best - pre.masked_fill(same, float("-inf")).amax(-1)
    return dict(y=best.clamp_min(0).reshape(B, CUT), am=am.to(torch.uint8).reshape(B, CUT), pre=pre, top=best,
                yerr=yerr, gap=gap, const=eq.all(-1).all(-1))


def _taps(xs):
    """[B, 3, 3, 26, 26]: the pixel under tap (kh, kw) of conv output (r, c), float64."""
    B = xs.shape[0]
    return xs.double().view(B, 28, 28).unfold(1, 26, 1).unfold(2, 26, 1)


def _scatter(v, am):
    """[B, 5408] per pooled position -> [B, 32, 26, 26] at the conv output that am names, else 0."""
    B = v.shape[0]
    a = am.long().view(B, 32, 13, 13)
    ph, pw = torch.arange(13).view(1, 1, 13, 1), torch.arange(13).view(1, 1, 1, 13)
    flat = ((2 * ph + a // 2) * 26 + 2 * pw + a % 2).reshape(B, 32, 169)
    return torch.zeros(B, 32, 676, dtype=torch.float64).scatter_(2, flat, v.double().reshape(B, 32, 169)).view(B, 32, 26, 26)


def bwd64(dy, y, am, xs, gerr=None, unc=None):
    """dW [32, 1, 3, 3], db [32] from (dy, y, am) with the gate y > 0, in float64, the sums of |terms|
    aW, adb, and their bounds eW, eb (see the docstring; gerr and unc [B, 5408] as there, or None)."""
    B = dy.shape[0]
    t = _taps(xs)
    dz = _scatter(dy.double() * (y > 0), am)
    es = lambda a, b_: torch.einsum("bors,bklrs->okl", a, b_).view(32, 1, 3, 3)      # noqa: E731
    dW, db = es(dz, t), dz.sum(dim=(0, 2, 3))
    aW, adb = es(dz.abs(), t.abs()), dz.abs().sum(dim=(0, 2, 3))
    eW, eb = 169 * B * U * aW, 169 * B * U * adb
    if gerr is not None:
        ge = _scatter(gerr * (y > 0), am)
        eW, eb = eW + es(ge, t.abs()), eb + ge.sum(dim=(0, 2, 3))
    if unc is not None and unc.any():
        # the largest |x| of each tap over the window's four positions, at every one of them
        tm = t.abs().reshape(B, 3, 3, 13, 2, 13, 2).amax(dim=(4, 6), keepdim=True).expand(B, 3, 3, 13, 2, 13, 2)
        gu = _scatter(dy.double().abs() * unc, am)
        eW, eb = eW + es(gu, t.abs() + tm.reshape(B, 3, 3, 26, 26)), eb + gu.sum(dim=(0, 2, 3))
    return dict(dW=dW, db=db, aW=aW, adb=adb, eW=eW, eb=eb)


def bwd_exact(dy, xs, aW):
    kd, kx = granule(dy), granule(xs)
    return kd is not None and kx is not None and bool(aW.max() * 2.0 ** (kd + kx) < 2 ** 24)


def opt_cfg(kind, wd=True):
    if kind == "adam":
        return OptimCfg("adam", 1e-3, weight_decay=1e-5 if wd else 0.0)
    return OptimCfg("sgd", 1e-2, momentum=0.9, weight_decay=1e-5 if wd else 0.0)


def opt_state(kind, p, seed, zero_dead=False):
    """A state away from zero: m or buf around 0.01, v in [0.001, 0.021]; zero_dead: the DEAD
    channel's entries are 0."""
    g = torch.Generator().manual_seed(seed)
    m = torch.randn(p.shape, generator=g) * 0.01
    st = {"m": m, "v": torch.rand(p.shape, generator=g) * 0.02 + 0.001} if kind == "adam" else {"buf": m}
    if zero_dead:
        for v in st.values():
            v[DEAD] = 0
    return st


def clone_state(st, dtype=None, device=None):
    return {k: v.detach().clone().to(dtype=dtype, device=device) for k, v in st.items()}


def step64(p, g, e, st, cfg, t, dp=None, dst=None):
    """The float64 update of p (fp32 or float64) with the gradient g known to e and, in a chain of
    steps, p known to dp and the state to dst: (p', state', bound of p', bounds of the state).  The
    update is evaluated at every corner of the operands' intervals and the largest deviation taken."""
    devs = {"g": e}
    if dp is not None:
        devs.update({"p": dp}, **dst)

    def run(sign):
        pp, ss = p.detach().double().clone(), clone_state(st, torch.float64)
        gg = g.double() + sign.get("g", 0) * e
        if "p" in sign:
            pp += sign["p"] * dp
            for k in ss:
                ss[k] += sign[k] * dst[k]
            if "v" in ss:
                ss["v"].clamp_(min=0)
        torch_ops.apply_update_(pp, gg, ss, cfg, t)
        return pp, ss
    p0, s0 = run({})
    wp, ws = torch.zeros_like(p0), {k: torch.zeros_like(v) for k, v in s0.items()}
    for signs in itertools.product((-1, 1), repeat=len(devs)):
        p1, s1 = run(dict(zip(devs, signs)))
        wp = torch.maximum(wp, (p1 - p0).abs())
        ws = {k: torch.maximum(ws[k], (s1[k] - s0[k]).abs()) for k in s0}
    tol = lambda r, d: d + OPT_RTOL * r.abs() + OPT_ATOL      # noqa: E731
    gg = g.double().abs() + e + cfg.weight_decay * p.detach().double().abs()
    hp = lambda k: 2.0 ** -25 * (st[k].double().abs() + (gg * gg if k == "v" else gg))      # noqa: E731
    return p0, s0, tol(p0, wp), {k: tol(s0[k], ws[k]) + hp(k) for k in s0}


def ratio(got, ref, bound):
    """max |got - ref| / bound in float64; 0 / 0 counts as 0, anything non-finite as inf."""
    got, ref = got.detach().double().cpu().reshape(-1), ref.detach().double().cpu().reshape(-1)
    bound = torch.as_tensor(bound, dtype=torch.float64).reshape(-1).expand_as(ref)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    if not (torch.isfinite(got).all() and torch.isfinite(ref).all()):
        return float("inf")
    d = (got - ref).abs()
    r = torch.where(d == 0, torch.zeros_like(d), d / bound)
    return r.max().item() if r.numel() else 0.0


def bit_equal(got, ref64):
    """got (fp32) is exactly the float64 reference, the sign of zeros aside."""
    return torch.equal(got.detach().cpu().double(), ref64)


# ---------------------------------------------------------------- cases
def batch_idx(B, seed=0):
    """Rows of the shard: the last row alone at B = 1; row 0 and the last at B = 2; else the last
    row, row 0, a repeated row and random rows."""
    if B == 1:
        return torch.tensor([N - 1])
    if B == 2:
        return torch.tensor([0, N - 1])
    g = torch.Generator().manual_seed(100 + B + seed)
    return torch.cat([torch.tensor([N - 1, 0, 5, 5]), torch.randint(0, N, (B - 4,), generator=g)])


@functools.lru_cache(maxsize=None)
def shard_labels():
    return torch.randint(0, CUT, (N,), generator=torch.Generator().manual_seed(3))


FWD_B = (1, 2, 17)


@functools.lru_cache(maxsize=None)
def fwd_case(kind, form, B):
    w, b = params()
    x, idx = shard(kind, form), batch_idx(B)
    ref = fwd64(x[idx], w, b)
    return dict(x=x, idx=idx, w=w, b=b, ref=ref, exact=form != "real", name=f"fwd {kind} {form} B={B}")


def check_forward(c, y, am, name=None):
    """y and am of a forward against case c (or any dict with ref / exact): bit for bit where exact,
    else within yerr and equal outside near-ties.  Returns (worst y error / bound, share left out)."""
    ref, name = c["ref"], name or c["name"]
    y, am = y.detach().cpu(), am.detach().cpu()
    pos = ref["y"] > 0
    if c["exact"]:
        assert not ref["yerr"].any()
        assert bit_equal(y, ref["y"]), f"{name}: y differs at {(y.double() != ref['y']).sum().item()} positions"
        bad = (am != ref["am"]) & pos
        assert not bad.any(), f"{name}: am differs at {bad.sum().item()} of {pos.sum().item()} positive positions"
        return 0.0, 0.0
    r = ratio(y, ref["y"], ref["yerr"].reshape(-1, CUT))
    clear = pos & (ref["gap"] > 2 * ref["yerr"]).reshape(-1, CUT)
    out = 1 - clear.sum().item() / max(pos.sum().item(), 1)
    bad = (am != ref["am"]) & clear
    print(f"{name}: y error / bound {r:.3f}, near-ties left out {out:.5f} of {pos.sum().item()}")
    assert r <= 1, f"{name}: y past its bound by {r}"
    assert out <= NEAR_TIE_CAP, f"{name}: {out} of the positive positions are near-ties"
    assert not bad.any(), f"{name}: am differs at {bad.sum().item()} clear positions"
    return r, out


BWD_B = (1, 5, 33)


@functools.lru_cache(maxsize=None)
def bwd_case(kind, form, B, hand=False):
    """dy: quarter-integers in [-1, 1] with exact zeros; (y, am) from the reference forward.  hand:
    am 1, 2, 3 in turn along the last pooled row and column (y = 1 there), DEAD left alone."""
    w, b = params()
    x, idx = shard(kind, form), batch_idx(B, seed=7)
    g = torch.Generator().manual_seed(500 + B)
    dy = torch.randint(-4, 5, (B, CUT), generator=g).float() / 4
    dy.view(-1)[::7] = 0.0
    f = fwd64(x[idx], w, b)
    y, am = f["y"].float(), f["am"].clone()
    if hand:
        y4, a4 = y.view(B, 32, 13, 13), am.view(B, 32, 13, 13)
        pat = (1 + torch.arange(13) % 3).to(torch.uint8)
        a4[:, :DEAD, 12, :], a4[:, :DEAD, :, 12] = pat, pat
        y4[:, :DEAD, 12, :], y4[:, :DEAD, :, 12] = 1.0, 1.0
    ref = bwd64(dy, y, am, x[idx])
    return dict(x=x, idx=idx, w=w, b=b, dy=dy, y=y, am=am, ref=ref, name=f"bwd {kind} {form} B={B} hand={hand}")


def bwd_cases():
    out = [(k, f, B, False) for k in KINDS for f in EXACT_FORMS for B in BWD_B]
    return out + [("edge", "u8", 5, True), ("edge", "dyadic", 5, True)]


def check_backward(c, dw, db):
    ref = c["ref"]
    assert bit_equal(dw, ref["dW"]), f"{c['name']}: dW differs, worst {(dw.cpu().double() - ref['dW']).abs().max().item()}"
    assert bit_equal(db, ref["db"]), f"{c['name']}: db differs"
    assert not dw.cpu()[DEAD].any() and not db.cpu()[DEAD].any()


STEP_B = (1, 33)
STEP_T = 3


@functools.lru_cache(maxsize=None)
def step_case(kind, B, opt):
    """Backward with update on the exact bwd case: SGD-momentum at weight decay 0 with the DEAD
    channel's momentum 0, Adam with weight decay."""
    c = bwd_case(kind, "u8" if B == 1 else "dyadic", B)
    cfg = opt_cfg(opt, wd=opt == "adam")
    sw, sb = opt_state(opt, c["w"], 31, zero_dead=True), opt_state(opt, c["b"], 32, zero_dead=True)
    zero = torch.zeros(())
    rw, rb = step64(c["w"], c["ref"]["dW"], zero, sw, cfg, STEP_T), step64(c["b"], c["ref"]["db"], zero, sb, cfg, STEP_T)
    return dict(c, cfg=cfg, sw=sw, sb=sb, rw=rw, rb=rb, opt=opt, name=f"step {opt} {c['name']}")


def check_params(name, w, b, sw, sb, rw, rb):
    """Parameters and states against step64's results rw, rb; prints and returns the worst ratio."""
    figs = {"w": ratio(w, rw[0], rw[2]), "b": ratio(b, rb[0], rb[2])}
    for k in rw[1]:
        figs[f"sw.{k}"], figs[f"sb.{k}"] = ratio(sw[k], rw[1][k], rw[3][k]), ratio(sb[k], rb[1][k], rb[3][k])
    print(f"{name}: error / bound " + ", ".join(f"{k} {v:.3f}" for k, v in figs.items()))
    bad = {k: v for k, v in figs.items() if not v <= 1}
    assert not bad, f"{name}: past the bound by the factor {bad}"
    return max(figs.values())


# ---------------------------------------------------------------- the SISA local step
LOCAL_B = (1, 5, 17)


@functools.lru_cache(maxsize=None)
def local_case(kind, form, B):
    """Labels of the batch's rows: 0..9 in turn, and at B >= 5 the last position 5407, a position
    whose reference activation is exactly 0 and the row's maximum."""
    w, b = params()
    x, idx = shard(kind, form), torch.arange(N - B, N)        # distinct rows, the last one included
    y = fwd64(x[idx], w, b)["y"]
    labels = shard_labels().clone()
    labels[idx] = torch.arange(B) % 10
    if B >= 5:
        labels[idx[1]] = CUT - 1
        zero_at = (y[2] == 0).nonzero().view(-1)
        labels[idx[2]] = zero_at[len(zero_at) // 2]
        labels[idx[3]] = y[3].argmax()
    return dict(x=x, idx=idx, labels=labels, w=w, b=b, name=f"local {kind} {form} B={B}")


def local_step64(xs, lab, w, b, sw, sb, cfg, t, dev=None):
    """One local step in float64 from fp32 operands: CE over the 5408-wide activation with scale
    1 / B, backward, update.  loss and its bound, then step64's results for w and b.  In a chain,
    dev = (dw, dsw, db, dsb) is what the step before leaves w, b and the states known to."""
    B = xs.shape[0]
    dw, dsw, db, dsb = dev or (None, None, None, None)
    f = fwd64(xs, w, b, dw, db)
    y, yerr = f["y"], f["yerr"].reshape(B, CUT)
    mx, dymax = y.amax(dim=1, keepdim=True), yerr.amax(dim=1, keepdim=True)
    p = torch.softmax(y, dim=1)
    loss = torch.logsumexp(y, dim=1) - y.gather(1, lab.view(-1, 1)).squeeze(1)
    g = p.clone()
    g.scatter_add_(1, lab.view(-1, 1), -torch.ones(B, 1, dtype=torch.float64))
    g = g / B
    gerr = p * ((CUT + 4 + mx) * U + 2 * dymax) / B + U * g.abs()
    unc = None
    if yerr.any():
        unc = ((f["gap"] <= 2 * f["yerr"]) | (f["top"].abs() <= f["yerr"])).reshape(B, CUT)
    r = bwd64(g, y, f["am"], xs, gerr, unc)
    return dict(loss=loss, loss_atol=loss_atol(mx.squeeze(1)) + 2 * dymax.squeeze(1), fwd=f, bwd=r,
                rw=step64(w, r["dW"], r["eW"], sw, cfg, t, dw, dsw), rb=step64(b, r["db"], r["eb"], sb, cfg, t, db, dsb))


def run_local_steps(c, step, opt, dev, steps=2, zero_state=False):
    """`steps` consecutive local steps of `step` (an ops module's conv_local_step_) on case c, each
    checked against the float64 step from the operands it started with.  Worst ratios returned."""
    cfg = opt_cfg(opt, wd=not zero_state)
    w, b = c["w"].clone().to(dev), c["b"].clone().to(dev)
    if zero_state:
        sw = {k: torch.zeros_like(v) for k, v in opt_state(opt, c["w"], 0).items()}
        sb = {k: torch.zeros_like(v) for k, v in opt_state(opt, c["b"], 0).items()}
    else:
        sw, sb = opt_state(opt, c["w"], 41), opt_state(opt, c["b"], 42)
    sw, sb = clone_state(sw, device=dev), clone_state(sb, device=dev)
    x, idx, labels = c["x"].to(dev), c["idx"].to(dev), c["labels"].to(dev)
    worst_loss = worst_p = 0.0
    for t in range(1, steps + 1):
        ref = local_step64(c["x"][c["idx"]], c["labels"][c["idx"]], w.cpu(), b.cpu(), clone_state(sw, device="cpu"),
                           clone_state(sb, device="cpu"), cfg, t)
        w0, b0 = w.clone(), b.clone()
        loss = step(x, labels, idx, w, b, cfg, sw, sb, t)
        name = f"{c['name']} {opt} t={t}" + (" zero state" if zero_state else "")
        rl = ratio(loss, ref["loss"], ref["loss_atol"])
        print(f"{name}: loss error / bound {rl:.3f}")
        assert rl <= 1, f"{name}: loss past its bound by {rl}"
        worst_loss = max(worst_loss, rl)
        worst_p = max(worst_p, check_params(name, w, b, sw, sb, ref["rw"], ref["rb"]))
        if zero_state:      # the DEAD channel: gradient exactly 0, zero state, no weight decay
            assert torch.equal(w[DEAD], w0[DEAD]) and torch.equal(b[DEAD], b0[DEAD])
            assert all(not v[DEAD].any() for v in sw.values()) and all(not v[DEAD].any() for v in sb.values())
    return worst_loss, worst_p


# ---------------------------------------------------------------- the deferred forward
PEND_PB, PEND_B = 7, 17


@functools.lru_cache(maxsize=None)
def pending_case(kind, form, opt):
    """A backward of 7 rows (exact gradient), then the forward of 17 other rows with that update
    applied: the float64 reference is update, then forward, its y bound carrying the parameters'."""
    w, b = params()
    x = shard(kind, form)
    pidx, idx = batch_idx(PEND_PB, seed=1), batch_idx(PEND_B, seed=2)
    g = torch.Generator().manual_seed(77)
    dy = torch.randint(-4, 5, (PEND_PB, CUT), generator=g).float() / 64
    f = fwd64(x[pidx], w, b)
    r = bwd64(dy, f["y"], f["am"], x[pidx])
    cfg = opt_cfg(opt)
    sw, sb = opt_state(opt, w, 51), opt_state(opt, b, 52)
    zero = torch.zeros(())
    rw, rb = step64(w, r["dW"], zero, sw, cfg, STEP_T), step64(b, r["db"], zero, sb, cfg, STEP_T)
    ref = fwd64(x[idx], rw[0], rb[0], rw[2], rb[2])
    return dict(x=x, pidx=pidx, idx=idx, dy=dy, py=f["y"].float(), pam=f["am"], w=w, b=b, cfg=cfg, sw=sw, sb=sb,
                rw=rw, rb=rb, ref=ref, exact=False, grad_exact=bwd_exact(dy, x[pidx], r["aW"]), labels=shard_labels(), name=f"pending {kind} {form} {opt}")


# ================================================================ the preconditions, on the CPU
def test_images_are_what_the_cases_need():
    s, e = images("stroke"), images("edge")
    assert not s[:, :4].any() and not s[:, 24:].any() and not s[:, :, :4].any() and not s[:, :, 24:].any()
    assert ((s > 0) & (s < 255)).sum() > 10 * N and (s == 255).sum() > 60 * N
    for line in (0, 26, 27):
        for t in (e[:, line, :], e[:, :, line]):
            assert (t > 0).all() and (t[:, 1:] != t[:, :-1]).all()       # no two neighbours alike
    for kind in KINDS:
        assert shard(kind, "u8").dtype == torch.uint8 and shard(kind, "dyadic").dtype == torch.float32
        d = shard(kind, "dyadic")
        assert (d < 0).any() and (d != d.round()).any() and granule(d) == 2
        assert granule(shard(kind, "real")) is None


def test_parameters_hold_every_bias_class():
    w, b = params()
    assert granule(w) <= 10 and granule(b) <= 10 and w.abs().max() <= 2.0 ** -4
    cls = bias_class()
    assert (cls[:30] == 1).sum() == 10 and (cls[:30] == 0).sum() == 10 and (cls[:30] == -1).sum() == 10
    assert (w[NEG] < 0).all() and b[NEG] > 0 and b[DEAD] == -256


@pytest.mark.parametrize("form", EXACT_FORMS)
@pytest.mark.parametrize("kind", KINDS)
def test_exact_cases_are_exact(kind, form):
    """The exactness condition of every exact case; nothing is rebuilt because none fails."""
    w, b = params()
    assert fwd_exact(shard(kind, form), w, b)
    assert not fwd_exact(shard(kind, "real"), w, b)
    for B in FWD_B:
        c = fwd_case(kind, form, B)
        assert not c["ref"]["yerr"].any() and not c["ref"]["y"].view(B, 32, 169)[:, DEAD].any()
    for k, f, B, hand in bwd_cases():
        if (k, f) == (kind, form):
            c = bwd_case(k, f, B, hand)
            assert bwd_exact(c["dy"], c["x"][c["idx"]], c["ref"]["aW"]), c["name"]
            assert (c["dy"] == 0).sum() > B * CUT // 8 and c["ref"]["dW"].abs().sum() > 0


@pytest.mark.parametrize("form", ("u8", "dyadic"))
def test_stroke_cases_hold_every_tie_class(form):
    """Constant 4x4 patches under a positive, a zero and a negative bias, and exact ties of
    non-constant patches (a bar's straight edge: two rows or columns of the window alike)."""
    c = fwd_case("stroke", form, 17)
    ref, cls = c["ref"], bias_class().view(1, 32, 1, 1)
    const = ref["const"].unsqueeze(1).expand(17, 32, 13, 13)
    pre = ref["pre"]
    tie = (pre == pre.amax(-1, keepdim=True)).sum(-1) > 1
    assert (tie | ~const).all()                                 # a constant patch always ties
    counts = {k: (const & (cls == v)).sum().item() for k, v in (("pos", 1), ("zero", 0), ("neg", -1))}
    counts["other"] = (tie & ~const & (ref["top"] > 0)).sum().item()
    counts["other, winner not 0"] = (tie & ~const & (ref["top"] > 0) & (ref["am"].view(17, 32, 13, 13) > 0)).sum().item()
    print(counts)
    assert all(v >= 10000 for k, v in counts.items() if k in ("pos", "zero", "neg")), counts
    assert counts["other"] >= 5000 and counts["other, winner not 0"] >= 2000, counts
    if form == "u8":        # a zero patch gives the bias at all four positions: y > 0 only under a positive bias
        z = const & (ref["pre"][..., 0] == params()[1].double().view(1, 32, 1, 1))
        assert z.sum() >= 3000 and ((ref["y"].view(17, 32, 13, 13) > 0) == (cls == 1))[z].all()
    assert not ref["am"].view(17, 32, 13, 13)[const].any()


def _twin_fwd(c):
    return torch_ops.conv_front_fwd(c["x"], c["idx"], c["w"], c["b"], labels=shard_labels())


@pytest.mark.parametrize("B", FWD_B)
@pytest.mark.parametrize("form", EXACT_FORMS)
@pytest.mark.parametrize("kind", KINDS)
def test_twin_forward_is_bit_equal(kind, form, B):
    """The twin's y is the reference bit for bit; its am differs only where y == 0, because the twin
    applies ReLU before the pool and so ties every non-positive window at position 0."""
    c = fwd_case(kind, form, B)
    y, am, lab = _twin_fwd(c)
    check_forward(c, y, am)
    assert torch.equal(lab, shard_labels()[c["idx"]])
    diff = am != c["ref"]["am"]
    assert not (diff & (c["ref"]["y"] > 0)).any()
    if B == 17:
        assert diff.any() and not am[c["ref"]["y"] == 0].any()


@pytest.mark.parametrize("B", FWD_B)
@pytest.mark.parametrize("kind", KINDS)
def test_twin_forward_real_normalisation(kind, B):
    """The twin within the y bound; the reference's own near-tie share under the cap."""
    c = fwd_case(kind, "real", B)
    assert c["ref"]["yerr"].min() > 0
    y, am, _ = _twin_fwd(c)
    check_forward(c, y, am)


@pytest.mark.parametrize("kind,form,B,hand", bwd_cases())
def test_twin_backward_is_bit_equal(kind, form, B, hand):
    c = bwd_case(kind, form, B, hand)
    if hand:
        a = c["am"].view(B, 32, 13, 13)
        assert set(a[:, 0, 12, :].unique().tolist()) == {1, 2, 3} == set(a[:, 0, :, 12].unique().tolist())
    dw, db = torch_ops.conv_front_bwd(c["dy"], c["y"], c["am"], c["x"], c["idx"], c["w"], c["b"])
    check_backward(c, dw, db)


@pytest.mark.parametrize("opt", ["sgd", "adam"])
@pytest.mark.parametrize("B", STEP_B)
@pytest.mark.parametrize("kind", KINDS)
def test_twin_backward_step_meets_the_bounds(kind, B, opt):
    c = step_case(kind, B, opt)
    w, b, sw, sb = c["w"].clone(), c["b"].clone(), clone_state(c["sw"]), clone_state(c["sb"])
    torch_ops.conv_front_bwd_step_(c["dy"], c["y"], c["am"], c["x"], c["idx"], w, b, c["cfg"], sw, sb, STEP_T)
    check_params(c["name"], w, b, sw, sb, c["rw"], c["rb"])
    assert not torch.equal(w[:DEAD], c["w"][:DEAD])
    if opt == "sgd":
        assert torch.equal(w[DEAD], c["w"][DEAD]) and torch.equal(b[DEAD], c["b"][DEAD])


@pytest.mark.parametrize("opt", ["sgd", "adam"])
@pytest.mark.parametrize("form", EXACT_FORMS)
@pytest.mark.parametrize("kind", KINDS)
def test_twin_update_then_forward_meets_the_bounds(kind, form, opt):
    c = pending_case(kind, form, opt)
    assert c["grad_exact"]          # the premise: the pending gradient is the same in every order
    w, b, sw, sb = c["w"].clone(), c["b"].clone(), clone_state(c["sw"]), clone_state(c["sb"])
    torch_ops.conv_front_bwd_step_(c["dy"], c["py"], c["pam"], c["x"], c["pidx"], w, b, c["cfg"], sw, sb, STEP_T)
    check_params(c["name"], w, b, sw, sb, c["rw"], c["rb"])
    y, am = torch_ops.conv_front_fwd(c["x"], c["idx"], w, b)
    check_forward(c, y, am)


@pytest.mark.parametrize("opt", ["sgd", "adam"])
@pytest.mark.parametrize("B", LOCAL_B)
@pytest.mark.parametrize("form", ("u8", "dyadic", "real"))
@pytest.mark.parametrize("kind", KINDS)
def test_twin_local_step_meets_the_bounds(kind, form, B, opt):
    c = local_case(kind, form, B)
    if B >= 5:
        lab, y = c["labels"][c["idx"]], fwd64(c["x"][c["idx"]], c["w"], c["b"])["y"]
        assert lab[1] == CUT - 1 and y[2, lab[2]] == 0 and y[3, lab[3]] == y[3].max() > 0
    run_local_steps(c, torch_ops.conv_local_step_, opt, "cpu")


@pytest.mark.parametrize("opt", ["sgd", "adam"])
def test_twin_local_step_from_zero_state_leaves_the_dead_channel(opt):
    run_local_steps(local_case("stroke", "u8", 5), torch_ops.conv_local_step_, opt, "cpu", steps=1, zero_state=True)



# ---------------------------------------------------------------- the local epoch
EPOCH_B, EPOCH_T0 = 16, 3
EPOCH_N = (3, 16, 33)           # n < B, n == B, and two full batches with a last batch of one


def epoch_cases():
    out = [("stroke", "u8", n, opt) for n in EPOCH_N for opt in ("sgd", "adam")]
    return out + [("edge", "u8", 33, "sgd"), ("edge", "u8", 33, "adam"), ("edge", "dyadic", 33, "adam"),
                  ("stroke", "real", 16, "adam")]


def local_epoch64(x, labels, order, B, w, b, sw, sb, cfg, t0):
    """ceil(n / B) local steps over `order` as a float64 chain with carried bounds: the losses [n]
    and their bounds, then step64's results of the last step."""
    w, b, sw, sb = w.double(), b.double(), clone_state(sw, torch.float64), clone_state(sb, torch.float64)
    dev, loss, atol = None, [], []
    for i, s in enumerate(range(0, order.numel(), B)):
        idx = order[s:s + B]
        r = local_step64(x[idx], labels[idx], w, b, sw, sb, cfg, t0 + i, dev)
        loss.append(r["loss"])
        atol.append(r["loss_atol"])
        (w, sw, dw, dsw), (b, sb, db, dsb) = r["rw"], r["rb"]
        dev = (dw, dsw, db, dsb)
    return dict(loss=torch.cat(loss), loss_atol=torch.cat(atol), rw=r["rw"], rb=r["rb"])


@functools.lru_cache(maxsize=None)
def epoch_case(kind, form, n, opt):
    """`order`: the shard's last row, row 0 and n - 2 other rows, none twice; labels anywhere in
    [0, 5408), the second row's on 5407."""
    w, b = params()
    x = shard(kind, form)
    g = torch.Generator().manual_seed(900 + n)
    order = torch.cat([torch.tensor([N - 1, 0]), 1 + torch.randperm(N - 2, generator=g)])[:n]
    labels = shard_labels().clone()
    labels[0] = CUT - 1
    # raw pixels up to 255 give gradients of several hundred: SGD's rate is set so that a step moves
    # a weight by about a tenth of its size (1e-2 would move it by many times its size, and a chain
    # of such steps tells nothing); Adam's step does not depend on the gradient's scale
    cfg = opt_cfg(opt) if opt == "adam" else OptimCfg("sgd", 1e-5, momentum=0.9, weight_decay=1e-5)
    sw, sb = opt_state(opt, w, 61), opt_state(opt, b, 62)
    ref = local_epoch64(x, labels, order, EPOCH_B, w, b, sw, sb, cfg, EPOCH_T0)
    return dict(x=x, labels=labels, order=order, w=w, b=b, sw=sw, sb=sb, cfg=cfg, ref=ref,
                name=f"epoch {kind} {form} n={n} {opt}")


def run_local_epoch(c, epoch, dev):
    """One conv_local_epoch_ of `epoch`'s ops module on case c against the float64 chain: the loss
    of every row, then the parameters and the states the epoch leaves."""
    w, b = c["w"].clone().to(dev), c["b"].clone().to(dev)
    sw, sb = clone_state(c["sw"], device=dev), clone_state(c["sb"], device=dev)
    loss = epoch(c["x"].to(dev), c["labels"].to(dev), c["order"].to(dev), EPOCH_B, w, b, c["cfg"], sw, sb, EPOCH_T0)
    ref = c["ref"]
    assert loss.shape == ref["loss"].shape
    per_step = [ratio(loss[s:s + EPOCH_B], ref["loss"][s:s + EPOCH_B], ref["loss_atol"][s:s + EPOCH_B])
                for s in range(0, loss.numel(), EPOCH_B)]
    print(f"{c['name']}: loss error / bound per step " + ", ".join(f"{v:.3f}" for v in per_step))
    assert max(per_step) <= 1, f"{c['name']}: loss past its bound by {per_step}"
    assert not torch.equal(w.cpu()[:DEAD], c["w"][:DEAD])
    return max(per_step), check_params(c["name"], w, b, sw, sb, ref["rw"], ref["rb"])


@pytest.mark.parametrize("kind,form,n,opt", epoch_cases())
def test_twin_local_epoch_meets_the_chain_bounds(kind, form, n, opt):
    c = epoch_case(kind, form, n, opt)
    assert sorted(c["order"].tolist())[0] == 0 and N - 1 in c["order"].tolist() and len(set(c["order"].tolist())) == n
    assert -(-n // EPOCH_B) == {3: 1, 16: 1, 33: 3}[n]
    # the carried bound stays under 0.3 of what the epoch moves the weights by (a missing or a
    # doubled step is off by the whole of it): the chain still tells a wrong step apart
    moved = (c["ref"]["rw"][0] - c["w"].double()).abs().max()
    assert c["ref"]["rw"][2].max() < 0.3 * moved, (c["ref"]["rw"][2].max(), moved)
    run_local_epoch(c, torch_ops.conv_local_epoch_, "cpu")
