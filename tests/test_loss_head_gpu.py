"""The loss and head kernels on an MI355X at their numeric and shape edges: softmax_ce (both kernels),
head_step_ (the MFMA and the FMA kernel), eval_counters, server_head3's softmax and relu_mask
against float64 references of the same operations, or bitwise against the twin where the operation
is exact.  The cases, the references and the bounds are those of tests/test_loss_head_cpu.py, which
also shows that the fp32 torch twin meets every bound used here.

What a wrong kernel would do: a softmax without its row maximum returns inf or NaN on the +-30000
rows (expf overflows at 88.7, and the all-negative rows divide 0 by 0), on the head's +-2000 logits
and on server_head3's +-300 ones; a stage of the head step that covers only the first 256 rows or
classes leaves raw logits in dX, dW and db (the 300 x 12 -> 3 and 3 x 4 -> 300 cases); a row stride
used as C writes outside a strided view."""
import pytest
import torch

from splitlearning_amd.ops import hip_ops
from test_loss_head_cpu import (CE_SHAPES, EVAL_C, EVAL_HAND_COUNTS, EVAL_HAND_OMIT, HEAD3, HEAD_LARGE, HEAD_MASKED,
                                HEAD_SHAPES, HEAD_T, ce_case, ce_check, clone_state, eval_case, eval_hand, head3_case,
                                head3_check, head_case, head_cfg, head_check, head_masked_inputs, head_variants,
                                bits, relu_case, relu_cases, relu_where)

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------- 1. softmax_ce against float64
@pytest.mark.parametrize("M,C", CE_SHAPES)
def test_softmax_ce_against_float64(cuda, M, C):
    c = ce_case(M, C)
    loss, d = hip_ops.softmax_ce(c["x"].to(cuda), c["y"].to(cuda), c["scale"])
    ce_check(c, loss, d, f"softmax_ce {M}x{C}")


@pytest.mark.parametrize("M,C", [s for s in CE_SHAPES if s[0] > 1])
def test_softmax_ce_strided_operands(cuda, M, C):
    """Logits and d_out as columns [3, 3 + C) of wider buffers: bitwise the contiguous run, and no
    element of d_out's buffer outside the view is written."""
    c = ce_case(M, C)
    x, y = c["x"].to(cuda), c["y"].to(cuda)
    R = x.shape[0]
    loss0, d0 = hip_ops.softmax_ce(x, y, c["scale"])
    sentinel = 12345.0
    xw = torch.full((R, C + 7), sentinel, device=cuda)
    xw[:, 3:3 + C] = x
    dw = torch.full((R, C + 9), sentinel, device=cuda)
    xv, dv = xw[:, 3:3 + C], dw[:, 3:3 + C]
    assert xv.stride(0) == C + 7 and dv.stride(0) == C + 9 and (C == 1 or not xv.is_contiguous())
    loss1, d1 = hip_ops.softmax_ce(xv, y, c["scale"], d_out=dv)
    assert d1 is dv
    assert torch.equal(loss1, loss0) and torch.equal(dv, d0)
    assert (dw[:, :3] == sentinel).all() and (dw[:, 3 + C:] == sentinel).all()
    assert torch.equal(xw[:, 3:3 + C], x) and (xw[:, :3] == sentinel).all() and (xw[:, 3 + C:] == sentinel).all()


# ---------------------------------------------------------------- 2. head_step_ against float64
def _run_head(c, dev, x=None, mask=False):
    """One head_step_ launch on device copies of case c; what the kernel left, keyed as the reference."""
    W = c["W"].to(dev)
    b = None if c["b"] is None else c["b"].to(dev)
    sw = clone_state(c["sw"], device=dev)
    sb = None if c["b"] is None else clone_state(c["sb"], device=dev)
    xin = (c["x"] if x is None else x).to(dev)
    loss, dx = hip_ops.head_step_(xin, W, b, c["y"].to(dev), 1.0 / xin.shape[0], head_cfg(c["kind"]), sw, sb, HEAD_T,
                                  mask_by_input=mask)
    return dict(loss=loss, dx=dx, W=W, b=b, sw=sw, sb=sb)


@pytest.mark.parametrize("kind", ["sgd", "adam"])
@pytest.mark.parametrize("M,K,C", HEAD_SHAPES)
def test_head_step_against_float64(cuda, M, K, C, kind):
    """Loss, dX, W, b and every state tensor, with a bias and without one; the first and the last
    row ignored (at M = 1 the lone row, in a run of its own)."""
    for bias, only in head_variants(M):
        c = head_case(M, K, C, kind, bias, False, only)
        head_check(c, _run_head(c, cuda), f"head {kind} {M}x{K}->{C} bias={bias} ignored_only={only}")


@pytest.mark.parametrize("kind", ["sgd", "adam"])
@pytest.mark.parametrize("M,K,C", HEAD_LARGE)
def test_head_step_large_logits(cuda, M, K, C, kind):
    c = head_case(M, K, C, kind, True, True)
    head_check(c, _run_head(c, cuda), f"head large {kind} {M}x{K}->{C}")


@pytest.mark.parametrize("kind", ["sgd", "adam"])
@pytest.mark.parametrize("M,K,C", HEAD_MASKED)
def test_head_step_mask_by_input(cuda, M, K, C, kind):
    """mask_by_input: dX is bitwise where(x > 0, the unmasked dX, 0), and nothing else changes."""
    c = head_case(M, K, C, kind)
    x = head_masked_inputs(M, K, C)
    assert (x == 0).any() and (x < 0).any() and (x > 0).any()
    plain, masked = _run_head(c, cuda, x), _run_head(c, cuda, x, mask=True)
    assert plain["dx"][1:-1].abs().sum() > 0
    assert torch.equal(masked["dx"], torch.where(x.to(cuda) > 0, plain["dx"], torch.zeros_like(plain["dx"])))
    assert torch.equal(masked["loss"], plain["loss"]) and torch.equal(masked["W"], plain["W"])
    assert torch.equal(masked["b"], plain["b"])
    for s in ("sw", "sb"):
        assert all(torch.equal(masked[s][k], plain[s][k]) for k in plain[s])


# ---------------------------------------------------------------- 3. eval_counters, exactly the twin
@pytest.mark.parametrize("C", EVAL_C)
def test_eval_counters_ties_and_accumulation(cuda, C):
    c = eval_case(C)
    x, y = c["x"].to(cuda), c["y"].to(cuda)
    counters = hip_ops.eval_counters(x, y, c["omit"])
    assert counters.cpu().tolist() == c["counts"]
    again = hip_ops.eval_counters(x, y, c["omit"], counters=counters)       # into non-zero counters
    assert again is counters and counters.cpu().tolist() == [2 * v for v in c["counts"]]


def test_eval_counters_hand_written_rows(cuda):
    """Duplicated maxima, the last column, NaN, all -inf and +inf rows, one row at a time so that a
    wrong row is named, then all of them in one launch."""
    x, y, pred = eval_hand()
    xg, yg = x.to(cuda), y.to(cuda)
    wrong = []
    for r in range(x.shape[0]):
        ok = int(pred[r] == y[r])
        unl = int(y[r] == EVAL_HAND_OMIT)
        want = [ok, 1, ok * unl, unl, ok * (1 - unl), 1 - unl]
        got = hip_ops.eval_counters(xg[r:r + 1], yg[r:r + 1], EVAL_HAND_OMIT).cpu().tolist()
        if got != want:
            wrong.append((r, got, want))
    assert not wrong, f"(row, counters, expected): {wrong}"
    assert hip_ops.eval_counters(xg, yg, EVAL_HAND_OMIT).cpu().tolist() == EVAL_HAND_COUNTS


# ---------------------------------------------------------------- 4. server_head3 at large logits
@pytest.mark.parametrize("G", [1, 4])
def test_server_head3_large_logits(cuda, G):
    c = head3_case(G)
    dev = lambda t: t.to(cuda)      # noqa: E731
    if G == 1:
        out = hip_ops.server_head3(dev(c["P2"]), dev(c["b2"]), True, 0.5, HEAD3["seed"], dev(c["W3"]), dev(c["b3"]),
                                   dev(c["y"]), 1.0 / HEAD3["M"])
    else:
        out = hip_ops.server_head3(dev(c["P2"]), dev(c["b2"]), True, 0.5, HEAD3["seed"], dev(c["W3"]), dev(c["b3"]),
                                   dev(c["y"]), 1.0, groups=G, gscale=dev(c["sc"]))
    h2, dlog, dz2, loss = out
    head3_check(c, h2, dlog, dz2, loss, f"server_head3 G={G}")


# ---------------------------------------------------------------- 5. relu_mask
@pytest.mark.parametrize("n,lone", relu_cases())
def test_relu_mask_special_values(cuda, n, lone):
    """h with 0.0, -0.0, denormals, -inf, +inf and NaN: bit for bit, the sign of every zero included,
    the select form of the twin (relu_where: +0.0 wherever h > 0 does not hold; the CPU file shows
    the twin's product form equal to it except for the -0.0 it leaves for a masked negative d)."""
    d, h, scale, ref = relu_case(n, lone)
    out = hip_ops.relu_mask(d.to(cuda), h.to(cuda), scale).cpu()
    sel = relu_where(d, h, scale)
    assert out.shape == ref.shape and out.dtype == ref.dtype
    assert torch.equal(bits(out), bits(sel))
    assert torch.isfinite(out).all() and torch.equal(out, ref)
