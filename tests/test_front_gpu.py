"""The client-front kernels (csrc/conv.hip) on an MI355X against float64: the forward with its argmax,
the backward, the backward with update, the deferred forward, the SISA local step and the local
epoch, on uint8 and float32 shards.  The cases, the references, the bounds and the checks are those of
tests/test_front_cpu.py, which also shows that the fp32 torch twin passes every one of them.

Where the arithmetic is exact (integer or dyadic pixels, dyadic parameters and gradients) the
comparison is bit for bit at every position, true ties of the pool window included.  What a wrong
kernel would do: `acc >= best` in the pool moves the argmax of every tied window off position 0; a
backward gate `y >= 0` lets the dead channel and the zero border collect gradient; a float staging
that truncates changes every dyadic pixel; an `img_idx` slip at row or column 27 changes the
gradient of the last pooled row and column under the hand-made argmax."""
import pytest
import torch

from splitlearning_amd.ops import hip_ops
from test_front_cpu import (BWD_B, CUT, DEAD, EXACT_FORMS, FWD_B, KINDS, LOCAL_B, PEND_B, PEND_PB, STEP_B, STEP_T,
                            bwd_case, bwd_cases, check_backward, check_forward, check_params, clone_state, fwd_case,
                            epoch_case, epoch_cases, local_case, opt_cfg, pending_case, run_local_epoch, run_local_steps,
                            shard_labels, step_case)

pytestmark = pytest.mark.gpu
SENTINEL = 12345.0


# ---------------------------------------------------------------- 1. forward
@pytest.mark.parametrize("B", FWD_B)
@pytest.mark.parametrize("form", EXACT_FORMS + ("real",))
@pytest.mark.parametrize("kind", KINDS)
def test_forward_against_float64(cuda, kind, form, B):
    """y and am at every position (bit for bit on the exact shards), the labels gathered in passing,
    and the two rows past B of preallocated outputs untouched."""
    c = fwd_case(kind, form, B)
    x, idx, w, b = c["x"].to(cuda), c["idx"].to(cuda), c["w"].to(cuda), c["b"].to(cuda)
    labels = shard_labels().to(cuda)
    y = torch.full((B + 2, CUT), SENTINEL, device=cuda)
    am = torch.full((B + 2, CUT), 77, device=cuda, dtype=torch.uint8)
    y1, am1, lab = hip_ops.conv_front_fwd(x, idx, w, b, y=y, am=am, labels=labels)
    assert y1 is y and am1 is am
    check_forward(c, y[:B], am[:B])
    assert torch.equal(lab, labels[idx])
    assert (y[B:] == SENTINEL).all() and (am[B:] == 77).all()
    y2, am2 = hip_ops.conv_front_fwd(x, idx, w, b)                  # outputs of its own, no labels
    assert torch.equal(y2, y[:B]) and torch.equal(am2, am[:B])


# ---------------------------------------------------------------- 2. backward, gradient only
@pytest.mark.parametrize("kind,form,B,hand", bwd_cases())
def test_backward_is_bit_equal_float64(cuda, kind, form, B, hand):
    assert B in BWD_B
    c = bwd_case(kind, form, B, hand)
    dev = lambda t: t.to(cuda)      # noqa: E731
    dw, db = hip_ops.conv_front_bwd(dev(c["dy"]), dev(c["y"]), dev(c["am"]), dev(c["x"]), dev(c["idx"]), dev(c["w"]),
                                    dev(c["b"]))
    check_backward(c, dw, db)


# ---------------------------------------------------------------- 3. backward with update
@pytest.mark.parametrize("opt", ["sgd", "adam"])
@pytest.mark.parametrize("B", STEP_B)
@pytest.mark.parametrize("kind", KINDS)
def test_backward_step_against_float64(cuda, kind, B, opt):
    c = step_case(kind, B, opt)
    dev = lambda t: t.to(cuda)      # noqa: E731
    w, b = dev(c["w"]).clone(), dev(c["b"]).clone()
    sw, sb = clone_state(c["sw"], device=cuda), clone_state(c["sb"], device=cuda)
    hip_ops.conv_front_bwd_step_(dev(c["dy"]), dev(c["y"]), dev(c["am"]), dev(c["x"]), dev(c["idx"]), w, b, c["cfg"],
                                 sw, sb, STEP_T)
    check_params(c["name"], w, b, sw, sb, c["rw"], c["rb"])
    assert not torch.equal(w.cpu()[:DEAD], c["w"][:DEAD])
    if opt == "sgd":        # weight decay 0, zero momentum, gradient exactly 0
        assert torch.equal(w.cpu()[DEAD], c["w"][DEAD]) and torch.equal(b.cpu()[DEAD], c["b"][DEAD])


# ---------------------------------------------------------------- 4. deferred forward
@pytest.mark.parametrize("opt", ["sgd", "adam"])
@pytest.mark.parametrize("form", EXACT_FORMS)
@pytest.mark.parametrize("kind", KINDS)
def test_deferred_forward_is_update_then_forward(cuda, kind, form, opt):
    """A deferred backward of 7 rows, then conv_front_fwd_pending of 17: y and am are those of the
    float64 update followed by the float64 forward; after conv_apply_ the stored parameters and states
    meet their bounds and the plain forward gives the same y and am."""
    c = pending_case(kind, form, opt)
    assert c["pidx"].numel() == PEND_PB and c["idx"].numel() == PEND_B
    dev = lambda t: t.to(cuda)      # noqa: E731
    x, w, b, labels = dev(c["x"]), dev(c["w"]).clone(), dev(c["b"]).clone(), dev(c["labels"])
    sw, sb = clone_state(c["sw"], device=cuda), clone_state(c["sb"], device=cuda)
    slab = torch.empty(PEND_PB * 320, device=cuda)
    hip_ops.conv_front_bwd_defer_(dev(c["dy"]), dev(c["py"]), dev(c["pam"]), x, dev(c["pidx"]), w, b, slab, None, sw, sb)
    assert torch.equal(w.cpu(), c["w"]) and torch.equal(b.cpu(), c["b"])          # nothing stored yet
    pend = (slab, PEND_PB, c["cfg"], sw, sb, STEP_T)
    idx = dev(c["idx"])
    y, am, lab = hip_ops.conv_front_fwd_pending(x, idx, w, b, labels, pend)
    check_forward(c, y, am, c["name"] + " pending")
    assert torch.equal(lab, labels[idx]) and torch.equal(w.cpu(), c["w"])
    hip_ops.conv_apply_(pend, w, b)
    check_params(c["name"], w, b, sw, sb, c["rw"], c["rb"])
    y2, am2 = hip_ops.conv_front_fwd(x, idx, w, b)
    check_forward(c, y2, am2, c["name"] + " applied")
    assert torch.equal(y2, y) and torch.equal(am2, am)


# ---------------------------------------------------------------- 5. SISA local step
@pytest.mark.parametrize("opt", ["sgd", "adam"])
@pytest.mark.parametrize("B", LOCAL_B)
@pytest.mark.parametrize("form", EXACT_FORMS + ("real",))
@pytest.mark.parametrize("kind", KINDS)
def test_local_step_against_float64(cuda, kind, form, B, opt):
    """Two consecutive steps: loss_rows, parameters and states of each against the float64 step from
    the operands the kernel started it with."""
    run_local_steps(local_case(kind, form, B), hip_ops.conv_local_step_, opt, cuda)


@pytest.mark.parametrize("opt", ["sgd", "adam"])
def test_local_step_from_zero_state_leaves_the_dead_channel(cuda, opt):
    run_local_steps(local_case("stroke", "u8", 5), hip_ops.conv_local_step_, opt, cuda, steps=1, zero_state=True)


# ---------------------------------------------------------------- 6. local epoch
@pytest.mark.parametrize("kind,form,n,opt", epoch_cases())
def test_local_epoch_against_the_float64_chain(cuda, kind, form, n, opt):
    """conv_local_epoch_ at B = 16 with n = 3 (n < B), 16 and 33 (a last batch of one): every row's
    loss, then the parameters and the states, against the float64 chain of local steps with its
    carried bounds; the bitwise comparison with the steps stays in test_kernels_gpu.py."""
    run_local_epoch(epoch_case(kind, form, n, opt), hip_ops.conv_local_epoch_, cuda)


# ---------------------------------------------------------------- 7. what the kernels do not promise
def test_local_step_label_out_of_range_leaves_loss_unwritten(cuda):
    """docs/ARCHITECTURE.md: front labels lie in [0, 5408).  A row whose label is outside matches no
    position, so its entry of a caller's loss_rows keeps what it held; the other rows are written."""
    c = local_case("edge", "u8", 5)
    labels = c["labels"].clone()
    labels[c["idx"][1]], labels[c["idx"][3]] = CUT, -1
    w, b = c["w"].to(cuda).clone(), c["b"].to(cuda).clone()
    sw, sb = {"buf": torch.zeros_like(w)}, {"buf": torch.zeros_like(b)}
    loss = torch.full((5,), SENTINEL, device=cuda)
    out = hip_ops.conv_local_step_(c["x"].to(cuda), labels.to(cuda), c["idx"].to(cuda), w, b, opt_cfg("sgd"), sw, sb, 1,
                                   loss_rows=loss)
    assert out is loss
    got = loss.cpu()
    assert got[1] == SENTINEL and got[3] == SENTINEL
    assert (got[[0, 2, 4]] != SENTINEL).all() and torch.isfinite(got).all() and torch.isfinite(w).all()
