"""Vanilla split learning (`--vanilla`): Alice conv front -> Bob MLP tail + loss
(labels go to Bob), round-robin clients with peer-to-peer weight relay, SGD with
momentum, and the "unlearn = retrain Alice_1 without the omitted label" loop.

Reference: `/root/reference/data_entities_vanilla.py` (alice `:24-207`, bob
`:210-301`), schedule `split_nn.py:47-60`.  Per batch the reference makes ~4 RPC
round trips (activation+labels, dist-autograd gradient, remote optimizer step,
context cleanup).  Here a batch is: one packed p2p message
Alice->Bob (activation + labels), Bob forward/CE/dgrad, the cut gradient
Bob->Alice posted asynchronously, Bob's fused wgrad+SGD kernels overlapping that
transfer, then Alice's fused conv backward+SGD.  Bob keeps one momentum slot per
Alice (the reference's per-Alice DistributedOptimizer, Q8), re-created on unlearn.
"""
from __future__ import annotations

import torch

from ..config import CUT_FEATURES
from ..engine.slots import sgd_momentum
from ..models import ServerTailSisa, sisa_server_spec
from .split import SplitSession


class VanillaSession(SplitSession):
    mode = "vanilla"

    def alice_optim(self):
        return sgd_momentum(self.args.lr)

    def bob_optim(self):
        return sgd_momentum(self.args.lr)

    def bob_module_and_spec(self):
        return self.make_bob_module(ServerTailSisa), sisa_server_spec()

    def before_eval(self):
        # Q7: the vanilla Bob never switches to eval mode -> dropout stays on during evaluation
        if self.args.eval_dropout_fix:
            self.switch_mode_to_eval()

    # ------------------------------------------------------------------ one split step
    def split_step(self, cid: int, idx, B: int):
        """One batch of split training for Alice_cid (collective over host + Bob ranks)."""
        host = self.host(cid)
        a = self.alices.get(cid)
        act = am = labels = None
        if a is not None:
            act, am, labels = a.front.forward(a.train, idx, with_labels=True)
        act_b, lab_b = self.send_act_labels(cid, act, labels, B)
        dxp = None
        fused = self.is_bob and self.tail.fused3_ok()
        if self.is_bob:
            if fused:
                _, dxp = self.tail.train_fwd_bwd3(act_b, lab_b, need_dx=True)
            else:
                out = self.tail.forward(act_b, train=True)
                _, dout = self.ops.softmax_ce(out, lab_b, 1.0 / B)
                dxp = self.tail.backward_dgrad(dout, need_dx=True)
        fin = self.comm.reduce_to_async(dxp, host, self.bob_ranks, (B, CUT_FEATURES), torch.float32)
        if self.is_bob:
            if fused:
                self.tail.fused_step(self.bob_slot(cid))
            else:
                self.tail.backward_step(self.bob_slot(cid))
        dx = fin()
        if a is not None:
            a.front.backward_step(dx, act, am, a.train, idx, a.slot)

    # ------------------------------------------------------------------ the mode's part of split_epoch
    _send_act = SplitSession.send_act_labels      # activation + labels, one packed message

    def _bob_middle(self, cid, a, act_b, lab_b, M, pre):
        """Bob's forward + CE + data gradients of one batch: the partial cut gradient, no `t`."""
        if not self.is_bob:
            return None, None
        if self.tail.fused3_ok():
            _, dxp = self.tail.train_fwd_bwd3(act_b, lab_b, need_dx=True, pre=pre)
        else:
            out = self.tail.forward(act_b, train=True)
            _, dout = self.ops.softmax_ce(out, lab_b, 1.0 / M)
            dxp = self.tail.backward_dgrad(dout, need_dx=True)
        return dxp, None

    def _bob_updater(self, cid, ahead):
        """Bob's wgrad + SGD.  In the look-ahead order the fused kernel also forms the next
        batch's fc1 product (TailEngine.fused_step) when that batch has at most 64 rows."""
        la = self.tail.fused3_ok() and self.tail.lookahead_ok(self.B) and ahead

        def update(x_next):
            if self.tail.fused3_ok():
                if not (la and x_next is not None and x_next.shape[0] <= 64):
                    x_next = None
                self.tail.fused_step(self.bob_slot(cid), x_next=x_next)
                return x_next is not None
            self.tail.backward_step(self.bob_slot(cid))
            return False
        return update

    def inference(self, x):
        return self.tail.forward(x)

    def train_and_backward(self, x, labels):
        """Bob-local forward + CE + backward + step on one batch (reference
        `bob.train_and_backward`, data_entities_vanilla.py:226-232); returns the loss."""
        out = self.tail.forward(x, train=True)
        loss, dout = self.ops.softmax_ce(out, labels, 1.0 / x.shape[0])
        self.tail.backward_dgrad(dout, need_dx=False)
        self.tail.backward_step(self.bob_slot(0))
        return loss.sum() / x.shape[0]
