"""U-shape split learning (default mode): Alice conv front -> Bob MLP middle ->
Alice head + loss.  Labels never leave the client.

Reference: `/root/reference/data_entities.py` (alice `:23-128`, bob `:131-180`),
schedule `split_nn.py:47-60`.  Per batch (data_entities.py:65-81) the reference
does an `inference` RPC forward and a dist-autograd backward that crosses the
process boundary twice, then a DistributedOptimizer Adam step over
model3 + Bob + model1.  Here: activation Alice->Bob, Bob's [B,100] output
Bob->Alice, head forward/CE/backward on Alice, dL/d(Bob output) Alice->Bob,
Bob dgrad -> cut gradient Bob->Alice (posted async, overlapping Bob's fused
wgrad+Adam), Alice's fused conv backward+Adam.  Bob keeps one Adam slot per
Alice (Q8).  The reference crashes after training because the U-shape bob has
no `eval_request_breakdown` (Q1); this module implements it and the U-shape
unlearn request so the reference schedule runs to completion.
"""
from __future__ import annotations

import torch

from ..config import CUT_FEATURES
from ..engine.slots import adam
from ..engine.tail import TailEngine
from ..models import ClientFront, Head, ServerTailUShape, head_spec, ushape_server_spec
from .base import AliceState
from .split import SplitSession


class UShapeSession(SplitSession):
    mode = "ushape"

    def front_module(self):
        return ClientFront()

    def alice_optim(self):
        return adam(self.args.lr)

    def bob_optim(self):
        return adam(self.args.lr)

    def bob_module_and_spec(self):
        return self.make_bob_module(ServerTailUShape), ushape_server_spec()

    def _extend_alice(self, a: AliceState):
        torch.manual_seed(self.seed + 2000 + a.cid)
        a.head = TailEngine(Head(), head_spec(), self.device)

    # ------------------------------------------------------------------ weights (model1 + model3)
    def give_weights(self, cid: int):
        a = self.alices[cid]
        return [{k: v.detach().clone() for k, v in a.front.module.state_dict().items()},
                {k: v.detach().clone() for k, v in a.head.module.state_dict().items()}]

    def _flat_client_weights(self, a):
        return torch.cat([a.front.flat_weights(), a.head.flat_weights()])

    def _load_flat_client_weights(self, a, flat):
        n = a.front.flat_numel
        a.front.load_flat_weights(flat[:n])
        a.head.load_flat_weights(flat[n:])

    def _client_flat_numel(self) -> int:
        return 32 * 9 + 32 + 100 * 10 + 10

    def _client_state(self, a):
        return {"model1": {k: v.detach().cpu() for k, v in a.front.module.state_dict().items()},
                "model3": {k: v.detach().cpu() for k, v in a.head.module.state_dict().items()}}

    def _load_client_state(self, a, sd):
        a.front.module.load_state_dict({k: v.to(self.device) for k, v in sd["model1"].items()})
        a.head.load_full_state_dict(sd["model3"])

    def reset_model(self, cid: int):
        a = self.alices[cid]
        a.front.reset_parameters(self.args.true_reset)
        with torch.no_grad():
            a.head.reset_parameters()

    # ------------------------------------------------------------------ one U-shape step
    def head_fused(self, M: int) -> bool:
        """Whether Alice's head runs as one `_C.head_step` launch for a batch of M.  Every
        rank evaluates this same rule (device kernels + the fixed 100 -> 10 head), so Bob
        knows that the dL/d(mid) he receives already carries his final ReLU's backward."""
        return hasattr(self.ops, "head_step_") and M * 100 <= 4096 and M * 10 <= 1024

    def head_train(self, a, mid, labels, t: int):
        """Alice's head on Bob's output: forward, CE, dL/d(mid) and the head's optimizer step
        (data_entities.py:74-81).  One launch when the head fits `_C.head_step`; that launch
        also applies the [mid > 0] mask of Bob's final ReLU (mid is that ReLU's output)."""
        if self.head_fused(mid.shape[0]):
            assert a.head.head_step_ok(mid.shape[0])
            _, dmid = a.head.head_step(mid, labels, a.slot, t, prefix="head.", mask_input=True)
            return dmid
        logits = a.head.forward(mid, train=True)
        _, dlog = self.ops.softmax_ce(logits, labels, 1.0 / mid.shape[0])
        dmid = a.head.backward_dgrad(dlog, need_dx=True)
        a.head.backward_step(a.slot, t, prefix="head.")
        return dmid

    def split_step(self, cid: int, idx, B: int):
        host = self.host(cid)
        a = self.alices.get(cid)
        act = am = labels = None
        if a is not None:
            act, am, labels = a.front.forward(a.train, idx, with_labels=True)
        act_b = self.act_to_bob(cid, act, B)
        out = self.tail.forward(act_b, train=True) if self.is_bob else None
        mid = self.from_bob(cid, out, (B, 100))
        dmid = None
        t = None
        if a is not None:
            t = a.slot.tick()
            dmid = self.head_train(a, mid, labels, t)
        dmid_b = self.to_bob(cid, dmid, (B, 100))
        dxp = self.tail.backward_dgrad(dmid_b, need_dx=True, premasked=self.head_fused(B)) if self.is_bob else None
        fin = self.comm.reduce_to_async(dxp, host, self.bob_ranks, (B, CUT_FEATURES), torch.float32)
        if self.is_bob:
            self.tail.backward_step(self.bob_slot(cid))
        dx = fin()
        if a is not None:
            a.front.backward_step(dx, act, am, a.train, idx, a.slot, t=t, prefix="front.")

    # ------------------------------------------------------------------ the mode's part of split_epoch
    def _send_act(self, cid, act, labels, rows):
        return self.act_to_bob(cid, act, rows), labels      # the labels stay with the Alice

    def _bob_middle(self, cid, a, act_b, labels, M, pre):
        """Bob's forward, the head + CE + head step on Alice, Bob's data gradients: the partial
        cut gradient and the Alice's step count `t`, which her conv update shares."""
        out = self.tail.forward(act_b, train=True, pre=pre) if self.is_bob else None
        mid = self.from_bob(cid, out, (M, 100))
        dmid = t = None
        if a is not None:
            t = a.slot.tick()
            dmid = self.head_train(a, mid, labels, t)
        dmid_b = self.to_bob(cid, dmid, (M, 100))
        dxp = (self.tail.backward_dgrad(dmid_b, need_dx=True, premasked=self.head_fused(M))
               if self.is_bob else None)
        return dxp, t

    def _bob_updater(self, cid, ahead):
        """Bob's wgrad + Adam, of both layers in one launch when grouped; in the look-ahead order
        that launch also forms the next batch's fc1 product when `grouped_ok` for its rows."""
        grouped = self.tail.grouped_ok()

        def update(x_next):
            if not grouped:
                self.tail.backward_step(self.bob_slot(cid))
                return False
            if x_next is not None and not self.tail.grouped_ok(x_next.shape[0]):
                x_next = None
            self.tail.group_step(self.bob_slot(cid), x_next=x_next)
            return x_next is not None
        return update

    # ------------------------------------------------------------------ eval hooks
    def bob_out_width(self) -> int:
        return 100

    def client_logits(self, cid: int, bob_out):
        return self.alices[cid].head.forward(bob_out, train=False)

    def inference(self, x):
        return self.tail.forward(x)
