"""What the two round-robin split modes share (`VanillaSession`, `UShapeSession`): the
session state of the native executors, the train / unlearn requests of the Bob schedule
(`split_nn.py:47-60`) and `split_epoch` — the executor ladder and, below it, the one
pipelined Python loop.  The loop reaches its mode through three methods:

    _send_act(cid, act, labels, rows)            the cut activation to Bob, with or without labels
    _bob_middle(cid, a, act_b, lab, rows, pre)   everything between the activation's arrival and the
                                                 partial cut gradient -> (dxp, t)
    _bob_updater(cid, ahead)                     per epoch: update(x_next) -> pre, Bob's wgrad +
                                                 optimizer and the mode's own look-ahead rule

The fourth difference, the `t` / `prefix` arguments of the Alice's backward, is written out in
the loop: with it as a method returning keyword arguments (and vanilla's send as a wrapper
instead of an alias) the vanilla loop measured about 1 % under the parent (docs/PERF.md).

`split_step`, the reference's per-batch unit, stays written out in each mode: it is what
tests/test_split_order_cpu.py compares this loop against.
"""
from __future__ import annotations

import torch

from ..config import CUT_FEATURES
from ..engine.slots import OptSlot
from .base import Session, _progress
from .split_native import (native_remote_role, native_split_ok, persistent_ok, run_native_remote_epoch,
                           run_native_split_epoch, run_persistent_epoch)


class SplitSession(Session):
    def __init__(self, args, comm, device):
        super().__init__(args, comm, device)
        # protocols/split_native.py keeps its per-session state here; bench.py reports the first three
        self.native_split_epochs: dict = {}      # epochs run natively, by executor kind
        self.split_persist_reason = None         # why a persistent epoch was not chosen
        self.split_persist_fallback = None       # the error after which it was switched off
        self.last_split_losses = None            # per-sample losses of the last persistent epoch
        self.persist_off = False                 # co-located persistent executor declined or failed
        self.persist_remote_off = False          # Bob's remote persistent executor declined
        self.persist_max_steps = None            # tests: the epoch as several launches
        self.persist_fault_step = None           # tests: one injected launch failure

    def bob_slot(self, cid: int) -> OptSlot:
        s = self.bob_slots.get(cid)
        if s is None:
            s = self.bob_slots[cid] = OptSlot(self.bob_optim())
        return s

    # ------------------------------------------------------------------ one epoch
    def split_epoch(self, cid: int, order, n: int):
        """Split training of Alice_cid over `order` (n samples), pipelined so Bob never re-reads
        fc1 for a forward: per batch i, Bob's middle (`_bob_middle`: forward up to the data
        gradients, with the loss on his side or on the Alice's), the cut gradient to Alice,
        Alice's backward + step, Alice's forward of batch i+1 (sent to Bob), and only then Bob's
        wgrad + optimizer, whose kernel also forms batch i+1's fc1 product with the freshly
        updated weights (look-ahead).  Same math and update order as `split_step` per batch
        (both sides step on batch i before either runs batch i+1); on one GPU the reordering is
        free because the launches were serial anyway.  When no Bob shard shares the Alice's GPU
        (`split_lookahead`), Bob's update is issued right after the cut gradient leaves instead,
        so it runs during her backward and next forward (§3.2 overlap)."""
        B, mode = self.B, self.mode
        a = self.alices.get(cid)
        host = self.host(cid)
        spans = [(s, min(s + B, n)) for s in range(0, n, B)]
        if not spans:
            return
        if order is not None and persistent_ok(self, cid, mode) and run_persistent_epoch(self, cid, order, mode):
            return                                # the whole epoch in one launch, state on-chip
        if order is not None and native_split_ok(self, cid, mode):
            run_native_split_epoch(self, cid, order, mode)   # the same launches, issued from C++
            return
        role = native_remote_role(self, cid, mode)   # collective over the Alice's and Bob's ranks
        if role is not None:                      # remote Alice: each side's half from C++
            run_native_remote_epoch(self, cid, order, n, mode, role)
            return
        ahead = self.split_lookahead(cid)        # False: Alice remote from every Bob shard
        bob_update = self._bob_updater(cid, ahead) if self.is_bob else None

        def alice_fwd(span):
            s, e = span
            idx = order[s:e] if order is not None else None
            act = am = labels = None
            if a is not None:
                act, am, labels = a.front.forward(a.train, idx, with_labels=True)
            return (idx, act, am) + self._send_act(cid, act, labels, e - s)

        cur = alice_fwd(spans[0])
        pre = False
        for i, (s, e) in enumerate(spans):
            idx, act, am, act_b, lab = cur
            M = e - s
            dxp, t = self._bob_middle(cid, a, act_b, lab, M, pre)
            dx = self.comm.reduce_to(dxp, host, self.bob_ranks, (M, CUT_FEATURES), torch.float32)
            pre = False
            if self.is_bob and not ahead:
                bob_update(None)                  # overlaps the Alice's backward + next forward
            if a is not None and t is None:
                a.front.backward_step(dx, act, am, a.train, idx, a.slot, defer=True)
            elif a is not None:       # U-shape: the conv update shares the head's step count
                a.front.backward_step(dx, act, am, a.train, idx, a.slot, t=t, prefix="front.", defer=True)
            nxt = alice_fwd(spans[i + 1]) if i + 1 < len(spans) else None
            if self.is_bob and ahead:
                pre = bob_update(nxt[3] if nxt is not None else None)
            cur = nxt
        if a is not None:
            a.front.flush()          # the last step's deferred client update

    def _run_epochs(self, cid: int, order_fn, n: int):
        for _ in _progress(range(self.args.epochs), self.show, desc="Epochs", ascii=" >="):
            a = self.alices.get(cid)
            order = order_fn(a) if a is not None else None
            self.split_epoch(cid, order, n)

    def _order_len(self, cid, order):
        """Collective: how many samples the host's filter left, agreed by every rank."""
        n = torch.tensor([order.numel() if order is not None else 0], dtype=torch.int64, device=self.device)
        n = self.comm.multicast(n if self.hosts(cid) else None, self.host(cid), range(self.comm.world),
                                (1,), torch.int64)
        return int(n.item())

    # ------------------------------------------------------------------ Bob API
    def train_request(self, client_id: int):
        self.bob_log.info(f"Train Request for Alice-{client_id}")
        a = self.alices.get(client_id)
        if a is not None:
            a.logger.info("Training")
            if self.last_alice_id is None:
                a.logger.info(f"Alice-{client_id} is first client to train")
            else:
                a.logger.info(f"Alice-{client_id} receiving weights from Alice-{self.last_alice_id}")
        if self.last_alice_id is not None:
            self.relay_weights(self.last_alice_id, client_id)
        self._run_epochs(client_id, lambda al: al.train.shuffled_order(al.gen), self.n_train[client_id])
        self.last_alice_id = client_id

    def unlearn_request(self, client_id: int, omit_label: int):
        """Unlearning = retrain Alice_cid without the omitted label: reset + fresh optimizer
        states (the client's and Bob's slot for her, the reference's new DistributedOptimizer)
        + epochs over the filtered shard.  Absent from the reference's U-shape bob (Q1)."""
        self.bob_log.info(f"Unlearn Request for Alice-{client_id}")
        a = self.alices.get(client_id)
        order = None
        if a is not None:
            a.logger.info("Retraining")
            self.reset_model(client_id)
            a.slot = OptSlot(self.alice_optim())
            order = self.filtered_order(a, omit_label)
            a.unlearn_order = order
            a.logger.info("Retraining dataset: {}".format(self.label_counter(a, order)))
            a.logger.info("Test dataset (retraining): {}".format(a.test.label_counter()))
        self.bob_slots[client_id] = OptSlot(self.bob_optim())
        self._run_epochs(client_id, lambda al: al.unlearn_order, self._order_len(client_id, order))
