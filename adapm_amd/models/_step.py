"""The training-step skeleton the app models share.

A model's step exists in three forms: the classic step (one pull, one
kernel, one push through the worker), the fused identity step (the
kernel works on the slab, world == 1) and the fused general step (the
same on the samples whose keys are all local; the rest miss). StepModel
owns what is the same in every model: the negative draw, the bounded
async pushes, the two halves of the classic step, the choice between
the three forms and the one-step deferral of misses. A model supplies
its keys and its kernels:

  _classic_step(arrays)        -> loss     pull / kernel / push
  _fused_identity_step(arrays) -> loss     `raw.*_step_fused`
  _fused_general_step(arrays)  -> (loss, missed sample indices)

`arrays` is the model's tuple of row-aligned per-sample numpy arrays,
e.g. (triples, negatives[B, N]); the skeleton only concatenates and
indexes them along axis 0.
"""
from __future__ import annotations

import os
import time
from collections import defaultdict

import numpy as np
import torch

_PHASE_TIMING = os.environ.get("ADAPM_PHASE_TIMING", "0") == "1"
MAX_PENDING = 64  # async pushes in flight before the oldest is waited for


class StepModel:
    def __init__(self, cfg, server, worker):
        self.cfg = cfg
        self.server = server
        self.worker = worker
        self.dev = server.rt.device
        self.rank = server.rt.rank
        self.world = server.rt.world
        self.rng = np.random.default_rng(cfg.seed + self.rank)
        self._pending = []
        self._deferred = None  # fused-general: missed samples retried next step
        self.phase_times = defaultdict(float)

    # ---------------------------------------------------- phase timing

    def _t0(self):
        return time.perf_counter() if _PHASE_TIMING else 0.0

    def _ph(self, name, t0):
        if _PHASE_TIMING:
            if self.dev.type == "cuda":
                torch.cuda.synchronize()
            t = time.perf_counter()
            self.phase_times[name] += t - t0
            return t
        return t0

    # ------------------------------------------------------------ init

    def _init_owned(self, num_keys, chunk, fill):
        """set() the keys this rank manages (key % world == rank), `chunk`
        rows at a time; fill(keys, vals) writes a zeroed chunk's values."""
        my_keys = np.arange(self.rank, num_keys, self.world, dtype=np.int64)
        for i in range(0, len(my_keys), chunk):
            ks = my_keys[i:i + chunk]
            vals = torch.zeros(len(ks), self.cfg.row, dtype=torch.float32, device=self.dev)
            fill(ks, vals)
            self.worker.set(ks, vals)
        self.worker.wait_sync()
        self.worker.barrier()

    # ------------------------------------------------- shared pieces

    def _negatives(self, n, num_keys):
        """n negative ids: from the sampling manager when the server has
        one (reference PrepareSample path), else uniform from the rng."""
        w = self.worker
        if self.server.sampling is not None:
            sid = w.prepare_sample(n, w.current_clock(), w.current_clock() + 2)
            neg = self.server.sampling.pull(w, sid, n)
            w.finish_sample(sid)
            return neg
        return self.rng.integers(0, num_keys, size=n, dtype=np.int64)

    def _track(self, ts):
        """Bounded async: remember a push ticket, cap the outstanding ones."""
        if ts != -1:
            self._pending.append(ts)
        while len(self._pending) > MAX_PENDING:
            self.worker.wait(self._pending.pop(0))

    def drain(self):
        if self._deferred is not None:
            # flush straggler samples through the classic path so an
            # epoch boundary never drops work
            arrays, self._deferred = self._deferred, None
            self._classic_step(arrays)
        for t in self._pending:
            self.worker.wait(t)
        self._pending.clear()

    def _loss_out(self, loss, sync_loss):
        """Per-sample losses -> what a step returns: the tensor itself (no
        host sync), or its mean as a float, 0.0 when no sample ran."""
        if not sync_loss:
            return loss
        return float(loss.mean().item()) if loss.numel() else 0.0

    # --------------------------------------------------- classic step

    def _begin_step(self, parts):
        """First half: one async pull of all rows, `parts` being the key
        arrays role by role (the first has one key per sample). Returns
        the handle for _finish_step."""
        keys = np.concatenate(parts)
        vals = torch.empty(len(keys) * self.cfg.row, dtype=torch.float32, device=self.dev)
        ts = self.worker.pull(keys, vals, async_=True)
        return [len(p) for p in parts], keys, vals, ts

    def _finish_step(self, handle, launch, sync_loss, t0=None, wait_push=False):
        """Second half: wait for the pull, run launch(values, deltas, loss)
        on the per-role [n, row] views of the pulled buffer and of a delta
        buffer of the same layout, push the deltas asynchronously. t0 is
        the phase clock of a step that timed its sampling."""
        sizes, keys, vals, ts = handle
        w = self.worker
        if t0 is None:
            t0 = self._t0()
        w.wait(ts)
        t0 = self._ph("pull", t0)

        row = self.cfg.row
        deltas = torch.empty_like(vals)
        v, d, a = [], [], 0
        for n in sizes:
            v.append(vals[a:a + n * row].view(n, row))
            d.append(deltas[a:a + n * row].view(n, row))
            a += n * row
        loss = torch.empty(sizes[0], dtype=torch.float32, device=self.dev)
        launch(v, d, loss)
        t0 = self._ph("kernel", t0)

        pt = w.push(keys, deltas, async_=True)
        if wait_push:
            w.wait(pt)
        self._track(pt)
        t0 = self._ph("push", t0)
        out = self._loss_out(loss, sync_loss)
        if sync_loss:
            self._ph("loss_sync", t0)
        return out

    # ----------------------------------------------------- fused step

    def _fused_identity(self, force_general):
        """The zero-host-work path: one rank, on the GPU, slab in key order."""
        return (self.dev.type == "cuda" and not force_general and self.world == 1
                and self.server.raw.layout_identity())

    def _fused_step(self, arrays, sync_loss, force_general):
        """Fused slab-direct step over `arrays`. Off the GPU the classic
        step runs instead, unless force_general (the gloo test tier runs
        the general path on the CPU store)."""
        if self.dev.type != "cuda" and not force_general:
            return self._loss_out(self._classic_step(arrays), sync_loss)
        if self._fused_identity(force_general):
            return self._loss_out(self._fused_identity_step(arrays), sync_loss)

        # A missed (any-key-remote) sample would block THIS step on a sync
        # round-trip through the classic path. Intent was signaled ahead,
        # so a miss is usually a straggler whose replica lands within a
        # round: DEFER it one step and retry fused. A second miss goes
        # classic immediately, so nothing starves.
        n_def = 0
        if self._deferred is not None:
            n_def = len(self._deferred[0])
            arrays = tuple(np.concatenate(p) for p in zip(self._deferred, arrays))
            self._deferred = None
        loss, missed = self._fused_general_step(arrays)
        if missed.numel():
            midx = missed.numpy()
            old = midx[midx < n_def]      # second miss: classic now
            fresh = midx[midx >= n_def]   # first miss: retry fused next step
            if len(fresh):
                self._deferred = tuple(a[fresh] for a in arrays)
            if len(old):
                mloss = self._classic_step(tuple(a[old] for a in arrays))
                loss = torch.cat([loss, mloss.to(loss.device)])
        return self._loss_out(loss, sync_loss)
