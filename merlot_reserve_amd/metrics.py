"""Step-metrics ring: the log of a step that is one replayed graph, read without a synchronise per step.

Every step pushes its raw loss accumulators, temperatures and schedule scalar into a device ring of `depth` rows (one mr_metrics_push launch
inside the step, captured with it: ops.metrics_push(..., *ring.tensors)); drain() reads them back without stalling the stream -- the lagged
log of pretrain/train.py:119-129."""
import torch

from . import ops


class StepMetricsRing:
    def __init__(self, depth, device, derive, nkeys, comm=None):
        """derive(loss_acc [3], diag [2][6]) -> the loss_info() dict of a row (engine.info_from), of `nkeys` keys.  With a comm the derived
        values are averaged over its ranks."""
        L = ops.METRICS_ROW
        assert depth >= 2, 'metrics_ring: a depth of at least 2 (twice a drain interval of one step)'
        self.depth, self.device, self.derive, self.comm = depth, torch.device(device), derive, comm
        cuda = self.device.type == 'cuda'
        # ONE buffer [depth rows of L floats | depth int32 step numbers], so a drain is one D2H copy
        self.buf = torch.zeros(depth * (L + 1), dtype=torch.float32, device=self.device)
        self.ring = self.buf[:depth * L].view(depth, L)
        self.steps = self.buf[depth * L:].view(torch.int32)
        self.steps.copy_(torch.full((depth,), -1, dtype=torch.int32))           # no row holds a step yet
        self.counter = torch.zeros(1, dtype=torch.int32, device=self.device)
        self.host = [torch.zeros(depth * (L + 1), dtype=torch.float32, pin_memory=cuda) for _ in range(2)]
        self.turn = 0
        self.copy_stream = torch.cuda.Stream(device=self.device) if cuda else None
        self.first = None                 # step of the first push (set with the device counter, at the first step)
        self.pushed = self.drained = 0    # steps [drained, pushed) are in the ring and not yet copied
        self.raw = None                   # (lo, hi, event, pinned buffer): a ring copy in flight
        self.red = None                   # (rows, keys, event, pinned buffer): an average over ranks in flight
        self.red_dev = torch.zeros((depth // 2) * nkeys, dtype=torch.float32, device=self.device) if comm is not None else None
        self.red_host = torch.zeros((depth // 2) * nkeys, dtype=torch.float32, pin_memory=cuda) if comm is not None else None      # (read back before its next use)

    @property
    def tensors(self):
        """(ring, row_steps, counter): the last three arguments of ops.metrics_push."""
        return self.ring, self.steps, self.counter

    def begin_step(self, step):
        """The host's count of the pushes; `step` = the step about to be enqueued."""
        if self.first is None:            # once: the device counter starts at the step the run starts from (0, or a restored step)
            self.first = self.pushed = self.drained = step
            self.counter.copy_(torch.tensor([step], dtype=torch.int32))
        assert self.pushed == step, 'the metrics ring counts the steps of train_step / train_step_graph'
        self.pushed += 1

    @staticmethod
    def rows(host, depth, lo, hi, derive):
        """Rows of the steps [lo, hi) out of a host copy of the ring buffer ([depth, METRICS_ROW] floats, then depth int32 step numbers).
        The step number stored with a row must be the expected one: a lost or overwritten row raises, it is never returned as data."""
        L = ops.METRICS_ROW
        vals = host[:depth * L].view(depth, L).tolist()
        steps = host[depth * L:].view(torch.int32).tolist()
        rows = []
        for step in range(lo, hi):
            r = step % depth
            if steps[r] != step:
                raise RuntimeError(f'metrics ring: row {r} holds step {steps[r]}, expected {step} (overwritten or never written)')
            v = vals[r]
            row = {'step': step}
            row.update(derive(v[0:3], [v[3:9], v[9:15]]))
            row['contrastive_scales'], row['lr_scale'] = v[15:18], v[18]
            rows.append(row)
        return rows

    def _enqueue_copy(self):
        lo, hi = self.drained, self.pushed
        host = self.host[self.turn]
        self.turn ^= 1
        if self.device.type != 'cuda':
            host.copy_(self.buf)
            self.raw = (lo, hi, None, host)
        else:
            main = torch.cuda.current_stream()
            ready = torch.cuda.Event()
            ready.record(main)                                   # the pushes of [lo, hi) are on the main stream before this point
            with torch.cuda.stream(self.copy_stream):
                self.copy_stream.wait_event(ready)
                host.copy_(self.buf, non_blocking=True)
                done = torch.cuda.Event()
                done.record(self.copy_stream)
            main.wait_event(done)                                # device-side: no later step writes a row while this copy reads the ring
            self.raw = (lo, hi, done, host)
        self.drained = hi

    def _enqueue_mean(self, rows):
        """The derived rows averaged over the ranks: ONE allreduce_mean_f32 behind the steps already enqueued, and a copy back
        (pretrain_model.py:336, once per drain instead of once per step) -- a COLLECTIVE."""
        keys = sorted(k for k in rows[0] if k not in ('step', 'contrastive_scales', 'lr_scale'))
        n = len(rows) * len(keys)
        host = self.red_host
        host[:n].copy_(torch.tensor([[r[k] for k in keys] for r in rows], dtype=torch.float32).view(-1))
        dev = self.red_dev[:n]
        dev.copy_(host[:n], non_blocking=True)
        self.comm.allreduce_mean_f32(dev)
        host[:n].copy_(dev, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        self.red = (rows, keys, ev, host)

    def _collect(self):
        """Whatever has arrived on the host: the averaged rows in flight, then the raw copy in flight (derived; with a comm, sent on to be averaged)."""
        out = []
        if self.red is not None:
            rows, keys, ev, host = self.red
            ev.synchronize()
            vals = host[:len(rows) * len(keys)].view(len(rows), len(keys)).tolist()
            for r, v in zip(rows, vals):
                r.update(zip(keys, v))
            out += rows
            self.red = None
        if self.raw is not None:
            lo, hi, ev, host = self.raw
            if ev is not None:
                ev.synchronize()
            rows = self.rows(host, self.depth, lo, hi, self.derive)
            self.raw = None
            if self.comm is not None and rows:
                self._enqueue_mean(rows)
            else:
                out += rows
        return out

    def drain(self, flush=False):
        """Start an asynchronous copy of the ring (copy stream, behind the steps enqueued so far) and return the rows of the PREVIOUS drain as
        [{'step', **loss_info() keys, 'contrastive_scales', 'lr_scale'}]: the host waits for a copy enqueued one drain interval ago, never for
        the steps it has just enqueued.  With a comm the loss_info keys are means over the ranks (they arrive one drain later still) and equal
        loss_info(reduce=True) of that step -- a COLLECTIVE: every rank drains at the same steps.  At most depth // 2 steps between two drains.
        flush=True (end of a run): synchronises and returns everything that is left."""
        n = self.pushed - self.drained
        assert 2 * n <= self.depth, f'metrics ring of {self.depth} rows: at most {self.depth // 2} steps between drains, got {n}'
        out = self._collect()
        if n:
            self._enqueue_copy()
        while flush and (self.raw is not None or self.red is not None):
            out += self._collect()
        return out
