"""Micro-batched pretraining step: the exact large-batch contrastive step on a GPU that cannot hold the batch's activations.

A GPU that steps B = K * b records in K micro-batches computes exactly what K reference devices with b records each compute:
  per virtual device    its own random draws and its own span top-k (planner.build_plan selects over the device's whole pool, so this is
                        NOT one device holding B records);
  per virtual device    the loss of its own queries against the rank-major keys of all W * K devices (pretrain/pretrain_model.py:290);
  across all W * K      pmean of the gradients and of the metrics (:329, :336).
With b = 2, K = 64 and 8 GPUs this is the reference's 512-device run.  Gradient accumulation alone would not do: a micro-batch's loss would
only see its own negatives.  This is the gradient-cache scheme -- one extra forward per micro-batch:

  A  for every micro-batch m: forward, E_loc[m] <- the packed embeddings                       (activations are overwritten by the next m)
     all-gather of E_loc (with a communicator) -> E_all [W * K, R, H], ordered by real rank, then micro-batch
  B  for every m: the loss of virtual device rank * K + m over E_all and its gradient wrt every embedding; the query side is kept (dQ[m]),
     the key side summed over m in fp32 (dK_acc, ops.accumulate_rows); fp32 reduce-scatter of dK_acc (with a communicator);
     upstream gradient of micro-batch m = bf16(float(dQ[m]) + dK_own[m]), one rounding
  C  for every m: forward again (bit-equal to phase A's), backward from that gradient into the bf16 gradient buffer, grad32 += grad / K
     (ops.accumulate_rows).  The LAST micro-batch runs the bucketed backward: each finished bucket is accumulated on its producer stream
     and handed to optim.BucketSchedule -- fp32 nan_to_num, fp32 all-reduce, mr_adam_f32grad_update_dev -- so the reduction and the
     optimizer hide under the last backward as they do in Trainer.

Metrics: loss_info() is the mean over the micro-batches (and over ranks, as Trainer's).  The `_stuff_to_span_from_*` diagnostics are
formed from the per-source sums and counts added over all micro-batches, i.e. they are a ratio over all micro-batches, where the
reference takes the mean of per-device ratios.
`state` is a plain TrainState: checkpoints are interchangeable between values of K."""
import numpy as np
import torch

from . import ops
from .optim import BucketSchedule
from .planner import build_plan
from .synthetic import make_draws
from .trainer import Trainer

BF16, F32, I32 = torch.bfloat16, torch.float32, torch.int32


def check_micro_batches(records_per_gpu, micro_batches):
    """b = records per micro-batch; ValueError unless K >= 1 divides the records of a GPU."""
    B, K = int(records_per_gpu), int(micro_batches)
    if K < 1 or B % K != 0:
        raise ValueError(f'--micro-batches {K} does not divide the {B} records of a GPU')
    return B // K


def slice_batch(batch, m, b):
    """Records [m b, (m + 1) b) of every key of the batch (the '_draws' entry is left out: slice_draws)."""
    return {k: v[m * b:(m + 1) * b] for k, v in batch.items() if k != '_draws'}


def slice_draws(draws, d, m, b):
    """The draws of micro-batch m out of a batch's (splits, z): splits are record-major with d.rows_a2t / d.rows_t2a rows per record (as
    build_plan reads them), z has one row per record."""
    splits, z = draws
    return [s[m * b * rows:(m + 1) * b * rows] for s, rows in zip(splits, (d.rows_a2t, d.rows_t2a))], z[m * b:(m + 1) * b]


class _AccumulatingSchedule(BucketSchedule):
    """BucketSchedule of the last micro-batch: a finished bucket's bf16 gradients are first added into the fp32 accumulator, on the stream that
    produced them; what the comm stream then reduces and applies is the accumulator's range (state.f32_grads)."""

    def __init__(self, scale, *a):
        super().__init__(*a)
        self.scale = scale

    def finish(self, key, producer):
        lo, hi = self.ranges[key]
        store = self.state.store
        with torch.cuda.stream(producer):
            ops.accumulate_rows(store.grad[lo:hi], store.grad32[lo:hi], scale=self.scale)
        super().finish(key, producer)


class MicroBatchTrainer(Trainer):
    def __init__(self, config, B, device, micro_batches=1, rank=0, world=1, seed=0, comm=None, bf16_grads=True, shard_optimizer=False,
                 metrics_ring=0):
        if not bf16_grads or shard_optimizer:
            raise ValueError('MicroBatchTrainer: the fp32-gradient program (bf16_grads=False) and sharded moments (shard_optimizer=True) are out of scope')
        self.K = int(micro_batches)
        self.b = check_micro_batches(B, self.K)
        # ONE engine of b records; it is virtual device rank * K + m among world * K when micro-batch m's loss is issued
        super().__init__(config, B, device, rank=rank, world=world, seed=seed, comm=comm, metrics_ring=metrics_ring,
                         engine_shape=(self.b, 0, world * self.K))
        self.params.enable_f32_grads()
        self.state.f32_grads = True          # the bucket chain reads the fp32 accumulator; the engine keeps writing the bf16 params.grad

    def _make_step_buffers(self):
        eng, K, W, dev = self.engine, self.K, self.world, self.device
        R, H = eng.R, eng.d.H
        z = lambda *s: torch.zeros(*s, dtype=BF16, device=dev)
        f = lambda *s: torch.zeros(*s, dtype=F32, device=dev)
        self.E_loc, self.dQ = z(K, R, H), z(K, R, H)
        self.E_all = z(W * K, R, H) if self.use_comm else self.E_loc
        self.loss_sum, self.diag_sum = f(3), f(2, 6)
        self.t2sp = torch.zeros(K, eng.d.Ns, dtype=I32, device=dev)             # every micro-batch's t2sp_src (phase B reads plan m's)
        if W * K > 1:
            self.dE_tmp = z(W * K, R, H)
            self.dK_acc = f(W * K * R, H)
            self.dK_own = f(K * R, H) if self.use_comm else self.dK_acc

    # ---- host side: K plans per step ----
    def plan(self, batch, draws=None):
        """[the plan of micro-batch m] for m < K: records [m b, (m + 1) b) of every key, with the matching slices of the batch's draws
        (or of `draws`); absent draws come from Trainer.plan's seed rule applied to the micro-batch."""
        d, b = self.engine.d, self.b
        if draws is None:
            draws = batch.get('_draws')
        plans = []
        for m in range(self.K):
            mb = slice_batch(batch, m, b)
            if draws is None:
                seed = int(mb['audio2text/text_ptr'].astype(np.uint32).sum() % (2 ** 31))          # pretrain_model.py:96
                dr = make_draws(self.config, b, seed=seed)
            else:
                dr = slice_draws(draws, d, m, b)
            plans.append(build_plan(mb, d, dr[0], dr[1]))
        return plans

    def _inputs(self, batch, m):
        b = self.b
        return batch['images'][m * b:(m + 1) * b], batch['audio_clips'][m * b:(m + 1) * b]

    # ---- the three phases as launch sequences ----
    def _keep_embeddings(self, m):
        """Behind micro-batch m's phase-A forward: its embeddings and its plan's t2sp_src stay on the device for phase B."""
        eng = self.engine
        self.E_loc[m].copy_(eng.E)
        self.t2sp[m].copy_(eng._pl('t2sp_src'))

    def _phase_b(self):
        eng, K, W = self.engine, self.K, self.world
        R, H = eng.R, eng.d.H
        if self.use_comm:
            self.comm.gather_embeddings(self.E_loc.view(K * R, H), self.E_all)                     # pretrain_model.py:290
        self.loss_sum.zero_()
        self.diag_sum.zero_()
        if W * K == 1:                       # one device in all: Trainer's loss, both gradient sides land in eng.dE
            eng.loss_and_grad_outputs()
            ops.axpby_(self.loss_sum, eng.loss_acc)
            ops.axpby_(self.diag_sum.view(-1), eng.diag.view(-1))
            return
        self.dK_acc.zero_()
        for m in range(K):
            eng.rank = self.rank * K + m                              # (read when the LSE launches are issued: a launch argument)
            eng.E.copy_(self.E_loc[m])
            eng._plan_views['t2sp_src'] = self.t2sp[m]
            eng.loss_and_grad_outputs(self.E_all, self.dE_tmp)
            self.dQ[m].copy_(eng.dE)
            ops.accumulate_rows(self.dE_tmp.view(W * K * R, H), self.dK_acc)
            ops.axpby_(self.loss_sum, eng.loss_acc, 1.0 / K, 1.0)
            ops.axpby_(self.diag_sum.view(-1), eng.diag.view(-1))
        eng.rank = 0
        if self.use_comm:
            self.comm.scatter_grad(self.dK_acc.view(W, K * R * H), self.dK_own.view(-1))          # fp32: transpose of the all-gather
        ops.accumulate_rows(self.dQ.view(K * R, H), self.dK_own)       # upstream gradient of m = bf16(float(dQ[m]) + dK_own[m]), cast below

    def _upstream(self, m):
        """eng.dE <- the gradient of micro-batch m's embeddings (one rounding of the fp32 sum)."""
        eng = self.engine
        if self.world * self.K > 1:          # (one device in all: phase B left it there)
            R = eng.R
            ops.cast_f32_to_bf16(self.dK_own[m * R:(m + 1) * R], eng.dE)

    def _phase_c_inner(self, images, audio):
        """Recompute + plain backward of one of the first K - 1 micro-batches: no collectives, no gemm_cus plan."""
        eng, p = self.engine, self.params
        eng.forward_device(images, audio)
        p.grad.zero_()                       # a leaf this backward does not write must contribute 0
        eng._backward()
        ops.accumulate_rows(p.grad, p.grad32, scale=1.0 / self.K)

    def _phase_c_last(self, images, audio, update=True):
        eng, p = self.engine, self.params
        if self.K > 1:                       # (K = 1: phase A's activations are still in place)
            eng.forward_device(images, audio)
        p.grad.zero_()
        self._backward_reduce_update(update=update)

    def _bucket_schedule(self, update):
        return _AccumulatingSchedule(1.0 / self.K, self.state, self.buckets, self.comm if self.use_comm else None, self.comm_stream, update,
                                     getattr(self, 'bucket_timeline', None))

    def _push_metrics(self):
        if self.metrics_ring:                # before phase C: the scales are the ones this step's forwards read
            ops.metrics_push(self.loss_sum, self.diag_sum, self.params.wm['contrastive_scales'], self.state.hyper,
                             *self.step_metrics.tensors)

    # ---- steps ----
    def train_step(self, batch, plan=None, draws=None, update=True):
        """One eager step; returns loss_sum [3] (device).  update=False leaves the averaged gradients in params.grad32 and the parameters
        untouched."""
        eng, K = self.engine, self.K
        plans = self.plan(batch, draws) if plan is None else plan
        assert len(plans) == K
        self.state.prepare_step()
        if self.metrics_ring:
            self.step_metrics.begin_step(self.state.step)
        for m in range(K):
            eng.set_plan(plans[m])
            eng.forward_device(*self._inputs(batch, m))
            self._keep_embeddings(m)
        self._phase_b()
        self._push_metrics()
        self.params.grad32.zero_()
        for m in range(K):
            eng.set_plan(plans[m])
            self._upstream(m)
            if m < K - 1:
                self._phase_c_inner(*self._inputs(batch, m))
            else:
                self._phase_c_last(*self._inputs(batch, m), update=update)
        self.state.finish_step()
        return self.loss_sum

    def forward_and_loss(self, batch, plan=None, draws=None):
        raise NotImplementedError('MicroBatchTrainer steps through train_step / train_step_graph')

    backward_and_reduce = train_step_timeline = forward_and_loss

    def capture(self, batch):
        """Three hipGraphs over fixed input buffers of b records: the phase-A forward, the phase-C pass without collectives, and the phase-C
        pass with the bucket hand-over.  Phase B stays eager (its own-block offset is a launch argument).  Call after one eager train_step."""
        assert not self.use_comm or self.comm.capturable, 'only the library RCCL communicator (dist.NativeComm) can be captured'
        eng = self.engine
        images, audio = self._inputs(batch, 0)
        self.images_in, self.audio_in = torch.zeros_like(images), torch.zeros_like(audio)
        eng.plan_frozen = True
        torch.cuda.synchronize()
        graphs = []
        for prog in ((lambda: eng.forward_device(self.images_in, self.audio_in)),
                     (lambda: self._phase_c_inner(self.images_in, self.audio_in)) if self.K > 1 else None,
                     (lambda: self._phase_c_last(self.images_in, self.audio_in))):
            if prog is None:
                graphs.append(None)
                continue
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, capture_error_mode='thread_local'):
                prog()
            graphs.append(g)
        self.graph = graphs

    def _stage_inputs(self, batch, m):
        images, audio = self._inputs(batch, m)
        self.images_in.copy_(images, non_blocking=True)
        self.audio_in.copy_(audio, non_blocking=True)

    def train_step_graph(self, batch, plan):
        eng, K = self.engine, self.K
        gA, gC, gLast = self.graph
        assert len(plan) == K
        self.state.prepare_step()
        if self.metrics_ring:
            self.step_metrics.begin_step(self.state.step)
        for m in range(K):
            eng.set_plan(plan[m])
            self._stage_inputs(batch, m)
            gA.replay()
            self._keep_embeddings(m)
        self._phase_b()
        self._push_metrics()
        self.params.grad32.zero_()
        for m in range(K):
            eng.set_plan(plan[m])
            self._stage_inputs(batch, m)
            self._upstream(m)
            (gC if m < K - 1 else gLast).replay()
        self.state.finish_step()
        return self.loss_sum

    def _local_loss_info(self):
        return self.engine.info_from(self.loss_sum.tolist(), self.diag_sum.tolist())
