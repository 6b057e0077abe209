"""train_step (pretrain/pretrain_model.py:306-340) + construct_train_state (pretrain/optimization.py:158-195) on top
of the engine: one process per GPU; data parallelism = RCCL over xGMI (merlot_reserve_amd/dist.py).

Per step and rank:  plan (host) -> forward -> all-gather of the packed contrastive embeddings -> loss + dL/dE ->
reduce-scatter of dL/dE_all -> backward, during which every finished gradient BUCKET (five for the stock models) is
handed to a third stream: nan_to_num -> all-reduce(mean, bf16, like pmean at :329) -> fused bf16 Adam + decay + schedule +
apply on that range of the flat buffers, while the main / side streams continue with the rest of backward.  With the
library's RCCL communicator (dist.NativeComm) the collectives are ordinary stream-ordered launches, so the whole step,
collectives included, is ONE hipGraph.
"""
import numpy as np
import torch

from . import ops
from .engine import PretrainEngine, side_stream_disabled
from .metrics import StepMetricsRing
from .optim import AdamStepState, BucketSchedule, lr_scale_linearwarmup_cosinedecay, vision_cut_buckets
from .params import ParamStore
from .planner import build_plan
from .synthetic import make_draws


class TrainState(AdamStepState):
    """Counterpart of flax TrainState for this path: step counter, parameters (fp32 master + bf16 working copy),
    optimizer state (bf16 mu, cube-coded bf16 nu) -- all inside the ParamStore's flat buffers.  The optax chain of
    pretrain/optimization.py:180-190: no bias correction unless the config asks (optimization.py:177)."""
    eps = 1e-8
    bias_correction = False

    @property
    def params(self):
        return self.store

    def _schedule(self):
        oc = self.opt_config
        return lr_scale_linearwarmup_cosinedecay(self.step, oc['num_warmup_steps'], oc['num_train_steps'], oc.get('final_lr_scale', 0.02))

    def _host_update(self, sched, neg_lr, bc1, bc2):
        p = self.store
        ops.adam_bf16_update(p.master, p.work, p.grad, p.mu, p.nu, p.decay_flags, *self._adam_args(), sched, neg_lr, bc1, bc2)

    # ---- checkpoint form: flax `to_state_dict(TrainState)` of the reference's optax chain (optimization.py:180-195):
    # opt_state = (ScaleByAdamState{count, mu, nu}, add_decayed_weights (empty), ScaleByScheduleState{count}, scale (empty))
    # serialised as dicts keyed '0'..'3' (merlot_reserve_amd/checkpoint.py writes / reads the msgpack file)
    def state_dict(self):
        p = self.store
        mu, nu = self._moments()
        return {'step': self.step, 'params': p.master_tree(),
                'opt_state': {'0': {'count': torch.tensor(self.step, dtype=torch.int32), 'mu': p._to_tree(mu), 'nu': p._to_tree(nu)},
                              '1': {}, '2': {'count': torch.tensor(self.step, dtype=torch.int32)}, '3': {}}}

    def load_state_dict(self, sd, reset_schedule=False):
        """reset_schedule = True is the resolution-adaptation restart (pretrain/train_fixres.py:94-113): parameters and the
        Adam moments are kept, the step and the schedule's count start again from 0."""
        self.store.load_tree(sd['params'])
        self.step = int(sd.get('step', 0))
        opt = sd.get('opt_state')
        if opt:
            adam = opt['0']
            self._load_moments(adam['mu'], adam['nu'])
            self.step = int(adam.get('count', self.step))
        if reset_schedule:
            self.step = 0


def construct_train_state(opt_config, params):
    return TrainState(params, opt_config)


class Trainer:
    f32 = False          # (instances built by __init__ set it from bf16_grads)
    shards = property(lambda self: self.state.shards)      # (zero.MomentShards when built with shard_optimizer=True; the state owns them)

    metrics_ring = 0     # (depth of the step-metrics ring; 0 = none, the program of every caller that does not ask for it)
    step_metrics = None  # (metrics.StepMetricsRing of that depth)

    def __init__(self, config, B, device, rank=0, world=1, seed=0, comm=None, bf16_grads=True, shard_optimizer=False, metrics_ring=0,
                 engine_shape=None):
        """bf16_grads = False is the reference's use_bfloat16_grads = False step (pretrain/pretrain_model.py:323-333; train.py:61-67): the
        fp32 master parameters are differentiated, the gradients stay fp32 through nan_to_num / pmean and enter the Adam chain as
        fp32 -- the fp32 program of the engine (mr_f32_* kernels, eager, several times slower than the bf16 step: the correctness
        path, not the benchmarked one).  Data parallel through either communicator (fp32 all-gather / reduce-scatter of the contrastive
        embeddings, fp32 all-reduce of the gradient buckets).
        shard_optimizer = True: the Adam moments are partitioned over the ranks of `comm` (pretrain/train_fixres.py:178-199; zero.py).
        metrics_ring = depth > 0: every step pushes its raw loss accumulators, temperatures and schedule scalar into a device ring of `depth`
        rows (one mr_metrics_push launch inside the step, captured with it); drain_metrics() reads them back without stalling the stream --
        the lagged log of pretrain/train.py:119-129.  0 allocates nothing and leaves the launch sequence as it is.
        engine_shape = (records, rank, world) of the engine where they are not (B, rank, world): microbatch.MicroBatchTrainer."""
        self.config, self.B, self.rank, self.world = config, B, rank, world
        self.device = torch.device(device)
        self.f32 = not bf16_grads
        self.params = ParamStore(config, self.device, seed=seed, with_optimizer=not shard_optimizer)          # same seed on every rank: replicated init
        self.state = construct_train_state(config['optimizer'], self.params)
        self.state.f32_grads = self.f32
        eB, erank, eworld = engine_shape or (B, rank, world)
        self.engine = PretrainEngine(config, eB, self.params, self.device, rank=erank, world=eworld,
                                     dtype=torch.float32 if self.f32 else torch.bfloat16, train=True)
        self.comm = comm
        # the collective path runs whenever a comm is given -- also with a single rank, which is how the RCCL calls
        # themselves are exercised on a 1-GPU box (tests/test_dist_gpu.py)
        assert world == 1 or comm is not None
        self.use_comm = comm is not None
        self.comm_stream = torch.cuda.Stream(device=self.device) if self.device.type == 'cuda' else None
        self.graph = None
        self._make_buckets()
        if shard_optimizer:
            assert self.use_comm, 'shard_optimizer needs a communicator (its world may be 1)'
            from .zero import MomentShards
            self.state.shards = MomentShards(self.params, self.buckets, comm)
        if self.use_comm:
            assert comm.world == world and comm.rank == rank
            self.metrics = torch.zeros(8, dtype=torch.float32, device=self.device)
        self._make_step_buffers()
        self.metrics_ring = int(metrics_ring)
        if self.metrics_ring:
            self.step_metrics = StepMetricsRing(self.metrics_ring, self.device, self.engine.info_from, len(self.engine.objectives) + 4, comm)

    def _make_step_buffers(self):
        if self.use_comm:
            R, H = self.engine.R, self.engine.d.H
            z = lambda *s: torch.zeros(*s, dtype=self.engine.dtype, device=self.device)
            self.E_all, self.dE_all, self.dE_red = z(self.world, R, H), z(self.world, R, H), z(R, H)

    def _make_buckets(self):
        """optim.vision_cut_buckets behind 'joint' = [scales, head, span, joint, token] (final after backward_stage_joint) and
        'audio' = the audio tower (final when the side stream's audio backward ends)."""
        a0, a1 = self.params.tower_ranges['audio_encoder']
        self.buckets, self.vision_cuts = vision_cut_buckets(self.params, self.engine.d.Lv, [('joint', 0, a0), ('audio', a0, a1)])

    def plan(self, batch, draws=None):
        if draws is None:
            seed = int(batch['audio2text/text_ptr'].astype(np.uint32).sum() % (2 ** 31))   # pretrain_model.py:96
            draws = make_draws(self.config, self.B, seed=seed)
        return build_plan(batch, self.engine.d, draws[0], draws[1])

    # ---- the step as a launch sequence (eager, or captured once into a hipGraph and replayed) ----
    def _loss_and_exchange(self):
        eng = self.engine
        if self.use_comm:
            self.comm.gather_embeddings(eng.E, self.E_all)                  # pretrain_model.py:290
            eng.loss_and_grad_outputs(self.E_all, self.dE_all)
            self.comm.scatter_grad(self.dE_all, self.dE_red)                # transpose of the all-gather
            ops.add_(eng.dE.view(-1), self.dE_red.view(-1))
        else:
            eng.loss_and_grad_outputs()

    def _bucket_schedule(self, update):
        """The hand-over of this backward's finished buckets (microbatch.MicroBatchTrainer accumulates a bucket before it hands it over)."""
        return BucketSchedule(self.state, self.buckets, self.comm if self.use_comm else None, self.comm_stream, update,
                              getattr(self, 'bucket_timeline', None))

    def _backward_reduce_update(self, update=True):
        """Backward with every finished gradient bucket handed to the comm stream (optim.BucketSchedule).  `bucket_timeline` (eager
        steps only: train_step_timeline) receives HIP events around each bucket's collective: bench.py --gpus N."""
        eng = self.engine
        main = torch.cuda.current_stream()
        q = self._bucket_schedule(update)
        self.bucket_log = q.log
        eng.backward_stage_joint()
        q.finish('joint', main)
        # from here to the end of backward a bucket's all-reduce is in flight beside the GEMMs: leave its kernel two CUs per XCD
        with ops.gemm_cus(self.world if self.use_comm else 1):
            eng.side_stream.wait_stream(main)
            eng._on_side(eng.backward_stage_audio)
            audio_stream = main if side_stream_disabled() else eng.side_stream     # (issued in line)
            pending = ['audio']                     # enqueued behind the first vision bucket: audio rarely ends before it

            def layer_done(l):
                if l in self.vision_cuts:
                    q.finish(('vision', l), main)
                    if pending:
                        q.finish(pending.pop(), audio_stream)
            eng.backward_stage_vision(layer_done=layer_done)
            if pending:
                q.finish(pending.pop(), audio_stream)
            q.finish('vision_end', main)
        main.wait_stream(eng.side_stream)
        main.wait_stream(self.comm_stream)

    def _program(self, images, audio):
        self.engine.forward_device(images, audio)
        self._loss_and_exchange()
        if self.metrics_ring:            # before backward: the scales are the ones this step's forward read, not the updated ones
            ops.metrics_push(self.engine.loss_acc, self.engine.diag, self.params.wm['contrastive_scales'], self.state.hyper,
                             *self.step_metrics.tensors)
        self._backward_reduce_update(update=True)

    # ---- pieces, for tests and for the reference-API adapter (eager) ----
    def forward_and_loss(self, batch, plan=None, draws=None):
        eng = self.engine
        eng.forward(batch, plan=plan if plan is not None else self.plan(batch, draws))
        self._loss_and_exchange()
        return eng.loss_acc

    def backward_and_reduce(self, update=True):
        """Backward from the engine's current dE, bucket by bucket all-reduced; update=False leaves the averaged gradients in
        params.grad and the parameters untouched."""
        if update:
            self.state.prepare_step()
        self._backward_reduce_update(update=update)
        if update:
            self.state.finish_step()

    def train_step(self, batch, plan=None, draws=None):
        eng = self.engine
        if plan is None:
            plan = self.plan(batch, draws)
        self.state.prepare_step()
        eng.set_plan(plan)
        if self.metrics_ring:
            self.step_metrics.begin_step(self.state.step)
        self._program(batch['images'], batch['audio_clips'])
        self.state.finish_step()
        return eng.loss_acc

    def train_step_timeline(self, batch, plan=None):
        """One EAGER step with HIP events around every gradient bucket's collective (events cannot be read back from a replayed graph):
        returns {'backward_ms': start of backward -> its last kernel on the main stream, 'buckets': [{bucket, mbytes, ready_ms (its
        gradients final = the all-reduce may start), reduced_ms, updated_ms}]}, times from the start of backward -- what the first run
        on more than one GPU needs to see whether the all-reduces hide under backward (pretrain/pretrain_model.py:329 is the pmean
        they implement).  A diagnostic: the step it times is a real optimizer step."""
        eng = self.engine
        if plan is None:
            plan = self.plan(batch)
        self.state.prepare_step()
        eng.set_plan(plan)
        eng.forward_device(batch['images'], batch['audio_clips'])
        self._loss_and_exchange()
        self.bucket_timeline = []
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        try:
            self._backward_reduce_update(update=True)
            t1.record()
            tl = self.bucket_timeline
        finally:
            self.bucket_timeline = None
        self.state.finish_step()
        torch.cuda.synchronize()
        return {'backward_ms': t0.elapsed_time(t1),
                'buckets': [{'bucket': k, 'mbytes': round(mb, 1), 'ready_ms': round(t0.elapsed_time(a), 3), 'reduced_ms': round(t0.elapsed_time(b), 3),
                             'updated_ms': round(t0.elapsed_time(c), 3)} for k, mb, a, b, c in tl]}

    # ---- hipGraph path: the step is a fixed launch sequence over fixed buffers; capture it once, replay per step ----
    def capture(self, batch):
        """Capture the WHOLE step -- forward, collectives, loss, backward, bucket reductions, optimizer -- into one hipGraph.
        Call after at least one eager train_step (buffers, plan capacities and the communicator's lazy state exist).
        A torch.distributed comm cannot be captured (its collectives are host-scheduled): such a trainer steps eagerly."""
        assert not self.use_comm or self.comm.capturable, 'only the library RCCL communicator (dist.NativeComm) can be captured'
        assert not self.f32, 'the fp32-gradient step runs eagerly (train_step)'
        eng = self.engine
        self.images_in = torch.zeros_like(batch['images'])
        self.audio_in = torch.zeros_like(batch['audio_clips'])
        eng.plan_frozen = True
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, capture_error_mode='thread_local'):      # other threads (RCCL proxies, torch's watchdog) may call HIP meanwhile
            self._program(self.images_in, self.audio_in)
        self.graph = g

    def train_step_graph(self, batch, plan):
        eng = self.engine
        self.state.prepare_step()
        self.images_in.copy_(batch['images'], non_blocking=True)
        self.audio_in.copy_(batch['audio_clips'], non_blocking=True)
        eng.set_plan(plan)
        if self.metrics_ring:
            self.step_metrics.begin_step(self.state.step)
        self.graph.replay()
        self.state.finish_step()
        return eng.loss_acc

    def _local_loss_info(self):
        return self.engine.loss_info()

    def loss_info(self, reduce=True):
        """Host dict of the last step's losses.  With a comm and reduce=True it is the mean over ranks, like the reference's
        pmean of loss_info (pretrain_model.py:336) -- a COLLECTIVE: every rank must call it."""
        info = self._local_loss_info()
        if self.use_comm and reduce and self.world > 1:
            keys = sorted(info)
            self.metrics[:len(keys)].copy_(torch.tensor([info[k] for k in keys], dtype=torch.float32))
            self.comm.allreduce_mean_f32(self.metrics)
            info = dict(zip(keys, self.metrics[:len(keys)].tolist()))
        return info

    def drain_metrics(self, flush=False):
        """The rows of the step-metrics ring, one drain late (metrics.StepMetricsRing.drain) -- with a comm a COLLECTIVE."""
        assert self.metrics_ring, 'Trainer(metrics_ring=depth) was not asked for'
        return self.step_metrics.drain(flush=flush)
