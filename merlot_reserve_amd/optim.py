"""What the host programs that issue an optimizer step share (trainer.py: pretraining; finetune.py: VCR and TVQA): the two
schedules, the optimizer step state over a ParamStore's flat buffers, the gradient-bucket table and the routine that takes a
finished bucket through nan_to_num -> all-reduce -> Adam on the comm stream.  The stage walk of backward stays with each program.
"""
import os

import numpy as np
import torch

from . import ops


def lr_scale_linearwarmup_cosinedecay(step, num_warmup_steps, num_train_steps, final_lr_scale=0.1):
    """pretrain/optimization.py:117-137, evaluated in float32 like jnp on an int32 step."""
    f = np.float32
    step = f(step)
    if step < num_warmup_steps:
        return float(step / f(num_warmup_steps))
    post = (step - f(num_warmup_steps)) / f(num_train_steps - num_warmup_steps + 1.0)
    post = min(post, f(1.0))
    post = f(1.0) - (f(1.0) - np.cos(f(np.pi) * post, dtype=np.float32)) / f(2.0)
    return float(f(final_lr_scale) + f(1.0 - final_lr_scale) * post)


def lr_scale_linearwarmup_lineardecay(step, num_warmup_steps, num_train_steps):
    """pretrain/optimization.py:140-155 in float32"""
    f = np.float32
    step = f(step)
    if step < num_warmup_steps:
        return float(step / f(num_warmup_steps))
    post = (step - f(num_warmup_steps)) / f(num_train_steps - num_warmup_steps + 1.0)
    return float(f(1.0) - min(post, f(1.0)))


class AdamStepState:
    """Step counter + the bf16-state Adam chain over a ParamStore's flat buffers (fp32 master, bf16 working copy, bf16 mu, cube-coded
    bf16 nu, `orig` where the store keeps one), either in ONE host-scalar launch (apply_gradients) or in pieces with the step's scalars
    in a device vector (prepare_step, then apply_range per finished gradient range), so that the launches can sit inside a hipGraph and
    overlap the rest of backward.  A subclass sets `eps` / `bias_correction` (the defaults its reference chain has), `_schedule()`,
    `_host_update()` (its host-scalar kernel) and its checkpoint form."""
    eps = None
    bias_correction = None

    def __init__(self, store, opt_config):
        self.store, self.opt_config, self.step = store, dict(opt_config), 0
        self.f32_grads = False          # use_bfloat16_grads = False: the chain reads store.grad32 (set by Trainer(bf16_grads=False))
        self.shards = None              # zero.MomentShards: mu / nu partitioned over the ranks (shard_optimizer=True)
        self.hyper = None               # device vector of the step's scalars (prepare_step)

    def _adam_args(self):
        oc = self.opt_config
        return oc.get('beta_1', 0.9), oc.get('beta_2', 0.98), oc.get('eps', self.eps), oc['weight_decay_rate']

    def _scalars(self):
        """(sched, neg_lr, bias_corr1, bias_corr2) of the current step: scale_by_schedule uses its own count, evaluated
        BEFORE the increment (first update is zero); bias correction as the config asks, else as the subclass's reference chain has it."""
        oc = self.opt_config
        assert oc.get('use_bfloat16_adam', True), 'only the bf16-state Adam of the reference configs is implemented'
        b1, b2 = self._adam_args()[:2]
        bc1 = bc2 = 1.0
        if oc.get('do_bias_correction', self.bias_correction):
            bc1, bc2 = 1.0 - b1 ** (self.step + 1), 1.0 - b2 ** (self.step + 1)
        return self._schedule(), -oc['learning_rate'], bc1, bc2

    def apply_gradients(self):
        """The optax chain + apply_updates over the whole flat buffers: one fused host-scalar launch; with partitioned moments (bucket
        by bucket, each rank its chunk: a COLLECTIVE) or fp32 gradients, the device-scalar form of the same chain."""
        if self.shards is not None or self.f32_grads:
            self.prepare_step()
            self.apply_all()
        else:
            self._host_update(*self._scalars())
            self.store.update_transposed()
        self.finish_step()

    def prepare_step(self):
        """Write this step's scalars {sched, -lr, fp32(1) / fp32(bc1), fp32(1) / fp32(bc2)} (the reciprocals as the host-scalar kernels form
        them from their float arguments) into the device vector the captured Adam launches read: a ring of two pinned host vectors, each
        rewritten only after the copy that last read it has completed, so the host may run ahead of the stream."""
        dev = self.store.device
        if self.hyper is None:
            self.hyper = torch.zeros(4, dtype=torch.float32, device=dev)
            self._hyper_host = [torch.zeros(4, dtype=torch.float32, pin_memory=dev.type == 'cuda') for _ in range(2)]
            self._hyper_ev, self._hyper_turn = [None, None], 0
        i = self._hyper_turn
        self._hyper_turn ^= 1
        if self._hyper_ev[i] is not None:
            self._hyper_ev[i].synchronize()
        sched, neg_lr, bc1, bc2 = self._scalars()
        f32 = np.float32
        self._hyper_host[i].copy_(torch.tensor([sched, neg_lr, float(f32(1.0) / f32(bc1)), float(f32(1.0) / f32(bc2))], dtype=torch.float32))
        self.hyper.copy_(self._hyper_host[i], non_blocking=True)
        if dev.type == 'cuda':
            self._hyper_ev[i] = torch.cuda.Event()
            self._hyper_ev[i].record()

    def apply_range(self, lo, hi, mu=None, nu=None, transposed=True):
        """mu / nu: the moments of [lo, hi) when they do not live at p.mu[lo:hi] (zero.MomentShards)."""
        p = self.store
        assert lo % 2048 == 0 and hi % 2048 == 0
        grad = p.grad32 if self.f32_grads else p.grad
        ops.adam_bf16_update_dev(p.master[lo:hi], p.work[lo:hi], grad[lo:hi], p.mu[lo:hi] if mu is None else mu,
                                 p.nu[lo:hi] if nu is None else nu, None if p.orig is None else p.orig[lo:hi],
                                 p.decay_flags[lo // 2048:hi // 2048], *self._adam_args(), self.hyper)
        if transposed:
            p.update_transposed(lo, hi)

    def apply_shard(self, lo, hi, mu, nu):
        self.apply_range(lo, hi, mu=mu, nu=nu, transposed=False)      # (MomentShards.update rewrites the bucket's transposed copies)

    def apply_all(self):
        """apply_range over the whole buffers; with partitioned moments every bucket's shard (a COLLECTIVE)."""
        if self.shards is None:
            self.apply_range(0, self.store.total)
            return
        for key in self.shards.table:
            self.shards.update(key, self.apply_shard)

    def finish_step(self):
        self.step += 1

    # ---- pieces of the checkpoint forms
    def _moments(self):
        """(mu, nu) of the whole model (partitioned: gathered from every rank, a COLLECTIVE)."""
        return (self.store.mu, self.store.nu) if self.shards is None else self.shards.full_moments()

    def _flat_bf16(self, tree):
        """A tree of the parameters' shape as the flat bf16 buffer of the store's layout (on the host)."""
        p = self.store
        host = torch.zeros(p.total, dtype=torch.bfloat16)
        for name, *_ in p.specs:
            o, n = p.offsets[name]
            leaf = tree
            for k in name.split('/'):
                leaf = leaf[k]
            host[o:o + n] = leaf.reshape(-1).to(torch.bfloat16)
        return host

    def _load_moments(self, mu_tree, nu_tree):
        mu, nu = self._flat_bf16(mu_tree), self._flat_bf16(nu_tree)
        if self.shards is None:
            self.store.mu.copy_(mu)
            self.store.nu.copy_(nu)
        else:
            self.shards.store_moments(mu, nu)


def vision_cut_buckets(params, Lv, head):
    """Gradient buckets [(key, lo, hi)] = ranges of the flat buffers in the order backward makes them final (params.py lays the towers
    out in that order, and a tower's layers in ascending order, which backward walks downwards), and the vision layers they are cut at:
      `head`         the buckets in front of the vision tower, e.g. 'joint' (final after backward_stage_joint) and 'audio'
      ('vision', l)  vision layers >= l (+ final_ln, cls_proj, attention pool), down to the previous cut
      'vision_end'   the rest of the vision tower (first layers, pre_ln, cls, patch embedding)
    The vision tower (the last to finish) is cut at 2/3 and 1/3 of its depth, so only ~1/3 of its gradients -- < 10 % of all gradient
    bytes for the base and large pretraining models -- is reduced after the last backward kernel."""
    v0, v1 = params.tower_ranges['vision_encoder']
    assert v1 == params.total and head[-1][2] == v0
    cuts = sorted({l for l in (Lv - Lv // 3, Lv - 2 * (Lv // 3)) if 0 < l < Lv}, reverse=True)
    lo_of = lambda l: params.offsets[f'vision_encoder/transformer/layer_{l:02d}/pre_attn_ln/scale'][0]
    buckets, hi = list(head), v1
    for l in cuts:
        buckets.append((('vision', l), lo_of(l), hi))
        hi = lo_of(l)
    buckets.append(('vision_end', v0, hi))
    assert all(lo % 2048 == 0 and hi_ % 2048 == 0 and lo < hi_ for _, lo, hi_ in buckets)
    assert sum(hi_ - lo for _, lo, hi_ in buckets) == params.total
    return buckets, cuts


def comm_stream_disabled():
    """MR_NO_COMM_STREAM=1, read when a bucket is issued (bench.py sets and clears it between steps of one process for its exclusive
    timing pass): the bucket's kernels are issued in line -- beside a bucket's Adam kernel a whole-CU GEMM of either tower waits for
    CUs, and its HIP-event duration would include that wait."""
    return os.environ.get('MR_NO_COMM_STREAM') == '1'


class BucketSchedule:
    """One backward's hand-over of finished gradient buckets to the comm stream.  Buckets are enqueued in ONE program order on ONE
    stream, the same on every rank, as RCCL requires; `log` lists their keys in that order.  With the library's RCCL communicator
    (dist.NativeComm) the whole sequence is capturable.  Serves the pretraining and the finetuning step alike, so MR_NO_COMM_STREAM
    (comm_stream_disabled) holds for the finetuning step as well, where nothing sets it.
    comm = None: no collective (the buckets are still updated one by one); update = False leaves the averaged gradients in the
    gradient buffer and the parameters untouched; timeline: a list that receives (key, megabytes, HIP events at ready / reduced /
    updated) per bucket (eager steps only)."""

    def __init__(self, state, buckets, comm, comm_stream, update=True, timeline=None):
        self.state, self.comm, self.comm_stream, self.update, self.timeline = state, comm, comm_stream, update, timeline
        self.ranges = {key: (lo, hi) for key, lo, hi in buckets}
        self.log = []

    def _event(self):
        if self.timeline is None:
            return None
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        return e

    def finish(self, key, producer):
        """The bucket's gradients are final on stream `producer`: on the comm stream, behind them, nan_to_num + all-reduce(mean)
        (pretrain_model.py:328-329; finetune/optimization.py:148-149) and the optimizer update of that range, while the producer
        goes on with backward."""
        st, (lo, hi) = self.state, self.ranges[key]
        self.log.append(key)
        cs = producer if comm_stream_disabled() else self.comm_stream
        cs.wait_stream(producer)
        with torch.cuda.stream(cs):
            g = (st.store.grad32 if st.f32_grads else st.store.grad)[lo:hi]
            e_ready = self._event()
            if self.comm is not None:
                ops.nan_to_num_(g)
                self.comm.allreduce_mean(g)
            e_reduced = self._event()
            if self.update and st.shards is not None:
                st.shards.update(key, st.apply_shard)
            elif self.update:
                st.apply_range(lo, hi)
            e_updated = self._event()
        if self.timeline is not None:
            self.timeline.append((str(key), (hi - lo) * g.element_size() / 1e6, e_ready, e_reduced, e_updated))
