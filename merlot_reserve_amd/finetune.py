"""VCR finetuning step on the MI355X kernels (BASELINE config 5): the reference's
finetune/vcr/qa_qar_joint_finetune.py (F) + finetune/optimization.py (FO), name for name.

    reference                                                     here
    ------------------------------------------------------------  ----------------------------------------------------
    MerlotReserveVCR.from_config / __call__(batch)      F:144-170 MerlotReserveVCR.from_config(config, device=...) /
                                                                  .apply({'params': p}, batch) -> logits [B, 2, A] fp32
    train_loss_fn(state, params, batch)                 F:188-195 train_loss_fn(...) -> (loss, {'is_right', 'loss'})
    construct_finetuning_train_state(opt_config, model, FO:56-105 same name -> (state, tx_fns=None)
      params)
    finetune_train_step(state, batch, loss_fn, tx_fns)  FO:106-191 same name -> (state, loss_info)

One process per GPU; with a merlot_reserve_amd.dist.Comm the bf16 gradients are averaged over ranks (pmean, FO:143)
in two buckets, the first overlapped with the vision tower's backward.  The optimizer is replicated: the 8-way
sharding of the Adam state (FO:38-53, 148-171) is a 16 GB-TPU-core memory measure, not arithmetic.

batch (one device's slice): 'image' [B, h*w, 768] bf16 on the GPU, 'answers' [B, 2, A, T] int32 (numpy),
'labels' [B, 2] int32 (numpy).

Program: ViT (S = h*w + 1) + attention pool -> [B, V, H]; ONE index-driven gather builds the 2*A*B joint sequences
[T text tokens | V vision tokens] (the 8-fold `repeat` of the image rows, F:157, is just the gather list);
joint encoder with one validity code per position; the row at the first MASK of every sequence; Dense(1); softmax
cross-entropy over the A answers; hand-written backward through the same kernels as the pretraining step.

The step itself (finetune_train_step, the scanned step, FinetuneTrainState, FinetuneGraphStep) is shared with the TVQA model of
tvqa.py: it asks the model's engine (a FinetuneEngine) for its backward stages and their gradient buckets, its metric names, how to
slice one example out of a batch and which batch entries live on the device.
"""
import numpy as np
import torch

from . import ops
from .engine import BF16, F32, I32, PooledTower, TowerEngine, TowerState
from .optim import AdamStepState, BucketSchedule, lr_scale_linearwarmup_lineardecay, vision_cut_buckets
from .params import VOCAB, ParamStore, decay_finetune, vcr_param_specs
from .planner import MASK, PADDING, csr_from_pairs, csr_gather, rot_scale_table, rotary_coords_2d, vit_tables


class VCRDims:
    def __init__(self, config, B):
        d, m = config['data'], config['model']
        self.B, self.H = B, m['hidden_size']
        self.nh = self.H // 64
        self.gh, self.gw = m['output_grid']
        self.hw = self.gh * self.gw
        self.pr = m['vit_pooling_ratio']
        self.V = self.hw // (self.pr ** 2)
        self.pp3 = m['vit_patch_size'] ** 2 * 3
        self.A = d.get('num_answers', 4)
        self.T = d['lang_seq_len']
        self.n = B * 2 * self.A
        self.Nv = B                                   # images
        self.Sv, self.Sj = self.hw + 1, self.T + self.V
        self.Lv, self.Lj = m['vit_num_layers'], m['joint_num_layers']


def build_vcr_plan(answers, d):
    """Every integer decision of MerlotReserveVCR.__call__ (F:150-168), from `answers` [B, 2, A, T] alone."""
    ans = np.asarray(answers).astype(np.int64).reshape(d.n, d.T)
    assert ans.min() >= 0 and ans.max() < VOCAB, 'token id out of range'
    b_of = np.arange(d.n) // (2 * d.A)
    codes = np.concatenate([ans, VOCAB + b_of[:, None] * d.V + np.arange(d.V)[None]], 1)            # [n, Sj]
    plan = {}
    plan['joint_gather_indptr'], plan['joint_gather_idx'] = csr_gather(codes)
    valid = np.concatenate([ans != PADDING, np.ones((d.n, d.V), bool)], 1)                          # M:726-728
    plan['joint_code'] = np.where(valid, 0, -1).astype(np.int32).reshape(-1)
    pool_idx = np.argmax((ans == MASK).astype(np.float32), 1)                                       # F:165: first MASK, else 0
    rows = np.arange(d.n) * d.Sj + pool_idx
    plan['pool_indptr'], plan['pool_idx'] = np.arange(d.n + 1, dtype=np.int32), rows.astype(np.int32)
    plan['poolT_indptr'], plan['poolT_idx'] = csr_from_pairs(rows, np.arange(d.n), d.n * d.Sj)
    # transpose of the embedding gather; PAD positions carry exactly zero gradient (masked keys, and never pooled)
    pos_rows = (np.arange(d.n)[:, None] * d.Sj + np.arange(d.T)[None])
    keep = ans != PADDING
    # ... unless the pooled position is itself PAD (a sequence with no MASK whose first token is PAD): that query row
    # attends uniformly to every position (all its keys carry the same -1e10, M:353-356), so the whole sequence gets gradient
    keep |= (ans[np.arange(d.n), pool_idx] == PADDING)[:, None]
    plan['embT_indptr'], plan['embT_idx'] = csr_from_pairs(ans[keep], pos_rows[keep], VOCAB)
    plan['pool_pos'] = pool_idx.astype(np.int32)
    return plan


class FinetuneEngine(TowerEngine):
    """What the finetuning programs (VCR here, TVQA in tvqa.py) share, and what the shared step (finetune_train_step, FinetuneGraphStep)
    asks of an engine.  A subclass sets: metric_names (the keys of loss_info()), device_keys (the batch entries that live on the device, in
    the order forward_device takes them), batch_size / slice_example (the size of a batch and one example of it), build_plan,
    forward_device, loss_and_grad_logits, backward_stages (the third field of a stage marks the vision tower's: the only one whose layers
    are cut into ('vision', l) buckets), head_buckets; and the buffers named below."""

    def _idx_capacity(self):
        return self.tj.M + 64

    def upload(self, batch, plan=None):
        """The host part of a step: the plan's index lists and the labels into their persistent device buffers."""
        self.set_plan(plan if plan is not None else self.build_plan(batch))
        self.labels_dev.copy_(torch.from_numpy(np.ascontiguousarray(np.asarray(batch['labels']).astype(np.int32).reshape(-1))), non_blocking=True)

    def forward(self, batch, plan=None):
        self.upload(batch, plan)
        return self.forward_device(*[batch[k] for k in self.device_keys])

    def backward(self):
        assert not self.fwd_only, f'this program was built forward-only ({type(self).__name__}(..., train=True) has the backward)'
        for stage, _key, _cuts in self.backward_stages():
            stage()

    def gradient_buckets(self):
        """(buckets, vision cuts): ranges of the flat gradient buffer in the order backward makes them final -- the subclass's
        head_buckets(), then the vision tower cut at 2/3 and 1/3 of its depth and 'vision_end' = the rest (optim.vision_cut_buckets)."""
        return vision_cut_buckets(self.p, self.d.Lv, self.head_buckets())

    def _backward_proj_head(self):
        """Backward of the Dense(1) head and of the pooling: d proj, d pooled_h, and self.Dj = zero except the pooled rows."""
        dl = self.dlogits[:, :1]
        self.gemm(dl, self.pooled_h, self.G['proj/kernel'], transA=True)              # d proj [1, H] = dlogits^T . pooled_h
        self.gemm(dl, self.W['proj/kernel'], self.d_pooled)                           # d pooled_h = dlogits . proj^T
        ops.segment_sum([self.d_pooled], self._pl('poolT_indptr'), self._pl('poolT_idx'), self.Dj)   # zero except the pooled rows


class VCREngine(FinetuneEngine):
    metric_names = ('loss', 'is_right')
    device_keys = ('image',)

    @staticmethod
    def batch_size(batch):
        return int(batch['image'].shape[0])

    @staticmethod
    def slice_example(batch, i):
        return {'image': batch['image'][i:i + 1], 'answers': np.asarray(batch['answers'])[i:i + 1], 'labels': np.asarray(batch['labels'])[i:i + 1]}

    def __init__(self, config, B, params, device, train=True):
        """train=False: the forward-only program (evaluation of a checkpoint: pred_step, finetune_eval.val_epoch) -- the same launch sequence up to
        the logits with nothing kept for a backward: no gradient buffers (Dv, Dj, d_*, dlogits), no backward scratch (the GEMMs then run
        without a split-K workspace), one layer's worth of tower activations and no gelu' copy (the fc1 GEMM's c2 = NULL)."""
        self.config, self.p, self.dev = config, params, torch.device(device)
        self.d = d = VCRDims(config, B)
        self.dtype, self.fwd_only, self.W, self.G = BF16, not train, params.w, getattr(params, 'g', None)
        dev, H = self.dev, d.H
        z = lambda *s: torch.zeros(*s, dtype=BF16, device=dev)
        f = lambda *s: torch.zeros(*s, dtype=F32, device=dev)
        self.vision = PooledTower('vision_encoder', B, d.hw, d.pp3, d.Lv, H, vit_tables(d.gh, d.gw, d.pr, B), dev, train=train, saved=train)
        self.tv = self.vision.st
        self.tj = TowerState(d.n * d.Sj, H, d.Lj, d.n, d.Sj, dev, saved=train)
        # joint rotary (text: segment 0, token index 1..T; vision: pooled-grid (h, w), segment 0 -- identical for every sequence:
        # M:697-720 with token_segment_idx = 0, F:161)
        coords = np.zeros((d.Sj, 4))
        coords[:d.T, 3] = (1.0 + np.arange(d.T)) / 1024.0
        coords[d.T:, :2] = rotary_coords_2d(d.gh // d.pr, d.gw // d.pr)
        self.joint_rot = torch.from_numpy(rot_scale_table(coords)).to(dev)
        self.pooled_h = z(d.n, H)
        self.logits = f(d.n, 8)                       # column 0 = the Dense(1) output
        self.loss_acc = f(2)                          # [loss, is_right]
        self.labels_dev = torch.zeros(2 * B, dtype=I32, device=dev)
        self.side_stream = None
        self.plan_dev, self._plan_caps, self._plan_views, self.plan_frozen = None, {}, {}, False
        self.cur = None
        if self.fwd_only:
            return
        # static transpose of the image-row tiling: d_imgs_seq[b*V + i] = sum_j Dj[(b*2A + j)*Sj + T + i]
        bb, ii, jj = np.meshgrid(np.arange(B), np.arange(d.V), np.arange(2 * d.A), indexing='ij')
        ip, ix = csr_from_pairs((bb * d.V + ii).reshape(-1), ((bb * 2 * d.A + jj) * d.Sj + d.T + ii).reshape(-1), B * d.V)
        self.visT = (torch.from_numpy(ip).to(dev), torch.from_numpy(ix).to(dev))
        self.d_pooled = z(d.n, H)
        self.dlogits = z(d.n, 8)
        self.Dj = z(self.tj.M, H)
        Mmax = max(self.tv.M, self.tj.M)
        self.sc_main = self._make_scratch(Mmax, B * d.V, B * d.hw, H, d.nh)
        self.sc_side = self.sc_main                   # single-stream program: the two towers are strictly sequential
        self.cur = self.sc_main

    def build_plan(self, batch):
        return build_vcr_plan(batch['answers'], self.d)

    def forward_device(self, image):
        d, W, tj = self.d, self.W, self.tj
        self.vision.forward(self, image.reshape(d.B * d.hw, d.pp3))
        ops.segment_sum([W['token_encoder/Embed_0/embedding'], self.vision.seq], self._pl('joint_gather_indptr'), self._pl('joint_gather_idx'), tj.xin)
        self.encoder_forward(tj, 'joint_transformer', self.joint_rot, self._pl('joint_code'))
        ops.segment_sum([tj.xf], self._pl('pool_indptr'), self._pl('pool_idx'), self.pooled_h)
        self.gemm(self.pooled_h, W['proj/kernel'], self.logits, transB=True)          # Dense(1): [n, H] x [1, H]^T -> column 0
        return self.logits[:, 0].view(d.B, 2, d.A)

    def loss_and_grad_logits(self):
        """train_loss_fn (F:188-195) on the device + dL/dlogits."""
        assert not self.fwd_only, 'the forward-only program forms no loss gradient'
        d = self.d
        self.loss_acc.zero_()
        ops.softmax_xent(self.logits, d.A * 8, 8, self.labels_dev, 2 * d.B, d.A, 1.0 / (2 * d.B), self.loss_acc[0:1], self.loss_acc[1:2], self.dlogits)
        return self.loss_acc

    def backward_stages(self):
        """[(stage, the bucket of gradient_buckets() that is final after it, whether it is the VISION tower's stage: that one takes
        layer_done and the step hands over the ('vision', l) buckets of gradient_buckets() from it)]"""
        return [(self.backward_stage_joint, 'joint', False), (self.backward_stage_vision, 'vision_end', True)]

    def head_buckets(self):
        """'joint' = [proj, joint tower, token table]"""
        return [('joint', 0, self.p.tower_ranges['vision_encoder'][0])]

    def backward_stage_joint(self):
        G, tj = self.G, self.tj
        self._backward_proj_head()
        # the tower-level reductions (final / pre LayerNorm) are deferred into ONE mr_reduce_partials launch each side of the layers, as in
        # the pretraining engine (they were two-level immediate reductions here: 19 launches of ~68 us per VCR step, round-3 profile)
        tr = self._begin_tower_reductions()
        Dj = self.encoder_backward(tj, 'joint_transformer', self.joint_rot, self._pl('joint_code'), self.Dj, tr=tr)
        self._flush_tower_reductions(tr)
        ops.segment_sum([Dj], self._pl('embT_indptr'), self._pl('embT_idx'), G['token_encoder/Embed_0/embedding'])
        ops.segment_sum([Dj], self.visT[0], self.visT[1], self.vision.d_seq)

    def loss_info(self):
        return self.info_from(self.loss_acc.tolist())

    @staticmethod
    def info_from(la):
        """The dict of loss_info() from a host copy of loss_acc (also the rows of the finetuning driver's metrics ring)."""
        return {'loss': la[0], 'is_right': la[1]}


def _mean_over_ranks(info, eng, comm):
    """The step's metrics averaged over the ranks of `comm` (FO:187-189)."""
    if comm is None or comm.world <= 1:
        return info
    t = torch.tensor([info[k] for k in eng.metric_names], dtype=torch.float32, device=eng.dev)
    comm.allreduce_mean(t)
    return {k: float(v) for k, v in zip(eng.metric_names, t)}


# ------------------------------------------------------------------------------------------------ reference-named API
class MerlotReserveVCR:
    """F:144-170"""
    engine_cls = VCREngine
    param_specs = staticmethod(vcr_param_specs)

    def __init__(self, config, device='cuda:0', rank=0, world=1, comm=None, seed=0, shard_optimizer=False, train=True, params_store=None):
        """shard_optimizer = True: the Adam moments are partitioned over the ranks of `comm` (FO:148-171; zero.py).
        train = False: the forward-only model (the engine's forward-only program over a parameter store without optimizer state and without a
        gradient buffer): what evaluates a checkpoint's `params` alone (finetune/vcr/submit_to_leaderboard.py:117-122); no train state can be
        built on it.  params_store: read the parameters of ANOTHER model's store instead of owning one (forward_only_view)."""
        self.config, self.device, self.rank, self.world, self.comm, self.seed = config, torch.device(device), rank, world, comm, seed
        self.params_store, self.engine, self._last_tree = params_store, None, None
        self.train, self._shared_store = bool(train), params_store is not None
        self.shard_optimizer, self._train_state = shard_optimizer, None      # (the FinetuneTrainState built on this model last)
        assert not shard_optimizer or comm is not None, 'shard_optimizer needs a communicator (its world may be 1)'
        assert train or not shard_optimizer, 'a forward-only model has no optimizer state to shard'
        assert params_store is None or not train, 'only a forward-only model may read another model\'s parameter store'

    @property
    def shards(self):
        """zero.MomentShards of a model built with shard_optimizer=True, once it has a train state (which owns them)."""
        return None if self._train_state is None else self._train_state.shards

    @classmethod
    def from_config(cls, config, **kwargs):
        if 'model' not in config or 'data' not in config:
            raise ValueError("config must have 'model' and 'data' sections (the reference's YAML schema)")
        return cls(config, **kwargs)

    def forward_only_view(self):
        """A forward-only model of the same class that READS THIS MODEL'S working parameters (no copy: a step of this model is seen by the
        next forward of the view): the driver's validation pass.  Its engine is built for the batch size of its first batch."""
        assert self.params_store is not None, 'call init_from_dummy_batch(batch) first'
        return type(self)(self.config, device=self.device, seed=self.seed, train=False, params_store=self.params_store)

    def _ensure(self, batch):
        B = self.engine_cls.batch_size(batch)
        if self.engine is None:
            if self.params_store is None:
                self.params_store = ParamStore(self.config, self.device, seed=self.seed, specs=self.param_specs(self.config),
                                               decay_rule=decay_finetune, with_orig=self.train,
                                               with_optimizer=self.train and not self.shard_optimizer, with_grad=self.train)
            self.engine = self.engine_cls(self.config, B, self.params_store, self.device, train=self.train)
        elif self.engine.d.B != B:
            raise ValueError(f'this model was initialised for {self.engine.d.B} examples per device, got {B}')
        return self.engine

    def init_from_dummy_batch(self, dummy_batch):
        self._ensure(dummy_batch)
        self._last_tree = self.params_store.master_tree()
        return self._last_tree

    def _load(self, variables):
        if variables is None:
            return
        assert not self._shared_store, 'this forward-only view reads another model\'s parameters: load them there'
        tree = variables['params'] if 'params' in variables else variables
        if tree is not self._last_tree:
            # a pretrained tree still holds audio_encoder / head / span_encoder (popped at F:181-183) -- they are not read
            self.params_store.load_tree(tree)
            self._last_tree = tree

    def apply(self, variables, batch):
        eng = self._ensure(batch)
        self._load(variables)
        return eng.forward(batch)

    def __call__(self, batch):
        return self.apply(None, batch)


class FinetuneTrainState(AdamStepState):
    """FO:77-90: the bf16 Adam with bias correction, subtract_old_weights decay (the store's `orig`) and the linear schedule."""
    eps = 1e-6
    bias_correction = True

    def __init__(self, model, opt_config):
        super().__init__(model.params_store, opt_config)
        self._model, self.apply_fn = model, model.apply
        if model.shard_optimizer:        # the model's moments exist once: a later state on the same model takes them over, as it does p.mu / p.nu
            from .zero import MomentShards
            self.shards = model.shards or MomentShards(self.store, model.engine.gradient_buckets()[0], model.comm)
        model._train_state = self

    @property
    def params(self):
        return self.store.master_tree()

    def _schedule(self):
        oc = self.opt_config
        return lr_scale_linearwarmup_lineardecay(self.step, oc['num_warmup_steps'], oc['num_train_steps'])

    def _host_update(self, sched, neg_lr, bc1, bc2):
        p = self.store
        ops.adam_bf16_update_finetune(p.master, p.work, p.grad, p.mu, p.nu, p.orig, p.decay_flags, *self._adam_args(), sched, neg_lr, bc1, bc2)

    def apply_gradients(self):
        """FO:77-90 + apply_updates."""
        super().apply_gradients()
        return self

    # ---- checkpoint form: flax `to_state_dict` of the finetuning chain (finetune/optimization.py:77-90): '0' = the bf16 Adam state
    # {count, mu, nu}, '1' = subtract_old_weights' orig_params (bf16), '2' = add_decayed_weights (empty), '3' = the schedule's count,
    # '4' = scale (empty).  (The reference notes that ITS finetuning state cannot be restarted; this one can.)  With partitioned
    # moments (shard_optimizer=True) state_dict() gathers them from every rank: a COLLECTIVE, see checkpoint.save_checkpoint(rank=).
    def state_dict(self):
        p = self.store
        mu, nu = self._moments()
        count = torch.tensor(self.step, dtype=torch.int32)
        return {'step': self.step, 'params': p.master_tree(),
                'opt_state': {'0': {'count': count, 'mu': p._to_tree(mu), 'nu': p._to_tree(nu)}, '1': {'orig_params': p._to_tree(p.orig)},
                              '2': {}, '3': {'count': count.clone()}, '4': {}}}

    def load_state_dict(self, sd):
        p = self.store
        p.load_tree(sd['params'])
        self.step = int(sd.get('step', 0))
        opt = sd.get('opt_state')
        if not opt:
            return self
        self._load_moments(opt['0']['mu'], opt['0']['nu'])
        if opt.get('1') and 'orig_params' in opt['1']:
            p.orig.copy_(self._flat_bf16(opt['1']['orig_params']))
        return self


def construct_finetuning_train_state(opt_config, model, params=None, only_state=False):
    """FO:56-105.  Returns (state, tx_fns) like the reference (tx_fns is None: the chain is one fused kernel)."""
    if model.engine is None:
        raise ValueError('call model.init_from_dummy_batch(batch) first')
    if not model.train:
        raise ValueError('a forward-only model (train=False) has no optimizer state: build the model with train=True')
    if params is not None:
        model._load({'params': params})
    state = FinetuneTrainState(model, opt_config)
    return state if only_state else (state, None)


def train_loss_fn(state, params, batch):
    """F:188-195: forward + softmax cross-entropy; returns (loss, {'is_right', 'loss'}) as host floats."""
    model = state._model
    model.apply(None if params is None else {'params': params}, batch)
    model.engine.loss_and_grad_logits()
    info = model.engine.loss_info()
    return info['loss'], info


def _model_of(state_or_model):
    """pred_step takes a train state (as the reference's does) or a model, forward-only ones included."""
    return getattr(state_or_model, '_model', state_or_model)


def pred_step(state_or_model, batch):
    """F:202-204: {'logprobs': log_softmax(logits) [B, 2, A], 'preds': argmax [B, 2]}; host arithmetic on the 2 B A logits."""
    logits = _model_of(state_or_model).apply(None, batch).float().cpu()
    return {'logprobs': torch.log_softmax(logits, -1), 'preds': torch.argmax(logits, -1)}


def _backward_reduce_update(state):
    """Backward from the engine's dlogits with every finished gradient BUCKET handed to a second stream (optim.BucketSchedule):
    nan_to_num -> all-reduce(mean) over ranks (FO:148-149) -> the optimizer chain on that range (FO:77-90), while the main stream goes
    on with the next stage of backward (engine.backward_stages(): VCR joint -> vision, four buckets; TVQA joint -> audio -> vision,
    five).  With the library's RCCL communicator the whole sequence is capturable (FinetuneGraphStep)."""
    model = state._model
    eng, comm = model.engine, model.comm
    main = torch.cuda.current_stream()
    if getattr(eng, 'comm_stream', None) is None:
        eng.comm_stream = torch.cuda.Stream(device=eng.dev)
    buckets, cuts = eng.gradient_buckets()
    q = BucketSchedule(state, buckets, comm, eng.comm_stream)
    eng.bucket_log = q.log
    stages = eng.backward_stages()
    stages[0][0]()
    q.finish(stages[0][1], main)
    with ops.gemm_cus(comm.world if comm is not None else 1):      # a bucket's all-reduce runs beside the next towers' GEMMs
        for stage, key, is_vision in stages[1:]:
            if is_vision:
                stage(layer_done=lambda l: q.finish(('vision', l), main) if l in cuts else None)
            else:
                stage()
            q.finish(key, main)
    main.wait_stream(eng.comm_stream)


def finetune_train_step(state, batch, loss_fn=None, tx_fns=None, scan_minibatch=False):
    """FO:106-191: bf16 parameter copy -> forward -> loss -> backward -> nan_to_num -> mean over ranks -> optimizer.
    scan_minibatch (FO:125-146): gradients of the examples taken one at a time and SUMMED in bf16 (not averaged: as the reference
    notes, Adam rescales), the metrics averaged."""
    model = state._model
    eng = model._ensure(batch)
    if scan_minibatch:
        return _finetune_train_step_scanned(state, batch)
    eng.forward(batch)
    eng.loss_and_grad_logits()
    state.prepare_step()
    _backward_reduce_update(state)
    state.step += 1
    return state, _mean_over_ranks(eng.loss_info(), eng, model.comm)


def _finetune_train_step_scanned(state, batch):
    model = state._model
    eng, comm, p = model.engine, model.comm, model.params_store
    if getattr(model, '_engine1', None) is None:              # an engine for ONE example on the same parameter store
        model._engine1 = type(eng)(model.config, 1, p, model.device)
    e1 = model._engine1
    # Memory: the one-example engine keeps its own activations / scratch beside the B-example one (the price of scan_minibatch here:
    # ~1/B of the big engine's activations; free it with `model._engine1 = None` when scanning is switched off), and ONE persistent
    # parameter-sized bf16 accumulator, zeroed in place each step.
    if getattr(model, '_scan_acc', None) is None or model._scan_acc.shape != p.grad.shape:
        model._scan_acc = torch.zeros_like(p.grad)
    acc = model._scan_acc
    acc.zero_()
    losses = []
    for i in range(eng.d.B):
        micro = eng.slice_example(batch, i)
        p.grad.zero_()                                        # a leaf this example's backward does not write must contribute 0, not the previous example's value
        e1.forward(micro)
        e1.loss_and_grad_logits()
        e1.backward()
        ops.add_(acc, p.grad)                                 # bf16 + bf16 -> bf16, like the scan's `a + b` on bf16 leaves
        losses.append(e1.loss_info())
    p.grad.copy_(acc)
    if comm is not None:
        ops.nan_to_num_(p.grad)
        comm.allreduce_mean(p.grad)
    state.prepare_step()
    state.apply_all()
    state.step += 1
    info = {k: float(np.mean([l[k] for l in losses])) for k in losses[0]}
    return state, _mean_over_ranks(info, eng, comm)


class FinetuneGraphStep:
    """hipGraph replay of finetune_train_step: the step is a fixed launch sequence over fixed buffers, so forward + loss + backward +
    the bucket reductions + the optimizer are captured ONCE and replayed -- with the library's RCCL communicator
    (dist.NativeComm) the collectives are stream-ordered launches inside the same graph (a torch.distributed comm is host-scheduled
    and cannot be captured); per batch only the engine's device inputs (VCR: the image), the labels, the plan's index lists and the
    step's four scalars are copied into their persistent buffers.  Same results as finetune_train_step (tests/test_vcr_gpu.py)."""

    def __init__(self, state, batch):
        self.state, self.model = state, state._model
        eng = self.eng = self.model._ensure(batch)
        comm = self.model.comm
        assert comm is None or getattr(comm, 'capturable', False), 'only the library RCCL communicator (dist.NativeComm) can be captured'
        finetune_train_step(state, batch)                  # eager step: every buffer and plan capacity exists afterwards
        self.inputs = [torch.zeros_like(batch[k]) for k in eng.device_keys]
        eng.plan_frozen = True
        torch.cuda.synchronize()
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph, capture_error_mode='thread_local'):
            eng.forward_device(*self.inputs)
            eng.loss_and_grad_logits()
            _backward_reduce_update(state)

    def __call__(self, batch, plan=None):
        eng = self.eng
        self.state.prepare_step()
        for buf, k in zip(self.inputs, eng.device_keys):
            buf.copy_(batch[k], non_blocking=True)
        eng.upload(batch, plan)
        self.graph.replay()
        self.state.step += 1
        return self.state


class VCRGraphStep(FinetuneGraphStep):
    """The captured VCR step."""


def make_vcr_batch(config, B, seed=0, device='cpu'):
    """Synthetic VCR batch with the structure of finetune/data: answers = [question tokens, MASK, answer tokens, PAD...]."""
    d = VCRDims(config, B)
    rng = np.random.default_rng(seed)
    ans = np.zeros((B, 2, d.A, d.T), dtype=np.int32)
    for idx in np.ndindex(B, 2, d.A):
        nq, na = int(rng.integers(4, d.T // 3)), int(rng.integers(2, d.T // 3))
        ans[idx][:nq] = rng.integers(10, VOCAB, size=nq)
        ans[idx][nq] = MASK
        ans[idx][nq + 1:nq + 1 + na] = rng.integers(10, VOCAB, size=na)
    g = torch.Generator().manual_seed(seed)
    return {'image': torch.rand(B, d.hw, d.pp3, generator=g).to(torch.bfloat16).to(device), 'answers': ans,
            'labels': rng.integers(0, d.A, size=(B, 2)).astype(np.int32)}
