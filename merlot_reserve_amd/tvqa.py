"""TVQA finetuning step on the MI355X kernels: the reference's finetune/tvqa/tvqa_finetune.py (F) on the shared finetuning
step of merlot_reserve_amd.finetune (finetune/optimization.py), name for name.

    reference                                                     here
    ------------------------------------------------------------  ----------------------------------------------------
    MerlotReserveTVQA.from_config / __call__(batch)     F:157-258 MerlotReserveTVQA.from_config(config, device=...) /
                                                                  .apply({'params': p}, batch) -> (logits_from_audio,
                                                                  logits_from_text), each [B, A] fp32
    train_loss_fn(state, params, batch)                 F:277-294 train_loss_fn(...) -> (loss, {'is_right_audio', 'is_right_text',
                                                                  'loss_audio', 'loss_text'})
    pred_step(state, batch)                             F:300-310 same name -> the five outputs
    finetune_train_step(state, batch, ...)                        finetune.finetune_train_step serves both programs

batch (one device's slice): 'images' [B, nseg, h*w, 768] and 'audio_clips' [B, nseg, 3, 60, 65] bf16 on the GPU,
'textonly_seqs' / 'audio_seqs' [B, A, T, 2] int32 (numpy; token id, segment index), 'labels' [B] int32 (numpy).

Program: ViT on the B*nseg frames and the audio tower on the B*nseg*3 clips, each with its attention pool; ONE index-driven
gather over [token table | audio rows | image rows] builds the 2*A*B joint sequences [T tokens | nseg*V image rows] (audio
stream first, then the text stream; the A-fold `repeat`s of F:179 / F:198 are just the gather list); joint encoder with one
validity code and one "rotary" row per position; the row at the first MASK of every sequence; Dense(1); one A-way softmax
cross-entropy per stream against the same labels; hand-written backward in three stages (joint, audio, vision) through the
same kernels as the pretraining step.  It is the one finetuning program that trains the audio tower.  Single stream, like VCR.
"""
import numpy as np
import torch

from . import ops
from .engine import BF16, F32, I32, PooledTower, TowerState
from .finetune import FinetuneEngine, FinetuneGraphStep, MerlotReserveVCR, _model_of
from .params import VOCAB, tvqa_param_specs
from .planner import AUDIOSPAN, MASK, audio_tables, build_tvqa_plan, tvqa_image_transpose, vit_tables


class TVQADims:
    def __init__(self, config, B):
        d, m = config['data'], config['model']
        self.B, self.H = B, m['hidden_size']
        self.nh = self.H // 64
        self.gh, self.gw = m['output_grid']
        self.hw = self.gh * self.gw
        self.pr = m['vit_pooling_ratio']
        self.V = self.hw // (self.pr ** 2)
        self.pp3 = m['vit_patch_size'] ** 2 * 3
        self.A = d.get('num_answers', 5)
        self.T = d['lang_seq_len']
        self.nseg = d['num_segments']
        self.nas = d.get('num_audio_subsegments', 3)
        self.nspans = self.nseg * self.nas
        self.a_raw, self.a_patch, self.a_tok = m['audio_seq_length'], m['audio_patch_size'], m['audio_token_length']
        self.a_len = self.a_raw // self.a_patch
        self.a_pool = self.a_raw // (self.a_tok * self.a_patch)
        self.span_len = m['text_span_length']
        self.n = 2 * self.A * B                                   # joint sequences: audio stream, then text stream
        self.Nv, self.Sv = B * self.nseg, self.hw + 1
        self.Na, self.Sa = B * self.nspans, self.a_len + 1
        self.Sj = self.T + self.nseg * self.V
        self.Lv, self.La, self.Lj = m['vit_num_layers'], m['audio_num_layers'], m['joint_num_layers']


class TVQAEngine(FinetuneEngine):
    metric_names = ('loss', 'is_right_audio', 'is_right_text', 'loss_audio', 'loss_text')
    device_keys = ('images', 'audio_clips')

    @staticmethod
    def batch_size(batch):
        return int(batch['images'].shape[0])

    @staticmethod
    def slice_example(batch, i):
        return {'images': batch['images'][i:i + 1], 'audio_clips': batch['audio_clips'][i:i + 1],
                'textonly_seqs': np.asarray(batch['textonly_seqs'])[i:i + 1], 'audio_seqs': np.asarray(batch['audio_seqs'])[i:i + 1],
                'labels': np.asarray(batch['labels'])[i:i + 1]}

    def __init__(self, config, B, params, device, train=True):
        """train=False: the forward-only program, as finetune.VCREngine's."""
        self.config, self.p, self.dev = config, params, torch.device(device)
        self.d = d = TVQADims(config, B)
        self.dtype, self.fwd_only, self.W, self.G = BF16, not train, params.w, getattr(params, 'g', None)
        dev, H = self.dev, d.H
        z = lambda *s: torch.zeros(*s, dtype=BF16, device=dev)
        f = lambda *s: torch.zeros(*s, dtype=F32, device=dev)
        # the two input towers (the joint tower's "rotary" table depends on the batch's segment indices: it is part of the plan)
        self.vision = PooledTower('vision_encoder', d.Nv, d.hw, d.pp3, d.Lv, H, vit_tables(d.gh, d.gw, d.pr, d.Nv), dev, train=train, saved=train)
        self.audio = PooledTower('audio_encoder', d.Na, d.a_len, d.a_patch * 65, d.La, H, audio_tables(d.a_len, d.a_pool, d.Na), dev, train=train,
                                 pad_input=True, saved=train)
        self.tv, self.ta = self.vision.st, self.audio.st
        self.tj = TowerState(d.n * d.Sj, H, d.Lj, d.n, d.Sj, dev, saved=train)
        self.pooled_h = z(d.n, H)
        self.logits = f(d.n, 8)                       # column 0 = the Dense(1) output; rows [0, A B) audio stream, [A B, 2 A B) text stream
        self.loss_acc = f(4)                          # [loss_audio, is_right_audio, loss_text, is_right_text]
        self.labels_dev = torch.zeros(B, dtype=I32, device=dev)
        self.side_stream = None
        self.plan_dev, self._plan_caps, self._plan_views, self.plan_frozen = None, {}, {}, False
        self.cur = None
        if self.fwd_only:
            return
        # static transpose of the image-row tiling: every image row is read by the 2 A sequences of its example
        ip, ix = tvqa_image_transpose(d)
        self.visT = (torch.from_numpy(ip).to(dev), torch.from_numpy(ix).to(dev))
        self.d_pooled = z(d.n, H)
        self.dlogits = z(d.n, 8)
        self.Dj = z(self.tj.M, H)
        # Single-stream program: the three towers are strictly sequential and share ONE scratch set (the cls outputs feed nothing: the
        # towers' d_cls stay zero)
        Mmax = max(self.tv.M, self.ta.M, self.tj.M)
        self.sc_main = self._make_scratch(Mmax, max(d.Nv * d.V, d.Na * d.a_tok), max(d.Nv * d.hw, d.Na * d.a_len), H, d.nh)
        self.sc_side = self.sc_main
        self.cur = self.sc_main

    def build_plan(self, batch):
        return build_tvqa_plan(batch['textonly_seqs'], batch['audio_seqs'], self.d)

    def forward_device(self, images, audio_clips):
        d, W, tj = self.d, self.W, self.tj
        self.vision.forward(self, images.reshape(d.Nv * d.hw, d.pp3))                        # the B nseg frames (F:166-168)
        self.audio.forward(self, audio_clips.reshape(d.Na * d.a_len, d.a_patch * 65))        # the B nseg 3 clips (F:191-197)
        # joint tower on the 2 A B sequences (F:242-246)
        ops.segment_sum([W['token_encoder/Embed_0/embedding'], self.audio.seq, self.vision.seq], self._pl('joint_gather_indptr'),
                        self._pl('joint_gather_idx'), tj.xin)
        self.encoder_forward(tj, 'joint_transformer', self._pl('joint_rot'), self._pl('joint_code'))
        ops.segment_sum([tj.xf], self._pl('pool_indptr'), self._pl('pool_idx'), self.pooled_h)       # F:250-251
        self.gemm(self.pooled_h, W['proj/kernel'], self.logits, transB=True)          # Dense(1): [n, H] x [1, H]^T -> column 0
        AB = d.A * d.B
        return self.logits[:AB, 0].view(d.B, d.A), self.logits[AB:, 0].view(d.B, d.A)               # F:254-256

    def loss_and_grad_logits(self):
        """train_loss_fn (F:277-294) on the device + dL/dlogits: one A-way cross-entropy per stream, each the mean over B."""
        assert not self.fwd_only, 'the forward-only program forms no loss gradient'
        d = self.d
        AB = d.A * d.B
        self.loss_acc.zero_()
        for s in range(2):
            ops.softmax_xent(self.logits[s * AB:], d.A * 8, 8, self.labels_dev, d.B, d.A, 1.0 / d.B, self.loss_acc[2 * s:2 * s + 1],
                             self.loss_acc[2 * s + 1:2 * s + 2], self.dlogits[s * AB:])
        return self.loss_acc

    def backward_stages(self):
        return [(self.backward_stage_joint, 'joint', False), (self.backward_stage_audio, 'audio', False),
                (self.backward_stage_vision, 'vision_end', True)]

    def head_buckets(self):
        """'joint' = [proj, joint tower, token table]; 'audio' = the audio tower"""
        a0, a1 = self.p.tower_ranges['audio_encoder']
        return [('joint', 0, a0), ('audio', a0, a1)]

    def backward_stage_joint(self):
        G, tj = self.G, self.tj
        self._backward_proj_head()
        tr = self._begin_tower_reductions()
        Dj = self.encoder_backward(tj, 'joint_transformer', self._pl('joint_rot'), self._pl('joint_code'), self.Dj, tr=tr)
        self._flush_tower_reductions(tr)
        # the three transposes of the gather, each a fixed-order segment sum (no atomics)
        ops.segment_sum([Dj], self._pl('embT_indptr'), self._pl('embT_idx'), G['token_encoder/Embed_0/embedding'])
        ops.segment_sum([Dj], self._pl('audT_indptr'), self._pl('audT_idx'), self.audio.d_seq)
        ops.segment_sum([Dj], self.visT[0], self.visT[1], self.vision.d_seq)

    def loss_info(self):
        return self.info_from(self.loss_acc.tolist())

    @staticmethod
    def info_from(la):
        """The dict of loss_info() from a host copy of loss_acc (also the rows of the finetuning driver's metrics ring)."""
        return {'loss': la[0] + la[2], 'is_right_audio': la[1], 'is_right_text': la[3], 'loss_audio': la[0], 'loss_text': la[2]}


# ------------------------------------------------------------------------------------------------ reference-named API
class MerlotReserveTVQA(MerlotReserveVCR):
    """F:157-258.  The model object of finetune.MerlotReserveVCR (parameter store, engine, communicator, optional moment shards) with
    the TVQA engine and parameter tree: construct_finetuning_train_state / finetune_train_step / FinetuneTrainState take it as it is."""
    engine_cls = TVQAEngine
    param_specs = staticmethod(tvqa_param_specs)

    def _load(self, variables):
        if variables is None:
            return
        assert not self._shared_store, 'this forward-only view reads another model\'s parameters: load them there'
        tree = variables['params'] if 'params' in variables else variables
        if tree is not self._last_tree:
            # a pretrained tree still holds head / span_encoder (popped at F:269-270) and contrastive_scales -- they are not read --
            # and has no proj yet (F:272): the initialised one stays
            load = tree if 'proj' in tree else dict(tree, proj={'kernel': self.params_store.master_tree()['proj']['kernel']})
            self.params_store.load_tree(load)
            self._last_tree = tree


def train_loss_fn(state, params, batch):
    """F:277-294: forward + the two cross-entropies; returns (loss, the four metrics) as host floats."""
    model = state._model
    model.apply(None if params is None else {'params': params}, batch)
    model.engine.loss_and_grad_logits()
    info = model.engine.loss_info()
    return info.pop('loss'), info


def pred_step(state_or_model, batch):
    """F:300-310: host arithmetic on the 2 B A logits.  Takes a train state, or a model (a forward-only one included)."""
    la, lt = _model_of(state_or_model).apply(None, batch)
    la, lt = la.float().cpu(), lt.float().cpu()
    out = {'logprobs_audio': torch.log_softmax(la, -1), 'preds_audio': torch.argmax(la, -1),
           'logprobs_text': torch.log_softmax(lt, -1), 'preds_text': torch.argmax(lt, -1)}
    out['preds_joint'] = torch.argmax(torch.softmax(la, -1) + torch.softmax(lt, -1), -1)
    return out


class TVQAGraphStep(FinetuneGraphStep):
    """The captured TVQA step: per batch the frames, the audio clips, the labels, the plan and the step's four scalars are copied."""


def make_tvqa_batch(config, B, seed=0, device='cpu'):
    """Synthetic TVQA batch with the structure of finetune/common_dataloader.py:184-212.  Per answer: the option tokens (question +
    choice) and MASK in segment 0, then per frame k (segment k + 1) its 3 * audio_token_length AUDIOSPAN tokens in the audio stream
    and its subtitle tokens in the text stream, truncated to T and PAD-filled.  The last mel column of audio_clips is 1 (:242-244)."""
    d = TVQADims(config, B)
    rng = np.random.default_rng(seed)
    streams = {k: np.zeros((B, d.A, d.T, 2), dtype=np.int32) for k in ('audio_seqs', 'textonly_seqs')}
    for b in range(B):
        query = rng.integers(10, VOCAB, size=int(rng.integers(2, max(3, d.T // 8))))
        subs = [rng.integers(10, VOCAB, size=int(rng.integers(0, max(2, d.T // (2 * d.nseg))))) for _ in range(d.nseg)]
        for a in range(d.A):
            option = np.concatenate([query, rng.integers(10, VOCAB, size=int(rng.integers(1, max(2, d.T // 8))))])[:d.T - 1]
            option = np.concatenate([option, [MASK]])
            for name, per_seg in (('audio_seqs', [np.full(d.nas * d.a_tok, AUDIOSPAN)] * d.nseg), ('textonly_seqs', subs)):
                rows = [option] + list(per_seg)
                toks = np.concatenate(rows)[:d.T]
                segs = np.concatenate([np.full(len(r), i) for i, r in enumerate(rows)])[:d.T]
                streams[name][b, a, :len(toks), 0] = toks
                streams[name][b, a, :len(toks), 1] = segs
    g = torch.Generator().manual_seed(seed)
    audio = torch.rand(B, d.nseg, d.nas, d.a_raw, 65, generator=g)
    audio[..., -1] = 1.0
    return {'images': torch.rand(B, d.nseg, d.hw, d.pp3, generator=g).to(torch.bfloat16).to(device),
            'audio_clips': audio.to(torch.bfloat16).to(device), **streams, 'labels': rng.integers(0, d.A, size=B).astype(np.int32)}
