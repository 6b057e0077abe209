"""Device program of one pretraining step: MerlotReservePretrainer.__call__ (pretrain/pretrain_model.py:38-259),
loss_fn_given_preds (:262-303) and their hand-written backward, as a fixed sequence of C-ABI kernel launches over
buffers allocated once (all shapes are static given config and B, so the whole step can be captured in a hipGraph).

Data layout in HBM (bf16 unless noted; M = sequences x positions of a tower):
  per tower and layer, kept for backward: X[l] layer input, ln1, qkv (post "rotary"), att, lse (fp32), xmid, ln2,
  hpre, hact  = 16 H bf16 / token / layer;  LN statistics fp32.
  joint input is ASSEMBLED by one index-driven gather from [token embedding | pooled audio | pooled vision] rows;
  the [S,S] attention mask never exists (one int32 code per position); the "rotary" is a [positions, 32] fp32 table.
"""
import math
import os

import numpy as np
import torch

from . import ops
from .config import Dims
from .planner import VOCAB, audio_tables, build_plan, span_rot_table, vit_tables
from .towers import BF16, F32, I32, PooledTower, TowerState, cls_view, encoder_forward, layer_names


def side_stream_disabled():
    """MR_NO_SIDE_STREAM=1, read when the work is issued (bench.py sets and clears it between steps of one process for its exclusive
    timing pass): the side stream's work is issued in line on the current stream."""
    return os.environ.get('MR_NO_SIDE_STREAM') == '1'


class TowerEngine:
    """What every program built from TransformerEncoder towers shares (pretraining step, VCR finetuning step): the
    encoder forward (towers.encoder_forward) / hand-written backward over a TowerState, the backward stages of the vision / audio
    input towers (towers.PooledTower), the two scratch sets (main / side stream) and the device copies of the per-batch plan.
    Subclasses set: self.p (ParamStore), self.W / self.G (weight / gradient views), self.dev, self.dtype, self.fwd_only, self.side_stream,
    self.vision / self.audio (the PooledTowers the program has; self.tv / self.ta name their TowerStates),
    self.sc_main / self.sc_side / self.cur (via _make_scratch), self.plan_dev / _plan_caps / _plan_views / plan_frozen."""

    def _make_scratch(self, Ms, Gs, Ps, H, nh):
        dev = self.dev
        z = lambda *s: torch.zeros(*s, dtype=self.dtype, device=dev)
        f = lambda *s: torch.zeros(*s, dtype=F32, device=dev)
        f32 = self.dtype == F32
        # fp32 program (use_bfloat16_grads = False): the reductions are immediate, a LayerNorm backward wants 2 floats per row
        ln_ws_shared = f(2 * Ms) if f32 else None
        ln_ws = (lambda: ln_ws_shared) if f32 else (lambda: ops.layernorm_bwd_workspace(H, dev))

        class Scratch:
            pass
        sc = Scratch()
        sc.T_a = z(Ms, H)
        # the weight gradients of up to WG layers share one launch (encoder_backward / _wgrad_group), so a layer's upstream gradients
        # (d qkv, d pre-activation, and the two [M, H] gradients of its residual stream) stay alive while the next layers' are produced:
        # WG sets of T_q / T_h, 2 WG [M, H] buffers (the caller's D joins their rotation)
        WG = self._wgrad_group(Ms, H)
        sc.T_qs, sc.T_hs = [z(Ms, 3 * H) for _ in range(WG)], [z(Ms, 4 * H) for _ in range(WG)]
        sc.T_ds = [z(Ms, H) for _ in range(2 * WG)]
        sc.WG = WG
        sc.delta = f(Ms * nh)
        sc.gemm_ws = f(32 * 1024 * 1024)                       # 128 MiB of fp32 split-K partials
        sc.ln_ws = ln_ws()
        sc.cs_ws = ops.colsum_workspace(4 * H, dev)
        # A layer's four deferred reductions (2 LayerNorm, 2 bias) keep their partial rows until ONE mr_reduce_partials launch per
        # weight-gradient GROUP of layers (engine._wgrad_group: 2 base, 4 large) -- the gradients are not needed before the group's
        # layer_done: one set of partial-row workspaces per position in the group
        sc.ln_wsA = [ln_ws() for _ in range(WG)]
        sc.ln_wsB = [ln_ws() for _ in range(WG)]
        sc.cs_wsA = [ops.colsum_workspace(4 * H, dev) for _ in range(WG)]
        sc.cs_wsB = [ops.colsum_workspace(4 * H, dev) for _ in range(WG)]
        # per-(tile, wave) column-sum partials written by the d(pre-activation) GEMM's epilogue (the fc1 bias gradient)
        sc.cs_fused = [f(4 * ((Ms + 255) // 256) * 4 * H) for _ in range(WG)]
        # per-(sequence, block) column-sum partials written by the attention backward kernels (the qkv bias gradient): at most
        # one row per 16 positions (short sequences) of [3H]
        sc.cs_attn = [f(((Ms + 15) // 16 + 64) * 3 * H) for _ in range(WG)]
        # tower-level reductions (pre / final LayerNorm, pooling and projection biases) keep their partial rows in these until
        # the tower's ONE mr_reduce_partials launch (they used to be two latency-bound launches each)
        sc.tower_ln_ws = [ln_ws() for _ in range(2)]
        sc.tower_cs_ws = [ops.colsum_workspace(H, dev) for _ in range(6)]
        sc.d_pool_q, sc.d_pool_po, sc.d_pool_qin = z(Gs, H), z(Gs, H), z(Gs, H)
        sc.Dpatch = z(Ps, H)
        return sc

    # GEMMs of this engine: split-K partials go to the scratch set being issued on (`self.cur`: main / side stream), which
    # belongs to THIS engine -- no module-level workspace (two engines, or a captured graph and a later engine, never share)
    def gemm(self, a, b, out, **kw):
        return ops.gemm(a, b, out, ws=None if self.cur is None else self.cur.gemm_ws, **kw)

    def fgemm(self, a, name, out, **kw):
        """Forward Dense: out = a @ W[name].  The bf16 program reads the TRANSPOSED working copy where the store keeps one
        (params.ParamStore.wT): both operands contraction-contiguous, the fast GEMM path; same values, same result."""
        b, transB = self._fweight(name)
        return self.gemm(a, b, out, transB=transB, **kw)

    def _fweight(self, name):
        wT = getattr(self.p, 'wT', None) if self.dtype == BF16 else None
        return (wT[name], True) if wT and name in wT else (self.W[name], False)

    def gemm_args(self, a, b, out, **kw):
        return ops.gemm_args(a, b, out, ws=None if self.cur is None else self.cur.gemm_ws, **kw)

    def fgemm_grouped(self, items):
        """Several independent forward Dense layers [(a, weight name, out, kwargs)] in one mr_gemm_grouped call (small problems of one
        operand layout share a launch; anything else falls back to one launch each inside the library)."""
        if self.dtype != BF16:
            for a, name, out, kw in items:
                self.fgemm(a, name, out, **kw)
            return
        args = []
        for a, name, out, kw in items:
            b, transB = self._fweight(name)
            args.append(self.gemm_args(a, b, out, transB=transB, **kw))
        ops.gemm_grouped(args)

    # tower-level deferred reductions: between _begin_tower_reductions() and _flush_tower_reductions() every LayerNorm /
    # colsum issued through _t_ln_bwd / _t_colsum leaves its partial rows in a workspace of its own
    def _begin_tower_reductions(self):
        return {'jobs': None if self.dtype == F32 else [], 'ln': 0, 'cs': 0, 'sc': self.cur}      # (fp32: immediate)

    def _t_ln_bwd(self, tr, *a, **k):
        if tr is None or tr['jobs'] is None:
            return ops.layernorm_bwd(*a, self.cur.ln_ws, **k)
        ws = tr['sc'].tower_ln_ws[tr['ln']]
        tr['ln'] += 1
        return ops.layernorm_bwd(*a, ws, jobs=tr['jobs'], **k)

    def _t_colsum(self, tr, x, out):
        if tr is None or tr['jobs'] is None:
            return ops.colsum(x, out, self.cur.cs_ws)
        ws = tr['sc'].tower_cs_ws[tr['cs']]
        tr['cs'] += 1
        return ops.colsum(x, out, ws, jobs=tr['jobs'])

    def _flush_tower_reductions(self, tr):
        if tr is not None and tr['jobs']:
            ops.reduce_partials(tr['jobs'])          # (clears the list)

    def _on_side(self, fn):
        """Issue fn()'s kernels on the side stream (forked from / joined to the current stream by the caller)."""
        if not self.fwd_only:
            self.cur = self.sc_side
        try:
            if side_stream_disabled():       # same work, issued in line
                return fn()
            with torch.cuda.stream(self.side_stream):
                return fn()
        finally:
            if not self.fwd_only:
                self.cur = self.sc_main

    # ------------------------------------------------------------------------------------------ plan upload
    def set_plan(self, plan):
        """Copy the host plan into ONE persistent device buffer (same addresses every step: graph-capturable) through a ring
        of two pinned host buffers and ONE asynchronous H2D copy per step.  A pinned buffer is rewritten only after the copy
        that last read it has completed (an event per buffer), so the host may plan step t+1 while the GPU runs step t and
        the copy engine never reads memory the host has since reused.  (Pageable sources made every copy a staged,
        stream-serialising one.)"""
        arrs = {k: np.ascontiguousarray(v) for k, v in plan.items() if isinstance(v, np.ndarray)}
        need_layout = any(k not in self._plan_caps or a.nbytes > self._plan_caps[k] for k, a in arrs.items())
        if need_layout:
            assert not self.plan_frozen, 'plan buffers would be reallocated after graph capture'
            # index lists are bounded by the number of joint + span positions; everything else has a fixed size
            off = 0
            self._plan_off, self._plan_caps = {}, {}
            for k, a in arrs.items():
                cap = max(self._idx_capacity() * a.itemsize if k.endswith('_idx') else a.nbytes, a.nbytes)
                cap = (cap + 255) // 256 * 256
                self._plan_off[k], self._plan_caps[k] = off, cap
                off += cap
            self.plan_dev = torch.zeros(off, dtype=torch.uint8, device=self.dev)
            pin = self.dev.type == 'cuda'
            self._plan_host = [torch.zeros(off, dtype=torch.uint8, pin_memory=pin) for _ in range(2)]
            self._plan_ev = [None, None]
            self._plan_turn = 0
        i = self._plan_turn
        self._plan_turn ^= 1
        if self._plan_ev[i] is not None:
            self._plan_ev[i].synchronize()
        host = self._plan_host[i].numpy()
        for k, a in arrs.items():
            o = self._plan_off[k]
            host[o:o + a.nbytes] = a.reshape(-1).view(np.uint8)
        self.plan_dev.copy_(self._plan_host[i], non_blocking=True)
        if self.dev.type == 'cuda':
            self._plan_ev[i] = torch.cuda.Event()
            self._plan_ev[i].record()
        for k, a in arrs.items():
            o = self._plan_off[k]
            self._plan_views[k] = self.plan_dev[o:o + a.nbytes].view(torch.from_numpy(a[:0].reshape(-1)).dtype).view(a.shape)
        self.plan = plan

    def _pl(self, k):
        return self._plan_views[k]

    def _joint_rot(self):
        """The joint tower's "rotary" table of the current plan, or None when the config drops the coordinates (do_rotary = False)."""
        return self._pl('joint_rot') if self.d.do_rotary else None

    def _idx_capacity(self):
        """Upper bound on the length of any index list of the plan (so the buffers never move after capture)."""
        return self.tj.M + self.ts.M + 64

    # ------------------------------------------------------------------------------------------ encoder
    encoder_forward = encoder_forward       # (towers.py; the engine is its `eng`)

    def _wgrad_group(self, M, H):
        """Layers whose weight gradients share one grouped launch of the one-tile-per-workgroup TN kernel (csrc/gemm3.hip): the count
        (<= 4) whose 256 x 256 output tiles fill the 256 CUs' rounds best, the smallest on a tie -- base model: 108 tiles per layer ->
        2 layers = 216 (one round at 84 %; 3 or 4 layers are no better); large: 192 per layer -> 4 layers = 768 = three full rounds
        (one layer per launch left a quarter of the chip idle: 24 rounds per tower instead of 18).  K = M tokens must be long
        enough to amortise a tile's prologue."""
        if M < 2048:
            return 1
        t = lambda m, n: ((m + 255) // 256) * ((n + 255) // 256)
        tiles = t(4 * H, H) + t(H, 4 * H) + t(H, H) + t(H, 3 * H)
        eff = lambda n: n / (((n + 255) // 256) * 256)
        best = 1
        for g in range(2, 5):
            if eff(g * tiles) > eff(best * tiles) + 0.05:
                best = g
        return best

    def encoder_backward(self, st, prefix, rot, code, D, layer_done=None, tr=None, extra_wgrads=None, dense_mask=None):
        """D [M,H]: gradient wrt st.xf.  Returns the buffer holding the gradient wrt st.xin (D or one of the scratch
        buffers that rotate through the layers).  Weight gradients go to the flat grad buffer; the four weight
        gradients of a layer -- of TWO layers when that fills the chip better (_wgrad_group) -- are deferred to ONE grouped
        GEMM launch (no split-K).
        layer_done(l): called once every parameter gradient of layers >= l is final on the issuing stream (the data-parallel
        trainer reduces gradient buckets from there while backward continues).
        extra_wgrads: [(x, dy, out)] weight gradients of the tower's head over the SAME tokens (attention-pool key / value
        projections, the joint head): they join the FIRST group's launch when its tiles still fit the same number of CU rounds
        (base: 216 + 9 per extra of 256) -- alone each is a 9-tile split-K launch of ~65 us --, else they are launched here."""
        W, G, H, nh, M = self.W, self.G, st.H, st.H // 64, st.M
        T_a = self.cur.T_a[:M]
        # [M, H] gradient buffers: a layer reads Dcur, writes Dmid and Dnext; Dcur / Dmid (and the layer's T_q / T_h) stay untouched
        # until the group's weight gradients have been issued
        group = min(self._wgrad_group(M, H), len(self.cur.T_qs))
        T_qs, T_hs = [t[:M] for t in self.cur.T_qs], [t[:M] for t in self.cur.T_hs]
        free = [t[:M] for t in self.cur.T_ds[:2 * group]]
        Dcur = D
        pending, held, done_layers = [], [], []
        if extra_wgrads:
            t256 = lambda m, n: ((m + 255) // 256) * ((n + 255) // 256)
            tiles = group * (t256(4 * H, H) + t256(H, 4 * H) + t256(H, H) + t256(H, 3 * H))
            extra = sum(t256(x.shape[1], dy.shape[1]) for x, dy, _ in extra_wgrads)
            rounds = lambda n: (n + 255) // 256
            if M >= 2048 and 4 * group + len(extra_wgrads) <= 20 and rounds(tiles + extra) == rounds(tiles):
                pending += [self.gemm_args(x, dy, out, transA=True) for x, dy, out in extra_wgrads]
            else:
                for x, dy, out in extra_wgrads:
                    self.gemm(x, dy, out, transA=True)
        k = 2 * st.L + 1
        self._t_ln_bwd(tr, Dcur, st.X[st.L], W[f'{prefix}/final_ln/scale'], st.stats[k, 0], st.stats[k, 1], Dcur,
                       G[f'{prefix}/final_ln/scale'], G[f'{prefix}/final_ln/bias'])
        # everything above the layers (heads, pooling, final LayerNorm) is reduced here: a data-parallel trainer hands the
        # tower's LAST layers' gradient bucket -- which holds these leaves -- to the all-reduce at the first layer_done
        self._flush_tower_reductions(tr)
        jobs = None if self.dtype == F32 else []      # (fp32: immediate reductions)
        for l in reversed(range(st.L)):
            n = layer_names(prefix, l)
            T_q, T_h = T_qs[len(done_layers)], T_hs[len(done_layers)]
            Dmid, Dnext = free.pop(), free.pop()
            gi = len(done_layers)               # position in the weight-gradient group: its own partial-row workspaces
            fused_bb1 = ops.gemm_colsum_job(Dcur, W[n['w2']], T_h, self.cur.cs_fused[gi], G[n['bb1']], jobs, transB=True,
                                            aux=st.hpre[l], ws=self.cur.gemm_ws)            # d hpre (+ its column sums = d bias)
            self.gemm(T_h, W[n['w1']], T_a, transB=True)                                    # d ln2
            ops.layernorm_bwd(T_a, st.xmid[l], W[n['g2']], st.stats[2 + 2 * l, 0], st.stats[2 + 2 * l, 1], Dmid,
                              G[n['g2']], G[n['b2']], self.cur.ln_wsA[gi], dx_add=Dcur, jobs=jobs)    # Dmid = d xmid
            self.gemm(Dmid, W[n['wo']], T_a, transB=True)                                   # d att
            fuse_q = jobs is not None and dense_mask is None
            if dense_mask is not None:       # any mask (the forward ran mr_attention_fwd_dense_mask): the plain backward pair; d bias = a column-sum pass below
                ops.attention_bwd_dense_mask(st.qkv[l], dense_mask, T_a, T_q, rot, st.nseq, st.S, nh)
            else:
                ops.attention_bwd(st.qkv[l], code, st.att[l], T_a, st.lse[l], self.cur.delta, T_q, rot, st.nseq, st.S, nh,
                                  colsum_ws=self.cur.cs_attn[gi], bias_grad=G[n['bqkv']], jobs=jobs if fuse_q else None)   # (+ column sums of T_q = d bias)
            if not fused_bb1:
                ops.colsum(T_h, G[n['bb1']], self.cur.cs_wsA[gi], jobs=jobs)
            if not fuse_q:
                ops.colsum(T_q, G[n['bqkv']], self.cur.cs_wsB[gi], jobs=jobs)
            self.gemm(T_q, W[n['wqkv']], T_a, transB=True)                                  # d ln1
            pending += [self.gemm_args(st.hact[l], Dcur, G[n['w2']], transA=True),
                        self.gemm_args(st.ln2[l], T_h, G[n['w1']], transA=True),
                        self.gemm_args(st.att[l], Dmid, G[n['wo']], transA=True),
                        self.gemm_args(st.ln1[l], T_q, G[n['wqkv']], transA=True)]
            held += [Dcur, Dmid]          # (the caller's D joins the rotation once its layer's weight gradients are issued)
            done_layers.append(l)
            ops.layernorm_bwd(T_a, st.X[l], W[n['g1']], st.stats[1 + 2 * l, 0], st.stats[1 + 2 * l, 1], Dnext,
                              G[n['g1']], G[n['b1']], self.cur.ln_wsB[gi], dx_add=Dmid, jobs=jobs)   # Dnext = d X[l]
            if len(done_layers) == group or l == 0:
                if jobs is not None:
                    ops.reduce_partials(jobs)      # the group's 2 LayerNorm + 2 bias gradients per layer: one launch (<= 16 jobs)
                ops.gemm_grouped(pending)
                free += held
                if layer_done is not None:
                    for dl in done_layers:
                        layer_done(dl)
                pending, held, done_layers = [], [], []
            Dcur = Dnext
        self._t_ln_bwd(tr, Dcur, st.xin, W[f'{prefix}/pre_ln/scale'], st.stats[0, 0], st.stats[0, 1], Dcur,
                       G[f'{prefix}/pre_ln/scale'], G[f'{prefix}/pre_ln/bias'])
        return Dcur

    # ------------------------------------------------------------------------------------------ input-tower backward stages
    def backward_stage_audio(self):
        self.audio.backward(self)

    def backward_stage_vision(self, layer_done=None):
        self.vision.backward(self, layer_done)


class PretrainEngine(TowerEngine):
    def __init__(self, config, B, params, device, rank=0, world=1, dtype=BF16, train=None):
        """dtype = torch.float32 builds the fp32 program on the fp32 master weights through the mr_f32_* kernels (the reference's
        use_bfloat16 = False arithmetic): forward + loss only by default (the 1e-3 forward-parity check); with train=True also the
        backward, gradients in fp32 (params.grad32) -- the reference's use_bfloat16_grads = False step (pretrain_model.py:323-333), a
        plain correctness path (no fused reductions, no grouped launches).  The default bf16 program is the fast training path."""
        self.config, self.p, self.dev = config, params, torch.device(device)
        self.d = d = Dims(config, B)
        self.rank, self.world = rank, world
        self.dtype = dtype
        train = dtype == BF16 if train is None else train
        self.fwd_only = not train
        self.W = params.w if dtype == BF16 else params.wm
        if train and dtype == F32:
            params.enable_f32_grads()
        self.G = params.g if dtype == BF16 else getattr(params, 'g32', None)
        hp = train
        dev, H = self.dev, d.H
        self.tables = {'span_rot': torch.as_tensor(span_rot_table(d.span_len)).to(dev)}
        z = lambda *s: torch.zeros(*s, dtype=dtype, device=dev)
        f = lambda *s: torch.zeros(*s, dtype=F32, device=dev)

        # vision tower (modeling.py:379-430) and audio tower (:433-476), each with its CLS head and attention pool
        self.vision = PooledTower('vision_encoder', d.Nv, d.hw, d.pp3, d.Lv, H, vit_tables(d.gh, d.gw, d.pr, d.Nv), dev, dtype, train, keep_hpre=hp)
        self.audio = PooledTower('audio_encoder', d.Na, d.a_len, d.a_patch * 65, d.La, H, audio_tables(d.a_len, d.a_pool, d.Na), dev, dtype, train,
                                 pad_input=True, keep_hpre=hp)
        self.tv, self.ta = self.vision.st, self.audio.st
        self.tj = TowerState(d.Nj * d.Sj, H, d.Lj, d.Nj, d.Sj, dev, dtype, hp)
        if not d.do_rotary:                 # d pe: position p sums rows p, Sj + p, 2 Sj + p, ... of the tower-input gradient (a static segment list)
            idx = (np.arange(d.Nj)[None, :] * d.Sj + np.arange(d.Sj)[:, None]).reshape(-1).astype(np.int32)
            self.pe_lists = (torch.as_tensor(np.arange(d.Sj + 1, dtype=np.int32) * d.Nj).to(dev), torch.as_tensor(idx).to(dev))
        self.ts = TowerState(d.Ns * d.Ss, H, d.Ls, d.Ns, d.Ss, dev, dtype, hp)
        Mmax = max(t.M for t in (self.tv, self.ta, self.tj, self.ts))

        self.hj = z(self.tj.M, H)
        self.s_cls = z(d.Ns, H)

        # contrastive sections (rows per rank), order of the packed buffer E
        n_i2a, n_t2a, n_ext, n_s2s = B * d.nseg, B * d.ntrg, B * (d.nspans - d.ntrg), B * d.n_inc
        self.sec = {}
        off = 0
        for name, n in (('i2a_x', n_i2a), ('i2a_y', n_i2a), ('t2a_x', n_t2a), ('t2a_y', n_t2a), ('t2a_ye', n_ext),
                        ('s2s_x', n_s2s), ('s2s_y', n_s2s)):
            self.sec[name] = (off, n)
            off += n
        self.R = off
        self.n_pool = n_i2a + n_t2a + n_s2s
        self.Xpool = z(self.n_pool, H)
        self.acls_g = z(d.Na, H)
        self.E, self.dE = z(self.R, H), z(self.R, H)
        self.inv_norm = f(self.R)
        self.loss_acc = f(3)
        self.diag = f(2, 6)
        self.dls = f(3)
        self.dls_part = f(((self.R + 3) // 4 if dtype == BF16 else self.R) + 8)
        # objectives: (name, x section, y sections (gathered across ranks), scale index)
        self.objectives = [('imgs_to_audio', 'i2a_x', ('i2a_y',), 0), ('text_to_audio', 't2a_x', ('t2a_y', 't2a_ye'), 1),
                           ('stuff_to_span', 's2s_x', ('s2s_y',), 2)]
        # One contrastive problem per (objective, direction) (P:276-295): queries = a local section, keys = the matching
        # section(s) of EVERY rank, rank-major (all_gather(...).reshape(-1, H), P:290).  The gathered embeddings E_all
        # [world, R, H] are re-packed once per step into Kcat, where each problem's keys are contiguous rows (so logits,
        # d(query) and d(key) are ONE GEMM each for any world size) and appear twice, for the hi / lo split of dL/dlogits:
        #   rows [kb, kb + ldv): key c of the problem at row kb + c (zero rows for c >= V = world * nk), [kb + ldv, kb + 2 ldv): again.
        self.cprob = []
        kb = 0
        for oi, (name, xs, ys, _) in enumerate(self.objectives):
            xo, nx = self.sec[xs]
            yo, ny, ny0 = self.sec[ys[0]][0], sum(self.sec[y][1] for y in ys), self.sec[ys[0]][1]
            for di, (q_off, Lq, k_off, nk) in enumerate(((xo, nx, yo, ny), (yo, ny0, xo, nx))):
                V = world * nk
                ldv = (V + 7) // 8 * 8
                self.cprob.append(dict(oi=oi, di=di, name=name, q_off=q_off, Lq=Lq, k_off=k_off, nk=nk, V=V, ldv=ldv, kb=kb,
                                       logits=f(Lq, ldv), dl=None if self.fwd_only or dtype == F32 else z(Lq, 2 * ldv)))
                kb += 2 * ldv
        self.Kcat = z(kb, H)
        self.lse_rows = f(max(p['Lq'] for p in self.cprob))
        # static index lists of the re-pack (a gather from E_all's rows) and of its transpose (dE_all row <- DK hi + lo rows)
        ip, ix = [0], []
        src_of = {}
        for p in self.cprob:
            for half in range(2):
                for c in range(p['ldv']):
                    if c < p['V']:
                        r, j = divmod(c, p['nk'])
                        ix.append(r * self.R + p['k_off'] + j)
                        if half == 0:
                            src_of[r * self.R + p['k_off'] + j] = (p['kb'] + c, p['kb'] + p['ldv'] + c)
                    ip.append(len(ix))
        self.kpack = (torch.tensor(ip, dtype=I32, device=dev), torch.tensor(ix if ix else [0], dtype=I32, device=dev))
        assert sorted(src_of) == list(range(world * self.R)), 'every gathered row is a key of exactly one problem'
        if not self.fwd_only:
            self.DK = z(kb, H)
            self.dE_keys = z(self.R, H) if dtype == F32 and world == 1 else None
            self.kunpack = (torch.arange(0, 2 * world * self.R + 1, 2, dtype=I32, device=dev),
                            torch.tensor([v for e in range(world * self.R) for v in src_of[e]], dtype=I32, device=dev))

        self.side_stream = torch.cuda.Stream(device=dev) if dev.type == 'cuda' else None
        self.plan_dev, self._plan_caps, self._plan_views, self.plan_frozen = None, {}, {}, False
        self.cur = None
        if self.fwd_only:
            return
        # backward scratch
        self.Dj, self.Ds = z(self.tj.M, H), z(self.ts.M, H)
        self.d_s_cls = z(d.Ns, H)
        # Two scratch sets: the audio tower runs on a side stream concurrently with the vision tower (forward and
        # backward), so that one tower's kernels fill the CUs the other leaves idle (partial last rounds of the
        # persistent GEMMs, small kernels).  `self.cur` is the set the ops being ISSUED right now may use.
        Gv, Ga = d.Nv * d.hw4, d.Na * d.a_tok
        self.sc_main = self._make_scratch(Mmax, max(Gv, Ga), max(d.Nv * d.hw, d.Na * d.a_len), H, d.nh)   # also serves audio when issued in line
        self.sc_side = self._make_scratch(self.ta.M, Ga, d.Na * d.a_len, H, d.nh)
        self.cur = self.sc_main
        self.dXpool = z(self.n_pool, H)
        self.d_hj = z(self.tj.M, H)
        self.d_acls_g = z(d.Na, H)

        # (device copies of the per-batch plan -- plan_dev / _plan_caps / _plan_views, set above -- have fixed sizes where
        # possible; index lists are padded to capacity)

    # ------------------------------------------------------------------------------------------ forward
    def forward(self, batch, plan=None, draws=None):
        """batch: dict of synthetic.make_batch layout (images / audio_clips on device, integer streams numpy)."""
        d, W, H = self.d, self.p.w, self.d.H
        if plan is None:
            from .synthetic import make_draws
            splits, z = draws if draws is not None else make_draws(self.config, d.B, seed=int(batch['audio2text/text_ptr'].astype(np.uint32).sum() % (2 ** 31)))
            plan = build_plan(batch, d, splits, z)
        self.set_plan(plan)
        return self.forward_device(batch['images'], batch['audio_clips'])

    def forward_device(self, images, audio_clips):
        """Device part of forward(): the plan is already in its device buffers."""
        d, W, H = self.d, self.W, self.d.H
        if images.dtype != self.dtype:          # the wire format is bf16 (pretrain/dataloader.py:786-788); the fp32 program casts up, like the
            images, audio_clips = images.to(self.dtype), audio_clips.to(self.dtype)     # reference model's first op (M: x.astype(self.dtype))
        tj, ts = self.tj, self.ts
        # vision tower (main stream) and audio tower (side stream) are independent until the joint tower
        main = torch.cuda.current_stream()
        self.side_stream.wait_stream(main)
        self._on_side(lambda: self.audio.forward(self, audio_clips.reshape(d.Na * d.a_len, d.a_patch * 65)))
        self.vision.forward(self, images.reshape(d.Nv * d.hw, d.pp3))
        if d.no_vision:                  # pretrain/pretrain_model.py:61-63: imgs_seq *= 0.0 (the cls output still feeds the contrastive loss)
            self.vision.seq.zero_()
        main.wait_stream(self.side_stream)
        emb = W['token_encoder/Embed_0/embedding']

        def span_fwd():       # needs only the token table and the plan: runs beside the joint tower
            # span tower on the chosen spans (modeling.py:479-504)
            ops.segment_sum([emb], self._pl('span_gather_indptr'), self._pl('span_gather_idx'), ts.xin)
            ops.fill_rows(W['span_encoder/transformer/cls'], ts.xin, ts.nseq, ts.S, 0)
            self.encoder_forward(ts, 'span_encoder/transformer', self.tables['span_rot'], self._pl('span_code'))
            self.fgemm(cls_view(ts.xf, ts.nseq, ts.S), 'span_encoder/transformer/cls_proj/kernel', self.s_cls,
                     bias=W['span_encoder/transformer/cls_proj/bias'])
        self.side_stream.wait_stream(main)
        self._on_side(span_fwd)
        # joint tower: one gather assembles [token embeddings | audio spans | vision tokens | zero padding]
        ops.segment_sum([emb, self.audio.seq, self.vision.seq], self._pl('joint_gather_indptr'), self._pl('joint_gather_idx'), tj.xin)
        if not d.do_rotary:                # pretrain_model.py:146-148 + modeling.py:335-341: no coordinates, x += pe (every position, padding included)
            ops.add_rows_periodic(tj.xin, W['joint_transformer/pe'])          # one launch for all d.Nj sequences
        self.encoder_forward(tj, 'joint_transformer', self._joint_rot(), self._pl('joint_code'))
        self.fgemm(tj.xf, 'head/kernel', self.hj, bias=W['head/bias'])
        ops.segment_sum([self.hj], self._pl('pool_indptr'), self._pl('pool_idx'), self.Xpool)
        ops.segment_sum([self.audio.cls], self._pl('acls_indptr'), self._pl('acls_idx'), self.acls_g)
        main.wait_stream(self.side_stream)
        # unit-normalise * temperature into the packed buffer E (pretrain_model.py:239-257)
        for src, names, si in self._norm_sections():
            o, n = self.sec[names[0]][0], sum(self.sec[k][1] for k in names)
            ops.unit_norm_scale_fwd(src, W['contrastive_scales'][si:si + 1], self.E[o:o + n], self.inv_norm[o:o + n])
        return self.E

    def _norm_sections(self):
        n1, n2 = self.sec['i2a_x'][1], self.sec['t2a_x'][1]
        return [(self.Xpool[:n1], ('i2a_x',), 0), (self.vision.cls, ('i2a_y',), 0),
                (self.Xpool[n1:n1 + n2], ('t2a_x',), 1), (self.acls_g, ('t2a_y', 't2a_ye'), 1),
                (self.Xpool[n1 + n2:], ('s2s_x',), 2), (self.s_cls, ('s2s_y',), 2)]

    def outputs(self):
        """The reference's output dict (pretrain_model.py:240-244 after :246-257), views of E."""
        s = lambda k: self.E[self.sec[k][0]:self.sec[k][0] + self.sec[k][1]]
        return {'imgs_to_audio': {'x': s('i2a_x'), 'y': s('i2a_y')},
                'text_to_audio': {'x': s('t2a_x'), 'y': s('t2a_y'), 'y_extra': s('t2a_ye')},
                'stuff_to_span': {'x': s('s2s_x'), 'y': s('s2s_y'), '_sources': torch.as_tensor(self.plan['t2sp_src'])}}

    # ------------------------------------------------------------------------------------------ loss (+ its backward)
    def loss_and_grad_outputs(self, E_all=None, dE_all=None):
        """loss_fn_given_preds (pretrain_model.py:262-303) for this rank and dL/dE.
        world > 1: E_all [world,R,H] is the rank-major all-gather of every rank's E (:290); the gradient wrt this rank's
        queries goes to self.dE, the gradient wrt EVERY rank's keys to dE_all [world,R,H] (every row written), which the
        caller reduce-scatters (sum) and adds to self.dE before backward().  world == 1: both land in self.dE.
        Per (objective, direction): one logits GEMM, the fp32 LSE, and -- dL/dlogits split into bf16 hi + lo side by side so
        that the products keep 16 mantissa bits (its rows sum to zero) with fp32 accumulation over BOTH halves -- one GEMM
        for d(queries) and one for d(keys); 30 launches + 2 re-packs per step whatever the world size.
        Returns the fp32 device vector loss_acc[3] (per-objective losses of this rank)."""
        world, rank, H = self.world, self.rank, self.d.H
        if world == 1:
            E_all = self.E[None]
        else:
            assert E_all is not None and dE_all is not None and E_all.shape[0] == world
        ops.segment_sum([E_all.view(world * self.R, H)], self.kpack[0], self.kpack[1], self.Kcat)
        self.dE.zero_()
        self.loss_acc.zero_()
        self.diag.zero_()
        # The six (objective, direction) problems are independent: each of the three products runs as ONE grouped launch over all of
        # them (bf16 program; alone, every one of these 18 GEMMs is a 17-23 us latency chain of k-tiles on one or two workgroups).
        grouped = not self.fwd_only and self.dtype == BF16
        qs = [self.E[p['q_off']:p['q_off'] + p['Lq']] for p in self.cprob]
        if grouped:
            ops.gemm_grouped([self.gemm_args(q, self.Kcat[p['kb']:p['kb'] + p['V']], p['logits'], transB=True) for p, q in zip(self.cprob, qs)])
        for p, q in zip(self.cprob, qs):
            kb, V, ldv = p['kb'], p['V'], p['ldv']
            logits = p['logits']
            if not grouped:
                self.gemm(q, self.Kcat[kb:kb + V], logits, transB=True)               # rank-major columns (:290)
            is_s2s = p['name'] == 'stuff_to_span'
            ops.contrastive_lse(logits[:, :V], rank * p['nk'], 0.5 / p['Lq'], self._pl('t2sp_src') if is_s2s else None,
                                self.loss_acc[p['oi']:p['oi'] + 1], self.diag[p['di']] if is_s2s else None, self.lse_rows)
            if self.fwd_only:
                continue
            if self.dtype == F32:        # fp32 program: dL/dlogits (left in `logits` by the LSE kernel) feeds both products as it is; the
                dlf = logits[:, :V]      # "lo" rows of DK stay zero
                self.gemm(dlf, self.Kcat[kb:kb + V], self.dE[p['q_off']:p['q_off'] + p['Lq']])
                self.gemm(dlf, q, self.DK[kb:kb + V], transA=True)
                continue
            dl = p['dl']                                                           # [Lq, hi(ldv) | lo(ldv)]; pad columns stay 0
            ops.split_hilo_rows(logits[:, :V], dl[:, :V], dl[:, ldv:ldv + V])
            if not grouped:
                self.gemm(dl, self.Kcat[kb:kb + 2 * ldv], self.dE[p['q_off']:p['q_off'] + p['Lq']])     # d(query side) = dlogits . keys
                self.gemm(dl, q, self.DK[kb:kb + 2 * ldv], transA=True)               # d(key side)   = dlogits^T . queries (hi rows, lo rows)
        if grouped:
            ops.gemm_grouped([self.gemm_args(p['dl'], self.Kcat[p['kb']:p['kb'] + 2 * p['ldv']], self.dE[p['q_off']:p['q_off'] + p['Lq']])
                              for p in self.cprob])                                # d(query side) = dlogits . keys
            ops.gemm_grouped([self.gemm_args(p['dl'], q, self.DK[p['kb']:p['kb'] + 2 * p['ldv']], transA=True)
                              for p, q in zip(self.cprob, qs)])                    # d(key side)   = dlogits^T . queries (hi rows, lo rows)
        if not self.fwd_only:
            if world == 1 and self.dtype == F32:
                ops.segment_sum([self.DK], self.kunpack[0], self.kunpack[1], self.dE_keys)
                ops.add_(self.dE, self.dE_keys)
            elif world == 1:
                ops.segment_sum([self.DK], self.kunpack[0], self.kunpack[1], self.dE, accumulate=True)
            else:
                ops.segment_sum([self.DK], self.kunpack[0], self.kunpack[1], dE_all.view(world * self.R, H))
        return self.loss_acc

    # ------------------------------------------------------------------------------------------ backward
    def backward(self):
        assert not self.fwd_only, 'this program was built forward-only (PretrainEngine(..., train=True) for the fp32 backward)'
        self._backward()

    def _backward(self):
        """Backward of forward() given self.dE; fills self.p.grad (bf16, per rank, un-reduced).
        Three stages, in the order the flat gradient buffer is laid out (params.py), so that a data-parallel caller can
        all-reduce each finished range while the next stage runs: [scales, head, span, joint, token] -> audio -> vision."""
        self.backward_stage_joint()
        main = torch.cuda.current_stream()
        self.side_stream.wait_stream(main)
        self._on_side(self.backward_stage_audio)
        self.backward_stage_vision()
        main.wait_stream(self.side_stream)

    def backward_stage_joint(self):
        d, W, G, H = self.d, self.W, self.G, self.d.H
        tv, ta, tj, ts = self.tv, self.ta, self.tj, self.ts
        self.dls.zero_()
        n1, n2 = self.sec['i2a_x'][1], self.sec['t2a_x'][1]
        dsts = [self.dXpool[:n1], self.vision.d_cls, self.dXpool[n1:n1 + n2], self.d_acls_g, self.dXpool[n1 + n2:], self.d_s_cls]
        for (src, names, si), dst in zip(self._norm_sections(), dsts):
            o, n = self.sec[names[0]][0], sum(self.sec[k][1] for k in names)
            ops.unit_norm_scale_bwd(src, W['contrastive_scales'][si:si + 1], self.inv_norm[o:o + n], self.dE[o:o + n], dst,
                                    self.dls[si:si + 1], self.dls_part, accumulate=True)
        if self.dtype == F32:
            G['contrastive_scales'].copy_(self.dls)
        else:
            ops.cast_f32_to_bf16(self.dls, G['contrastive_scales'])

        def span_bwd():
            # span tower (only its cls output is used: gradient enters at the CLS rows)
            Ds = self.Ds
            Ds.zero_()
            tr = self._begin_tower_reductions()
            cls_in = cls_view(ts.xf, ts.nseq, ts.S)
            self._t_colsum(tr, self.d_s_cls, G['span_encoder/transformer/cls_proj/bias'])
            self.gemm(cls_in, self.d_s_cls, G['span_encoder/transformer/cls_proj/kernel'], transA=True)
            self.gemm(self.d_s_cls, W['span_encoder/transformer/cls_proj/kernel'], cls_view(Ds, ts.nseq, ts.S), transB=True)
            Ds = self.encoder_backward(ts, 'span_encoder/transformer', self.tables['span_rot'], self._pl('span_code'), Ds, tr=tr)
            self._flush_tower_reductions(tr)
            ops.sum_rows_strided(Ds, ts.nseq, ts.S, 0, G['span_encoder/transformer/cls'])
            if Ds.data_ptr() != self.Ds.data_ptr():            # the joint tower reuses the rotating scratch: keep a copy
                self.Ds.copy_(Ds)
                Ds = self.Ds

            return Ds
        main = torch.cuda.current_stream()
        self.side_stream.wait_stream(main)
        Ds = self._on_side(span_bwd)
        # joint tower
        ops.segment_sum([self.dXpool], self._pl('poolT_indptr'), self._pl('poolT_idx'), self.d_hj)
        trj = self._begin_tower_reductions()
        self._t_colsum(trj, self.d_hj, G['head/bias'])
        Dj = self.Dj
        self.gemm(self.d_hj, W['head/kernel'], Dj, transB=True)
        Dj = self.encoder_backward(tj, 'joint_transformer', self._joint_rot(), self._pl('joint_code'), Dj, tr=trj,
                                   extra_wgrads=[(tj.xf, self.d_hj, G['head/kernel'])])
        self._flush_tower_reductions(trj)
        if not d.do_rotary:                # d pe[p] = sum over the joint sequences of the tower-input gradient at position p
            ops.segment_sum([Dj], self.pe_lists[0], self.pe_lists[1], G['joint_transformer/pe'])
        main.wait_stream(self.side_stream)
        # scatter-adds of the joint / span inputs, as segment sums over the planner's inverted lists
        ops.segment_sum([Dj, Ds], self._pl('embT_indptr'), self._pl('embT_idx'), G['token_encoder/Embed_0/embedding'])
        ops.segment_sum([Dj], self._pl('audT_indptr'), self._pl('audT_idx'), self.audio.d_seq)
        ops.segment_sum([Dj], self._pl('visT_indptr'), self._pl('visT_idx'), self.vision.d_seq)
        if d.no_vision:                  # d(imgs_seq * 0) = 0
            self.vision.d_seq.zero_()
        ops.segment_sum([self.d_acls_g], self._pl('aclsT_indptr'), self._pl('aclsT_idx'), self.audio.d_cls)

    def loss_info(self):
        """Host dict like the reference's loss_info (pretrain_model.py:263-303) from the device accumulators."""
        return self.info_from(self.loss_acc.tolist(), self.diag.tolist())

    def info_from(self, la, dg):
        """The dict of loss_info() from host copies of loss_acc [3] and diag [2][6] (also the rows of the trainer's metrics ring)."""
        info = {k: la[i] for i, (k, *_r) in enumerate(self.objectives)}
        for i, t in enumerate(['text2audio', 'audio2text', 'random_text']):
            info[f'_stuff_to_span_from_{t}'] = sum(dg[di][i] / (dg[di][3 + i] + 1e-5) / 2.0 for di in range(2))
        info['loss'] = sum(la)
        return info
