"""The transformer tower, defined once for every program: the activations of one TransformerEncoder (TowerState), its forward body
(encoder_forward) and the CLS + attention-pool input tower of the vision / audio encoders (PooledTower: embedding -> encoder -> cls_proj
+ pool, forward and hand-written backward).

The launches are issued through an `eng` that supplies the weights and the GEMM entry points: W (name -> tensor), fgemm(a, weight name, out,
**epilogue) and fgemm_grouped([(a, weight name, out, epilogue)]) for a forward; for PooledTower.backward also what engine.TowerEngine has
(G, dtype, cur, gemm, gemm_args, encoder_backward, the tower-level reductions).  The training / evaluation programs pass their engine; the
inference API (modeling.py) passes a three-line adapter over its bound weights."""
import numpy as np
import torch

from . import ops

BF16, F32, I32 = torch.bfloat16, torch.float32, torch.int32


class _LayerRing:
    """buffers[l % len(buffers)] for every layer l: what a forward-only TowerState keeps in place of one buffer per layer."""

    def __init__(self, buffers):
        self.buffers = buffers

    def __getitem__(self, l):
        return self.buffers[l % len(self.buffers)]


class TowerState:
    """Saved activations of one TransformerEncoder (modeling.py:283-376) over M = nseq*S rows.
    saved=False (a forward-only program on ONE stream): nothing is kept for a backward -- every layer writes the same one layer's worth of
    buffers (the residual stream alternates between two), and hpre does not exist.
    percall=True (the inference API, which builds a state per call): forward-only over UNINITIALISED buffers (no memset per buffer per
    call), no LayerNorm statistics, lse only where the bf16 attention kernel writes one, one buffer for both LayerNorm outputs, the final
    LayerNorm writes the residual ring's free buffer; xin: the caller's tower input instead of a buffer of the state's own."""

    def __init__(self, M, H, L, nseq, S, dev, dtype=BF16, keep_hpre=None, saved=True, percall=False, xin=None):
        nh = H // 64
        new = torch.empty if percall else torch.zeros
        z = lambda *s: new(*s, dtype=dtype, device=dev)
        f = lambda *s: new(*s, dtype=F32, device=dev)
        self.M, self.H, self.L, self.nseq, self.S = M, H, L, nseq, S
        self.xin = z(M, H) if xin is None else xin
        self.stats = None if percall else f(2 * L + 2, 2, M)      # [ln index][mean|rstd][row]; index 0 = pre_ln, 1+2l / 2+2l = layer l, last = final
        if percall or not saved:
            self.X = _LayerRing([z(M, H), z(M, H)])
            self.ln1, self.xmid, self.att = (_LayerRing([z(M, H)]) for _ in range(3))
            self.ln2 = self.ln1 if percall else _LayerRing([z(M, H)])
            self.xf = self.X[L + 1] if percall else z(M, H)
            self.qkv, self.hact, self.hpre = _LayerRing([z(M, 3 * H)]), _LayerRing([z(M, 4 * H)]), None
            self.lse = _LayerRing([f(nseq, nh, S) if dtype == BF16 or not percall else None])
            return
        self.xf = z(M, H)
        self.X = z(L + 1, M, H)
        self.ln1, self.ln2, self.xmid, self.att = z(L, M, H), z(L, M, H), z(L, M, H), z(L, M, H)
        self.qkv = z(L, M, 3 * H)
        self.hact = z(L, M, 4 * H)
        keep_hpre = dtype == BF16 if keep_hpre is None else keep_hpre
        self.hpre = z(L, M, 4 * H) if keep_hpre else None           # gelu'(pre-activation), only kept for backward
        self.lse = f(L, nseq, nh, S)

    def ln_stats(self, i):
        """(mean, rstd) rows of LayerNorm i, or (None, None) where none are kept."""
        return (None, None) if self.stats is None else (self.stats[i, 0], self.stats[i, 1])


def layer_names(prefix, l):
    p = f'{prefix}/layer_{l:02d}'
    return dict(g1=f'{p}/pre_attn_ln/scale', b1=f'{p}/pre_attn_ln/bias', wqkv=f'{p}/attention_layer/qkv/kernel',
                bqkv=f'{p}/attention_layer/qkv/bias', wo=f'{p}/attention_layer/attn_proj/kernel',
                g2=f'{p}/pre_mlp_ln/scale', b2=f'{p}/pre_mlp_ln/bias', w1=f'{p}/mlp_layer/intermediate/kernel',
                bb1=f'{p}/mlp_layer/intermediate/bias', w2=f'{p}/mlp_layer/out/kernel')


def cls_view(t, nseq, S):
    """The CLS rows (row 0 of every sequence) of t [nseq * S, H] as a strided [nseq, H] view."""
    return t.view(nseq, S * t.shape[1])[:, :t.shape[1]]


def encoder_forward(eng, st, prefix, rot, code, dense_mask=None):
    """TransformerEncoder body (modeling.py:360-366) on st.xin (CLS row already in place) -> st.xf.
    dense_mask: uint8 [nseq, S, S] (!= 0 = allowed) -- ANY attention mask (modeling.py:303, 350-356) instead of the position codes; the
    attention then runs on the plain dense-mask kernels, forward here and backward in encoder_backward (round 6: a correctness path)."""
    W, H, nh = eng.W, st.H, st.H // 64
    ops.layernorm_fwd(st.xin, W[f'{prefix}/pre_ln/scale'], W[f'{prefix}/pre_ln/bias'], st.X[0], *st.ln_stats(0))
    for l in range(st.L):
        n = layer_names(prefix, l)
        x = st.X[l]
        ops.layernorm_fwd(x, W[n['g1']], W[n['b1']], st.ln1[l], *st.ln_stats(1 + 2 * l))
        eng.fgemm(st.ln1[l], n['wqkv'], st.qkv[l], bias=W[n['bqkv']], rot_tab=rot, rot_cols=2 * H)
        if dense_mask is not None:
            ops.attention_fwd_dense_mask(st.qkv[l], dense_mask, st.att[l], st.nseq, st.S, nh)
        else:
            ops.attention_fwd(st.qkv[l], code, st.att[l], st.lse[l], st.nseq, st.S, nh)
        eng.fgemm(st.att[l], n['wo'], st.xmid[l], residual=x)
        ops.layernorm_fwd(st.xmid[l], W[n['g2']], W[n['b2']], st.ln2[l], *st.ln_stats(2 + 2 * l))
        eng.fgemm(st.ln2[l], n['w1'], st.hact[l], bias=W[n['bb1']], act=ops.ACT_GELU, c2=None if st.hpre is None else st.hpre[l])
        eng.fgemm(st.hact[l], n['w2'], st.X[l + 1], residual=st.xmid[l])
    ops.layernorm_fwd(st.X[st.L], W[f'{prefix}/final_ln/scale'], W[f'{prefix}/final_ln/bias'], st.xf, *st.ln_stats(2 * st.L + 1))


class PooledTower:
    """One CLS + attention-pool input tower: VisionTransformer (modeling.py:379-430; name = 'vision_encoder') or AudioTransformer
    (:433-476; 'audio_encoder') on nseq sequences of n_in input rows [K] each.  It owns its TowerState (st), its static tables (rot: the
    "rotary" scales, pool_rows: the key rows of every pooled position), the buffers of its head -- outputs: seq [pooled positions, H] and
    cls [nseq, H] -- and, built with train=True, what its backward needs: the gradients wrt its outputs (d_seq, d_cls: the program
    writes them), D (wrt st.xf, then down the layers), d_k / d_v (whose CLS rows nothing writes: they stay zero) and the patch rows of
    the [nseq, S] grid.  pad_input: a bf16 tower copies its input into rows of a multiple of 8 columns (16-byte rows for the GEMM).
    **state: TowerState's keep_hpre / saved / percall."""

    def __init__(self, name, nseq, n_in, K, L, H, tables, dev, dtype=BF16, train=False, pad_input=False, **state):
        S = n_in + 1
        self.name, self.n_in, self.K = name, n_in, K
        self.st = TowerState(nseq * S, H, L, nseq, S, dev, dtype, **state)
        self.rot, self.pool_rows = (torch.as_tensor(t).to(dev) for t in tables)
        percall = state.get('percall', False)
        new = torch.empty if percall else torch.zeros
        z = lambda *s: new(*s, dtype=dtype, device=dev)
        G, M, npool = self.pool_rows.shape[0], self.st.M, self.pool_rows.shape[1]
        self.qin, self.q, self.po, self.seq = z(4, G, H)          # (buffers of one shape: one allocation, its rows handed out)
        self.k, self.v = z(2, M, H)
        self.probs = new(G, H // 64, npool, dtype=F32, device=dev) if dtype == BF16 or not percall else None
        self.cls = z(nseq, H)
        self.x_pad = z(nseq * n_in, (K + 7) // 8 * 8) if pad_input and dtype == BF16 else None
        self.x2d = None                               # the 2-D view of the last input (the embedding's weight gradient reads it)
        if train:
            self.D, self.d_k, self.d_v = z(3, M, H)
            self.d_seq, self.d_cls = z(G, H), z(nseq, H)
            # static gather lists: patch rows of the [nseq, S] grid without the CLS rows
            rows = (np.arange(nseq)[:, None] * S + 1 + np.arange(n_in)[None]).reshape(-1).astype(np.int32)
            self.unpad = (torch.as_tensor(np.arange(len(rows) + 1, dtype=np.int32)).to(dev), torch.as_tensor(rows).to(dev))

    def forward(self, eng, x):
        """x [nseq * n_in, K] -> self.seq, self.cls (and st.xf): the patch / hop embedding (the audio tower's stride-2 conv is a GEMM over
        2 consecutive hops = 130 inputs), CLS fill, encoder, cls_proj and the attention pool with a mean query (modeling.py:412-427, 464-472)."""
        st, W, p, nh = self.st, eng.W, self.name, self.st.H // 64
        t, pool = f'{p}/transformer', f'{p}/seq_attnpool'
        if self.x_pad is not None:
            ops.pad_cols(x, self.x_pad)
            x = self.x_pad[:, :self.K]
        self.x2d = x
        eng.fgemm(x, f'{p}/embedding/kernel', st.xin, bias=W[f'{p}/embedding/bias'], row_map=(self.n_in, st.S, 1))
        ops.fill_rows(W[f'{t}/cls'], st.xin, st.nseq, st.S, 0)
        encoder_forward(eng, st, t, self.rot, None)
        ops.rows_mean_fwd(st.xf, self.pool_rows, self.qin)
        # the CLS head and the pool's query projection are independent small GEMMs (64 / 1152 rows): handed over as a group -- ONE launch when both fall to
        # the small-problem kernel (tiny configs); at base / large size the 1152-row query projection is claimed by the few-tile kernel (gemm5_wanted, csrc/gemm_route.cpp)
        # and the library launches the two separately
        eng.fgemm_grouped([(cls_view(st.xf, st.nseq, st.S), f'{t}/cls_proj/kernel', self.cls, dict(bias=W[f'{t}/cls_proj/bias'])),
                           (self.qin, f'{pool}/query/kernel', self.q, dict(bias=W[f'{pool}/query/bias']))])
        eng.fgemm(st.xf, f'{pool}/key/kernel', self.k, bias=W[f'{pool}/key/bias'])
        eng.fgemm(st.xf, f'{pool}/value/kernel', self.v, bias=W[f'{pool}/value/bias'])
        ops.poolattn_fwd(self.q, self.k, self.v, self.pool_rows, self.po, self.probs, nh)
        eng.fgemm(self.po, f'{pool}/out/kernel', self.seq, bias=W[f'{pool}/out/bias'])

    def backward(self, eng, layer_done=None):
        """Backward of forward() given d_seq (gradient wrt the pooled sequence output) and d_cls (wrt the cls output), down to the embedding's
        parameters; layer_done: as in TowerEngine.encoder_backward."""
        st, W, G, p, nh = self.st, eng.W, eng.G, self.name, self.st.H // 64
        t, pool = f'{p}/transformer', f'{p}/seq_attnpool'
        Gn, D, d_k, d_v = self.qin.shape[0], self.D, self.d_k, self.d_v
        d_po, d_q, d_qin = eng.cur.d_pool_po[:Gn], eng.cur.d_pool_q[:Gn], eng.cur.d_pool_qin[:Gn]
        tr = eng._begin_tower_reductions()
        # the small weight gradients of the head (pool out / query projections, cls_proj: K = 1152 / 1152 / 64 rows) feed nothing in this
        # backward: they leave the chain of data gradients and run as ONE grouped launch at its end
        small_wgrads = []
        defer = eng.dtype == BF16

        def wgrad(x, dy, out):
            if defer:
                small_wgrads.append(eng.gemm_args(x, dy, out, transA=True))
            else:
                eng.gemm(x, dy, out, transA=True)
        eng._t_colsum(tr, self.d_seq, G[f'{pool}/out/bias'])
        wgrad(self.po, self.d_seq, G[f'{pool}/out/kernel'])
        eng.gemm(self.d_seq, W[f'{pool}/out/kernel'], d_po, transB=True)
        ops.poolattn_bwd(self.q, self.k, self.v, self.pool_rows, self.probs, d_po, d_q, d_k, d_v, nh)
        eng._t_colsum(tr, d_q, G[f'{pool}/query/bias'])
        wgrad(self.qin, d_q, G[f'{pool}/query/kernel'])
        eng.gemm(d_q, W[f'{pool}/query/kernel'], d_qin, transB=True)
        eng._t_colsum(tr, d_k, G[f'{pool}/key/bias'])
        eng.gemm(d_k, W[f'{pool}/key/kernel'], D, transB=True)
        eng._t_colsum(tr, d_v, G[f'{pool}/value/bias'])
        eng.gemm(d_v, W[f'{pool}/value/kernel'], D, transB=True, residual=D)
        # the key / value weight gradients (K = all M tokens) ride in the encoder's first grouped weight-gradient launch
        extra = [(st.xf, d_k, G[f'{pool}/key/kernel']), (st.xf, d_v, G[f'{pool}/value/kernel'])]
        ops.rows_mean_bwd(d_qin, self.pool_rows, D)
        # cls head
        eng._t_colsum(tr, self.d_cls, G[f'{t}/cls_proj/bias'])
        wgrad(cls_view(st.xf, st.nseq, st.S), self.d_cls, G[f'{t}/cls_proj/kernel'])
        Dc = cls_view(D, st.nseq, st.S)
        eng.gemm(self.d_cls, W[f'{t}/cls_proj/kernel'], Dc, transB=True, residual=Dc)
        if small_wgrads:
            ops.gemm_grouped(small_wgrads)
        D = eng.encoder_backward(st, t, self.rot, None, D, layer_done=layer_done, tr=tr, extra_wgrads=extra)
        ops.sum_rows_strided(D, st.nseq, st.S, 0, G[f'{t}/cls'])
        Dp = eng.cur.Dpatch[:st.nseq * self.n_in]
        ops.segment_sum([D], self.unpad[0], self.unpad[1], Dp)
        eng._t_colsum(tr, Dp, G[f'{p}/embedding/bias'])
        eng._flush_tower_reductions(tr)
        eng.gemm(self.x2d, Dp, G[f'{p}/embedding/kernel'], transA=True)
