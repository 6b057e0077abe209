"""Host logic of the TVQA step (CPU only): build_tvqa_plan's integer decisions against the literal restatement of the reference's index
code (tests/tvqa_ref.py: finetune/tvqa/tvqa_finetune.py:170-250 on oracle.ref_torch.prepare_multimodal_inputs), the joint "rotary"
table, and the parameter tree.  Everything here is bit-exact."""
import numpy as np
import torch

from merlot_reserve_amd.params import ALIGN, VOCAB, ParamStore, decay_finetune, param_specs, tvqa_param_specs
from merlot_reserve_amd.planner import build_tvqa_plan, rot_scale_table, rotary_coords_2d, tvqa_image_transpose
from merlot_reserve_amd.tvqa import TVQADims
from oracle import ref_torch as R
from tests.tvqa_ref import ref_batch, tvqa_batch, tvqa_cfg, tvqa_joint_inputs


def _scattered_batch(cfg, d, seed):
    """Random streams whose AUDIOSPAN tokens are scattered and number more than nspans * a_tok (the span pointer wraps around)."""
    rng = np.random.default_rng(seed)
    batch = {}
    for k in ('audio_seqs', 'textonly_seqs'):
        tok = rng.integers(0, 40, size=(d.B, d.A, d.T))
        tok = np.where(rng.random((d.B, d.A, d.T)) < 0.9, R.AUDIOSPAN, tok)
        tok[:, :, -3:] = R.PADDING
        batch[k] = np.stack([tok, rng.integers(0, d.nseg + 1, size=tok.shape)], -1).astype(np.int32)
    assert ((batch['audio_seqs'][..., 0] == R.AUDIOSPAN).sum(-1) > d.nspans * d.a_tok).any()
    return batch


def _markers(d):
    """Row tables of width 2 that name their own rows: (table 1 = tokens / 2 = audio rows / 3 = image rows, row)."""
    mk = lambda t, n: torch.stack([torch.full((n,), float(t), dtype=torch.float64), torch.arange(n, dtype=torch.float64)], -1)
    return mk(1, VOCAB), mk(2, d.Na * d.a_tok), mk(3, d.Nv * d.V)


def _check_plan(cfg, d, batch):
    plan = build_tvqa_plan(batch['textonly_seqs'], batch['audio_seqs'], d)
    emb, aud, img = _markers(d)
    rb = {k: torch.from_numpy(batch[k].astype(np.int64)) for k in ('textonly_seqs', 'audio_seqs')}
    x, coords, mask, pool_idx = tvqa_joint_inputs({'token_encoder': {'Embed_0': {'embedding': emb}}}, R.Cfg(cfg), rb,
                                                  img.reshape(d.B, d.nseg, d.V, 2), aud.reshape(d.B, d.nspans, d.a_tok, 2))
    n, Sj = d.n, d.Sj
    assert x.shape == (n, Sj, 2) and coords.shape == (n, Sj, 4) and mask.shape == (n, Sj, Sj)
    # the source table and row of every joint position
    ip, ix = plan['joint_gather_indptr'], plan['joint_gather_idx'].astype(np.int64)
    assert np.array_equal(ip, np.arange(n * Sj + 1)), 'every position reads exactly one row'
    table = torch.cat([emb, aud, img])
    assert torch.equal(table[ix], x.reshape(n * Sj, 2))
    # one validity code per position reproduces the [Sj, Sj] mask
    valid = torch.from_numpy(plan['joint_code'].reshape(n, Sj) == 0)
    assert set(np.unique(plan['joint_code'])) <= {0, -1}
    assert torch.equal(valid[:, :, None] & valid[:, None, :], mask)
    # the pool rows and their transpose
    want_rows = (torch.arange(n) * Sj + pool_idx).numpy()
    assert np.array_equal(plan['pool_idx'], want_rows) and np.array_equal(plan['pool_indptr'], np.arange(n + 1))
    assert np.array_equal(plan['pool_pos'], pool_idx.numpy())
    _assert_inverse(plan['poolT_indptr'], plan['poolT_idx'], {int(r): [q] for q, r in enumerate(want_rows)}, n * Sj)
    # the "rotary" table of the restatement's coordinates
    assert np.array_equal(plan['joint_rot'], rot_scale_table(coords).reshape(n * Sj, 32))
    # transposed lists: the exact inverse of the gather, ascending positions.  Token rows: PAD positions are left out (exactly-zero
    # gradient) unless the sequence's pooled position is PAD
    src_t, src_r = x[..., 0].reshape(-1).long().numpy(), x[..., 1].reshape(-1).long().numpy()
    seq = np.arange(n * Sj) // Sj
    pooled_is_pad = ~valid.numpy()[np.arange(n), pool_idx.numpy()]
    inv = {1: {}, 2: {}, 3: {}}
    for pos in range(n * Sj):
        if src_t[pos] == 1 and src_r[pos] == R.PADDING and not pooled_is_pad[seq[pos]]:
            continue
        inv[src_t[pos]].setdefault(int(src_r[pos]), []).append(pos)
    _assert_inverse(plan['embT_indptr'], plan['embT_idx'], inv[1], VOCAB)
    _assert_inverse(plan['audT_indptr'], plan['audT_idx'], inv[2], d.Na * d.a_tok)
    vp, vx = tvqa_image_transpose(d)
    _assert_inverse(vp, vx, inv[3], d.Nv * d.V)
    assert all(len(v) == 2 * d.A for v in inv[3].values()) and len(inv[3]) == d.Nv * d.V
    return plan, x, pool_idx


def _assert_inverse(indptr, idx, want, n_dst):
    assert len(indptr) == n_dst + 1 and indptr[0] == 0 and indptr[-1] == len(idx) == sum(len(v) for v in want.values())
    for dst in np.nonzero(np.diff(indptr))[0]:
        assert idx[indptr[dst]:indptr[dst + 1]].tolist() == want[int(dst)], dst
    assert set(np.nonzero(np.diff(indptr))[0].tolist()) == set(want)


def test_plan_matches_the_restatement_on_the_test_batch():
    cfg = tvqa_cfg()
    d = TVQADims(cfg, 2)
    assert (d.V, d.Sj, d.n, d.Nv, d.Sv, d.Na, d.Sa) == (6, 82, 12, 6, 25, 18, 31)
    batch = tvqa_batch(cfg, 2, seed=0)
    plan, x, pool_idx = _check_plan(cfg, d, batch)
    AB = d.A * d.B
    # the cases the batch holds by construction
    a00 = batch['audio_seqs'][0, 0, :, 0]
    assert (a00 == R.AUDIOSPAN).sum() == d.T - 21 and a00[-1] == R.AUDIOSPAN and (d.T - 21) % d.a_tok != 0      # a span cut in the middle
    assert x[0, d.T - 1].tolist() == [2.0, float(((d.T - 22) // d.a_tok) * d.a_tok + (d.T - 22) % d.a_tok)]
    assert R.MASK not in batch['textonly_seqs'][0, 1, :, 0] and pool_idx[AB + 1] == 0
    assert batch['audio_seqs'][1, 0, 0, 0] == R.PADDING and pool_idx[d.A] == 0 and plan['joint_code'][d.A * d.Sj] == -1
    q = AB + d.A + 2
    assert x[q, 1].tolist() == [1.0, float(R.AUDIOSPAN)], 'token id 5 is an ordinary token in the text stream'
    assert len(plan['embT_idx'][plan['embT_indptr'][R.AUDIOSPAN]:plan['embT_indptr'][R.AUDIOSPAN + 1]]) == 2
    assert plan['embT_indptr'][1] > 0, 'a sequence pooled at a PAD position sends gradient to the PAD row'
    # repeat-each, not tile: sequence b*A + a of either stream reads the image rows of example b
    img_rows = x[:, d.T:, 1].long()
    for s in range(2):
        for b in range(d.B):
            for a in range(d.A):
                assert torch.equal(img_rows[s * AB + b * d.A + a], b * d.nseg * d.V + torch.arange(d.nseg * d.V))


def test_plan_matches_the_restatement_with_scattered_audio_tokens():
    cfg = tvqa_cfg()
    d = TVQADims(cfg, 2)
    for seed in (1, 2):
        _check_plan(cfg, d, _scattered_batch(cfg, d, seed))


def test_rotary_rows_of_the_frames_known_answer():
    """Frame k's pooled tokens carry (pooled-grid h, w, segment k + 1, no token index); text tokens (their segment, token index p + 1)."""
    cfg = tvqa_cfg()
    d = TVQADims(cfg, 2)
    batch = tvqa_batch(cfg, 2, seed=0)
    rot = build_tvqa_plan(batch['textonly_seqs'], batch['audio_seqs'], d)['joint_rot'].reshape(d.n, d.Sj, 32)
    hw = rotary_coords_2d(d.gh // d.pr, d.gw // d.pr)
    for k in range(d.nseg):
        c = np.concatenate([hw, np.full((d.V, 1), (k + 1) / 16.0), np.zeros((d.V, 1))], 1)
        want = rot_scale_table(c)
        for q in range(d.n):
            assert np.array_equal(rot[q, d.T + k * d.V:d.T + (k + 1) * d.V], want), (k, q)
    AB = d.A * d.B
    for s, key in enumerate(('audio_seqs', 'textonly_seqs')):
        seg = batch[key][..., 1].reshape(AB, d.T)
        c = np.zeros((AB, d.T, 4))
        c[..., 2], c[..., 3] = seg / 16.0, (1.0 + np.arange(d.T))[None] / 1024.0
        assert np.array_equal(rot[s * AB:(s + 1) * AB, :d.T], rot_scale_table(c))


def test_tvqa_param_specs():
    cfg = tvqa_cfg()
    specs = tvqa_param_specs(cfg)
    names = [s[0] for s in specs]
    pre = {s[0]: s for s in param_specs(cfg)}
    want = {n for n in pre if not n.startswith(('head/', 'span_encoder/', 'contrastive_scales'))} | {'proj/kernel'}
    assert set(names) == want and len(names) == len(set(names))
    assert all(s == pre[s[0]] for s in specs if s[0] != 'proj/kernel'), 'shapes, views and initialisers of the pretraining tree'
    assert dict((s[0], s[1]) for s in specs)['proj/kernel'] == (128, 1)
    assert 'audio_encoder/seq_attnpool/query/kernel' in names
    # the order backward finishes them: proj, joint tower, token table, audio tower, vision tower
    towers = [n.split('/')[0] for n in names]
    assert [t for i, t in enumerate(towers) if i == 0 or towers[i - 1] != t] == ['proj', 'joint_transformer', 'token_encoder', 'audio_encoder', 'vision_encoder']
    store = ParamStore(cfg, 'meta', init=False, specs=specs, decay_rule=decay_finetune, with_orig=True)
    assert list(store.tower_ranges) == ['proj', 'joint_transformer', 'token_encoder', 'audio_encoder', 'vision_encoder']
    a0, a1 = store.tower_ranges['audio_encoder']
    assert a0 == store.tower_ranges['token_encoder'][1] and a1 == store.tower_ranges['vision_encoder'][0] and store.tower_ranges['vision_encoder'][1] == store.total
    assert all(lo % ALIGN == 0 and hi % ALIGN == 0 for lo, hi in store.tower_ranges.values())
    # the engine's gradient buckets on that layout: joint, audio, the vision cuts -- every boundary a whole Adam block
    from merlot_reserve_amd.tvqa import TVQAEngine
    eng = TVQAEngine.__new__(TVQAEngine)
    eng.p, eng.d = store, TVQADims(cfg, 2)
    buckets, cuts = eng.gradient_buckets()
    assert [b[0] for b in buckets][:2] == ['joint', 'audio'] and buckets[-1][0] == 'vision_end' and buckets[1][1:] == (a0, a1)
    assert all(lo % 2048 == 0 and hi % 2048 == 0 for _, lo, hi in buckets) and sum(hi - lo for _, lo, hi in buckets) == store.total
