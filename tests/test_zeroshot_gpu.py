"""The zero-shot head on the MI355X (merlot_reserve_amd.zeroshot: score_topk over mrz_score_topk / mrz_workspace_bytes, ZeroShotClassifier,
the zeroshot_eval command) against the float64 restatements of tests/zeroshot_refs.py.  Every case checks every row of every output.

Exact cases: elements in {-4 .. 4} / 16 make every dot product exact in fp32 in any order (and the inputs exact in bf16), so the logits, the
top-k, and the group outputs must equal the restatement BIT FOR BIT, ties (about half of a row's logits collide) broken by lower index."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from zeroshot_refs import (exact_rows, lse_bound, ref_group_walk, ref_logits64, ref_lse, ref_topk, round_f32, to_bf16_values, unit_rows)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QS, KS, HS = (1, 15, 16, 17, 33), (1, 5, 10, 64), (64, 768, 1024)
PAIRS = [(torch.float32, torch.float32), (torch.float32, torch.bfloat16), (torch.bfloat16, torch.float32), (torch.bfloat16, torch.bfloat16)]
QMAX, KMAX = max(QS), max(KS)


def slice_labels():
    from merlot_reserve_amd import zeroshot
    return zeroshot.SLICE_LABELS


def label_counts():
    s = 512                          # checked against the exported constant in the test: parametrisation happens before the package is importable
    return [1, 5, 63, 64, 65, 1000, 3806, s - 1, s, s + 1]


def bits(t):
    return t.contiguous().view(torch.int32)


def same_bits(got, want):
    return got.shape == want.shape and got.dtype == want.dtype and torch.equal(bits(got) if got.dtype == torch.float32 else got, bits(want) if want.dtype == torch.float32 else want)


def group_map(rng, L, G):
    """[L] int32 in [0, G), with groups left empty where G allows it (group 3 of G >= 7 is emptied; a random draw of G = L leaves about a third empty)"""
    g = rng.integers(0, G, size=L).astype(np.int32)
    if G >= 7:
        g[g == 3] = 0
    return g


@pytest.mark.parametrize('L', label_counts())
def test_exact_cases_are_bit_identical(dev, L):
    """Largest |lse - lse64| observed on the MI355X over all these cases: 1.52e-5 (at lse64 = 303, L = 513; bound there 1.0e-4, one fp32 ulp is
    3.1e-5); the largest error / bound ratio is 0.21 (1.38e-5 at lse64 = 262, L = 64).  Each case prints its own figure."""
    from merlot_reserve_amd.zeroshot import score_topk
    assert slice_labels() == 512 and {slice_labels() - 1, slice_labels(), slice_labels() + 1} <= set(label_counts())
    Gs = sorted({g for g in (1, 7, 97, L) if g <= L})
    c = 0
    worst = (0.0, 0.0, 0.0)
    for H in HS:
        rng = np.random.default_rng(1000 * L + H)
        qn, ln = exact_rows(rng, QMAX, H), exact_rows(rng, L, H)
        assert np.array_equal(to_bf16_values(qn), qn) and np.array_equal(to_bf16_values(ln), ln)
        qd = {dt: torch.from_numpy(qn).to(dev).to(dt) for dt in (torch.float32, torch.bfloat16)}
        ld = {dt: torch.from_numpy(ln).to(dev).to(dt) for dt in (torch.float32, torch.bfloat16)}
        gmaps = {G: group_map(rng, L, G) for G in Gs}
        gdev = {G: torch.from_numpy(g).to(dev) for G, g in gmaps.items()}
        for scale in (128.0, 100.0):
            x64 = ref_logits64(qn, ln, scale)
            x = round_f32(x64)
            if scale == 128.0:
                assert np.array_equal(x.astype(np.float64), x64)
            lse64 = ref_lse(x64)
            want = {'logits': x, 'top': ref_topk(x, KMAX), **{G: ref_group_walk(x, gmaps[G], KMAX) for G in Gs}}
            wd = {key: (torch.from_numpy(v).to(dev) if isinstance(v, np.ndarray) else tuple(torch.from_numpy(a).to(dev) for a in v)) for key, v in want.items()}
            for qdt, ldt in PAIRS:
                for Q in QS:
                    k, G = KS[c % len(KS)], Gs[(c // 20) % len(Gs)]
                    c += 1
                    r = score_topk(qd[qdt][:Q], ld[ldt], k, scale=scale, groups=gdev[G], num_groups=G, return_logits=True)
                    tag = (L, H, scale, qdt, ldt, Q, k, G)
                    assert same_bits(r.logits, wd['logits'][:Q]), tag
                    assert same_bits(r.values, wd['top'][0][:Q, :k].contiguous()) and same_bits(r.indices, wd['top'][1][:Q, :k].contiguous()), tag
                    for got, ref in zip((r.group_values, r.group_ids, r.group_labels), wd[G]):
                        assert same_bits(got, ref[:Q, :k].contiguous()), tag
                    err = np.abs(r.lse.cpu().numpy().astype(np.float64) - lse64[:Q])
                    bound = lse_bound(L, lse64[:Q])
                    i = int(np.argmax(err / bound))
                    if err[i] / bound[i] > worst[0]:
                        worst = (err[i] / bound[i], err[i], lse64[i])
                    assert (err <= bound).all(), (tag, err[i], bound[i], lse64[i])
            # without groups and without the logits output: with one slice no workspace and no second launch
            r = score_topk(qd[torch.float32], ld[torch.bfloat16], 10, scale=scale)
            assert r.logits is None and r.group_values is None
            assert same_bits(r.values, wd['top'][0][:, :10].contiguous()) and same_bits(r.indices, wd['top'][1][:, :10].contiguous()), (L, H, scale)
    print(f'L = {L}: largest lse error / bound {worst[0]:.3g} (error {worst[1]:.3g} at lse64 {worst[2]:.6g}); {c} calls')


def test_identical_labels_come_back_in_index_order(dev):
    from merlot_reserve_amd.zeroshot import score_topk
    rng = np.random.default_rng(5)
    L, H, Q = 1000, 768, 17
    qn = exact_rows(rng, Q, H)
    ln = np.repeat(exact_rows(rng, 1, H), L, axis=0)
    x = round_f32(ref_logits64(qn, ln, 100.0))
    groups = (np.arange(L) % 7).astype(np.int32)
    for qdt, ldt in PAIRS:
        r = score_topk(torch.from_numpy(qn).to(dev).to(qdt), torch.from_numpy(ln).to(dev).to(ldt), 64, groups=torch.from_numpy(groups).to(dev), num_groups=7)
        assert torch.equal(r.indices.cpu(), torch.arange(64, dtype=torch.int32).repeat(Q, 1))
        assert np.array_equal(r.values.cpu().numpy(), np.repeat(x[:, :1], 64, axis=1))
        assert torch.equal(r.group_labels.cpu()[:, :7], torch.arange(7, dtype=torch.int32).repeat(Q, 1)) and (r.group_labels.cpu()[:, 7:] == -1).all()
        assert torch.equal(r.group_ids.cpu(), r.group_labels.cpu()) and torch.isneginf(r.group_values.cpu()[:, 7:]).all()
        lse64 = ref_lse(x.astype(np.float64))
        assert (np.abs(r.lse.cpu().numpy() - lse64) <= lse_bound(L, lse64)).all()


@pytest.mark.parametrize('bf16', [False, True])
@pytest.mark.parametrize('shape', [(33, 3806, 768), (17, 1000, 1024)])
def test_realistic_rows(dev, shape, bf16):
    """Unit-normalised Gaussian rows, scale 100; delta = scale (H + 2) 2^-24 is the worst-case fp32 dot-product error of unit rows (4.6e-3 at
    H = 768).  Largest |top_val - logit64| observed on the MI355X: 1.57e-5 (fp32 inputs), 6.7e-6 (bf16 inputs, against their exact values); over
    the full logits output 1.74e-5 and 9.6e-6."""
    from merlot_reserve_amd.zeroshot import score_topk
    Q, L, H = shape
    k, scale = 64, 100.0
    rng = np.random.default_rng(Q + L)
    qn, ln = unit_rows(rng, Q, H), unit_rows(rng, L, H)
    dt = torch.bfloat16 if bf16 else torch.float32
    if bf16:
        qn, ln = to_bf16_values(qn), to_bf16_values(ln)
    qd, ld = torch.from_numpy(qn).to(dev).to(dt), torch.from_numpy(ln).to(dev).to(dt)
    assert torch.equal(qd.float().cpu(), torch.from_numpy(qn))
    r = score_topk(qd, ld, k, scale=scale, return_logits=True)
    x64 = ref_logits64(qn, ln, scale)
    delta = scale * (H + 2) * 2.0 ** -24
    vals, idx = r.values.cpu().numpy().astype(np.float64), r.indices.cpu().numpy()
    lse, logits = r.lse.cpu().numpy().astype(np.float64), r.logits.cpu().numpy().astype(np.float64)
    assert idx.shape == (Q, k) and (idx >= 0).all() and (idx < L).all()
    assert all(len(set(row.tolist())) == k for row in idx)
    at = np.take_along_axis(x64, idx, 1)
    print(f'{shape} bf16={bf16}: max |top_val - logit64| {np.abs(vals - at).max():.3g}, max |logits - logit64| {np.abs(logits - x64).max():.3g}, delta {delta:.3g}')
    assert (np.abs(vals - at) <= delta).all()
    assert (np.abs(logits - x64) <= delta).all()
    rth = -np.sort(-x64, axis=1)[:, :k]
    assert (at >= rth - 2 * delta).all()
    assert (np.diff(vals, axis=1) <= 0).all()
    assert (np.diff(idx, axis=1)[np.diff(vals, axis=1) == 0] > 0).all()
    assert np.array_equal(vals, np.take_along_axis(logits, idx, 1))          # the values ARE the logits at the indices
    lse64 = ref_lse(x64)
    bound = delta + lse_bound(L, lse64)
    assert (np.abs(lse - lse64) <= bound).all()
    assert (np.abs(np.exp(logits - lse[:, None]).sum(1) - 1.0) <= bound).all()
    assert np.allclose(r.probs.cpu().numpy(), np.exp(vals - lse[:, None]), rtol=1e-5, atol=0)


def test_a_row_does_not_depend_on_its_batch(dev):
    """33 rows at once, each alone, and in reversed order: every output of a row bit-identical in all three."""
    from merlot_reserve_amd.zeroshot import score_topk
    rng = np.random.default_rng(11)
    Q, L, H, k, G = 33, 1000, 768, 10, 97
    qd, ld = torch.from_numpy(unit_rows(rng, Q, H)).to(dev), torch.from_numpy(unit_rows(rng, L, H)).to(dev)
    groups = torch.from_numpy(group_map(rng, L, G)).to(dev)
    fields = ('values', 'indices', 'lse', 'logits', 'group_values', 'group_ids', 'group_labels')

    def run(q):
        r = score_topk(q, ld, k, groups=groups, num_groups=G, return_logits=True)
        return {f: getattr(r, f) for f in fields}
    for dt in (torch.float32, torch.bfloat16):
        q = qd.to(dt)
        full, rev = run(q), run(q.flip(0))
        for f in fields:
            assert same_bits(rev[f].flip(0), full[f]), (dt, f)
        for i in range(Q):
            one = run(q[i:i + 1])
            for f in fields:
                assert same_bits(one[f], full[f][i:i + 1]), (dt, f, i)


# ------------------------------------------------------------------------------------------------ classifier
class CountingModel:
    def __init__(self, pm):
        self.pm, self.label_calls, self.label_rows = pm, 0, 0

    def embed_text_spans_only(self, ids):
        self.label_calls += 1
        self.label_rows += len(ids)
        return self.pm.embed_text_spans_only(ids)

    def __getattr__(self, name):
        return getattr(self.pm, name)


def tiny_videos(cfg):
    from merlot_reserve_amd import preprocess as P
    gh, gw = cfg['model']['output_grid']
    videos = []
    for seed, n_mask in ((0, 1), (1, 1), (2, 1), (3, 2)):
        rng = np.random.default_rng(seed)
        text = rng.integers(10, 32768, size=7).tolist() + [3] + (rng.integers(10, 32768, size=3).tolist() + [3] if n_mask == 2 else [])
        segs = [{'patches': rng.random((gh * gw, 768)).astype(np.float32), 'text': text}]
        for i in range(1, 4):
            spec = (rng.random((3, 60, 65)) * 5).astype(np.float32)
            spec[..., 64] = 1.0
            segs.append({'patches': rng.random((gh * gw, 768)).astype(np.float32), 'spectrogram': spec, 'use_text_as_input': False})
        videos.append(P.preprocess_video(segs, (gh, gw)))
    return videos


def test_classifier_on_a_model(dev):
    """The smallest model configuration of the suite (tiny_config: hidden 128, grid 4 x 6, 4 segments), 40 token-id options, two group maps; the
    reference is 100 * out_h[tokens == MASK] @ label_space.T in float64 from the model's own embed_video / embed_text_spans_only.  With
    batch_size 4 the model's batched forward is not bit-identical to its single forward, so a row's tolerance grows by
    scale * |q_batched - q_single| * max |label| (Cauchy-Schwarz), both embeddings taken from the model here."""
    from merlot_reserve_amd import modeling as M
    from merlot_reserve_amd.config import tiny_config
    from merlot_reserve_amd.zeroshot import ZeroShotClassifier
    cfg = tiny_config()
    cfg['model']['use_bfloat16'] = False
    model = M.MerlotReserve.from_config(cfg, device=dev)
    pm = CountingModel(M.PretrainedMerlotReserve(encoder=None, params=model.init_from_dummy_batch(seed=5), model=model))
    H, L, k, scale = 128, 40, 5, 100.0
    rng = np.random.default_rng(2)
    option_ids = np.zeros((L, 15), dtype=np.int64)
    for row in option_ids:
        m = int(rng.integers(1, 6))
        row[:m] = rng.integers(10, 32768, size=m)
    groups = {'verb': (np.arange(L) % 7).tolist(), 'noun': [f'noun{i // 3}' for i in range(L)]}
    clf = ZeroShotClassifier(pm, option_ids=option_ids, groups=groups, encode_chunk=16)
    assert (pm.label_calls, pm.label_rows) == (3, L) and clf.label_space.shape == (L, H) and clf.label_space.dtype == torch.float32
    videos = tiny_videos(cfg)
    lab64 = pm.pm.embed_text_spans_only(option_ids).double().cpu().numpy()
    assert np.array_equal(lab64, clf.label_space.double().cpu().numpy())
    singles = [pm.embed_video(**v)[torch.from_numpy(v['tokens'] == 3).to(dev)].double().cpu().numpy() for v in videos]
    batched = pm.batch_embed_video(*[np.stack([v[key] for v in videos]) for key in ('images', 'audio_clips', 'tokens', 'subseg_idxs')])
    batched = [batched[i][torch.from_numpy(v['tokens'] == 3).to(dev)].double().cpu().numpy() for i, v in enumerate(videos)]
    delta = scale * (H + 2) * 2.0 ** -24
    lab_norm = np.linalg.norm(lab64, axis=1).max()
    for bs, embedded in ((1, singles), (4, batched)):
        out = clf.classify(videos, k=k, batch_size=bs)
        assert [len(o) for o in out] == [1, 1, 1, 2]
        for v, q_single, q_used, res in zip(videos, singles, embedded, out):
            x64 = scale * q_single @ lab64.T
            for m, entry in enumerate(res):
                d = delta + scale * np.linalg.norm(q_used[m] - q_single[m]) * lab_norm
                idx, p = np.array(entry['indices']), np.array(entry['probs'])
                assert len(idx) == k and len(set(idx.tolist())) == k and (idx >= 0).all() and (idx < L).all() and entry['options'] is None
                at = x64[m][idx]
                assert (at >= -np.sort(-x64[m])[:k] - 2 * d).all() and (np.diff(p) <= 0).all()
                assert (np.diff(idx)[np.diff(p) == 0] > 0).all()
                lse64 = ref_lse(x64[m:m + 1])[0]
                assert (np.abs(np.log(p) + lse64 - at) <= 2 * d + lse_bound(L, lse64)).all()
                for name, gid in (('verb', np.arange(L) % 7), ('noun', np.arange(L) // 3)):
                    g = entry['groups'][name]
                    assert len(g['ids']) == k and len(set(g['ids'])) == k and (gid[g['labels']] == g['ids']).all()
                    assert g['names'] == (None if name == 'verb' else [f'noun{i}' for i in g['ids']])
                    gmax = np.array([x64[m][gid == i].max() for i in range(gid.max() + 1)])
                    assert (x64[m][g['labels']] >= gmax[g['ids']] - 2 * d).all()              # the representative attains its group's maximum
                    assert (gmax[g['ids']] >= -np.sort(-gmax)[:k] - 2 * d).all() and (np.diff(g['probs']) <= 0).all()
        assert pm.label_calls == 3                              # encoded once, never again
    full = clf.ranking(videos[3])
    assert len(full) == 2 and all(len(r) == L and abs(sum(p for p, _ in r) - 1.0) <= 1e-5 for r in full)
    assert all(sorted(o for _, o in r) == list(range(L)) and all(a[0] >= b[0] for a, b in zip(r, r[1:])) for r in full)
    acc = clf.evaluate([(v, {'option': int(o[0]['indices'][0]), 'verb': int(o[0]['groups']['verb']['ids'][1])}) for v, o in zip(videos, out)], ks=(1, 5))
    assert acc == {'options': {1: 1.0, 5: 1.0}, 'verb': {1: 0.0, 5: 1.0}, 'n': 4} and pm.label_calls == 3


def test_zeroshot_eval_command(dev, tmp_path):
    out = str(tmp_path / 'run')
    cmd = [sys.executable, '-m', 'merlot_reserve_amd.zeroshot_eval', 'base', '--random-weights', '--synthetic', '6', '--grid', '12', '20', '--out', out,
           '-k', '1', '5', '10', '--batch-size', '4']
    p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    acc = json.load(open(os.path.join(out, 'accuracy.json')))
    preds = [json.loads(line) for line in open(os.path.join(out, 'predictions.jsonl'))]
    assert acc['n'] == 6 and len(preds) == 6 and set(acc) == {'n', 'options', 'verb', 'noun'}
    assert json.loads(p.stdout.strip().splitlines()[-1])['n'] == 6
    for key, field in (('options', None), ('verb', 'verb'), ('noun', 'noun')):
        for k in (1, 5, 10):
            hits = 0
            for rec in preds:
                assert len(rec['masks']) == 1
                first = rec['masks'][0]
                ranked = first['indices'] if field is None else first['groups'][field]['ids']
                gold = rec['answer']['option' if field is None else field]
                hits += gold in ranked[:k]
            assert 0.0 <= acc[key][str(k)] <= 1.0 and abs(acc[key][str(k)] - hits / 6) < 1e-12, (key, k)
    first = preds[0]['masks'][0]
    assert len(first['indices']) == 10 and abs(sum(first['probs'])) <= 1.0 + 1e-5 and all(a >= b for a, b in zip(first['probs'], first['probs'][1:]))
