"""Host side of the zero-shot head (no GPU): the C-ABI of libmreserve_zeroshot.so (exports, prototypes, argument checks, a ledger of which test
calls which export), the build scans over zeroshot.hip, the restatements of tests/zeroshot_refs.py against each other, the accuracy books of
ZeroShotClassifier.evaluate on hand-made rankings (the scoring step injected), and the synthetic manifest round trip."""
import ctypes
import json
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from zeroshot_refs import ref_group_max, ref_group_walk, ref_logits64, ref_lse, ref_topk, round_f32

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'mreserve_zeroshot.h')


def _built():
    import __graft_entry__
    __graft_entry__.build()


def declared_symbols():
    text = re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r'\b(mrz_[a-z0-9_]+)\s*\(', text)))


# ------------------------------------------------------------------------------------------------ the library
def test_zeroshot_library_exports_the_header_and_nothing_else():
    _built()
    from merlot_reserve_amd import _lib, _media_lib, _zeroshot_lib
    names = declared_symbols()
    assert names == ['mrz_last_error', 'mrz_score_topk', 'mrz_version', 'mrz_workspace_bytes']
    out = subprocess.check_output(['nm', '-D', '--defined-only', _zeroshot_lib.LIB_PATH], text=True)
    assert sorted(line.split()[-1] for line in out.splitlines() if line.strip()) == names
    assert set(_zeroshot_lib.PROTOTYPES) == set(names)
    assert not set(_zeroshot_lib.PROTOTYPES) & (set(_lib.PROTOTYPES) | set(_media_lib.PROTOTYPES))
    assert _zeroshot_lib.load().mrz_version() >= 1
    # the three libraries carry only their own prefix
    for path, own in ((_lib.LIB_PATH, 'mr_'), (_media_lib.LIB_PATH, 'mrm_'), (_zeroshot_lib.LIB_PATH, 'mrz_')):
        syms = [line.split()[-1] for line in subprocess.check_output(['nm', '-D', '--defined-only', path], text=True).splitlines() if line.strip()]
        assert syms and all(s.startswith(own) for s in syms), path
    text = open(HEADER).read()
    assert (_zeroshot_lib.SLICE, _zeroshot_lib.MAX_K, _zeroshot_lib.MAX_H) == tuple(int(re.search(rf'#define {n} (\d+)', text).group(1))
                                                                                    for n in ('MRZ_SLICE', 'MRZ_MAX_K', 'MRZ_MAX_H'))
    assert (_zeroshot_lib.DT_BF16, _zeroshot_lib.DT_F32) == (0, 1) and '#define MRZ_DT_BF16 0' in text and '#define MRZ_DT_F32 1' in text


def test_prototypes_match_the_header():
    """Argument counts and the C types of every parameter against the ctypes table."""
    from merlot_reserve_amd import _zeroshot_lib as M
    text = re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)
    ctype = {'int': M.i32, 'int32_t': M.i32, 'int64_t': M.i64, 'float': M.f32, 'const char*': ctypes.c_char_p}
    found = re.findall(r'^([a-z0-9_ ]+?\*?)\s*(mrz_[a-z0-9_]+)\s*\(([^)]*)\)\s*;', text, flags=re.M | re.S)
    assert sorted(name for _, name, _ in found) == declared_symbols()
    for ret, name, args in found:
        res, argtypes = M.PROTOTYPES[name]
        assert res is ctype[ret.strip()], name
        params = [] if args.strip() == 'void' else [a.strip() for a in args.split(',')]
        assert len(params) == len(argtypes), name
        for p, t in zip(params, argtypes):
            want = M.vp if '*' in p else ctype[p.rsplit(' ', 1)[0].strip()]
            assert t is want, (name, p)


def test_unsupported_ranges_are_refused_without_a_launch():
    _built()
    from merlot_reserve_amd import _zeroshot_lib as M
    lib = M.load()
    p = 1 << 20                      # fake 16-byte aligned device addresses: never dereferenced, every case is rejected before a launch
    F, B = M.DT_F32, M.DT_BF16
    #     queries ldq dt labels ldl dt Q  L   H    scale  k  val idx lse logits groups G  gval ggrp glab ws stream
    ok = (p, 768, F, p, 768, B, 4, 1000, 768, 100.0, 5, p, p, p, None, p, 7, p, p, p, p, None)

    def refused(i, v, *words):
        rc = lib.mrz_score_topk(*(ok[:i] + (v,) + ok[i + 1:]))
        msg = lib.mrz_last_error()
        assert rc == -1 and msg.startswith(b'mrz_score_topk:') and all(w in msg for w in words), (i, v, rc, msg)
    for H in (0, 32, 96, 2048 + 64):
        refused(8, H, b'H = ')
    for k in (0, 65, -1):
        refused(10, k, b'k = ')
    for L in (0, 1 << 24):
        refused(7, L, b'L = ')
    for Q in (0, -3, (1 << 31) - 16):
        refused(6, Q, b'Q = ')
    refused(16, 1001, b'G = ')       # G > L
    refused(16, 0, b'G = ')          # groups given, no group
    refused(1, 767, b'row stride')
    refused(4, 760, b'row stride')
    refused(1, 770, b'16-byte')      # fp32 rows of 770 elements: stride 3080 bytes
    refused(4, 772, b'16-byte')      # bf16 rows of 772 elements: stride 1544 bytes
    refused(0, p + 4, b'16-byte')
    refused(3, p + 8, b'16-byte')
    refused(2, 2, b'dtypes')
    refused(5, -1, b'dtypes')
    for i in (0, 3, 11, 12, 13):
        refused(i, None, b'null pointer')
    for i in (17, 18, 19):
        refused(i, None, b'null pointer', b'group')
    refused(20, None, b'null pointer', b'workspace')
    refused(20, p + 8, b'workspace')
    # the workspace: none for one slice without groups; the same ranges refused
    assert lib.mrz_workspace_bytes(33, M.SLICE, 0, 64) == 0 and lib.mrz_workspace_bytes(1, 1, 0, 1) == 0
    assert lib.mrz_workspace_bytes(33, M.SLICE + 1, 0, 64) > 0 and lib.mrz_workspace_bytes(33, 5, 5, 1) > 0
    assert lib.mrz_workspace_bytes(4, 3806, 97, 5) % 16 == 0
    for bad in ((0, 10, 0, 1), (1, 0, 0, 1), (1, 1 << 24, 0, 1), (1, 10, 11, 1), (1, 10, 0, 0), (1, 10, 0, 65)):
        assert lib.mrz_workspace_bytes(*bad) == -1 and lib.mrz_last_error().startswith(b'mrz_workspace_bytes:'), bad
    with pytest.raises(M.MreserveZeroshotError, match='mrz_workspace_bytes'):
        M.check(-1, 'mrz_workspace_bytes')
    # without groups G is not looked at, and one slice needs no workspace: refused only for the next thing wrong (H)
    rc = lib.mrz_score_topk(p, 768, F, p, 768, F, 4, 100, 32, 100.0, 5, p, p, p, None, None, 12345, None, None, None, None, None)
    assert rc == -1 and b'H = 32' in lib.mrz_last_error()


# which test file calls which export: (the Python names tests reach it by, the test files), in the style of test_media_host.py
HOST, GPU = 'test_zeroshot_host.py', 'test_zeroshot_gpu.py'
LEDGER = {
    'mrz_version': ((), (HOST,)),
    'mrz_last_error': ((), (HOST,)),
    'mrz_workspace_bytes': (('score_topk',), (GPU, HOST)),
    'mrz_score_topk': (('score_topk',), (GPU, HOST)),
}


def test_every_zeroshot_export_names_its_test():
    assert set(LEDGER) == set(declared_symbols())
    binding = open(os.path.join(ROOT, 'merlot_reserve_amd', 'zeroshot.py')).read()
    for export, (wrappers, files) in LEDGER.items():
        assert files, export
        for w in wrappers:
            assert re.search(rf'^def {re.escape(w)}\b', binding, flags=re.M) and re.search(rf'\b{export}\b', binding), export
        for fname in files:
            text = open(os.path.join(ROOT, 'tests', fname)).read()
            assert any(re.search(rf'\b{re.escape(n)}\b', text) for n in (export,) + tuple(wrappers)), (export, fname)
    assert set(LEDGER) != set(declared_symbols()) | {'mrz_some_new_export'}


def test_build_scans_cover_the_zeroshot_library():
    _built()
    from merlot_reserve_amd import build as B
    assert B.ZEROSHOT_HIP_FILES == ['zeroshot.hip']
    assert not set(B.ZEROSHOT_SOURCES) & (set(B.SOURCES) | set(B.MEDIA_SOURCES))
    assert '-fno-slp-vectorize' in B.EXTRA_FLAGS['zeroshot.hip']
    assert not any(re.search(rx, 'score_slice_kernel') or re.search(rx, 'merge_kernel') for rx in B.SPILL_ALLOWED)
    if B._asm_stale():
        B.build(force=True, verbose=False)
    assert B.scan_packed_op_sel(files=B.ZEROSHOT_HIP_FILES) == [] and B.scan_spills(files=B.ZEROSHOT_HIP_FILES) == []
    res = B.kernel_resources(B.ZEROSHOT_HIP_FILES)['zeroshot.hip']
    assert len(res) == 5 and all(e['vgpr_spill'] == 0 and e['sgpr_spill'] == 0 and e['scratch'] == 0 for e in res.values())     # four dtype pairs + the merge
    assert json.load(open(os.path.join(os.path.dirname(B.STAMP), 'resources.json')))['zeroshot.hip'] == res
    asm = open(B._asm_path('zeroshot.hip')).read()
    assert 'v_mfma_f32_16x16x4_f32' in asm and not re.search(r'global_atomic_(add|max|min)_f(32|64)', asm)


# ------------------------------------------------------------------------------------------------ the restatements against each other
def test_group_walk_is_max_per_group_with_ties_to_the_lower_representative():
    rng = np.random.default_rng(0)
    for case in range(200):
        Q, L = int(rng.integers(1, 4)), int(rng.integers(1, 40))
        G = int(rng.integers(1, L + 1))
        k = int(rng.integers(1, 12))
        x = rng.integers(-2, 3, size=(Q, L)).astype(np.float32) / 4 + np.float32(0.0)       # five values: ties everywhere
        groups = rng.integers(0, G, size=L)
        walk, best = ref_group_walk(x, groups, k), ref_group_max(x, groups, G, k)
        for a, b in zip(walk, best):
            assert a.dtype == b.dtype and np.array_equal(a, b), case
        n = min(k, len(set(groups.tolist())))
        assert (walk[1][:, :n] >= 0).all() and (walk[1][:, n:] == -1).all() and np.isneginf(walk[0][:, n:]).all()
        for q in range(Q):
            assert len(set(walk[1][q, :n].tolist())) == n
            assert (groups[walk[2][q, :n]] == walk[1][q, :n]).all() and (x[q, walk[2][q, :n]] == walk[0][q, :n]).all()


def test_topk_restatement_on_a_hand_made_row():
    x = np.array([[1.0, 3.0, 3.0, -0.0, 0.0, 3.0]], dtype=np.float32) + np.float32(0.0)
    vals, idx = ref_topk(x, 8)
    assert idx.tolist() == [[1, 2, 5, 0, 3, 4, -1, -1]] and vals[0, :6].tolist() == [3.0, 3.0, 3.0, 1.0, 0.0, 0.0] and np.isneginf(vals[0, 6:]).all()
    assert abs(ref_lse(x.astype(np.float64))[0] - np.log(3 * np.exp(3.0) + np.exp(1.0) + 2.0)) < 1e-12
    assert round_f32(np.array([-0.0])).view(np.uint32)[0] == 0
    assert ref_logits64(np.array([[0.25, 0.5]], np.float32), np.array([[1.0, 1.0], [0.0, -2.0]], np.float32), 100.0).tolist() == [[75.0, -100.0]]


# ------------------------------------------------------------------------------------------------ the accuracy books
class FakeModel:
    """out_h row of a <|MASK|> = the one-hot-ish vector the video names; label i = unit vector i.  Counts its calls."""
    H = 64

    def __init__(self):
        self.label_calls, self.video_calls, self.batch_sizes = 0, 0, []

    def embed_text_spans_only(self, ids):
        self.label_calls += 1
        out = torch.zeros((len(ids), self.H))
        out[torch.arange(len(ids)), torch.as_tensor(np.asarray(ids)[:, 0])] = 1.0          # the option's first token id names its axis
        return out

    def batch_embed_video(self, images, audio_clips, tokens, subseg_idxs):
        self.video_calls += 1
        self.batch_sizes.append(len(tokens))
        out = torch.zeros((len(tokens), tokens.shape[1], self.H))
        for b in range(len(tokens)):
            out[b, :, :images.shape[-1]] = torch.as_tensor(np.asarray(images[b, 0]), dtype=torch.float32)   # every row: the video's scores
        return out


def restated_scorer(label_space, scale):
    from merlot_reserve_amd.zeroshot import ScoreResult

    def scorer(queries, k, return_logits, groups, num_groups):
        x64 = ref_logits64(queries.numpy(), label_space.numpy(), scale)
        x = round_f32(x64)
        vals, idx = ref_topk(x, k)
        res = ScoreResult(torch.from_numpy(vals), torch.from_numpy(idx), torch.from_numpy(ref_lse(x64).astype(np.float32)))
        if return_logits:
            res.logits = torch.from_numpy(x)
        if groups is not None:
            g = ref_group_walk(x, np.asarray(groups), k)
            res.group_values, res.group_ids, res.group_labels = (torch.from_numpy(a) for a in g)
        return res
    return scorer


def fake_video(scores, n_mask=1, n_seg=1):
    """A preprocess_video-shaped dict whose 'images' carry the option scores the fake model turns into out_h"""
    tokens = np.zeros(160, dtype=np.int32)
    tokens[:4] = [11, 12, 13, 14]
    tokens[4:4 + n_mask] = 3
    img = np.zeros((n_seg, 1, len(scores)), dtype=np.float32)
    img[:, 0] = scores
    return {'images': img, 'audio_clips': np.zeros((3 * n_seg, 60, 65), np.float32), 'tokens': tokens, 'subseg_idxs': np.zeros(160, np.int32)}


def test_evaluate_books_on_hand_made_rankings():
    from merlot_reserve_amd.zeroshot import ZeroShotClassifier, topk_accuracy
    assert topk_accuracy([[3, 1, 2], [0, 4], [], [5]], [1, 4, 0, -1], (1, 2, 3)) == {1: 0.0, 2: 0.5, 3: 0.5}
    options = ['open door', 'close door', 'open fridge', 'wash cup', 'wash plate', 'cut onion']
    ids = np.zeros((6, 15), dtype=np.int64)
    ids[:, 0] = np.arange(6)
    groups = {'verb': [o.split()[0] for o in options], 'noun': [0, 0, 1, 2, 3, 4]}
    model = FakeModel()
    clf = ZeroShotClassifier(model, options=options, option_ids=ids, groups=groups, scale=1.0, encode_chunk=4)
    assert model.label_calls == 2 and clf.label_space.shape == (6, 64)          # 4 + 2 options, once
    assert clf.group_ids['verb'].tolist() == [0, 1, 0, 2, 2, 3] and clf.group_names['verb'] == ['open', 'close', 'wash', 'cut'] and clf.group_names['noun'] is None
    clf._scorer = restated_scorer(clf.label_space, 1.0)
    #         scores per option                      ranking (ties by index)   verbs           nouns
    videos = [fake_video([5, 1, 4, 0, 0, 3]),        # 0 2 5 1 3 4             open cut close  0 1 4
              fake_video([2, 2, 2, 2, 2, 2]),        # 0 1 2 3 4 5             open close wash 0 1 2
              fake_video([0, 0, 1, 7, 7, 0], 2),     # 3 4 2 0 1 5             wash open close 2 3 1
              fake_video([1, 2, 3, 4, 5, 6], 0),     # no <|MASK|>: no prediction
              fake_video([0, 9, 0, 0, 1, 0], 1, 2)]  # 1 4 0 2 3 5 (other shape: a batch of its own)
    out = clf.classify(videos, k=3, batch_size=2)
    assert model.batch_sizes == [2, 2, 1] and model.label_calls == 2
    assert [len(r) for r in out] == [1, 1, 2, 0, 1]
    assert out[0][0]['indices'] == [0, 2, 5] and out[0][0]['options'] == ['open door', 'open fridge', 'cut onion']
    assert out[0][0]['groups']['verb']['names'] == ['open', 'cut', 'close'] and out[0][0]['groups']['verb']['labels'] == [0, 5, 1]
    assert out[0][0]['groups']['noun']['ids'] == [0, 1, 4] and out[0][0]['groups']['noun']['names'] is None
    assert out[1][0]['indices'] == [0, 1, 2] and out[1][0]['groups']['verb']['ids'] == [0, 1, 2] and np.allclose(out[1][0]['probs'], 1 / 6)
    assert out[2][0] == out[2][1] and out[2][0]['indices'] == [3, 4, 2] and out[2][0]['groups']['noun']['ids'] == [2, 3, 1]
    assert abs(out[0][0]['probs'][0] - np.exp(5) / np.exp(np.array([5, 1, 4, 0, 0, 3.0])).sum()) < 1e-6
    assert out[0][0]['groups']['verb']['probs'][1] == out[0][0]['probs'][2]      # a group's probability is its representative's
    one = clf.classify(videos[4], k=10)
    assert one[0]['indices'] == [1, 4, 0, 2, 3, 5] and len(one[0]['groups']['verb']['ids']) == 4      # k > L: no padding entries
    full = clf.ranking(videos[0])
    assert [o for _, o in full[0]] == ['open door', 'open fridge', 'cut onion', 'close door', 'wash cup', 'wash plate']
    assert abs(sum(p for p, _ in full[0]) - 1.0) < 1e-6 and clf.ranking(videos[3]) == []
    golds = ['open fridge',                                   # rank 2
             {'option': 0, 'verb': 'close', 'noun': 2},       # rank 1; verb rank 2; noun rank 3
             {'option': 'wash plate', 'verb': 'wash'},        # rank 2; verb rank 1
             3,                                               # no MASK: wrong
             {'option': 'peel potato', 'verb': 'peel', 'noun': 0}]    # not in the table: wrong; noun: option 1 leads, noun 0: rank 1
    acc = clf.evaluate(zip(videos, golds), ks=(1, 2, 3))
    assert acc['n'] == 5
    assert acc['options'] == {1: 1 / 5, 2: 3 / 5, 3: 3 / 5}
    assert acc['verb'] == {1: 1 / 3, 2: 2 / 3, 3: 2 / 3}
    assert acc['noun'] == {1: 1 / 2, 2: 1 / 2, 3: 2 / 2}
    with pytest.raises(KeyError):
        clf.evaluate([(videos[0], {'adverb': 1})])
    with pytest.raises(ValueError):
        clf.evaluate([(videos[0], 0)], ks=(1, 65))
    with pytest.raises(ValueError):
        ZeroShotClassifier(model)
    with pytest.raises(ValueError):
        ZeroShotClassifier(model, option_ids=ids, groups={'verb': [0, 1]})


def test_synthetic_manifest_round_trip(tmp_path):
    from merlot_reserve_amd import zeroshot_eval as Z
    labels, manifest = Z.write_synthetic(str(tmp_path), 3, (2, 3), num_options=11, seed=4)
    options, ids, groups = Z.read_labels(labels)
    assert options is None and ids.shape == (11, 15) and ids.dtype == np.int64 and (ids[:, 0] >= 10).all() and (ids[:, 5:] == 0).all()
    assert set(groups) == {'verb', 'noun'} and all(len(v) == 11 for v in groups.values())
    samples = Z.read_manifest(manifest)
    assert [s[0] for s in samples] == ['sample_0000', 'sample_0001', 'sample_0002']
    for sid, video, answer in samples:
        assert set(video) == set(Z.VIDEO_KEYS)
        assert video['images'].shape == (2, 6, 768) and video['images'].dtype == np.float32 and video['audio_clips'].shape == (6, 60, 65)
        assert video['tokens'].shape == (160,) and video['tokens'].dtype == np.int32 and int((video['tokens'] == 3).sum()) == 1
        assert 0 <= answer['option'] < 11 and answer['verb'] == groups['verb'][answer['option']] and answer['noun'] == groups['noun'][answer['option']]
    again = Z.write_synthetic(str(tmp_path / 'b'), 3, (2, 3), num_options=11, seed=4)
    assert open(again[1]).read() == open(manifest).read()
    assert all(np.array_equal(a[1][k], b[1][k]) for a, b in zip(samples, Z.read_manifest(again[1])) for k in Z.VIDEO_KEYS)
