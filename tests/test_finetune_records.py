"""The finetuning reader (merlot_reserve_amd/finetune_records.py = the reference's finetune/common_dataloader.py) on the host: hand-built VCR and
TVQA records with known answers, the two builders over synthetic shards, and the planners on what the readers produce.  Nothing touches a GPU."""
import io

import numpy as np
import pytest

from merlot_reserve_amd import finetune_records as FR
from merlot_reserve_amd import records as R
from merlot_reserve_amd.config import tiny_config

MASK, AUDIOSPAN = 3, 5
SEP = {'qa': [901, 902], 'qar': [903, 904, 905]}


def _jpeg(arr, _mode=None):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(arr).save(buf, format='JPEG', quality=95)
    return buf.getvalue()


def vcr_cfg():
    cfg = tiny_config(hidden_size=128, grid=(4, 6))
    cfg['data'].update(lang_seq_len=16, num_answers=4)
    return cfg


def tvqa_cfg(nseg=7):
    cfg = tiny_config(hidden_size=128, grid=(4, 6), num_segments=nseg, lang_seq_len=64)
    cfg['data'].update(num_answers=3)
    return cfg


# ---------------------------------------------------------------------------------------------------- 1. a VCR record with a known answer
def _vcr_record():
    red = np.zeros((64, 96, 3), np.uint8)
    red[..., 0] = 220
    blue = np.zeros((64, 96, 3), np.uint8)
    blue[..., 2] = 220
    feats = {'image': _jpeg(red, 'RGB'), 'image_fliplr': _jpeg(blue, 'RGB'), 'id': b'val-7-qar_2', 'qa_label': 2, 'qar_label': 1,
             'qa_query': list(range(100, 112)),                 # 12 + 2 separator tokens + a choice > T - 1 = 15: cut
             'qar_query': [200, 201, 202]}
    for i in range(4):
        feats[f'qa_choice_{i}'] = [300 + 10 * i, 301 + 10 * i, 302 + 10 * i]
        feats[f'qar_choice_{i}'] = [400 + i] * (i + 1)
    return R.make_example(feats)


def _is_red(image):
    px = image.reshape(-1, 3)                                   # patches are (dy, dx, c) triples
    return px[:, 0].mean() > 0.5 > px[:, 2].mean()


def test_vcr_record_with_known_answer():
    cfg = R.merged_data_config(vcr_cfg())
    rec = _vcr_record()
    out = FR.preprocess_vcr(rec, dict(cfg, do_random_scale=False), np.random.default_rng(0), sep_tokens=SEP)
    assert out['id'] == 'val-7-qar_2' and out['labels'].tolist() == [2, 1] and out['labels'].dtype == np.int32
    assert out['image'].shape == (24, 768) and out['image'].dtype == np.float32
    assert out['answers'].shape == (2, 4, 16) and out['answers'].dtype == np.int32
    for i in range(4):                                           # qa: 12 query + 2 separator + 1 choice token = T - 1, then MASK: no padding at all
        assert out['answers'][0, i].tolist() == list(range(100, 112)) + [901, 902, 300 + 10 * i, MASK]
    for i in range(4):                                           # qar: query + separator + (i + 1) choice tokens + MASK, zero padded
        want = [200, 201, 202, 903, 904, 905] + [400 + i] * (i + 1) + [MASK]
        assert out['answers'][1, i].tolist() == want + [0] * (16 - len(want))
    # do_random_scale=False always takes `image`; with it, both occur
    for s in range(20):
        assert _is_red(FR.preprocess_vcr(rec, dict(cfg, do_random_scale=False), np.random.default_rng(s), sep_tokens=SEP)['image'])
    rng = np.random.default_rng(5)
    reds = sum(_is_red(FR.preprocess_vcr(rec, cfg, rng, sep_tokens=SEP)['image']) for _ in range(200))
    assert 60 < reds < 140, reds                                 # 200 fair draws: 100 +- 5.7 standard deviations of 7.07
    bits = FR.preprocess_vcr(rec, dict(cfg, do_random_scale=False), np.random.default_rng(0), sep_tokens=SEP, as_bf16_bits=True)['image']
    assert bits.dtype == np.uint16 and np.array_equal(bits, R.bf16_bits(out['image']))


def test_missing_vocabulary_names_the_argument(monkeypatch):
    monkeypatch.delenv('MRESERVE_TOKENIZER_JSON', raising=False)
    import merlot_reserve_amd.modeling as M

    def no_vocab(path=None):
        raise FileNotFoundError('tokenizer vocabulary not found')
    monkeypatch.setattr(M, 'get_encoder', no_vocab)
    with pytest.raises(FileNotFoundError, match='sep_tokens'):
        FR.preprocess_vcr(_vcr_record(), R.merged_data_config(vcr_cfg()), np.random.default_rng(0))
    with pytest.raises(NotImplementedError, match='singleimg_jointoptions'):
        next(FR.finetune_input_fn_builder(vcr_cfg(), 'singleimg_jointoptions'))
    with pytest.raises(NotImplementedError, match='singleimg_linearqaoptions'):
        next(FR.finetune_val_input_fn_builder(vcr_cfg(), 'singleimg_linearqaoptions'))


# ---------------------------------------------------------------------------------------------------- 2. a TVQA record with a known answer
SUBS = [[500 + k] * 10 for k in range(7)]
SUBS[2] = []                                                     # a frame without subtitle
QUERY, CHOICES = [600, 601, 602, 603], [[700, 701], [710], [720, 721, 722]]


def _tvqa_record(num_frames=5):
    rng = np.random.default_rng(3)
    feats = {'id': b'123~4', 'magic_number': np.float32(25.0), 'qa_label': 1, 'num_frames': num_frames, 'qa_query': QUERY}
    for i, c in enumerate(CHOICES):
        feats[f'qa_choice_{i}'] = c
    for k in range(7):
        frame = np.full((48, 72, 3), 40 + 20 * k, np.uint8)
        feats[f'c{k:02d}/image_encoded'] = _jpeg(frame, 'RGB')
        feats[f'c{k:02d}/spec_encoded'] = _jpeg(np.clip(rng.normal(110, 40, size=(180, 65)), 1, 255).astype(np.uint8), 'L')
        feats[f'c{k:02d}/sub'] = SUBS[k]
    return R.make_example(feats)


def _expected_stream(option, per_segment, T):
    toks, segs = list(option), [0] * len(option)
    for k, row in enumerate(per_segment):
        toks += list(row)
        segs += [k + 1] * len(row)
    toks, segs = toks[:T], segs[:T]
    return np.array([toks + [0] * (T - len(toks)), segs + [0] * (T - len(segs))]).T


def test_tvqa_record_with_known_answer():
    cfg = R.merged_data_config(tvqa_cfg())
    T, a_tok = 64, cfg['audio_token_length']
    rec = _tvqa_record(num_frames=5)
    out = FR.preprocess_tvqa(rec, dict(cfg, do_random_scale=False), np.random.default_rng(0), sep_tokens=SEP)
    assert out['id'] == '123~4' and int(out['labels']) == 1
    assert out['images'].shape == (7, 24, 768) and out['audio_clips'].shape == (7, 3, 60, 65)
    assert out['textonly_seqs'].shape == out['audio_seqs'].shape == (3, T, 2) and out['textonly_seqs'].dtype == np.int32
    for i, c in enumerate(CHOICES):
        option = QUERY + SEP['qa'] + c + [MASK]
        want_text = _expected_stream(option, SUBS, T)
        want_audio = _expected_stream(option, [[AUDIOSPAN] * (3 * a_tok)] * 7, T)
        assert np.array_equal(out['textonly_seqs'][i], want_text), i
        assert np.array_equal(out['audio_seqs'][i], want_audio), i
        assert len(option) + sum(len(s) for s in SUBS) > T and want_text[-1, 0] != 0        # the text stream is cut at T ...
        assert want_audio[-1].tolist() == [AUDIOSPAN, (T - 1 - len(option)) // (3 * a_tok) + 1]    # ... and so is the audio stream, inside a span
    segs = out['textonly_seqs'][0][:, 1].tolist()
    assert 2 in segs and 4 in segs and 3 not in segs, 'frame 2 has no subtitle: segment 3 does not occur'
    # frames / clips 5 and 6 are exactly zero but for the last mel column, which is 1 everywhere
    assert float(np.abs(out['images'][5:]).max()) == 0.0 and float(np.abs(out['images'][:5]).min()) > 0.0
    assert float(np.abs(out['audio_clips'][5:, ..., :-1]).max()) == 0.0 and float(np.abs(out['audio_clips'][:5, ..., :-1]).sum()) > 0.0
    assert np.all(out['audio_clips'][..., -1] == 1.0)
    # a long option is cut to T - 1 tokens before MASK
    long = R.parse_example(rec)
    long['qa_query'] = np.arange(1000, 1100)
    cut = FR.preprocess_tvqa(long, dict(cfg, do_random_scale=False), np.random.default_rng(0), sep_tokens=SEP)
    assert cut['textonly_seqs'][0, :, 0].tolist() == list(range(1000, 1000 + T - 1)) + [MASK] and not cut['textonly_seqs'][0, :, 1].any()
    # a token id 0 inside a subtitle is refused
    bad = R.parse_example(rec)
    bad['c01/sub'] = np.array([5, 0, 7])
    with pytest.raises(AssertionError, match='token id 0'):
        FR.preprocess_tvqa(bad, dict(cfg, do_random_scale=False), np.random.default_rng(0), sep_tokens=SEP)


def test_tvqa_audio_shift_is_a_window_of_the_input():
    cfg = R.merged_data_config(tvqa_cfg())
    rec = _tvqa_record(num_frames=5)
    plain = FR.preprocess_tvqa(rec, dict(cfg, do_random_scale=False), np.random.default_rng(0), sep_tokens=SEP)['audio_clips']
    giant = plain[:5].reshape(-1, 65)[:, :64]                    # the valid rows as decoded (the last column is overwritten by 1)
    starts = set()
    for seed in range(12):
        out = FR.preprocess_tvqa(rec, cfg, np.random.default_rng(seed), sep_tokens=SEP)['audio_clips']
        assert out.shape == (7, 3, 60, 65) and np.all(out[..., -1] == 1.0) and float(np.abs(out[5:, ..., :-1]).max()) == 0.0
        rows = out[:5].reshape(-1, 65)[:, :64]                   # row j = padded[s + j]; padded[4 + i] = giant[i]
        fits = []
        for s in range(5):
            j = np.arange(max(0, 4 - s), len(giant))
            j = j[j + s - 4 < len(giant)]
            if np.array_equal(rows[j], giant[j + s - 4]):
                fits.append(s)
        assert len(fits) == 1, (seed, fits)
        s = fits[0]
        if s < 4:                                                # the rows in front of the sequence are Gaussian draws, not input rows
            assert not np.array_equal(rows[:4 - s], giant[:4 - s])
        starts.add(s)
    assert len(starts) >= 3 and starts <= set(range(5)), starts


# ---------------------------------------------------------------------------------------------------- 3. the builders over 3 shards x 5 records
@pytest.fixture(scope='module')
def shards(tmp_path_factory):
    d = tmp_path_factory.mktemp('vcr_shards')
    cfg = vcr_cfg()
    keys = FR.write_synthetic_shards(cfg, 'vcr', str(d), seed=1, train=(3, 5), val=(3, 5))
    cfg['data'].update(keys)
    cfg['device'] = dict(cfg.get('device', {}), batch_size=4)
    val_ids = [f'val-{i}' for i in range(15, 30)]                # write_synthetic_shards numbers the train records first
    return cfg, val_ids


def _same(a, b):
    import torch
    return torch.equal(a, b) if isinstance(a, torch.Tensor) else np.array_equal(a, b)


def test_val_builder_order_padding_and_rank_slices(shards):
    import torch
    cfg, val_ids = shards
    batches = list(FR.finetune_val_input_fn_builder(cfg, 'vcr', sep_tokens=SEP))
    assert len(batches) == 4
    ids = [i for b_ids, _b in batches for i in b_ids]
    assert ['-'.join(i.split('-')[:2]) for i in ids[:15]] == val_ids and ids[15:] == ['pad']          # every id once, in file order
    for b_ids, b in batches:
        assert len(b_ids) == 4 and b['image'].shape == (4, 24, 768) and b['image'].dtype == torch.bfloat16
        assert b['answers'].shape == (4, 2, 4, 16) and b['answers'].dtype == np.int32 and b['labels'].shape == (4, 2)
    last = batches[-1][1]
    assert not last['answers'][3].any() and not last['labels'][3].any() and float(last['image'][3].float().abs().max()) == 0.0
    assert last['answers'][2].any()
    # two ranks: their slices partition each batch
    r0 = list(FR.finetune_val_input_fn_builder(cfg, 'vcr', rank=0, world=2, sep_tokens=SEP))
    r1 = list(FR.finetune_val_input_fn_builder(cfg, 'vcr', rank=1, world=2, sep_tokens=SEP))
    assert len(r0) == len(r1) == 4
    for (ids_a, a), (ids_b, b), (ids_f, full) in zip(r0, r1, batches):
        assert ids_a + ids_b == ids_f and len(ids_a) == 2
        for k in full:
            assert _same(a[k], full[k][:2]) and _same(b[k], full[k][2:]), k
    # a thread pool yields the same batches
    pooled = list(FR.finetune_val_input_fn_builder(cfg, 'vcr', workers=2, processes=False, sep_tokens=SEP))
    assert [i for i, _b in pooled] == [i for i, _b in batches] and all(_same(p[1][k], q[1][k]) for p, q in zip(pooled, batches) for k in q[1])
    fp32 = dict(cfg, model=dict(cfg['model'], use_bfloat16=False))
    assert next(FR.finetune_val_input_fn_builder(fp32, 'vcr', sep_tokens=SEP))[1]['image'].dtype == torch.float32


def test_train_builder_drops_the_remainder_and_is_reproducible(shards):
    cfg, _val_ids = shards
    run = lambda **kw: list(FR.finetune_input_fn_builder(cfg, 'vcr', seed=11, epochs=1, sep_tokens=SEP, **kw))
    a = run(workers=0)
    assert len(a) == 3                                           # 15 records, batches of 4: the remainder of 3 is dropped
    ids = [i for b_ids, _b in a for i in b_ids]
    assert 'pad' not in ids and len(set(ids)) == 12 and all(i.startswith('train-') for i in ids)
    assert ids != sorted(ids, key=lambda i: int(i.split('-')[1])), 'the shuffle buffer reorders the records'
    for mode in (dict(workers=0), dict(workers=2, processes=False), dict(workers=2, processes=True)):
        b = run(**mode)
        assert [i for i, _b in b] == [i for i, _b in a], mode
        assert all(_same(x[1][k], y[1][k]) for x, y in zip(a, b) for k in x[1]), mode
    assert [i for i, _b in FR.finetune_input_fn_builder(cfg, 'vcr', seed=12, epochs=1, workers=0, sep_tokens=SEP)] != [i for i, _b in a]
    # rank r of 2 reads the files i with i mod 2 == r; its batch is device.batch_size // world
    r1 = list(FR.finetune_input_fn_builder(cfg, 'vcr', rank=1, world=2, seed=11, epochs=1, workers=0, sep_tokens=SEP))
    assert len(r1) == 2 and all(len(i) == 2 and {int(x.split('-')[1]) // 5 for x in i} == {1} for i, _b in r1)
    # skip_batches resumes the seed's stream; the stream goes on over the epochs
    two = list(FR.finetune_input_fn_builder(cfg, 'vcr', seed=11, epochs=2, workers=0, sep_tokens=SEP))
    assert len(two) == 6 and [i for i, _b in two[:3]] == [i for i, _b in a]
    for skip in (1, 4):
        rest = list(FR.finetune_input_fn_builder(cfg, 'vcr', seed=11, epochs=2, workers=0, sep_tokens=SEP, skip_batches=skip))
        assert [i for i, _b in rest] == [i for i, _b in two[skip:]]
        assert all(_same(x[1][k], y[1][k]) for x, y in zip(rest, two[skip:]) for k in x[1])
    assert FR._workers(64) == 16 and FR.DEFAULT_WORKERS <= 16


# ---------------------------------------------------------------------------------------------------- 4. the planners take what the readers give
def test_planners_accept_reader_batches_with_a_padded_example(shards, tmp_path):
    from merlot_reserve_amd.finetune import VCRDims, build_vcr_plan
    from merlot_reserve_amd.planner import build_tvqa_plan
    from merlot_reserve_amd.tvqa import TVQADims
    cfg, _ = shards
    _ids, last = list(FR.finetune_val_input_fn_builder(cfg, 'vcr', sep_tokens=SEP))[-1]
    d = VCRDims(cfg, 4)
    plan = build_vcr_plan(last['answers'], d)
    code = plan['joint_code'].reshape(d.n, d.Sj)
    assert (code[3 * 8:, :d.T] == -1).all() and (code[3 * 8:, d.T:] == 0).all() and (code[:3 * 8, 0] == 0).all()      # the padded example: no valid token
    assert (plan['pool_pos'][3 * 8:] == 0).all() and (plan['pool_pos'][:3 * 8] > 0).all()
    tcfg = tvqa_cfg(nseg=3)
    tcfg['data'].update(FR.write_synthetic_shards(tcfg, 'tvqa', str(tmp_path), seed=2, train=(1, 1), val=(1, 3)))
    tcfg['device'] = dict(tcfg.get('device', {}), batch_size=2)
    batches = list(FR.finetune_val_input_fn_builder(tcfg, 'tvqa', sep_tokens=SEP))
    assert [i for i, _b in batches] == [['1~0', '2~0'], ['3~0', 'pad']]
    b = batches[-1][1]
    assert b['images'].shape == (2, 3, 24, 768) and b['audio_clips'].shape == (2, 3, 3, 60, 65) and b['labels'].shape == (2,)
    assert b['textonly_seqs'].shape == b['audio_seqs'].shape == (2, 3, 64, 2)
    td = TVQADims(tcfg, 2)
    tplan = build_tvqa_plan(b['textonly_seqs'], b['audio_seqs'], td)
    tcode = tplan['joint_code'].reshape(td.n, td.Sj)
    pad_rows = [s * td.A * td.B + td.A + a for s in range(2) for a in range(td.A)]       # example 1 of both streams
    assert (tcode[pad_rows, :td.T] == -1).all() and (tcode[pad_rows, td.T:] == 0).all()
    ids, tb = next(FR.finetune_input_fn_builder(dict(tcfg, device=dict(tcfg['device'], batch_size=1)), 'tvqa', seed=0, epochs=1, workers=0, sep_tokens=SEP))
    assert ids == ['0~0'] and np.all(tb['audio_clips'][..., -1].float().numpy() == 1.0)
    build_tvqa_plan(tb['textonly_seqs'], tb['audio_seqs'], TVQADims(tcfg, 1))


def test_reference_import_name():
    import finetune.common_dataloader as C
    assert C.finetune_input_fn_builder is FR.finetune_input_fn_builder and C.finetune_val_input_fn_builder is FR.finetune_val_input_fn_builder
    assert C.preprocess_vcr is FR.preprocess_vcr and C.preprocess_tvqa is FR.preprocess_tvqa
