"""The pretraining driver and the held-out loss end to end on the GPU (tiny shapes): an interrupted and resumed run against an uninterrupted one,
a run fed from record shards, and merlot_reserve_amd.validate against the oracle's loss of the concatenated batch.  The driver runs as child
processes that end normally at --max-steps."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import yaml

from util import oracle_batch, oracle_draws, tree_to

from merlot_reserve_amd import checkpoint as C
from merlot_reserve_amd.config import tiny_config

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TIMING = ('ms_per_step', 'video_segments_per_sec')


def _config(tmp_path, **device):
    cfg = tiny_config(seq_len=80, lang_seq_len=40)
    cfg['optimizer'].update(num_warmup_steps=2, learning_rate=1e-3)
    cfg['device'] = dict(cfg.get('device', {}), iterations_per_loop=4, commit_every_nsteps=2, batch_size=2, **device)
    fn = tmp_path / 'tiny.yaml'
    fn.write_text(yaml.dump(cfg))
    return str(fn), cfg


def _drive(cfg_fn, out_dir, *extra):
    cmd = [sys.executable, '-m', 'merlot_reserve_amd.train', cfg_fn, '-output_dir', str(out_dir), '--seed', '3', *extra]
    p = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    print(p.stdout[-3000:])
    assert p.returncode == 0, p.stdout[-3000:]
    return p.stdout


def _log(out_dir):
    return [json.loads(line) for line in open(os.path.join(str(out_dir), 'train_log.jsonl'))]


def _leaves(tree, prefix=''):
    if isinstance(tree, dict):
        for k in sorted(tree):
            yield from _leaves(tree[k], f'{prefix}/{k}')
    else:
        yield prefix, tree


def _raw(fn):
    return C.msgpack_restore(open(fn, 'rb').read())


def test_resumed_run_is_bit_identical(dev, tmp_path):
    """A: 0 -> 8, saving at 4 and 8.  B: 0 -> 4 and ends.  C: resumes from B's directory, 4 -> 8.  A's and C's final checkpoints hold the same step,
    parameters and Adam moments bit for bit, and their log lines of steps 4..7 agree on every field but the timing ones."""
    cfg_fn, _cfg = _config(tmp_path)
    a, b = tmp_path / 'a', tmp_path / 'b'
    _drive(cfg_fn, a, '--synthetic', '--max-steps', '8')
    assert sorted(os.listdir(a)) == ['ckpt_4', 'ckpt_8', 'train_log.jsonl']
    _drive(cfg_fn, b, '--synthetic', '--max-steps', '4')
    assert sorted(os.listdir(b)) == ['ckpt_4', 'train_log.jsonl'] and [r['step'] for r in _log(b)] == [0, 1, 2, 3]
    out = _drive(cfg_fn, b, '--synthetic', '--max-steps', '8')
    assert 'at step 4' in out
    for name in ('ckpt_4', 'ckpt_8'):
        sa, sc = _raw(a / name), _raw(b / name)
        assert sa['step'] == sc['step'] == int(name.split('_')[1])
        la, lc = list(_leaves(sa)), list(_leaves(sc))
        assert [n for n, _ in la] == [n for n, _ in lc] and len(la) > 150
        for (n, x), (_n, y) in zip(la, lc):
            if isinstance(x, torch.Tensor):
                assert x.dtype == y.dtype and torch.equal(x.view(torch.uint8) if x.dim() else x, y.view(torch.uint8) if y.dim() else y), (name, n)
            else:
                assert x == y, (name, n)
        assert all(t.dtype == torch.float32 for _n, t in _leaves(sa['params']))                      # the exact restart file
        assert all(t.dtype == torch.bfloat16 for _n, t in _leaves(sa['opt_state']['0']['mu']))
    assert not torch.equal(_raw(a / 'ckpt_4')['params']['head']['kernel'], _raw(a / 'ckpt_8')['params']['head']['kernel'])      # the run trains
    log_a, log_c = _log(a), _log(b)
    assert [r['step'] for r in log_a] == [r['step'] for r in log_c] == list(range(8))
    for ra, rc in zip(log_a, log_c):
        assert set(ra) == set(rc) and set(TIMING) <= set(ra)
        for k in ra:
            if k not in TIMING:
                assert ra[k] == rc[k], (ra['step'], k, ra[k], rc[k])
        assert math.isfinite(ra['loss']) and ra['ms_per_step'] > 0
    assert {'loss', 'imgs_to_audio', 'text_to_audio', 'stuff_to_span', 'lr_scale', 'temperature/imgs_to_audio/log',
            'temperature/stuff_to_span/exp', '_stuff_to_span_from_random_text'} <= set(log_a[0])
    assert log_a[0]['lr_scale'] == 0.0 and log_a[1]['lr_scale'] == 0.5


def test_reference_format_resume(dev, tmp_path):
    """--reference-format: the restart file holds fp16 parameter leaves (what tests/test_checkpoint.py pins for the reference's format); a run resumed
    from it starts at the saved step and completes with finite losses.  It is fp16-rounded, not exact: nothing closer is claimed."""
    cfg_fn, _cfg = _config(tmp_path)
    d = tmp_path / 'ref'
    _drive(cfg_fn, d, '--synthetic', '--max-steps', '4', '--reference-format')
    raw = _raw(d / 'ckpt_4')
    assert all(t.dtype == torch.float16 for _n, t in _leaves(raw['params']))
    out = _drive(cfg_fn, d, '--synthetic', '--max-steps', '8', '--reference-format')
    assert 'at step 4' in out
    log = _log(d)
    assert [r['step'] for r in log] == list(range(8)) and all(math.isfinite(r['loss']) for r in log)
    sd = C.load_checkpoint(str(d))
    assert sd['step'] == 8 and int(sd['opt_state']['0']['count']) == 8


def test_driver_from_record_shards(dev, tmp_path):
    from merlot_reserve_amd import records as R
    cfg_fn, cfg = _config(tmp_path)
    rng = np.random.default_rng(9)
    for s in range(2):
        R.write_tfrecord(tmp_path / f'train{s:05d}of00002.tfrecord', [R.make_synthetic_record(cfg, rng) for _ in range(6)])
    cfg['data'] = dict(cfg['data'], train_fns=str(tmp_path / 'train{:05d}of00002.tfrecord'), num_train_files=2)
    cfg['device'] = dict(cfg['device'], iterations_per_loop=100, shuffle_buffer_size=4, n_fns_per_cycle=2)
    open(cfg_fn, 'w').write(yaml.dump(cfg))
    out = tmp_path / 'out'
    _drive(cfg_fn, out, '--max-steps', '6')
    log = _log(out)
    assert [r['step'] for r in log] == list(range(6)) and all(math.isfinite(r['loss']) and r['loss'] > 0 for r in log)
    assert sorted(os.listdir(out)) == ['ckpt_6', 'train_log.jsonl']
    sd = C.load_checkpoint(str(out))
    assert sd['step'] == 6 and sd['params']['head']['kernel'].dtype == torch.float32 and torch.isfinite(sd['params']['head']['kernel']).all()


def test_held_out_loss_of_the_concatenated_batch(dev, tmp_path, capsys):
    """merlot_reserve_amd.validate, num_accumulations = 2 passes of 2 synthetic records, against the oracle: pretrain_forward on each pass and the mean
    over r of loss_fn_given_preds([preds_0, preds_1], rank=r).  Tolerances: those of tests/test_pretrain_gpu.py::test_tiny_forward_and_loss_parity for
    the same quantities (2e-2 relative per objective and for the sum, 3e-2 relative + 1e-3 for the _stuff_to_span_from_* terms).  Without a tolerance:
    the megabatch loss differs from the mean of the single-pass losses (more negatives) in the direction the oracle shows."""
    from merlot_reserve_amd import validate as V
    from merlot_reserve_amd.params import ParamStore
    from merlot_reserve_amd.train import synthetic_batches
    from oracle import ref_torch as O
    cfg_fn, cfg = _config(tmp_path, output_dir='')
    cfg['device']['batch_size'] = 4
    open(cfg_fn, 'w').write(yaml.dump(cfg))
    B, seed = 2, 11
    store = ParamStore(cfg, dev, seed=4)
    ck = tmp_path / 'run'
    C.save_checkpoint({'step': 3, 'params': store.master_tree(), 'opt_state': None}, str(ck), no_optimizer=True, keep_fp32=True)
    assert V.main([cfg_fn, '-output_dir', str(ck), '-batch_size', str(B), '-max_num_megabatch', '1', '--synthetic', '--seed', str(seed)]) == 0
    lines = [json.loads(s) for s in capsys.readouterr().out.splitlines() if s.startswith('{')]
    assert [(r['dset'], r['nbatch'], r['nstep'], os.path.basename(r['ckpt'])) for r in lines] == [('val', 1, 3, 'ckpt_3'), ('train', 1, 3, 'ckpt_3')]
    params = tree_to(store.work_tree(), torch.float32)
    single = V.MegabatchLoss(cfg, B, store, dev, 1)
    for rec in lines:
        base = seed + (0 if rec['dset'] == 'train' else 1 << 30)
        passes = list(synthetic_batches(cfg, B, base, 0, 2))
        with torch.no_grad():
            preds = [O.pretrain_forward(params, cfg, oracle_batch({k: v for k, v in b.items() if k != '_draws'}), *oracle_draws(*b['_draws'])) for b in passes]
            per_rank = [O.loss_fn_given_preds(preds, rank=r) for r in range(2)]
            alone = [O.loss_fn_given_preds([p]) for p in preds]
        want = {k: sum(float(info[k]) for _l, info in per_rank) / 2 for k in per_rank[0][1]}
        want['loss'] = sum(float(l) for l, _i in per_rank) / 2
        print(rec['dset'], {k: (rec[k], want[k]) for k in want})
        for k in ('imgs_to_audio', 'text_to_audio', 'stuff_to_span', 'loss'):
            assert abs(rec[k] - want[k]) <= 2e-2 * abs(want[k]), (k, rec[k], want[k])
        for t in ('text2audio', 'audio2text', 'random_text'):
            k = f'_stuff_to_span_from_{t}'
            assert abs(rec[k] - want[k]) <= 3e-2 * abs(want[k]) + 1e-3, (k, rec[k], want[k])
        # more negatives: the megabatch loss against the mean of the two single-pass losses
        ours_alone = []
        for b in passes:
            b = dict(b, images=b['images'].to(dev), audio_clips=b['audio_clips'].to(dev))
            assert single.add_pass(b, b['_draws'])
            ours_alone.append(single.loss_info()['loss'])
        d_ours = rec['loss'] - sum(ours_alone) / 2
        d_oracle = want['loss'] - sum(float(l) for l, _i in alone) / 2
        print('megabatch - mean of single passes:', d_ours, d_oracle)
        assert d_ours != 0.0 and d_oracle != 0.0 and (d_ours > 0) == (d_oracle > 0)
