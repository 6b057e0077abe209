"""The finetuning driver (merlot_reserve_amd/finetune_train.py, driver.py), the validation arithmetic and the prediction files (finetune_eval.py) on the host:
the per-task config overrides, the step counts, the epoch / restart cadence, the lagged log, the `--gpus N` child command, accuracies with 'pad'
skipping, and the VCR CSV / TVQA JSON writers against hand-written text.  Nothing here touches a GPU."""
import json
import os
import types
import zipfile

import numpy as np
import pytest
import torch
import yaml

from merlot_reserve_amd import driver
from merlot_reserve_amd import finetune_eval as E
from merlot_reserve_amd import finetune_train as FT
from merlot_reserve_amd.config import load_config, tiny_config


def _args(*argv):
    return FT.build_parser().parse_args(list(argv))


# ---------------------------------------------------------------------------------------------------- arguments and config overrides
def test_vcr_overrides_are_the_scripts():
    args = _args('vcr', 'base', '', '-lr', '2e-5', '-ne', '3')
    assert (args.output_grid_h, args.output_grid_w, args.gpus, args.scan_minibatch, args.max_steps, args.val_batch_size) == (12, 20, 1, False, None, None)
    base = load_config('base')
    cfg = FT.task_overrides(base, 'vcr', args)
    assert base['data'].get('num_answers') != 4 or base['data']['lang_seq_len'] != 144, 'the given config is not modified'
    d, dev = cfg['data'], cfg['device']
    assert (d['num_answers'], d['random_scale_max'], d['random_scale_min'], d['lang_seq_len'], d['num_train_files']) == (4, 1.1, 1.0, 144, 256)
    assert 'train_fns' not in d and 'train_fns' in base['data'], "the pretraining shards are not the task's"
    with_dir = FT.task_overrides(base, 'vcr', _args('vcr', 'base', '', '--data-dir', '/data/vcr'))['data']
    assert with_dir['train_fns'] == '/data/vcr/train{:03d}of256.tfrecord' and (with_dir['val_fns'], with_dir['num_val_files']) == ('/data/vcr/val{:03d}of008.tfrecord', 8)
    assert (dev['batch_size'], dev['prefetch_size'], dev['n_fns_per_cycle']) == (32, 0, 256)
    spe = 212736 // 32
    assert spe == 6648 and dev['iterations_per_loop'] == spe
    assert cfg['optimizer'] == {'beta_2': 0.98, 'eps': 1e-6, 'learning_rate': 2e-5, 'num_train_steps': 3 * spe, 'num_warmup_steps': spe // 2,
                                'use_bfloat16_adam': True, 'weight_decay_rate': 0.1, 'do_bias_correction': True}
    assert cfg['model']['output_grid'] == [12, 20] and d['num_segments'] == base['data']['num_segments']
    assert FT.task_overrides(base, 'vcr', _args('vcr', 'base', '', '-output_grid_h', '18', '-output_grid_w', '32'))['model']['output_grid'] == [18, 32]


def test_tvqa_overrides_are_the_scripts():
    cfg = FT.task_overrides(load_config('base'), 'tvqa', _args('tvqa', 'base', 'some/ckpt', '-lr', '5e-6', '-ne', '5', '-scan_minibatch'))
    d, dev = cfg['data'], cfg['device']
    assert (d['num_answers'], d['num_segments'], d['lang_seq_len'], d['random_scale_max'], d['random_scale_min']) == (5, 7, 256, 1.1, 1.0)
    spe = 122112 // 32
    assert spe == 3816 and dev['iterations_per_loop'] == spe and dev['batch_size'] == 32
    assert cfg['optimizer']['num_train_steps'] == 5 * spe and cfg['optimizer']['num_warmup_steps'] == 1908 and cfg['optimizer']['learning_rate'] == 5e-6
    # the loop ends at num_train_steps: the script's 100 extra steps are not reproduced
    st = FT.driver_settings(cfg, _args('tvqa', 'base', '', '-output_dir', 'x'))
    assert st['end_step'] == 5 * spe and st['epoch_every'] == spe and st['log_every'] == cfg['device'].get('commit_every_nsteps', 50)


def test_step_counts_from_ne_and_train_size(tmp_path):
    argv = ['vcr', 'base', '', '-ne', '2', '--train-size', '6', '--records-per-gpu', '2', '-output_dir', str(tmp_path)]
    args = _args(*argv)
    cfg = FT.task_overrides(load_config('base'), 'vcr', args)
    assert cfg['device']['batch_size'] == 2 and cfg['device']['iterations_per_loop'] == 3
    assert cfg['optimizer']['num_train_steps'] == 6 and cfg['optimizer']['num_warmup_steps'] == 1
    st = FT.driver_settings(cfg, args)
    assert st == {'output_dir': str(tmp_path), 'epoch_every': 3, 'log_every': cfg['device'].get('commit_every_nsteps', 50), 'end_step': 6,
                  'records_per_gpu': 2, 'val_batch_size': 2}
    assert FT.driver_settings(cfg, _args(*argv, '--max-steps', '4'))['end_step'] == 4
    assert FT.driver_settings(cfg, _args(*argv, '--max-steps', '100'))['end_step'] == 6
    assert FT.driver_settings(cfg, _args(*argv, '-val_batch_size', '8'))['val_batch_size'] == 8
    two = _args(*argv, '--gpus', '2')
    cfg2 = FT.task_overrides(load_config('base'), 'vcr', two)
    assert cfg2['device']['batch_size'] == 4 and cfg2['device']['iterations_per_loop'] == 1 and FT.driver_settings(cfg2, two)['records_per_gpu'] == 2
    assert FT.driver_settings(FT.task_overrides(load_config('base'), 'vcr', _args('vcr', 'base', '', '--gpus', '8', '-output_dir', 'x')),
                              _args('vcr', 'base', '', '--gpus', '8', '-output_dir', 'x'))['records_per_gpu'] == 4
    with pytest.raises(ValueError, match='holds no batch'):
        FT.task_overrides(load_config('base'), 'vcr', _args('vcr', 'base', '', '--train-size', '16'))
    cfg['device']['output_dir'] = ''
    with pytest.raises(ValueError, match='output directory'):
        FT.driver_settings(cfg, _args('vcr', 'base', ''))
    cfg['device']['output_dir'] = 'runs'
    assert FT.driver_settings(cfg, _args('vcr', 'base', '', '-output_name', 'a'))['output_dir'] == os.path.join('runs', 'a')


def test_epoch_and_restart_cadence():
    """Every epoch: checkpoint + validation; the restart file also at the end of a run that stops between two epochs."""
    epochs = [s for s in range(0, 11) if FT.epoch_due(s, 3)]
    assert epochs == [3, 6, 9]
    assert [s for s in range(1, 8) if FT.checkpoint_due(s, 3, 7)] == [3, 6, 7]
    assert [s for s in range(4, 7) if FT.checkpoint_due(s, 3, 6)] == [6]             # a resumed run keeps the cadence of the run's step count


# ---------------------------------------------------------------------------------------------------- the lagged log
@pytest.mark.parametrize('start,end,log_every', [(0, 7, 2), (3, 9, 4), (0, 3, 50), (5, 5, 2)])
def test_row_of_step_n_is_written_at_n_plus_log_every(start, end, log_every):
    written, events = [], []
    log = FT.LaggedLog(log_every, lambda s: {'step': s}, lambda row: (written.append(row['step']), events.append((row['step'], now[0]))), first_step=start)
    now = [None]
    for n in range(start, end):
        now[0] = n                                                # step n has just been enqueued
        log.pushed(n)
        assert written == list(range(start, max(start, n - log_every + 1)))
    now[0] = 'flush'
    log.flush(end)
    assert written == list(range(start, end))                    # every step once, in order
    for step, at in events:
        assert at == step + log_every if step + log_every < end else at == 'flush'


def test_metrics_ring_rows_and_a_stale_row():
    eng = types.SimpleNamespace(loss_acc=torch.zeros(2), dev=torch.device('cpu'), info_from=lambda la: {'loss': la[0], 'is_right': la[1]})
    ring = FT.MetricsRing(eng, depth=4)
    for s in range(3, 7):
        ring.push(s, info={'loss': 0.5 * s, 'is_right': 1.0}, lr_scale=0.1 * s)
    assert ring.row(4) == {'step': 4, 'loss': 2.0, 'is_right': 1.0, 'lr_scale': 0.1 * 4}
    ring.push(7, info={'loss': 0.0, 'is_right': 0.0})
    with pytest.raises(RuntimeError, match='holds step 7, expected 3'):
        ring.row(3)


def test_interval_ms_reports_once_per_interval_and_skips_epoch_work():
    class Ev:
        clock = [0.0]

        def __init__(self):
            self.t = Ev.clock[0]

        def synchronize(self):
            pass

        def elapsed_time(self, other):
            return other.t - self.t
    t = driver.IntervalTimer(10, Ev, 4, 'examples_per_sec', last_row_only=True)
    Ev.clock[0] = 60.0
    t.mark(12)
    t.mark(12)                                                       # no empty interval
    Ev.clock[0] = 90.0
    t.mark(13)                                                       # an epoch ends at 13: its interval is closed ...
    Ev.clock[0] = 5090.0                                             # ... five seconds of checkpoint and validation ...
    t.resume(13)                                                     # ... belong to no interval
    Ev.clock[0] = 5130.0
    t.mark(15)
    assert t.of(10) == {} and t.of(11) == {'ms_per_step': 30.0, 'examples_per_sec': 4 / 0.030} and t.of(12)['ms_per_step'] == 30.0 and t.of(13) == {}
    assert t.of(14) == {'ms_per_step': 20.0, 'examples_per_sec': 4 / 0.020}


def test_a_resumed_run_drops_the_rows_it_runs_again(tmp_path):
    fn = tmp_path / 'train_log.jsonl'
    fn.write_text(''.join(json.dumps({'step': s, 'loss': 1.0}) + '\n' for s in range(5)))
    assert FT.truncate_log(str(fn), lambda row: row['step'] < 3) == 2                     # killed after step 4, restart file at step 3
    assert [json.loads(line)['step'] for line in open(fn)] == [0, 1, 2]
    assert FT.truncate_log(str(fn), lambda row: row['step'] < 3) == 0 and FT.truncate_log(str(tmp_path / 'none.jsonl'), lambda row: True) == 0
    val = tmp_path / 'val_log.jsonl'
    val.write_text(''.join(json.dumps({'step': s}) + '\n' for s in (3, 6)))
    assert FT.truncate_log(str(val), lambda row: row['step'] <= 3) == 1 and [json.loads(line)['step'] for line in open(val)] == [3]


# ---------------------------------------------------------------------------------------------------- --gpus N
def test_gpus_builds_a_child_launch_and_touches_no_gpu(tmp_path, monkeypatch):
    import subprocess
    import sys
    fn = tmp_path / 'tiny.yaml'
    fn.write_text(yaml.dump(tiny_config()))
    seen = {}

    def fake_run(cmd, env=None, **kw):
        seen['cmd'], seen['env'] = cmd, env
        return types.SimpleNamespace(returncode=0)
    monkeypatch.setattr(subprocess, 'run', fake_run)
    for name in ('execv', 'execve', 'execvp', 'execvpe', 'execl', 'execle', 'execlp', 'execlpe'):
        monkeypatch.setattr(os, name, lambda *a, **k: pytest.fail('the driver must start a child, never replace its own program'))
    monkeypatch.delenv('WORLD_SIZE', raising=False)
    argv = ['vcr', str(fn), '', '-output_dir', str(tmp_path / 'out'), '--synthetic-shards', str(tmp_path / 'shards'), '--gpus', '2', '--max-steps', '3']
    assert FT.main(argv) == 0
    cmd = seen['cmd']
    assert cmd[:3] == [sys.executable, '-m', 'torch.distributed.run'] and '--nproc-per-node=2' in cmd and '--nnodes=1' in cmd
    i = cmd.index('merlot_reserve_amd.finetune_train')
    assert cmd[i - 1] == '-m' and cmd[i + 1:] == argv                # the ranks run this module with the same arguments
    assert int(cmd[cmd.index('--master-port') + 1]) > 0
    assert not torch.cuda.is_initialized()                           # the parent has not touched the GPU
    assert not (tmp_path / 'out').exists() and not (tmp_path / 'shards').exists()      # ... nor started the run itself
    assert driver.launch_command('merlot_reserve_amd.finetune_train', ['a'], 8, 1234)[3:8] == ['--nnodes=1', '--nproc-per-node=8', '--master-addr', '127.0.0.1', '--master-port']


# ---------------------------------------------------------------------------------------------------- validation arithmetic
def test_vcr_val_epoch_counts_and_skips_pad():
    logp = torch.log_softmax(torch.arange(16, dtype=torch.float32).reshape(2, 2, 4), -1)
    batches = [(['val-1-a_0', 'val-2-a_1'], {'labels': np.array([[3, 3], [0, 3]])}),
               (['val-3-a_2', 'pad'], {'labels': np.array([[1, 2], [0, 0]])})]
    preds = iter([{'preds': torch.tensor([[3, 0], [0, 3]]), 'logprobs': logp}, {'preds': torch.tensor([[1, 1], [0, 0]]), 'logprobs': logp}])
    acc, rows = E.val_epoch(None, iter(batches), 'vcr', pred_fn=lambda batch: next(preds))
    assert [r['id'] for r in rows] == ['val-1-a_0', 'val-2-a_1', 'val-3-a_2']                 # the padded example (which would count as right) is skipped
    assert acc == {'qa_acc': 1.0, 'qar_acc': 1.0 / 3.0}
    assert rows[1] == {'id': 'val-2-a_1', 'preds': [0, 3], 'logprobs': logp[1].tolist(), 'labels': [0, 3]}
    assert E.accuracies(rows, 'vcr') == acc and all(np.isnan(v) for v in E.accuracies([], 'vcr').values())
    json.dumps(rows)


def test_tvqa_val_epoch_counts_and_skips_pad():
    lp = torch.log_softmax(torch.zeros(3, 5), -1)
    pred = {'preds_text': torch.tensor([1, 2, 0]), 'preds_audio': torch.tensor([4, 2, 0]), 'preds_joint': torch.tensor([1, 0, 0]),
            'logprobs_text': lp, 'logprobs_audio': lp}
    acc, rows = E.val_epoch(None, iter([(['7~0', '8~1', 'pad'], {'labels': np.array([1, 2, 0])})]), 'tvqa', pred_fn=lambda b: pred)
    assert len(rows) == 2 and acc == {'text_acc': 1.0, 'audio_acc': 0.5, 'joint_acc': 0.5}
    assert rows[0]['preds'] == {'text': 1, 'audio': 4, 'joint': 1} and rows[0]['labels'] == 1 and set(rows[0]['logprobs']) == {'text', 'audio'}


# ---------------------------------------------------------------------------------------------------- the prediction files
def test_predictions_jsonl_round_trip(tmp_path):
    rows = [{'id': 'a', 'preds': [1, 2], 'logprobs': [[-0.5, -1.25], [-2.0, -0.125]], 'labels': [1, 0]}]
    fn = E.write_predictions(rows, str(tmp_path / 'p.jsonl'))
    assert open(fn).read() == '{"id": "a", "preds": [1, 2], "logprobs": [[-0.5, -1.25], [-2.0, -0.125]], "labels": [1, 0]}\n'
    assert E.read_predictions(fn) == rows


def test_vcr_submission_csv(tmp_path):
    """Probabilities that are exact in fp32 (powers of two): the text is written by hand."""
    lp = lambda *p: [float(np.log(np.float32(x))) for x in p]
    rows = [{'id': 'test-10-qar_1', 'preds': [0, 0], 'labels': [0, 0], 'logprobs': [lp(0.5, 0.25, 0.125, 0.125), lp(0.25, 0.25, 0.25, 0.25)]},
            {'id': 'test-2-qar_1', 'preds': [0, 0], 'labels': [0, 0], 'logprobs': [lp(0.125, 0.125, 0.25, 0.5), lp(0.5, 0.125, 0.125, 0.25)]}]
    fn = E.write_vcr_submission(rows, str(tmp_path / 's.csv'))
    cols = [f'answer_{i}' for i in range(4)] + [f'rationale_conditioned_on_1_{i}' for i in range(4)]
    assert open(fn).read() == (','.join(['annot_id'] + cols) + '\n'
                               'test-2,0.125,0.125,0.25,0.5,0.5,0.125,0.125,0.25\n'             # sorted by the integer in the id: 2 before 10
                               'test-10,0.5,0.25,0.125,0.125,0.25,0.25,0.25,0.25\n')
    # an annotation seen under two conditionees fills both column groups; one that misses a group is refused
    both = [dict(rows[0], id='test-4-qar_0'), dict(rows[1], id='test-4-qar_3')]
    text = open(E.write_vcr_submission(both, str(tmp_path / 'b.csv'))).read().splitlines()
    assert text[0].split(',')[5:] == [f'rationale_conditioned_on_0_{i}' for i in range(4)] + [f'rationale_conditioned_on_3_{i}' for i in range(4)]
    assert text[1] == 'test-4,0.125,0.125,0.25,0.5,0.25,0.25,0.25,0.25,0.5,0.125,0.125,0.25' and len(text) == 2
    with pytest.raises(AssertionError, match='no value'):
        E.write_vcr_submission(both + [dict(rows[0], id='test-5-qar_0')], str(tmp_path / 'c.csv'))


def test_tvqa_submission_files(tmp_path):
    row = lambda i, t, a, j: {'id': i, 'preds': {'text': t, 'audio': a, 'joint': j}, 'logprobs': {'text': [], 'audio': []}, 'labels': 0}
    E.write_tvqa_submission({'val': [row('11~a', 1, 2, 3), row('12~b', 0, 4, 4)], 'test': [row('90~c', 2, 2, 1)]}, str(tmp_path), model_size='Base')
    want = {'text': ('{"11": 1, "12": 0}', '{"90": 2}', '(subtitles)'), 'audio': ('{"11": 2, "12": 4}', '{"90": 2}', '(audio)'),
            'joint': ('{"11": 3, "12": 4}', '{"90": 1}', '(subtitles and audio)')}
    for sub, (val, test, suffix) in want.items():
        assert open(tmp_path / sub / 'prediction_val.json').read() == val
        assert open(tmp_path / sub / 'prediction_test_public.json').read() == test
        assert json.load(open(tmp_path / sub / 'meta.json')) == {
            'model_name': f'MerlotReserve-Base {suffix}', 'is_ensemble': False, 'with_ts': True, 'show_on_leaderboard': True, 'author': 'Anonymous',
            'institution': 'Anonymous', 'description': f'A Base-sized model, given {suffix.strip("()")} at test time', 'paper_link': '', 'code_link': ''}
        with zipfile.ZipFile(tmp_path / f'{sub}.zip') as z:
            assert sorted(z.namelist()) == ['meta.json', 'prediction_test_public.json', 'prediction_val.json']
            assert z.read('prediction_val.json').decode() == val


def test_tvqa_submission_skips_a_split_that_was_not_run(tmp_path):
    row = {'id': '5~x', 'preds': {'text': 1, 'audio': 2, 'joint': 3}, 'logprobs': {'text': [], 'audio': []}, 'labels': 0}
    E.write_tvqa_submission({'val': [row]}, str(tmp_path), model_size='Large')
    for sub in ('text', 'audio', 'joint'):
        assert sorted(os.listdir(tmp_path / sub)) == ['meta.json', 'prediction_val.json']
        with zipfile.ZipFile(tmp_path / f'{sub}.zip') as z:
            assert sorted(z.namelist()) == ['meta.json', 'prediction_val.json']
    assert json.load(open(tmp_path / 'joint' / 'meta.json'))['model_name'] == 'MerlotReserve-Large (subtitles and audio)'
    with pytest.raises(AssertionError, match='unknown split'):
        E.write_tvqa_submission({'train': [row]}, str(tmp_path))


def test_predict_model_size_comes_from_the_flag_or_the_file_name():
    from merlot_reserve_amd import finetune_predict as P
    parse = lambda cfg, *more: P.build_parser().parse_args(['tvqa', cfg, 'ck', '-fns', 'v', '-num_files', '1', '-out', 'o', *more])
    assert P.model_size(parse('configs/base.yaml')) == 'Base' and P.model_size(parse('large')) == 'Large'
    assert P.model_size(parse('/data/database/large.yaml')) == 'Large', "a directory named '...base...' does not make the model Base"
    assert P.model_size(parse('mine.yaml', '--model-size', 'Base')) == 'Base'
    with pytest.raises(SystemExit):
        P.main(['vcr', 'base', 'ck', '-fns', 'v', '-num_files', '1', '-out', 'o', '-test_fns', 't', '-num_test_files', '1'])


def test_predict_config_points_at_the_given_shards():
    from merlot_reserve_amd import finetune_predict as P
    args = P.build_parser().parse_args(['tvqa', 'base', 'ck', '-fns', 'v{:03d}.tfrecord', '-num_files', '8', '-out', 'o.jsonl', '-val_batch_size', '16'])
    cfg = P.predict_config(load_config('base'), 'tvqa', args)
    assert cfg['data']['val_fns'] == 'v{:03d}.tfrecord' and cfg['data']['num_val_files'] == 8 and cfg['device']['batch_size'] == 16
    assert (cfg['data']['num_answers'], cfg['data']['num_segments'], cfg['data']['lang_seq_len']) == (5, 7, 256) and args.split == 'val'
