"""The pretraining driver (merlot_reserve_amd/train.py, driver.py) and the step-metrics ring's bookkeeping (metrics.py), on the host: argument parsing and the YAML
keys, rows returned one drain late, a wrong stored step raises, the checkpoint cadence and the resume arithmetic with a fake trainer, the
`--gpus N` child command.  Nothing here touches a GPU."""
import json
import types

import pytest
import torch
import yaml

from merlot_reserve_amd import driver, train
from merlot_reserve_amd.config import tiny_config
from merlot_reserve_amd.engine import PretrainEngine
from merlot_reserve_amd.metrics import StepMetricsRing
from merlot_reserve_amd.trainer import Trainer

OBJECTIVES = [('imgs_to_audio',), ('text_to_audio',), ('stuff_to_span',)]


def _write_config(tmp_path, **device):
    cfg = tiny_config()
    cfg['device'] = dict(cfg.get('device', {}), **device)
    fn = tmp_path / 'tiny.yaml'
    fn.write_text(yaml.dump(cfg))
    return str(fn), cfg


# ---------------------------------------------------------------------------------------------------- arguments and YAML keys
def test_arguments_and_yaml_keys(tmp_path):
    fn, cfg = _write_config(tmp_path, output_dir=str(tmp_path / 'from_yaml'), iterations_per_loop=40, commit_every_nsteps=5, batch_size=8)
    args = train.build_parser().parse_args([fn])
    assert (args.config_file, args.output_dir, args.synthetic, args.gpus, args.seed, args.max_steps, args.reference_format) == (fn, '', False, 1, 0, None, False)
    st = train.driver_settings(cfg, args)
    assert st == {'output_dir': str(tmp_path / 'from_yaml'), 'ckpt_every': 40, 'log_every': 5, 'end_step': cfg['optimizer']['num_train_steps'], 'records_per_gpu': 8}
    args = train.build_parser().parse_args([fn, '-output_dir', 'elsewhere', '--synthetic', '--records-per-gpu', '3', '--max-steps', '12', '--gpus', '2',
                                            '--seed', '7', '--reference-format'])
    st = train.driver_settings(cfg, args)
    assert st['output_dir'] == 'elsewhere' and st['end_step'] == 12 and st['records_per_gpu'] == 3
    assert args.synthetic and args.gpus == 2 and args.seed == 7 and args.reference_format
    assert train.driver_settings(cfg, train.build_parser().parse_args([fn, '--gpus', '2']))['records_per_gpu'] == 4      # device.batch_size // gpus
    cfg['device'].pop('commit_every_nsteps')
    assert train.driver_settings(cfg, args)['log_every'] == 50                                                           # the reference's default
    cfg['device']['output_dir'] = ''
    with pytest.raises(ValueError):
        train.driver_settings(cfg, train.build_parser().parse_args([fn]))
    assert train.driver_settings(cfg, train.build_parser().parse_args([fn, '-output_dir', 'x', '--max-steps', '10000000']))['end_step'] == cfg['optimizer']['num_train_steps']


# ---------------------------------------------------------------------------------------------------- the metrics ring, host side
def _ring(depth, step=0):
    """A metrics ring on the CPU, without model or library, and the step count of the trainer it would belong to."""
    eng = types.SimpleNamespace(objectives=OBJECTIVES)
    t = StepMetricsRing(depth, 'cpu', lambda la, dg: PretrainEngine.info_from(eng, la, dg), len(OBJECTIVES) + 4)
    t.state = types.SimpleNamespace(step=step)
    return t


def _sources(step):
    la = [1.0 + step, 2.0 + 0.5 * step, 3.0 + 0.25 * step]
    dg = [[0.5 * step + i for i in range(3)] + [1.0, 2.0, 4.0], [0.25 * step + i for i in range(3)] + [2.0, 0.0, 8.0]]
    return la, dg, [2.5, 2.25, 2.0 - 0.125 * step], 0.1 * step


def _fake_step(t):
    """What one train_step does to the ring: the host count, and mr_metrics_push's effect written by hand."""
    t.begin_step(t.state.step)
    ring, steps, counter = t.tensors
    c = int(counter)
    la, dg, sc, lr = _sources(c)
    ring[c % t.depth] = torch.tensor(la + dg[0] + dg[1] + sc + [lr])
    steps[c % t.depth] = c
    counter += 1
    t.state.step += 1


def _expected(step):
    la, dg, sc, lr = _sources(step)
    f = lambda xs: torch.tensor(xs, dtype=torch.float32).tolist()
    row = {'step': step, **PretrainEngine.info_from(types.SimpleNamespace(objectives=OBJECTIVES), f(la), [f(dg[0]), f(dg[1])])}
    row['contrastive_scales'], row['lr_scale'] = f(sc), f([lr])[0]
    return row


@pytest.mark.parametrize('start', [0, 37])
def test_rows_come_back_one_drain_late(start):
    t = _ring(depth=8, step=start)
    for _ in range(4):
        _fake_step(t)
    assert t.drain() == []                                           # the first drain only starts a copy
    for _ in range(3):
        _fake_step(t)
    rows = t.drain()
    assert rows == [_expected(start + i) for i in range(4)]          # the rows of the PREVIOUS drain, derived like loss_info()
    assert set(rows[0]) == {'step', 'imgs_to_audio', 'text_to_audio', 'stuff_to_span', 'loss', '_stuff_to_span_from_text2audio',
                            '_stuff_to_span_from_audio2text', '_stuff_to_span_from_random_text', 'contrastive_scales', 'lr_scale'}
    for _ in range(4):                                               # rows wrap: steps start + 7 ... start + 10 reuse the slots of the first four
        _fake_step(t)
    assert [r['step'] for r in t.drain()] == [start + 4, start + 5, start + 6]
    assert t.drain(flush=True) == [_expected(start + i) for i in range(7, 11)]
    assert t.drain(flush=True) == [] and int(t.tensors[2]) == start + 11


def test_wrong_stored_step_raises():
    t = _ring(depth=8)
    for _ in range(4):
        _fake_step(t)
    t.tensors[1][2] = 10                                             # as if a later step had overwritten row 2
    t.drain()
    with pytest.raises(RuntimeError, match='row 2 holds step 10, expected 2'):
        t.drain()
    t = _ring(depth=8)
    t.begin_step(0)                                                  # a step whose push never ran: the row holds no step
    t.state.step += 1
    with pytest.raises(RuntimeError, match='expected 0'):
        t.drain(flush=True)


def test_depth_must_be_twice_the_drain_interval():
    t = _ring(depth=8)
    for _ in range(5):
        _fake_step(t)
    with pytest.raises(AssertionError, match='at most 4 steps between drains'):
        t.drain()
    with pytest.raises(AssertionError):
        _ring(depth=1)
    fake = types.SimpleNamespace(metrics_ring=6, state=types.SimpleNamespace(step=0))
    with pytest.raises(AssertionError, match='2 x the log interval'):
        train.run_loop(fake, iter(()), end_step=4, log_every=4, ckpt_every=2, save=None, write=None)
    with pytest.raises(AssertionError):
        Trainer.drain_metrics(types.SimpleNamespace(metrics_ring=0))


# ---------------------------------------------------------------------------------------------------- the loop with a fake trainer
class FakeTrainer:
    """Counts what the loop asks for; its ring is a real one."""

    def __init__(self, depth, step=0):
        self.ring = _ring(depth, step)
        self.state, self.metrics_ring = self.ring.state, depth
        self.calls = []

    def plan(self, batch, draws=None):
        return ('plan', batch['id'], draws)

    def train_step(self, batch, plan=None):
        assert plan == ('plan', batch['id'], batch.get('_draws'))
        self.calls.append(('eager', self.state.step, batch['id']))
        _fake_step(self.ring)

    def capture(self, batch):
        self.calls.append(('capture', self.state.step, batch['id']))

    def train_step_graph(self, batch, plan):
        assert any(c[0] == 'capture' for c in self.calls)
        self.calls.append(('graph', self.state.step, batch['id']))
        _fake_step(self.ring)

    def drain_metrics(self, flush=False):
        self.calls.append(('flush' if flush else 'drain', self.state.step, None))
        return self.ring.drain(flush=flush)


def _batches(first):
    i = first
    while True:
        yield {'id': i, '_draws': ('draws', i)}
        i += 1


@pytest.mark.parametrize('start,end', [(0, 8), (0, 4), (4, 8), (3, 7), (8, 8)])
def test_checkpoint_cadence_and_resume_arithmetic(start, end):
    tr = FakeTrainer(depth=4, step=start)
    saved, rows = [], []
    n = train.run_loop(tr, _batches(start), end_step=end, log_every=2, ckpt_every=4, save=saved.append, write=lambda row, timing: rows.append((row, timing)))
    assert n == end - start and tr.state.step == end
    assert saved == [s for s in range(start + 1, end + 1) if s % 4 == 0 or s == end]                # the cadence follows the RUN's step, also after a resume
    assert [r['step'] for r, _t in rows] == list(range(start, end)) and all(t is None for _r, t in rows)   # every step logged once, in order
    assert [r for r, _t in rows] == [_expected(s) for s in range(start, end)]
    steps = [c for c in tr.calls if c[0] in ('eager', 'graph')]
    assert [c[1:] for c in steps] == [(s, s) for s in range(start, end)]                            # step s consumes batch s
    if end > start:
        assert steps[0][0] == 'eager' and all(c[0] == 'graph' for c in steps[1:])                   # one eager step, then replays
        assert tr.calls[1] == ('capture', start + 1, start)
    drains = [c[1] for c in tr.calls if c[0] == 'drain']
    assert drains == [s for s in range(start + 1, end + 1) if (s - start) % 2 == 0 or s == end]     # every log_every steps and at the end
    assert tr.calls[-1] == ('flush', end, None)


def test_uncapturable_trainer_steps_eagerly():
    tr = FakeTrainer(depth=4)
    train.run_loop(tr, _batches(0), end_step=5, log_every=2, ckpt_every=100, save=lambda s: None, write=lambda r, t: None, use_graph=False)
    assert [c[0] for c in tr.calls if c[0] in ('eager', 'graph', 'capture')] == ['eager'] * 5


def test_log_record_fields():
    rec = train.log_record(_expected(3), {'ms_per_step': 29.5, 'video_segments_per_sec': 2169.0})
    assert rec['step'] == 3 and rec['lr_scale'] == _expected(3)['lr_scale'] and 'contrastive_scales' not in rec
    for name, v in zip(('imgs_to_audio', 'text_to_audio', 'stuff_to_span'), _expected(3)['contrastive_scales']):
        assert rec[f'temperature/{name}/log'] == v and rec[f'temperature/{name}/exp'] == pytest.approx(float(torch.tensor(v).exp()), rel=1e-6)
    assert set(train.TIMING_KEYS) <= set(rec)
    json.dumps(rec)


# ---------------------------------------------------------------------------------------------------- --gpus N
def test_gpus_builds_a_child_launch_and_touches_no_gpu(tmp_path, monkeypatch):
    import subprocess
    import sys
    fn, _cfg = _write_config(tmp_path, iterations_per_loop=4)
    seen = {}

    def fake_run(cmd, env=None, **kw):
        seen['cmd'], seen['env'] = cmd, env
        return types.SimpleNamespace(returncode=0)
    monkeypatch.setattr(subprocess, 'run', fake_run)
    monkeypatch.delenv('WORLD_SIZE', raising=False)
    argv = [fn, '-output_dir', str(tmp_path / 'out'), '--synthetic', '--gpus', '2', '--max-steps', '3']
    assert train.main(argv) == 0
    cmd = seen['cmd']
    assert cmd[:3] == [sys.executable, '-m', 'torch.distributed.run'] and '--nproc-per-node=2' in cmd and '--nnodes=1' in cmd
    i = cmd.index('merlot_reserve_amd.train')
    assert cmd[i - 1] == '-m' and cmd[i + 1:] == argv                # the ranks run this module with the same arguments
    assert int(cmd[cmd.index('--master-port') + 1]) > 0
    assert not torch.cuda.is_initialized()                           # the parent has not touched the GPU (and never execs)
    assert not (tmp_path / 'out').exists()                           # ... nor started the run itself
    assert driver.launch_command('merlot_reserve_amd.train', ['a'], 8, 1234)[3:8] == ['--nnodes=1', '--nproc-per-node=8', '--master-addr', '127.0.0.1', '--master-port']


def test_interval_timer_divides_an_interval_by_its_steps():
    class Ev:
        clock = [0.0]

        def __init__(self):
            self.t = Ev.clock[0]

        def synchronize(self):
            pass

        def elapsed_time(self, other):
            return other.t - self.t
    t = driver.IntervalTimer(100, Ev, 64, 'video_segments_per_sec')
    Ev.clock[0] = 150.0
    t.mark(105)
    t.mark(105)                                                      # the end of the run marks again: no empty interval
    Ev.clock[0] = 210.0
    t.mark(107)
    assert t.of(100) == t.of(104) == {'ms_per_step': 30.0, 'video_segments_per_sec': 64 / 0.030}
    assert t.of(105)['ms_per_step'] == 30.0 and t.of(106) is t.of(105) and t.of(107) == {}
