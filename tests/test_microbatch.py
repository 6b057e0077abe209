"""Host side of the micro-batched step (merlot_reserve_amd/microbatch.py), no GPU: the slicing of a batch and its draws into K micro-batches, the
driver flag, and the collective PROGRAM of one step at world = 8, K = 4 with a recording communicator, recording streams and a stub engine on a
layout-only parameter store (the style of tests/test_multigpu_program.py)."""
import contextlib
import types

import numpy as np
import pytest
import torch

from merlot_reserve_amd import microbatch as MB
from merlot_reserve_amd import ops, train
from merlot_reserve_amd.config import Dims, load_config, tiny_config
from merlot_reserve_amd.params import ParamStore
from merlot_reserve_amd.planner import build_plan
from merlot_reserve_amd.synthetic import make_batch, make_draws


# ------------------------------------------------------------------------------------------------------------ slicing of batch and draws
def _host_trainer(cfg, B, K):
    tr = MB.MicroBatchTrainer.__new__(MB.MicroBatchTrainer)
    tr.config, tr.B, tr.K, tr.b = cfg, B, K, B // K
    tr.engine = types.SimpleNamespace(d=Dims(cfg, B // K))
    return tr


def _same_plan(a, b):
    assert set(a) == set(b)
    for k in a:
        if isinstance(a[k], np.ndarray):
            assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]), k
        else:
            assert a[k] == b[k], k


@pytest.mark.parametrize('B,K', [(4, 2), (6, 3), (4, 4), (3, 1)])
def test_plan_of_a_micro_batch_is_the_plan_of_its_records(B, K):
    """K independent batches of b records, concatenated record-major with their draws, are one batch of B records: plan m of the
    micro-batched trainer is build_plan of batch m with its own draws."""
    cfg = tiny_config(seq_len=80, lang_seq_len=40)
    b = B // K
    d = Dims(cfg, b)
    small = [make_batch(cfg, b, seed=40 + m) for m in range(K)]
    draws = [make_draws(cfg, b, seed=90 + m) for m in range(K)]
    big = {k: (np.concatenate if isinstance(small[0][k], np.ndarray) else torch.cat)([s[k] for s in small]) for k in small[0]}
    big_draws = ([np.concatenate([dr[0][i] for dr in draws]) for i in range(2)], np.concatenate([dr[1] for dr in draws]))
    tr = _host_trainer(cfg, B, K)
    want = [build_plan(small[m], d, draws[m][0], draws[m][1]) for m in range(K)]
    for plans in (tr.plan(big, big_draws), tr.plan(dict(big, _draws=big_draws))):
        assert len(plans) == K
        for m in range(K):
            _same_plan(plans[m], want[m])
    for m in range(K):
        mb = MB.slice_batch(dict(big, _draws=big_draws), m, b)
        assert '_draws' not in mb and all(len(v) == b for v in mb.values()) and torch.equal(mb['images'], small[m]['images'])
        sp, z = MB.slice_draws(big_draws, d, m, b)
        assert all(np.array_equal(x, y) for x, y in zip(sp, draws[m][0])) and np.array_equal(z, draws[m][1])
    # without draws: Trainer.plan's seed rule, applied to the micro-batch
    for m, p in enumerate(tr.plan(big)):
        seed = int(small[m]['audio2text/text_ptr'].astype(np.uint32).sum() % (2 ** 31))
        sp, z = make_draws(cfg, b, seed=seed)
        _same_plan(p, build_plan(small[m], d, sp, z))


# ------------------------------------------------------------------------------------------------------------ the driver flag
def test_driver_flag(tmp_path, monkeypatch):
    import yaml
    cfg = tiny_config()
    cfg['device'] = dict(cfg.get('device', {}), iterations_per_loop=4, commit_every_nsteps=2, batch_size=8)
    fn = tmp_path / 'tiny.yaml'
    fn.write_text(yaml.dump(cfg))
    parse = lambda *a: train.build_parser().parse_args([str(fn), '-output_dir', str(tmp_path / 'o'), *a])
    assert parse().micro_batches == 1 and 'micro_batches' not in train.driver_settings(cfg, parse())          # the default: the settings as they were
    st = train.driver_settings(cfg, parse('--micro-batches', '4'))
    assert st['micro_batches'] == 4 and st['records_per_gpu'] == 8
    assert train.driver_settings(cfg, parse('--gpus', '2', '--micro-batches', '2'))['records_per_gpu'] == 4
    for bad in (('--micro-batches', '3'), ('--records-per-gpu', '4', '--micro-batches', '8'), ('--micro-batches', '0')):
        with pytest.raises(ValueError):
            train.driver_settings(cfg, parse(*bad))

    # main(): the ValueError comes before any GPU call
    def no_gpu(*a, **k):
        raise AssertionError('a GPU call before the arguments were checked')
    monkeypatch.setattr(torch.cuda, 'set_device', no_gpu)
    with pytest.raises(ValueError, match='micro-batches'):
        train.main([str(fn), '-output_dir', str(tmp_path / 'o'), '--synthetic', '--records-per-gpu', '4', '--micro-batches', '3', '--max-steps', '2'])
    for kw in (dict(bf16_grads=False), dict(shard_optimizer=True)):
        with pytest.raises(ValueError):
            MB.MicroBatchTrainer(cfg, 4, 'cpu', micro_batches=2, **kw)
    with pytest.raises(ValueError):
        MB.MicroBatchTrainer(cfg, 4, 'cpu', micro_batches=3)


# ------------------------------------------------------------------------------------------------------------ the collective program
class _Stream:
    def __init__(self, name, log):
        self.name, self.log = name, log

    def wait_stream(self, other):
        self.log.append(('wait', self.name, other.name))


class _Comm:
    capturable, backend = True, 'recording'

    def __init__(self, world, log, cur):
        self.world, self.rank, self.log, self.cur = world, 0, log, cur

    @staticmethod
    def _dt(t):
        return str(t.dtype).replace('torch.', '')

    def gather_embeddings(self, E, E_all):
        self.log.append(('allgather', E.numel(), E_all.numel(), self._dt(E), self.cur[0].name))

    def scatter_grad(self, dE_all, out):
        assert dE_all.dtype == out.dtype
        self.log.append(('reducescatter', dE_all.numel(), out.numel(), self._dt(out), self.cur[0].name))

    def allreduce_mean(self, t):
        self.log.append(('allreduce_mean', t.numel(), self._dt(t), self.cur[0].name))
        return t


class _Engine:
    """The calls the step makes on PretrainEngine, logged; buffers on the 'meta' device (shapes only)."""

    def __init__(self, config, b, world, log, cur, streams):
        self.d, self.log, self.cur, self.world, self.rank = Dims(config, b), log, cur, world, 0
        d = self.d
        self.R = 2 * b * d.nseg + 2 * b * d.ntrg + b * (d.nspans - d.ntrg) + 2 * b * d.n_inc        # the sections of engine.PretrainEngine.sec
        z = lambda *s, dt=torch.bfloat16: torch.zeros(*s, dtype=dt, device='meta')
        self.E, self.dE = z(self.R, d.H), z(self.R, d.H)
        self.loss_acc, self.diag = z(3, dt=torch.float32), z(2, 6, dt=torch.float32)
        self._plan_views = {}
        self.side_stream = streams['side']

    def set_plan(self, plan):
        self._plan_views['t2sp_src'] = torch.zeros(self.d.Ns, dtype=torch.int32, device='meta')
        self.log.append(('set_plan', plan['m']))

    def _pl(self, k):
        return self._plan_views[k]

    def forward_device(self, images, audio):
        assert images.shape[0] == self.d.B and audio.shape[0] == self.d.B
        self.log.append(('forward',))

    def loss_and_grad_outputs(self, E_all, dE_all):
        assert E_all.shape == dE_all.shape == (self.world, self.R, self.d.H)
        self.log.append(('loss', self.rank))

    def _on_side(self, fn):
        prev = self.cur[0]
        self.cur[0] = self.side_stream
        try:
            return fn()
        finally:
            self.cur[0] = prev

    def _backward(self):
        self.log.append(('backward_plain',))

    def backward_stage_joint(self):
        self.log.append(('stage', 'joint', self.cur[0].name))

    def backward_stage_audio(self):
        self.log.append(('stage', 'audio', self.cur[0].name))

    def backward_stage_vision(self, layer_done=None):
        group = 2 if self.d.H <= 768 else 4
        self.log.append(('stage', 'vision', self.cur[0].name))
        for hi in range(self.d.Lv, 0, -group):
            for l in range(hi - 1, max(hi - group, 0) - 1, -1):
                layer_done(l)


def test_collective_program_at_world_8_with_4_micro_batches(monkeypatch):
    W, K, b = 8, 4, 2
    config = load_config('base')
    log, cur = [], [None]
    streams = {k: _Stream(k, log) for k in ('main', 'side', 'comm')}
    cur[0] = streams['main']
    monkeypatch.setattr(torch.cuda, 'current_stream', lambda *a, **k: cur[0])

    @contextlib.contextmanager
    def use(stream):
        prev, cur[0] = cur[0], stream
        try:
            yield
        finally:
            cur[0] = prev
    monkeypatch.setattr(torch.cuda, 'stream', use)
    monkeypatch.setattr(ops, 'nan_to_num_', lambda g: log.append(('nan_to_num', g.numel(), str(g.dtype), cur[0].name)))
    monkeypatch.setattr(ops, 'accumulate_rows', lambda src, dst, scale=1.0, accumulate=True:
                        log.append(('accumulate', src.numel(), str(dst.dtype), scale, cur[0].name)))
    monkeypatch.setattr(ops, 'axpby_', lambda y, x, a=1.0, b=1.0: log.append(('axpby', y.numel(), a, b)))
    monkeypatch.setattr(ops, 'cast_f32_to_bf16', lambda src, dst: log.append(('cast', src.numel())))

    tr = MB.MicroBatchTrainer.__new__(MB.MicroBatchTrainer)
    tr.config, tr.B, tr.K, tr.b, tr.rank, tr.world = config, K * b, K, b, 0, W
    tr.device = torch.device('meta')
    tr.params = ParamStore(config, 'meta', init=False)
    tr.params.enable_f32_grads()
    tr.engine = eng = _Engine(config, b, W * K, log, cur, streams)
    tr.comm, tr.use_comm, tr.comm_stream = _Comm(W, log, cur), True, streams['comm']
    tr.metrics_ring = 0

    class _State:
        f32_grads, shards, step = True, None, 0

        def prepare_step(self):
            pass

        def finish_step(self):
            self.step += 1

        def apply_range(self, lo, hi):
            log.append(('adam', lo, hi, cur[0].name))
    tr.state = _State()
    tr.state.store = tr.params
    tr._make_buckets()
    tr._make_step_buffers()
    d = eng.d
    batch = {'images': torch.zeros(K * b, d.nseg * d.hw, d.pp3, device='meta'), 'audio_clips': torch.zeros(K * b, d.nspans * d.a_raw, 65, device='meta')}
    before = ops.get_option('gemm_cus')
    tr.train_step(batch, plan=[{'m': m} for m in range(K)])
    assert ops.get_option('gemm_cus') == before and tr.state.step == 1

    R, H, total = eng.R, d.H, tr.params.total
    coll = [e for e in log if e[0] in ('allgather', 'reducescatter', 'allreduce_mean')]
    sizes = {str(k): hi - lo for k, lo, hi in tr.buckets}
    keys = [str(k) for k, _lo, _hi in tr.buckets]
    # ONE order: the all-gather of this rank's K x R x H embeddings, the fp32 reduce-scatter of the key gradients, then the fp32 bucket
    # all-reduces in Trainer's order (audio rides behind the first vision bucket)
    assert coll[0] == ('allgather', K * R * H, W * K * R * H, 'bfloat16', 'main')
    assert coll[1] == ('reducescatter', W * K * R * H, K * R * H, 'float32', 'main')
    assert [e[1] for e in coll[2:]] == [sizes['joint'], sizes[keys[2]], sizes['audio'], sizes[keys[3]], sizes['vision_end']]
    assert all(e[0] == 'allreduce_mean' and e[2] == 'float32' and e[3] == 'comm' for e in coll[2:]) and len(coll) == 2 + len(tr.buckets)
    assert tr.bucket_log == ['joint', tr.buckets[2][0], 'audio', tr.buckets[3][0], 'vision_end']
    # phase A: K forwards, each behind its own plan, all before the all-gather; phase B: the loss of virtual devices rank K + m, after it
    i_gather, i_scatter = log.index(coll[0]), log.index(coll[1])
    assert [e for e in log[:i_gather] if e[0] in ('set_plan', 'forward')] == [x for m in range(K) for x in (('set_plan', m), ('forward',))]
    assert [e for e in log[i_gather:i_scatter] if e[0] == 'loss'] == [('loss', m) for m in range(K)] and eng.rank == 0
    key_acc = [e for e in log[i_gather:i_scatter] if e[0] == 'accumulate']
    assert key_acc == [('accumulate', W * K * R * H, 'torch.float32', 1.0, 'main')] * K
    # phase C: K - 1 plain backwards, each accumulated whole with 1 / K; the bucket all-reduces come only behind the last of them
    tail = log[i_scatter:]
    plain = [i for i, e in enumerate(tail) if e[0] == 'backward_plain']
    assert len(plain) == K - 1 and len([e for e in tail if e[0] == 'forward']) == K
    first_ar = tail.index(coll[2])
    assert first_ar > plain[-1] and [e[0] for e in tail[:first_ar]].count('stage') == 1          # (the joint stage of the last micro-batch)
    assert [e for e in tail if e[0] == 'accumulate' and e[1] == total] == [('accumulate', total, 'torch.float32', 1.0 / K, 'main')] * (K - 1)
    assert [e for e in tail if e[0] == 'cast'] == [('cast', R * H)] * K
    # per bucket of the last micro-batch: accumulated on the producer's stream, then nan_to_num -> all-reduce -> Adam on the comm stream, in fp32
    seq = [e for e in tail[plain[-1]:] if e[0] in ('accumulate', 'nan_to_num', 'allreduce_mean', 'adam') and e[:2] != ('accumulate', total)]
    assert len(seq) == 4 * len(tr.buckets)
    for i in range(0, len(seq), 4):
        acc, n2n, red, adam = seq[i:i + 4]
        assert (acc[0], n2n[0], red[0], adam[0]) == ('accumulate', 'nan_to_num', 'allreduce_mean', 'adam')
        assert acc[1] == n2n[1] == red[1] == adam[2] - adam[1] and acc[3] == 1.0 / K and n2n[2] == 'torch.float32'
        assert acc[4] == ('side' if acc[1] == sizes['audio'] else 'main') and n2n[3] == red[3] == adam[3] == 'comm'
    assert [e for e in log if e[0] == 'wait'][-2:] == [('wait', 'main', 'side'), ('wait', 'main', 'comm')]
