"""First-contact kit for the 8-GPU step (no hardware): Trainer._backward_reduce_update's collective PROGRAM at world = 8 for the base and
the large model, and the shared finetuning step's (finetune._backward_reduce_update) for the VCR and the TVQA engine, driven with a
recording communicator, recording streams and a stub engine on a layout-only ('meta') parameter store --
bucket sizes, order (one program order on one stream, as RCCL requires), the fraction of gradient bytes reduced after the last backward
kernel, and the 240-CU tile plan set around the part of backward that overlaps the buckets and restored after it.
Collectives of the reference being matched: pretrain/pretrain_model.py:290 (all_gather), :329 (pmean of the gradients), :336 (pmean of loss_info)."""
import contextlib

import pytest
import torch

from merlot_reserve_amd import ops
from merlot_reserve_amd.config import Dims, load_config
from merlot_reserve_amd.params import ParamStore
from merlot_reserve_amd.trainer import Trainer


class _Stream:
    def __init__(self, name, log):
        self.name, self.log = name, log

    def wait_stream(self, other):
        self.log.append(('wait', self.name, other.name))


class _Comm:
    capturable, backend = True, 'recording'

    def __init__(self, world, log, cur):
        self.world, self.rank, self.log, self.cur = world, 0, log, cur

    def allreduce_mean(self, t):
        self.log.append(('allreduce_mean', t.numel(), str(t.dtype).replace('torch.', ''), self.cur[0].name, ops.get_option('gemm_cus')))
        return t


class _Engine:
    """Calls layer_done the way TowerEngine.encoder_backward does: once per weight-gradient group, for every layer of the group."""

    def __init__(self, config, B, log, cur, streams):
        self.d, self.log, self.cur = Dims(config, B), log, cur
        self.side_stream = streams['side']

    def _on_side(self, fn):
        prev = self.cur[0]
        self.cur[0] = self.side_stream
        try:
            return fn()
        finally:
            self.cur[0] = prev

    def backward_stage_joint(self):
        self.log.append(('stage', 'joint', self.cur[0].name, ops.get_option('gemm_cus')))

    def backward_stage_audio(self):
        self.log.append(('stage', 'audio', self.cur[0].name, ops.get_option('gemm_cus')))

    def backward_stage_vision(self, layer_done=None):
        group = 2 if self.d.H <= 768 else 4
        self.log.append(('stage', 'vision', self.cur[0].name, ops.get_option('gemm_cus')))
        for hi in range(self.d.Lv, 0, -group):
            for l in range(hi - 1, max(hi - group, 0) - 1, -1):
                layer_done(l)


def _state(store, log, cur):
    class _State:
        f32_grads, shards = False, None

        def apply_range(self, lo, hi):
            log.append(('adam', lo, hi, cur[0].name))
    st = _State()
    st.store = store
    return st


def _recording(monkeypatch):
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
    monkeypatch.setattr(ops, 'nan_to_num_', lambda g: log.append(('nan_to_num', g.numel(), cur[0].name)))
    return log, cur, streams


def _program(monkeypatch, name, world):
    config = load_config(name)
    log, cur, streams = _recording(monkeypatch)
    tr = Trainer.__new__(Trainer)
    tr.config, tr.B, tr.rank, tr.world = config, 4, 0, world
    tr.params = ParamStore(config, 'meta', init=False)             # layout only: offsets, tower ranges, no storage
    tr.engine = _Engine(config, 4, log, cur, streams)
    tr.comm, tr.use_comm, tr.comm_stream = _Comm(world, log, cur), True, streams['comm']

    tr.state = _state(tr.params, log, cur)
    tr._make_buckets()
    before = ops.get_option('gemm_cus')
    tr._backward_reduce_update(update=True)
    assert ops.get_option('gemm_cus') == before, 'the 240-CU plan must be restored after backward'
    return tr, log


@pytest.mark.parametrize('name,nparams,last_frac', [('base', 316.4e6, (0.05, 0.12)), ('large', 853.1e6, (0.05, 0.14))])
def test_collective_program_at_world_8(monkeypatch, name, nparams, last_frac):
    tr, log = _program(monkeypatch, name, 8)
    keys = [str(b[0]) for b in tr.buckets]
    Lv = tr.engine.d.Lv
    assert keys == ['joint', 'audio', f"('vision', {Lv - Lv // 3})", f"('vision', {Lv - 2 * (Lv // 3)})", 'vision_end']
    # the buckets tile the flat gradient buffer exactly, each a whole number of Adam blocks
    assert sum(hi - lo for _, lo, hi in tr.buckets) == tr.params.total and abs(tr.params.total - nparams) / nparams < 0.01
    ar = [e for e in log if e[0] == 'allreduce_mean']
    # reduced in the order backward finishes them; audio rides behind the first vision bucket (it rarely ends before it)
    sizes = {str(k): hi - lo for k, lo, hi in tr.buckets}
    assert [e[1] for e in ar] == [sizes['joint'], sizes[keys[2]], sizes['audio'], sizes[keys[3]], sizes['vision_end']]
    assert tr.bucket_log == ['joint', tr.buckets[2][0], 'audio', tr.buckets[3][0], 'vision_end']
    assert all(e[2] == 'bfloat16' and e[3] == 'comm' for e in ar), 'every all-reduce on ONE stream in ONE program order, bf16 (pmean on bf16 grads, P:329)'
    # nan_to_num -> all-reduce -> Adam of the same range, per bucket, on the comm stream (P:328-329, O:180-190)
    seq = [e for e in log if e[0] in ('nan_to_num', 'allreduce_mean', 'adam')]
    for i in range(0, len(seq), 3):
        n2n, red, adam = seq[i:i + 3]
        assert (n2n[0], red[0], adam[0]) == ('nan_to_num', 'allreduce_mean', 'adam') and n2n[1] == red[1] == adam[2] - adam[1]
    # only the last bucket is reduced after the last backward kernel
    exposed = sizes['vision_end'] / tr.params.total
    assert last_frac[0] < exposed < last_frac[1], exposed
    # the 240-CU tile plan covers the stages that run beside a bucket in flight (audio + vision), not the joint stage before the first
    stages = {e[1]: e[3] for e in log if e[0] == 'stage'}
    assert stages == {'joint': 0, 'audio': 240, 'vision': 240}
    assert [e[4] for e in ar] == [0, 240, 240, 240, 240], 'the first bucket is handed over before the plan is switched'
    # the comm stream waits for the producer of each bucket; main joins side and comm at the end
    waits = [e for e in log if e[0] == 'wait']
    assert waits[-2:] == [('wait', 'main', 'side'), ('wait', 'main', 'comm')]
    assert ('wait', 'comm', 'side') in waits, "the audio bucket's producer is the side stream"


def test_single_rank_program_leaves_the_tile_plan_alone(monkeypatch):
    tr, log = _program(monkeypatch, 'base', 1)
    assert {e[1]: e[3] for e in log if e[0] == 'stage'} == {'joint': 0, 'audio': 0, 'vision': 0}


# ---- the finetuning step (finetune.finetune_train_step / FinetuneGraphStep): one stream walks engine.backward_stages() ----
def _finetune_program(monkeypatch, kind, world):
    import types

    from merlot_reserve_amd import finetune as F
    from merlot_reserve_amd.params import decay_finetune, tvqa_param_specs, vcr_param_specs
    from merlot_reserve_amd.tvqa import TVQAEngine
    config = load_config('base')
    engine_cls, specs = {'vcr': (F.VCREngine, vcr_param_specs), 'tvqa': (TVQAEngine, tvqa_param_specs)}[kind]
    log, cur, streams = _recording(monkeypatch)
    sets = []
    real_set = ops.set_option
    monkeypatch.setattr(ops, 'set_option', lambda name, value: (sets.append((name, value)), real_set(name, value))[1])
    store = ParamStore(config, 'meta', init=False, specs=specs(config), decay_rule=decay_finetune, with_orig=True)
    Lv, H = config['model']['vit_num_layers'], config['model']['hidden_size']

    class _Eng(engine_cls):
        """The real engine's bucket table and stage list on the layout; the stages themselves only log."""

        def __init__(self):
            self.p, self.d, self.dev, self.comm_stream = store, types.SimpleNamespace(Lv=Lv), 'meta', streams['comm']

        def _stage(self, name):
            log.append(('stage', name, cur[0].name, ops.get_option('gemm_cus')))

        def backward_stage_joint(self):
            self._stage('joint')

        def backward_stage_audio(self):
            self._stage('audio')

        def backward_stage_vision(self, layer_done=None):
            self._stage('vision')
            group = 2 if H <= 768 else 4
            for hi in range(Lv, 0, -group):
                for l in range(hi - 1, max(hi - group, 0) - 1, -1):
                    layer_done(l)
    eng = _Eng()
    state = _state(store, log, cur)
    state._model = types.SimpleNamespace(engine=eng, comm=_Comm(world, log, cur), params_store=store)
    before = ops.get_option('gemm_cus')
    F._backward_reduce_update(state)
    assert ops.get_option('gemm_cus') == before, 'the 240-CU plan must be restored after backward'
    return eng, store, log, sets


@pytest.mark.parametrize('kind,heads', [('vcr', ['joint']), ('tvqa', ['joint', 'audio'])])
def test_finetune_collective_program_at_world_8(monkeypatch, kind, heads):
    eng, store, log, sets = _finetune_program(monkeypatch, kind, 8)
    buckets, cuts = eng.gradient_buckets()
    Lv = eng.d.Lv
    keys = [b[0] for b in buckets]
    assert keys == heads + [('vision', Lv - Lv // 3), ('vision', Lv - 2 * (Lv // 3)), 'vision_end'] and len(keys) == len(heads) + 3
    assert eng.bucket_log == keys, 'handed over in the order backward finishes them'
    # the buckets tile the flat gradient buffer exactly, each a whole number of Adam blocks
    assert buckets[0][1] == 0 and buckets[len(heads)][2] == store.total and sum(hi - lo for _, lo, hi in buckets) == store.total
    assert all(lo % 2048 == 0 and hi % 2048 == 0 and lo < hi for _, lo, hi in buckets)
    # per bucket: the comm stream waits for the producer (main), then nan_to_num -> all-reduce -> Adam of the same range on the comm stream
    seq = [e for e in log if e[0] != 'stage']
    assert len(seq) == 4 * len(keys) + 1
    for i, (_key, lo, hi) in enumerate(buckets):
        wait, n2n, red, adam = seq[4 * i:4 * i + 4]
        assert wait == ('wait', 'comm', 'main')
        assert n2n == ('nan_to_num', hi - lo, 'comm') and red[:4] == ('allreduce_mean', hi - lo, 'bfloat16', 'comm') and adam == ('adam', lo, hi, 'comm')
    assert seq[-1] == ('wait', 'main', 'comm'), 'main joins the comm stream last'
    # the 240-CU tile plan covers the stages that run beside a bucket in flight, not the first stage and its bucket
    stages = [e for e in log if e[0] == 'stage']
    assert [e[1] for e in stages] == heads + ['vision'] and all(e[2] == 'main' for e in stages)
    assert [e[3] for e in stages] == [0] + [240] * (len(stages) - 1)
    assert [e[4] for e in log if e[0] == 'allreduce_mean'] == [0] + [240] * (len(keys) - 1)
    assert sets == [('gemm_cus', 240), ('gemm_cus', 0)], 'set once after the first bucket, restored once at the end'


@pytest.mark.parametrize('kind', ['vcr', 'tvqa'])
def test_finetune_single_rank_program_leaves_the_tile_plan_alone(monkeypatch, kind):
    eng, store, log, sets = _finetune_program(monkeypatch, kind, 1)
    assert sets == [], 'gemm_cus is never touched at world 1'
    assert all(e[3] == 0 for e in log if e[0] == 'stage') and len(eng.bucket_log) == len(eng.gradient_buckets()[0])
