"""The micro-batched pretraining step (merlot_reserve_amd/microbatch.py) on the GPU, tiny shapes, against the oracle's virtual devices:
B = K b records stepped as K micro-batches are K reference devices of b records -- the mean over r of
R.loss_fn_given_preds([preds_0 .. preds_{K-1}], rank=r), preds_m = R.pretrain_forward of micro-batch m with its own draws.
(B, K) = (4, 2), (4, 4), (6, 3); b = 2 gives contrastive blocks that are no multiple of 8 rows.  One eager step and one oracle evaluation per
case are shared by the tests of that case (computed once, kept unchanged)."""
import json
import math
import os

import pytest
import torch
import yaml

from tests.util import oracle_batch, oracle_draws, relerr, tiny_setup, tree_to

pytestmark = pytest.mark.gpu

CASES = [(4, 2), (4, 4), (6, 3)]
IDS = [f'B{B}_K{K}' for B, K in CASES]
SECTIONS = (('imgs_to_audio', 'x', 'i2a_x'), ('imgs_to_audio', 'y', 'i2a_y'), ('text_to_audio', 'x', 't2a_x'),
            ('text_to_audio', 'y', 't2a_y'), ('text_to_audio', 'y_extra', 't2a_ye'), ('stuff_to_span', 'x', 's2s_x'),
            ('stuff_to_span', 'y', 's2s_y'))
_CACHE = {}


def _case(dev, B, K):
    """One eager step (update=False) of MicroBatchTrainer(B, K) with every forward's embeddings recorded, and the oracle's K devices on the same
    bf16-rounded weights, records and draws (parameters with requires_grad: the gradient tests differentiate through `preds`)."""
    if (B, K) in _CACHE:
        return _CACHE[(B, K)]
    from merlot_reserve_amd.microbatch import MicroBatchTrainer, slice_batch, slice_draws
    from oracle import ref_torch as R
    cfg, _store, batch, splits, z = tiny_setup(B=B, seed=3, device=dev)
    del _store
    tr = MicroBatchTrainer(cfg, B, dev, micro_batches=K, seed=3)
    eng = tr.engine
    plans = tr.plan(batch, (splits, z))
    seen, fwd = [], eng.forward_device

    def recording(*a):
        out = fwd(*a)
        seen.append(eng.E.clone())
        return out
    eng.forward_device = recording
    try:
        tr.train_step(batch, plan=plans, update=False)
        torch.cuda.synchronize()
    finally:
        del eng.forward_device
    c = dict(cfg=cfg, tr=tr, batch=batch, draws=(splits, z), plans=plans, seen=seen, E_loc=tr.E_loc.clone(), grad32=tr.params.grad32.clone(),
             info=tr.loss_info())
    b = B // K
    params = R.tree_map(lambda t: t.clone().requires_grad_(True), tree_to(tr.params.work_tree(), torch.float32))
    preds = []
    for m in range(K):
        sp, zz = slice_draws((splits, z), eng.d, m, b)
        preds.append(R.pretrain_forward(params, cfg, oracle_batch(slice_batch(batch, m, b)), *oracle_draws(sp, zz)))
    c.update(params=params, preds=preds, per_rank=[R.loss_fn_given_preds(preds, rank=r) for r in range(K)])
    _CACHE[(B, K)] = c
    return c


def _gradient_report(store, flat32, params, what):
    """Every leaf of the flat fp32 gradient buffer against the .grad of the oracle's parameters: the bound of
    tests/test_pretrain_gpu.py::test_tiny_backward_parity -- err <= 8e-2 |g| + 1.5e-2 max|g|, cosine >= 0.995 where |g| > 5e-2 max|g|."""
    from oracle import ref_torch as R
    gt = store._to_tree(flat32)
    leaves = [(n, t.grad if t.grad is not None else torch.zeros_like(t)) for n, t in R.tree_leaves(params)]
    gmax = max(float(g.norm()) for _, g in leaves)
    rows = []
    for name, g in leaves:
        mine = gt
        for part in name.split('/'):
            mine = mine[part]
        gn, err = float(g.norm()), float((mine.double() - g.double()).norm())
        cos = float((mine.double().flatten() @ g.double().flatten()) / (mine.double().norm() * g.double().norm() + 1e-30))
        rows.append((err / (8e-2 * gn + 1.5e-2 * gmax), err, gn, cos, name))
    rows.sort(reverse=True)
    print(f'{what}: gmax {gmax:.3e}; worst leaves (error / bound, error, |g|, cosine):')
    for r in rows[:8]:
        print(f'  {r[0]:.3f} {r[1]:.3e} {r[2]:.3e} {r[3]:.5f} {r[4]}')
    return [(n, e, gn, cos) for q, e, gn, cos, n in rows if q > 1 or (gn > 5e-2 * gmax and cos < 0.995)]


@pytest.mark.parametrize('B,K', CASES, ids=IDS)
def test_loss_is_the_mean_over_the_virtual_devices(dev, B, K):
    c = _case(dev, B, K)
    want = {k: sum(float(info[k].detach()) for _l, info in c['per_rank']) / K for k in ('imgs_to_audio', 'text_to_audio', 'stuff_to_span')}
    want['loss'] = sum(float(l.detach()) for l, _i in c['per_rank']) / K
    print({k: (c['info'][k], want[k]) for k in want})
    for k in want:
        assert abs(c['info'][k] - want[k]) <= 2e-2 * abs(want[k]), (k, c['info'][k], want[k])
    assert all(math.isfinite(v) for v in c['info'].values())


@pytest.mark.parametrize('B,K', CASES, ids=IDS)
def test_recomputed_embeddings_are_bit_equal(dev, B, K):
    """Phase C's forward of micro-batch m reproduces phase A's embeddings to the bit (the gradient of phase B belongs to exactly these values)."""
    c = _case(dev, B, K)
    assert len(c['seen']) == 2 * K
    for m in range(K):
        assert torch.equal(c['seen'][m].view(torch.int16), c['E_loc'][m].view(torch.int16)), m
        assert torch.equal(c['seen'][K + m].view(torch.int16), c['E_loc'][m].view(torch.int16)), m
    assert not torch.equal(c['E_loc'][0], c['E_loc'][1])


@pytest.mark.parametrize('B,K', CASES, ids=IDS)
def test_gradients_of_an_injected_upstream_gradient(dev, B, K):
    """Phase C alone: a well-scaled upstream gradient per micro-batch in place of phase B's (the check of test_tiny_backward_parity, which is
    independent of the conditioning of the loss at random init): grad32 = (1 / K) sum_m backward_m(dE_m), every leaf, under that test's bound.
    The gradient of the TRUE mean loss is not held to this bound: a random-init tower emits near-identical rows, the contrastive gradient is
    then a difference of near-equal vectors and is lost in bf16 (tests/test_pretrain_gpu.py::test_loss_gradient_wrt_outputs says the same of
    the one-device step).  Measured at B = 4, K = 2: max leaf norm 6.1e-3, worst leaf 156 x the bound, cosines 0.09 .. 0.38 on cls, cls_proj,
    head/kernel and the token table, while the loss itself agrees to 2e-2; the one-device Trainer(B=4) on the same records misses the same bound
    the same way (worst leaf 164 x, cosines 0.33 .. 0.64, 34 leaves outside).  So the chain is checked in its two halves: this test (phase C,
    phase B bypassed) and test_phase_b_on_well_conditioned_embeddings (phase B on unit-norm embeddings, 1e-2 relative on dE)."""
    from oracle import ref_torch as R
    c = _case(dev, B, K)
    tr, eng = c['tr'], c['tr'].engine
    Rr, H = eng.R, eng.d.H
    g = torch.Generator().manual_seed(1)
    dE = (torch.randn(K, Rr, H, generator=g) * 1e-2).to(torch.bfloat16)

    def inject():
        tr.loss_sum.zero_()
        tr.dK_own.view(K, Rr, H).copy_(dE.float().to(dev))            # (bf16 values: the cast of phase C returns them exactly)
    tr._phase_b = inject
    try:
        tr.train_step(c['batch'], plan=c['plans'], update=False)
        torch.cuda.synchronize()
    finally:
        del tr._phase_b
    for _n, t in R.tree_leaves(c['params']):
        t.grad = None
    total = 0.0
    for m in range(K):
        for k, k2, name in SECTIONS:
            o, n = eng.sec[name]
            total = total + (c['preds'][m][k][k2] * dE[m, o:o + n].float()).sum()
    (total / K).backward(retain_graph=True)
    bad = _gradient_report(tr.params, tr.params.grad32, c['params'], f'B {B} K {K}, injected dE')
    assert not bad, bad[:10]


@pytest.mark.parametrize('B,K', CASES, ids=IDS)
def test_phase_b_on_well_conditioned_embeddings(dev, B, K):
    """Phase B alone on unit-norm embeddings (tests/test_pretrain_gpu.py::test_two_rank_contrastive_path_on_one_gpu): the loss of every virtual
    device and the upstream gradient bf16-free sum dQ[m] + dK_own[m] against autograd of the sum of the oracle's K losses: 1e-2 relative per section."""
    from oracle import ref_torch as R
    c = _case(dev, B, K)
    tr, eng = c['tr'], c['tr'].engine
    Rr, H = eng.R, eng.d.H
    g = torch.Generator().manual_seed(10)
    E = torch.randn(K, Rr, H, generator=g)
    E = (E / E.norm(dim=-1, keepdim=True) * 1.6).to(torch.bfloat16)
    tr.E_loc.copy_(E.to(dev))
    tr._phase_b()
    torch.cuda.synchronize()
    Es = [E[m].float().requires_grad_(True) for m in range(K)]
    preds = []
    for m in range(K):
        p = {}
        for k, k2, name in SECTIONS:
            o, n = eng.sec[name]
            p.setdefault(k, {})[k2] = Es[m][o:o + n]
        p['stuff_to_span']['_sources'] = torch.as_tensor(c['plans'][m]['t2sp_src']).long()
        preds.append(p)
    losses = [R.loss_fn_given_preds(preds, rank=r) for r in range(K)]
    sum(l for l, _i in losses).backward()
    want = sum(float(l) for l, _i in losses) / K
    got = tr.loss_info()['loss']
    assert abs(got - want) <= 1e-3 * abs(want), (got, want)
    up = tr.dK_own.view(K, Rr, H)
    for m in range(K):
        for k, k2, name in SECTIONS:
            o, n = eng.sec[name]
            e = relerr(up[m, o:o + n], Es[m].grad[o:o + n])
            print(f'micro-batch {m} dE {name}: {e:.3e}')
            assert e <= 1e-2, (m, name, e)


@pytest.mark.parametrize('B,K', CASES, ids=IDS)
def test_the_same_step_twice_gives_the_same_bits(dev, B, K):
    c = _case(dev, B, K)
    tr = c['tr']
    runs = []
    for _ in range(2):
        tr.train_step(c['batch'], plan=c['plans'], update=False)
        torch.cuda.synchronize()
        runs.append((tr.params.grad32.view(torch.int32).clone(), tr.loss_sum.view(torch.int32).clone()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    assert torch.equal(runs[0][0], c['grad32'].view(torch.int32)), 'and the bits of the first step of this state'
    assert bool(torch.isfinite(tr.params.grad32).all()) and float(tr.params.grad32.abs().max()) > 0


@pytest.mark.parametrize('B,K', CASES, ids=IDS)
def test_graph_replay_equals_the_eager_step(dev, B, K):
    """capture + train_step_graph against eager train_step: loss_sum and params.master bit for bit over two steps."""
    from merlot_reserve_amd.config import tiny_config
    from merlot_reserve_amd.microbatch import MicroBatchTrainer
    from merlot_reserve_amd.synthetic import make_batch
    cfg = tiny_config(seq_len=80, lang_seq_len=40)
    cfg['optimizer'].update(num_warmup_steps=1, learning_rate=1e-3)
    bs = [make_batch(cfg, B, seed=10 + i, device=dev) for i in range(3)]
    tr, ref = (MicroBatchTrainer(cfg, B, dev, micro_batches=K, seed=0) for _ in range(2))
    tr.train_step(bs[0])
    ref.train_step(bs[0])
    before = tr.params.master.clone()
    tr.capture(bs[1])
    for bt in bs[1:]:
        a = tr.train_step_graph(bt, tr.plan(bt))
        e = ref.train_step(bt, plan=ref.plan(bt))
        torch.cuda.synchronize()
        assert torch.equal(a.view(torch.int32), e.view(torch.int32)) and bool(torch.isfinite(a).all())
        assert torch.equal(tr.params.master.view(torch.int32), ref.params.master.view(torch.int32))
    assert tr.state.step == ref.state.step == 3 and not torch.equal(before, tr.params.master)
    assert tr.loss_info() == ref.loss_info()


def test_one_micro_batch_is_the_trainer(dev):
    """K = 1: the same loss bits as Trainer on the same batch and draws; master within the trainer test's Adam bound (rtol 2e-6, atol 1e-9: the
    fp32-gradient chain reads the same bf16 gradient values through an fp32 buffer)."""
    from merlot_reserve_amd.config import tiny_config
    from merlot_reserve_amd.microbatch import MicroBatchTrainer
    from merlot_reserve_amd.synthetic import make_batch, make_draws
    from merlot_reserve_amd.trainer import Trainer
    cfg = tiny_config(seq_len=80, lang_seq_len=40)
    cfg['optimizer'].update(num_warmup_steps=1, learning_rate=1e-3)           # (the first update is zero: the count starts at 0)
    B = 2
    mb, tr = MicroBatchTrainer(cfg, B, dev, micro_batches=1, seed=5), Trainer(cfg, B, dev, seed=5)
    assert mb.engine.world == 1
    for i in range(2):
        batch, draws = make_batch(cfg, B, seed=50 + i, device=dev), make_draws(cfg, B, seed=50 + i)
        a = mb.train_step(batch, draws=draws)
        e = tr.train_step(batch, draws=draws)
        torch.cuda.synchronize()
        assert torch.equal(a.view(torch.int32), e.view(torch.int32)), (a, e)
        same = torch.equal(mb.params.master.view(torch.int32), tr.params.master.view(torch.int32))
        print(f'step {i}: master bit-equal to Trainer: {same}; max |d| {float((mb.params.master - tr.params.master).abs().max()):.3e}')
        torch.testing.assert_close(mb.params.master, tr.params.master, rtol=2e-6, atol=1e-9)
    assert mb.loss_info()['loss'] == tr.loss_info()['loss'] and mb.state.step == 2


def test_buffers_are_sized_by_the_micro_batch(dev):
    import gc

    from merlot_reserve_amd.config import tiny_config
    from merlot_reserve_amd.microbatch import MicroBatchTrainer
    from merlot_reserve_amd.trainer import Trainer
    cfg = tiny_config(seq_len=80, lang_seq_len=40)
    B, K = 8, 4
    b = B // K

    def allocated(make):
        gc.collect()
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        base = torch.cuda.memory_allocated()
        t = make()
        n = torch.cuda.memory_allocated() - base
        return t, n
    mb, n_mb = allocated(lambda: MicroBatchTrainer(cfg, B, dev, micro_batches=K))
    eng, d = mb.engine, mb.engine.d
    assert (eng.tv.M, eng.ta.M, eng.tj.M, eng.ts.M) == (b * d.nseg * d.Sv, b * d.nspans * d.Sa, d.Nj * d.Sj, b * d.n_inc * d.Ss)
    assert d.B == b and d.Nj % b == 0 and eng.world == K and mb.E_loc.shape == (K, eng.R, d.H)
    del mb, eng
    tr, n_tr = allocated(lambda: Trainer(cfg, B, dev))
    assert tr.engine.tv.M == K * b * d.nseg * d.Sv
    print(f'memory_allocated: MicroBatchTrainer(B={B}, K={K}) {n_mb / 2 ** 20:.1f} MiB, Trainer(B={B}) {n_tr / 2 ** 20:.1f} MiB')
    assert n_mb < n_tr


def test_driver_with_micro_batches_and_resume(dev, tmp_path, capsys):
    """train.main --synthetic --micro-batches 2 --records-per-gpu 4: four log lines with finite losses; a run resumed at step 2 ends with the same
    master bits."""
    from merlot_reserve_amd import checkpoint as C
    from merlot_reserve_amd import train
    from merlot_reserve_amd.config import tiny_config
    from oracle import ref_torch as R
    cfg = tiny_config(seq_len=80, lang_seq_len=40)
    cfg['optimizer'].update(num_warmup_steps=2, learning_rate=1e-3)
    cfg['device'] = dict(cfg.get('device', {}), iterations_per_loop=4, commit_every_nsteps=2, batch_size=2)
    fn = tmp_path / 'tiny.yaml'
    fn.write_text(yaml.dump(cfg))
    threads = torch.get_num_threads()

    def drive(out, steps):
        try:
            assert train.main([str(fn), '-output_dir', str(out), '--seed', '3', '--synthetic', '--micro-batches', '2', '--records-per-gpu', '4',
                               '--max-steps', str(steps)]) == 0
        finally:
            torch.set_num_threads(threads)           # (the synthetic feed caps torch's intra-op pool for its process)
        return capsys.readouterr().out
    a, b = tmp_path / 'a', tmp_path / 'b'
    out = drive(a, 4)
    assert 'micro_batches=2' in out
    log = [json.loads(line) for line in open(a / 'train_log.jsonl')]
    assert [r['step'] for r in log] == [0, 1, 2, 3] and all(math.isfinite(r['loss']) and r['loss'] > 0 for r in log)
    assert sorted(os.listdir(a)) == ['ckpt_4', 'train_log.jsonl']
    drive(b, 2)
    assert sorted(os.listdir(b)) == ['ckpt_2', 'train_log.jsonl']
    assert 'at step 2' in drive(b, 4)
    sa, sb = C.load_checkpoint(str(a)), C.load_checkpoint(str(b))
    assert sa['step'] == sb['step'] == 4
    la, lb = dict(R.tree_leaves(sa['params'])), dict(R.tree_leaves(sb['params']))
    assert set(la) == set(lb) and len(la) > 50
    for n in la:
        assert la[n].dtype == torch.float32 and torch.equal(la[n].view(torch.int32), lb[n].view(torch.int32)), n
    assert [r['loss'] for r in log] == [json.loads(line)['loss'] for line in open(b / 'train_log.jsonl')]
