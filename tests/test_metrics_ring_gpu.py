"""The step-metrics ring on the GPU: mr_metrics_push alone, and Trainer(metrics_ring=...) against a twin trainer that calls loss_info()
after every step (tiny shapes; eager first step, captured replays after)."""
import ctypes

import numpy as np
import pytest
import torch

from merlot_reserve_amd.config import tiny_config
from merlot_reserve_amd.synthetic import make_batch

pytestmark = pytest.mark.gpu


def test_metrics_push_kernel(dev):
    """depth 4, 10 pushes from changing sources: every surviving row equals its sources bit for bit, rows wrap, the counter reads 10."""
    from merlot_reserve_amd import _lib, ops
    depth, L = 4, ops.METRICS_ROW + 2                                   # two spare columns: the kernel must leave them alone
    g = torch.Generator().manual_seed(5)
    ring = torch.full((depth, L), -7.0, device=dev)
    steps = torch.full((depth,), -1, dtype=torch.int32, device=dev)
    counter = torch.zeros(1, dtype=torch.int32, device=dev)
    srcs = []
    la, dg, sc, sched = (torch.zeros(n, device=dev) for n in (3, 12, 3, 4))
    for i in range(10):
        vals = [torch.randn(n, generator=g) * 10.0 ** (i - 5) for n in (3, 12, 3, 4)]
        vals[0][0] = float(np.float32(1e-40)) * (i + 1)                # a subnormal goes through unchanged
        srcs.append(vals)
        for t, v in zip((la, dg, sc, sched), vals):
            t.copy_(v)
        ops.metrics_push(la, dg.view(2, 6), sc, sched, ring, steps, counter)
    torch.cuda.synchronize()
    assert counter.item() == 10
    assert steps.tolist() == [8, 9, 6, 7]                               # rows wrap: row = step mod depth
    host = ring.cpu()
    for row, step in enumerate(steps.tolist()):
        v = srcs[step]
        want = torch.cat([v[0], v[1], v[2], v[3][:1]])
        assert torch.equal(host[row, :ops.METRICS_ROW].view(torch.int32), want.view(torch.int32)), (row, step)
        assert host[row, ops.METRICS_ROW:].tolist() == [-7.0, -7.0]
    # a counter that starts at a restored step
    counter.copy_(torch.tensor([1001], dtype=torch.int32))
    ops.metrics_push(la, dg.view(2, 6), sc, sched, ring, steps, counter)
    torch.cuda.synchronize()
    assert counter.item() == 1002 and steps.tolist() == [8, 1001, 6, 7]
    # invalid arguments: MR_EINVAL and a message, nothing launched (the ring is as it was)
    lib = _lib.load()
    before = (ring.clone(), steps.clone())
    p = [t.data_ptr() for t in (la, dg, sc, sched, ring, steps, counter)]
    s = torch.cuda.current_stream().cuda_stream
    for k in range(7):
        bad = list(p)
        bad[k] = None
        assert lib.mr_metrics_push(*bad, depth, L, s) == -1 and b'mr_metrics_push' in lib.mr_last_error()
    assert lib.mr_metrics_push(*p, 0, L, s) == -1 and b'depth' in lib.mr_last_error()
    assert lib.mr_metrics_push(*p, -4, L, s) == -1
    assert lib.mr_metrics_push(*p, depth, ops.METRICS_ROW - 1, s) == -1 and b'row_len' in lib.mr_last_error()
    torch.cuda.synchronize()
    assert counter.item() == 1002 and torch.equal(ring, before[0]) and torch.equal(steps, before[1])
    assert lib.mr_version() >= 8


def _run(dev, cfg, B, batches, comm, ring):
    from merlot_reserve_amd.trainer import Trainer
    tr = Trainer(cfg, B, dev, seed=0, comm=comm, world=1, rank=0, **({'metrics_ring': 8} if ring else {}))
    infos, rows = [], []
    for i, b in enumerate(batches):
        plan = tr.plan(b)
        if i == 0:
            tr.train_step(b, plan=plan)
            tr.capture(b)
        else:
            tr.train_step_graph(b, plan)
        if ring:
            if (i + 1) % 4 == 0:
                rows += tr.drain_metrics()
        else:
            infos.append((tr.loss_info(), tr.params.wm['contrastive_scales'].tolist()))
    if ring:
        assert len(rows) < len(batches)                                # the rows lag: nothing of the last interval has been returned yet
        rows += tr.drain_metrics(flush=True)
    torch.cuda.synchronize()
    return tr, infos, rows


@pytest.mark.parametrize('with_comm', [False, True])
def test_ring_rows_equal_loss_info_of_a_twin(dev, with_comm):
    """12 steps (eager, then captured).  Every key of every drained row equals the twin's loss_info() of that step EXACTLY, and the master parameters
    of the two trainers are bit-identical after the last step: the push changes nothing it does not own.
    with_comm: a one-rank NativeComm, so the drain takes the collective path -- the derived values go through the fp32 buffer of ONE
    allreduce_mean_f32, exactly as loss_info(reduce=True) sends them for world > 1; the twin's (float64) values are therefore compared after the
    same rounding to fp32 (a one-rank mean is the identity).  No other tolerance."""
    from merlot_reserve_amd.dist import NativeComm
    from merlot_reserve_amd.trainer import lr_scale_linearwarmup_cosinedecay
    cfg = tiny_config(seq_len=80, lang_seq_len=40)
    cfg['optimizer'].update(num_warmup_steps=3, learning_rate=1e-3)
    B = 2
    batches = [make_batch(cfg, B, seed=500 + i, device=dev) for i in range(12)]
    comm = NativeComm() if with_comm else None
    twin, infos, _ = _run(dev, cfg, B, batches, comm, ring=False)
    if comm is not None:
        comm.close()
    comm = NativeComm() if with_comm else None
    tr, _, rows = _run(dev, cfg, B, batches, comm, ring=True)
    assert [r['step'] for r in rows] == list(range(12))
    rnd = (lambda v: float(np.float32(v))) if with_comm else (lambda v: v)
    oc = cfg['optimizer']
    for row, (info, scales) in zip(rows, infos):
        assert set(row) == set(info) | {'step', 'contrastive_scales', 'lr_scale'}
        for k, v in info.items():
            assert row[k] == rnd(v), (row['step'], k, row[k], v)
        # the temperatures are the ones the step's forward read: the twin read them AFTER the step's update, i.e. they are the NEXT row's
        if row['step'] + 1 < 12:
            assert rows[row['step'] + 1]['contrastive_scales'] == scales
        want = lr_scale_linearwarmup_cosinedecay(row['step'], oc['num_warmup_steps'], oc['num_train_steps'], oc.get('final_lr_scale', 0.02))
        assert row['lr_scale'] == float(np.float32(want))
    assert rows[0]['contrastive_scales'] != rows[-1]['contrastive_scales']
    assert torch.equal(tr.params.master, twin.params.master) and torch.equal(tr.params.mu, twin.params.mu) and torch.equal(tr.params.nu, twin.params.nu)
    assert tr.state.step == twin.state.step == 12
    if comm is not None:
        comm.close()


def test_default_trainer_has_no_ring(dev):
    """metrics_ring defaults to 0: nothing is allocated and the step issues no push (the launch sequence of every existing caller)."""
    from merlot_reserve_amd import ops
    from merlot_reserve_amd.trainer import Trainer
    cfg = tiny_config(seq_len=80, lang_seq_len=40)
    tr = Trainer(cfg, 2, dev, seed=0)
    assert tr.metrics_ring == 0 and tr.step_metrics is None
    calls = []
    real = ops.metrics_push
    ops.metrics_push = lambda *a, **k: calls.append(1) or real(*a, **k)
    try:
        b = make_batch(cfg, 2, seed=1, device=dev)
        tr.train_step(b, plan=tr.plan(b))
        tr2 = Trainer(cfg, 2, dev, seed=0, metrics_ring=4)
        tr2.train_step(b, plan=tr2.plan(b))
    finally:
        ops.metrics_push = real
    torch.cuda.synchronize()
    assert calls == [1]
    with pytest.raises(AssertionError):
        tr.drain_metrics()
