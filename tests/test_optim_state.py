"""The optimizer step state shared by the three programs (merlot_reserve_amd/optim.py).  Host part: the device scalars of prepare_step are the
contract of mr_adam_bf16_update_dev, hyper = {sched, -lr, fp32(1) / fp32(bc1), fp32(1) / fp32(bc2)} (tests/test_exports_direct_gpu.py pins the kernel
side), for both state classes.  GPU part: with that vector the chain in pieces (prepare_step + apply_range) is the host-scalar chain
(apply_gradients) bit for bit."""
import types

import numpy as np
import pytest
import torch

from merlot_reserve_amd.config import tiny_config
from merlot_reserve_amd.finetune import FinetuneTrainState
from merlot_reserve_amd.params import ParamStore
from merlot_reserve_amd.trainer import TrainState
from oracle import ref_torch as R

B1, B2 = 0.9, 0.98


def _cfg():
    return tiny_config(hidden_size=128, seq_len=80, lang_seq_len=40)


def _state(kind, store, opt_config):
    oc = dict(opt_config, do_bias_correction=True, beta_1=B1, beta_2=B2)
    if kind == 'pretrain':
        return TrainState(store, oc)
    return FinetuneTrainState(types.SimpleNamespace(params_store=store, shard_optimizer=False, apply=None), oc)


def _want(kind, oc, step):
    if kind == 'pretrain':
        sched = float(R.lr_scale_linearwarmup_cosinedecay(step, oc['num_warmup_steps'], oc['num_train_steps'], oc.get('final_lr_scale', 0.02)))
    else:
        sched = float(R.lr_scale_linearwarmup_lineardecay(step, oc['num_warmup_steps'], oc['num_train_steps']))
    f = np.float32
    bc1, bc2 = 1.0 - B1 ** (step + 1), 1.0 - B2 ** (step + 1)
    return [float(f(sched)), float(f(-oc['learning_rate'])), float(f(1) / f(bc1)), float(f(1) / f(bc2))]


@pytest.mark.parametrize('kind', ['pretrain', 'finetune'])
def test_device_scalars_are_the_kernel_contract(kind):
    cfg = _cfg()
    store = ParamStore(cfg, 'cpu')
    state = _state(kind, store, cfg['optimizer'])
    for step in (0, 6, 11, 41):
        state.step = step
        state.prepare_step()
        assert state.hyper.tolist() == _want(kind, state.opt_config, step), step
    # three consecutive steps: the ring of two host vectors wraps, the device vector is the current step's each time
    for step in (41, 42, 43):
        state.step = step
        state.prepare_step()
        assert state.hyper.tolist() == _want(kind, state.opt_config, step), step


@pytest.mark.gpu
@pytest.mark.parametrize('kind', ['pretrain', 'finetune'])
def test_chain_in_pieces_equals_host_scalar_chain_bit_for_bit(dev, kind):
    """Twin stores, the same seeded bf16 gradients (NaN and +-inf among them), bias correction on, step 6: apply_gradients() against
    prepare_step() + apply_range(0, total) -- master, working copy and both moments identical word for word."""
    from tests.util import as_bits
    cfg = _cfg()
    g = torch.Generator().manual_seed(5)
    twins = []
    for _ in range(2):
        store = ParamStore(cfg, dev, seed=3, with_orig=kind == 'finetune')
        state = _state(kind, store, cfg['optimizer'])
        state.step = 6
        twins.append((store, state))
    n = twins[0][0].total
    grad = (torch.randn(n, generator=g) * 1e-2).to(torch.bfloat16)
    grad[5], grad[2048 + 6], grad[n - 7] = float('nan'), float('inf'), -float('inf')
    mu = (torch.randn(n, generator=g) * 1e-3).to(torch.bfloat16)
    nu = (torch.rand(n, generator=g) * 1e-2).to(torch.bfloat16)
    for store, _state_ in twins:
        store.grad.copy_(grad)
        store.mu.copy_(mu)
        store.nu.copy_(nu)
    (pa, sa), (pb, sb) = twins
    sa.apply_gradients()
    sb.prepare_step()
    sb.apply_range(0, n)
    torch.cuda.synchronize()
    assert sa.step == 7 and sb.step == 6
    for name in ('master', 'work', 'mu', 'nu'):
        a, b = getattr(pa, name), getattr(pb, name)
        assert torch.equal(as_bits(a), as_bits(b)), name
    assert not torch.equal(as_bits(pa.master), as_bits(ParamStore(cfg, dev, seed=3).master)), 'the step moved the parameters'
