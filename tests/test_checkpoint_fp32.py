"""save_checkpoint(keep_fp32=True): the exact restart file of merlot_reserve_amd.train.  fp32 leaves stay fp32 on disk and read back bit for bit;
the default (and keep_fp32=False) is the reference's format, byte for byte what it was: fp32 leaves as fp16 (mreserve/checkpoint.py:26-37)."""
import numpy as np
import torch

from merlot_reserve_amd import checkpoint as C


def _state():
    g = torch.Generator().manual_seed(1)
    kernel = torch.randn(7, 3, 64, generator=g)
    kernel.view(-1)[0] = 70000.0                                   # above the largest fp16 (65504)
    kernel.view(-1)[1] = float(np.float32(1e-40))                  # an fp32 subnormal
    kernel.view(-1)[2] = 1.0 + 2.0 ** -20                          # needs more mantissa than fp16 or bf16 have
    params = {'enc': {'kernel': kernel, 'bias': torch.full((3, 64), 1e-9)}, 'contrastive_scales': torch.tensor([2.5, 2.25, 1.0 / 3.0])}
    mu = C.tree_map(lambda x: (x * 0.1).to(torch.bfloat16), params)
    cnt = torch.tensor(5, dtype=torch.int32)
    return {'step': 5, 'params': params, 'opt_state': {'0': {'count': cnt, 'mu': mu, 'nu': mu}, '1': {}, '2': {'count': cnt}, '3': {}}}


def _leaves(tree, prefix=''):
    if isinstance(tree, dict):
        for k, v in tree.items():
            yield from _leaves(v, f'{prefix}/{k}')
    else:
        yield prefix, tree


def test_keep_fp32_round_trips_bit_for_bit(tmp_path):
    state = _state()
    assert state['params']['enc']['kernel'].view(-1)[1].item() != 0.0
    fn = C.save_checkpoint(state, str(tmp_path), keep_fp32=True)
    raw = C.msgpack_restore(open(fn, 'rb').read())                  # what is on disk, before load_checkpoint's fp16 -> fp32 cast
    sd = C.load_checkpoint(str(tmp_path))
    assert sd['step'] == 5
    for (name, want), (_n, disk), (_m, got) in zip(_leaves(state['params']), _leaves(raw['params']), _leaves(sd['params'])):
        assert disk.dtype == torch.float32, name
        assert got.dtype == torch.float32 and got.shape == want.shape
        assert torch.equal(got.view(torch.int32), want.view(torch.int32)), name          # bit patterns, not values
    k = sd['params']['enc']['kernel'].view(-1)
    assert k[0].item() == 70000.0 and k[1].item() == float(np.float32(1e-40)) and k[2].item() == 1.0 + 2.0 ** -20
    for (name, want), (_m, got) in zip(_leaves(state['opt_state']), _leaves(sd['opt_state'])):
        assert got.dtype == want.dtype and torch.equal(got, want), name                  # bf16 moments and int32 counts as before


def test_default_is_the_reference_format_unchanged(tmp_path):
    state = _state()
    a = C.save_checkpoint(state, str(tmp_path / 'a'))
    b = C.save_checkpoint(state, str(tmp_path / 'b'), keep_fp32=False)
    c = C.save_checkpoint(state, str(tmp_path / 'c'), keep_fp32=True)
    assert open(a, 'rb').read() == open(b, 'rb').read()
    assert open(a, 'rb').read() != open(c, 'rb').read()
    raw = C.msgpack_restore(open(a, 'rb').read())
    assert all(t.dtype == torch.float16 for _n, t in _leaves(raw['params']))
    sd = C.load_checkpoint(a)
    for (name, want), (_m, got) in zip(_leaves(state['params']), _leaves(sd['params'])):
        assert got.dtype == torch.float32 and torch.equal(got, want.to(torch.float16).float()), name      # fp16-rounded, as tests/test_checkpoint.py pins
    k = sd['params']['enc']['kernel'].view(-1)
    assert torch.isinf(k[0]) and k[1].item() == 0.0 and k[2].item() == 1.0               # what the fp16 form loses
    assert sd['opt_state']['0']['mu']['enc']['kernel'].dtype == torch.bfloat16
