"""Shared helpers for the parity tests (test infrastructure: may import oracle/)."""
import numpy as np
import torch

from merlot_reserve_amd.config import Dims, tiny_config
from merlot_reserve_amd.params import ParamStore
from merlot_reserve_amd.synthetic import make_batch, make_draws

INT_KEYS = ['text2audio', 'audio2text', 'audio_text_matching', 'random_text']


def oracle_batch(batch, dtype=torch.float32):
    """synthetic.make_batch layout -> the dict the oracle's pretrain_forward consumes (int64 indices, float inputs)."""
    ob = {}
    for k, v in batch.items():
        if isinstance(v, np.ndarray):
            ob[k] = torch.from_numpy(v.astype(np.int64))
        else:
            ob[k] = v.detach().to('cpu').to(torch.float32).to(dtype)
    return ob


def oracle_draws(splits, z):
    return [torch.from_numpy(s.astype(np.int64)) for s in splits], torch.from_numpy(z)


def tree_to(tree, dtype):
    if isinstance(tree, dict):
        return {k: tree_to(v, dtype) for k, v in tree.items()}
    return tree.to(dtype)


def tiny_setup(B=2, seed=3, device='cpu', hidden_size=128, model_flags=None, data_flags=None):
    cfg = tiny_config(hidden_size=hidden_size, seq_len=80, lang_seq_len=40)
    cfg['model'].update(model_flags or {})
    cfg['data'].update(data_flags or {})
    store = ParamStore(cfg, device, seed=seed)
    batch = make_batch(cfg, B, seed=seed, device=device)
    splits, z = make_draws(cfg, B, seed=seed)
    # force at least one video-source split so the masking branch is exercised
    splits[0][0] = 1
    return cfg, store, batch, splits, z


def relerr(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


# ---------------------------------------------------------------------------------------------------------------------------------
# Bit-exact GEMM checks (tests/test_gemm_exact_gpu.py; tests/test_gemm_exact_checker.py shows that they cannot be fooled).
# Operands and outputs are LEADING VIEWS of larger allocations: what lies past an operand's extent is NaN (a kernel that reads it into a
# result is caught by the exact comparison), what lies past an output's extent is a sentinel bit pattern that must survive the launch.
SENTINEL_BITS = {2: 0xFFA5 - (1 << 16), 4: 0xFFA5A5A5 - (1 << 32)}     # per element size, as signed integers; both are NaNs with a payload


def as_bits(t):
    """The raw words of a bf16 / fp32 tensor (any strides) as int16 / int32."""
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


def padded_operand(vals, ld, tail_rows=256):
    """vals [R, C] as the leading view of an [R + tail_rows, ld] allocation: zeros up to the next multiple of 8 columns (the contract of
    include/mreserve_hip.h: "pad on the host"), NaN in every other cell -- the rest of each row and `tail_rows` whole rows behind."""
    R, C = vals.shape
    c8 = (C + 7) // 8 * 8
    assert ld >= c8
    alloc = torch.full((R + tail_rows, ld), float('nan'), dtype=vals.dtype, device=vals.device)
    alloc[:R, :C] = vals
    alloc[:R, C:c8] = 0
    return alloc[:R, :C]


def padded_vector(vals, tail=256):
    """A contiguous tensor (bias [N], "rotary" table [rows, 32]) as the head of a flat allocation whose tail is NaN."""
    flat = torch.full((vals.numel() + tail,), float('nan'), dtype=vals.dtype, device=vals.device)
    flat[:vals.numel()] = vals.reshape(-1)
    return flat[:vals.numel()].view(vals.shape)


def guarded_output(rows, ld, dtype, device, tail_rows=8):
    """An output allocation [rows + tail_rows, ld] in which every cell holds the sentinel."""
    alloc = torch.empty((rows + tail_rows, ld), dtype=dtype, device=device)
    as_bits(alloc).fill_(SENTINEL_BITS[alloc.element_size()])
    return alloc


def exact_report(alloc, ref, row_index=None):
    """'' when the allocation holds exactly `ref` [M, N] (same dtype: the expected stored VALUES, compared as bits) at rows
    `row_index` (None: rows 0..M-1), columns 0..N-1, and the sentinel in EVERY other cell; otherwise what is wrong and where."""
    assert alloc.dtype == ref.dtype and ref.dim() == 2
    M, N = ref.shape
    got = as_bits(alloc)
    exp = torch.full_like(got, SENTINEL_BITS[alloc.element_size()])
    stored = torch.zeros(got.shape, dtype=torch.bool, device=got.device)
    rb = as_bits(ref.contiguous())
    if row_index is None:
        exp[:M, :N] = rb
        stored[:M, :N] = True
    else:
        assert row_index.numel() == M
        exp[row_index, :N] = rb
        stored[row_index, :N] = True
    if torch.equal(got, exp):
        return ''
    bad = got != exp
    in_bad, guard_bad = bad & stored, bad & ~stored
    msg = []
    if in_bad.any():
        r, c = [int(v) for v in in_bad.nonzero()[0]]
        msg.append(f'{int(in_bad.sum())} of {M * N} stored elements differ from the reference, first at storage row {r}, column {c}: '
                   f'got 0x{int(got[r, c]) & (0xFFFF if alloc.element_size() == 2 else 0xFFFFFFFF):x}, '
                   f'want 0x{int(exp[r, c]) & (0xFFFF if alloc.element_size() == 2 else 0xFFFFFFFF):x}; '
                   f'bad rows {int(in_bad.any(1).sum())}, bad columns {int(in_bad.any(0).sum())}')
    if guard_bad.any():
        r, c = [int(v) for v in guard_bad.nonzero()[0]]
        msg.append(f'{int(guard_bad.sum())} guard cells overwritten, first at row {r}, column {c} of the [{alloc.shape[0]}, {alloc.shape[1]}] allocation')
    return '; '.join(msg)


def bf16_ulp_distance(a, b):
    """Elementwise distance of two bf16 tensors in units of one bf16 code (sign-magnitude words mapped onto one ordered integer line)."""
    def line(t):
        w = as_bits(t.contiguous()).to(torch.int32) & 0xFFFF
        return torch.where(w >= 0x8000, -(w & 0x7FFF), w)
    return (line(a) - line(b)).abs()


def one_ulp_report(got, ref):
    """'' when every element of the bf16 tensor `got` is finite and within ONE bf16 code of `ref` (bf16); no allowance for outliers."""
    if not torch.isfinite(got.float()).all():
        return f'{int((~torch.isfinite(got.float())).sum())} non-finite elements'
    d = bf16_ulp_distance(got, ref)
    if int(d.max()) <= 1:
        return ''
    r = [int(v) for v in (d > 1).nonzero()[0]]
    return f'{int((d > 1).sum())} elements more than one bf16 ulp from the reference (max {int(d.max())}), first at {r}'


def same_input_same_bits_report(key, got):
    """The output of a pointwise epilogue is a function of its exact pre-activation alone: '' when all elements of `got` whose integer
    `key` (the pre-activation in units of its grid) is equal carry the same bits; otherwise how many keys have more than one output."""
    k = key.reshape(-1).to(torch.int64)
    w = as_bits(got.contiguous()).reshape(-1).to(torch.int64)
    uniq, inv = torch.unique(k, return_inverse=True)
    lo = torch.full((uniq.numel(),), 1 << 40, dtype=torch.int64, device=k.device).scatter_reduce(0, inv, w, 'amin')
    hi = torch.full((uniq.numel(),), -(1 << 40), dtype=torch.int64, device=k.device).scatter_reduce(0, inv, w, 'amax')
    bad = lo != hi
    if not bad.any():
        return ''
    return f'{int(bad.sum())} of {uniq.numel()} distinct pre-activations map to more than one output word, first key {int(uniq[bad][0])}'
