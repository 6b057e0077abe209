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


# ---------------------------------------------------------------------------------------------------------------------------------
# Element-wise checks of the row kernels (tests/test_rowops_exact_gpu.py; tests/test_rowops_exact_checker.py shows that they bite).
# Where the arithmetic is exact (small integers) the result is compared by bits with exact_report; elsewhere EVERY element must lie inside
#     |got - ref| <= (2^-8 + 2^-14) |ref| + n_terms 2^-23 mag            (fp32 outputs: 2^-14 in place of 2^-8 + 2^-14)
# 2^-8 |ref| is one round-to-nearest into bf16.  n 2^-23 mag is twice the worst-case fp32 error of an n-term sum taken in any order (the running
# error bound: n u sum|term|, u = 2^-24), `mag` being the result's formula in fp64 with every summed term replaced by its absolute value and the
# error of an earlier sum carried to first order through what follows it.  2^-14 |ref| is 256 fp32 ulps of headroom for rsqrtf / __expf /
# __logf and the handful of single roundings between the sums.  Both extra terms stay far below one bf16 code.
def bound_report(got_alloc, ref64, mag64, n_terms, row_index=None, alt_ref64=None):
    """'' when every stored element of the allocation (rows `row_index`, None: 0..M-1; columns 0..N-1 of ref64 [M, N]) is finite and inside the
    bound above against ref64 -- or, where given, against alt_ref64 (a second admissible reference: the other side of a rounding boundary
    that the kernel's intermediate may legitimately fall on) -- and EVERY other cell still holds the sentinel; otherwise what is wrong and where."""
    assert ref64.dtype == torch.float64 and ref64.dim() == 2
    M, N = ref64.shape
    rnd = 2.0 ** -8 + 2.0 ** -14 if got_alloc.element_size() == 2 else 2.0 ** -14
    bits = as_bits(got_alloc)
    stored = torch.zeros(bits.shape, dtype=torch.bool, device=bits.device)
    rows = slice(0, M) if row_index is None else row_index.long()
    assert row_index is None or row_index.numel() == M
    stored[rows, :N] = True
    got = got_alloc[rows, :N].double()
    noise = n_terms * 2.0 ** -23 * (mag64 + torch.zeros_like(ref64))
    assert bool((noise >= 0).all())

    def excess(ref):            # error / tolerance; an exact hit of a zero tolerance counts as 0
        err, tol = (got - ref).abs(), rnd * ref.abs() + noise
        return torch.where(err <= tol, err / tol.clamp_min(1e-300), torch.full_like(err, float('inf'))).nan_to_num(nan=float('inf'))
    ex = excess(ref64)
    if alt_ref64 is not None:
        ex = torch.minimum(ex, excess(alt_ref64))
    bad = ~torch.isfinite(got) | (ex > 1)
    guard_bad = (bits != SENTINEL_BITS[got_alloc.element_size()]) & ~stored
    msg = []
    if bad.any():
        r, c = [int(v) for v in bad.nonzero()[0]]
        sr = r if row_index is None else int(row_index[r])
        err = float((got[r, c] - ref64[r, c]).abs())
        tol = float(rnd * ref64[r, c].abs() + noise[r, c])
        msg.append(f'{int(bad.sum())} of {M * N} stored elements outside the bound, first at storage row {sr}, column {c}: got {float(got[r, c])!r}, '
                   f'want {float(ref64[r, c])!r} (error {err:.3e}, tolerance {tol:.3e}); bad rows {int(bad.any(1).sum())}, '
                   f'bad columns {int(bad.any(0).sum())}')
    if guard_bad.any():
        r, c = [int(v) for v in guard_bad.nonzero()[0]]
        msg.append(f'{int(guard_bad.sum())} guard cells overwritten, first at row {r}, column {c} of the [{got_alloc.shape[0]}, {got_alloc.shape[1]}] allocation')
    return '; '.join(msg)


def bound_margin(got_alloc, ref64, mag64, n_terms, row_index=None):
    """(worst error / tolerance over the stored elements, worst noise term / rounding term): what a test prints next to its assertion."""
    M, N = ref64.shape
    rnd = 2.0 ** -8 + 2.0 ** -14 if got_alloc.element_size() == 2 else 2.0 ** -14
    got = got_alloc[slice(0, M) if row_index is None else row_index.long(), :N].double()
    noise = n_terms * 2.0 ** -23 * (mag64 + torch.zeros_like(ref64))
    tol = rnd * ref64.abs() + noise
    nz, rz = tol > 0, ref64 != 0
    return (float(((got - ref64).abs()[nz] / tol[nz]).max()) if nz.any() else 0.0,
            float((noise[rz] / (rnd * ref64.abs()[rz])).median()) if rz.any() else 0.0)


# Integer-valued operands: with every sum of magnitudes <= 256 each fp32 partial sum, in any order, and the bf16 result are exact, so a kernel's
# output is known to the bit.  The precondition is asserted on the REFERENCE (exact_bf16), never on what a kernel returned.
def small_ints(shape, k, seed, dtype=torch.bfloat16, device='cpu'):
    """Uniform integers in [-k, k] (every one a bf16 / fp32 value)."""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-k, k + 1, shape, generator=g).to(dtype).to(device)


def sparse_int_rows(rows, cols, seed, dtype=torch.bfloat16, device='cpu'):
    """Integers [rows, cols] whose column sums are exact in any order -- sum |x| <= 256 in every column -- and in which EVERY row has a non-zero
    entry, so that a dropped or doubled row changes a column sum.  Up to 256 rows the matrix is dense; beyond, row r holds one entry in column r % cols."""
    g = torch.Generator().manual_seed(seed)
    per_col = (rows + cols - 1) // cols
    if rows <= 256:
        k = min(3, 256 // rows)
        x = torch.randint(-k, k + 1, (rows, cols), generator=g)
    else:
        k = min(3, 256 // per_col)
        assert k >= 1, f'{rows} rows need more than {cols} columns'
        x = torch.zeros(rows, cols, dtype=torch.int64)
    r = torch.arange(rows)
    x[r, r % cols] = torch.randint(1, k + 1, (rows,), generator=g) * (2 * torch.randint(0, 2, (rows,), generator=g) - 1)
    assert int(x.abs().sum(0).max()) <= 256 and bool((x != 0).any(1).all())
    return x.to(dtype).to(device)


def exact_bf16(ref64):
    """The fp64 reference as bf16, after asserting that nothing is lost: every value is a bf16 value (an integer of magnitude <= 256 is one)."""
    out = ref64.to(torch.bfloat16)
    assert torch.equal(out.double(), ref64), 'the reference is not exactly representable in bf16: the test data break the precondition'
    return out
