"""The comparison behind tests/test_rowops_exact_gpu.py, without a GPU.  (1) The bound of util.bound_report is met, with no element left out, by a
plain torch-fp32 evaluation of each bound-checked kernel's formulas at the edge shapes of the GPU file: the magnitude models of tests/rowops_refs.py
hold for honest fp32 arithmetic.  (2) Small corruptions of such an output are flagged: one element moved by two bf16 codes, a row replaced by its
neighbour, a stale last 8-element chunk, an overwritten guard cell, a row lost from a reduction.  (3) The ops wrappers of entry points that take no
leading dimension refuse a strided view before any library call."""
import pytest
import torch

import rowops_refs as RR
from util import (SENTINEL_BITS, as_bits, bound_margin, bound_report, exact_bf16, exact_report, guarded_output, padded_operand, small_ints,
                  sparse_int_rows)

BF16, F32 = torch.bfloat16, torch.float32


def _store(vals, ld_pad=8, row_index=None, rows=None):
    """A kernel's output [M, N] (or [N]) as it would lie in a guarded allocation."""
    vals = vals.reshape(1, -1) if vals.dim() == 1 else vals
    M, N = vals.shape
    alloc = guarded_output(rows or M, N + ld_pad, vals.dtype, 'cpu')
    alloc[slice(0, M) if row_index is None else row_index.long(), :N] = vals
    return alloc


def _passes(vals, ref_mag, n, what, **kw):
    alloc = _store(vals)
    rep = bound_report(alloc, ref_mag[0], ref_mag[1], n, **kw)
    worst, noise = bound_margin(alloc, ref_mag[0], ref_mag[1], n)
    print(f'{what}: worst error / tolerance {worst:.3f}, median noise term / rounding term {noise:.3f}')
    assert rep == '', f'{what}: {rep}'
    assert worst <= 1.0


@pytest.mark.parametrize('rows,H', RR.LN_CHECKER_SHAPES + [(300, 768)])
def test_fp32_layernorm_meets_the_bound(rows, H):
    x, gamma, beta, dy = RR.ln_inputs(rows, H, seed=rows + H)
    y, mean, rstd = RR.ln_fwd_f32(x, gamma, beta)
    ref = RR.ln_fwd_ref(x, gamma, beta)
    _passes(y, ref['y'], H, 'y')
    _passes(mean, ref['mean'], H, 'mean')
    _passes(rstd, ref['rstd'], H, 'rstd')
    add = RR.rnd((rows, H), 9)
    for dx_add in (None, add):
        dx, dg, db = RR.ln_bwd_f32(dy, x, gamma, mean, rstd, dx_add)
        rb = RR.ln_bwd_ref(dy, x, gamma, mean, rstd, dx_add)
        _passes(dx, rb['dx'], H, 'dx')
        _passes(dg, rb['dgamma'], rows, 'dgamma')
        assert exact_report(_store(db), exact_bf16(rb['dbeta'][0])) == ''


@pytest.mark.parametrize('G,H', RR.MEAN_CHECKER_SHAPES)
def test_fp32_rows_mean_meets_the_bound(G, H):
    R = 3
    src = RR.rnd((G * R + 2, H), G + H, 2.0)
    rows = RR.disjoint_rows(G, R, G * R + 2, 1)
    _passes(RR.rows_mean_fwd_f32(src, rows), RR.rows_mean_fwd_ref(src, rows), R + 2, 'rows mean')
    d = RR.rnd((G, H), 5)
    got = (src.float()[rows.long().reshape(-1)] + (d.float() * torch.tensor(1.0 / R, dtype=F32)).repeat_interleave(R, 0)).to(BF16)
    _passes(got, RR.rows_mean_bwd_ref(d, rows, src), 3, 'rows mean backward')


@pytest.mark.parametrize('G,R,nh', RR.POOL_CHECKER_SHAPES)
def test_fp32_poolattn_meets_the_bound(G, R, nh):
    H, n = nh * 64, G * R + 3
    q, k, v, dout = RR.rnd((G, H), 1), RR.rnd((n, H), 2), RR.rnd((n, H), 3), RR.rnd((G, H), 4)
    kr = RR.disjoint_rows(G, R, n, 5)
    out, probs = RR.poolattn_fwd_f32(q, k, v, kr, nh)
    ref = RR.poolattn_fwd_ref(q, k, v, kr, nh)
    _passes(out, ref['out'], 64 + R, 'out')
    _passes(probs.reshape(G, nh * R), ref['probs'], 64 + R, 'probs')
    p32 = ref['probs'][0].reshape(G, nh, R).float()
    rb = RR.poolattn_bwd_ref(q, k, v, kr, p32, dout, nh)
    for name, got in zip(('dq', 'dk', 'dv'), RR.poolattn_bwd_f32(q, k, v, kr, p32, dout, nh)):
        _passes(got, rb[name], 64 + R, name)


@pytest.mark.parametrize('ls', RR.LOG_SCALES)
@pytest.mark.parametrize('rows,H', RR.UNIT_CHECKER_SHAPES)
def test_fp32_unit_norm_meets_the_bound(rows, H, ls):
    x, dy = RR.rnd((rows, H), rows + H, 3.0), RR.rnd((rows, H), 7)
    x[rows - 1] = 0                                                   # an all-zero row: inv = 1e-5 ^ -1/2, y = 0
    y, inv = RR.unit_norm_fwd_f32(x, ls)
    lo, hi, mag, inv_ref, inv_mag = RR.unit_norm_fwd_ref(x, ls)
    rep = bound_report(_store(y), lo, mag, 1, alt_ref64=hi)
    assert rep == '', rep
    _passes(inv, (inv_ref, inv_mag), H, 'inv_norm')
    dx, dls = RR.unit_norm_bwd_f32(x, ls, inv, dy)
    rb = RR.unit_norm_bwd_ref(x, ls, inv, dy)
    _passes(dx, rb['dx'], H, 'dx')
    _passes(dls, rb['dls'], rows * H, 'dlog_scale')
    if ls > 4.61:
        assert float(dls) == 0.0 and float(rb['dls'][0]) == 0.0


# ------------------------------------------------------------------------------------------------------------------------ corruptions
def _ln_y(rows=9, H=136):
    x, gamma, beta, _ = RR.ln_inputs(rows, H, seed=3)
    y, _, _ = RR.ln_fwd_f32(x, gamma, beta)
    ref, mag = RR.ln_fwd_ref(x, gamma, beta)['y']
    return y, ref, mag, H


def test_two_codes_in_one_element_are_flagged():
    y, ref, mag, H = _ln_y()
    for r, c, step in ((8, 135, 2), (0, 0, -2), (4, 77, 2)):
        alloc = _store(y)
        as_bits(alloc)[r, c] += step
        rep = bound_report(alloc, ref, mag, H)
        assert '1 of 1224 stored elements outside the bound' in rep and f'row {r}, column {c}' in rep, rep
    alloc = _store(y)
    alloc[3, 3] = float('inf')
    assert 'row 3, column 3' in bound_report(alloc, ref, mag, H)
    alloc = _store(y)
    alloc[3, 3] = float('nan')
    assert 'row 3, column 3' in bound_report(alloc, ref, mag, H)


def test_a_row_replaced_by_its_neighbour_is_flagged():
    y, ref, mag, H = _ln_y()
    alloc = _store(y)
    alloc[5, :H] = y[4]
    rep = bound_report(alloc, ref, mag, H)
    assert 'bad rows 1,' in rep and 'storage row 5' in rep, rep


def test_a_stale_last_chunk_is_flagged():
    y, ref, mag, H = _ln_y()
    alloc = _store(y)
    alloc[8, H - 8:H] = y[7, H - 8:H]                                 # what a store guard of `c < nch - 1` leaves behind when the buffer is reused
    rep = bound_report(alloc, ref, mag, H)
    assert 'bad rows 1,' in rep and 'storage row 8, column 12' in rep, rep       # columns 128..135
    alloc = _store(y)
    as_bits(alloc)[8, H - 8:H] = SENTINEL_BITS[2]                     # ... or when it is fresh: the sentinel is a NaN
    assert '8 of 1224 stored elements outside the bound' in bound_report(alloc, ref, mag, H)


def test_an_overwritten_guard_cell_is_flagged():
    y, ref, mag, H = _ln_y()
    for r, c in ((0, H), (8, H + 7), (9, 0), (16, H + 7)):
        alloc = _store(y)
        alloc[r, c] = ref[min(r, 8), min(c, H - 1)]
        rep = bound_report(alloc, ref, mag, H)
        assert '1 guard cells overwritten' in rep and f'row {r}, column {c}' in rep, rep
    idx = torch.tensor([0, 2, 3, 5, 6, 7, 9, 10, 12])                 # stored rows with gaps: a gap row written with a plausible value
    alloc = _store(y, row_index=idx, rows=13)
    assert bound_report(alloc, ref, mag, H, row_index=idx) == ''
    alloc[4, :H] = y[3]
    assert '136 guard cells overwritten' in bound_report(alloc, ref, mag, H, row_index=idx)
    a32 = _store(torch.ones(5, dtype=F32))
    assert bound_report(a32, torch.ones(1, 5, dtype=torch.float64), torch.ones(1, 5, dtype=torch.float64), 4) == ''
    a32[0, 2] += 2.0 ** -13                                           # fp32 outputs: 2^-14 relative, not 2^-8
    assert 'column 2' in bound_report(a32, torch.ones(1, 5, dtype=torch.float64), torch.ones(1, 5, dtype=torch.float64), 4)


@pytest.mark.parametrize('rows', [2, 9, 17])
def test_a_row_lost_from_a_reduction_is_flagged(rows):
    H = 136
    x, gamma, beta, dy = RR.ln_inputs(rows, H, seed=rows)
    _, mean, rstd = RR.ln_fwd_f32(x, gamma, beta)
    rb = RR.ln_bwd_ref(dy, x, gamma, mean, rstd)
    for lost in (0, rows - 1):
        keep = [r for r in range(rows) if r != lost]
        _, dg, db = RR.ln_bwd_f32(dy[keep], x[keep], gamma, mean[keep], rstd[keep])
        assert 'outside the bound' in bound_report(_store(dg), rb['dgamma'][0], rb['dgamma'][1], rows)
        assert 'stored elements differ' in exact_report(_store(db), exact_bf16(rb['dbeta'][0]))
    dbl = list(range(rows)) + [rows - 1]                              # ... and a row counted twice
    _, dg, db = RR.ln_bwd_f32(dy[dbl], x[dbl], gamma, mean[dbl], rstd[dbl])
    assert 'outside the bound' in bound_report(_store(dg), rb['dgamma'][0], rb['dgamma'][1], rows)
    assert 'stored elements differ' in exact_report(_store(db), exact_bf16(rb['dbeta'][0]))


def test_integer_operands_keep_their_promise():
    for rows, cols in ((1, 8), (5, 8), (256, 8), (257, 8), (513, 8), (1027, 8), (4097, 136), (512, 1032)):
        x = sparse_int_rows(rows, cols, seed=rows)
        assert x.dtype == BF16 and float(x.double().abs().sum(0).max()) <= 256 and bool((x != 0).any(1).all())
        exact_bf16(x.double().sum(0, keepdim=True))
    assert small_ints((4, 8), 3, 0).abs().max() <= 3
    with pytest.raises(AssertionError):
        exact_bf16(torch.tensor([[257.0]], dtype=torch.float64))
    with pytest.raises(AssertionError):
        sparse_int_rows(4097, 8, 0)                                   # 513 entries per column cannot keep sum |x| <= 256
    v = padded_operand(small_ints((3, 8), 3, 1), 32, tail_rows=2)
    assert v.stride() == (32, 1)


# ------------------------------------------------------------------------------------------------------------------------ wrappers
def test_wrappers_without_a_leading_dimension_refuse_strided_views():
    """q / out / dout / dq / probs of the attention pool, dst of rows_mean_fwd, ddst of rows_mean_bwd and the operands of add_ reach the library as bare
    pointers: a strided view would be read as if it were dense.  Each wrapper raises before it touches the library (CPU tensors, nothing is launched)."""
    from merlot_reserve_amd import ops
    G, R, nh, H = 4, 2, 1, 64
    wide = torch.zeros(G, 2 * H, dtype=BF16)
    view, dense = wide[:, :H], torch.zeros(G, H, dtype=BF16)
    assert not view.is_contiguous()
    kv = torch.zeros(G * R, H, dtype=BF16)
    kr = torch.arange(G * R, dtype=torch.int32).reshape(G, R)
    probs = torch.zeros(G, nh, R)
    for q, out in ((view, dense), (dense, view)):
        with pytest.raises(AssertionError, match='contiguous'):
            ops.poolattn_fwd(q, kv, kv, kr, out, probs, nh)
    with pytest.raises(AssertionError, match='contiguous'):
        ops.poolattn_fwd(dense, kv, kv, kr, dense, torch.zeros(G, nh, 2 * R)[:, :, :R], nh)
    for q, dout, dq in ((view, dense, dense), (dense, view, dense), (dense, dense, view)):
        with pytest.raises(AssertionError, match='contiguous'):
            ops.poolattn_bwd(q, kv, kv, kr, probs, dout, dq, kv, kv, nh)
    with pytest.raises(AssertionError, match='contiguous'):
        ops.rows_mean_fwd(kv, kr, view)
    with pytest.raises(AssertionError, match='contiguous'):
        ops.rows_mean_bwd(view, kr, kv)
    with pytest.raises(AssertionError, match='contiguous'):
        ops.rows_mean_fwd(kv, torch.arange(2 * G * R, dtype=torch.int32).reshape(G, 2 * R)[:, :R], dense)
    for a, b, y in ((view, dense, None), (dense, view, None), (dense, dense, view)):
        with pytest.raises(AssertionError, match='contiguous'):
            ops.add_(a, b, y)
    with pytest.raises(AssertionError, match='one size'):
        ops.add_(dense, torch.zeros(G + 1, H, dtype=BF16))
