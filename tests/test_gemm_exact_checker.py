"""The comparison behind tests/test_gemm_exact_gpu.py cannot be fooled: each of four small corruptions of a correct result -- one bf16 ulp in one
element, one zeroed 16 x 16 fragment, one overwritten guard cell, two elements of equal pre-activation that differ by one ulp -- is flagged, and
the untouched result passes.  No GPU."""
import torch

from util import (SENTINEL_BITS, as_bits, bf16_ulp_distance, exact_report, guarded_output, one_ulp_report, padded_operand,
                  same_input_same_bits_report)

BF16 = torch.bfloat16


def _case(M=300, N=200, ld=208, row_index=None, rows=None):
    g = torch.Generator().manual_seed(0)
    ref = (torch.randint(-600, 600, (M, N), generator=g).float()).to(BF16)          # values past 256: rounded ones among them
    alloc = guarded_output(rows or M, ld, BF16, 'cpu')
    if row_index is None:
        alloc[:M, :N] = ref
    else:
        alloc[row_index, :N] = ref
    return alloc, ref


def test_untouched_result_passes():
    alloc, ref = _case()
    assert exact_report(alloc, ref) == ''
    idx = (torch.arange(300) // 60) * 61 + 1 + torch.arange(300) % 60               # a row map with a gap row before every group
    alloc, ref = _case(row_index=idx, rows=5 * 61)
    assert exact_report(alloc, ref, idx) == ''
    a32 = guarded_output(4, 16, torch.float32, 'cpu')
    r32 = torch.arange(4 * 10, dtype=torch.float32).reshape(4, 10)
    a32[:4, :10] = r32
    assert exact_report(a32, r32) == ''


def test_one_ulp_in_one_element_is_flagged():
    alloc, ref = _case()
    as_bits(alloc)[299, 199] += 1
    rep = exact_report(alloc, ref)
    assert '1 of 60000 stored elements differ' in rep and 'row 299, column 199' in rep, rep
    alloc, ref = _case()
    as_bits(alloc)[0, 0] ^= -0x8000                                                 # the sign of one element (+0 against -0 included)
    assert 'row 0, column 0' in exact_report(alloc, ref)


def test_zeroed_fragment_is_flagged():
    alloc, ref = _case()
    alloc[272:288, 176:192] = 0
    rep = exact_report(alloc, ref)
    assert 'stored elements differ' in rep and 'bad rows 16, bad columns 16' in rep, rep


def test_overwritten_guard_cell_is_flagged():
    for r, c in ((0, 200), (299, 207), (300, 0), (307, 207)):                       # beside the first / last row, below the last row, the last cell
        alloc, ref = _case()
        alloc[r, c] = 1.0
        rep = exact_report(alloc, ref)
        assert '1 guard cells overwritten' in rep and f'row {r}, column {c}' in rep, rep
    idx = (torch.arange(300) // 60) * 61 + 1 + torch.arange(300) % 60
    alloc, ref = _case(row_index=idx, rows=5 * 61)
    alloc[61, 5] = ref[0, 5]                                                        # a gap row between two groups, written with a plausible value
    assert 'guard cells overwritten' in exact_report(alloc, ref, idx)
    alloc, ref = _case()
    as_bits(alloc)[300, 3] = SENTINEL_BITS[2] ^ 1                                   # another NaN is not the sentinel
    assert 'guard cells overwritten' in exact_report(alloc, ref)


def test_equal_pre_activations_with_different_outputs_are_flagged():
    g = torch.Generator().manual_seed(1)
    key = torch.randint(-40, 40, (64, 48), generator=g)                             # pre-activations in eighths
    x = key.double() / 8
    out = (x * torch.sigmoid(1.702 * x)).to(BF16)
    assert same_input_same_bits_report(key, out) == ''
    assert one_ulp_report(out, out.clone()) == ''
    bad = out.clone()
    r, c = [int(v) for v in (key == key[5, 7]).nonzero()[-1]]                        # another element with the pre-activation of [5, 7]
    assert (r, c) != (5, 7)
    as_bits(bad)[r, c] += 1
    assert int(bf16_ulp_distance(bad, out).max()) == 1
    assert one_ulp_report(bad, out) == ''                                           # inside the one-ulp band ...
    assert '1 of' in same_input_same_bits_report(key, bad)                          # ... but caught: same input, different bits
    far = out.clone()
    as_bits(far)[3, 3] += 2
    assert 'more than one bf16 ulp' in one_ulp_report(far, out)
    far = out.clone()
    far[3, 3] = float('nan')
    assert 'non-finite' in one_ulp_report(far, out)


def test_operand_padding_is_zero_then_nan():
    v = torch.ones(5, 13, dtype=BF16)
    a = padded_operand(v, 24, tail_rows=3)
    assert a.shape == (5, 13) and a.stride() == (24, 1)
    whole = torch.as_strided(a, (8, 24), (24, 1))
    assert torch.equal(whole[:5, :13], v) and (whole[:5, 13:16] == 0).all()
    assert torch.isnan(whole[:5, 16:].float()).all() and torch.isnan(whole[5:].float()).all()
