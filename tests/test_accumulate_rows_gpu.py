"""The identity case of mr_segment_sum (indptr == indices == NULL: dst row i (+)= scale * src row i) through ops.accumulate_rows, element by element.

The reference is torch on the host: `dst + scale * src.float()` in fp32 (`scale * src.float()` without accumulate), for a bf16 destination taken through
util.exact_bf16, i.e. the data are integers for which the bf16 result loses nothing.  scale in {1, 0.5, 0.25} makes the product exact, so the result is
known to the bit whether or not the compiler contracts the multiply and the add into an fma.  scale = 1/3: the kernel may round the product (like the
reference) or not (fma); with operands of ONE sign the result is at least as large as the product, the product's rounding error is at most half an ulp of
the result, and the two evaluations are at most one fp32 ulp apart -- the data of that case are positive for this reason (with cancellation the bound
of one ulp of a small difference would not follow from anything).

Shapes: one 16-byte vector; a tail far shorter than a workgroup's span; a width that is no multiple of 64 lanes x 8 elements; more rows than
workgroups; and (2050, 2048) = 524800 vectors, 512 more than the capped grid of 2048 x 256 lanes covers in one pass, so the grid stride is taken.
Every shape runs flat (ld == H: one range) and with padded leading dimensions (NaN behind every source row, sentinels behind every destination row)."""
import ctypes as C

import pytest
import torch

from util import as_bits, exact_bf16, exact_report, guarded_output, padded_operand

pytestmark = pytest.mark.gpu

BF16, F32 = torch.bfloat16, torch.float32
SHAPES = [(1, 8), (3, 8), (5, 2056), (4097, 128), (1030, 2048), (2050, 2048)]
MR_EINVAL = -1


def _data(rows, H, dst_dtype, seed):
    """(src bf16, dst0) on the host.  bf16 destination: integers, src multiples of 4 in [-64, 64], dst0 in [-64, 64]: dst0 + s * src is an integer of
    magnitude <= 128 for s in {1, 1/2, 1/4}.  fp32 destination: any values."""
    g = torch.Generator().manual_seed(seed)
    if dst_dtype == BF16:
        src = (4 * torch.randint(-16, 17, (rows, H), generator=g)).to(BF16)
        dst0 = torch.randint(-64, 65, (rows, H), generator=g).to(BF16)
    else:
        src = torch.randn(rows, H, generator=g).to(BF16)
        dst0 = torch.randn(rows, H, generator=g) * 3
    return src, dst0


def _reference(src, dst0, scale, accumulate, dst_dtype):
    s = torch.tensor(scale, dtype=F32)
    ref = s * src.float()
    if accumulate:
        ref = dst0.float() + ref
    return exact_bf16(ref.double()) if dst_dtype == BF16 else ref


def _operands(src, dst0, padded, dev):
    rows, H = src.shape
    if padded:
        s = padded_operand(src.to(dev), H + 8)
        alloc = guarded_output(rows, H + 24, dst0.dtype, dev)
    else:
        s = src.to(dev)
        alloc = guarded_output(rows, H, dst0.dtype, dev)
    return s, alloc


@pytest.mark.parametrize('padded', [False, True], ids=['flat', 'padded_ld'])
@pytest.mark.parametrize('accumulate', [True, False], ids=['accumulate', 'overwrite'])
@pytest.mark.parametrize('dst_dtype', [F32, BF16], ids=['f32', 'bf16'])
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: f'{s[0]}x{s[1]}')
def test_accumulate_rows_is_exact(dev, shape, dst_dtype, accumulate, padded):
    from merlot_reserve_amd import ops
    rows, H = shape
    src, dst0 = _data(rows, H, dst_dtype, seed=rows * 31 + H)
    s, alloc = _operands(src, dst0, padded, dev)
    for scale in (1.0, 0.5, 0.25):
        ref = _reference(src, dst0, scale, accumulate, dst_dtype).to(dev)
        runs = []
        for _ in range(2):                       # the same launch twice: the same bits
            alloc[:rows, :H] = dst0.to(dev)
            ops.accumulate_rows(s, alloc[:rows, :H], scale=scale, accumulate=accumulate)
            rep = exact_report(alloc, ref)
            assert rep == '', f'{shape} scale {scale}: {rep}'
            runs.append(as_bits(alloc).clone())
        assert torch.equal(runs[0], runs[1])


def _ordered(t):
    w = as_bits(t.contiguous()).to(torch.int64)
    return torch.where(w < 0, -(w & 0x7FFFFFFF), w)


@pytest.mark.parametrize('padded', [False, True], ids=['flat', 'padded_ld'])
@pytest.mark.parametrize('shape', [(5, 2056), (4097, 128)], ids=lambda s: f'{s[0]}x{s[1]}')
def test_scale_one_third_within_one_fp32_ulp(dev, shape, padded):
    from merlot_reserve_amd import ops
    rows, H = shape
    g = torch.Generator().manual_seed(5)
    src = (torch.rand(rows, H, generator=g) + 0.5).to(BF16)           # one sign: see the module docstring
    dst0 = torch.rand(rows, H, generator=g) * 4 + 0.25
    scale = 1.0 / 3.0
    for accumulate in (True, False):
        s, alloc = _operands(src, dst0, padded, dev)
        alloc[:rows, :H] = dst0.to(dev)
        ops.accumulate_rows(s, alloc[:rows, :H], scale=scale, accumulate=accumulate)
        ref = _reference(src, dst0, scale, accumulate, F32).to(dev)
        got = alloc[:rows, :H]
        d = (_ordered(got) - _ordered(ref)).abs()
        print(f'{shape} accumulate {accumulate}: max distance {int(d.max())} ulp, {int((d > 0).sum())} of {d.numel()} elements differ')
        assert bool(torch.isfinite(got).all()) and int(d.max()) <= 1
        probe = alloc.clone()
        probe[:rows, :H] = ref                    # (the guard cells: untouched)
        assert exact_report(probe, ref) == ''


def test_one_dimensional_buffers_are_one_flat_range(dev):
    """The flat gradient buffers of a ParamStore: 1-D, a multiple of 2048 elements."""
    from merlot_reserve_amd import ops
    n = 3 * 2048
    src, dst0 = _data(1, n, F32, seed=9)
    acc = dst0.view(-1).to(dev).clone()
    ops.accumulate_rows(src.view(-1).to(dev), acc, scale=0.25)
    assert torch.equal(as_bits(acc), as_bits(_reference(src, dst0, 0.25, True, F32).view(-1).to(dev)))


def test_refusals_launch_nothing(dev):
    """n0 != n_dst, a second source table, one list NULL and the other not: MR_EINVAL with a message, the destination untouched."""
    from merlot_reserve_amd import _lib
    lib = _lib.load()
    rows, H = 6, 64
    src = torch.ones(rows, H, dtype=BF16, device=dev)
    lists = torch.arange(rows + 1, dtype=torch.int32, device=dev)
    nothing = torch.empty(0, 1, dtype=F32, device=dev)

    def call(n0=rows, src1=None, n1=0, indptr=None, indices=None):
        alloc = guarded_output(rows, H, F32, dev)
        rc = lib.mr_segment_sum(src.data_ptr(), H, n0, src1, H if src1 else 0, n1, None, 0, 0, indptr, indices, alloc.data_ptr(), H, 1, rows, H,
                                C.c_float(1.0), 1, torch.cuda.current_stream().cuda_stream)
        msg = lib.mr_last_error().decode()
        torch.cuda.synchronize()
        assert exact_report(alloc, nothing) == '', 'a refused call wrote to the destination'
        return rc, msg

    for kw in (dict(n0=rows - 1), dict(n0=rows + 1), dict(src1=src.data_ptr()), dict(src1=src.data_ptr(), n1=rows),
               dict(indptr=lists.data_ptr()), dict(indices=lists.data_ptr())):
        rc, msg = call(**kw)
        assert rc == MR_EINVAL and 'mr_segment_sum' in msg, (kw, rc, msg)
