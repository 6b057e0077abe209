"""Direct tests of the include/mreserve_hip.h exports that so far ran only inside model-level tests: each against float64 torch or oracle/ref_torch.py,
at the sizes where its loops wrap, with strides wider than the extents and a sentinel in every cell the call must leave alone.  Labels and indices
stay inside their documented ranges: these tests check results, not what happens outside the contract."""
import numpy as np
import pytest
import torch

from util import SENTINEL_BITS, as_bits, bf16_ulp_distance, relerr

pytestmark = pytest.mark.gpu

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
BF16_MAX = float(torch.finfo(BF16).max)
F32_MAX = float(torch.finfo(F32).max)


@pytest.fixture
def dev():
    return torch.device('cuda:0')


def sentinel_like(shape, dtype, dev):
    t = torch.empty(shape, dtype=dtype, device=dev)
    as_bits(t).fill_(SENTINEL_BITS[t.element_size()])
    return t


def is_sentinel(t):
    return as_bits(t) == SENTINEL_BITS[t.element_size()]


# ---------------------------------------------------------------------------------------------------------------- mr_softmax_xent
@pytest.mark.parametrize('head_layout', [False, True], ids=['contiguous', 'answer-head'])
@pytest.mark.parametrize('C', [1, 4, 64])
@pytest.mark.parametrize('rows', [1, 8, 300])            # 300 > the kernel's 256 threads: its row loop runs
def test_softmax_xent(dev, rows, C, head_layout):
    from merlot_reserve_amd import ops
    row_stride, class_stride = (C * 8, 8) if head_layout else (C, 1)         # the finetune head: row_stride = A * 8, class_stride = 8
    g = torch.Generator().manual_seed(rows * 100 + C)
    x = (torch.randn(rows, C, generator=g) * 2).to(F32)
    labels = torch.randint(0, C, (rows,), generator=g)
    if C >= 2:                                                                # ties: the FIRST maximum is the prediction
        for r in range(0, rows, 3):
            c1, c2 = sorted(torch.randperm(C, generator=g)[:2].tolist())
            x[r, c1] = x[r, c2] = x[r].max() + 1
            labels[r] = c2 if (r // 3) % 2 else c1                            # the second maximum as the label is not a hit
    flat = torch.full((rows * row_stride,), float('nan'))
    cells = (torch.arange(rows)[:, None] * row_stride + torch.arange(C)[None, :] * class_stride).reshape(-1)
    flat[cells] = x.reshape(-1)
    coef = 0.25
    x64 = x.double()
    logp = torch.log_softmax(x64, -1)
    nll = -logp[torch.arange(rows), labels]
    first_max = torch.where(x == x.max(1, keepdim=True).values, torch.arange(C)[None, :], C).min(1).values
    want_loss = 3.0 + coef * nll.sum().item()
    want_correct = 5.0 + coef * (first_max == labels).sum().item()
    want_d = (coef * (torch.softmax(x64, -1) - torch.nn.functional.one_hot(labels, C).double())).to(BF16)
    d_logits, d_labels = flat.to(dev), labels.to(torch.int32).to(dev)
    loss, correct = torch.full((1,), 3.0, device=dev), torch.full((1,), 5.0, device=dev)      # both accumulate: they start non-zero
    dl = sentinel_like((rows * row_stride,), BF16, dev)
    ops.softmax_xent(d_logits, row_stride, class_stride, d_labels, rows, C, coef, loss, correct, dl)
    print(f'softmax_xent rows={rows} C={C}: loss {loss.item():.7f} want {want_loss:.7f}; correct {correct.item()} want {want_correct}')
    assert abs(loss.item() - want_loss) <= 1e-4 * abs(want_loss)
    assert correct.item() == want_correct                                     # multiples of 1 / 4: exact in fp32
    got_d = dl.cpu()[cells].reshape(rows, C)
    assert int(bf16_ulp_distance(got_d, want_d).max()) <= 1
    between = torch.ones(rows * row_stride, dtype=torch.bool)
    between[cells] = False
    assert is_sentinel(dl.cpu())[between].all(), 'a cell between the strides was written'
    # correct_out = NULL and dlogits = NULL: the same loss bits (fixed-order sums), nothing else touched
    loss2 = torch.full((1,), 3.0, device=dev)
    ops.softmax_xent(d_logits, row_stride, class_stride, d_labels, rows, C, coef, loss2, None, None)
    assert torch.equal(loss2, loss)
    loss3, dl3 = torch.full((1,), 3.0, device=dev), sentinel_like((rows * row_stride,), BF16, dev)
    ops.softmax_xent(d_logits, row_stride, class_stride, d_labels, rows, C, coef, loss3, None, dl3)
    assert torch.equal(loss3, loss) and torch.equal(as_bits(dl3), as_bits(dl))


# ---------------------------------------------------------------------------------------------------------------- mr_masked_lm_xent
@pytest.mark.parametrize('n,V', [(301, 100), (7, 32768)])          # n is not a multiple of the kernel's 4 rows per workgroup
def test_masked_lm_xent(dev, n, V):
    """out2 and dlogits against float64 autograd.  Tolerances from the arithmetic: the kernel works in fp32 (eps = 6e-8); a row's sum of V <= 32768
    exponentials in per-thread partials and a tree costs at most ~150 eps relative, log and exp a few ulp each: the loss, ~ ln V, is good to 1e-5
    relative or better; 1e-4 is the bound tests/test_kernels_gpu.py::test_contrastive_lse uses for the same quantity.  A gradient element
    (p - onehot) / count inherits p's relative error (<= ~2e-5) as an ABSOLUTE error p / count when it cancels against the one-hot: 1e-4 * (|ref| + p / count)."""
    from merlot_reserve_amd import ops
    ldl = V + 8
    g = torch.Generator().manual_seed(V + n)
    x = (torch.randn(n, V, generator=g) * 3).to(F32)
    labels = torch.randint(1, V, (n,), generator=g)
    labels[::3] = 0                                                         # label 0 = masked out
    labels[1] = V - 1
    alloc = torch.full((n, ldl), float('nan'))
    alloc[:, :V] = x
    xr = x.double().requires_grad_(True)
    mask = (labels != 0).double()
    logp = torch.log_softmax(xr, -1)[torch.arange(n), labels]
    ref = -(mask * logp).sum() / mask.sum()
    ref.backward()
    p_over_count = torch.softmax(x.double(), -1) / mask.sum()
    d_alloc, d_labels = alloc.to(dev), labels.to(torch.int32).to(dev)
    logits = d_alloc[:, :V]
    out2 = sentinel_like((2,), F32, dev)
    dl_alloc = sentinel_like((n, ldl), F32, dev)
    ops.masked_lm_xent(logits, d_labels, out2, dl_alloc[:, :V])
    print(f'masked_lm_xent n={n} V={V}: loss {out2[0].item():.7f} want {ref.item():.7f}; count {out2[1].item()}')
    assert abs(out2[0].item() - ref.item()) <= 1e-4 * abs(ref.item())
    assert out2[1].item() == mask.sum().item()
    got = dl_alloc.cpu()
    assert is_sentinel(got[:, V:]).all(), 'the padding of dlogits was written'
    err = (got[:, :V].double() - xr.grad).abs()
    tol = 1e-4 * (xr.grad.abs() + p_over_count)
    assert (err <= tol).all(), f'{int((err > tol).sum())} gradient elements outside the bound, worst {float((err / tol).max()):.3g} x'
    out2b, dl_b = sentinel_like((2,), F32, dev), sentinel_like((n, ldl), F32, dev)
    ops.masked_lm_xent(logits, d_labels, out2b, dl_b[:, :V])               # fixed-order sums: identical bits
    assert torch.equal(out2b, out2) and torch.equal(as_bits(dl_b), as_bits(dl_alloc))
    out2c = sentinel_like((2,), F32, dev)
    ops.masked_lm_xent(logits, d_labels, out2c, None)
    assert torch.equal(out2c, out2)


# ---------------------------------------------------------------------------------------------------------------- hi / lo split
def wide_f32(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * torch.exp(torch.randn(shape, generator=g) * 6)).to(F32)


def test_split_hilo(dev):
    from merlot_reserve_amd import ops
    n = 4096 * 256 + 100003                                                 # more than the capped grid covers in one pass; not a multiple of 256
    x = wide_f32((n,), 5)
    x[:4] = torch.tensor([0.0, -0.0, 1.0, -3.0])
    hi_ref = x.to(BF16)
    lo_ref = (x - hi_ref.float()).to(BF16)                                  # x - hi is exact in fp32
    hi, lo = sentinel_like((n + 64,), BF16, dev), sentinel_like((n + 64,), BF16, dev)
    ops.split_hilo(x.to(dev), hi[:n], lo[:n])
    assert torch.equal(as_bits(hi[:n].cpu()), as_bits(hi_ref)) and torch.equal(as_bits(lo[:n].cpu()), as_bits(lo_ref))
    assert is_sentinel(hi[n:]).all() and is_sentinel(lo[n:]).all()


def test_split_hilo_rows(dev):
    from merlot_reserve_amd import ops
    rows, cols, lds, ldo = 37, 100, 108, 104
    x = wide_f32((rows, cols), 6)
    src = torch.full((rows, lds), float('nan'))
    src[:, :cols] = x
    hi_ref = x.to(BF16)
    lo_ref = (x - hi_ref.float()).to(BF16)
    hi, lo = sentinel_like((rows + 2, ldo), BF16, dev), sentinel_like((rows + 2, ldo), BF16, dev)
    ops.split_hilo_rows(src.to(dev)[:, :cols], hi[:rows, :cols], lo[:rows, :cols])
    for got, ref in ((hi.cpu(), hi_ref), (lo.cpu(), lo_ref)):
        assert torch.equal(as_bits(got[:rows, :cols].contiguous()), as_bits(ref))
        assert is_sentinel(got[:rows, cols:]).all() and is_sentinel(got[rows:]).all(), 'padding written'


# ---------------------------------------------------------------------------------------------------------------- mr_transpose_leaves
def test_transpose_leaves(dev):
    from merlot_reserve_amd import ops
    shapes = [(64, 64), (128, 192), (768, 3072)]
    offs, tile0, leaves, off, t = [], [], [], 2048, 0                        # leaves at non-zero offsets, with gaps between them
    for r, c in shapes:
        leaves.append([off, r, c, t])
        offs.append(off)
        tile0.append(t)
        off += r * c + 4096
        t += (r // 64) * (c // 64)
    total, ntile = off, t
    assert ntile == 1 + 6 + 576
    g = torch.Generator().manual_seed(9)
    work = torch.randint(-32768, 32767, (total,), generator=g, dtype=torch.int16).view(BF16).to(dev)       # any bit pattern: a transpose moves words
    table = torch.tensor(leaves, dtype=torch.int32, device=dev)

    def expected(lo, hi):
        exp = torch.full((total,), SENTINEL_BITS[2], dtype=torch.int16, device=dev)
        wb = as_bits(work)
        for (o, r, c, t0) in leaves:
            src = wb[o:o + r * c].view(r, c)
            dst = exp[o:o + r * c].view(c, r)                                # workT[off + n * rows + k] = work[off + k * cols + n]
            tc = c // 64
            for tile in range(max(lo, t0), min(hi, t0 + (r // 64) * tc)):
                r0, c0 = ((tile - t0) // tc) * 64, ((tile - t0) % tc) * 64
                dst[c0:c0 + 64, r0:r0 + 64] = src[r0:r0 + 64, c0:c0 + 64].t()
        return exp

    for lo, hi in ((0, ntile), (3, 300), (1, 7), (582, 583)):               # everything; starting and ending inside leaves; one leaf; the last tile
        workT = sentinel_like((total,), BF16, dev)
        ops.transpose_leaves(work, workT, table, len(leaves), lo, hi)
        assert torch.equal(as_bits(workT), expected(lo, hi)), f'tiles [{lo}, {hi})'


# ---------------------------------------------------------------------------------------------------------------- nan_to_num / cast
BIG_N = 8192 * 256 * 8 + 8 * 1237          # past one pass of the capped grid (8192 blocks x 256 threads x 8 elements), ragged multiple of 8


def test_nan_to_num_bf16(dev):
    from merlot_reserve_amd import ops
    g = torch.Generator().manual_seed(11)
    words = torch.randint(-32768, 32767, (BIG_N,), generator=g, dtype=torch.int16)          # every class of bf16 word, NaNs, infinities, denormals included
    words[:8] = torch.tensor([0x7FC0, 0x7F80, 0xFF80 - 65536, 0x8000 - 65536, 0x0001, 0x8001 - 65536, 0x7F7F, 0x7F81], dtype=torch.int16)
    words[-3:] = torch.tensor([0x7F80, 0xFFC1 - 65536, 0x0040], dtype=torch.int16)
    x = words.view(BF16)
    xf = x.float()
    want = words.clone()
    want[torch.isnan(xf)] = 0
    want[xf == float('inf')] = 0x7F7F                                       # the largest bf16
    want[xf == -float('inf')] = 0xFF7F - 65536
    assert (want != words).sum() > BIG_N // 500                             # ... and -0.0, denormals, ordinary values: bit-unchanged
    buf = sentinel_like((BIG_N + 64,), BF16, dev)
    buf[:BIG_N] = x.to(dev)
    ops.nan_to_num_(buf[:BIG_N])
    got = as_bits(buf.cpu())
    assert torch.equal(got[:BIG_N], want)
    assert (got[BIG_N:] == SENTINEL_BITS[2]).all()


def test_cast_f32_to_bf16_params(dev):
    from merlot_reserve_amd import ops
    x = wide_f32((BIG_N,), 12)
    x[:6] = torch.tensor([0.0, -0.0, float('inf'), -float('inf'), 1.00390625, -1.01171875])    # (ties to even on both sides)
    work = sentinel_like((BIG_N + 64,), BF16, dev)
    ops.cast_params(x.to(dev), work[:BIG_N])
    got = as_bits(work.cpu())
    assert torch.equal(got[:BIG_N], as_bits(x.to(BF16)))
    assert (got[BIG_N:] == SENTINEL_BITS[2]).all()


# ---------------------------------------------------------------------------------------------------------------- Adam
def words(t):
    return t.reshape(-1).contiguous().view(torch.int16).to(torch.int32) & 0xFFFF


def assert_state_words(name, got, ref):
    """The criterion of tests/test_kernels_gpu.py::test_adam_bf16_state_words_bit_exact: >= 99.9 % of the words equal, the rest neighbouring codes."""
    gb, rb = words(got), words(ref)
    neq = (gb != rb).nonzero().reshape(-1)
    frac = 1.0 - neq.numel() / gb.numel()
    print(f'adam state {name}: {gb.numel() - neq.numel()} of {gb.numel()} bf16 words equal ({frac * 100:.4f} %)')
    assert frac >= 0.999, (name, frac)
    for i in neq.tolist():
        a, b = int(gb[i]), int(rb[i])
        assert abs((a & 0x7FFF) - (b & 0x7FFF)) <= 1, (name, i, hex(a), hex(b))


def adam_state(n, seed):
    from oracle import ref_torch as R
    g = torch.Generator().manual_seed(seed)
    master = torch.randn(n, generator=g) * 0.05
    grad = (torch.randn(n, generator=g) * 1e-3 * torch.exp(torch.randn(n, generator=g))).to(BF16)
    mu = (torch.randn(n, generator=g) * 1e-3).to(BF16)
    nu = R.unsigned_bf16_encode((torch.rand(n, generator=g) * 1e-3 * torch.exp(torch.randn(n, generator=g))).float())
    nu[:64] = 0.0
    return master, grad, mu, nu


class DevState:
    """master / work / mu / nu on the device (work starts as a sentinel: every word must be written)."""

    def __init__(self, dev, master, mu, nu):
        self.master, self.mu, self.nu = master.to(dev).clone(), mu.to(dev).clone(), nu.to(dev).clone()
        self.work = sentinel_like(master.shape, BF16, dev)

    def buffers(self):
        return (self.master, self.work, self.mu, self.nu)

    def same_bits(self, other, sl=slice(None)):
        return all(torch.equal(as_bits(a[sl]), as_bits(b[sl])) for a, b in zip(self.buffers(), other.buffers()))


B1, B2, EPS, WD, LR = 0.9, 0.98, 1e-6, 0.1, 4e-4


def hyper_vector(dev, sched, neg_lr, bc1, bc2):
    return torch.tensor([np.float32(sched), np.float32(neg_lr), np.float32(1) / np.float32(bc1), np.float32(1) / np.float32(bc2)],
                        dtype=F32, device=dev)


def test_adam_finetune_against_the_oracle(dev):
    """mr_adam_bf16_update_finetune against R.finetune_adam_apply, decay flags on and off: the checks of test_adam_bf16 (master to 1e-6, working copy =
    bf16(master)) and the state-word criterion of test_adam_bf16_state_words_bit_exact."""
    from merlot_reserve_amd import ops
    from oracle import ref_torch as R
    nblk = 32
    n = 2048 * nblk
    master, grad, mu, nu = adam_state(n, 21)
    orig = (master * 0.5).to(BF16)                                          # far enough from the parameters for the decay term to show
    flags = (torch.arange(nblk) % 2 == 0).to(torch.uint8)                    # decay on in the even blocks
    cfg = dict(learning_rate=LR, num_train_steps=20000, num_warmup_steps=1000, weight_decay_rate=WD, beta_2=B2, eps=EPS)
    count = 1500
    sched = float(R.lr_scale_linearwarmup_lineardecay(count, 1000, 20000))
    bc1, bc2 = float(np.float32(1 - B1 ** (count + 1))), float(np.float32(1 - B2 ** (count + 1)))
    st = DevState(dev, master, mu, nu)
    ops.adam_bf16_update_finetune(st.master, st.work, grad.to(dev), st.mu, st.nu, orig.to(dev), flags.to(dev), B1, B2, EPS, WD, sched, -LR, bc1, bc2)
    el = flags.repeat_interleave(2048).bool()
    for decay in (True, False):
        sel = el if decay else ~el
        shape = (-1, 1) if decay else (-1,)                                  # ndim > 1 and size > 4096 <=> the decay mask
        newp, nm, nv = R.finetune_adam_apply(master[sel].reshape(shape), orig[sel].reshape(shape), grad[sel].float().reshape(shape),
                                             mu[sel].reshape(shape), nu[sel].reshape(shape), count, cfg)
        assert relerr(st.master.cpu()[sel], newp.reshape(-1)) < 1e-6, decay
        assert_state_words(f'finetune mu decay={decay}', st.mu.cpu()[sel], nm)
        assert_state_words(f'finetune nu decay={decay}', st.nu.cpu()[sel], nv)
    assert torch.equal(as_bits(st.work), as_bits(st.master.to(BF16)))
    # decay matters: the two halves would not pass each other's reference
    newp_wrong, _, _ = R.finetune_adam_apply(master[el], orig[el], grad[el].float(), mu[el], nu[el], count, cfg)
    assert relerr(st.master.cpu()[el], newp_wrong) > 1e-6


@pytest.mark.parametrize('finetune', [False, True], ids=['pretrain', 'finetune'])
def test_adam_dev_scalars_equal_host_scalars_bit_for_bit(dev, finetune):
    """mr_adam_bf16_update_dev, both chains: all four output buffers identical to the host-scalar entry point's, with
    hyper = {sched, neg_lr, fp32(1) / fp32(bc1), fp32(1) / fp32(bc2)}; a run on a sub-range (pointers offset by a multiple of 2048 elements, flags
    by the same number of blocks) is identical to that range of the full run and leaves the rest alone."""
    from merlot_reserve_amd import ops
    nblk = 8
    n = 2048 * nblk
    master, grad, mu, nu = adam_state(n, 31)
    grad[5], grad[6], grad[7] = float('nan'), float('inf'), -float('inf')
    orig = master.to(BF16)
    flags = torch.tensor([1, 0, 1, 1, 0, 0, 1, 0], dtype=torch.uint8).to(dev)
    sched, bc1, bc2 = 0.37, float(np.float32(1 - B1 ** 41)), float(np.float32(1 - B2 ** 41))
    d_grad, d_orig = grad.to(dev), orig.to(dev) if finetune else None
    host = DevState(dev, master, mu, nu)
    if finetune:
        ops.adam_bf16_update_finetune(host.master, host.work, d_grad, host.mu, host.nu, d_orig, flags, B1, B2, EPS, WD, sched, -LR, bc1, bc2)
    else:
        ops.adam_bf16_update(host.master, host.work, d_grad, host.mu, host.nu, flags, B1, B2, EPS, WD, sched, -LR, bc1, bc2)
    hyper = hyper_vector(dev, sched, -LR, bc1, bc2)
    full = DevState(dev, master, mu, nu)
    ops.adam_bf16_update_dev(full.master, full.work, d_grad, full.mu, full.nu, d_orig, flags, B1, B2, EPS, WD, hyper)
    assert full.same_bits(host)
    part = DevState(dev, master, mu, nu)
    start = DevState(dev, master, mu, nu)
    sl = slice(2 * 2048, 5 * 2048)
    ops.adam_bf16_update_dev(part.master[sl], part.work[sl], d_grad[sl], part.mu[sl], part.nu[sl], None if d_orig is None else d_orig[sl],
                             flags[2:5], B1, B2, EPS, WD, hyper)
    assert part.same_bits(full, sl)
    for rest in (slice(0, 2 * 2048), slice(5 * 2048, n)):
        assert part.same_bits(start, rest)


def f32grad_update(dev, st, grad_f32, flags, hyper):
    from merlot_reserve_amd import _lib, ops
    assert grad_f32.dtype == F32
    _lib.check(_lib.load().mr_adam_f32grad_update_dev(st.master.data_ptr(), st.work.data_ptr(), grad_f32.data_ptr(), st.mu.data_ptr(), st.nu.data_ptr(),
                                                      flags.data_ptr(), st.master.numel(), B1, B2, EPS, WD, hyper.data_ptr(),
                                                      torch.cuda.current_stream().cuda_stream), 'mr_adam_f32grad_update_dev')


def test_adam_f32grad(dev):
    """mr_adam_f32grad_update_dev: bit-identical to the bf16-gradient entry point when the fp32 gradients are bf16-representable; against
    R.adam_bf16_apply when they are not; +-inf gradients clamp at the fp32 range and NaN counts as 0."""
    from merlot_reserve_amd import ops
    from oracle import ref_torch as R
    nblk = 32
    n = 2048 * nblk
    master, grad, mu, nu = adam_state(n, 41)
    flags_h = (torch.arange(nblk) % 3 != 0).to(torch.uint8)
    flags = flags_h.to(dev)
    count = 4000
    cfg = dict(learning_rate=LR, num_train_steps=750000, num_warmup_steps=3750, weight_decay_rate=WD, beta_2=B2, eps=EPS, use_bfloat16_adam=True)
    sched = float(R.lr_scale_linearwarmup_cosinedecay(count, 3750, 750000, 0.02))
    hyper = hyper_vector(dev, sched, -LR, 1.0, 1.0)
    a, b = DevState(dev, master, mu, nu), DevState(dev, master, mu, nu)
    ops.adam_bf16_update_dev(a.master, a.work, grad.to(dev), a.mu, a.nu, None, flags, B1, B2, EPS, WD, hyper)
    f32grad_update(dev, b, grad.float().to(dev), flags, hyper)
    assert b.same_bits(a)
    # gradients with 24-bit mantissas: no bf16 round trip, so the oracle is fed the fp32 values
    g32 = (torch.randn(n, generator=torch.Generator().manual_seed(42)) * 1e-3).to(F32)
    assert not torch.equal(g32.to(BF16).float(), g32)
    c = DevState(dev, master, mu, nu)
    f32grad_update(dev, c, g32.to(dev), flags, hyper)
    el = flags_h.repeat_interleave(2048).bool()
    for decay in (True, False):
        sel = el if decay else ~el
        shape = (-1, 1) if decay else (-1,)
        newp, nm, nv = R.adam_bf16_apply(master[sel].reshape(shape), g32[sel].reshape(shape), mu[sel].reshape(shape), nu[sel].reshape(shape), count, cfg)
        assert relerr(c.master.cpu()[sel], newp.reshape(-1)) < 1e-6, decay
        assert_state_words(f'f32grad mu decay={decay}', c.mu.cpu()[sel], nm)
        assert_state_words(f'f32grad nu decay={decay}', c.nu.cpu()[sel], nv)
    assert torch.equal(as_bits(c.work), as_bits(c.master.to(BF16)))
    # non-finite gradients: NaN -> 0, +-inf -> +-the largest fp32 (bit-identical to a run that is handed those values)
    bad, clean = g32.clone(), g32.clone()
    bad[3], bad[2048 + 9], bad[5000] = float('nan'), float('inf'), -float('inf')
    clean[3], clean[2048 + 9], clean[5000] = 0.0, F32_MAX, -F32_MAX
    d, e = DevState(dev, master, mu, nu), DevState(dev, master, mu, nu)
    f32grad_update(dev, d, bad.to(dev), flags, hyper)
    f32grad_update(dev, e, clean.to(dev), flags, hyper)
    assert d.same_bits(e)
    assert not torch.isnan(d.mu.float()).any()


def test_f32_axpby_and_nan_to_num(dev):
    """mr_f32_axpby and mr_f32_nan_to_num (no ops wrapper of their own: ops.add_ and ops.nan_to_num_ reach them for fp32 tensors) against torch.
    y = a x + b y is two products and a sum, or one product and a fused multiply-add: either way within 2^-23 (|a x| + |b y|) of the exact value (three roundings of 2^-24 each, to first order)."""
    from merlot_reserve_amd import _lib
    lib = _lib.load()
    n = 4096 * 256 + 1003
    x, y = wide_f32((n,), 51).clamp(-1e30, 1e30), wide_f32((n,), 52).clamp(-1e30, 1e30)
    stream = torch.cuda.current_stream().cuda_stream
    xd = x.to(dev)
    for a, b in ((1.0, 1.0), (0.5, 0.0), (-1.25, 0.75), (0.3, -1.7)):
        buf = sentinel_like((n + 16,), F32, dev)
        buf[:n] = y.to(dev)
        _lib.check(lib.mr_f32_axpby(buf.data_ptr(), xd.data_ptr(), a, b, n, stream), 'mr_f32_axpby')
        got = buf.cpu()
        af, bf = float(np.float32(a)), float(np.float32(b))
        exact = af * x.double() + bf * y.double()
        bound = 1.001 * 2.0 ** -23 * ((af * x.double()).abs() + (bf * y.double()).abs())
        assert ((got[:n].double() - exact).abs() <= bound).all(), (a, b)
        if (a, b) == (1.0, 1.0):
            assert torch.equal(got[:n], x + y)
        assert is_sentinel(got[n:]).all()
    z = wide_f32((n,), 53)
    z[:5] = torch.tensor([float('nan'), float('inf'), -float('inf'), -0.0, 1e-42])
    z[-1] = float('nan')
    buf = sentinel_like((n + 16,), F32, dev)
    buf[:n] = z.to(dev)
    _lib.check(lib.mr_f32_nan_to_num(buf.data_ptr(), n, stream), 'mr_f32_nan_to_num')
    got = buf.cpu()
    assert torch.equal(as_bits(got[:n]), as_bits(torch.nan_to_num(z, nan=0.0, posinf=F32_MAX, neginf=-F32_MAX)))
    assert is_sentinel(got[n:]).all()
