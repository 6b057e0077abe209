"""The k-loop of the grouped TN weight-gradient kernel (g3::gemm3_tn_kernel) at the sizes where its ring schedule can go wrong, element for element.

The kernel stages A [64 k][256] in a 3-stage ring two k-tiles ahead and B in a 2-stage ring, reads fragments behind counted lgkmcnt waits (the second row
half's fragments are requested inside the first MFMA block) and meets its partner wave group at four barriers per k-tile.  K walks the ring depths:
64 = one k-tile (the prologue alone feeds it), 128 = the B ring's depth, 192 = the A ring's, 256, 320 = both rings wrap, 328 = a ragged last k-tile
(8 valid rows, the rest the descriptor's zero fill), 2056 = 32 full k-tiles and a ragged one.  (M, N) = (8, 8): one tile with 8 valid rows and columns;
(256, 256): one exact tile; (264, 776), (520, 264): several tiles with a ragged last one on either side.

The method is that of tests/test_gemm_exact_gpu.py: integer operands in [-2, 2], so every partial sum is an integer below 2^24 and fp32 accumulation is
exact in any order; operands are leading views of NaN-padded allocations with unequal lda / ldb, outputs of sentinel-filled ones with ldc = N + 8; the
comparison is on the bits, and every guard cell must keep its sentinel.  The route is forced (gemm3 = 256) and the kernel name asserted.

The last test holds the barrier / wait pattern to determinism on gaussian data (where a stale or early fragment would change low bits, not only exact
integers): two launches of one group agree bit for bit, and agree with the same members launched one per call."""
import pytest
import torch

from util import as_bits, exact_report, guarded_output, padded_operand

pytestmark = pytest.mark.gpu

BF16, F64 = torch.bfloat16, torch.float64
KS = [64, 128, 192, 256, 320, 328, 2056]
MNS = [(8, 8), (256, 256), (264, 776), (520, 264)]
TN_MAXG = 20                                        # csrc/gemm_plan.h
# groups of 1, 3 and TN_MAXG members of mixed sizes (the shapes above, cycled)
GROUPS = {1: [(264, 776)], 3: [(8, 8), (520, 264), (256, 256)], TN_MAXG: [MNS[k % 4] for k in range(TN_MAXG)]}


@pytest.fixture
def dev():
    return torch.device('cuda:0')


def ceil8(n):
    return (n + 7) // 8 * 8


class Member:
    """One problem C[M, N] = A^T B with A stored [K, M], B stored [K, N]: integer operands, the exact reference, a guarded output."""

    def __init__(self, dev, M, N, K, seed):
        gen = torch.Generator(device=dev).manual_seed(seed)
        A = torch.randint(-2, 3, (K, M), device=dev, generator=gen).to(BF16)
        B = torch.randint(-2, 3, (K, N), device=dev, generator=gen).to(BF16)
        self.acc = A.double().t() @ B.double()                    # integers, |.| <= 4 K < 2^24
        self.a = padded_operand(A, ceil8(M) + 24)
        self.b = padded_operand(B, ceil8(N) + 8)
        self.M, self.N, self.K = M, N, K

    def expected(self):
        """fp32 accumulation of integers below 2^24 is exact in any order; the stored value is its round-to-nearest-even bf16."""
        v32 = self.acc.to(torch.float32)
        assert torch.equal(v32.double(), self.acc)
        return v32.to(BF16)

    def output(self, dev):
        return guarded_output(self.M, self.N + 8, BF16, dev)


_MEMBERS = {}


def member(dev, M, N, K, slot=0):
    key = (M, N, K, slot)
    if key not in _MEMBERS:
        if len(_MEMBERS) > 64:
            _MEMBERS.clear()
        _MEMBERS[key] = Member(dev, M, N, K, 7919 * M + 104729 * N + 31 * K + slot)
    return _MEMBERS[key]


def launch(members, outs):
    """One forced grouped launch; returns the kernel name."""
    from merlot_reserve_amd import _lib, ops
    prev = {k: ops.get_option(k) for k in ('gemm3', 'gemm_trace')}
    try:
        ops.set_option('gemm3', 256)
        ops.set_option('gemm_trace', 1)
        ops.gemm_grouped([ops.gemm_args(m.a, m.b, o[:m.M, :m.N], transA=True) for m, o in zip(members, outs)])
        return _lib.load().mr_last_gemm_kernel().decode()
    finally:
        for k, v in prev.items():
            ops.set_option(k, v)


def check(members, outs, name, tag):
    assert name == f'g3::gemm3_tn_kernel grouped x{len(members)}', f'{tag}: meant to test the TN ping-pong kernel, ran {name}'
    for m, o in zip(members, outs):
        rep = exact_report(o, m.expected())
        assert rep == '', f'{tag}: member {m.M}x{m.N}x{m.K}: {rep}'


@pytest.mark.parametrize('K', KS)
@pytest.mark.parametrize('M,N', MNS)
def test_tn_kloop_single_member(dev, M, N, K):
    m = member(dev, M, N, K)
    outs = [m.output(dev)]
    check([m], outs, launch([m], outs), f'TN {M}x{N}x{K}')


@pytest.mark.parametrize('K', KS)
@pytest.mark.parametrize('count', [3, TN_MAXG])
def test_tn_kloop_groups(dev, count, K):
    members = [member(dev, M, N, K, slot) for slot, (M, N) in enumerate(GROUPS[count])]
    outs = [m.output(dev) for m in members]
    check(members, outs, launch(members, outs), f'TN group x{count} K={K}')


def test_tn_kloop_group_is_deterministic_and_equals_single_launches(dev):
    """Gaussian data, K = 2056 (33 k-tiles, a ragged last one), three members of mixed sizes: the grouped launch twice and one launch per member."""
    K = 2056
    gen = torch.Generator(device=dev).manual_seed(20240607)

    class G:
        pass
    members = []
    for M, N in GROUPS[3]:
        g = G()
        g.M, g.N, g.K = M, N, K
        g.a = padded_operand(torch.randn(K, M, device=dev, generator=gen).to(BF16), ceil8(M) + 24)
        g.b = padded_operand((torch.randn(K, N, device=dev, generator=gen) * 0.05).to(BF16), ceil8(N) + 8)
        members.append(g)
    runs = []
    for _ in range(2):
        outs = [guarded_output(g.M, g.N + 8, BF16, dev) for g in members]
        name = launch(members, outs)
        assert name == 'g3::gemm3_tn_kernel grouped x3', name
        runs.append(outs)
    singles = [guarded_output(g.M, g.N + 8, BF16, dev) for g in members]
    for g, o in zip(members, singles):
        name = launch([g], [o])
        assert name == 'g3::gemm3_tn_kernel grouped x1', name
    for g, o0, o1, os_ in zip(members, runs[0], runs[1], singles):
        got = o0[:g.M, :g.N]
        assert torch.isfinite(got.float()).all(), f'member {g.M}x{g.N}: non-finite outputs'
        ref = g.a.double().t() @ g.b.double()
        err = ((got.double() - ref).norm() / ref.norm()).item()
        assert err < 2.0 ** -8, f'member {g.M}x{g.N}: relative error {err:.3e} against float64 (one bf16 rounding is 2^-9 per element)'
        assert torch.equal(as_bits(o0), as_bits(o1)), f'member {g.M}x{g.N}: two launches of the same group differ'
        assert torch.equal(as_bits(o0), as_bits(os_)), f'member {g.M}x{g.N}: the grouped launch differs from the member launched alone'
