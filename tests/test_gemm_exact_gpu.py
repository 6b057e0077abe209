"""Every GEMM route against an EXACT reference, element for element.

Inputs are chosen so that every value a kernel should produce is exactly representable: A and B hold integers in [-2, 2] (bf16), K <= 15424, so
every partial sum is an integer below 2^24 and fp32 accumulation is exact in ANY order (split-K included); bias entries are integers in [-8, 8];
"rotary" table entries are k / 16, so (acc + bias) * tab is one exact fp32 product; residual and aux entries are small integers, so bf16(v) + residual
and bf16(v) * aux are exact in fp32 before the final round-to-nearest-even.  The reference is a float64 torch.matmul of the same integers followed by
the epilogue in the order include/mreserve_hip.h gives, rounded to bf16 where the header says bf16(v); the comparison is torch.equal on the bits.
The GELU epilogue (and its c2 = gelu' copy) is not exact: there B is scaled by 1 / 8, every pre-activation is an exact multiple of 1 / 8, every element
must lie within ONE bf16 ulp of the float64 reference, and all elements with the same pre-activation must carry the same bits.

Operands and outputs are leading views of larger allocations (tests/util.py): leading dimensions wider than the extents and different from each
other, zeros up to the next multiple of 8 elements (the header's contract), NaN in everything past that -- the rest of each row and 256 whole rows
behind each operand -- and a sentinel in every cell of the output allocations that the launch must leave alone (columns N .. ldc - 1, rows past M,
the rows between the groups of a row map; the same for c2 and the column-sum rows).

Every forced route asserts the kernel instance it means to test (mr_last_gemm_kernel under "gemm_trace"); a forced option that cannot take a problem
is a skip with the reason, never a silent run elsewhere.  The default route is exercised without pinning its kernel names.  expected_kernel() below
mirrors csrc/gemm_route.cpp for the forced options only."""
import collections
import contextlib

import pytest
import torch

from util import (as_bits, exact_report, guarded_output, one_ulp_report, padded_operand, padded_vector, same_input_same_bits_report)

pytestmark = pytest.mark.gpu

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
ROT_ROWS = 241
ROW_MAP = (240, 241, 1)

# name -> (kind, options).  The eight forced configurations of tests/test_gemm3_gpu.py, the four forced widths of the one-barrier kernel, the
# small-tile kernel (reached through shapes nothing else takes), the library's own choice.
ROUTES = collections.OrderedDict([
    ('g3-256-ph1', ('g3', dict(gemm3=256, gemm3_phases=1, gemm4=0, gemm5=0))),
    ('g3-192-ph1', ('g3', dict(gemm3=192, gemm3_phases=1, gemm4=0, gemm5=0))),
    ('g3-256-ph2', ('g3', dict(gemm3=256, gemm3_phases=2, gemm4=0, gemm5=0))),
    ('g3-192-ph2', ('g3', dict(gemm3=192, gemm3_phases=2, gemm4=0, gemm5=0))),
    ('g4-256', ('g4', dict(gemm3=256, gemm3_phases=0, gemm4=1, gemm5=0))),
    ('g4-192', ('g4', dict(gemm3=192, gemm3_phases=0, gemm4=1, gemm5=0))),
    ('g5-256x128', ('g5', dict(gemm3=256, gemm3_phases=1, gemm4=0, gemm5=1))),
    ('g5-128x128', ('g5', dict(gemm3=256, gemm3_phases=1, gemm4=0, gemm5=3))),
    ('t96', ('tile', dict(gemm3=0, gemm5=0, gemm_tile_n=96))),
    ('t128', ('tile', dict(gemm3=0, gemm5=0, gemm_tile_n=128))),
    ('t192', ('tile', dict(gemm3=0, gemm5=0, gemm_tile_n=192))),
    ('t256', ('tile', dict(gemm3=0, gemm5=0, gemm_tile_n=256))),
    ('small', ('small', dict(gemm3=0, gemm5=0))),
    ('default', ('default', dict())),
])

EPI_MODE = {'plain': 5, 'bias': 0, 'rowmap': 0, 'rot768': 1, 'rot832': 1, 'gelu': 2, 'c2': 2, 'res': 3, 'res_inplace': 3, 'aux': 4, 'aux_cs': 4,
            'f32bias': 0}
CENSUS = collections.Counter()          # kernel instance -> number of cases that reached it (printed by the last test of this file)


@contextlib.contextmanager
def options(**kw):
    """Sets the given options and "gemm_trace"; puts every one of them back to the value it had, also when the body raises."""
    from merlot_reserve_amd import ops
    names = set(kw) | {'gemm_trace'}
    prev = {k: ops.get_option(k) for k in names}
    try:
        for k, v in kw.items():
            ops.set_option(k, v)
        ops.set_option('gemm_trace', 1)
        yield
    finally:
        for k, v in prev.items():
            ops.set_option(k, v)


def last_kernel():
    from merlot_reserve_amd import _lib
    name = _lib.load().mr_last_gemm_kernel().decode()
    CENSUS[name] += 1
    return name


# ---- what the router does with a forced option (csrc/gemm_route.cpp): the kernel instance, or the reason the option cannot take the problem
def nt_fusable(M, N, K, ta, tb, epi):
    return (not ta) and tb and K % 64 == 0 and epi not in ('f32bias', 'c2')     # c2 exactly with GELU; bf16 output


def gemm256_eligible(M, N, K, ta, tb):
    return M >= 512 and N >= 96 and (ta or K % 64 == 0) and (not tb or K % 64 == 0)


def expected_kernel(route, M, N, K, ta, tb, epi, ws=False):
    """-> (kernel name | None for "not pinned", skip reason | None)"""
    kind, opt = ROUTES[route]
    mode = EPI_MODE[epi]
    big = gemm256_eligible(M, N, K, ta, tb)
    if epi == 'aux_cs' and not big:
        return None, 'column sums need a problem the 256-row kernels take (mr_gemm_colsum_supported)'
    if kind == 'default':
        return None, None
    if kind in ('g3', 'g4', 'g5') and not nt_fusable(M, N, K, ta, tb, epi):
        return None, 'the fused NT kernels take A [M, K], B [N, K], K % 64 == 0, bf16 output, c2 only with GELU'
    if kind == 'g5':
        if K < 128:
            return None, 'gemm5 needs K >= 128'
        return ('g5::gemm5_kernel<%d,4,128,8>' if opt['gemm5'] == 3 else 'g5::gemm5_kernel<%d,4>') % mode, None
    if kind == 'g3':
        m3 = 0 if mode == 5 else mode
        if m3 == 4 and opt['gemm3'] == 256 and opt['gemm3_phases'] == 1:
            return None, 'gemm3_kernel<256,4,1> is not built: the router runs <256,4,2>, which the two-phase case covers'
        return 'g3::gemm3_kernel<%d,%d,%d>' % (opt['gemm3'], m3, opt['gemm3_phases']), None
    if kind == 'g4':
        if mode not in (0, 3, 5) or (opt['gemm3'] == 256 and mode == 0):
            return None, 'gemm4 has the plain, residual and (192-wide only) bias epilogues'
        return 'g4::gemm4_kernel<%d,%d>' % (opt['gemm3'], mode), None
    if kind == 'tile':
        if not big:
            return None, 'the one-barrier kernel takes M >= 512, N >= 96, K-contiguous operands with K % 64 == 0'
        bn = opt['gemm_tile_n']
        if bn > 128 and N < bn:
            return None, f'N < {bn}: the router chooses the width itself'
        if mode == 1 and bn == 96:
            return None, 'the "rotary" epilogue runs on 128-wide tiles when 96 is asked for (covered by t128)'
        if epi == 'aux_cs' and bn == 256 and N >= 192:
            return None, 'column sums run on 192-wide tiles when 256 is asked for (covered by t192)'
        return 'g256::gemm256_kernel<%d,%d,%d>%s' % (bn, ta, tb, ' + splitk_reduce' if ws else ''), None
    if kind == 'small':
        if big:
            return None, 'the one-barrier kernel takes this problem before the small-tile kernel'
        return 'gemm_bf16_kernel<%d,%d>%s' % (ta, tb, ' + splitk_reduce' if ws else ''), None
    raise AssertionError(kind)


# ---- problems: operands, float64 accumulators and per-epilogue references, built once per shape and reused over the routes
def ceil8(n):
    return (n + 7) // 8 * 8


class Problem:
    def __init__(self, dev, M, N, K, ta, tb):
        self.dev, self.M, self.N, self.K, self.ta, self.tb = dev, M, N, K, ta, tb
        assert K <= 15424
        self.gen = torch.Generator(device=dev).manual_seed(1000003 * M + 1009 * N + K + 2 * ta + tb)
        A = self.ints(-2, 2, (M, K)).to(BF16)
        B = self.ints(-2, 2, (K, N)).to(BF16)
        self.acc = A.double() @ B.double()                       # integers, |.| <= 4 K < 2^24: exact in fp32 in any order
        a_st = A.t().contiguous() if ta else A
        b_st = B.t().contiguous() if tb else B
        self.a = padded_operand(a_st, ceil8(a_st.shape[1]) + (24 if ta else 8))
        self.b = padded_operand(b_st, ceil8(b_st.shape[1]) + (24 if tb else 8))
        self.b_eighth = padded_operand((b_st.float() / 8).to(BF16), self.b.stride(0))     # exact: +-1/4, +-1/8, 0
        self.bias_v = self.ints(-8, 8, (N,)).to(BF16)
        self.bias = padded_vector(self.bias_v)
        self._lazy = {}

    def ints(self, lo, hi, shape):
        return torch.randint(lo, hi + 1, shape, device=self.dev, generator=self.gen)

    def lazy(self, name):
        if name not in self._lazy:
            M, N = self.M, self.N
            if name == 'tab':
                self._lazy[name] = padded_vector(self.ints(-16, 16, (ROT_ROWS, 32)).float() / 16)
            elif name == 'res':
                self._lazy[name] = padded_operand(self.ints(-8, 8, (M, N)).to(BF16), N + 16)
            elif name == 'aux':
                self._lazy[name] = padded_operand(self.ints(-3, 3, (M, N)).to(BF16), N + 24)
            else:
                assert name.startswith('ref:')
                self._lazy[name] = self.reference(name[4:])
        return self._lazy[name]

    @staticmethod
    def exact_bf16(v64):
        v32 = v64.to(F32)
        assert torch.equal(v32.double(), v64), 'the reference is not exactly representable in fp32: the case is not an exact one'
        return v32.to(BF16)

    def reference(self, epi):
        """{'out': expected stored values [M, N], optionally 'c2', 'key' (pre-activation in eighths), 'cs' (column-sum partial rows)}"""
        acc, bias = self.acc, self.bias_v.double()
        if epi == 'plain':
            return {'out': self.exact_bf16(acc)}
        if epi in ('bias', 'rowmap'):
            return {'out': self.exact_bf16(acc + bias)}
        if epi == 'f32bias':
            v = acc + bias
            assert torch.equal(v.to(F32).double(), v)
            return {'out': v.to(F32)}
        if epi == 'c2':                                           # c2 = bf16(v) without an activation
            o = self.exact_bf16(acc + bias)
            return {'out': o, 'c2': o}
        if epi.startswith('rot'):
            rot_cols = int(epi[3:])
            tab = self.lazy('tab').double()
            m = torch.arange(self.M, device=self.dev) % ROT_ROWS
            n = torch.arange(self.N, device=self.dev)
            scale = tab[m][:, n & 31]                             # [M, N]: tab[m % rot_rows, n & 63] where (n & 63) < 32
            on = ((n < rot_cols) & ((n & 63) < 32)).unsqueeze(0)
            v = acc + bias
            return {'out': self.exact_bf16(torch.where(on, v * scale, v))}
        if epi == 'gelu':
            pre = acc / 8 + bias                                  # exact multiples of 1 / 8
            s = torch.sigmoid(1.702 * pre)
            return {'out': (pre * s).to(BF16), 'c2': (s + 1.702 * pre * s * (1 - s)).to(BF16), 'key': (pre * 8).round().to(torch.int64)}
        if epi in ('res', 'res_inplace'):
            return {'out': self.exact_bf16(self.exact_bf16(acc).double() + self.lazy('res').double())}
        if epi in ('aux', 'aux_cs'):
            o = self.exact_bf16(self.exact_bf16(acc).double() * self.lazy('aux').double())
            nrows = 4 * ((self.M + 255) // 256)
            band = torch.zeros(nrows * 64, self.N, dtype=F64, device=self.dev)
            band[:self.M] = o.double()
            cs = band.reshape(nrows, 64, self.N).sum(1)           # partial row 4 * (m / 256) + (m % 256) / 64: integers < 2^24
            assert torch.equal(cs.to(F32).double(), cs)
            return {'out': o, 'cs': cs.to(F32)}
        raise AssertionError(epi)


_PROBLEMS = collections.OrderedDict()


def problem(dev, M, N, K, ta, tb):
    key = (M, N, K, ta, tb)
    if key not in _PROBLEMS:
        while len(_PROBLEMS) >= 2:                                # cases come grouped by shape: two live problems bound the memory
            _PROBLEMS.popitem(last=False)
        _PROBLEMS[key] = Problem(dev, M, N, K, ta, tb)
    _PROBLEMS.move_to_end(key)
    return _PROBLEMS[key]


def run_single(dev, route, M, N, K, ta, tb, epi, ws=None):
    """One mr_gemm launch under `route`; every output allocation checked cell by cell.  Returns (kernel name, the stored [M, N] output)."""
    from merlot_reserve_amd import _lib, ops
    P = problem(dev, M, N, K, ta, tb)
    ref = P.lazy('ref:' + epi)
    want, why = expected_kernel(route, M, N, K, ta, tb, epi, ws is not None)
    assert why is None, why
    ldc = N + 8
    kw = dict(transA=ta, transB=tb, ws=ws)
    rows, row_index = M, None
    if epi not in ('plain', 'res', 'res_inplace', 'aux', 'aux_cs'):
        kw['bias'] = P.bias
    if epi == 'rowmap':
        m = torch.arange(M, device=dev)
        row_index = (m // ROW_MAP[0]) * ROW_MAP[1] + ROW_MAP[2] + m % ROW_MAP[0]
        rows = int(row_index[-1]) + 1
        kw['row_map'] = ROW_MAP
    out = guarded_output(rows, ldc, F32 if epi == 'f32bias' else BF16, dev)
    c2 = cs = None
    if epi.startswith('rot'):
        kw.update(rot_tab=P.lazy('tab'), rot_cols=int(epi[3:]))
    if epi in ('gelu', 'c2'):
        c2 = guarded_output(rows, ldc, BF16, dev)
        kw['c2'] = c2[:rows, :N]
        if epi == 'gelu':
            kw['act'] = ops.ACT_GELU
    if epi == 'res':
        kw['residual'] = P.lazy('res')
    if epi == 'res_inplace':
        out[:M, :N] = P.lazy('res')
        kw['residual'] = out[:M, :N]
    if epi in ('aux', 'aux_cs'):
        kw['aux'] = P.lazy('aux')
    if epi == 'aux_cs':
        nrows = _lib.load().mr_gemm_colsum_rows(M)
        assert nrows == ref['cs'].shape[0]
        cs = guarded_output(nrows, N + 12, F32, dev)
        kw['colsum'] = cs[:nrows, :N]
    b = P.b_eighth if epi == 'gelu' else P.b
    with options(**ROUTES[route][1]):
        ops.gemm(P.a, b, out[:rows, :N], **kw)
        name = last_kernel()
    tag = f'{M}x{N}x{K} ta={int(ta)} tb={int(tb)} {epi} on {route} [{name}]'
    if want is not None:
        assert name == want, f'{tag}: meant to test {want}'
    if epi == 'gelu':
        for what, alloc in (('out', out), ('c2', c2)):
            got = alloc[:M, :N].contiguous()
            assert one_ulp_report(got, ref[what]) == '', f'{tag}: {what}: ' + one_ulp_report(got, ref[what])
            rep = same_input_same_bits_report(ref['key'], got)
            assert rep == '', f'{tag}: {what}: {rep}'
            rep = exact_report(alloc, got)                        # the stored region as it is; every guard cell must hold the sentinel
            assert rep == '', f'{tag}: {what}: {rep}'
    else:
        rep = exact_report(out, ref['out'], row_index)
        assert rep == '', f'{tag}: {rep}'
        if c2 is not None:
            rep = exact_report(c2, ref['c2'], row_index)
            assert rep == '', f'{tag}: c2: {rep}'
    if cs is not None:
        nrows = ref['cs'].shape[0]
        got = cs[:nrows, :N]
        assert not torch.isnan(got).any(), f'{tag}: a column-sum partial row was not written'
        assert torch.equal(got, ref['cs']), f'{tag}: column-sum partial rows differ from the per-(256-row tile, 64-row band) layout of the header'
        assert torch.equal(got.double().sum(0), out[:M, :N].double().sum(0)), f'{tag}: total of the partial rows != column sum of the stored output'
        filled = cs.clone()
        filled[:nrows, :N] = ref['cs']
        rep = exact_report(filled, ref['cs'])
        assert rep == '', f'{tag}: column sums: {rep}'
    return name, out[:M, :N]


def cases(shapes, epis, routes):
    """pytest params, grouped by shape (the reference is computed once per shape); a route that cannot take a case is a skip with the reason."""
    out = []
    for (M, N, K, ta, tb) in shapes:
        for epi in epis:
            for route in routes:
                _, why = expected_kernel(route, M, N, K, ta, tb, epi)
                marks = [pytest.mark.skip(reason=why)] if why else []
                out.append(pytest.param(M, N, K, ta, tb, epi, route, marks=marks,
                                        id=f'{M}x{N}x{K}-{"T" if ta else "N"}{"T" if tb else "N"}-{epi}-{route}'))
    return out


@pytest.fixture
def dev():
    return torch.device('cuda:0')


BIG_ROUTES = [r for r in ROUTES if r != 'small']
TILE_ROUTES = ['t96', 't128', 't192', 't256', 'default']

# NT problems: M ragged against 256 / 128 / 64 / 16, one row tile's worth up to the XCD-partitioned case (>= 2 rounds of tiles); N ragged against
# every tile width (a multiple of 8), smaller than one tile, and the model's 768 / 2304 / 3072; K = one k-tile, two, an odd count, 768, 3072
NT_SHAPES = [
    (1446, 768, 256, False, True),
    (2308, 1000, 192, False, True),
    (4616, 200, 64, False, True),
    (5952, 264, 128, False, True),
    (1446, 1544, 768, False, True),
    (4616, 768, 3072, False, True),
    (9000, 3072, 192, False, True),          # 432 tiles of 256 x 256: several per persistent workgroup
    (15424, 2304, 768, False, True),         # 549 tiles: the XCD partition
]
# the other three layouts (the one-barrier kernel has all four); ragged K where the layout allows it (A stored [K, M])
LAYOUT_SHAPES = [
    (2308, 1000, 192, False, False),
    (1446, 768, 768, False, False),
    (1000, 264, 200, True, False),
    (9000, 1544, 128, True, False),
    (640, 264, 704, True, True),
    (2308, 200, 1500, True, False),
]
# what only the small-tile kernel takes: M < 512, N < 96, or a ragged K on a K-contiguous operand
SMALL_SHAPES = [
    (300, 200, 1500, False, True),
    (100, 56, 200, False, False),
    (448, 264, 192, True, False),
    (200, 1000, 200, True, True),
    (5000, 64, 128, False, True),
]
# epilogues: N = 1000 is ragged against 96 / 128 / 192 / 256; M = 1450 is not a multiple of rot_rows = 241 nor of 16
EPI_SHAPE_NT = (1450, 1000, 256, False, True)
EPI_SHAPE_NN = (1450, 1000, 256, False, False)
EPI_SHAPE_SMALL = (300, 1000, 256, False, True)
# rot_cols = 768 ends on a tile boundary of every width (96, 128, 192, 256); 832 = 13 * 64 ends inside a tile of every width
EPILOGUES = ['bias', 'rot768', 'rot832', 'gelu', 'c2', 'res', 'res_inplace', 'aux', 'aux_cs', 'f32bias']


@pytest.mark.parametrize('M,N,K,ta,tb,epi,route', cases(NT_SHAPES, ['plain'], BIG_ROUTES) + cases(LAYOUT_SHAPES, ['plain'], TILE_ROUTES) +
                         cases(SMALL_SHAPES, ['plain'], ['small', 'default']))
def test_plain_product(dev, M, N, K, ta, tb, epi, route):
    run_single(dev, route, M, N, K, ta, tb, epi)


@pytest.mark.parametrize('M,N,K,ta,tb,epi,route', cases([EPI_SHAPE_NT], EPILOGUES, BIG_ROUTES) + cases([EPI_SHAPE_NN], EPILOGUES, TILE_ROUTES) +
                         cases([EPI_SHAPE_SMALL], EPILOGUES + ['rowmap'], ['small', 'default']))
def test_epilogues(dev, M, N, K, ta, tb, epi, route):
    run_single(dev, route, M, N, K, ta, tb, epi)


# several tiles per persistent workgroup (456 / 252-324 / 432 tiles): the row map [CLS | 240 patches] with a bias, the inexact GELU pair and the
# column sums, where a tile's stores are in flight under the next tile's k-loop
@pytest.mark.parametrize('M,N,K,ta,tb,epi,route', cases([(9120, 3072, 128, False, True)], ['rowmap'], BIG_ROUTES) +
                         cases([(9000, 1544, 192, False, True)], ['aux_cs', 'gelu'], BIG_ROUTES) +
                         cases([(9120, 3072, 128, False, False)], ['rowmap'], TILE_ROUTES))
def test_epilogues_over_several_tiles_per_workgroup(dev, M, N, K, ta, tb, epi, route):
    run_single(dev, route, M, N, K, ta, tb, epi)


@pytest.mark.parametrize('route', ['t96', 't128', 't192', 't256', 'small', 'default'])
@pytest.mark.parametrize('M,N,K', [(768, 3072, 1500), (768, 768, 5000), (448, 264, 1500)])
def test_split_k_equals_the_unsplit_product(dev, M, N, K, route):
    """Weight-gradient shapes (A stored [K, M], ragged K) with a workspace: split along K and summed by the reduction kernel.  Integers: the split
    result equals the reference and the same problem without a workspace, bit for bit."""
    _, why = expected_kernel(route, M, N, K, True, False, 'plain', True)
    if why:
        pytest.skip(why)
    ws = torch.full((32 << 20,), float('nan'), device=dev)                   # 128 MiB of fp32 partials, NaN: every partial read must have been written
    name, split = run_single(dev, route, M, N, K, True, False, 'plain', ws=ws)
    if route != 'default':
        assert 'splitk_reduce' in name
    _, whole = run_single(dev, route, M, N, K, True, False, 'plain')
    assert torch.equal(as_bits(split), as_bits(whole))


# ---- grouped launches
def grouped_members(dev, shapes, K, ta, tb, f32=False, bias=False):
    """[(Problem, output allocation, gemm args)] for mr_gemm_grouped; the problems live outside the two-entry cache for the length of a test."""
    from merlot_reserve_amd import ops
    members = []
    for M, N in shapes:
        P = Problem(dev, M, N, K, ta, tb)
        out = guarded_output(M, N + 8, F32 if f32 else BF16, dev)
        g = ops.gemm_args(P.a, P.b, out[:M, :N], transA=ta, transB=tb, bias=P.bias if bias else None)
        members.append((P, out, g))
    return members


def check_members(members, bias, tag):
    for P, out, _ in members:
        v = P.acc + (P.bias_v.double() if bias else 0)
        ref = v.to(F32) if out.dtype == F32 else Problem.exact_bf16(v)
        rep = exact_report(out, ref)
        assert rep == '', f'{tag}: member {P.M}x{P.N}x{P.K}: {rep}'


@pytest.mark.parametrize('K,forced', [(4616, True), (5000, True), (15424, True), (4616, False)])
def test_grouped_tn_weight_gradients(dev, K, forced):
    """The grouped TN weight-gradient kernel with members whose M and N are not multiples of its 256 x 256 tile, padded lda / ldb / ldc, a K
    that is not a multiple of 64 among them: forced, and by default (with a 3072 x 3072 member the tiles fill the chip, so the router takes it)."""
    from merlot_reserve_amd import ops
    shapes = [(776, 1000), (3072, 200), (264, 776)] + ([] if forced else [(3072, 3072)])
    members = grouped_members(dev, shapes, K, True, False)
    with options(**(dict(gemm3=256) if forced else {})):
        ops.gemm_grouped([g for _, _, g in members])
        name = last_kernel()
    if forced:
        assert name == f'g3::gemm3_tn_kernel grouped x{len(shapes)}', name
    check_members(members, False, f'TN group K={K} [{name}]')


@pytest.mark.parametrize('group_tile', [0, 128, 256])
def test_grouped_one_barrier(dev, group_tile):
    """Four bias-only problems of one layout in ONE launch of the one-barrier kernel, at both tile widths of the shared launch."""
    from merlot_reserve_amd import ops
    shapes = [(1000, 512), (776, 1024), (520, 256), (2048, 768)]
    members = grouped_members(dev, shapes, 1500, True, False, bias=True)
    with options(gemm_group_tile_n=group_tile):
        ops.gemm_grouped([g for _, _, g in members])
        name = last_kernel()
    assert name.startswith('g256::gemm256_kernel<') and name.endswith(',1,0> grouped x4'), name
    if group_tile:
        assert name == f'g256::gemm256_kernel<{group_tile},1,0> grouped x4', name
    check_members(members, True, f'one-barrier group [{name}]')


def test_grouped_more_than_four(dev):
    """Six problems: the one-barrier kernel groups four per launch, so the list is cut into a launch of four and one of two."""
    from merlot_reserve_amd import ops
    shapes = [(1000, 512), (776, 1024), (520, 256), (2048, 768), (640, 384), (1448, 128)]
    members = grouped_members(dev, shapes, 704, False, True, bias=True)
    with options():
        ops.gemm_grouped([g for _, _, g in members])
        name = last_kernel()
    assert name.startswith('g256::gemm256_kernel<') and name.endswith(',0,1> grouped x2'), name
    check_members(members, True, f'six problems [{name}]')


@pytest.mark.parametrize('f32', [True, False], ids=['f32-logits', 'bf16'])
def test_grouped_small_tile(dev, f32):
    """The small-tile grouped kernel with a bias: the contrastive-logits shape (a few hundred queries against V keys, fp32 logits of differing V in
    rows padded past V), and bf16 outputs."""
    from merlot_reserve_amd import ops
    shapes = [(300, 600), (452, 900), (100, 204)] if f32 else [(300, 600), (452, 904), (100, 200)]
    members = grouped_members(dev, shapes, 768, False, True, f32=f32, bias=True)
    with options():
        ops.gemm_grouped([g for _, _, g in members])
        name = last_kernel()
    assert name == 'gemm_bf16_grouped_kernel<0,1> x3', name
    check_members(members, True, f'small-tile group [{name}]')


def test_grouped_mixed_list_falls_back_to_single_launches(dev):
    """Layouts that differ: no shared launch takes the list, every member runs as its own mr_gemm -- with the same exact results."""
    from merlot_reserve_amd import ops
    big = grouped_members(dev, [(1446, 768)], 256, False, True, bias=True)
    wgrad = grouped_members(dev, [(776, 264)], 1500, True, False)
    tiny = grouped_members(dev, [(100, 56)], 200, False, False, bias=True)
    with options():
        ops.gemm_grouped([m[2] for m in big + wgrad + tiny])
        name = last_kernel()
    assert 'grouped' not in name, name
    check_members(big, True, 'mixed list')
    check_members(wgrad, False, 'mixed list')
    check_members(tiny, True, 'mixed list')


def test_zz_census_of_kernel_instances(dev):
    """Prints, per kernel instance, how many cases of this file reached it (run the file with -s), and checks that every family was reached."""
    _PROBLEMS.clear()
    if not CENSUS:
        pytest.skip('the cases of this file did not run in this process')
    for name in sorted(CENSUS):
        print(f'CENSUS {CENSUS[name]:4d}  {name}')
    if sum(CENSUS.values()) < 300:
        return                                                    # a selection of cases (-k): nothing to conclude
    for family in ('g3::gemm3_kernel<', 'g4::gemm4_kernel<', 'g5::gemm5_kernel<', 'g256::gemm256_kernel<', 'gemm_bf16_kernel<',
                   'g3::gemm3_tn_kernel', 'gemm_bf16_grouped_kernel<', 'splitk_reduce', 'grouped x'):
        assert any(family in n for n in CENSUS), f'no case reached {family}'
