"""Every element of what csrc/layernorm.hip and csrc/rowops.hip write, through the ops wrappers the engine calls, on the MI355X.

Inputs are LEADING VIEWS with padded leading dimensions (+8 / +24 / +40 elements): the padding and 256 rows behind hold NaN, vectors are followed by NaN
(util.padded_operand / padded_vector), so a read past a row or past the last row lands in a result.  Outputs are guarded allocations: every cell a
kernel must not write holds a sentinel that has to survive (util.guarded_output).  The reference is fp64 on the bf16 values of the inputs
(tests/rowops_refs.py).  Integer-valued data are compared by bits (util.exact_report); everything else must lie, element by element and with no
share left out, inside util.bound_report's bound, whose derivation stands in util.py and rowops_refs.py and which
tests/test_rowops_exact_checker.py proves on a plain fp32 evaluation.  Each test prints its worst error / tolerance before it asserts."""
import pytest
import torch

import rowops_refs as RR
from util import (as_bits, bound_margin, bound_report, exact_bf16, exact_report, guarded_output, padded_operand, padded_vector, small_ints,
                  sparse_int_rows)

pytestmark = pytest.mark.gpu

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
NOTHING = {2: torch.empty(0, 1, dtype=BF16), 4: torch.empty(0, 1, dtype=F32)}


def po(vals, pad):
    return padded_operand(vals, (vals.shape[1] + 7) // 8 * 8 + pad)


def vec_out(n, dtype, dev):
    """A guarded 1-D output: (allocation [1 + 8, n + 8], the contiguous view [n] handed to the kernel)."""
    alloc = guarded_output(1, n + 8, dtype, dev)
    return alloc, alloc[0, :n]


def check(alloc, ref_mag, n, what, row_index=None, alt=None):
    ref, mag = ref_mag
    worst, noise = bound_margin(alloc, ref, mag, n, row_index)
    print(f'{what}: worst error / tolerance {worst:.3f} (median noise term / rounding term {noise:.3f})')
    rep = bound_report(alloc, ref, mag, n, row_index, alt)
    assert rep == '', f'{what}: {rep}'


def check_bits(alloc, ref64, what, row_index=None):
    """ref64: the fp64 reference of integer-valued data; it must be exactly representable in the output's type (asserted on the reference)."""
    ref = exact_bf16(ref64) if alloc.dtype == BF16 else ref64.float()
    assert torch.equal(ref.double(), ref64)
    rep = exact_report(alloc, ref, row_index)
    assert rep == '', f'{what}: {rep}'


def untouched(alloc, what):
    rep = exact_report(alloc, NOTHING[alloc.element_size()].to(alloc.device))
    assert rep == '', f'{what}: {rep}'


@pytest.fixture
def ln_impl():
    from merlot_reserve_amd import ops

    def use(v):
        ops.set_option('ln_impl', v)
    yield use
    ops.set_option('ln_impl', 1)


# ------------------------------------------------------------------------------------------------------------------------ LayerNorm
def _layernorm_case(dev, rows, H, pads, defer=False, stats=True):
    from merlot_reserve_amd import ops
    p0, p1 = pads
    what = f'rows {rows}, H {H}'
    xv, gv, bv, dyv = RR.ln_inputs(rows, H, seed=7 * rows + H, device=dev)
    assert bool((dyv != 0).any(1).all()) and float(dyv.double().abs().sum(0).max()) <= 256          # (on the INPUT: dbeta sees every row, exactly)
    x, gamma, beta, dy = po(xv, p0), padded_vector(gv), padded_vector(bv), po(dyv, p1)
    ref = RR.ln_fwd_ref(xv, gv, bv)
    ya = guarded_output(rows, H + p1, BF16, dev)
    if not stats:
        ops.layernorm_fwd(x, gamma, beta, ya[:rows, :H])
        check(ya, ref['y'], H, f'y without saved statistics ({what})')
        return
    (ma, m), (ra, r) = vec_out(rows, F32, dev), vec_out(rows, F32, dev)
    ops.layernorm_fwd(x, gamma, beta, ya[:rows, :H], m, r)
    check(ya, ref['y'], H, f'y ({what})')
    check(ma, ref['mean'], H, f'mean ({what})')
    check(ra, ref['rstd'], H, f'rstd ({what})')
    # backward, on the reference's statistics rounded to fp32 (inputs like any other: the backward is checked on its own)
    m32, r32 = ref['mean'][0][0].float(), ref['rstd'][0][0].float()
    mean, rstd = padded_vector(m32), padded_vector(r32)
    addv = RR.rnd((rows, H), 11, device=dev)
    ws = ops.layernorm_bwd_workspace(H, dev)
    for variant in ('plain', 'add_to_dx', 'dx_add'):
        dxa = guarded_output(rows, H + p0, BF16, dev)
        (dga, dg), (dba, db) = vec_out(H, BF16, dev), vec_out(H, BF16, dev)
        kw = {}
        if variant == 'add_to_dx':
            dxa[:rows, :H] = addv
            kw = dict(add_to_dx=True)
        elif variant == 'dx_add':
            kw = dict(dx_add=po(addv, 40))                                   # a leading dimension of its own
        jobs = [] if defer else None
        ops.layernorm_bwd(dy, x, gamma, mean, rstd, dxa[:rows, :H], dg, db, ws, jobs=jobs, **kw)
        if defer:
            untouched(dga, 'dgamma before the deferred reduction')
            assert len(jobs) == 1
            ops.reduce_partials(jobs)
        rb = RR.ln_bwd_ref(dyv, xv, gv, m32, r32, None if variant == 'plain' else addv)
        check(dxa, rb['dx'], H, f'dx {variant} ({what})')
        check(dga, rb['dgamma'], rows, f'dgamma {variant} ({what})')
        check_bits(dba, rb['dbeta'][0], f'dbeta {variant} ({what}, deferred {defer})')


@pytest.mark.parametrize('impl', [1, 0], ids=['round6', 'round5'])
@pytest.mark.parametrize('H', RR.LN_H)
def test_layernorm_chunk_and_row_edges(dev, H, impl, ln_impl):
    """H: 8 = one lane; 136 = 17 chunks; 512 = exactly 64 chunks; 520 = one lane in the second pass; 1024; 1032 = the first MC = 4; 2048 = all four passes full.
    rows 1, 2, 7, 8, 9: the forward does 2 rows per wave and 8 per workgroup (an odd last row, a second workgroup), the backward kernels 8 / 4 per workgroup."""
    ln_impl(impl)
    for i, rows in enumerate(RR.LN_SMALL_ROWS):
        _layernorm_case(dev, rows, H, (8, 24) if i % 2 == 0 else (24, 8))


@pytest.mark.parametrize('defer', [False, True], ids=['immediate', 'deferred'])
@pytest.mark.parametrize('impl', [1, 0], ids=['round6', 'round5'])
@pytest.mark.parametrize('H', [136, 1032])
def test_layernorm_partial_row_counts(dev, H, impl, defer, ln_impl):
    """ln_impl = 1: 512 / 513 rows leave 64 / 65 partial rows (8 rows per workgroup); ln_impl = 0: 256 / 257 rows do (4 per workgroup): launch_reduce goes
    single-level against two-level.  Deferred: the same partial rows through mr_reduce_partials.  H = 1032 takes the round-5 kernel on either grid."""
    ln_impl(impl)
    for rows in ((512, 513) if impl == 1 else (256, 257)):
        _layernorm_case(dev, rows, H, (24, 8), defer=defer)


@pytest.mark.parametrize('impl', [1, 0], ids=['round6', 'round5'])
def test_layernorm_one_row_past_the_grid_cap(dev, impl, ln_impl):
    """4097 rows: one past 512 workgroups x 8 rows and 1024 x 4, so exactly one wave runs a second iteration, on the row it prefetched."""
    ln_impl(impl)
    _layernorm_case(dev, 4097, 136, (8, 24))


def test_layernorm_forward_without_saved_statistics(dev):
    _layernorm_case(dev, 9, 136, (8, 24), stats=False)


def test_layernorm_rejected_arguments_write_nothing(dev):
    from merlot_reserve_amd import ops
    from merlot_reserve_amd._lib import MreserveHipError
    for H, ld in ((2056, 2056), (12, 16), (136, 140)):          # beyond 64 lanes x 4 chunks; no multiple of 8; a leading dimension that is none
        rows = 9
        x = torch.ones(rows, ld, dtype=BF16, device=dev)[:, :H]
        g = torch.ones(H, dtype=BF16, device=dev)
        st = torch.ones(rows, device=dev)
        ya = guarded_output(rows, 2056 + 8, BF16, dev)
        (dga, dg), (dba, db) = vec_out(H, BF16, dev), vec_out(H, BF16, dev)
        with pytest.raises(MreserveHipError, match='mr_layernorm_fwd'):
            ops.layernorm_fwd(x, g, g, ya[:rows, :H], st, st)
        with pytest.raises(MreserveHipError, match='mr_layernorm_bwd'):
            ops.layernorm_bwd(x, x, g, st, st, ya[:rows, :H], dg, db, ops.layernorm_bwd_workspace(2048, dev))
        torch.cuda.synchronize()
        for a in (ya, dga, dba):
            untouched(a, f'H {H}, ld {ld}')


# ------------------------------------------------------------------------------------------------------------------------ colsum, reduce_partials
@pytest.mark.parametrize('N', [8, 136, 512, 520])
def test_colsum_strip_edges(dev, N):
    """4 rows per strip, at most 128 strips: 1 / 3 / 4 / 5 rows = a partly filled, a full and a second strip; 511 / 512 / 513 rows = just below, at and past the
    cap (the strip loop runs); 1027 rows = a third pass for three rows.  N = 512 fills the 64 lanes of one block, 520 starts a second.  Immediate and deferred."""
    from merlot_reserve_amd import ops
    ws = ops.colsum_workspace(N, dev)
    for i, rows in enumerate((1, 3, 4, 5, 511, 512, 513, 1027)):
        xv = sparse_int_rows(rows, N, seed=rows + N, device=dev)
        x = po(xv, (8, 24)[i % 2])
        ref = xv.double().sum(0, keepdim=True)
        for defer in (False, True):
            oa, out = vec_out(N, BF16, dev)
            jobs = [] if defer else None
            ops.colsum(x, out, ws, jobs=jobs)
            if defer:
                untouched(oa, 'colsum before the deferred reduction')
                ops.reduce_partials(jobs)
            check_bits(oa, ref, f'colsum rows {rows}, N {N}, deferred {defer}')


NPARTS = [1, 31, 32, 33, 127, 128, 129, 512]                 # the 32-group stride and the 4 x 32 unrolled loop, on either side
COLS_SPLIT = [(8, 8), (16, 8), (40, 24), (2 * 136, 136)]     # (40, 24): one 32-column block writes out0 AND out1


def _reduce_job(dev, nparts, ncols, split, seed):
    """A hand-built job on integer-valued fp32 partials [nparts, ncols] with NaN behind them; -> (ReduceJob, verify(), tensors kept alive)."""
    from merlot_reserve_amd import _lib
    pv = sparse_int_rows(nparts, ncols, seed, dtype=F32, device=dev)
    partials = padded_vector(pv)
    a0, out0 = vec_out(split, BF16, dev)
    a1, out1 = vec_out(ncols - split, BF16, dev) if ncols > split else (None, None)
    job = _lib.ReduceJob(partials.data_ptr(), nparts, ncols, split, out0.data_ptr(), None if out1 is None else out1.data_ptr())
    ref = pv.double().sum(0, keepdim=True)

    def verify():
        check_bits(a0, ref[:, :split], f'reduce_partials out0 (nparts {nparts}, ncols {ncols}, split {split})')
        if a1 is not None:
            check_bits(a1, ref[:, split:], f'reduce_partials out1 (nparts {nparts}, ncols {ncols}, split {split})')
    return job, verify, (partials, a0, a1)


@pytest.mark.parametrize('nparts', NPARTS)
def test_reduce_partials_one_job(dev, nparts):
    from merlot_reserve_amd import ops
    for ncols, split in COLS_SPLIT:
        job, verify, keep = _reduce_job(dev, nparts, ncols, split, seed=nparts + ncols)
        ops.reduce_partials([job])
        verify()


@pytest.mark.parametrize('count', [16, 17])
def test_reduce_partials_batches(dev, count):
    """16 jobs fill one launch; at 17 the wrapper issues two.  The jobs walk through every nparts and every (ncols, split)."""
    from merlot_reserve_amd import ops
    made = [_reduce_job(dev, NPARTS[(3 * j) % 8], *COLS_SPLIT[j % 4], seed=100 + j) for j in range(count)]
    jobs = [m[0] for m in made]
    ops.reduce_partials(jobs)
    assert jobs == []
    for m in made:
        m[1]()


# ------------------------------------------------------------------------------------------------------------------------ segment sum
def _segments(n_dst, bounds):
    """indptr / indices for n_dst segments over tables whose first / last row codes are `bounds`.  1: every first and last row; 4: empty, 300 repeats of
    one row, every first and last row, empty; 5: empty, empty, one entry, every first and last row, empty."""
    ends = [c for b in bounds for c in b]
    segs = {1: [ends], 4: [[], [ends[-1]] * 300, ends, []], 5: [[], [], [ends[0]], ends, []]}[n_dst]
    indptr = [0]
    for s in segs:
        indptr.append(indptr[-1] + len(s))
    return segs, torch.tensor(indptr, dtype=torch.int32), torch.tensor([c for s in segs for c in s], dtype=torch.int32)


@pytest.mark.parametrize('ntab', [1, 2, 3])
@pytest.mark.parametrize('H', [8, 520])
def test_segment_sum_exact(dev, H, ntab):
    """Integer tables, so every sum is exact: bits.  1..3 tables, each with a leading dimension of its own; the first and last row of each table; empty
    segments first, last and two in a row; one entry; 300 repeats of one row (entries <= 3: 300 x 3 = 225 x 4 is a bf16 value); bf16 and fp32
    destinations with a padded leading dimension; scale 1 and 0.5; accumulate onto integers (0 in the row of the 300 repeats)."""
    from merlot_reserve_amd import ops
    sizes, pads = [6, 3, 4][:ntab], [8, 24, 40]
    tabs_v = [small_ints((n, H), 3, seed=H + 10 * t, device=dev) for t, n in enumerate(sizes)]
    tabs = [po(v, pads[t]) for t, v in enumerate(tabs_v)]
    cat = torch.cat(tabs_v).double()
    offs = [sum(sizes[:t]) for t in range(ntab)]
    bounds = [(offs[t], offs[t] + sizes[t] - 1) for t in range(ntab)]
    for n_dst in (1, 4, 5):
        segs, indptr, idx = _segments(n_dst, bounds)
        base = torch.stack([cat[torch.tensor(s, dtype=torch.long)].sum(0) if s else torch.zeros(H, dtype=F64, device=dev) for s in segs])
        oldv = small_ints((n_dst, H), 3, seed=n_dst, device=dev).double()
        for r, s in enumerate(segs):
            if len(s) == 300:
                oldv[r] = 0
        for dtype in (BF16, F32):
            for scale in (1.0, 0.5):
                for acc in (False, True):
                    da = guarded_output(n_dst, H + (24 if acc else 8), dtype, dev)
                    if acc:
                        da[:n_dst, :H] = oldv.to(dtype)
                    ops.segment_sum(tabs, indptr.to(dev), idx.to(dev), da[:n_dst, :H], scale=scale, accumulate=acc)
                    check_bits(da, scale * base + (oldv if acc else 0), f'segment_sum H {H}, {ntab} tables, n_dst {n_dst}, {dtype}, scale {scale}, accumulate {acc}')
    # x[r] += table[r % S]: a segment sum of one static entry per row, accumulated onto x
    n, S = 3, 5
    xa = guarded_output(n * S, H + 24, BF16, dev)
    xv = small_ints((n * S, H), 100, seed=4, device=dev)
    xa[:n * S, :H] = xv
    ops.add_rows_periodic(xa[:n * S, :H], tabs[0][:S])
    check_bits(xa, xv.double() + tabs_v[0][:S].double().repeat(n, 1), f'add_rows_periodic H {H}')


# ------------------------------------------------------------------------------------------------------------------------ rows mean
@pytest.mark.parametrize('R', [1, 2, 4, 3, 5])
def test_rows_mean_fwd_bwd(dev, R):
    """R = 1, 2, 4 on integers: the scale is a power of two, every result exact: bits.  R = 3, 5: by the bound (n = R + 2 forward, 3 backward).  G = 1, 4, 5: one
    wave, a full workgroup, a second one.  H = 8 / 520: one lane, a second pass.  The backward adds into the rows the index names and must leave every
    other row of dsrc alone: they hold the sentinel.  No row is named twice (a group owns its rows: the kernel's contract)."""
    from merlot_reserve_amd import ops
    exact = R in (1, 2, 4)
    for H in (8, 520):
        for G in (1, 4, 5):
            n = G * R + 3
            what = f'R {R}, G {G}, H {H}'
            srcv = small_ints((n, H), 3, seed=G + H, device=dev) if exact else RR.rnd((n, H), G + H, 2.0, device=dev)
            rows = RR.disjoint_rows(G, R, n, seed=R + G, device=dev)
            da = guarded_output(G, H, BF16, dev)                                    # dst has no leading dimension: contiguous, guard rows behind
            ops.rows_mean_fwd(po(srcv, 8 if G != 4 else 24), rows, da[:G])
            ref = RR.rows_mean_fwd_ref(srcv, rows)
            check_bits(da, ref[0], f'rows_mean_fwd {what}') if exact else check(da, ref, R + 2, f'rows_mean_fwd {what}')
            dv = small_ints((G, H), 3, seed=9, device=dev) if exact else RR.rnd((G, H), 9, device=dev)
            sa = guarded_output(n, H + (24 if G != 4 else 8), BF16, dev)
            named = rows.long().reshape(-1)
            sa[named, :H] = srcv[named]
            ops.rows_mean_bwd(padded_vector(dv), rows, sa[:n, :H])
            refb = RR.rows_mean_bwd_ref(dv, rows, srcv)
            check_bits(sa, refb[0], f'rows_mean_bwd {what}', named) if exact else check(sa, refb, 3, f'rows_mean_bwd {what}', named)


# ------------------------------------------------------------------------------------------------------------------------ attention pool
@pytest.mark.parametrize('nh', [1, 2, 8, 9, 12, 16])
def test_poolattn_fwd_bwd(dev, nh):
    """8 lanes per head: nh = 8 is exactly one 64-lane pass, nh = 9 puts 8 lanes into a second (c += 64), nh = 16 fills two.  R = 1, 5, 8 (= MAXR); G = 1, 4, 5.
    k and v are column slices of one wider buffer (ldkv = 3 H + padding) whose unnamed rows hold NaN.  Key rows are disjoint between groups -- the kernel's
    contract: the backward STORES dk / dv rows, it does not add -- and every dk / dv row that no group names keeps the sentinel."""
    from merlot_reserve_amd import ops
    H = nh * 64
    for R in (1, 5, 8):
        for G in (1, 4, 5):
            n, what, nt = G * R + 3, f'nh {nh}, R {R}, G {G}', 64 + R
            pad = 8 if G != 4 else 24
            kr = RR.disjoint_rows(G, R, n, seed=nh + R + G, device=dev)
            named = kr.long().reshape(-1)
            qkv = RR.rnd((n, 3 * H), nh + R, device=dev)
            keep = torch.zeros(n, dtype=torch.bool, device=dev)
            keep[named] = True
            qkv[~keep] = float('nan')
            wide = po(qkv, pad)
            k, v = wide[:, H:2 * H], wide[:, 2 * H:]
            qv, dov = RR.rnd((G, H), 1, device=dev), RR.rnd((G, H), 2, device=dev)
            q, dout = padded_vector(qv), padded_vector(dov)
            oa, pa = guarded_output(G, H, BF16, dev), guarded_output(G, nh * R, F32, dev)
            ops.poolattn_fwd(q, k, v, kr, oa[:G], pa[:G].view(G, nh, R), nh)
            ref = RR.poolattn_fwd_ref(qv, qkv[:, H:2 * H], qkv[:, 2 * H:], kr, nh)
            check(oa, ref['out'], nt, f'poolattn out ({what})')
            check(pa, ref['probs'], nt, f'poolattn probs ({what})')
            p32 = ref['probs'][0].reshape(G, nh, R).float()
            dqa = guarded_output(G, H, BF16, dev)
            dka, dva = guarded_output(n, 3 * H + pad, BF16, dev), guarded_output(n, 3 * H + pad, BF16, dev)
            ops.poolattn_bwd(q, k, v, kr, padded_vector(p32), dout, dqa[:G], dka[:n, :H], dva[:n, :H], nh)
            rb = RR.poolattn_bwd_ref(qv, qkv[:, H:2 * H], qkv[:, 2 * H:], kr, p32, dov, nh)
            check(dqa, rb['dq'], nt, f'poolattn dq ({what})')
            check(dka, rb['dk'], nt, f'poolattn dk ({what})', named)
            check(dva, rb['dv'], nt, f'poolattn dv ({what})', named)


def test_poolattn_rejects_nine_keys(dev):
    from merlot_reserve_amd import ops
    from merlot_reserve_amd._lib import MreserveHipError
    G, R, nh, H = 4, 9, 2, 128
    n = G * R
    kv = torch.ones(n, 3 * H, dtype=BF16, device=dev)
    k, v = kv[:, H:2 * H], kv[:, 2 * H:]
    q = torch.ones(G, H, dtype=BF16, device=dev)
    kr = RR.disjoint_rows(G, R, n, 0, device=dev)
    oa, pa, dqa = guarded_output(G, H, BF16, dev), guarded_output(G, nh * R, F32, dev), guarded_output(G, H, BF16, dev)
    dka, dva = guarded_output(n, 3 * H, BF16, dev), guarded_output(n, 3 * H, BF16, dev)
    probs = pa[:G].view(G, nh, R)
    with pytest.raises(MreserveHipError, match='R <= 8'):
        ops.poolattn_fwd(q, k, v, kr, oa[:G], probs, nh)
    with pytest.raises(MreserveHipError, match='R <= 8'):
        ops.poolattn_bwd(q, k, v, kr, torch.ones(G, nh, R, device=dev), q, dqa[:G], dka[:n, :H], dva[:n, :H], nh)
    torch.cuda.synchronize()
    for a in (oa, pa, dqa, dka, dva):
        untouched(a, 'R = 9')


# ------------------------------------------------------------------------------------------------------------------------ unit-norm
@pytest.mark.parametrize('ls', RR.LOG_SCALES)
def test_unit_norm_scale_fwd_bwd(dev, ls):
    """log_scale 1.0, and the bf16 neighbours of ln 100 on either side: below it the temperature gradient flows, above it it is exactly 0 and the temperature
    is the clip's.  rows 1, 4, 5; H 8, 520, 768 (one lane, a second pass, a full pass); the last row of every multi-row case is all zero.  The forward rounds
    x inv to bf16 BEFORE the temperature multiply, as does the reference; within the fp32 noise of a rounding boundary of that intermediate either
    neighbour is admitted (rowops_refs.unit_norm_fwd_ref)."""
    from merlot_reserve_amd import ops
    lsb = padded_vector(torch.tensor([ls], dtype=BF16, device=dev))
    assert float(lsb) == ls
    for H in (8, 520, 768):
        for rows in (1, 4, 5):
            what = f'log_scale {ls}, rows {rows}, H {H}'
            p0, p1 = (8, 24) if rows != 4 else (24, 8)
            xv, dyv = RR.rnd((rows, H), rows + H, 3.0, device=dev), RR.rnd((rows, H), 7, device=dev)
            if rows > 1:
                xv[rows - 1] = 0
            x, dy = po(xv, p0), po(dyv, p1)
            ya, (ia, inv) = guarded_output(rows, H + p1, BF16, dev), vec_out(rows, F32, dev)
            ops.unit_norm_scale_fwd(x, lsb, ya[:rows, :H], inv)
            lo, hi, mag, inv_ref, inv_mag = RR.unit_norm_fwd_ref(xv, ls)
            check(ya, (lo, mag), 1, f'unit_norm y ({what})', alt=hi)
            check(ia, (inv_ref, inv_mag), H, f'unit_norm inv_norm ({what})')
            inv32 = inv_ref[0].float()
            dxa, (da, dls) = guarded_output(rows, H + p0, BF16, dev), vec_out(1, F32, dev)
            (wa, part) = vec_out((rows + 3) // 4, F32, dev)
            dls.fill_(123.0)                                                        # accumulate = False overwrites
            ops.unit_norm_scale_bwd(x, lsb, padded_vector(inv32), dy, dxa[:rows, :H], dls, part)
            rb = RR.unit_norm_bwd_ref(xv, ls, inv32, dyv)
            check(dxa, rb['dx'], H, f'unit_norm dx ({what})')
            check(da, rb['dls'], rows * H, f'unit_norm dlog_scale ({what})')
            if ls > RR.LN100_F32:
                assert float(rb['dls'][0]) == 0.0 and float(dls) == 0.0
            first = dls.clone()
            ops.unit_norm_scale_bwd(x, lsb, padded_vector(inv32), dy, dxa[:rows, :H], dls, part, accumulate=True)
            assert float(dls) == 2 * float(first), what                             # fixed-order sums: the second call adds the same bits
            wbits = as_bits(wa)
            wbits[0, :(rows + 3) // 4] = wbits[1, 0]
            untouched(wa, 'the partials workspace beyond (rows + 3) // 4 floats')


# ------------------------------------------------------------------------------------------------------------------------ fill / sum / pad / add
@pytest.mark.parametrize('H', [8, 520])
def test_fill_rows_exact(dev, H):
    from merlot_reserve_amd import ops
    ngroups, stride = 5, 7
    vecv = RR.rnd((H,), H, device=dev)
    for off in (0, stride - 1):                                                     # the first and the last row of a group
        for pad in (8, 24):
            da = guarded_output(ngroups * stride, H + pad, BF16, dev)
            ops.fill_rows(padded_vector(vecv), da[:ngroups * stride, :H], ngroups, stride, off)
            idx = torch.arange(ngroups, device=dev) * stride + off
            check_bits(da, vecv.double()[None].repeat(ngroups, 1), f'fill_rows H {H}, off {off}', idx)


@pytest.mark.parametrize('H', [8, 200, 72])
def test_sum_rows_strided_exact(dev, H):
    """One thread per column in 16 row groups: 1 / 15 / 16 / 17 / 70 groups = one, one short of all, all, a second round, a fifth.  H = 200 and 72 are no multiple of 64."""
    from merlot_reserve_amd import ops
    stride = 3
    for i, ngroups in enumerate((1, 15, 16, 17, 70)):
        off = i % stride
        xv = small_ints((ngroups * stride, H), 3, seed=H + ngroups, device=dev)
        oa, out = vec_out(H, BF16, dev)
        ops.sum_rows_strided(po(xv, (8, 24)[i % 2]), ngroups, stride, off, out)
        check_bits(oa, xv.double()[off::stride].sum(0, keepdim=True), f'sum_rows_strided H {H}, {ngroups} groups')


@pytest.mark.parametrize('cols_in,cols_out', [(1, 8), (130, 136), (136, 144), (136, 136)])
def test_pad_cols_exact(dev, cols_in, cols_out):
    from merlot_reserve_amd import ops
    rows = 9
    sv = RR.rnd((rows, cols_in), cols_in, device=dev)
    da = guarded_output(rows, cols_out, BF16, dev)
    ops.pad_cols(padded_vector(sv), da[:rows])
    check_bits(da, torch.cat([sv.double(), torch.zeros(rows, cols_out - cols_in, dtype=F64, device=dev)], 1), f'pad_cols {cols_in} -> {cols_out}')


@pytest.mark.parametrize('rows,cols', [(1, 8), (2049, 4096)])
def test_add_exact(dev, rows, cols):
    """n = 8: one thread.  The launch caps its grid at 4096 blocks of 256 threads x 8 elements = 8,388,608: 2049 x 4096 elements make the grid-stride loop iterate
    for the last 4096.  Out of place and in place; bf16 + bf16 rounds once (integers here: exact)."""
    from merlot_reserve_amd import ops
    av, bv = small_ints((rows, cols), 100, seed=1, device=dev), small_ints((rows, cols), 100, seed=2, device=dev)
    ref = av.double() + bv.double()
    ya = guarded_output(rows, cols, BF16, dev)
    ops.add_(padded_vector(av), padded_vector(bv), ya[:rows])
    check_bits(ya, ref, f'add_ out of place, n {rows * cols}')
    ya = guarded_output(rows, cols, BF16, dev)
    ya[:rows] = av
    ops.add_(ya[:rows], padded_vector(bv))
    check_bits(ya, ref, f'add_ in place, n {rows * cols}')
