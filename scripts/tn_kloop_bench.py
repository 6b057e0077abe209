"""The grouped weight-gradient kernel (g3::gemm3_tn_kernel) alone, on the three group shapes of the step, next to the NT ping-pong kernel at 8192^3.

    python scripts/tn_kloop_bench.py time          us per launch over cold operands (rotating operand sets), TF/s and TF/s per occupied CU
    python scripts/tn_kloop_bench.py once tn-base  a few launches of one shape and nothing else: the process to put under a counter pass
    python scripts/tn_kloop_bench.py once nt       (rocprofv3 --pmc ... --kernel-trace -- python scripts/tn_kloop_bench.py once tn-base)

A/B of two builds: run it under MR_LIB=<other library> and under the shipped one, alternating, in one job on one box."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from merlot_reserve_amd import _lib, ops      # noqa: E402

dev = torch.device('cuda:0')
lib = _lib.load()
BF16 = torch.bfloat16


def layer_shapes(H, layers):
    return [(4 * H, H), (H, 4 * H), (H, H), (H, 3 * H)] * layers


# name -> (hidden size, layers per launch, tokens, operand sets)
TN_GROUPS = {'tn-base': (768, 2, 15424, 4), 'tn-audio': (768, 2, 5952, 8), 'tn-large': (1024, 4, 15424, 2)}


def tn_sets(name):
    H, layers, K, nsets = TN_GROUPS[name]
    shapes = layer_shapes(H, layers)
    sets = []
    for _ in range(nsets):
        xs = [torch.randn(K, m, device=dev).to(BF16) for m, n in shapes]
        dys = [(torch.randn(K, n, device=dev) * 0.05).to(BF16) for m, n in shapes]
        outs = [torch.zeros(m, n, dtype=BF16, device=dev) for m, n in shapes]
        sets.append(([ops.gemm_args(x, dy, o, transA=True) for x, dy, o in zip(xs, dys, outs)], xs, dys, outs))
    tiles = sum(((m + 255) // 256) * ((n + 255) // 256) for m, n in shapes)
    return sets, sum(2.0 * K * m * n for m, n in shapes), tiles


def nt_sets(n=8192, nsets=3):
    sets = []
    for _ in range(nsets):
        a = torch.randn(n, n, device=dev).to(BF16)
        b = (torch.randn(n, n, device=dev) * 0.05).to(BF16)
        sets.append((a, b, torch.zeros(n, n, dtype=BF16, device=dev)))
    return sets, 2.0 * n ** 3, (n // 256) ** 2


def runner(name):
    """-> (launch one pass over the operand sets, launches per pass, FLOP per launch, tiles per launch, kernel name)"""
    if name == 'nt':
        sets, fl, tiles = nt_sets()
        ops.set_option('gemm4', 0)          # the ping-pong NT kernel of gemm3.hip (the TN kernel's sibling), not the one-wave-per-SIMD kernel
        ops.set_option('gemm5', 0)

        def go():
            for a, b, o in sets:
                ops.gemm(a, b, o, transB=True)
    else:
        sets, fl, tiles = tn_sets(name)

        def go():
            for s in sets:
                ops.gemm_grouped(s[0])
    ops.set_option('gemm_trace', 1)
    go()
    kernel = lib.mr_last_gemm_kernel().decode()
    ops.set_option('gemm_trace', 0)
    torch.cuda.synchronize()
    return go, len(sets), fl, tiles, kernel


def time_one(name, reps=11):
    go, n, fl, tiles, kernel = runner(name)
    go()
    go()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        go()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3 / n)
    ts.sort()
    med = ts[len(ts) // 2]
    # a CU is occupied for the rounds it has a tile in: tiles / 256 rounds when the tiles fill whole rounds, else one tile time on `tiles` CUs
    cus = min(tiles, 256)
    print(f'{name:9s} {kernel:44s} tiles {tiles:5d}  median {med:8.1f} us  min {ts[0]:8.1f}  {fl / med / 1e6:7.1f} TF/s  '
          f'{fl / med / 1e6 / cus:6.3f} TF/s per occupied CU ({cus})', flush=True)
    return med


if __name__ == '__main__':
    mode = sys.argv[1] if len(sys.argv) > 1 else 'time'
    if mode == 'time':
        for name in (sys.argv[2:] or ['tn-base', 'tn-audio', 'tn-large', 'nt']):
            time_one(name)
    elif mode == 'once':
        go, n, fl, tiles, kernel = runner(sys.argv[2])
        go()
        torch.cuda.synchronize()
        print(f'{sys.argv[2]}: {2 * n} launches of {kernel}', flush=True)
    else:
        raise SystemExit(__doc__)
