"""Where a k-tile of g3::gemm3_tn_kernel spends its cycles: the -DMR_TN_STAMPS build of csrc/gemm3.hip (in-kernel s_memtime stamps, summed per section
in scalar registers; the launcher prints them) run on the base weight-gradient group.

    python scripts/tn_kloop_stamps.py build [-DNAME=VALUE ...]   compiles gemm3.hip with -DMR_TN_STAMPS into merlot_reserve_amd/variants/libmreserve_tn_stamps.so
                                                                 (the other objects come from the regular build under merlot_reserve_amd/build/)
    python scripts/tn_kloop_stamps.py run [LIB] [GROUP]          runs scripts/tn_kloop_bench.py once GROUP (default tn-base) in a child under MR_LIB=LIB,
                                                                 prints cycles per k-tile and section for both wave groups

The stamps fence the sections (each carries an lgkmcnt(0)), so the build is slower than the real kernel: read the shares, not the total."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = os.path.join(ROOT, 'merlot_reserve_amd')
STAMP_LIB = os.path.join(PKG, 'variants', 'libmreserve_tn_stamps.so')
SEGMENTS = ['memory section 0', 'barrier 1 wait', 'MFMA block 0', 'barrier 2 wait', 'memory section 1', 'ring wait (vmcnt)', 'barrier 3 wait',
            'MFMA block 1', 'barrier 4 wait']


def build(defines):
    from merlot_reserve_amd import build as B
    B.build(force=False)
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    os.makedirs(os.path.dirname(STAMP_LIB), exist_ok=True)
    obj = os.path.join(PKG, 'variants', 'gemm3_tn_stamps.o')
    subprocess.check_call([hipcc, '--offload-arch=gfx950', '-O3', '-fPIC', '-std=c++17', '-DMR_TN_STAMPS'] + defines +
                          ['-x', 'hip', '-c', os.path.join(B.CSRC, 'gemm3.hip'), '-o', obj])
    objs = [os.path.join(PKG, 'build', s.rsplit('.', 1)[0] + '.o') for s in B.SOURCES if s != 'gemm3.hip']
    subprocess.check_call([hipcc, '--offload-arch=gfx950', '-shared', '-fPIC', '-Wl,-z,defs', '-Wl,--version-script=' + os.path.join(B.CSRC, 'exports.map'),
                           '-o', STAMP_LIB] + objs + [obj, '-ldl'])
    print('built', STAMP_LIB)


def run(lib, group):
    env = dict(os.environ, MR_LIB=lib)
    p = subprocess.run([sys.executable, os.path.join(ROOT, 'scripts', 'tn_kloop_bench.py'), 'once', group], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       text=True, timeout=300)
    if p.returncode != 0:
        sys.stderr.write(p.stderr[-3000:])
        raise SystemExit(f'the stamped run failed with status {p.returncode}')
    rows = [[int(v) for v in ln.split()[1:]] for ln in p.stderr.splitlines() if ln.startswith('TNSTAMP ')]
    if not rows:
        raise SystemExit(f'{lib} printed no stamps: is it the -DMR_TN_STAMPS build?')
    print(p.stdout.strip())
    nseg = len(SEGMENTS)
    print(f'{len(rows)} stamped waves (wave 0 of each group, every workgroup, every launch); shader clocks per k-tile, mean over waves [min .. max of the per-wave means]')
    for g in (0, 1):
        sel = [r for r in rows if r[1] == g]
        tot = [sum(r[3:3 + nseg]) / r[2] for r in sel]
        print(f'group {g}: {sum(tot) / len(tot):8.1f} clocks per k-tile [{min(tot):.0f} .. {max(tot):.0f}]')
        for k, name in enumerate(SEGMENTS):
            v = [r[3 + k] / r[2] for r in sel]
            mean = sum(v) / len(v)
            print(f'    {name:20s} {mean:8.1f}  {100 * mean / (sum(tot) / len(tot)):5.1f} %   [{min(v):.0f} .. {max(v):.0f}]')
        mf = sum((r[5] + r[10]) / r[2] for r in sel) / len(sel)
        print(f'    MFMA blocks {mf:.0f} of {sum(tot) / len(tot):.0f} clocks; the bare issue time of 2 x 32 MFMAs is 2 x 512')


if __name__ == '__main__':
    if len(sys.argv) > 1 and sys.argv[1] == 'build':
        build(sys.argv[2:])
    elif len(sys.argv) > 1 and sys.argv[1] == 'run':
        run(sys.argv[2] if len(sys.argv) > 2 else STAMP_LIB, sys.argv[3] if len(sys.argv) > 3 else 'tn-base')
    else:
        raise SystemExit(__doc__)
