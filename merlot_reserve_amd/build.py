"""Builds libmreserve_hip.so, libmreserve_media.so, libmreserve_zeroshot.so and libmreserve_ingest.so (gfx950) in-tree with hipcc.  No torch extension
machinery: the libraries are plain C-ABI shared objects (include/mreserve_hip.h, include/mreserve_media.h, include/mreserve_zeroshot.h,
include/mreserve_ingest.h) loaded through ctypes."""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, 'csrc')
LIB = os.path.join(HERE, 'libmreserve_hip.so')
# attention.hip: the SLP vectoriser turns adjacent scalar fp32 adds / multiplies of the softmax into v_pk_add_f32 / v_pk_mul_f32, which
# issue slower than the scalar pairs they replace on gfx950 (MI355X_MICROARCH.md): 961 -> 192 packed ops, backward kernels 2-4 % faster
# layernorm.hip / rowops.hip / adam.hip: -fno-slp-vectorize for CORRECTNESS.  With SLP the LayerNorm kernels' (x - mean) * (rstd * gamma) + beta
# became v_pk_add_f32 / v_pk_mul_f32 / v_pk_fma_f32 with op_sel operands, and in ~1e-4 of the rows element 0 of the 16-byte vectors of
# lanes 48-63 came out as if computed from other mean / rstd -- only while a second queue's kernels shared the chip (the audio tower on
# the side stream), never with one stream; run-to-run differences of a bf16 ulp or seven that made eager steps, hipGraph replays
# and repeated replays of the SAME step disagree (scripts/det_check.py).  Scalar fp32 code: bit-identical
# results in every mode.  These kernels are HBM-bound: no cost.  adam.hip also -ffp-contract=off: the optimizer state is byte data
# (pretrain/optimization.py:36-51), the oracle evaluates (1 - b) * g + b * m without fused multiply-adds.
# Round 4 reduced the trigger (scripts/slp_repro.py, tests/test_coresident_determinism_gpu.py): packed fp32 code with op_sel / neg operands goes wrong
# in lanes 48-63 while waves of an MFMA kernel (the small 128 x 128 GEMM) share the SIMD.  f32path.hip / f32bwd.hip (not performance paths) are built
# scalar as well; the bf16 GEMM files keep their packed epilogues (3.2 ms of the step) and are held to bit-stability under that neighbour by the test.
EXTRA_FLAGS = {'attention.hip': ['-fno-slp-vectorize'], 'layernorm.hip': ['-fno-slp-vectorize'], 'rowops.hip': ['-fno-slp-vectorize'],
               'adam.hip': ['-fno-slp-vectorize', '-ffp-contract=off'], 'f32bwd.hip': ['-fno-slp-vectorize'], 'f32path.hip': ['-fno-slp-vectorize'],
               'media.hip': ['-fno-slp-vectorize'], 'zeroshot.hip': ['-fno-slp-vectorize'], 'ingest.hip': ['-fno-slp-vectorize']}
# The hazard at instruction level (scripts/micro/pk_probe.hip, scripts/pk_probe.py): v_pk_add_f32 / v_pk_fma_f32 (any packed fp32 arithmetic) with an
# `op_sel:[..1..]` source -- the LOW result element reading the HIGH register of a source pair -- returns wrong values in lanes 48-63 of a wave
# while another kernel's MFMA waves are resident on its SIMD (0 mismatches alone; op_sel_hi, neg_lo / neg_hi, v_pk_mov_b32 op_sel are unaffected).
# EVERY .hip file is scanned (round 5: the files built without the SLP pass still contain packed fp32 arithmetic from explicit vector
# expressions -- attention.hip 272 instructions -- so "built scalar" alone does not exclude the form): the device assembly of each
# object is kept under build/ (a by-product of the object's own compile, --save-temps) and build() fails if such an instruction appears.
SLP_FILES = ['gemm.hip', 'gemm256.hip', 'gemm3.hip', 'gemm4.hip', 'gemm5.hip']        # the files that keep the SLP vectoriser (packed epilogues)
HAZARD_RE = r'^\s*v_pk_(add|mul|fma|min|max)_f32\b.*\bop_sel:\['
SOURCES = ['gemm.hip', 'gemm256.hip', 'gemm3.hip', 'gemm4.hip', 'gemm5.hip', 'gemm_route.cpp', 'attention.hip', 'layernorm.hip', 'rowops.hip', 'adam.hip', 'f32path.hip', 'f32bwd.hip', 'mr_error.cpp', 'comm.cpp', 'hostio.cpp']
HIP_FILES = [f for f in SOURCES if f.endswith('.hip')]
# libmreserve_media.so (include/mreserve_media.h, symbols mrm_*): the media front end, a library of its own -- it needs none of the other library's
# handles or options.  fp32 code, built scalar like the other fp32 files, scanned like them, and with no spill allowance.
MEDIA_LIB = os.path.join(HERE, 'libmreserve_media.so')
MEDIA_SOURCES = ['media.hip']
MEDIA_HIP_FILES = [f for f in MEDIA_SOURCES if f.endswith('.hip')]
# libmreserve_zeroshot.so (include/mreserve_zeroshot.h, symbols mrz_*): the zero-shot head (logits, log-sum-exp, top-k, group marginal), a third
# library on the same terms: its own symbols only, fp32 code built scalar, scanned, no spill allowance.
ZEROSHOT_LIB = os.path.join(HERE, 'libmreserve_zeroshot.so')
ZEROSHOT_SOURCES = ['zeroshot.hip']
ZEROSHOT_HIP_FILES = [f for f in ZEROSHOT_SOURCES if f.endswith('.hip')]
# libmreserve_ingest.so (include/mreserve_ingest.h, symbols mri_*): PCM resampling / downmix and black-bar bounds, a fourth library on the same
# terms: its own symbols only, fp32 code built scalar, scanned, no spill allowance.
INGEST_LIB = os.path.join(HERE, 'libmreserve_ingest.so')
INGEST_SOURCES = ['ingest.hip']
INGEST_HIP_FILES = [f for f in INGEST_SOURCES if f.endswith('.hip')]
LIBS = (LIB, MEDIA_LIB, ZEROSHOT_LIB, INGEST_LIB)
# Register spills (metadata .vgpr_spill_count / .sgpr_spill_count of every kernel in the device assembly): a spill inside a k-loop costs more than any
# schedule gains (gemm4<256,0> with 183 spilled registers: 299 vs 91 us), so build() FAILS on a kernel with spilled vector registers unless it is
# listed here with the number it is known to carry and the reason it is tolerated.  {regex on the demangled-ish symbol: (max spilled VGPRs, why)}
# Round 5 state (scripts/spill_sites.py prints, per kernel, the basic blocks with scratch traffic and whether they lie in the k-loop; its output is
# committed as profiles/r05_spill_sites.txt): removed -- gemm4<256,0> (183, reloads in the k-loop: the 256-wide bias mode stays on the ping-pong
# kernel), gemm3<256,4,1> (20, one reload in the k-loop's MFMA block: that mode always runs two-phase), gemm_bf16_kernel / gemm_bf16_grouped_kernel
# (22-42: address arithmetic hoisted over the epilogue's staging loop, now pinned behind an opaque move).  Tolerated, all COLD (per-tile epilogue /
# item-switch / prologue code of persistent kernels; `hot_spill_blocks()` = scratch instructions in a basic block that also holds MFMAs, which
# tests/test_build_isa_guard.py holds to the three kernels marked HOT below):
SPILL_ALLOWED = {
    r'gemm4_kernelILi256ELi[35]E': (5, 'epilogue: two row-offset registers and three fragment registers of the next tile held across the store section; k-loop block clean'),
    r'gemm256_kernelILi256E': (24, 'DMA source offsets of the tile pieces, reloaded in the per-item setup (also where the cursor switches items inside the unrolled k-loop, under its uniform branch) and epilogue prefetch registers; no MFMA block touches scratch'),
    r'gemm256_kernelILi192E': (5, 'as the 256-wide instance'),
    r'gemm5_kernelILi[012]ELi4ELi256ELi3E': (11, 'per-tile item decode + epilogue offsets of the two-per-CU geometry (<= 128 registers per wave by design); no MFMA block touches scratch'),
    r'gemm5_kernelILi4ELi4ELi256ELi3E': (20, 'HOT (4 stores in an MFMA block).  aux mode of the two-per-CU geometry: NOT dispatched by the default policy (aux arrives with column sums, which it refuses); option gemm5=1 only'),
    r'attn_bwd_dq_kernelILi2ELb1E': (4, 'HOT (3 reloads in an MFMA block).  held to three waves per SIMD on purpose: 168 registers + 14 spilled is faster than 184 at two waves (joint backward 181 -> 175 us, round 2)'),
    r'attn_bwd1_kernelILb1E': (6, 'HOT (1 reload in an MFMA block).  masked one-pass backward (no stock tower routes to it)'),
    r'attn_bwd1_kernelILb0E': (3, 'one register held from the prologue to the epilogue, reloaded once outside the tile loop (round 5: the per-query scalars of the next tile now stay in registers across a tile)'),
}
STAMP = os.path.join(HERE, 'build', 'flags.txt')
JOBS = max(1, min(8, (os.cpu_count() or 2)))


def _flag_stamp():
    """What the objects under build/ were compiled with: a rebuild is needed when it differs (e.g. EXTRA_FLAGS changed), not only when a source is newer."""
    return ''.join(f'{k}: {" ".join(v)}\n' for k, v in sorted(EXTRA_FLAGS.items()))


def _asm_path(src):
    return os.path.join(HERE, 'build', src.rsplit('.', 1)[0] + '.s')


def _needs_build():
    if not all(os.path.exists(p) for p in LIBS):
        return True
    if not os.path.exists(STAMP):
        # a library that travelled without its build/ directory (the GPU box's snapshot carries both; a bare copy does not): trust the mtimes
        pass
    elif open(STAMP).read() != _flag_stamp():
        return True
    t = min(os.path.getmtime(p) for p in LIBS)
    deps = [os.path.join(CSRC, f) for f in os.listdir(CSRC)] + [os.path.join(HERE, '..', 'include', h) for h in ('mreserve_hip.h', 'mreserve_media.h', 'mreserve_zeroshot.h', 'mreserve_ingest.h')]
    return any(os.path.getmtime(d) > t for d in deps)


def _asm_stale():
    return any(not os.path.exists(_asm_path(f)) or os.path.getmtime(_asm_path(f)) < os.path.getmtime(os.path.join(CSRC, f)) for f in HIP_FILES + MEDIA_HIP_FILES + ZEROSHOT_HIP_FILES + INGEST_HIP_FILES)


def scan_packed_op_sel(files=None):
    """[(file, count, example)] of hazardous packed-fp32 instructions in the device assembly build() left under build/ (see HAZARD_RE), every .hip file."""
    import re
    out = []
    rx = re.compile(HAZARD_RE, re.M)
    for src in (files or HIP_FILES):
        asm = _asm_path(src)
        if not os.path.exists(asm):
            raise FileNotFoundError(f'{asm}: run merlot_reserve_amd.build.build(force=True)')
        hits = [m.group(0).strip() for m in rx.finditer(open(asm).read())]
        if hits:
            out.append((src, len(hits), hits[0]))
    return out


def kernel_resources(files=None):
    """{file: {kernel symbol: {'vgpr', 'agpr', 'sgpr', 'vgpr_spill', 'sgpr_spill', 'lds', 'scratch'}}} from the amdhsa.kernels metadata of the device assembly."""
    import re
    res = {}
    key = {'.vgpr_count': 'vgpr', '.agpr_count': 'agpr', '.sgpr_count': 'sgpr', '.vgpr_spill_count': 'vgpr_spill', '.sgpr_spill_count': 'sgpr_spill',
           '.group_segment_fixed_size': 'lds', '.private_segment_fixed_size': 'scratch'}
    for src in (files or HIP_FILES):
        text = open(_asm_path(src)).read()
        i = text.find('amdhsa.kernels:')
        if i < 0:
            res[src] = {}
            continue
        j = text.find('amdhsa.target:', i)
        ks = {}
        for block in re.split(r'\n  - ', text[i:j if j > 0 else len(text)])[1:]:
            ent = {}
            name = None
            for line in block.splitlines():
                m = re.match(r'\s*(\.[a-z_]+):\s*(\S+)\s*$', line)
                if not m:
                    continue
                if m.group(1) == '.name':
                    name = m.group(2).strip("'\"")
                elif m.group(1) in key:
                    ent[key[m.group(1)]] = int(m.group(2))
            if name:
                ks[name] = ent
        res[src] = ks
    return res


def hot_spill_blocks(files=None):
    """[(file, kernel, block label, MFMAs, scratch stores, scratch loads)]: basic blocks of the device assembly that hold both MFMAs and scratch traffic."""
    import re
    out = []
    for src in (files or HIP_FILES):
        name, blk = None, None
        for line in open(_asm_path(src)):
            m = re.match(r'^(_Z\w+):', line)
            if m:
                name, blk = m.group(1), ['<entry>', 0, 0, 0]
                continue
            if name is None:
                continue
            if line.startswith('.Lfunc_end') or re.match(r'^\.LBB\d+_\d+:', line):
                if blk[1] and (blk[2] or blk[3]):
                    out.append((src, name, *blk))
                blk = [line.split(':')[0], 0, 0, 0]
                if line.startswith('.Lfunc_end'):
                    name = None
                continue
            t = line.strip()
            if t.startswith('v_mfma'):
                blk[1] += 1
            elif t.startswith('scratch_store'):
                blk[2] += 1
            elif t.startswith('scratch_load'):
                blk[3] += 1
    return out


def scan_spills(files=None):
    """[(file, kernel, spilled VGPRs)] of kernels with spilled vector registers that SPILL_ALLOWED does not cover."""
    import re
    bad = []
    for src, ks in kernel_resources(files).items():
        for name, ent in ks.items():
            n = ent.get('vgpr_spill', 0)
            if n <= 0:
                continue
            cap = max([c for rx, (c, _why) in SPILL_ALLOWED.items() if re.search(rx, name)], default=0)
            if n > cap:
                bad.append((src, name, n))
    return bad


def build(force=False, verbose=True):
    if not force and not _needs_build():
        return LIB
    import json
    all_hip = HIP_FILES + MEDIA_HIP_FILES + ZEROSHOT_HIP_FILES + INGEST_HIP_FILES
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    bdir = os.path.join(HERE, 'build')
    os.makedirs(bdir, exist_ok=True)
    objs, media_objs, zeroshot_objs, ingest_objs, queue, running, failed = [], [], [], [], [], [], []
    for src in SOURCES + MEDIA_SOURCES + ZEROSHOT_SOURCES + INGEST_SOURCES:
        stem = src.rsplit('.', 1)[0]
        obj = os.path.join(bdir, stem + '.o')
        cmd = [hipcc, '--offload-arch=gfx950', '-O3', '-fPIC', '-std=c++17'] + EXTRA_FLAGS.get(src, []) + ['-x', 'hip', '-c', os.path.join(CSRC, src), '-o', obj]
        if src.endswith('.hip'):
            cmd.append('--save-temps=obj')          # leaves <stem>-hip-amdgcn-amd-amdhsa-gfx950.s: the device assembly OF THIS OBJECT, for the scans
        queue.append((src, cmd))
        (media_objs if src in MEDIA_SOURCES else zeroshot_objs if src in ZEROSHOT_SOURCES else ingest_objs if src in INGEST_SOURCES else objs).append(obj)
    while queue or running:
        while queue and len(running) < JOBS:
            src, cmd = queue.pop(0)
            running.append((src, subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, cwd=bdir)))
        src, p = running.pop(0)
        out, _ = p.communicate()
        if p.returncode != 0:
            failed.append(f'hipcc failed on {src}:\n{out.decode()}')
    if failed:
        raise RuntimeError('\n'.join(failed))
    for src in all_hip:
        stem = src.rsplit('.', 1)[0]
        os.replace(os.path.join(bdir, stem + '-hip-amdgcn-amd-amdhsa-gfx950.s'), _asm_path(src))
        for f in os.listdir(bdir):                  # the other intermediates (preprocessed sources, bitcode, host assembly) are not needed
            if f.startswith(stem + '-h') or f.startswith(stem + '.hip-hip-'):
                os.remove(os.path.join(bdir, f))
    bad = scan_packed_op_sel(files=all_hip)
    if bad:
        raise RuntimeError('packed fp32 instructions with an op_sel source (wrong in lanes 48-63 beside MFMA waves, see build.py) in:\n' +
                           '\n'.join(f'{f}: {n} e.g. {ex}' for f, n, ex in bad) + '\nrestructure the code (SLP files: or compile with -fno-slp-vectorize)')
    with open(os.path.join(bdir, 'resources.json'), 'w') as f:
        json.dump(kernel_resources(all_hip), f, indent=1, sort_keys=True)
    spills = scan_spills(files=all_hip)
    if spills:
        raise RuntimeError('kernels with spilled vector registers (build.py SPILL_ALLOWED lists the tolerated ones):\n' +
                           '\n'.join(f'{f}: {k}: {n} VGPRs' for f, k, n in spills))
    # -z defs: an undefined kernel stub (a template the host pass silently failed to emit) fails the build instead of the first launch
    # --version-script: the dynamic symbol table is include/mreserve_hip.h's C names (mr_*) and nothing else -- the mangled C++ helpers the
    # translation units share, kernel handles and device stubs stay local (tests/test_cabi_exports.py reads `nm -D`)
    cmd = [hipcc, '--offload-arch=gfx950', '-shared', '-fPIC', '-Wl,-z,defs', '-Wl,--version-script=' + os.path.join(CSRC, 'exports.map'), '-o', LIB] + objs + ['-ldl']
    subprocess.check_call(cmd)
    cmd = [hipcc, '--offload-arch=gfx950', '-shared', '-fPIC', '-Wl,-z,defs', '-Wl,--version-script=' + os.path.join(CSRC, 'media_exports.map'), '-o', MEDIA_LIB] + media_objs
    subprocess.check_call(cmd)
    cmd = [hipcc, '--offload-arch=gfx950', '-shared', '-fPIC', '-Wl,-z,defs', '-Wl,--version-script=' + os.path.join(CSRC, 'zeroshot_exports.map'), '-o', ZEROSHOT_LIB] + zeroshot_objs
    subprocess.check_call(cmd)
    cmd = [hipcc, '--offload-arch=gfx950', '-shared', '-fPIC', '-Wl,-z,defs', '-Wl,--version-script=' + os.path.join(CSRC, 'ingest_exports.map'), '-o', INGEST_LIB] + ingest_objs
    subprocess.check_call(cmd)
    with open(STAMP, 'w') as f:
        f.write(_flag_stamp())
    if verbose:
        print(f'built {LIB}, {MEDIA_LIB}, {ZEROSHOT_LIB} and {INGEST_LIB}', file=sys.stderr)
    return LIB


if __name__ == '__main__':
    build(force='--force' in sys.argv)
