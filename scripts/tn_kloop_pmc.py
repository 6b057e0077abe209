"""Sums the counters of one `rocprofv3 --pmc ... --kernel-trace --output-format csv -d DIR -- python scripts/tn_kloop_bench.py once GROUP` pass over the
dispatches of the GEMM kernel under test and prints them with the ratios the k-loop comparison reads (profiles/tn_kloop_before.txt).

    python scripts/tn_kloop_pmc.py DIR [label]"""
import collections
import csv
import glob
import sys

d, label = sys.argv[1], (sys.argv[2] if len(sys.argv) > 2 else '')
cc = glob.glob(d + '/**/*counter_collection.csv', recursive=True)
kt = glob.glob(d + '/**/*kernel_trace.csv', recursive=True)
if not cc or not kt:
    raise SystemExit(f'{d}: no counter_collection / kernel_trace csv')
dur = {r['Dispatch_Id']: int(r['End_Timestamp']) - int(r['Start_Timestamp']) for r in csv.DictReader(open(kt[0]))}
agg = collections.defaultdict(lambda: collections.defaultdict(float))
seen = collections.defaultdict(set)
for r in csv.DictReader(open(cc[0])):
    k = r['Kernel_Name']
    if 'gemm3' not in k:
        continue
    k = 'gemm3_tn_kernel' if 'gemm3_tn' in k else k.split('(')[0].replace('void ', '')
    agg[k][r['Counter_Name']] += float(r['Counter_Value'])
    if r['Dispatch_Id'] not in seen[k]:
        seen[k].add(r['Dispatch_Id'])
        agg[k]['_ns'] += dur.get(r['Dispatch_Id'], 0)
for k, a in agg.items():
    n = len(seen[k])
    print(f'[{label}] {k}: {n} dispatches, {a["_ns"] / n / 1e3:.1f} us each under the counter pass')
    for c in sorted(a):
        if not c.startswith('_'):
            print(f'    {c:34s} {a[c] / n:16.0f} per dispatch')
    wc, busy = a.get('SQ_WAVE_CYCLES', 0.0), a.get('SQ_BUSY_CYCLES', 0.0)

    def ratio(name, x, y):
        if a.get(x) and a.get(y):
            print(f'    {name:52s} {a[x] / a[y]:8.4f}')
    ratio('MFMA busy / wave cycles', 'SQ_VALU_MFMA_BUSY_CYCLES', 'SQ_WAVE_CYCLES')
    ratio('MFMA busy / SQ busy cycles', 'SQ_VALU_MFMA_BUSY_CYCLES', 'SQ_BUSY_CYCLES')
    ratio('MFMA busy / (GRBM_GUI_ACTIVE)', 'SQ_VALU_MFMA_BUSY_CYCLES', 'GRBM_GUI_ACTIVE')
    ratio('wave cycles parked (WAIT_ANY / WAVE_CYCLES)', 'SQ_WAIT_ANY', 'SQ_WAVE_CYCLES')
    ratio('wave cycles issue-stalled (WAIT_INST_ANY / WAVE_CYCLES)', 'SQ_WAIT_INST_ANY', 'SQ_WAVE_CYCLES')
    ratio('wave cycles issuing (ACTIVE_INST_ANY / WAVE_CYCLES)', 'SQ_ACTIVE_INST_ANY', 'SQ_WAVE_CYCLES')
    ratio('LDS array active / wave cycles', 'SQ_LDS_IDX_ACTIVE', 'SQ_WAVE_CYCLES')
    ratio('LDS bank conflict cycles / LDS array active', 'SQ_LDS_BANK_CONFLICT', 'SQ_LDS_IDX_ACTIVE')
    ratio('LDS issue-stall / wave cycles', 'SQ_WAIT_INST_LDS', 'SQ_WAVE_CYCLES')
    ratio('LDS array active cycles per LDS instruction', 'SQ_LDS_IDX_ACTIVE', 'SQ_INSTS_LDS')
