"""Measurements of the micro-batched step (merlot_reserve_amd/microbatch.py) on one MI355X; one JSON line per result (profiles/microbatch_step.txt).

    python scripts/microbatch_bench.py time   [--model base] [--B 16] [--K 4] [--steps 100]   graph step of MicroBatchTrainer(B, K) against Trainer(B / K),
                                                                                               alternating blocks of 10 steps in one process: ms per record
    python scripts/microbatch_bench.py kernel [--model base]                                   ops.accumulate_rows on the model's flat gradient: us, GB/s
    python scripts/microbatch_bench.py memory --model base --B 16 --K 4                        torch.cuda.max_memory_allocated of construction + two steps
                                                                                               (K = 0: Trainer(B)); run once per process
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from merlot_reserve_amd import ops                                # noqa: E402
from merlot_reserve_amd.config import load_config                 # noqa: E402
from merlot_reserve_amd.microbatch import MicroBatchTrainer       # noqa: E402
from merlot_reserve_amd.synthetic import make_batch               # noqa: E402
from merlot_reserve_amd.trainer import Trainer                    # noqa: E402


def _tiled_batch(cfg, b, K, seed, dev):
    """K copies of one micro-batch of b records (time and memory do not depend on the contents; a base batch of 128 records costs minutes of host time)."""
    mb = make_batch(cfg, b, seed=seed, device=dev)
    if K == 1:
        return mb
    import numpy as np
    return {k: (np.concatenate([v] * K) if isinstance(v, np.ndarray) else torch.cat([v] * K)) for k, v in mb.items()}


def _timed(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / n


def cmd_time(args, dev):
    cfg = load_config(args.model)
    B, K = args.B, args.K
    b = B // K
    runs = {}
    for name, tr, batch in (('trainer', Trainer(cfg, b, dev, seed=0), make_batch(cfg, b, seed=1234, device=dev)),
                            ('microbatch', MicroBatchTrainer(cfg, B, dev, micro_batches=K, seed=0), _tiled_batch(cfg, b, K, 1234, dev))):
        plan = tr.plan(batch)
        tr.train_step(batch, plan=plan)
        tr.capture(batch)
        for _ in range(3):
            tr.train_step_graph(batch, plan)
        torch.cuda.synchronize()
        runs[name] = (tr, batch, plan, B if name == 'microbatch' else b, [])
    block = 10
    for _ in range(max(args.steps // block, 1)):
        for name, (tr, batch, plan, _n, ms) in runs.items():
            ms.append(_timed(lambda: tr.train_step_graph(batch, plan), block))
    out = {'what': 'time', 'model': args.model, 'B': B, 'K': K, 'steps_each': block * len(runs['trainer'][4])}
    for name, (_tr, _b, _p, n, ms) in runs.items():
        ms = sorted(ms)
        med = ms[len(ms) // 2]
        out[name] = {'records': n, 'ms_per_step_median_of_blocks': round(med, 3), 'min': round(ms[0], 3), 'max': round(ms[-1], 3), 'ms_per_record': round(med / n, 3)}
    out['ratio_ms_per_record'] = round(out['microbatch']['ms_per_record'] / out['trainer']['ms_per_record'], 4)
    print(json.dumps(out), flush=True)


def cmd_kernel(args, dev):
    from merlot_reserve_amd.params import ParamStore
    n = ParamStore(load_config(args.model), 'meta', init=False).total
    src = torch.randn(n, device=dev).to(torch.bfloat16)
    acc = torch.zeros(n, dtype=torch.float32, device=dev)
    for _ in range(3):
        ops.accumulate_rows(src, acc, scale=0.25)
    torch.cuda.synchronize()
    ms = sorted(_timed(lambda: ops.accumulate_rows(src, acc, scale=0.25), 20) for _ in range(5))
    us = ms[len(ms) // 2] * 1e3
    print(json.dumps({'what': 'kernel', 'model': args.model, 'elements': n, 'bytes': 10 * n, 'us_median_of_5x20': round(us, 1), 'min_us': round(ms[0] * 1e3, 1),
                      'max_us': round(ms[-1] * 1e3, 1), 'GBps': round(10 * n / us / 1e3, 1), 'of_6300_GBps_achievable': round(10 * n / us / 1e3 / 6300, 3)}), flush=True)


def cmd_memory(args, dev):
    cfg = load_config(args.model)
    B, K = args.B, args.K
    torch.cuda.reset_peak_memory_stats()
    if K == 0:
        tr, batch = Trainer(cfg, B, dev, seed=0), make_batch(cfg, B, seed=1234, device=dev)
    else:
        tr, batch = MicroBatchTrainer(cfg, B, dev, micro_batches=K, seed=0), _tiled_batch(cfg, B // K, K, 1234, dev)
    built = torch.cuda.memory_allocated()
    plan = tr.plan(batch)
    for _ in range(2):
        tr.train_step(batch, plan=plan)
    torch.cuda.synchronize()
    loss = tr.loss_info()['loss']
    print(json.dumps({'what': 'memory', 'model': args.model, 'B': B, 'K': K, 'b': B // max(K, 1), 'allocated_after_construction_GiB': round(built / 2 ** 30, 2),
                      'max_memory_allocated_GiB': round(torch.cuda.max_memory_allocated() / 2 ** 30, 2), 'loss': loss}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('cmd', choices=['time', 'kernel', 'memory'])
    ap.add_argument('--model', default='base')
    ap.add_argument('--B', type=int, default=16)
    ap.add_argument('--K', type=int, default=4)
    ap.add_argument('--steps', type=int, default=100)
    args = ap.parse_args()
    dev = torch.device('cuda', 0)
    torch.cuda.set_device(dev)
    {'time': cmd_time, 'kernel': cmd_kernel, 'memory': cmd_memory}[args.cmd](args, dev)


if __name__ == '__main__':
    main()
