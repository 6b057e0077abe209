"""What logging costs the replayed step: the base step (4 records, resident synthetic batches, hipGraph replay) timed with device events in one
process, alternating three loops:
  plain      train_step_graph only (what bench.py times)
  ring       Trainer(metrics_ring=100): mr_metrics_push inside the graph, drain_metrics() every 50 steps (the driver's log)
  loss_info  Trainer.loss_info() after every step (a device synchronise per step: the stall the ring removes)
usage: python scripts/train_loop_cost.py [steps per pass = 300] [rounds = 2] [model = base] [records = 4]"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from merlot_reserve_amd.config import load_config  # noqa: E402
from merlot_reserve_amd.synthetic import make_batch  # noqa: E402
from merlot_reserve_amd.trainer import Trainer  # noqa: E402


def main():
    steps = int(sys.argv[1]) if len(sys.argv) > 1 else 300
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 2
    model = sys.argv[3] if len(sys.argv) > 3 else 'base'
    B = int(sys.argv[4]) if len(sys.argv) > 4 else 4
    dev = torch.device('cuda:0')
    cfg = load_config(model)
    batches = [make_batch(cfg, B, seed=1234 + 1000 * i, device=dev) for i in range(2)]
    trainers = {'plain': Trainer(cfg, B, dev, seed=0), 'ring': Trainer(cfg, B, dev, seed=0, metrics_ring=100)}
    for tr in trainers.values():
        tr.train_step(batches[0], plan=tr.plan(batches[0]))
        tr.capture(batches[0])
    trainers['ring'].drain_metrics(flush=True)                     # (the row of the eager step)
    trainers['loss_info'] = trainers['plain']

    def run(name, n):
        tr = trainers[name]
        rows = 0
        plan = tr.plan(batches[0])
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for i in range(n):
            tr.train_step_graph(batches[i % 2], plan)
            if name == 'loss_info':
                tr.loss_info()
            plan = tr.plan(batches[(i + 1) % 2])
            if name == 'ring' and (i + 1) % 50 == 0:
                rows += len(tr.drain_metrics())
        e1.record()
        if name == 'ring':
            rows += len(tr.drain_metrics(flush=True))
            assert rows == n, (rows, n)
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / n

    for name in trainers:
        run(name, 20)                                              # warm-up of every loop
    out = {k: [] for k in trainers}
    for _ in range(rounds):
        for name in trainers:
            out[name].append(round(run(name, steps), 4))
            print(name, out[name][-1], 'ms / step', flush=True)
    print(json.dumps({'what': f'{model}, {B} records, {steps} graph-replayed steps per pass, ms / step per pass', **out}))


if __name__ == '__main__':
    main()
