"""What feeding the finetuning step from shards costs, on one MI355X in one session (profiles/finetune_driver_cost.txt):
python scripts/finetune_driver_cost.py OUT.txt [--quick]

  1. the driver's interval ms_per_step (merlot_reserve_amd.finetune_train on synthetic shards whose frames are stored at 288 x 512) against the
     resident-batch step of scripts/bench_vcr.py (large, B = 4) and scripts/bench_tvqa.py (B = 4), alternating, each as a child process
  2. the readers' examples per second at 16 parser processes against what the step consumes
  3. max_memory_allocated of the forward-only model against the training model at the same B
  4. validation examples per second (val_epoch on the forward-only model)
Every child runs under its own time limit and the script stops at the first one that fails."""
import json
import os
import re
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def child(out, limit, *cmd):
    t0 = time.perf_counter()
    p = subprocess.run([sys.executable, *cmd], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=limit)
    if p.returncode != 0:
        out.write(f'FAILED ({p.returncode}): {" ".join(cmd)}\n{p.stdout[-2000:]}\n')
        out.flush()
        sys.exit(1)
    return p.stdout, time.perf_counter() - t0


def write_shards(task, cfg, directory, n_train, n_val, frame_hw=(288, 512)):
    import numpy as np
    from merlot_reserve_amd import finetune_records as FR
    os.makedirs(directory, exist_ok=True)
    rng = np.random.default_rng(0)
    keys, index = {}, 0
    for split, n in (('train', n_train), ('val', n_val)):
        pattern = os.path.join(directory, f'{split}{{:03d}}of002.tfrecord')
        for i in range(2):
            recs = []
            for _ in range(n // 2):
                kw = {'split': split} if task == 'vcr' else {}
                recs.append(FR.SYNTHETIC_RECORD[task](cfg, rng, index=index, frame_hw=frame_hw, **kw))
                index += 1
            FR.write_tfrecord(pattern.format(i), recs)
        keys[f'{split}_fns'], keys[f'num_{split}_files'] = pattern, 2
    json.dump(keys, open(os.path.join(directory, 'shards.json'), 'w'))
    return keys


def main():
    out = open(sys.argv[1], 'w')
    quick = '--quick' in sys.argv
    import torch
    from merlot_reserve_amd import finetune_eval as E
    from merlot_reserve_amd import finetune_records as FR
    from merlot_reserve_amd import finetune_train as FT
    from merlot_reserve_amd.config import load_config
    tmp = tempfile.mkdtemp(prefix='ftcost_')
    B, steps = 4, 60 if quick else 150
    say = lambda s: (out.write(s + '\n'), out.flush(), print(s, flush=True))
    say(f'finetuning driver cost, one session on {torch.cuda.get_device_name(0)}; B = {B}, {steps} driver steps per run, log interval 50')
    tasks = {'vcr': (['-output_grid_h', '18', '-output_grid_w', '32'], 'large'), 'tvqa': (['-output_grid_h', '12', '-output_grid_w', '20'], 'large')}
    cfgs = {}
    for task, (grid, name) in tasks.items():
        args = FT.build_parser().parse_args([task, name, '', '--records-per-gpu', str(B), '--train-size', str(B * steps), '-ne', '1', *grid])
        cfg = FT.task_overrides(load_config(name), task, args)
        cfg['data'].update(write_shards(task, cfg, os.path.join(tmp, task), 256, 64))
        cfgs[task] = cfg
    say('\n1. shard-fed driver interval ms_per_step against the resident-batch step (alternating)')
    for rnd in range(1 if quick else 2):
        for task, (grid, name) in tasks.items():
            if task == 'vcr':
                txt, _ = child(out, 400, 'scripts/bench_vcr.py', name, str(B), '40')
            else:
                txt, _ = child(out, 500, 'scripts/bench_tvqa.py', '30', '--limit', '400')
            for line in txt.splitlines():
                if 'ms/step' in line:
                    say(f'  round {rnd} resident  {line.strip()[:150]}')
            d = os.path.join(tmp, f'{task}_run{rnd}')
            _txt, wall = child(out, 600, '-m', 'merlot_reserve_amd.finetune_train', task, name, '', '--records-per-gpu', str(B), '--train-size', str(B * steps),
                               '-ne', '1', '--max-steps', str(steps), *grid, '--synthetic-shards', os.path.join(tmp, task), '-output_dir', d, '-val_batch_size', '32')
            ms = [round(r['ms_per_step'], 2) for r in map(json.loads, open(os.path.join(d, 'train_log.jsonl'))) if 'ms_per_step' in r]
            val = [json.loads(l) for l in open(os.path.join(d, 'val_log.jsonl'))]
            say(f'  round {rnd} driver    {task} {name} B={B}: interval ms_per_step {ms} (the first interval holds the eager step and the capture); '
                f'validation of {val[-1]["num_examples"]} examples at the end; {wall:.0f} s wall in all')
    say('\n2. reader throughput, 16 parser processes, frames stored at 288 x 512 (examples / s over 256 examples after the pool is up)')
    for task, cfg in cfgs.items():
        it = FR.finetune_input_fn_builder(cfg, task, seed=0, workers=16, sep_tokens=FR.SEP_TOKEN_IDS)
        next(it)
        t0, n = time.perf_counter(), 0
        while n < 256:
            ids, _b = next(it)
            n += len(ids)
        dt = time.perf_counter() - t0
        it.close()
        say(f'  {task}: {n / dt:.0f} examples / s')
    say('\n3. max_memory_allocated, training model against forward-only model (large, B = 4), and 4. validation examples / s (64 examples, batches of 32)')
    dev = torch.device('cuda:0')
    for task, cfg in cfgs.items():
        peak = {}
        for train in (True, False):
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            torch.cuda.reset_peak_memory_stats(dev)
            base = torch.cuda.memory_allocated(dev)
            model, batch = FT.model_and_batch(task, cfg, B, dev, train=train)
            model.init_from_dummy_batch(batch)
            model.apply(None, batch)
            torch.cuda.synchronize()
            peak[train] = (torch.cuda.max_memory_allocated(dev) - base) / 2 ** 20
            del model, batch
        say(f'  {task}: training model {peak[True]:.0f} MiB, forward-only model {peak[False]:.0f} MiB ({100 * peak[False] / peak[True]:.1f} %)')
        vcfg = json.loads(json.dumps(cfg))
        vcfg['device']['batch_size'] = 32
        model, batch = FT.model_and_batch(task, vcfg, 32, dev, train=False)
        model.init_from_dummy_batch(batch)
        for rep in range(2):
            t0 = time.perf_counter()
            acc, rows = E.val_epoch(model, FR.finetune_val_input_fn_builder(vcfg, task, workers=8, processes=False, sep_tokens=FR.SEP_TOKEN_IDS), task)
            dt = time.perf_counter() - t0
        say(f'  {task}: validation {len(rows) / dt:.1f} examples / s (second pass; reader on 8 threads in the same process)')
        del model, batch
    out.close()


if __name__ == '__main__':
    main()
