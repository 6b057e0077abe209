"""The pretraining loop: the counterpart of pretrain/train.py:55-145 on top of this package's own pieces.

    python -m merlot_reserve_amd.train CONFIG.yaml -output_dir DIR [--synthetic] [--records-per-gpu B] [--micro-batches K] [--max-steps N] [--gpus N] [--seed S]

data    records.ShardFeeder -> loader.PrefetchLoader (the config's train_fns), or --synthetic: synthetic.make_batch(seed + step) -> PrefetchLoader
step    Trainer(metrics_ring=...): the latest checkpoint of DIR is restored if there is one (train.py:101), one eager train_step, Trainer.capture,
        then one hipGraph replay per step; a communicator that cannot be captured (or the fp32-gradient program) steps eagerly
log     DIR/train_log.jsonl, one JSON line per step, written when the step's row of the trainer's metrics ring has reached the host -- one
        drain interval (device.commit_every_nsteps) late, like the reference's lagged log (train.py:119-129); the host never waits for the
        step it has just enqueued.  ms_per_step / video_segments_per_sec are per drain interval, from device events around it.
ckpt    checkpoint.save_checkpoint every device.iterations_per_loop steps and at the end, called on EVERY rank (sharded moments gather);
        fp32 leaves stay fp32 (keep_fp32) so that a restart is exact; --reference-format writes the reference's fp16 form instead.
--micro-batches K > 1: microbatch.MicroBatchTrainer steps the GPU's B records as K micro-batches of B / K -- exactly K reference devices per GPU, the
        loss over the keys of all gpus x K of them (the reference's device.batch_size: --gpus 8 --micro-batches K); the default 1 is Trainer as it is.
--gpus N without a launcher around it starts N ranks under torch.distributed.run as a CHILD process before this process touches the GPU.

With --synthetic a resumed run is bit-identical to an uninterrupted one (batch and draws are functions of (seed, step), the kernels reduce in a
fixed order, the Adam scalars are functions of the step).  With shards the reader starts again from its seed, as the reference's does."""
import argparse
import math
import os
import sys

from .driver import IntervalTimer, JsonlLog, checkpoint_due, init_rank, new_event, self_launch

OBJECTIVES = ('imgs_to_audio', 'text_to_audio', 'stuff_to_span')      # order of contrastive_scales (pretrain/train.py:134-139)
TIMING_KEYS = ('ms_per_step', 'video_segments_per_sec')


def build_parser():
    ap = argparse.ArgumentParser(description='MERLOT Reserve pretraining on MI355X')
    ap.add_argument('config_file', help="the config.yaml ('base' / 'large': the packaged ones)")
    ap.add_argument('-output_dir', dest='output_dir', default='', help='overrides device.output_dir of the config')
    ap.add_argument('--synthetic', action='store_true', help='batches from synthetic.make_batch(seed + step) instead of record shards')
    ap.add_argument('--records-per-gpu', type=int, default=None, help='records per GPU and step (default: device.batch_size // gpus)')
    ap.add_argument('--micro-batches', type=int, default=1, help='step the records of a GPU as K micro-batches of records-per-gpu / K (exact large-batch loss)')
    ap.add_argument('--max-steps', type=int, default=None, help='stop at this step (default: optimizer.num_train_steps)')
    ap.add_argument('--gpus', type=int, default=1)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--reference-format', action='store_true', help="checkpoints in the reference's format (fp32 leaves as fp16): a restart is fp16-rounded")
    return ap


def driver_settings(config, args):
    """What the loop reads from the YAML (as the reference does) and the command line."""
    dev, opt = config.get('device', {}), config['optimizer']
    out = args.output_dir or dev.get('output_dir', '')
    if not out:
        raise ValueError('no output directory: pass -output_dir or set device.output_dir')
    num_train_steps = int(opt.get('num_train_steps_override', opt['num_train_steps']))
    end = num_train_steps if args.max_steps is None else min(int(args.max_steps), num_train_steps)
    B = args.records_per_gpu if args.records_per_gpu is not None else max(int(dev.get('batch_size', args.gpus)) // args.gpus, 1)
    st = {'output_dir': out, 'ckpt_every': int(dev['iterations_per_loop']), 'log_every': int(dev.get('commit_every_nsteps', 50)),
          'end_step': end, 'records_per_gpu': int(B)}
    K = int(getattr(args, 'micro_batches', 1))
    if K != 1:                               # (the default leaves the settings as they were)
        from .microbatch import check_micro_batches
        check_micro_batches(B, K)            # ValueError here: before any GPU call
        st['micro_batches'] = K
    return st


def log_record(row, timing=None):
    """One line of train_log.jsonl from a row of Trainer.drain_metrics."""
    rec = {k: v for k, v in row.items() if k != 'contrastive_scales'}
    for name, v in zip(OBJECTIVES, row['contrastive_scales']):
        rec[f'temperature/{name}/log'] = v
        rec[f'temperature/{name}/exp'] = math.exp(v)
    rec.update(timing or {})
    return rec


def run_loop(trainer, feed, *, end_step, log_every, ckpt_every, save, write, timer=None, use_graph=True):
    """feed: iterator of batches (a '_draws' entry, if present, holds the step's random draws).  save(step) writes a checkpoint,
    write(row, timing) one log line.  Returns the number of steps run."""
    assert trainer.metrics_ring >= 2 * log_every, f'metrics ring of {trainer.metrics_ring} rows < 2 x the log interval {log_every}'
    step = start = trainer.state.step
    since = 0

    def emit(rows):
        for row in rows:
            write(row, timer.of(row['step']) if timer is not None else None)

    if step < end_step:
        for batch in feed:
            plan = trainer.plan(batch, batch.get('_draws'))
            if step > start and use_graph:
                trainer.train_step_graph(batch, plan)
            else:
                trainer.train_step(batch, plan=plan)
                if use_graph:
                    trainer.capture(batch)
            step += 1
            since += 1
            assert trainer.state.step == step
            if since == log_every or step == end_step:
                if timer is not None:
                    timer.mark(step)
                emit(trainer.drain_metrics())
                since = 0
            if checkpoint_due(step, ckpt_every, end_step):
                save(step)
            if step >= end_step:
                break
    if timer is not None:
        timer.mark(step)
    emit(trainer.drain_metrics(flush=True))            # the one synchronise of the run
    return step - start


class _Ahead:
    """items[i] = make(i) for i in order, `depth` of them in flight on `workers` threads: the synthetic batches are made on the host while
    the GPU steps (a base batch costs more host time than a step takes; torch's generators release the GIL)."""

    def __init__(self, make, indices, workers=4, depth=8):
        from collections import deque
        from concurrent.futures import ThreadPoolExecutor
        self.make, self.indices = make, iter(indices)
        self.pool, self.pending = ThreadPoolExecutor(workers), deque()
        for _ in range(depth):
            self._submit()

    def _submit(self):
        for i in self.indices:
            self.pending.append(self.pool.submit(self.make, i))
            return

    def __iter__(self):
        return self

    def __next__(self):
        if not self.pending:
            raise StopIteration
        item = self.pending.popleft().result()
        self._submit()
        return item

    def close(self):
        self.indices = iter(())
        for f in self.pending:
            f.cancel()
        self.pool.shutdown(wait=True)


def synthetic_batch(config, B, seed, step, rank=0, world=1):
    """Step s of rank r: make_batch(seed + s * world + r) and make_draws of the same seed -- functions of (seed, step) alone."""
    from .synthetic import make_batch, make_draws
    sd = seed + step * world + rank
    batch = make_batch(config, B, seed=sd, device='cpu')
    batch['_draws'] = make_draws(config, B, seed=sd)
    return batch


def synthetic_batches(config, B, seed, start_step, end_step, rank=0, world=1):
    for s in range(start_step, end_step):
        yield synthetic_batch(config, B, seed, s, rank, world)


def main(argv=None):
    argv = sys.argv[1:] if argv is None else list(argv)
    args = build_parser().parse_args(argv)
    if args.gpus > 1 and 'WORLD_SIZE' not in os.environ:
        return self_launch('merlot_reserve_amd.train', argv, args.gpus)

    import torch
    from . import checkpoint, records
    from .config import load_config
    from .loader import PrefetchLoader
    from .trainer import Trainer

    config = load_config(args.config_file)
    config['_path'] = args.config_file
    st = driver_settings(config, args)
    dev, comm, rank, world = init_rank(args.gpus)

    B, out_dir, log_every = st['records_per_gpu'], st['output_dir'], st['log_every']
    config.setdefault('device', {})['batch_size'] = B * world                 # what the shard reader divides by the world size
    bf16 = bool(config['model'].get('use_bfloat16', True))
    K = st.get('micro_batches', 1)
    if K == 1:
        trainer = Trainer(config, B, dev, rank=rank, world=world, seed=args.seed, comm=comm, bf16_grads=bf16, metrics_ring=2 * log_every)
    else:
        from .microbatch import MicroBatchTrainer
        trainer = MicroBatchTrainer(config, B, dev, micro_batches=K, rank=rank, world=world, seed=args.seed, comm=comm, bf16_grads=bf16,
                                    metrics_ring=2 * log_every)
    if rank == 0:
        print(f'training: gpus={world} records_per_gpu={B} micro_batches={K} (contrastive batch of {world * B} records as {world * K} devices)', flush=True)
    os.makedirs(out_dir, exist_ok=True)
    if checkpoint.latest_checkpoint(out_dir) is not None:                     # load if we can (train.py:101)
        checkpoint.load_checkpoint(out_dir, state=trainer.state)
        print(f'[rank {rank}] resumed from {checkpoint.latest_checkpoint(out_dir)} at step {trainer.state.step}', flush=True)
    start = trainer.state.step

    feeder = None
    if args.synthetic:
        torch.set_num_threads(1)                                              # (loader._stage: a spinning intra-op pool starves the runtime's helper threads)
        source = feeder = _Ahead(lambda s: synthetic_batch(config, B, args.seed, s, rank, world), range(start, st['end_step']))
    else:
        workers = max(2, min(14, (os.cpu_count() or 4) // world - 2))
        source = feeder = records.ShardFeeder(config, rank=rank, world=world, seed=args.seed, workers=workers)
    feed = PrefetchLoader(source, dev, depth=2, dtype=torch.bfloat16)

    log = JsonlLog(os.path.join(out_dir, 'train_log.jsonl'), rank)

    def save(step):
        fn = checkpoint.save_checkpoint(trainer.state, out_dir, rank=rank, keep_fp32=not args.reference_format)
        if rank == 0:
            print(f'saved {fn}', flush=True)

    timer = IntervalTimer(start, new_event, world * B * config['data']['num_segments'], 'video_segments_per_sec')
    use_graph = bf16 and (comm is None or comm.capturable)
    try:
        n = run_loop(trainer, feed, end_step=st['end_step'], log_every=log_every, ckpt_every=st['ckpt_every'], save=save,
                     write=lambda row, timing: log.write(log_record(row, timing)),
                     timer=timer, use_graph=use_graph)
    finally:
        feeder.close()
        log.close()
    torch.cuda.synchronize()
    if rank == 0:
        print(f'ran {n} steps to step {trainer.state.step}; log and checkpoints in {out_dir}', flush=True)
    if comm is not None:
        comm.close()
    return 0


if __name__ == '__main__':
    sys.exit(main())
