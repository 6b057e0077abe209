"""The finetuning loop: the counterpart of finetune/vcr/qa_qar_joint_finetune.py:96-133, 241-271 (V) and finetune/tvqa/tvqa_finetune.py:105-139,
363-390 (T) on top of this package's own pieces.

    python -m merlot_reserve_amd.finetune_train {vcr,tvqa} CONFIG.yaml CKPT [-lr LR] [-ne EPOCHS] [-output_grid_h H] [-output_grid_w W]
        [-output_name NAME] [-output_dir DIR] [-val_batch_size N] [-scan_minibatch] [--gpus N] [--records-per-gpu B] [--train-size N]
        [--max-steps N] [--data-dir DIR | --synthetic-shards DIR] [--seed S]

config  the pretraining YAML with the task's overrides (task_overrides: V:96-121 / T:105-131).  CKPT = '' starts from the initialised parameters
        (V:175-176), else the checkpoint's `params` are taken as they are: a pretraining tree's head / span_encoder (and, for VCR, audio_encoder)
        are not read, a tree without `proj` keeps the initialised one (V:183).
data    finetune_records.finetune_input_fn_builder -> loader.PrefetchLoader over --data-dir DIR's train{:03d}of256.tfrecord (validation:
        val{:03d}of008.tfrecord), the names the reference's scripts give their shards; --synthetic-shards DIR reads (and, if it holds none, first writes)
        synthetic shards there.  The reader's stream is a function of the seed, and a resumed run skips the batches the saved step has consumed.
step    one eager step, then VCRGraphStep / TVQAGraphStep replay; -scan_minibatch (or a communicator that cannot be captured) steps eagerly.
        The loop stops at optimizer.num_train_steps: the 100 extra steps of T:368 ("for some reason it crashes otherwise") are not reproduced.
log     DIR/train_log.jsonl, one JSON line per step (a resumed run first drops the rows from its restart step onwards, so no step appears twice).  The finetuning engines have no metrics ring, so each step's loss_acc is copied on the stream
        into a row of a small device ring and from there to pinned host memory; the row of step n - log_every is read while step n is being
        enqueued (the reference's copy_to_host_async, V:250-257), never with a per-step synchronise.  ms_per_step per log interval, from events;
        an interval ends at an epoch's end too, and the epoch's checkpoint and validation pass lie in none.
epoch   every device.iterations_per_loop steps (= one epoch): the reference-format checkpoint DIR/ckpt_<step> (no optimizer, V:262), the exact
        restart file DIR/restart_<step> (fp32 masters, both moments, the step, the bf16 anchor of the decay term), val_epoch on a forward-only
        model that reads the trained parameters, one line of DIR/val_log.jsonl and DIR/val_preds_<step>.jsonl.  A run that ends between two epochs
        writes the restart file alone.  The latest restart file of DIR is resumed from.
--gpus N without a launcher around it starts N ranks under torch.distributed.run as a CHILD process before this process touches the GPU.  The
        validation pass of a multi-rank run is rank 0's, over whole batches."""
import argparse
import copy
import json
import os
import sys

from .driver import IntervalTimer, JsonlLog, checkpoint_due, epoch_due, init_rank, new_event, self_launch, truncate_log

TASKS = {'vcr': dict(num_answers=4, lang_seq_len=144, train_size=212736), 'tvqa': dict(num_answers=5, lang_seq_len=256, train_size=122112, num_segments=7)}
RESTART_PREFIX = 'restart_'


def build_parser():
    ap = argparse.ArgumentParser(description='MERLOT Reserve finetuning (VCR, TVQA) on MI355X')
    ap.add_argument('task', choices=sorted(TASKS))
    ap.add_argument('pretrain_config_file', help="the config.yaml ('base' / 'large': the packaged ones)")
    ap.add_argument('ckpt', help="checkpoint to start from ('' = the initialised parameters)")
    ap.add_argument('-lr', type=float, default=5e-6)
    ap.add_argument('-ne', type=int, default=5, help='epochs')
    ap.add_argument('-output_grid_h', type=int, default=12)
    ap.add_argument('-output_grid_w', type=int, default=20)
    ap.add_argument('-output_name', default='')
    ap.add_argument('-output_dir', default='', help='overrides device.output_dir[/output_name] of the config')
    ap.add_argument('-val_batch_size', type=int, default=None, help='examples per validation batch (default: the training batch)')
    ap.add_argument('-scan_minibatch', action='store_true', help='the examples of a batch one at a time, gradients summed (finetune/optimization.py:125-146)')
    ap.add_argument('--gpus', type=int, default=1)
    ap.add_argument('--records-per-gpu', type=int, default=None, help='examples per GPU and step (default: 32 // gpus)')
    ap.add_argument('--train-size', type=int, default=None, help="examples per epoch (default: the task's TRAIN_SIZE)")
    ap.add_argument('--max-steps', type=int, default=None, help='stop at this step (default: optimizer.num_train_steps)')
    ap.add_argument('--data-dir', default='', metavar='DIR', help="the task's shards: DIR/train{:03d}of256.tfrecord and DIR/val{:03d}of008.tfrecord")
    ap.add_argument('--synthetic-shards', default='', metavar='DIR', help='train and validate on synthetic shards under DIR (written if absent)')
    ap.add_argument('--seed', type=int, default=0)
    return ap


def task_overrides(config, task, args):
    """V:96-121 / T:105-131 on a copy of the pretraining config: the task's data keys, the batch, the optimizer dictionary with its schedule of
    -ne epochs of TRAIN_SIZE // batch steps, iterations_per_loop = the steps of one epoch, the image grid."""
    t = TASKS[task]
    config = copy.deepcopy(config)
    data, dev = config['data'], config.setdefault('device', {})
    data.update(num_answers=t['num_answers'], random_scale_max=1.1, random_scale_min=1.0, lang_seq_len=t['lang_seq_len'])
    # the shards: <data dir>/train{:03d}of256.tfrecord and val{:03d}of008.tfrecord (V:96-97, V:215-216); the pretraining config's own train_fns name
    # pretraining shards and are dropped
    data.pop('train_fns', None), data.pop('val_fns', None)
    data.update(num_train_files=256, num_val_files=8)
    if getattr(args, 'data_dir', ''):
        data.update(train_fns=os.path.join(args.data_dir, 'train{:03d}of256.tfrecord'), val_fns=os.path.join(args.data_dir, 'val{:03d}of008.tfrecord'))
    if 'num_segments' in t:
        data['num_segments'] = t['num_segments']
    gpus = int(getattr(args, 'gpus', 1))
    rpg = getattr(args, 'records_per_gpu', None)
    dev.update(batch_size=32 if rpg is None else int(rpg) * gpus, prefetch_size=0, n_fns_per_cycle=256)
    train_size = t['train_size'] if getattr(args, 'train_size', None) is None else int(args.train_size)
    steps_per_epoch = train_size // dev['batch_size']
    if steps_per_epoch < 1:
        raise ValueError(f"an epoch of {train_size} examples holds no batch of {dev['batch_size']}")
    config['optimizer'] = {'beta_2': 0.98, 'eps': 1e-6, 'learning_rate': args.lr, 'num_train_steps': int(args.ne) * steps_per_epoch,
                           'num_warmup_steps': int(0.5 * steps_per_epoch), 'use_bfloat16_adam': True, 'weight_decay_rate': 0.1,
                           'do_bias_correction': True}
    dev['iterations_per_loop'] = steps_per_epoch
    config['model']['output_grid'] = [int(args.output_grid_h), int(args.output_grid_w)]
    return config


def driver_settings(config, args):
    """What the loop reads from the overridden config and the command line."""
    dev, opt = config['device'], config['optimizer']
    out = args.output_dir or os.path.join(dev.get('output_dir', ''), args.output_name)
    if not out:
        raise ValueError('no output directory: pass -output_dir or set device.output_dir')
    n = int(opt['num_train_steps'])
    end = n if args.max_steps is None else min(int(args.max_steps), n)
    gpus = int(args.gpus)
    if dev['batch_size'] % gpus:
        raise ValueError(f"device.batch_size {dev['batch_size']} is no multiple of --gpus {gpus}")
    return {'output_dir': out, 'epoch_every': int(dev['iterations_per_loop']), 'log_every': int(dev.get('commit_every_nsteps', 50)), 'end_step': end,
            'records_per_gpu': dev['batch_size'] // gpus, 'val_batch_size': int(args.val_batch_size or dev['batch_size'])}


class LaggedLog:
    """The lagged log of V:250-257: pushed(n) -- step n has been enqueued -- writes the row of step n - log_every, which has long left the
    device; flush(n_done) writes what is left at the end of the run.  read(step) returns the step's row (waiting, if at all, for that step only);
    the ring behind it must hold more than log_every rows."""

    def __init__(self, log_every, read, write, first_step=0):
        self.log_every, self.read, self.write, self.next = int(log_every), read, write, int(first_step)

    def pushed(self, n):
        while self.next <= n - self.log_every:
            self.write(self.read(self.next))
            self.next += 1

    def flush(self, n_done):
        while self.next < n_done:
            self.write(self.read(self.next))
            self.next += 1


class MetricsRing:
    """Each step's loss_acc, kept without a synchronise: push(step) copies the engine's accumulators on the current stream into row
    step % depth of a device ring and from there, asynchronously, into pinned host memory, with an event behind the copy; row(step) waits for
    that event alone.  A step whose metrics exist on the host already (the scanned step) is pushed as a dict."""

    def __init__(self, engine, depth):
        import torch
        self.eng, self.depth = engine, int(depth)
        n = engine.loss_acc.numel()
        self.dev = torch.zeros(depth, n, dtype=torch.float32, device=engine.dev)
        self.host = torch.zeros(depth, n, dtype=torch.float32, pin_memory=engine.dev.type == 'cuda')
        self.events, self.steps, self.infos, self.extra = [None] * depth, [None] * depth, [None] * depth, [None] * depth

    def push(self, step, info=None, **extra):
        import torch
        i = step % self.depth
        self.steps[i], self.infos[i], self.extra[i] = step, None if info is None else dict(info), extra
        if info is None:
            self.dev[i].copy_(self.eng.loss_acc)
            self.host[i].copy_(self.dev[i], non_blocking=True)
            self.events[i] = torch.cuda.Event()
            self.events[i].record()

    def row(self, step):
        i = step % self.depth
        if self.steps[i] != step:
            raise RuntimeError(f'metrics ring: row {i} holds step {self.steps[i]}, expected {step}')
        if self.infos[i] is not None:
            info = self.infos[i]
        else:
            self.events[i].synchronize()
            info = self.eng.info_from(self.host[i].tolist())
        return {'step': step, **info, **self.extra[i]}


def initial_params(model, ckpt):
    """The parameter tree the run starts from: None for CKPT = '' (the initialised parameters stay), else the checkpoint's `params`; a tree
    without `proj` (a pretraining checkpoint) gets the model's initialised one (V:183)."""
    if not ckpt:
        return None
    from .checkpoint import load_checkpoint
    params = load_checkpoint(ckpt)['params']
    if 'proj' not in params:
        params = dict(params, proj=model.params_store.master_tree()['proj'])
    return params


def model_and_batch(task, config, B, device, **kw):
    """(model, a synthetic batch of B examples to initialise it with)"""
    if task == 'vcr':
        from .finetune import MerlotReserveVCR, make_vcr_batch
        return MerlotReserveVCR.from_config(config, device=device, **kw), make_vcr_batch(config, B, seed=0, device=device)
    from .tvqa import MerlotReserveTVQA, make_tvqa_batch
    return MerlotReserveTVQA.from_config(config, device=device, **kw), make_tvqa_batch(config, B, seed=0, device=device)


def use_synthetic_shards(config, task, directory, seed):
    """Point the config at the synthetic shards under `directory`, writing them first if it holds none: two epochs' worth of training
    examples (at most 256) in two files, two validation files."""
    from . import finetune_records as FR
    marker = os.path.join(directory, 'shards.json')
    if not os.path.exists(marker):
        n = min(max(2 * config['device']['iterations_per_loop'] * config['device']['batch_size'], 8), 256)
        keys = FR.write_synthetic_shards(config, task, directory, seed=seed, train=(2, (n + 1) // 2), val=(2, 3))
        with open(marker + '.tmp', 'w') as f:
            json.dump(keys, f)
        os.replace(marker + '.tmp', marker)
    config['data'].update(json.load(open(marker)))
    return config


def validate(model, config, task, val_batch_size, workers=8):
    """val_epoch (V:208-239 / T:316-361) of the forward-only view of `model` over data.val_fns; returns (accuracies, rows)."""
    from . import finetune_eval as E
    from . import finetune_records as FR
    if getattr(model, '_val_view', None) is None:
        model._val_view = model.forward_only_view()
    val_config = copy.deepcopy(config)
    val_config['device']['batch_size'] = val_batch_size
    it = FR.finetune_val_input_fn_builder(val_config, task, workers=workers, processes=False, sep_tokens=FR.SEP_TOKEN_IDS)      # (threads: no step runs beside it)
    return E.val_epoch(model._val_view, it, task)


def main(argv=None):
    argv = sys.argv[1:] if argv is None else list(argv)
    args = build_parser().parse_args(argv)
    if args.gpus > 1 and 'WORLD_SIZE' not in os.environ:
        return self_launch('merlot_reserve_amd.finetune_train', argv, args.gpus)

    import torch
    from . import checkpoint
    from . import finetune as F
    from . import finetune_eval as E
    from . import finetune_records as FR
    from .config import load_config
    from .loader import PrefetchLoader

    task = args.task
    config = task_overrides(load_config(args.pretrain_config_file), task, args)
    st = driver_settings(config, args)
    dev, comm, rank, world = init_rank(args.gpus)
    B, out_dir, log_every = st['records_per_gpu'], st['output_dir'], st['log_every']
    os.makedirs(out_dir, exist_ok=True)
    if args.synthetic_shards:
        config = use_synthetic_shards(config, task, args.synthetic_shards, args.seed)
    if 'train_fns' not in config['data']:
        raise ValueError('no training shards: pass --data-dir DIR or --synthetic-shards DIR')

    model, dummy = model_and_batch(task, config, B, dev, rank=rank, world=world, comm=comm, seed=args.seed)
    model.init_from_dummy_batch(dummy)
    state, _tx = F.construct_finetuning_train_state(config['optimizer'], model, initial_params(model, args.ckpt))
    restart = checkpoint.latest_checkpoint(out_dir, prefix=RESTART_PREFIX)
    if restart is not None:
        checkpoint.load_checkpoint(restart, state=state)
        print(f'[rank {rank}] resumed from {restart} at step {state.step}', flush=True)
    start, end = state.step, st['end_step']
    if rank == 0:
        print(f'finetuning {task}: gpus={world} examples_per_gpu={B} steps {start} -> {end} of {config["optimizer"]["num_train_steps"]} '
              f'({st["epoch_every"]} per epoch)', flush=True)

    torch.set_num_threads(1)                                                  # (loader._stage: a spinning intra-op pool starves the runtime's helper threads)
    workers = max(0, min(FR.MAX_WORKERS // world - 2, 14))
    reader = FR.finetune_input_fn_builder(config, task, rank=rank, world=world, seed=args.seed, workers=workers, sep_tokens=FR.SEP_TOKEN_IDS,
                                          skip_batches=start)
    feed = PrefetchLoader((dict(batch, _ids=ids) for ids, batch in reader), dev, depth=2, dtype=torch.bfloat16 if config['model'].get('use_bfloat16', True)
                          else torch.float32, keys=FR.FLOAT_KEYS[task]) if start < end else iter(())

    eng = model.engine
    ring = MetricsRing(eng, log_every + 2)
    if rank == 0:                                                             # rows an interrupted run wrote past its last restart file are run again
        truncate_log(os.path.join(out_dir, 'train_log.jsonl'), lambda row: row['step'] < start)
        truncate_log(os.path.join(out_dir, 'val_log.jsonl'), lambda row: row['step'] <= start)
    log = JsonlLog(os.path.join(out_dir, 'train_log.jsonl'), rank)
    timer = IntervalTimer(start, new_event, world * B, 'examples_per_sec', last_row_only=True)
    lagged = LaggedLog(log_every, ring.row, lambda row: log.write(dict(row, **timer.of(row['step']))), first_step=start)

    def end_of_epoch(step):
        if rank != 0:
            return
        fn = checkpoint.save_checkpoint(state, out_dir, no_optimizer=True)                                      # the reference's file (V:262)
        acc, rows = validate(model, config, task, st['val_batch_size'])
        E.write_predictions(rows, os.path.join(out_dir, f'val_preds_{step}.jsonl'))
        with open(os.path.join(out_dir, 'val_log.jsonl'), 'a') as f:
            f.write(json.dumps({'step': step, **acc, 'num_examples': len(rows)}) + '\n')
        print(f'step {step}: saved {fn}; validation {acc}', flush=True)

    def save_restart(step):
        fn = checkpoint.save_checkpoint(state, out_dir, rank=rank, keep_fp32=True, prefix=RESTART_PREFIX, keep=1)
        if rank == 0:
            print(f'saved {fn}', flush=True)

    use_graph = not args.scan_minibatch and (comm is None or getattr(comm, 'capturable', False))
    if task == 'vcr':
        graph_cls = F.VCRGraphStep
    else:
        from .tvqa import TVQAGraphStep as graph_cls
    graph_step = None
    step = start
    try:
        for batch in feed:
            sched = state._schedule()
            if use_graph and graph_step is not None:
                graph_step(batch)
                ring.push(step, lr_scale=sched)
            elif use_graph:
                graph_step = graph_cls(state, batch)                       # one eager step, then the capture
                ring.push(step, lr_scale=sched)
            else:
                _s, info = F.finetune_train_step(state, batch, scan_minibatch=args.scan_minibatch)
                ring.push(step, info=info, lr_scale=sched)
            step += 1
            assert state.step == step
            lagged.pushed(step - 1)
            if (step - start) % log_every == 0 or step == end:
                timer.mark(step)
            if epoch_due(step, st['epoch_every']):
                timer.mark(step)                                           # the epoch's checkpoint and validation are in no interval
                end_of_epoch(step)
                timer.resume(step)
            if checkpoint_due(step, st['epoch_every'], end):
                save_restart(step)
            if step >= end:
                break
        timer.mark(step)
        torch.cuda.synchronize()
        lagged.flush(step)
    finally:
        reader.close()
        log.close()
    if rank == 0:
        print(f'ran {step - start} steps to step {state.step}; log, checkpoints and predictions in {out_dir}', flush=True)
    if comm is not None:
        comm.close()
    return 0


if __name__ == '__main__':
    sys.exit(main())
