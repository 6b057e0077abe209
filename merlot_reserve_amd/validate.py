"""Held-out loss of the checkpoints of a run: the counterpart of pretrain/validate.py:105-149.

    python -m merlot_reserve_amd.validate CONFIG.yaml -output_dir DIR [-batch_size B] [-max_num_megabatch N] [-step S] [--synthetic] [--seed S]

For every checkpoint in DIR (or the one of -step) and for the `val` and `train` shards (the reference's file pattern, :101-102; --synthetic:
synthetic batches): num_accumulations = device.batch_size // B forward passes of B records each, the embeddings of every pass kept, and the loss
of the CONCATENATED batch (:136-138) -- every query against the keys of all passes.  The engine's loss takes a rank-major E_all [world, R, H],
so the megabatch loss is the mean over r of the loss of "rank" r among num_accumulations (times the communicator's world size when there is
one).  The engine is the forward-only program (PretrainEngine(train=False)): the loss stops after the LSE, no gradient is formed.
One JSON line per (checkpoint, dataset): the averaged loss_info, nbatch, dset, ckpt, nstep (:144-149)."""
import argparse
import glob
import json
import os
import sys


def build_parser():
    ap = argparse.ArgumentParser(description='MERLOT Reserve held-out loss on MI355X')
    ap.add_argument('config_file')
    ap.add_argument('-output_dir', dest='output_dir', default='', help='the directory of ckpt_<step> files')
    ap.add_argument('-batch_size', dest='batch_size', type=int, default=32, help='records per forward pass')
    ap.add_argument('-max_num_megabatch', dest='max_num_megabatch', type=int, default=4)
    ap.add_argument('-step', dest='step', type=int, default=None, help='only the checkpoint of this step')
    ap.add_argument('--synthetic', action='store_true')
    ap.add_argument('--seed', type=int, default=0)
    return ap


def num_accumulations(config, batch_size):
    orig = int(config['device']['batch_size'])
    if orig % batch_size != 0:
        raise ValueError(f'device.batch_size {orig} is not a multiple of -batch_size {batch_size}')
    return orig // batch_size


def checkpoint_files(output_dir, step=None, prefix='ckpt_'):
    if step is not None:
        return [os.path.join(output_dir, f'{prefix}{step}')]
    fns = [f for f in glob.glob(os.path.join(output_dir, prefix + '*')) if f.rsplit('_', 1)[-1].isdigit()]
    return sorted(fns, key=lambda f: int(f.rsplit('_', 1)[-1]))


def dataset_files(config, dset):
    """pretrain/validate.py:101-102: every `val*` shard beside the training shards, and as many training shards."""
    train_fns = config['data']['train_fns']
    val = sorted(glob.glob(train_fns.split('train{:05d}')[0] + 'val*'))
    return val if dset == 'val' else [train_fns.format(i) for i in range(len(val))]


def mean_info(infos):
    return {k: sum(i[k] for i in infos) / len(infos) for k in infos[0]}


class MegabatchLoss:
    """Forward passes of B records each; after num_accumulations of them, the loss of the concatenated batch."""

    def __init__(self, config, B, params, device, num_accumulations, comm=None):
        import torch
        from .engine import PretrainEngine
        self.A, self.comm = num_accumulations, comm
        self.W, self.r0 = (comm.world, comm.rank) if comm is not None else (1, 0)
        self.eng = eng = PretrainEngine(config, B, params, device, rank=0, world=self.A * self.W, train=False)
        z = lambda n: torch.zeros(n, eng.R, eng.d.H, dtype=eng.dtype, device=eng.dev)
        self.E_loc = z(self.A)
        self.E_all = self.E_loc if comm is None else z(self.A * self.W)       # rank-major: real rank, then pass
        self.plans = []

    def add_pass(self, batch, draws=None):
        """One forward pass; its embeddings are kept.  True when the megabatch is complete."""
        eng = self.eng
        eng.forward(batch, draws=draws)
        self.E_loc[len(self.plans)].copy_(eng.E)
        self.plans.append(eng.plan)
        return len(self.plans) == self.A

    def loss_info(self):
        """loss_info of the megabatch: the mean over the passes r of the loss of rank r among all passes (a COLLECTIVE with a comm)."""
        import torch
        assert len(self.plans) == self.A
        eng = self.eng
        if self.comm is not None:
            self.comm.gather_embeddings(self.E_loc.view(self.A * eng.R, eng.d.H), self.E_all)
        infos = []
        for a, plan in enumerate(self.plans):
            eng.rank = self.r0 * self.A + a
            eng.E.copy_(self.E_loc[a])
            eng.set_plan(plan)
            eng.loss_and_grad_outputs(self.E_all, self.E_all)       # (forward-only: the gradient argument is never written)
            infos.append(eng.loss_info())
        eng.rank = 0
        self.plans = []
        info = mean_info(infos)
        if self.comm is not None and self.W > 1:
            keys = sorted(info)
            t = torch.tensor([info[k] for k in keys], dtype=torch.float32, device=eng.dev)
            self.comm.allreduce_mean_f32(t)
            info = dict(zip(keys, t.tolist()))
        return info


def validate_params(mb, batches, max_num_megabatch):
    """batches: iterable of device batches of B records (a '_draws' entry, if present, holds the pass's draws).  Returns (averaged loss_info, nbatch)."""
    agg = []
    for batch in batches:
        if mb.add_pass(batch, batch.get('_draws')):
            agg.append(mb.loss_info())
        if len(agg) == max_num_megabatch:
            break
    if not agg:
        raise ValueError(f'not enough data for one megabatch of {mb.A} passes')
    return mean_info(agg), len(agg)


def main(argv=None):
    args = build_parser().parse_args(sys.argv[1:] if argv is None else list(argv))
    if not args.output_dir:
        raise ValueError('must provide -output_dir')
    import torch
    from . import checkpoint, records
    from .config import load_config
    from .loader import PrefetchLoader
    from .params import ParamStore
    from .train import synthetic_batches

    config = load_config(args.config_file)
    config['device']['output_dir'] = args.output_dir
    A = num_accumulations(config, args.batch_size)
    config['device']['batch_size'] = args.batch_size
    config['data']['do_random_scale'] = False
    dev = torch.device('cuda', 0)
    torch.cuda.set_device(dev)
    store = ParamStore(config, dev, seed=0, with_optimizer=False)
    mb = MegabatchLoss(config, args.batch_size, store, dev, A)
    npass = A * args.max_num_megabatch
    results = []
    for fn in checkpoint_files(args.output_dir, args.step):
        sd = checkpoint.load_checkpoint(fn)
        store.load_tree(sd['params'])
        for dset in ('val', 'train'):
            if args.synthetic:        # train: the batches of the first training steps of --seed; val: seeds no training step uses
                source = synthetic_batches(config, args.batch_size, args.seed + (0 if dset == 'train' else 1 << 30), 0, npass)
            else:
                source = records.make_dataset(config, dataset_files(config, dset), args.batch_size, is_training=False, seed=args.seed)
            mb.plans = []
            info, nbatch = validate_params(mb, PrefetchLoader(source, dev, depth=2), args.max_num_megabatch)
            torch.cuda.synchronize()
            info.update(nbatch=nbatch, dset=dset, ckpt=fn, nstep=int(sd['step']))
            results.append(info)
            print(json.dumps(info), flush=True)
    return 0


if __name__ == '__main__':
    sys.exit(main())
