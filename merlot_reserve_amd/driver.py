"""What the training loops (train.py, finetune_train.py) share: the `--gpus N` child launch, the rank / device / communicator set-up, the
checkpoint cadence, the JSONL log files and the interval timer."""
import json
import os
import sys


def launch_command(module, argv, gpus, port):
    """The child command of `--gpus N` without a launcher: N fresh ranks of `module` under torch.distributed.run."""
    return [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', f'--nproc-per-node={gpus}', '--master-addr', '127.0.0.1',
            '--master-port', str(port), '-m', module] + list(argv)


def self_launch(module, argv, gpus):
    """Runs the ranks as a CHILD process (before this process touches the GPU; its program is never replaced); returns their exit status."""
    import socket
    import subprocess
    with socket.socket() as sk:
        sk.bind(('127.0.0.1', 0))
        port = sk.getsockname()[1]
    env = dict(os.environ)
    env.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')
    return subprocess.run(launch_command(module, argv, gpus, port), env=env).returncode


def init_rank(gpus):
    """(device, communicator or None, rank, world) of this process from the launcher's environment."""
    import torch
    world, rank, local_rank = (int(os.environ.get(k, d)) for k, d in (('WORLD_SIZE', '1'), ('RANK', '0'), ('LOCAL_RANK', '0')))
    assert world == gpus, f'--gpus {gpus} but WORLD_SIZE={world}'
    torch.cuda.set_device(local_rank)
    dev = torch.device('cuda', local_rank)
    comm = None
    if world > 1:
        import torch.distributed as dist
        from .dist import NativeComm
        dist.init_process_group('gloo', rank=rank, world_size=world)          # control plane only: rendezvous + the RCCL id
        comm = NativeComm.from_torch_distributed(dev)
    return dev, comm, rank, world


def checkpoint_due(step, ckpt_every, end_step):
    """After `step` steps in all: every ckpt_every steps of the RUN'S step count (a resumed run keeps the cadence) and at the end."""
    return step % ckpt_every == 0 or step == end_step


def epoch_due(step, epoch_every):
    """After `step` steps in all: the end of an epoch (V:259) -- checkpoint, restart file, validation."""
    return step > 0 and step % epoch_every == 0


def new_event():
    """A timing event recorded on the current stream."""
    import torch
    e = torch.cuda.Event(enable_timing=True)
    e.record()
    return e


class JsonlLog:
    """One JSON line per write, appended and flushed; every rank but 0 writes nothing."""

    def __init__(self, path, rank=0):
        self.f = open(path, 'a') if rank == 0 else None

    def write(self, rec):
        if self.f is not None:
            self.f.write(json.dumps(rec) + '\n')
            self.f.flush()

    def close(self):
        if self.f is not None:
            self.f.close()


def truncate_log(path, keep):
    """A resumed run starts at its restart file's step, which may lie before the last row an interrupted run wrote: drop the rows (JSON lines)
    for which keep(row) is false, so that no step or epoch is logged twice.  Returns the number of rows dropped."""
    if not os.path.exists(path):
        return 0
    lines = [line for line in open(path) if line.strip()]
    kept = [line for line in lines if keep(json.loads(line))]
    if len(kept) != len(lines):
        with open(path + '.tmp', 'w') as f:
            f.writelines(kept)
        os.replace(path + '.tmp', path)
    return len(lines) - len(kept)


class IntervalTimer:
    """ms per step of each log interval from device events recorded at its two ends.  of(step) answers for every step of a closed interval, or
    (last_row_only) for its LAST step alone: one figure per interval; it waits for the interval's closing event, which lies behind the copy
    that brought the step's row.  Work that is no step (an epoch's checkpoint and validation pass) is kept out: mark(step) before it closes
    the running interval, resume(step) after it opens the next one with a fresh event."""

    def __init__(self, start_step, new_event, units_per_step, rate_key, last_row_only=False):
        self.new_event, self.units, self.rate_key, self.last_row_only = new_event, units_per_step, rate_key, last_row_only
        self.intervals = []                                # (first step, steps done at its end, opening event, closing event)
        self.open = (start_step, new_event())
        self.done = {}

    def mark(self, step):
        lo, e0 = self.open
        if step > lo:
            e1 = self.new_event()
            self.intervals.append((lo, step, e0, e1))
            self.open = (step, e1)

    def resume(self, step):
        self.mark(step)
        self.open = (step, self.new_event())

    def of(self, step):
        for lo, hi, e0, e1 in self.intervals:
            if hi == step + 1 if self.last_row_only else lo <= step < hi:
                if hi not in self.done:
                    e1.synchronize()
                    ms = e0.elapsed_time(e1) / (hi - lo)
                    self.done[hi] = {'ms_per_step': ms, self.rate_key: self.units / (ms / 1e3) if ms > 0 else None}
                return self.done[hi]
        return {}
