"""What the zero-shot head costs on one MI355X, and what caching the label table and batching the videos save.

  1  zeroshot.score_topk (k = 10, two launches, no [Q, L] logits in HBM) against torch's matmul + log_softmax + topk on the same tensors,
     Q in {1, 64, 4096} x L in {1000, 3806} at H = 768 and 1024, fp32 and bf16.  torch.topk does not promise the lower index among equal
     values, so the torch side is the faster-or-slower yardstick only, not a replacement.
  2  one encoding of a 3806-option table (embed_text_spans_only, chunks of 1024) against one embed_video of 8 segments: what
     zero_shot_eval_ek100.py:146 pays per video for re-encoding the table.
  3  ZeroShotClassifier.classify of 64 videos (8 segments, grid 18 x 32, base, fp32, random weights) at batch_size 1 against batch_size 8.

Device events around blocks of calls after a warm-up of every shape; the two sides of a comparison take turns, block by block, in one process;
the median block is reported with the spread (min .. max).  Inputs are resident on the device except in 3, where the videos start in host
memory as preprocess_video leaves them.
python scripts/zeroshot_cost.py [--out FILE]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from merlot_reserve_amd import modeling as M, preprocess as P, zeroshot

GRID = (18, 32)


def alternate(sides, calls, rounds, warm=3):
    """sides: {name: fn}.  -> {name: (median, min, max) ms per call} over `rounds` blocks of `calls` calls, the sides taking turns."""
    for fn in sides.values():
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    ms = {name: [] for name in sides}
    for _ in range(rounds):
        for name, fn in sides.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(calls):
                fn()
            t1.record()
            t1.synchronize()
            ms[name].append(t0.elapsed_time(t1) / calls)
    return {name: (float(np.median(v)), min(v), max(v)) for name, v in ms.items()}


def torch_head(q, lab, k, scale=100.0):
    logits = scale * torch.matmul(q, lab.t()).float()
    lp = torch.log_softmax(logits, -1)
    return torch.topk(lp, k, dim=-1)


def main():
    assert torch.cuda.is_available(), 'needs the GPU: there is no CPU figure for the kernels'
    dev = torch.device('cuda:0')
    g = torch.Generator(device='cpu').manual_seed(0)
    lines = [f'zero-shot head, device {torch.cuda.get_device_name(0)}; ms per call, median of the blocks (min .. max); k = 10, scale 100']
    lines.append(f'{"Q":>5s} {"L":>5s} {"H":>5s} {"dtype":>5s}   {"score_topk":>28s}   {"matmul + log_softmax + topk":>28s}   ratio')
    for H in (768, 1024):
        for dt, name in ((torch.float32, 'fp32'), (torch.bfloat16, 'bf16')):
            for L in (1000, 3806):
                lab = torch.nn.functional.normalize(torch.randn(L, H, generator=g), dim=-1).to(dev).to(dt)
                for Q in (1, 64, 4096):
                    q = torch.nn.functional.normalize(torch.randn(Q, H, generator=g), dim=-1).to(dev).to(dt)
                    calls, rounds = (200, 15) if Q < 4096 else (20, 15)
                    r = alternate({'ours': lambda: zeroshot.score_topk(q, lab, 10), 'torch': lambda: torch_head(q, lab, 10)}, calls, rounds)
                    fmt = lambda t: f'{t[0]:9.4f} ({t[1]:.4f} .. {t[2]:.4f})'
                    lines.append(f'{Q:5d} {L:5d} {H:5d} {name:>5s}   {fmt(r["ours"]):>28s}   {fmt(r["torch"]):>28s}   {r["ours"][0] / r["torch"][0]:5.2f}')
    print('\n'.join(lines), flush=True)

    pm = M.PretrainedMerlotReserve.from_random('base', image_grid_size=GRID, device=dev)
    rng = np.random.default_rng(0)
    L = 3806
    option_ids = np.zeros((L, 15), dtype=np.int64)
    for row in option_ids:
        m = int(rng.integers(1, 8))
        row[:m] = rng.integers(10, 32768, size=m)

    def video(seed):
        r = np.random.default_rng(seed)
        segs = []
        for i in range(8):
            spec = (r.random((3, 60, 65)) * 5).astype(np.float32)
            spec[..., 64] = 1.0
            segs.append({'patches': r.random((GRID[0] * GRID[1], 768)).astype(np.float32), 'spectrogram': spec, 'use_text_as_input': i == 0})
        segs[0]['text'] = r.integers(10, 32768, size=12).tolist() + [P.MASK]
        return P.preprocess_video(segs, GRID)
    distinct = [video(s) for s in range(8)]

    def encode_table():
        return torch.cat([pm.embed_text_spans_only(option_ids[i:i + 1024]) for i in range(0, L, 1024)], 0)
    r = alternate({'table': encode_table, 'video': lambda: pm.embed_video(**distinct[0])}, 5, 9, warm=2)
    out = ['', 'base, fp32, random weights, grid 18 x 32; ms per call, median of the blocks (min .. max)',
           f'encode the 3806-option table (4 encoder calls)          {r["table"][0]:9.3f} ({r["table"][1]:.3f} .. {r["table"][2]:.3f})',
           f'embed_video of 8 segments (inputs in host memory)       {r["video"][0]:9.3f} ({r["video"][1]:.3f} .. {r["video"][2]:.3f})',
           f're-encoding the table per video would multiply the cost of a video by {1 + r["table"][0] / r["video"][0]:.2f}']
    clf = zeroshot.ZeroShotClassifier(pm, option_ids=option_ids, groups={'verb': (np.arange(L) % 97).tolist(), 'noun': (np.arange(L) % 300).tolist()})
    videos = [distinct[i % 8] for i in range(64)]
    r = alternate({'bs1': lambda: clf.classify(videos, k=5, batch_size=1), 'bs8': lambda: clf.classify(videos, k=5, batch_size=8)}, 1, 7, warm=1)
    out += [f'classify 64 videos (3806 options, 2 group maps), batch_size 1   {r["bs1"][0]:9.2f} ({r["bs1"][1]:.2f} .. {r["bs1"][2]:.2f})  = {r["bs1"][0] / 64:.2f} per video',
            f'classify 64 videos (3806 options, 2 group maps), batch_size 8   {r["bs8"][0]:9.2f} ({r["bs8"][1]:.2f} .. {r["bs8"][2]:.2f})  = {r["bs8"][0] / 64:.2f} per video']
    q8 = torch.nn.functional.normalize(torch.randn(8, 768, generator=g), dim=-1).to(dev)
    gdev = torch.from_numpy((np.arange(L) % 97).astype(np.int32)).to(dev)
    r = alternate({'plain': lambda: zeroshot.score_topk(q8, clf.label_space, 5), 'groups': lambda: zeroshot.score_topk(q8, clf.label_space, 5, groups=gdev, num_groups=97)}, 200, 9)
    out.append(f'score_topk of 8 queries x 3806 labels: {r["plain"][0]:.4f} without, {r["groups"][0]:.4f} with a group map of 97')
    print('\n'.join(out), flush=True)
    if '--out' in sys.argv:
        with open(sys.argv[sys.argv.index('--out') + 1], 'w') as f:
            f.write('\n'.join(lines + out) + '\n')


if __name__ == '__main__':
    main()
