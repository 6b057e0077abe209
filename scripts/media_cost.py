"""What the media front end costs beside the model it feeds: 8 segments of one clip (1080p uint8 frames to grid 18x32, 5 s of 22050 Hz audio each).

  CPU      records.resize_and_pad (PIL, float planes) + patchify per frame, and a scipy / numpy log-mel per segment, capped at 16 threads
  GPU      media.frames_to_patches and media.logmel (one launch each for the 8 segments), inputs already on the device; and with the copy
           of the uint8 frames / float32 waveforms from host memory included
  model    embed_video of the same 8 segments (base, fp32, random weights)

Wall clock around a device synchronise, after warm-up, the median of the repeats; the spread (min .. max) is printed with it.
python scripts/media_cost.py [--out FILE]"""
import os
import sys
import time

os.environ.setdefault('OMP_NUM_THREADS', '16')
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import scipy.signal
import torch

from merlot_reserve_amd import media, modeling as M, preprocess as P, records

torch.set_num_threads(min(16, torch.get_num_threads()))
GRID, NSEG, L = (18, 32), 8, 110250


def cpu_logmel(w, fb, win):
    """float32 in, float64 arithmetic: reflect pad, frame, window, rfft, mel, log -- the reference's librosa call, restated"""
    p = np.pad(w.astype(np.float64), 768, mode='reflect')
    T = 1 + len(w) // 588
    frames = np.lib.stride_tricks.as_strided(p, (T, 1536), (588 * p.strides[0], p.strides[0])) * win
    mel = (np.abs(np.fft.rfft(frames, axis=-1)) ** 2) @ fb.T
    return np.log(mel + 0.1) - np.log(0.1)


def timed(fn, sync, reps, warm=2):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        if sync:
            torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        if sync:
            torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    ts.sort()
    return ts[len(ts) // 2], ts[0], ts[-1]


def main():
    assert torch.cuda.is_available(), 'needs the GPU: there is no CPU figure for the kernels'
    dev = torch.device('cuda:0')
    rng = np.random.default_rng(0)
    frames = rng.integers(0, 256, (NSEG, 1080, 1920, 3), dtype=np.uint8)
    waves = (rng.standard_normal((NSEG, L)) * 0.3).astype(np.float32)
    fb, win = media.mel_filterbank(), scipy.signal.windows.hann(1536)
    lines = [f'media front end, {NSEG} segments: uint8 1080 x 1920 frames -> grid {GRID[0]} x {GRID[1]}, {L} samples of audio each',
             f'device {torch.cuda.get_device_name(0)}; host threads capped at {torch.get_num_threads()}; ms per 8 segments, median (min .. max)']

    def row(name, r):
        lines.append(f'{name:<58s} {r[0]:9.3f}  ({r[1]:.3f} .. {r[2]:.3f})')

    def cpu_frames():
        return [P.patchify(records.resize_and_pad(f.astype(np.float32) / np.float32(255.0), (16 * GRID[0], 16 * GRID[1]), None, do_random_scale=False,
                                                  do_flip_if_vertical=False, resize_method='bilinear')[0], GRID) for f in frames]
    row('CPU resize_and_pad + patchify (PIL, float planes)', timed(cpu_frames, False, 5, warm=1))
    row('CPU log-mel (numpy rfft, float64)', timed(lambda: [cpu_logmel(w, fb, win) for w in waves], False, 10))
    dframes, dwaves = torch.from_numpy(frames).to(dev), torch.from_numpy(waves).to(dev)
    po = torch.empty((NSEG, GRID[0] * GRID[1], 768), dtype=torch.float32, device=dev)
    lo = torch.empty((NSEG, 188, 65), dtype=torch.float32, device=dev)
    row('GPU frames_to_patches, frames on the device', timed(lambda: media.frames_to_patches(dframes, GRID, out=po), True, 50, warm=3))
    row('GPU logmel, waveforms on the device', timed(lambda: media.logmel(dwaves, out=lo), True, 50, warm=3))
    row('GPU frames_to_patches incl. copy of 49.8 MB of frames', timed(lambda: media.frames_to_patches(frames, GRID, out=po, device=dev), True, 20, warm=3))
    row('GPU logmel incl. copy of 3.5 MB of waveforms', timed(lambda: media.logmel(waves, out=lo, device=dev), True, 20, warm=3))
    # the kernels against the CPU paths they replace, on these inputs
    ref = np.stack(cpu_frames())
    lines.append(f'max |GPU - CPU| patches {np.abs(po.cpu().numpy() - ref).max():.3g}, log-mel '
                 f'{np.abs(lo.cpu().numpy()[..., :64] - np.stack([cpu_logmel(w, fb, win) for w in waves])).max():.3g}')
    pm = M.PretrainedMerlotReserve.from_random('base', image_grid_size=GRID, device=dev)
    segs = [{'frame': dframes[i], 'waveform': dwaves[i], 'use_text_as_input': False} for i in range(NSEG)]
    segs[0].update(text=rng.integers(10, 32768, size=12).tolist() + [3], use_text_as_input=True)
    row('preprocess_video(device=...) from device frames / waveforms', timed(lambda: P.preprocess_video(segs, GRID, device=dev), True, 20, warm=3))
    v = P.preprocess_video(segs, GRID, device=dev)
    row('embed_video base fp32', timed(lambda: pm.embed_video(**v), True, 10, warm=3))
    text = '\n'.join(lines)
    print(text)
    if '--out' in sys.argv:
        with open(sys.argv[sys.argv.index('--out') + 1], 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
