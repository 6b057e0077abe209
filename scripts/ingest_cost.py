"""What media ingest costs (libmreserve_ingest.so) beside the CPU steps it replaces: one clip of 8 segments -- 8 uint8 1080p frames, 40 s of
48 kHz stereo int16 audio.

  bounds     mri_content_bounds over the 8 frames: the bare launch with the frames on the device (200 launches between two synchronises, per
             launch), ingest.content_bounds as called (bounds initialised, launched, 16 bytes copied back), and with the copy of the frames from
             host memory included
  resample   mri_resample_mono on the 40 s: the same three ways
  segments   the whole preprocess.segments_from_pcm call (resample, normalise, cut, log-mel, bounds, crop), inputs on the host / on the device
  CPU        numpy's frames.max(axis=(0, -1)) (one thread: numpy does not thread this reduction) and torch.amax on 16 threads;
             scipy.signal.resample_poly of the downmix if scipy is there -- otherwise there is no CPU resampler on the machine to compare with

Wall clock around a device synchronise, after warm-up, the median of the repeats; the spread (min .. max) is printed with it.
python scripts/ingest_cost.py [--out FILE]"""
import os
import sys
import time

os.environ.setdefault('OMP_NUM_THREADS', '16')
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from merlot_reserve_amd import _ingest_lib, ingest, preprocess as P

torch.set_num_threads(min(16, torch.get_num_threads()))
NSEG, SR_IN, SECONDS = 8, 48000, 40


def timed(fn, sync, reps, warm=2, per=1):
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
        ts.append((time.perf_counter() - t0) * 1e3 / per)
    ts.sort()
    return ts[len(ts) // 2], ts[0], ts[-1]


def main():
    assert torch.cuda.is_available(), 'needs the GPU: there is no CPU figure for the kernels'
    dev = torch.device('cuda:0')
    rng = np.random.default_rng(0)
    frames = np.zeros((NSEG, 1080, 1920, 3), dtype=np.uint8)
    frames[:, 138:942] = rng.integers(0, 256, (NSEG, 804, 1920, 3), dtype=np.uint8)             # a 2.39 : 1 picture in a 16 : 9 frame
    pcm = (rng.standard_normal((SECONDS * SR_IN, 2)) * 6000).astype(np.int16)                   # interleaved, as `wave` gives it
    lines = [f'media ingest, one clip: {NSEG} uint8 1080 x 1920 frames ({frames.nbytes / 1e6:.1f} MB), {SECONDS} s of {SR_IN} Hz stereo int16 ({pcm.nbytes / 1e6:.2f} MB)',
             f'device {torch.cuda.get_device_name(0)}; host threads capped at {torch.get_num_threads()}; ms, median (min .. max)']

    def row(name, r):
        lines.append(f'{name:<72s} {r[0]:9.4f}  ({r[1]:.4f} .. {r[2]:.4f})')

    lib = _ingest_lib.load()
    st = torch.cuda.current_stream(dev).cuda_stream
    dframes, dpcm = torch.from_numpy(frames).to(dev), torch.from_numpy(pcm).to(dev)
    init = torch.tensor([1080, -1, 1920, -1], dtype=torch.int32, device=dev)
    bounds = init.clone()

    def bounds_launches(k=200):
        for _ in range(k):
            _ingest_lib.check(lib.mri_content_bounds(dframes.data_ptr(), NSEG, 1080, 1920, 32, bounds.data_ptr(), st), 'mri_content_bounds')
    row('mri_content_bounds, frames on the device, per launch of 200', timed(bounds_launches, True, 20, per=200))
    lines.append(f'    {frames.nbytes / 1e6:.1f} MB read: {frames.nbytes / 1e6 / 6.3e3 * 1e3:.1f} us at 6.3 TB/s; after the first of these launches the bounds are final and the atomics are skipped --')
    lines.append('    the call below starts from {H, -1, W, -1} every time')
    row('ingest.content_bounds, frames on the device (with the 16-byte copy back)', timed(lambda: ingest.content_bounds(dframes, 32), True, 50, warm=3))
    row('ingest.content_bounds incl. copy of the frames from the host', timed(lambda: ingest.content_bounds(frames, 32, device=dev), True, 10, warm=2))
    assert ingest.content_bounds(dframes, 32) == (138, 941, 0, 1919)

    L, M, K, taps = ingest.resample_table(SR_IN)
    dtaps = torch.from_numpy(taps).to(dev)
    n_out = lib.mri_resample_len(pcm.shape[0], L, M)
    y = torch.empty(n_out, dtype=torch.float32, device=dev)
    peak = torch.zeros(1, dtype=torch.int32, device=dev)

    def resample_launches(k=200):
        for _ in range(k):
            _ingest_lib.check(lib.mri_resample_mono(dpcm.data_ptr(), _ingest_lib.DT_S16, 2, pcm.shape[0], 1, 2, dtaps.data_ptr(), L, M, K, y.data_ptr(),
                                                    peak.data_ptr(), st), 'mri_resample_mono')
    row(f'mri_resample_mono, PCM on the device, per launch of 200 ({n_out} outputs x {K} taps)', timed(resample_launches, True, 20, per=200))
    row('ingest.resample_mono, PCM on the device', timed(lambda: ingest.resample_mono(dpcm, SR_IN), True, 50, warm=3))
    row('ingest.resample_mono incl. copy of the PCM from the host', timed(lambda: ingest.resample_mono(pcm, SR_IN, device=dev), True, 20, warm=3))

    row('segments_from_pcm(device=...), frames and PCM on the host', timed(lambda: P.segments_from_pcm(frames, pcm, SR_IN, device=dev), True, 10, warm=2))
    row('segments_from_pcm(device=...), frames and PCM on the device', timed(lambda: P.segments_from_pcm(dframes, dpcm, SR_IN, device=dev), True, 20, warm=3))

    row('CPU numpy frames.max(axis=(0, -1)) >= 32 (one thread)', timed(lambda: frames.max(axis=(0, -1)) >= 32, False, 5, warm=1))
    tframes = torch.from_numpy(frames)
    row(f'CPU torch.amax(frames, (0, 3)) >= 32 ({torch.get_num_threads()} threads)', timed(lambda: torch.amax(tframes, (0, 3)) >= 32, False, 5, warm=1))
    try:
        import scipy.signal
    except ImportError:
        lines.append('scipy is not installed: there is no CPU resampler on this machine to compare with')
    else:
        mono = pcm.astype(np.float32).mean(1)
        row(f'CPU scipy.signal.resample_poly(mono, {L}, {M}) (its default Kaiser 5.0 filter, float32)', timed(lambda: scipy.signal.resample_poly(mono, L, M), False, 5, warm=1))
    text = '\n'.join(lines)
    print(text)
    if '--out' in sys.argv:
        with open(sys.argv[sys.argv.index('--out') + 1], 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
