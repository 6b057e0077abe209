"""Media ingest on the GPU (libmreserve_ingest.so): the resampler against the float64 restatement of tests/ingest_refs.py within a derived bound,
its prefix property and peak bit for bit, the black-bar bounds as exact integers, trim_black_bars as a view, and the plumbing through
segments_from_pcm, preprocess_video and the zeroshot_eval command."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from ingest_refs import bar_cases, ref_bounds, ref_detect_black_bars, ref_resample
from media_refs import ref_filterbank, ref_logmel

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RATES = (44100, 48000, 16000, 96000, 44101)      # 44101: L = 22050, a table of 22050 x 66 that no LDS holds
LENGTHS = (7, 5000, 70001)                       # shorter than the filter; one or two blocks; many blocks with a ragged tail
LOGMEL_BOUND = 1e-4                              # tests/test_media_gpu.py


def resample_bound(sr, max_abs):
    """|y - ref| <= (K + 3) 2^-24 max_p sum_j |taps[p, j]| max|x|: K fused multiply-adds, the downmix division and the table's own rounding, each
    at most half an ulp of a partial result that sum_j |taps| max|x| bounds."""
    from merlot_reserve_amd import ingest
    L, M, K, taps = ingest.resample_table(sr)
    return (K + 3) * 2.0 ** -24 * float(np.abs(taps.astype(np.float64)).sum(1).max()) * max_abs


@functools.lru_cache(maxsize=None)
def _pcm(N):
    """(int16 [3, N], float32 [3, N] in [-1, 1]), read-only"""
    rng = np.random.default_rng(N)
    s16 = rng.integers(-32768, 32768, (3, N), dtype=np.int16)
    f32 = rng.uniform(-1.0, 1.0, (3, N)).astype(np.float32)
    s16.setflags(write=False)
    f32.setflags(write=False)
    return s16, f32


@functools.lru_cache(maxsize=None)
def _channel_refs(sr, N):
    """float64 resampling of each of the six channels of _pcm(N), one evaluation of the filter for all: by linearity the reference of a downmix is
    the mean of its channels' references."""
    s16, f32 = _pcm(N)
    r = ref_resample(np.concatenate([s16.astype(np.float64), f32.astype(np.float64)]), sr)
    r.setflags(write=False)
    return r[:3], r[3:]


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32).numpy()


@pytest.mark.parametrize('N', LENGTHS)
@pytest.mark.parametrize('sr', RATES)
def test_resampler_matches_the_float64_formula(dev, sr, N):
    """int16 and float32, mono / two channels planar / two channels interleaved (host arrays) / three channels as a strided device view, against
    the float64 restatement within resample_bound; length, peak and the layouts' agreement bit for bit.  Measured on the MI355X: int16 at most
    0.020 (bounds 0.156 .. 0.522), float32 at most 6.4e-7 (bounds 4.75e-6 .. 1.59e-5)."""
    from merlot_reserve_amd import ingest
    L, M, K, _ = ingest.resample_table(sr)
    n_out = -((-N * L) // M)
    for data, refs, max_abs in zip(_pcm(N), _channel_refs(sr, N), (32768.0, 1.0)):
        bound = resample_bound(sr, max_abs)
        wide = torch.zeros((N, 7), dtype=torch.from_numpy(data).dtype, device=dev)
        wide[:, 1::2] = torch.from_numpy(np.ascontiguousarray(data.T)).to(dev)
        view = wide[:, 1::2]                                             # [N, 3], strides (7, 2): used in place
        assert view.stride() == (7, 2) and not view.is_contiguous()
        cases = {'mono': (np.array(data[0]), None, refs[0]), 'planar2': (np.array(data[:2]), None, refs[:2].mean(0)),
                 'interleaved2': (np.ascontiguousarray(data[:2].T), None, refs[:2].mean(0)), 'strided3': (view, True, refs.mean(0))}
        got = {}
        for name, (x, cl, ref) in cases.items():
            y, peak = ingest.resample_mono(x, sr, channels_last=cl, device=dev)
            assert y.shape == (n_out,) and y.dtype == torch.float32 and y.device == dev and peak.shape == () and peak.dtype == torch.float32
            err = float(np.abs(y.cpu().numpy().astype(np.float64) - ref).max())
            print(f'resample {sr} N={N} {data.dtype} {name}: max abs error {err:.3g}, bound {bound:.3g}')
            assert err <= bound, (name, err, bound)
            assert _bits(peak) == _bits(y.abs().max())
            got[name] = _bits(y)
        assert np.array_equal(got['planar2'], got['interleaved2'])       # the same samples through other strides: the same bits


def test_prefix_property_and_determinism(dev):
    """48 kHz: an output whose taps lie inside the first N1 samples has the same bits whether N1 or N samples follow -- block boundaries and the
    length of the signal do not reach it; and two calls agree in every bit of wave and peak."""
    from merlot_reserve_amd import ingest
    N1, N = 30011, 70001
    L, M, K, _ = ingest.resample_table(48000)
    x = _pcm(N)[0][0]
    full, peak = ingest.resample_mono(np.array(x), 48000, device=dev)
    again, peak2 = ingest.resample_mono(np.array(x), 48000, device=dev)
    part, _ = ingest.resample_mono(np.array(x[:N1]), 48000, device=dev)
    assert np.array_equal(_bits(full), _bits(again)) and _bits(peak) == _bits(peak2)
    n = np.arange(part.numel(), dtype=np.int64)
    inside = (n * M) // L + K // 2 <= N1 - 1
    assert 13000 < inside.sum() < part.numel()                           # several blocks' worth, and the tail differs
    assert np.array_equal(_bits(part)[inside], _bits(full)[:part.numel()][inside])
    assert not np.array_equal(_bits(part)[~inside], _bits(full)[:part.numel()][~inside])


def test_stop_band_on_the_kernel_output(dev):
    """A 2 s unit sine of 15 kHz from 48 kHz stays <= -80 dB: the restatement's -106 dB degraded by at most the rounding bound (8e-6 per sample, -102 dB)."""
    from merlot_reserve_amd import ingest
    x = np.sin(2 * np.pi * 15000.0 * np.arange(96000) / 48000.0).astype(np.float32)
    y, peak = ingest.resample_mono(x, 48000, device=dev)
    y = y.cpu().numpy().astype(np.float64)[2000:-2000]
    level = 20 * np.log10(np.sqrt(2.0 * np.mean(y ** 2)))
    print(f'15 kHz from 48 kHz on the kernel: {level:.1f} dB')
    assert level <= -80.0
    tone, _ = ingest.resample_mono(np.sin(2 * np.pi * 1000.0 * np.arange(96000) / 48000.0).astype(np.float32), 48000, device=dev)
    t = tone.cpu().numpy().astype(np.float64)[2000:-2000]
    assert abs(20 * np.log10(np.sqrt(2.0 * np.mean(t ** 2)))) <= 0.01


def test_native_rate_is_the_exact_downmix_and_launches_nothing(dev, monkeypatch):
    from merlot_reserve_amd import _ingest_lib, ingest

    def no_library():
        raise AssertionError('22050 Hz must not reach the library')
    monkeypatch.setattr(_ingest_lib, 'load', no_library)
    s16, f32 = _pcm(5000)
    y, peak = ingest.resample_mono(np.array(f32[0]), 22050, device=dev)
    assert np.array_equal(y.cpu().numpy(), f32[0]) and float(peak) == np.abs(f32[0]).max()
    y, peak = ingest.resample_mono(np.ascontiguousarray(s16.T), 22050, device=dev)
    want = ((s16[0].astype(np.float32) + s16[1].astype(np.float32)) + s16[2].astype(np.float32)) / np.float32(3.0)
    assert y.dtype == torch.float32 and np.array_equal(y.cpu().numpy(), want) and float(peak) == np.abs(want).max()


def test_layout_guessing(dev):
    from merlot_reserve_amd import ingest
    s16, _ = _pcm(5000)
    a, _ = ingest.resample_mono(np.array(s16[:2]), 44100, device=dev)
    b, _ = ingest.resample_mono(np.ascontiguousarray(s16[:2].T), 44100, device=dev)
    c, _ = ingest.resample_mono(torch.from_numpy(np.array(s16[:2])).to(dev), 44100)
    d, _ = ingest.resample_mono(np.array(s16[:2]).astype(np.float64), 44100, device=dev)                 # float64 host arrays are cast
    e, _ = ingest.resample_mono(np.array(s16[:2]).astype(np.float32), 44100, device=dev)
    assert np.array_equal(_bits(a), _bits(b)) and np.array_equal(_bits(a), _bits(c)) and np.array_equal(_bits(d), _bits(e))
    with pytest.raises(ValueError, match='channels_last'):
        ingest.resample_mono(np.zeros((4, 4), np.int16), 44100, device=dev)
    with pytest.raises(TypeError):
        ingest.resample_mono(np.zeros(100, np.int32), 44100, device=dev)
    with pytest.raises(ValueError):
        ingest.resample_mono(np.zeros((2, 3, 4), np.int16), 44100, device=dev)


# ------------------------------------------------------------------------------------------------ black bars
BOUNDS_SHAPES = [(3, 37, 53), (2, 130, 258), (1, 1, 1), (2, 64, 1024), (3, 7, 5)]       # 3 W mod 4 = 3; rows of 774 bytes; one pixel; aligned rows; rows shorter than a vector


@pytest.mark.parametrize('shape', BOUNDS_SHAPES)
def test_bounds_are_the_numpy_bounds(dev, shape):
    """Every pattern of the host test, a single bright value in one channel of the last frame at each corner and in the middle, an all-dark stack,
    thresholds on both sides of 128, and the same frames at a byte offset that is no multiple of 16: exact integers."""
    from merlot_reserve_amd import ingest
    n, H, W = shape
    for thr in (32, 200, 1):
        for name, (frames, t) in bar_cases(n, H, W, thr).items():
            want = ref_bounds(frames, t)
            assert ingest.content_bounds(frames, t, device=dev) == want, (name, thr)
            if name == 'dark':
                assert want == (H, -1, W, -1)
    for y, x in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (H // 2, W // 2)):
        for ch in range(3):
            f = np.zeros((n, H, W, 3), np.uint8)
            f[n - 1, y, x, ch] = 255
            assert ingest.content_bounds(f, 32, device=dev) == (y, y, x, x), (y, x, ch)
    frames = bar_cases(n, H, W, 32)['pillarbox'][0]
    flat = torch.zeros(frames.size + 32, dtype=torch.uint8, device=dev)
    for off in (5, 16):
        flat[off:off + frames.size] = torch.from_numpy(frames.reshape(-1)).to(dev)
        view = flat[off:off + frames.size].view(n, H, W, 3)
        assert view.data_ptr() % 16 == (flat.data_ptr() + off) % 16
        assert ingest.content_bounds(view, 32) == ref_bounds(frames, 32), off
    assert ingest.content_bounds(frames[0], 0, device=dev) == (0, H - 1, 0, W - 1)                        # [H, W, 3]; threshold 0: everything
    assert ingest.content_bounds(np.full((n, H, W, 3), 254, np.uint8), 255, device=dev) == (H, -1, W, -1)


def test_bounds_of_a_1080p_letterbox(dev):
    from merlot_reserve_amd import ingest
    frames = np.zeros((1, 1080, 1920, 3), np.uint8)
    frames[0, 138:942] = np.random.default_rng(0).integers(0, 256, (804, 1920, 3), dtype=np.uint8)
    frames[0, 138, 0] = frames[0, 941, 1919] = 255
    assert ingest.content_bounds(frames, 32, device=dev) == ref_bounds(frames, 32) == (138, 941, 0, 1919)
    assert ingest.detect_black_bars(frames, 32, device=dev) == ref_detect_black_bars(frames, 32) == (138, 942, 0, 1920)


def test_trim_is_a_view_and_feeds_the_patch_kernel(dev):
    from merlot_reserve_amd import ingest, media
    frames = bar_cases(2, 96, 160, 32)['letterbox'][0]
    y1, y2, x1, x2 = ref_detect_black_bars(frames, 32)
    assert (y1, y2, x1, x2) == (12, 84, 0, 160)
    host = ingest.trim_black_bars(frames, device=dev)
    assert isinstance(host, np.ndarray) and np.shares_memory(host, frames) and np.array_equal(host, frames[:, y1:y2, x1:x2])
    d = torch.from_numpy(frames).to(dev)
    t = ingest.trim_black_bars(d)
    assert t.data_ptr() == d.data_ptr() + (y1 * 160 + x1) * 3 and t.stride() == d.stride() and tuple(t.shape) == (2, y2 - y1, x2 - x1, 3)
    side = bar_cases(2, 96, 160, 32)['pillarbox'][0]
    ds = torch.from_numpy(side).to(dev)
    ts = ingest.trim_black_bars(ds)
    assert ts.data_ptr() == ds.data_ptr() + 20 * 3 and tuple(ts.shape) == (2, 96, 120, 3) and not ts.is_contiguous()
    for view, crop in ((t, frames[:, y1:y2, x1:x2]), (ts, side[:, :, 20:140])):
        got = media.frames_to_patches(view, (6, 10))
        want = media.frames_to_patches(np.ascontiguousarray(crop), (6, 10), device=dev)
        assert torch.equal(got, want)


# ------------------------------------------------------------------------------------------------ end to end
def _clip(seed=0):
    rng = np.random.default_rng(seed)
    frames = np.zeros((2, 96, 160, 3), np.uint8)
    frames[:, 12:84] = rng.integers(40, 256, (2, 72, 160, 3), dtype=np.uint8)
    t = np.arange(480000) / 48000.0
    pcm = np.stack([9000 * np.sin(2 * np.pi * 440.0 * t) + 2500 * rng.standard_normal(t.size),
                    7000 * np.sin(2 * np.pi * 660.0 * t) + 2500 * rng.standard_normal(t.size)], 1)
    return frames, np.clip(np.round(pcm), -32768, 32767).astype(np.int16)


def test_segments_from_pcm_end_to_end(dev):
    """2 letterboxed 96 x 160 frames and 10 s of 48 kHz stereo int16 -> segments on the device.

    Spectrogram bound, per element: LOGMEL_BOUND (the log-mel kernel against float64 on the same waveform) plus the resampling error carried
    through.  With B the resample_bound on the int16 scale and p the float64 peak, a normalised sample is off by at most
        d = 2 B / p + 2^-24          (its own error, the peak's error -- relative B / p on |w| <= 1 --, the float32 division)
    a windowed DFT bin by at most D = d sum(window), a mel value by at most 2 D sqrt(F mel) + F D^2 (Cauchy-Schwarz over the bins, F = the
    filter's sum of weights), and log(mel + 0.1) by that over (mel + 0.1), mel taken from the reference.  Measured on the MI355X: at most 6.0e-6
    (allowances 9.1e-4 .. 2.9e-2)."""
    from merlot_reserve_amd import ingest, preprocess as P
    import scipy.signal
    frames, pcm = _clip()
    segs = P.segments_from_pcm(frames, pcm, 48000, device=dev)
    assert [(s['start_time'], s['end_time'], s['idx']) for s in segs] == [(0.0, 5.0, 0), (5.0, 10.0, 1)]
    ref = ref_resample(pcm.astype(np.float64).mean(1), 48000)
    assert ref.size == 220500
    p = np.abs(ref).max()
    w = ref / max(p, 1.0)
    want = ref_logmel(np.stack([w[:110250], w[110250:220500]]))
    d = 2 * resample_bound(48000, 32768.0) / p + 2.0 ** -24
    D = d * scipy.signal.windows.hann(1536).sum()
    F = ref_filterbank().sum(1)
    mel = 0.1 * np.exp(want[..., :64]) - 0.1
    bound = LOGMEL_BOUND + (2 * D * np.sqrt(F * np.maximum(mel, 0.0)) + F * D * D) / (mel + 0.1)
    starts = (2, 64, 126)
    for i, s in enumerate(segs):
        spec = s['spectrogram']
        assert spec.device == dev and tuple(spec.shape) == (3, 60, 65) and spec.dtype == torch.float32
        g = spec.cpu().numpy().astype(np.float64)
        for j, a in enumerate(starts):
            err = np.abs(g[j, :, :64] - want[i, a:a + 60, :64])
            print(f'segment {i} clip {j}: max abs error {err.max():.3g}, largest allowance {bound[i, a:a + 60].max():.3g}, smallest {bound[i, a:a + 60].min():.3g}')
            assert np.all(err <= bound[i, a:a + 60])
            assert np.all(g[j, :, 64] == 1.0)
        assert s['frame'].device == dev and np.array_equal(s['frame'].cpu().numpy(), frames[i, 12:84])
    plain = P.segments_from_pcm(frames, pcm, 48000, trim_black_bars=False)                                # host in, host out
    assert isinstance(plain[0]['frame'], np.ndarray) and plain[0]['frame'].shape == (96, 160, 3) and isinstance(plain[0]['spectrogram'], np.ndarray)
    assert np.array_equal(plain[1]['spectrogram'], segs[1]['spectrogram'].cpu().numpy())


def test_zeroshot_eval_command_on_decoded_media(dev, tmp_path):
    from merlot_reserve_amd import ingest, preprocess as P, zeroshot_eval as Z
    from merlot_reserve_amd.planner import AUDIOSPAN
    out = str(tmp_path / 'run')
    cmd = [sys.executable, '-m', 'merlot_reserve_amd.zeroshot_eval', 'base', '--random-weights', '--synthetic-media', '2', '--grid', '12', '20', '--out', out,
           '-k', '1', '5']
    p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    acc = json.load(open(os.path.join(out, 'accuracy.json')))
    preds = [json.loads(line) for line in open(os.path.join(out, 'predictions.jsonl'))]
    assert acc['n'] == 2 and len(preds) == 2 and all(len(r['masks']) == 1 for r in preds) and [r['id'] for r in preds] == ['media_0000', 'media_0001']
    # what the command fed the model: read_manifest against the chain by hand, bit for bit
    fed = Z.read_manifest(os.path.join(out, 'samples.jsonl'), grid=(12, 20), device=dev)
    recs = [json.loads(line) for line in open(os.path.join(out, 'samples.jsonl'))]
    assert len(fed) == 2
    for (sid, video, answer), rec in zip(fed, recs):
        frames = np.load(os.path.join(out, rec['frames']))
        pcm, sr = ingest.read_wav(os.path.join(out, rec['wav']))
        assert frames.shape == (2, 96, 160, 3) and pcm.shape == (480000, 2) and sr == 48000 and sid == rec['id'] and answer == rec['answer']
        segs = P.segments_from_pcm(frames, pcm, sr, device=dev)
        assert tuple(segs[0]['frame'].shape) == (72, 160, 3)
        for s, extra in zip(segs, rec['segments']):
            s.update(extra)
        want = P.preprocess_video(segs, (12, 20), device=dev)
        assert set(video) == set(Z.VIDEO_KEYS)
        assert torch.equal(video['images'], want['images']) and torch.equal(video['audio_clips'], want['audio_clips'])
        assert np.array_equal(video['tokens'], want['tokens']) and np.array_equal(video['subseg_idxs'], want['subseg_idxs'])
        assert (video['tokens'] == P.MASK).sum() == 1 and (video['tokens'] == AUDIOSPAN).sum() == 18 and tuple(video['images'].shape) == (2, 240, 768)
