"""Host side of media ingest (no GPU): the C-ABI of libmreserve_ingest.so (exports, prototypes, argument checks, a ledger of which test calls
which export, the build scans), the polyphase table and the filter's quality on the float64 restatement of tests/ingest_refs.py, the
finishing logic of detect_black_bars, read_wav, the slicing of segments_from_pcm / segments_from_decoded_zero_shot, and read_manifest unchanged
on the manifests it took before."""
import ctypes
import json
import os
import re
import subprocess
import wave

import numpy as np
import pytest

from ingest_refs import bar_cases, ref_bounds, ref_detect_black_bars, ref_kernel, ref_ratio, ref_resample

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'mreserve_ingest.h')
NAMES = ['mri_content_bounds', 'mri_last_error', 'mri_resample_len', 'mri_resample_mono', 'mri_version']


def _built():
    import __graft_entry__
    __graft_entry__.build()


def declared_symbols():
    text = re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r'\b(mri_[a-z0-9_]+)\s*\(', text)))


# ------------------------------------------------------------------------------------------------ the library
def test_ingest_library_exports_the_header_and_nothing_else():
    _built()
    from merlot_reserve_amd import _ingest_lib, _lib, _media_lib, _zeroshot_lib
    assert declared_symbols() == NAMES
    out = subprocess.check_output(['nm', '-D', '--defined-only', _ingest_lib.LIB_PATH], text=True)
    assert sorted(line.split()[-1] for line in out.splitlines() if line.strip()) == NAMES
    assert sorted(_ingest_lib.PROTOTYPES) == NAMES
    assert not set(_ingest_lib.PROTOTYPES) & (set(_lib.PROTOTYPES) | set(_media_lib.PROTOTYPES) | set(_zeroshot_lib.PROTOTYPES))
    assert _ingest_lib.load().mri_version() >= 1
    for other in (_lib.LIB_PATH, _media_lib.LIB_PATH, _zeroshot_lib.LIB_PATH):           # the other three carry none of these
        assert 'mri_' not in subprocess.check_output(['nm', '-D', '--defined-only', other], text=True)
    text = open(HEADER).read()
    assert (_ingest_lib.DT_S16, _ingest_lib.DT_F32) == (0, 1) and '#define MRI_DT_S16 0' in text and '#define MRI_DT_F32 1' in text
    assert '#define MRI_SR 22050' in text
    assert 'mri_*' in open(os.path.join(ROOT, 'merlot_reserve_amd', 'csrc', 'ingest_exports.map')).read()


def test_prototypes_match_the_header():
    """Argument counts and the C types of every parameter against the ctypes table."""
    from merlot_reserve_amd import _ingest_lib as M
    text = re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)
    ctype = {'int': M.i32, 'int32_t': M.i32, 'int64_t': M.i64, 'float': M.f32, 'const char*': ctypes.c_char_p}
    found = re.findall(r'^([a-z0-9_ ]+?\*?)\s*(mri_[a-z0-9_]+)\s*\(([^)]*)\)\s*;', text, flags=re.M | re.S)
    assert sorted(name for _, name, _ in found) == NAMES
    for ret, name, args in found:
        res, argtypes = M.PROTOTYPES[name]
        assert res is ctype[ret.strip()], name
        params = [] if args.strip() == 'void' else [a.strip() for a in args.split(',')]
        assert len(params) == len(argtypes), name
        for p, t in zip(params, argtypes):
            want = M.vp if '*' in p else ctype[p.rsplit(' ', 1)[0].strip()]
            assert t is want, (name, p)


def test_bad_arguments_are_reported_without_a_launch():
    _built()
    from merlot_reserve_amd import _ingest_lib as M
    lib = M.load()
    p = 1 << 20                      # fake device addresses: never dereferenced, every case is rejected before a launch
    assert lib.mri_resample_len(70001, 147, 320) == 32157 and lib.mri_resample_len(7, 1, 2) == 4 and lib.mri_resample_len(2, 441, 320) == 3
    assert lib.mri_resample_len(0, 1, 2) == 0 and lib.mri_resample_len(5, 0, 2) == 0 and lib.mri_resample_len(5, 1, 0) == 0
    #     x  dtype     C  N     ch    ss taps L    M    K   y  peak stream
    ok = (p, M.DT_S16, 2, 5000, 5000, 1, p, 147, 320, 70, p, p, None)

    def with_(i, v, base=ok):
        return base[:i] + (v,) + base[i + 1:]
    for i in (0, 6, 10, 11):
        assert lib.mri_resample_mono(*with_(i, None)) == -1 and b'mri_resample_mono: null pointer' in lib.mri_last_error(), i
    for i, v, word in ((3, 0, b'shape'), (2, 0, b'shape'), (7, 0, b'ratio'), (8, 0, b'ratio'), (9, 0, b'taps'), (9, 1, b'taps'), (9, 71, b'taps'),
                       (1, 2, b'dtype'), (1, -1, b'dtype'), (4, 0, b'zero stride'), (5, 0, b'zero stride')):
        assert lib.mri_resample_mono(*with_(i, v)) == -1, (i, v)
        assert word in lib.mri_last_error(), (i, v, lib.mri_last_error())
    # a ratio whose 64-output span cannot be staged is refused too (nothing of the kind between 4 and 192 kHz)
    assert lib.mri_resample_mono(*with_(9, 6400, with_(8, 200 * 147))) == -1 and b'does not fit' in lib.mri_last_error()
    okb = (p, 2, 37, 53, 32, p, None)
    for i in (0, 5):
        assert lib.mri_content_bounds(*with_(i, None, okb)) == -1 and b'mri_content_bounds: null pointer' in lib.mri_last_error()
    for i, v, word in ((1, 0, b'shape'), (2, 0, b'shape'), (3, 0, b'shape'), (4, -1, b'threshold'), (4, 256, b'threshold')):
        assert lib.mri_content_bounds(*with_(i, v, okb)) == -1, (i, v)
        assert word in lib.mri_last_error(), (i, v, lib.mri_last_error())
    assert lib.mri_content_bounds(p, 1, 1 << 15, 1 << 15, 32, p, None) == -1 and b'2^30' in lib.mri_last_error()      # 3 x 2^30 bytes a frame
    with pytest.raises(M.MreserveIngestError, match='2\\^30'):
        M.check(-1, 'mri_content_bounds')


# which test file calls which export: (the Python names tests reach it by, the test files), in the style of test_cabi_test_ledger.py
HOST, GPU = 'test_ingest_host.py', 'test_ingest_gpu.py'
LEDGER = {
    'mri_version': ((), (HOST,)),
    'mri_last_error': ((), (HOST,)),
    'mri_resample_len': ((), (HOST,)),
    'mri_resample_mono': (('resample_mono',), (GPU, HOST)),
    'mri_content_bounds': (('content_bounds',), (GPU, HOST)),
}


def test_every_ingest_export_names_its_test():
    assert set(LEDGER) == set(declared_symbols())
    binding = open(os.path.join(ROOT, 'merlot_reserve_amd', 'ingest.py')).read()
    for export, (wrappers, files) in LEDGER.items():
        assert files, export
        for w in wrappers:
            assert re.search(rf'^def {re.escape(w)}\b', binding, flags=re.M) and re.search(rf'\b{export}\b', binding), export
        for fname in files:
            text = open(os.path.join(ROOT, 'tests', fname)).read()
            assert any(re.search(rf'\b{re.escape(n)}\b', text) for n in (export,) + tuple(wrappers)), (export, fname)


def test_build_scans_cover_the_ingest_library():
    _built()
    from merlot_reserve_amd import build as B
    assert B.INGEST_HIP_FILES == ['ingest.hip'] and B.INGEST_SOURCES == ['ingest.hip']
    assert not set(B.INGEST_SOURCES) & (set(B.SOURCES) | set(B.MEDIA_SOURCES) | set(B.ZEROSHOT_SOURCES))
    assert '-fno-slp-vectorize' in B.EXTRA_FLAGS['ingest.hip'] and B.INGEST_LIB.endswith('libmreserve_ingest.so')
    if B._asm_stale():
        B.build(force=True, verbose=False)
    assert B.scan_packed_op_sel(files=B.INGEST_HIP_FILES) == [] and B.scan_spills(files=B.INGEST_HIP_FILES) == []
    res = B.kernel_resources(B.INGEST_HIP_FILES)['ingest.hip']
    assert len(res) == 3                                                   # resample (int16, fp32), bounds
    assert all(e['vgpr_spill'] == 0 and e['sgpr_spill'] == 0 and e['scratch'] == 0 for e in res.values())
    asm = open(B._asm_path('ingest.hip')).read()
    assert not re.search(r'v_(sin|cos|exp|log)_f32', asm)                  # the filter is a table: no transcendental in the kernels
    assert not re.search(r'global_atomic_\w*f32', asm)                     # integer atomics only
    # the fourth library is part of the rebuild conditions
    os.utime(B._asm_path('ingest.hip'), (0, 0))
    try:
        assert B._asm_stale()
    finally:
        os.utime(B._asm_path('ingest.hip'))


# ------------------------------------------------------------------------------------------------ the table
@pytest.mark.parametrize('sr,lmk', [(44100, (1, 2, 64)), (48000, (147, 320, 70)), (16000, (441, 320, 32)), (32000, (441, 640, 48)),
                                    (96000, (147, 640, 140))])
def test_resample_table(sr, lmk):
    from merlot_reserve_amd import ingest
    L, M, K, taps = ingest.resample_table(sr)
    assert (L, M, K) == lmk and taps.shape == (L, K) and taps.dtype == np.float32
    assert ingest.resample_table(sr)[3] is taps                                             # cached per rate
    t64 = taps.astype(np.float64)
    assert np.abs(t64.sum(1) - 1.0).max() <= 2.0 ** -22
    assert np.abs(t64).sum(1).max() <= 2.4
    # the table is the restated continuous kernel at the phase offsets, each row over its float64 sum, rounded once
    Lr, Mr, half, c = ref_ratio(sr)
    assert (Lr, Mr, 2 * half) == lmk
    frac = ((np.arange(L) * M) % L) / L
    w = ref_kernel((np.arange(K) - half + 1)[None, :] - frac[:, None], half, c)
    assert 1.80 - 0.005 <= np.abs(w).sum(1).max() <= 2.28 + 0.005                                    # the un-normalised design: 1.80 (44.1 kHz) .. 2.28 (16 kHz)
    w /= w.sum(1, keepdims=True)
    assert np.abs(t64 - w).max() <= 2.0 ** -24 * np.abs(w).max() * 1.0001
    assert ingest.resample_len(70001, sr) == -((-70001 * L) // M)


def test_resample_table_rejects_other_rates():
    from merlot_reserve_amd import ingest
    for sr in (3999, 192001, 0, -44100, 44100.0, '48000', None, True):
        with pytest.raises(ValueError):
            ingest.resample_table(sr)
    L, M, K, taps = ingest.resample_table(44101)
    assert (L, M, K) == (22050, 44101, 66) and taps.shape == (22050, 66)
    assert ingest.resample_table(22050)[:3] == (1, 1, 32)


def _tone_db(sr, f):
    """level in dB re a unit sine of a 2 s unit sine of f Hz after resampling from sr, 2000 output samples dropped at each end"""
    x = np.sin(2 * np.pi * f * np.arange(2 * sr) / sr)
    y = ref_resample(x, sr)[2000:-2000]
    return 20 * np.log10(np.sqrt(2.0 * np.mean(y ** 2)))


@pytest.mark.parametrize('sr', [44100, 48000])
def test_filter_quality_downsampling(sr):
    """Pass band flat, stop band down, on the float64 restatement.  Evaluated: 1 kHz 0.00 dB; 9 kHz -0.02 (44.1 kHz) / -0.01 (48 kHz);
    15 kHz -99.3 / -106.5."""
    levels = {f: _tone_db(sr, f) for f in (1000, 9000, 15000)}
    print(sr, levels)
    assert abs(levels[1000]) <= 0.01
    assert abs(levels[9000]) <= 0.05
    assert levels[15000] <= -90.0


def test_filter_quality_upsampling():
    assert abs(_tone_db(16000, 1000)) <= 0.01


# ------------------------------------------------------------------------------------------------ black bars
@pytest.mark.parametrize('shape', [(2, 40, 60), (1, 7, 9), (3, 100, 50)])
@pytest.mark.parametrize('thr,perc', [(16, .2), (32, .2), (32, .05)])
def test_detect_black_bars_finishing_logic(monkeypatch, shape, thr, perc):
    """content_bounds replaced by the numpy restatement: letterbox within the cap and beyond it (the cap binds), pillarbox, content touching all four
    edges, all dark (both fall-backs), a pixel exactly at the threshold and one below."""
    from merlot_reserve_amd import ingest
    calls = []

    def fake(frames, threshold, device=None):
        calls.append(threshold)
        return ref_bounds(np.asarray(frames), threshold)
    monkeypatch.setattr(ingest, 'content_bounds', fake)
    n, H, W = shape
    for name, (frames, t) in bar_cases(n, H, W, thr).items():
        got = ingest.detect_black_bars(frames, blackbar_threshold=t, max_perc_to_trim=perc)
        assert got == ref_detect_black_bars(frames, t, perc), name
        assert all(isinstance(v, int) for v in got)
        y1, y2, x1, x2 = got
        if name == 'full':
            assert got == (0, H, 0, W)
        if name in ('dark', 'below_threshold'):                            # the middle row / column stand in, then the caps
            assert got == (min(H // 2, int(H * perc)), max(H // 2 + 1, int(H * (1 - perc))), min(W // 2, int(W * perc)), max(W // 2 + 1, int(W * (1 - perc))))
        if name == 'at_threshold':
            assert y1 <= H // 2 < y2 and x1 <= W // 2 < x2
        if name == 'deep_letterbox' and H >= 40:                           # a third of the height is bar: the cap binds
            assert (y1, y2) == (int(H * perc), int(H * (1 - perc)))
        if name == 'letterbox' and H >= 40 and perc == .2:                 # an eighth: within the cap, trimmed exactly
            assert (y1, y2) == (H // 8, H - H // 8)
        trimmed = ingest.trim_black_bars(frames, blackbar_threshold=t, max_perc_to_trim=perc)
        assert np.shares_memory(trimmed, frames) and trimmed.shape == (n, y2 - y1, x2 - x1, 3) and np.array_equal(trimmed, frames[:, y1:y2, x1:x2])
    assert calls and all(c == thr for c in calls)
    assert ingest.detect_black_bars.__defaults__[:2] == (16, .2) and ingest.trim_black_bars.__defaults__[:2] == (32, .2)


# ------------------------------------------------------------------------------------------------ wav files
@pytest.mark.parametrize('channels,sr', [(1, 16000), (2, 48000)])
def test_read_wav_round_trip(tmp_path, channels, sr):
    from merlot_reserve_amd import ingest
    rng = np.random.default_rng(channels)
    pcm = rng.integers(-32768, 32768, (1234, channels), dtype=np.int16)
    path = tmp_path / 'a.wav'
    with wave.open(str(path), 'wb') as f:
        f.setnchannels(channels)
        f.setsampwidth(2)
        f.setframerate(sr)
        f.writeframes(pcm.astype('<i2').tobytes())
    got, got_sr = ingest.read_wav(path)
    assert got_sr == sr and got.dtype == np.int16 and got.shape == (1234, channels) and np.array_equal(got, pcm)
    with wave.open(str(path), 'wb') as f:
        f.setnchannels(channels)
        f.setsampwidth(1)
        f.setframerate(sr)
        f.writeframes(bytes(100 * channels))
    with pytest.raises(ValueError, match='16-bit'):
        ingest.read_wav(path)


# ------------------------------------------------------------------------------------------------ preprocess
def _patch(monkeypatch, P, wave22050, peak):
    import torch
    from merlot_reserve_amd import ingest
    seen = {}

    def fake_resample(pcm, sr, channels_last=None, device=None):
        seen['pcm'], seen['sr_in'], seen['channels_last'] = pcm, sr, channels_last
        return torch.from_numpy(wave22050), torch.tensor(peak, dtype=torch.float32)

    def fake_spec(waves, playback_speed=1, sr=22050, pad_size=2, device=None):
        seen.setdefault('waves', []).append(np.array(waves))
        seen['sr'] = sr
        return np.arange(waves.shape[0] * 3 * 60 * 65, dtype=np.float32).reshape(waves.shape[0], 3, 60, 65)
    monkeypatch.setattr(ingest, 'resample_mono', fake_resample)
    monkeypatch.setattr(P, 'make_spectrograms', fake_spec)
    monkeypatch.setattr(ingest, 'content_bounds', lambda frames, threshold, device=None: ref_bounds(np.asarray(frames), threshold))
    return seen


def test_segments_from_pcm_slices_and_normalises(monkeypatch):
    from merlot_reserve_amd import preprocess as P
    rng = np.random.default_rng(0)
    wave22050 = (rng.standard_normal(300000) * 9000).astype(np.float32)   # shorter than 3 segments from 2.5 s: zero-padded
    peak = float(np.abs(wave22050).max())
    seen = _patch(monkeypatch, P, wave22050, peak)
    frames = np.zeros((3, 20, 30, 3), np.uint8)
    frames[:, 3:17, :] = rng.integers(32, 256, (3, 14, 30, 3), dtype=np.uint8)
    pcm = np.zeros((1000, 2), np.int16)
    segs = P.segments_from_pcm(frames, pcm, 48000, segment_start_time=2.5, channels_last=True)
    assert seen['pcm'] is pcm and seen['sr_in'] == 48000 and seen['channels_last'] is True and seen['sr'] == 22050
    assert [(s['start_time'], s['end_time'], s['mid_time'], s['idx']) for s in segs] == [(2.5, 7.5, 5.0, 0), (7.5, 12.5, 10.0, 1), (12.5, 17.5, 15.0, 2)]
    w = wave22050 / np.float32(peak)
    w = np.concatenate([w, np.zeros(int(22050 * 17.5) - w.size, dtype=np.float32)])
    waves, = seen['waves']
    assert waves.dtype == np.float32 and waves.shape == (3, 110250)
    for i, (a, b) in enumerate([(55125, 165375), (165375, 275625), (275625, 385875)]):
        assert np.array_equal(waves[i], w[a:b])
        assert segs[i]['spectrogram'].shape == (3, 60, 65) and np.array_equal(segs[i]['frame'], frames[i, 3:17])       # trimmed: 3 <= int(20 * .2)
    assert np.all(waves[2][300000 - 275625:] == 0)
    # untouched frames on request, and a list of frames
    segs = P.segments_from_pcm(list(frames[:1]), pcm, 44100, trim_black_bars=False, time_interval=2.5 + 5.0)
    assert np.array_equal(segs[0]['frame'], frames[0])
    assert P.segments_from_pcm([], pcm, 44100) == []
    with pytest.raises(ValueError, match='unequal length'):
        P.segments_from_pcm(frames, pcm, 48000, time_interval=5.00002)               # int(22050 * 15.00006) - int(22050 * 10.00004) = 110251


def test_segments_from_pcm_quiet_clip_is_not_amplified(monkeypatch):
    """The divisor is max(peak, 1)."""
    from merlot_reserve_amd import preprocess as P
    seen = _patch(monkeypatch, P, np.full(110250, 0.25, np.float32), 0.25)
    P.segments_from_pcm(np.zeros((1, 8, 8, 3), np.uint8), np.zeros(10, np.int16), 44100, trim_black_bars=False)
    assert np.all(seen['waves'][0] == np.float32(0.25))


def test_segments_from_decoded_zero_shot_cuts(monkeypatch):
    from merlot_reserve_amd import preprocess as P
    rng = np.random.default_rng(1)
    seen = _patch(monkeypatch, P, np.zeros(1, np.float32), 1.0)
    wave_in = (rng.standard_normal(20 * 22050) * 3.0).astype(np.float32)
    w = wave_in / np.float32(np.abs(wave_in).max())
    frames = rng.integers(0, 256, (3, 4, 5, 3), dtype=np.uint8)
    times = [{'start_time': 1.0, 'end_time': 3.0, 'mid_time': 2.0},          # 2 s: centred in zeros
             {'start_time': 4.0, 'end_time': 12.0, 'mid_time': 8.0},         # 8 s: mid +- 2.5
             {'start_time': 12.0, 'end_time': 17.0, 'mid_time': 14.5}]       # exactly 5 s: the mid +- 2.5 branch as well
    segs = P.segments_from_decoded_zero_shot(frames, wave_in, times)
    assert 'spectrogram' not in times[0] and [s['idx'] for s in segs] == [0, 1, 2] and seen['sr'] == 22050
    assert len(seen['waves']) == 1 and seen['waves'][0].shape == (3, 110250)                  # one length, one launch
    waves = seen['waves'][0]
    left = int((22050 * 5.0 - 44100) / 2)
    assert left == 33075 and int(22050 * 5.0 - 44100 - left) == 33075
    assert np.all(waves[0][:left] == 0) and np.array_equal(waves[0][left:left + 44100], w[22050:66150]) and np.all(waves[0][left + 44100:] == 0)
    assert np.array_equal(waves[1], w[int(22050 * 5.5):int(22050 * 10.5)])
    assert np.array_equal(waves[2], w[int(22050 * 12.0):int(22050 * 17.0)])
    for i, s in enumerate(segs):
        assert np.array_equal(s['frame'], frames[i]) and s['spectrogram'].shape == (3, 60, 65) and s['mid_time'] == times[i]['mid_time']
    # a quiet waveform is not amplified; an odd segment length keeps the int() paddings; a waveform shorter than the last end is padded
    seen.pop('waves')
    segs = P.segments_from_decoded_zero_shot(frames[:1], np.full(30000, 0.5), [{'start_time': 0.0, 'end_time': 1.5001, 'mid_time': 0.75005}])
    cut, = seen['waves']
    n = int(22050 * 1.5001)
    left = int((110250.0 - n) / 2)
    assert n == 33077 and left == 38586 and cut.shape == (1, left + n + int(110250.0 - n - left)) == (1, 110250)
    assert np.all(cut[0, left:left + 30000] == np.float32(0.5)) and np.all(cut[0, :left] == 0) and np.all(cut[0, left + 30000:] == 0)
    # cuts of different lengths (a start before 0 slices from the end, as in numpy: here an empty cut): one launch per length
    seen.pop('waves')
    P.segments_from_decoded_zero_shot(frames[:2], wave_in, [times[0], {'start_time': -1.0, 'end_time': 5.0, 'mid_time': 2.0}])
    assert sorted(x.shape for x in seen['waves']) == [(1, 0), (1, 110250)]
    assert P.segments_from_decoded_zero_shot([], wave_in, []) == []


def test_a_cut_of_the_wrong_length_raises_the_reference_error():
    """Not patched: make_spectrograms itself refuses before any launch."""
    from merlot_reserve_amd import preprocess as P
    with pytest.raises(ValueError, match=r'provided mel spectrogram \(1, 65\). target size: \(188, 65\)'):
        P.segments_from_decoded_zero_shot(np.zeros((1, 4, 4, 3), np.uint8), np.zeros(200000, np.float32),
                                          [{'start_time': -1.0, 'end_time': 5.0, 'mid_time': 2.0}])


def test_new_names_are_reexported_and_old_ones_unchanged():
    import inspect
    import mreserve.preprocess as MP
    from merlot_reserve_amd import preprocess as P
    for name in ('segments_from_pcm', 'segments_from_decoded_zero_shot'):
        assert getattr(MP, name) is getattr(P, name)
    assert list(inspect.signature(P.segments_from_pcm).parameters) == ['frames', 'pcm', 'sr', 'time_interval', 'segment_start_time', 'trim_black_bars',
                                                                       'blackbar_threshold', 'max_perc_to_trim', 'channels_last', 'device']
    assert P.segments_from_pcm.__defaults__ == (5.0, 0.0, True, 32, .2, None, None)
    assert list(inspect.signature(P.segments_from_decoded_zero_shot).parameters) == ['frames', 'waveform', 'times', 'sr', 'device']
    assert list(inspect.signature(P.segments_from_decoded).parameters) == ['frames', 'waveform', 'sr', 'time_interval', 'segment_start_time', 'device']
    with pytest.raises(NotImplementedError, match='segments_from_pcm'):
        P.video_to_segments('clip.mp4')
    assert not hasattr(P, 'video_to_segments_for_action_segmentation')


def test_resample_mono_rejects_bad_input_before_any_launch():
    from merlot_reserve_amd import ingest
    with pytest.raises(ValueError):
        ingest.resample_mono(np.zeros(10, np.int16), 1000)
    with pytest.raises(ValueError):
        ingest.resample_mono(np.zeros(10, np.int16), 44100.5)


# ------------------------------------------------------------------------------------------------ the command's manifest
def test_read_manifest_on_npz_lines_is_unchanged(tmp_path):
    from merlot_reserve_amd import zeroshot_eval as Z
    rng = np.random.default_rng(4)
    video = {'images': rng.random((2, 6, 768)).astype(np.float32), 'audio_clips': rng.random((6, 60, 65)).astype(np.float32),
             'tokens': rng.integers(0, 100, 160).astype(np.int32), 'subseg_idxs': rng.integers(-1, 6, 160).astype(np.int32)}
    np.savez(tmp_path / 'a.npz', **video)
    with open(tmp_path / 'm.jsonl', 'w') as f:
        f.write(json.dumps({'id': 'a', 'npz': 'a.npz', 'answer': 3}) + '\n\n')
        f.write(json.dumps({'id': 'b', 'npz': 'a.npz', 'answer': {'option': 1}}) + '\n')
    for got in (Z.read_manifest(str(tmp_path / 'm.jsonl')), Z.read_manifest(str(tmp_path / 'm.jsonl'), grid=(2, 3), device=None)):
        assert [(i, a) for i, _, a in got] == [('a', 3), ('b', {'option': 1})]
        for _, v, _ in got:
            assert set(v) == set(Z.VIDEO_KEYS) and all(isinstance(v[k], np.ndarray) and v[k].dtype == video[k].dtype and np.array_equal(v[k], video[k]) for k in video)
    with open(tmp_path / 'media.jsonl', 'w') as f:
        f.write(json.dumps({'id': 'c', 'frames': 'c.npy', 'wav': 'c.wav', 'segments': [], 'answer': 0}) + '\n')
    with pytest.raises(ValueError, match='grid'):
        Z.read_manifest(str(tmp_path / 'media.jsonl'))
