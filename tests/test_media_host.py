"""Host side of the media front end (no GPU): the float64 tables of merlot_reserve_amd.media against the restated formulas and
records.resize_and_pad, the slicing of segments_from_decoded, the C-ABI of libmreserve_media.so (exports, prototypes, argument checks, a
ledger of which test calls which export), and preprocess_video unchanged on the inputs it took before."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from media_refs import ref_filterbank, ref_patchify, ref_resize_pad, ref_scaled_size

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (input H, W) -> output (dh, dw): up- and down-scaling, portrait, square, zero rows, a height that clamps to 1, the two model grids
RESIZE_CASES = [((37, 53), (64, 96)), ((200, 90), (64, 96)), ((48, 48), (64, 96)), ((90, 160), (64, 96)), ((3, 500), (64, 96)),
                ((360, 640), (192, 320)), ((1080, 1920), (288, 512))]


def _built():
    import __graft_entry__
    __graft_entry__.build()


def declared_symbols():
    text = open(os.path.join(ROOT, 'include', 'mreserve_media.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    return sorted(set(re.findall(r'\b(mrm_[a-z0-9_]+)\s*\(', text)))


# ------------------------------------------------------------------------------------------------ tables
def test_filterbank():
    from merlot_reserve_amd import media
    fb = media.mel_filterbank()
    assert fb.shape == (64, 769) and fb.dtype == np.float64
    np.testing.assert_allclose(fb[:3].sum(1), [0.0706895, 0.06850934, 0.07088739], rtol=2e-7)
    assert int((fb == 0).all(0).sum()) == 3
    np.testing.assert_allclose(fb, ref_filterbank(), rtol=1e-12, atol=1e-18)


def test_window_is_the_symmetric_hann():
    import scipy.signal
    from merlot_reserve_amd import media
    win = media.hann_window()
    assert win.shape == (1536,) and win[0] == 0 and win[1535] == 0 and win[767] == win[768]
    np.testing.assert_allclose(win, scipy.signal.windows.hann(1536), atol=1e-15)
    tw = media.twiddle_table()
    assert tw.shape == (2, 1536) and tw[0, 0] == 1 and tw[1, 0] == 0 and abs(tw[1, 384] - 1) < 1e-15 and abs(tw[0, 768] + 1) < 1e-15


@pytest.mark.parametrize('hw,out', RESIZE_CASES)
def test_resample_formula_is_resize_and_pad(hw, out):
    """The float64 triangle filter agrees with records.resize_and_pad (PIL's antialiased bilinear on float planes) to 1e-6, and the host's
    (sh, sw) is the size that function scales to."""
    from merlot_reserve_amd import media, records
    rng = np.random.default_rng(hw[0] * 7 + hw[1])
    img = rng.random((hw[0], hw[1], 3)).astype(np.float32)
    got, info = records.resize_and_pad(img, out, None, do_random_scale=False, do_flip_if_vertical=False, resize_method='bilinear')
    ref = ref_resize_pad(img, *out)
    assert np.abs(ref - got).max() <= 1e-6
    sh, sw = media.resize_geometry(hw[0], hw[1], *out)
    assert (sh, sw) == ref_scaled_size(hw[0], hw[1], *out)
    assert min(sh, out[0]) == max(int(round(float(info[0]) * out[0])), 1) and min(sw, out[1]) == max(int(round(float(info[1]) * out[1])), 1)
    assert np.all(ref[min(sh, out[0]):] == 0) and np.all(ref[:, min(sw, out[1]):] == 0)


@pytest.mark.parametrize('hw,out', RESIZE_CASES[:6])
def test_tap_tables_restate_the_formula(hw, out):
    """The float32 tables the kernel receives, applied in numpy, give the float64 formula; padding outputs have no taps; ranges stay inside the frame."""
    from merlot_reserve_amd import media
    rng = np.random.default_rng(5)
    img = rng.integers(0, 256, (hw[0], hw[1], 3), dtype=np.uint8)
    sh, sw = media.resize_geometry(hw[0], hw[1], *out)
    (yr, yw), (xr, xw) = media.tap_tables(hw[0], sh, out[0]), media.tap_tables(hw[1], sw, out[1])
    assert yr.dtype == np.int32 and yw.dtype == np.float32 and yr.shape == (out[0], 2) and xw.shape[0] == out[1]
    for r, w, a, b, o in ((yr, yw, hw[0], sh, out[0]), (xr, xw, hw[1], sw, out[1])):
        assert np.all(r[:, 0] >= 0) and np.all(r[:, 0] + r[:, 1] <= a) and np.all(r[:, 1] <= w.shape[1])
        assert np.all(r[min(b, o):, 1] == 0) and np.all(r[:min(b, o), 1] >= 1)
        np.testing.assert_allclose(w.sum(1)[:min(b, o)], 1.0, atol=3e-7)
    My = np.zeros((out[0], hw[0]))
    for i, (lo, cnt) in enumerate(yr):
        My[i, lo:lo + cnt] = yw[i, :cnt]
    Mx = np.zeros((out[1], hw[1]))
    for i, (lo, cnt) in enumerate(xr):
        Mx[i, lo:lo + cnt] = xw[i, :cnt]
    got = np.clip(np.einsum('yh,hxc->yxc', My, np.einsum('hwc,xw->hxc', img.astype(np.float64), Mx)), 0, 255) / 255.0
    assert np.abs(got - ref_resize_pad(img.astype(np.float32) / np.float32(255.0), *out)).max() <= 1e-6


# ------------------------------------------------------------------------------------------------ preprocess
def test_segments_from_decoded_slices_and_normalises(monkeypatch):
    from merlot_reserve_amd import preprocess as P
    seen = {}

    def fake(waves, playback_speed=1, sr=22050, pad_size=2, device=None):
        seen['waves'], seen['sr'] = np.array(waves), sr
        return np.arange(waves.shape[0] * 3 * 60 * 65, dtype=np.float32).reshape(waves.shape[0], 3, 60, 65)
    monkeypatch.setattr(P, 'make_spectrograms', fake)
    rng = np.random.default_rng(0)
    frames = rng.integers(0, 256, (3, 10, 12, 3), dtype=np.uint8)
    wave = (rng.standard_normal(300000) * 9000).astype(np.int16)          # shorter than 3 segments from 2.5 s: zero-padded
    segs = P.segments_from_decoded(frames, wave, segment_start_time=2.5)
    assert [(s['start_time'], s['end_time'], s['mid_time'], s['idx']) for s in segs] == [(2.5, 7.5, 5.0, 0), (7.5, 12.5, 10.0, 1), (12.5, 17.5, 15.0, 2)]
    w = wave.astype('float32')
    w = w / max(np.abs(w).max(), 1.0)
    w = np.concatenate([w, np.zeros(int(22050 * 17.5) - w.size, dtype=np.float32)])
    assert seen['waves'].dtype == np.float32 and seen['waves'].shape == (3, 110250) and seen['sr'] == 22050
    for i, (a, b) in enumerate([(55125, 165375), (165375, 275625), (275625, 385875)]):
        assert (a, b) == (int(22050 * segs[i]['start_time']), int(22050 * segs[i]['end_time']))
        assert np.array_equal(seen['waves'][i], w[a:b])
        assert np.array_equal(segs[i]['frame'], frames[i]) and segs[i]['spectrogram'].shape == (3, 60, 65)
    assert np.all(seen['waves'][2][300000 - 275625:] == 0)
    # a quiet float waveform is not amplified: the divisor is max(|w|.max(), 1)
    P.segments_from_decoded(frames[:1], np.full(110250, 0.25, dtype=np.float64))
    assert np.all(seen['waves'] == np.float32(0.25))
    assert P.segments_from_decoded([], np.zeros(10)) == []


def test_make_spectrogram_rejects_a_wrong_length_before_any_launch():
    from merlot_reserve_amd import preprocess as P
    with pytest.raises(ValueError, match=r'provided mel spectrogram \(187, 65\). target size: \(188, 65\)'):
        P.make_spectrogram(np.zeros(110250 - 588 + 100, dtype=np.float32))
    with pytest.raises(ValueError, match=r'target size: \(192, 65\)'):
        P.make_spectrogram(np.zeros(110250, dtype=np.float32), pad_size=3)
    with pytest.raises(NotImplementedError):
        P.make_spectrogram(np.zeros(110250, dtype=np.float32), playback_speed=2)
    with pytest.raises(NotImplementedError, match='segments_from_decoded'):
        P.video_to_segments('clip.mp4')


def test_reference_names_are_reexported():
    import mreserve.preprocess as MP
    from merlot_reserve_amd import preprocess as P
    for name in ('make_spectrogram', 'make_spectrograms', 'preprocess_image_to_patches', 'segments_from_decoded', 'preprocess_video', 'video_to_segments'):
        assert getattr(MP, name) is getattr(P, name)
    with pytest.raises(AssertionError, match="didn't pretrain"):
        P.preprocess_image_to_patches(np.zeros((8, 8, 3), dtype=np.uint8), (25, 32))
    with pytest.raises(AssertionError, match="didn't pretrain"):
        P.preprocess_image_to_patches(np.zeros((8, 8, 3), dtype=np.uint8), (18, 33))


def test_preprocess_video_unchanged_on_the_inputs_it_took_before():
    """'patches', float 'frame' at the exact size and 'spectrogram' give the arrays computed here, byte for byte, as numpy."""
    from merlot_reserve_amd import preprocess as P
    from merlot_reserve_amd.planner import AUDIOSPAN
    rng = np.random.default_rng(3)
    frame = rng.random((32, 48, 3))                                       # float64 in: cast to float32, as before
    patches = rng.random((6, 768)).astype(np.float32)
    specs = [(rng.random((3, 60, 65)) * 5).astype(np.float32) for _ in range(2)]
    segs = [{'frame': frame, 'spectrogram': specs[0], 'use_text_as_input': False},
            {'patches': patches, 'text': [11, 12, 13]},
            {'patches': patches[::-1], 'spectrogram': specs[1].astype(np.float64), 'use_text_as_input': False}]
    out = P.preprocess_video(segs, (2, 3))
    assert all(isinstance(v, np.ndarray) for v in out.values())
    images = np.stack([ref_patchify(frame.astype(np.float32)), patches, patches[::-1]])
    audio = np.concatenate([specs[0], np.zeros((3, 60, 65), np.float32), specs[1]])
    tokens = [AUDIOSPAN] * 18 + [11, 12, 13] + [AUDIOSPAN] * 18
    idxs = [0] * 6 + [1] * 6 + [2] * 6 + [3] * 3 + [6] * 6 + [7] * 6 + [8] * 6
    assert out['images'].dtype == np.float32 and out['images'].tobytes() == images.tobytes()
    assert out['audio_clips'].dtype == np.float32 and out['audio_clips'].shape == (9, 60, 65) and out['audio_clips'].tobytes() == audio.tobytes()
    assert out['tokens'].dtype == np.int32 and out['tokens'].tolist() == tokens + [0] * (160 - len(tokens))
    assert out['subseg_idxs'].dtype == np.int32 and out['subseg_idxs'].tolist() == idxs + [-1] * (160 - len(idxs))


# ------------------------------------------------------------------------------------------------ the library
def test_media_library_exports_the_header_and_nothing_else():
    _built()
    from merlot_reserve_amd import _lib, _media_lib
    names = declared_symbols()
    assert names == ['mrm_frames_to_patches', 'mrm_last_error', 'mrm_logmel', 'mrm_logmel_frames', 'mrm_version']
    out = subprocess.check_output(['nm', '-D', '--defined-only', _media_lib.LIB_PATH], text=True)
    assert sorted(line.split()[-1] for line in out.splitlines() if line.strip()) == names
    assert set(_media_lib.PROTOTYPES) == set(names)
    assert not set(_media_lib.PROTOTYPES) & set(_lib.PROTOTYPES)
    lib = _media_lib.load()
    assert lib.mrm_version() >= 1
    # the other library carries none of these
    other = subprocess.check_output(['nm', '-D', '--defined-only', _lib.LIB_PATH], text=True)
    assert 'mrm_' not in other


def test_prototypes_match_the_header():
    """Argument counts and the C types of every parameter against the ctypes table."""
    from merlot_reserve_amd import _media_lib as M
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'mreserve_media.h')).read(), flags=re.S)
    ctype = {'int': M.i32, 'int32_t': M.i32, 'int64_t': M.i64, 'float': M.f32, 'const char*': ctypes.c_char_p}
    for ret, name, args in re.findall(r'^([a-z0-9_ ]+?\*?)\s*(mrm_[a-z0-9_]+)\s*\(([^)]*)\)\s*;', text, flags=re.M | re.S):
        res, argtypes = M.PROTOTYPES[name]
        assert res is ctype[ret.strip()], name
        params = [] if args.strip() == 'void' else [a.strip() for a in args.split(',')]
        assert len(params) == len(argtypes), name
        for p, t in zip(params, argtypes):
            want = M.vp if '*' in p else ctype[p.rsplit(' ', 1)[0].strip()]
            assert t is want, (name, p)


def test_bad_arguments_are_reported_without_a_launch():
    _built()
    from merlot_reserve_amd import _media_lib as M
    lib = M.load()
    p = 1 << 20                      # fake device addresses: never dereferenced, every case is rejected before a launch
    assert lib.mrm_logmel_frames(768) == 0 and lib.mrm_logmel_frames(769) == 2 and lib.mrm_logmel_frames(110250) == 188
    assert lib.mrm_logmel(p, 768, 1, 768, p, p, p, 1.0, p, M.DT_F32, None) == -1
    assert b'mrm_logmel' in lib.mrm_last_error() and b'769' in lib.mrm_last_error()
    assert lib.mrm_logmel(p, 7056, 1, 7056, p, None, p, 1.0, p, M.DT_F32, None) == -1 and b'null pointer' in lib.mrm_last_error()
    assert lib.mrm_logmel(p, 7056, 1, 7056, p, p, p, 1.0, p, 7, None) == -1 and b'out_dtype' in lib.mrm_last_error()
    assert lib.mrm_logmel(p, 7000, 2, 7056, p, p, p, 1.0, p, M.DT_BF16, None) == -1 and b'row stride' in lib.mrm_last_error()
    ok = (p, 1, 37, 53, 64, 96, p, p, 2, p, p, 2, p, M.DT_F32, None)

    def with_(i, v):
        return ok[:i] + (v,) + ok[i + 1:]
    assert lib.mrm_frames_to_patches(*with_(0, None)) == -1 and b'mrm_frames_to_patches: null pointer' in lib.mrm_last_error()
    assert lib.mrm_frames_to_patches(*with_(13, 2)) == -1 and b'out_dtype' in lib.mrm_last_error()
    assert lib.mrm_frames_to_patches(*with_(4, 60)) == -1 and b'multiples of 16' in lib.mrm_last_error()
    assert lib.mrm_frames_to_patches(*with_(8, 0)) == -1 and b'tap table' in lib.mrm_last_error()
    with pytest.raises(M.MreserveMediaError, match='tap table'):
        M.check(-1, 'mrm_frames_to_patches')


# which test file calls which export: (the Python names tests reach it by, the test files), in the style of test_cabi_test_ledger.py
HOST, GPU = 'test_media_host.py', 'test_media_gpu.py'
LEDGER = {
    'mrm_version': ((), (HOST,)),
    'mrm_last_error': ((), (HOST,)),
    'mrm_logmel_frames': ((), (HOST,)),
    'mrm_logmel': (('logmel',), (GPU, HOST)),
    'mrm_frames_to_patches': (('frames_to_patches',), (GPU, HOST)),
}


def test_every_media_export_names_its_test():
    assert set(LEDGER) == set(declared_symbols())
    binding = open(os.path.join(ROOT, 'merlot_reserve_amd', 'media.py')).read()
    for export, (wrappers, files) in LEDGER.items():
        assert files, export
        for w in wrappers:
            assert re.search(rf'^def {re.escape(w)}\b', binding, flags=re.M) and re.search(rf'\b{export}\b', binding), export
        for fname in files:
            text = open(os.path.join(ROOT, 'tests', fname)).read()
            assert any(re.search(rf'\b{re.escape(n)}\b', text) for n in (export,) + tuple(wrappers)), (export, fname)
    assert set(LEDGER) != set(declared_symbols()) | {'mrm_some_new_export'}


def test_build_scans_cover_the_media_library():
    _built()
    from merlot_reserve_amd import build as B
    assert B.MEDIA_HIP_FILES == ['media.hip'] and not set(B.MEDIA_SOURCES) & set(B.SOURCES)
    assert '-fno-slp-vectorize' in B.EXTRA_FLAGS['media.hip']
    if B._asm_stale():
        B.build(force=True, verbose=False)
    assert B.scan_packed_op_sel(files=B.MEDIA_HIP_FILES) == [] and B.scan_spills(files=B.MEDIA_HIP_FILES) == []
    res = B.kernel_resources(B.MEDIA_HIP_FILES)['media.hip']
    assert len(res) == 4 and all(e['vgpr_spill'] == 0 and e['scratch'] == 0 for e in res.values())
    asm = open(B._asm_path('media.hip')).read()
    assert 'v_mfma_f32_16x16x4_f32' in asm and not re.search(r'v_(sin|cos)_f32', asm)
