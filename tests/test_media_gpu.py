"""The media front end on the GPU (libmreserve_media.so): the log-mel and resize / patchify kernels against the float64 restatements of
tests/media_refs.py, batch independence and bf16 rounding bit for bit, and the plumbing through segments_from_decoded, preprocess_video and
embed_video."""
import functools

import numpy as np
import pytest
import torch

from media_refs import bf16_bits, ref_frames_to_patches, ref_logmel, ref_patchify

pytestmark = pytest.mark.gpu

LENGTHS = (769, 6568, 7056, 110250)          # T = 2 (nearly all reflection), 12, 13 (last frame's right half reflected), 188 (a 5 s segment)
SIGNALS = ('noise', 'quiet', 'tone', 'impulse0', 'impulse_end', 'zeros')
LOGMEL_BOUND = 1e-4          # the float32 CPU evaluation of the same matrix formulation stays within 1e-5 of float64 on these signals; 10x for another summation order
RESIZE_BOUND = 1e-5


@functools.lru_cache(maxsize=None)
def _signals(L):
    rng = np.random.default_rng(L)
    w = np.zeros((len(SIGNALS), L), dtype=np.float32)
    w[0] = rng.standard_normal(L) * 0.3
    w[1] = rng.standard_normal(L) * 1e-3                     # N(0, 1e-6)
    w[2] = np.sin(2 * np.pi * 440.0 * np.arange(L) / 22050.0)
    w[3, 0] = 1.0
    w[4, L - 1] = 1.0
    w.setflags(write=False)
    return w


@functools.lru_cache(maxsize=None)
def _logmel_ref(L):
    r = ref_logmel(_signals(L))
    r.setflags(write=False)
    return r


def _bits(t):
    return t.view(torch.int16).cpu().numpy().view(np.uint16) if t.dtype == torch.bfloat16 else t.cpu().numpy()


@pytest.mark.parametrize('L', LENGTHS)
def test_logmel_matches_the_float64_formula(dev, L):
    """Max abs error <= 1e-4 over noise N(0, 0.3^2), noise N(0, 1e-6), a 440 Hz unit tone, impulses at sample 0 and L - 1 and silence, in batches
    of 3 and 1; silence is exactly 0; every row of a batch equals the row run alone bit for bit; the bf16 output is the rounded float32 output.
    Measured on the MI355X (profiles/media_front_end.txt): maximum 7.13e-6 (the tone, at L >= 6568); noise 2.6e-6, quiet noise 3.4e-7, impulses 3.5e-7."""
    from merlot_reserve_amd import media
    sig, ref = _signals(L), _logmel_ref(L)
    T = 1 + L // 588
    if L == 110250:
        assert abs(ref[2, :, :64].max() - 10.38) < 0.01      # the tone's peak: the values the bound is relative to
    wave = torch.from_numpy(np.array(sig)).to(dev)
    got = torch.cat([media.logmel(wave[:3]), media.logmel(wave[3:])])
    assert got.shape == (6, T, 65) and got.dtype == torch.float32
    g = got.cpu().numpy()
    err = np.abs(g - ref).reshape(6, -1).max(1)
    print(f'logmel L={L} T={T}: max abs error per signal ' + ', '.join(f'{s} {e:.3g}' for s, e in zip(SIGNALS, err)))
    assert np.all(g[..., 64] == 1.0)
    assert np.all(g[5, :, :64] == 0.0), 'silence must come out exactly 0'
    assert err.max() <= LOGMEL_BOUND, dict(zip(SIGNALS, err))
    for i in range(6):                                       # batches of 1: the same bits as inside the batch
        alone = media.logmel(wave[i])
        assert alone.shape == (T, 65) and torch.equal(alone, got[i]), SIGNALS[i]
    shuffled = media.logmel(wave[[4, 0, 2]].contiguous())
    assert torch.equal(shuffled, got[[4, 0, 2]])
    strided = torch.zeros((3, L + 5), dtype=torch.float32, device=dev)
    strided[:, :L] = wave[:3]
    assert torch.equal(media.logmel(strided[:, :L]), got[:3])               # a row stride
    b = media.logmel(wave[:3], dtype=torch.bfloat16)
    assert b.dtype == torch.bfloat16 and np.array_equal(_bits(b), bf16_bits(g[:3]))
    out = torch.empty((3, T, 65), dtype=torch.float32, device=dev)
    assert media.logmel(wave[:3], out=out) is out and torch.equal(out, got[:3])
    assert torch.equal(media.logmel(np.array(sig[:2]), device=dev, playback_speed=1.0), got[:2])      # a host array is copied


def test_logmel_rejects_what_the_library_rejects(dev):
    from merlot_reserve_amd import media
    with pytest.raises(ValueError, match='too short'):
        media.logmel(torch.zeros(768, device=dev))
    with pytest.raises(TypeError):
        media.logmel(torch.zeros(769, device=dev), dtype=torch.float16)
    with pytest.raises(TypeError):
        media.logmel(torch.zeros(769, dtype=torch.float64, device=dev))


@functools.lru_cache(maxsize=None)
def _frames(n, H, W):
    f = np.random.default_rng(H * 31 + W).integers(0, 256, (n, H, W, 3), dtype=np.uint8)
    f.setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def _patches_ref(n, H, W, grid):
    r = ref_frames_to_patches(_frames(n, H, W), grid)
    r.setflags(write=False)
    return r


# (frames, H, W, grid, first padding row, first padding column)
RESIZE_CASES = [(2, 37, 53, (4, 6), 64, 91), (2, 200, 90, (4, 6), 64, 28), (2, 48, 48, (4, 6), 64, 64), (2, 90, 160, (4, 6), 54, 96),
                (2, 3, 500, (4, 6), 1, 96), (8, 360, 640, (12, 20), 180, 320), (8, 1080, 1920, (18, 32), 288, 512)]


@pytest.mark.parametrize('n,H,W,grid,pad_y,pad_x', RESIZE_CASES, ids=[f'{c[1]}x{c[2]}' for c in RESIZE_CASES])
def test_frames_to_patches_matches_the_float64_formula(dev, n, H, W, grid, pad_y, pad_x):
    """Max abs error <= 1e-5 against the float64 triangle filter on float32(u8) / 255; all padding exactly 0; a batch and its first frame alone
    agree bit for bit; the bf16 output is the rounded float32 output.  Measured on the MI355X: maximum 1.8e-7 (1080 x 1920 -> 288 x 512)."""
    from merlot_reserve_amd import media
    frames, ref = _frames(n, H, W), _patches_ref(n, H, W, grid)
    h1, w1 = grid
    dframes = torch.from_numpy(np.array(frames)).to(dev)
    got = media.frames_to_patches(dframes, grid)
    assert got.shape == (n, h1 * w1, 768) and got.dtype == torch.float32
    g = got.cpu().numpy()
    err = np.abs(g - ref).max()
    print(f'frames_to_patches {H}x{W} -> {16 * h1}x{16 * w1}: max abs error {err:.3g}')
    img = g.reshape(n, h1, w1, 16, 16, 3).transpose(0, 1, 3, 2, 4, 5).reshape(n, 16 * h1, 16 * w1, 3)
    assert np.all(img[:, pad_y:] == 0) and np.all(img[:, :, pad_x:] == 0), 'padding must be exactly 0'
    assert np.all(img[:, :pad_y, :pad_x].reshape(n, -1).max(1) > 0)
    assert err <= RESIZE_BOUND
    one = media.frames_to_patches(dframes[0], grid)
    assert one.shape == (h1 * w1, 768) and torch.equal(one, got[0])
    b = media.frames_to_patches(dframes, grid, dtype=torch.bfloat16)
    assert b.dtype == torch.bfloat16 and np.array_equal(_bits(b), bf16_bits(g))
    out = torch.empty_like(got)
    assert media.frames_to_patches(np.array(frames), grid, out=out, device=dev) is out and torch.equal(out, got)      # a host array is copied


def test_identity_size_is_patchify_of_u8_over_255(dev):
    from merlot_reserve_amd import media, records
    from merlot_reserve_amd.preprocess import patchify, preprocess_image_to_patches
    frame = _frames(1, 64, 96)[0]
    want = patchify(frame.astype(np.float32) / np.float32(255.0), (4, 6))
    assert np.array_equal(want, ref_patchify(frame.astype(np.float32) / np.float32(255.0)))
    got = media.frames_to_patches(torch.from_numpy(np.array(frame)).to(dev), (4, 6))
    assert np.array_equal(got.cpu().numpy(), want)
    b = media.frames_to_patches(torch.from_numpy(np.array(frame)).to(dev), (4, 6), dtype=torch.bfloat16)
    assert np.array_equal(_bits(b), patchify(records.u8_to_bf16_bits(frame).astype(np.float32), (4, 6)).astype(np.uint16))
    host = preprocess_image_to_patches(np.array(frame), (4, 6))
    assert isinstance(host, np.ndarray) and np.array_equal(host, want)


def test_plumbing_from_decoded_media_to_embed_video(dev):
    """Eight uint8 360 x 640 frames and 40 s of noise: segments_from_decoded -> preprocess_video(device=dev) -> embed_video.  What embed_video
    receives is what the stand-alone kernels give, bit for bit."""
    from merlot_reserve_amd import media
    from mreserve.modeling import PretrainedMerlotReserve
    from mreserve.preprocess import make_spectrogram, preprocess_video, segments_from_decoded
    grid = (12, 20)
    frames = _frames(8, 360, 640)
    wave = (np.random.default_rng(9).standard_normal(40 * 22050) * 3000).astype(np.int16)
    segs = segments_from_decoded(np.array(frames), wave, device=dev)
    assert len(segs) == 8 and all(s['spectrogram'].shape == (3, 60, 65) and s['spectrogram'].is_cuda for s in segs)
    for s in segs:
        s['use_text_as_input'] = False
    segs[0]['text'] = [5, 6, 7, 3]
    segs[0]['use_text_as_input'] = True
    pre = preprocess_video(segs, grid, device=dev)
    assert pre['images'].is_cuda and pre['audio_clips'].is_cuda and pre['images'].shape == (8, 240, 768) and pre['audio_clips'].shape == (24, 60, 65)
    assert torch.equal(pre['images'], media.frames_to_patches(torch.from_numpy(np.array(frames)).to(dev), grid))
    w = wave.astype(np.float32)
    w = (w / max(np.abs(w).max(), 1.0)).reshape(8, 110250)
    lm = media.logmel(torch.from_numpy(w).to(dev))
    clips = torch.stack([lm[:, 2:62], lm[:, 64:124], lm[:, 126:186]], 1)
    assert torch.all(pre['audio_clips'][:3] == 0) and torch.equal(pre['audio_clips'][3:], clips.reshape(24, 60, 65)[3:])
    # the host-returning forms and the 'waveform' key give the same bits
    host = make_spectrogram(w[1])
    assert isinstance(host, np.ndarray) and np.array_equal(host, clips[1].cpu().numpy())
    raw = [{'frame': frames[i], 'waveform': w[i], 'use_text_as_input': False} for i in range(2)]
    pre2 = preprocess_video(raw, grid)
    assert isinstance(pre2['images'], np.ndarray) and np.array_equal(pre2['images'], pre['images'][:2].cpu().numpy())
    assert isinstance(pre2['audio_clips'], np.ndarray) and np.array_equal(pre2['audio_clips'], clips[:2].reshape(6, 60, 65).cpu().numpy())
    model = PretrainedMerlotReserve.from_random('base', image_grid_size=grid, seed=0, device=dev)
    out = model.embed_video(**pre)
    assert out.shape == (160, 768) and torch.isfinite(out).all()
