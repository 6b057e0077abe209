"""Media front end on the GPU (libmreserve_media.so, include/mreserve_media.h): the two numeric transforms between decoded media and
`MerlotReserve.embed_video` (mreserve/preprocess.py:121-156 and 464-481).

  logmel             waveform [n, L] -> log-mel rows [n, 1 + L // 588, 65]: librosa's melspectrogram as the reference calls it (n_fft 1536, hop 588,
                     symmetric Hann, reflect padding, Slaney filterbank of 64 mels over 20 .. 11025 Hz), log(mel + 0.1) - log(0.1), playback speed
                     as column 64
  frames_to_patches  uint8 frames [n, H, W, 3] of any size -> [n, h w, 768]: records.resize_and_pad (bilinear with antialiasing, no random scale,
                     no flip, zero padding) and space_to_depth in one pass

The tables (window, twiddles, filterbank, filter taps) are made here in float64, rounded once to float32 and uploaded once per device.  File
decoding (ffmpeg) stays outside the package; PCM resampling and black-bar trimming are merlot_reserve_amd.ingest."""
import numpy as np
import torch

from . import _media_lib

N_FFT, HOP, N_BINS, N_MELS, SR = 1536, 588, 769, 64, 22050
FMIN, FMAX = 20.0, 11025.0
PATCH = 16


# ------------------------------------------------------------------------------------------------ tables (float64)
def hann_window():
    """scipy.signal.windows.hann(1536): the SYMMETRIC window (librosa calls the callable the reference passes with its default sym=True)."""
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(N_FFT, dtype=np.float64) / (N_FFT - 1))


def twiddle_table():
    """[2, 1536]: cos(2 pi i / 1536), sin(2 pi i / 1536); the kernel looks them up at (n k) mod 1536."""
    a = 2.0 * np.pi * np.arange(N_FFT, dtype=np.float64) / N_FFT
    return np.stack([np.cos(a), np.sin(a)])


def hz_to_mel(f):
    """Slaney: linear at 200 / 3 Hz per mel below 1000 Hz, logarithmic with step ln(6.4) / 27 above."""
    f = np.asarray(f, dtype=np.float64)
    return np.where(f >= 1000.0, 15.0 + np.log(np.maximum(f, 1e-300) / 1000.0) / (np.log(6.4) / 27.0), f * 3.0 / 200.0)


def mel_to_hz(m):
    m = np.asarray(m, dtype=np.float64)
    return np.where(m >= 15.0, 1000.0 * np.exp((np.log(6.4) / 27.0) * (m - 15.0)), m * 200.0 / 3.0)


def mel_filterbank():
    """[64, 769] float64: librosa.filters.mel(sr=22050, n_fft=1536, n_mels=64, fmin=20, fmax=11025), Slaney scale and normalisation."""
    fftfreqs = np.linspace(0.0, SR / 2.0, N_BINS)
    mel_f = mel_to_hz(np.linspace(hz_to_mel(FMIN), hz_to_mel(FMAX), N_MELS + 2))
    fdiff = np.diff(mel_f)
    ramps = mel_f[:, None] - fftfreqs[None, :]
    lower = -ramps[:-2] / fdiff[:-1, None]
    upper = ramps[2:] / fdiff[1:, None]
    return np.maximum(0.0, np.minimum(lower, upper)) * (2.0 / (mel_f[2:] - mel_f[:-2]))[:, None]


def logmel_frames(L):
    """Rows of the spectrogram of L samples (centred frames)."""
    return 1 + int(L) // HOP


def resize_geometry(H, W, dh, dw):
    """(sh, sw): the size records.resize_and_pad scales an [H, W] frame to for a [dh, dw] output without random scale, in its float32 arithmetic."""
    f32 = np.float32
    scale = min(f32(dw) / f32(float(W)), f32(dh) / f32(float(H)))
    return max(int(f32(float(H)) * scale), 1), max(int(f32(float(W)) * scale), 1)


def resample_taps(a, b):
    """The antialiased triangle filter from length a to length b: [(first input index, float64 weights normalised over the in-range taps)] per output."""
    s = a / b
    sup = max(s, 1.0)
    taps = []
    for i in range(b):
        c = (i + 0.5) * s
        lo, hi = max(int(c - sup + 0.5), 0), min(int(c + sup + 0.5), a)
        w = np.maximum(0.0, 1.0 - np.abs((np.arange(lo, hi) + 0.5 - c) / sup))
        taps.append((lo, w / w.sum()))
    return taps


def tap_tables(a, b, out_len):
    """(range int32 [out_len, 2], weights float32 [out_len, k]) for mrm_frames_to_patches: outputs past min(b, out_len) have no taps (padding); taps of
    weight exactly zero at either end of a range are dropped."""
    taps = resample_taps(a, b)[:out_len]
    rng = np.zeros((out_len, 2), dtype=np.int32)
    rows = []
    for i, (lo, w) in enumerate(taps):
        nz = np.nonzero(w)[0]
        first, last = int(nz[0]), int(nz[-1]) + 1
        rng[i] = (lo + first, last - first)
        rows.append(w[first:last])
    k = max(len(r) for r in rows)
    wts = np.zeros((out_len, k), dtype=np.float32)
    for i, r in enumerate(rows):
        wts[i, :len(r)] = r
    return rng, wts


# ------------------------------------------------------------------------------------------------ device side
_DT = {torch.float32: _media_lib.DT_F32, torch.bfloat16: _media_lib.DT_BF16}
_mel_tables = {}
_tap_cache = {}


def _device(x, device):
    if device is not None:
        return torch.device(device)
    if isinstance(x, torch.Tensor) and x.is_cuda:
        return x.device
    return torch.device('cuda', torch.cuda.current_device())


def _to_device(x, dtype, dev):
    """Device tensors pass through; host arrays (and host tensors) are copied."""
    if not isinstance(x, torch.Tensor):
        x = torch.from_numpy(np.ascontiguousarray(np.asarray(x)))
    if x.dtype != dtype:
        raise TypeError(f'expected {dtype}, got {x.dtype}')
    return x.to(dev)


def _check_out(out, shape, dtype, dev):
    if out is None:
        return torch.empty(shape, dtype=dtype, device=dev)
    if tuple(out.shape) != tuple(shape) or out.dtype != dtype or out.device != dev or not out.is_contiguous():
        raise ValueError(f'out must be a contiguous {dtype} tensor of shape {tuple(shape)} on {dev}')
    return out


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def logmel(wave, out=None, dtype=torch.float32, playback_speed=1.0, device=None):
    """wave float32 [n, L] (or [L]) -> [n, 1 + L // 588, 65] (or [T, 65]) on the device, `dtype` float32 or bfloat16.  L >= 769."""
    if dtype not in _DT:
        raise TypeError(f'dtype must be torch.float32 or torch.bfloat16, got {dtype}')
    dev = _device(wave, device)
    w = _to_device(wave, torch.float32, dev)
    single = w.dim() == 1
    if single:
        w = w[None]
    if w.dim() != 2:
        raise ValueError(f'wave must be [n, L] or [L], got {tuple(w.shape)}')
    if w.stride(1) != 1:
        w = w.contiguous()
    n, L = w.shape
    if L < N_BINS:
        raise ValueError(f'a waveform of {L} samples is too short: reflect padding by {N_FFT // 2} needs at least {N_BINS}')
    T = logmel_frames(L)
    res = _check_out(out, (T, 65) if single else (n, T, 65), dtype, dev)
    if dev not in _mel_tables:
        _mel_tables[dev] = tuple(torch.from_numpy(np.ascontiguousarray(t, dtype=np.float32)).to(dev)
                                 for t in (hann_window(), twiddle_table(), mel_filterbank()))
    win, tw, fb = _mel_tables[dev]
    lib = _media_lib.load()
    with torch.cuda.device(dev):
        _media_lib.check(lib.mrm_logmel(w.data_ptr(), w.stride(0) if n > 1 else L, n, L, win.data_ptr(), tw.data_ptr(), fb.data_ptr(),
                                        float(playback_speed), res.data_ptr(), _DT[dtype], _stream(dev)), 'mrm_logmel')
    return res


def frames_to_patches(frames, output_grid_size, out=None, dtype=torch.float32, device=None):
    """frames uint8 [n, H, W, 3] (or [H, W, 3]), any H, W -> [n, h1 w1, 768] (or [h1 w1, 768]) on the device: scaled to fit (16 h1, 16 w1)
    keeping the aspect ratio, zero-padded below / to the right, in the patch order of preprocess.patchify."""
    if dtype not in _DT:
        raise TypeError(f'dtype must be torch.float32 or torch.bfloat16, got {dtype}')
    h1, w1 = int(output_grid_size[0]), int(output_grid_size[1])
    if h1 < 1 or w1 < 1:
        raise ValueError(f'bad output grid {output_grid_size}')
    dev = _device(frames, device)
    f = _to_device(frames, torch.uint8, dev)
    single = f.dim() == 3
    if single:
        f = f[None]
    if f.dim() != 4 or f.shape[3] != 3 or f.shape[1] < 1 or f.shape[2] < 1:
        raise ValueError(f'frames must be uint8 [n, H, W, 3] or [H, W, 3], got {tuple(f.shape)}')
    f = f.contiguous()
    n, H, W, _ = f.shape
    dh, dw = h1 * PATCH, w1 * PATCH
    res = _check_out(out, (h1 * w1, 768) if single else (n, h1 * w1, 768), dtype, dev)
    key = (H, W, dh, dw, dev)
    if key not in _tap_cache:
        if len(_tap_cache) >= 16:
            _tap_cache.clear()
        sh, sw = resize_geometry(H, W, dh, dw)
        yr, yw = tap_tables(H, sh, dh)
        xr, xw = tap_tables(W, sw, dw)
        _tap_cache[key] = tuple(torch.from_numpy(t).to(dev) for t in (yr, yw, xr, xw))
    yr, yw, xr, xw = _tap_cache[key]
    lib = _media_lib.load()
    with torch.cuda.device(dev):
        _media_lib.check(lib.mrm_frames_to_patches(f.data_ptr(), n, H, W, dh, dw, yr.data_ptr(), yw.data_ptr(), yw.shape[1], xr.data_ptr(),
                                                   xw.data_ptr(), xw.shape[1], res.data_ptr(), _DT[dtype], _stream(dev)), 'mrm_frames_to_patches')
    return res
