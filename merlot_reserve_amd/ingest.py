"""Media ingest on the GPU (libmreserve_ingest.so, include/mreserve_ingest.h): decoded media as decoders hand it out -> what
`preprocess.segments_from_decoded` and `media` take.  The two steps the reference leaves to ffmpeg's `-ac 1 -ar 22050` and to
`_detect_black_bars_from_video` (mreserve/preprocess.py:34-59, 115-118, 216-217, 290-291):

  resample_mono      PCM of any integer rate from 4 to 192 kHz, int16 or float32, [N], [C, N] or [N, C] -> mono float32 at 22050 Hz and its peak
  content_bounds     uint8 frames [n, H, W, 3] -> first / last row and column holding a value >= threshold
  detect_black_bars  the reference's function over content_bounds;  trim_black_bars  the crop, as a view
  read_wav           16-bit PCM files through the stdlib `wave` module

The resampling filter is a Kaiser-windowed sinc of our own design, close to libswresample's documented defaults (filter size 32, cut-off 0.97,
Kaiser beta 9) -- what the reference's ffmpeg call ran -- but NOT a restatement of that library, which is not bit-defined: parity is against the
float64 evaluation of the formulas below (tests/ingest_refs.py).  The polyphase table is made here in float64, rounded once to float32 and
uploaded once per rate and device."""
import math

import numpy as np
import torch

from . import _ingest_lib

SR = 22050
ZERO_CROSSINGS = 16          # half-width of the filter in zero crossings at the lower of the two rates
CUTOFF = 0.97                # of the lower Nyquist frequency
KAISER_BETA = 9.0
SR_MIN, SR_MAX = 4000, 192000

_tables = {}
_device_tables = {}


# ------------------------------------------------------------------------------------------------ the filter (float64)
def resample_ratio(sr_in):
    """(L, M): output sample n sits at input time n M / L."""
    if isinstance(sr_in, bool) or not isinstance(sr_in, (int, np.integer)) or not SR_MIN <= sr_in <= SR_MAX:
        raise ValueError(f'the sample rate must be an integer from {SR_MIN} to {SR_MAX} Hz, got {sr_in!r}')
    g = math.gcd(int(sr_in), SR)
    return SR // g, int(sr_in) // g


def resample_table(sr_in):
    """(L, M, K, taps float32 [L, K]).  half = ceil(16 / min(1, L / M)), K = 2 half, c = 0.97 min(1, L / M); phase p = n mod L has
    frac = ((p M) mod L) / L and tap j sits at t = (j - half + 1) - frac from floor(n M / L):
        w = c sinc(c t) I0(beta sqrt(1 - (t / half)^2)) / I0(beta)   for |t| < half, else 0
    each phase row divided by its float64 sum (DC gain = the rounding of 1)."""
    L, M = resample_ratio(sr_in)
    if sr_in not in _tables:
        half = 16 if L >= M else -((-ZERO_CROSSINGS * M) // L)
        K = 2 * half
        c = CUTOFF * min(1.0, L / M)
        frac = ((np.arange(L, dtype=np.int64) * M) % L).astype(np.float64) / L
        t = (np.arange(K, dtype=np.float64) - half + 1)[None, :] - frac[:, None]
        w = c * np.sinc(c * t) * np.i0(KAISER_BETA * np.sqrt(np.maximum(0.0, 1.0 - (t / half) ** 2))) / np.i0(KAISER_BETA)
        w[np.abs(t) >= half] = 0.0
        w /= w.sum(1, keepdims=True)
        taps = w.astype(np.float32)
        taps.setflags(write=False)
        if len(_tables) >= 8:
            _tables.clear()
            _device_tables.clear()
        _tables[sr_in] = (L, M, K, taps)
    return _tables[sr_in]


def resample_len(N, sr_in):
    """Output samples of N input samples: ceil(N L / M)."""
    L, M = resample_ratio(sr_in)
    return -((-int(N) * L) // M)


# ------------------------------------------------------------------------------------------------ device side
def _device(x, device):
    if device is not None:
        return torch.device(device)
    if isinstance(x, torch.Tensor) and x.is_cuda:
        return x.device
    return torch.device('cuda', torch.cuda.current_device())


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def _pcm_tensor(pcm, dev):
    """numpy / torch, int16 / float32 (float64 host arrays are cast) -> a tensor on `dev`; device tensors pass through with their strides."""
    if not isinstance(pcm, torch.Tensor):
        a = np.asarray(pcm)
        if a.dtype == np.float64:
            a = a.astype(np.float32)
        if a.dtype not in (np.int16, np.float32):
            raise TypeError(f'PCM must be int16 or float32, got {a.dtype}')
        pcm = torch.from_numpy(np.ascontiguousarray(a))
    if pcm.dtype not in (torch.int16, torch.float32):
        raise TypeError(f'PCM must be int16 or float32, got {pcm.dtype}')
    return pcm.to(dev)


def _channel_view(x, channels_last):
    """-> x as [C, N] (a view)"""
    if x.dim() == 1:
        return x[None]
    if x.dim() != 2:
        raise ValueError(f'PCM must be [N], [C, N] or [N, C], got {tuple(x.shape)}')
    if channels_last is None:
        if x.shape[0] == x.shape[1]:
            raise ValueError(f'PCM of shape {tuple(x.shape)}: cannot tell channels from samples, pass channels_last')
        channels_last = x.shape[1] < x.shape[0]
    return x.t() if channels_last else x


def resample_mono(pcm, sr, channels_last=None, device=None):
    """-> (wave float32 [ceil(N L / M)] on the device, peak = max |wave| as a 0-dim float32 tensor there).  Channels are averaged in float32
    (sum in channel order, a true division); `channels_last=None` takes the shorter axis of a 2-D input as the channels.  sr == 22050 launches
    nothing: the downmix and the peak come from torch, so the identity is exact.  A NaN sample gives NaNs around it and a NaN peak."""
    L, M, K, taps = resample_table(sr)
    dev = _device(pcm, device)
    x = _channel_view(_pcm_tensor(pcm, dev), channels_last)
    C, N = x.shape
    if N < 1 or C < 1:
        raise ValueError(f'empty PCM {tuple(x.shape)}')
    if sr == SR:
        m = x[0].to(torch.float32)
        for c in range(1, C):
            m = m + x[c].to(torch.float32)
        m = (m / torch.full((), float(C), dtype=torch.float32, device=dev)).contiguous()      # by a tensor: torch turns a Python divisor into a reciprocal
        return m, m.abs().max()
    key = (sr, dev)
    if key not in _device_tables:
        _device_tables[key] = torch.from_numpy(taps).to(dev)
    dtaps = _device_tables[key]
    lib = _ingest_lib.load()
    n_out = lib.mri_resample_len(N, L, M)
    y = torch.empty(n_out, dtype=torch.float32, device=dev)
    peak = torch.zeros(1, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _ingest_lib.check(lib.mri_resample_mono(x.data_ptr(), _ingest_lib.DT_S16 if x.dtype == torch.int16 else _ingest_lib.DT_F32, C, N,
                                                x.stride(0) if C > 1 else max(N, 1), x.stride(1) if N > 1 else 1, dtaps.data_ptr(), L, M, K,
                                                y.data_ptr(), peak.data_ptr(), _stream(dev)), 'mri_resample_mono')
    return y, peak.view(torch.float32)[0]


def content_bounds(frames, threshold, device=None):
    """frames uint8 [n, H, W, 3] (or [H, W, 3]) -> (y_first, y_last, x_first, x_last) of the pixels whose maximum over frames and channels is
    >= threshold (an integer 0 .. 255), as Python ints: one 16-byte copy back, the only synchronisation.  (H, -1, W, -1) when nothing is."""
    dev = _device(frames, device)
    f = frames if isinstance(frames, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(frames)))
    if f.dtype != torch.uint8:
        raise TypeError(f'expected uint8 frames, got {f.dtype}')
    if f.dim() == 3:
        f = f[None]
    if f.dim() != 4 or f.shape[3] != 3 or min(f.shape[:3]) < 1:
        raise ValueError(f'frames must be uint8 [n, H, W, 3] or [H, W, 3], got {tuple(f.shape)}')
    f = f.to(dev).contiguous()
    n, H, W, _ = f.shape
    bounds = torch.tensor([H, -1, W, -1], dtype=torch.int32, device=dev)
    lib = _ingest_lib.load()
    with torch.cuda.device(dev):
        _ingest_lib.check(lib.mri_content_bounds(f.data_ptr(), n, H, W, int(threshold), bounds.data_ptr(), _stream(dev)), 'mri_content_bounds')
    return tuple(bounds.tolist())


def detect_black_bars(frames, blackbar_threshold=16, max_perc_to_trim=.2, device=None):
    """_detect_black_bars_from_video (preprocess.py:34-59) -> (y1, y2, x1, x2): the content box, each side trimmed by at most
    int(size * max_perc_to_trim); with no content at all the middle row and column stand in, as there."""
    h, w = frames.shape[-3], frames.shape[-2]
    thr = max(int(math.ceil(blackbar_threshold)), 0)
    ya, yb, xa, xb = content_bounds(frames, thr, device=device) if thr <= 255 else (h, -1, w, -1)
    if yb < 0:
        ya = yb = h // 2
    if xb < 0:
        xa = xb = w // 2
    y1 = min(ya, int(h * max_perc_to_trim))
    y2 = max(yb + 1, int(h * (1 - max_perc_to_trim)))
    x1 = min(xa, int(w * max_perc_to_trim))
    x2 = max(xb + 1, int(w * (1 - max_perc_to_trim)))
    return y1, y2, x1, x2


def trim_black_bars(frames, blackbar_threshold=32, max_perc_to_trim=.2, device=None):
    """frames [n, H, W, 3] -> frames[:, y1:y2, x1:x2], a view (numpy or torch) -- the crop of extract_frames_from_video (preprocess.py:83,
    116-118, whose threshold 32 is the default here).  media.frames_to_patches makes a stacked batch contiguous on the device itself."""
    y1, y2, x1, x2 = detect_black_bars(frames, blackbar_threshold=blackbar_threshold, max_perc_to_trim=max_perc_to_trim, device=device)
    return frames[:, y1:y2, x1:x2]


def read_wav(path):
    """-> (int16 [N, C], sample rate) of a 16-bit PCM file, through the stdlib `wave` module."""
    import wave
    with wave.open(str(path), 'rb') as f:
        if f.getsampwidth() != 2:
            raise ValueError(f'{path}: only 16-bit PCM is read, this file has {8 * f.getsampwidth()}-bit samples')
        C, sr = f.getnchannels(), f.getframerate()
        data = f.readframes(f.getnframes())
    return np.frombuffer(data, dtype='<i2').reshape(-1, C).astype(np.int16, copy=False), sr
