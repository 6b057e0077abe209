"""float64 numpy restatements of the two media transforms (no product code): librosa's melspectrogram as mreserve/preprocess.py:121-156 calls it,
and records.resize_and_pad(bilinear, antialiased, no random scale, no flip) followed by space_to_depth.  Explicit framing, np.fft.rfft,
scipy.signal.windows.hann."""
import numpy as np
import scipy.signal

N_FFT, HOP, N_BINS, N_MELS = 1536, 588, 769, 64


def ref_filterbank():
    def hz_to_mel(f):
        return 15.0 + np.log(f / 1000.0) / (np.log(6.4) / 27.0) if f >= 1000.0 else f / (200.0 / 3.0)

    def mel_to_hz(m):
        return np.where(m >= 15.0, 1000.0 * np.exp(np.log(6.4) / 27.0 * (m - 15.0)), m * (200.0 / 3.0))
    fftfreqs = np.linspace(0.0, 11025.0, N_BINS)
    mel_f = mel_to_hz(np.linspace(hz_to_mel(20.0), hz_to_mel(11025.0), N_MELS + 2))
    fb = np.zeros((N_MELS, N_BINS))
    for m in range(N_MELS):
        lower = (fftfreqs - mel_f[m]) / (mel_f[m + 1] - mel_f[m])
        upper = (mel_f[m + 2] - fftfreqs) / (mel_f[m + 2] - mel_f[m + 1])
        fb[m] = np.maximum(0.0, np.minimum(lower, upper)) * 2.0 / (mel_f[m + 2] - mel_f[m])
    return fb


def ref_logmel(wave, playback_speed=1.0):
    """wave [n, L] -> float64 [n, 1 + L // 588, 65]"""
    wave = np.asarray(wave, dtype=np.float64)
    n, L = wave.shape
    T = 1 + L // HOP
    j = np.arange(L + N_FFT) - N_FFT // 2
    r = np.where(j < 0, -j, np.where(j >= L, 2 * (L - 1) - j, j))
    p = wave[:, r]
    win = scipy.signal.windows.hann(N_FFT)
    frames = np.stack([p[:, HOP * t:HOP * t + N_FFT] for t in range(T)], 1) * win
    S = np.abs(np.fft.rfft(frames, axis=-1)) ** 2
    mel = S @ ref_filterbank().T
    out = np.empty((n, T, 65))
    out[..., :64] = np.log(mel + 0.1) - np.log(0.1)
    out[..., 64] = playback_speed
    return out


def _axis_matrix(a, b, out_len):
    """[out_len, a]: the normalised triangle filter from length a to length b; rows past min(b, out_len) are zero (padding)."""
    s = a / b
    sup = max(s, 1.0)
    M = np.zeros((out_len, a))
    for i in range(min(b, out_len)):
        c = (i + 0.5) * s
        lo, hi = max(int(c - sup + 0.5), 0), min(int(c + sup + 0.5), a)
        w = np.maximum(0.0, 1.0 - np.abs((np.arange(lo, hi) + 0.5 - c) / sup))
        M[i, lo:hi] = w / w.sum()
    return M


def ref_scaled_size(H, W, dh, dw):
    f32 = np.float32
    scale = min(f32(dw) / f32(W), f32(dh) / f32(H))
    return max(int(f32(H) * scale), 1), max(int(f32(W) * scale), 1)


def ref_resize_pad(img, dh, dw):
    """img float [H, W, 3] in [0, 1] -> float64 [dh, dw, 3]"""
    img = np.asarray(img, dtype=np.float64)
    H, W = img.shape[:2]
    sh, sw = ref_scaled_size(H, W, dh, dw)
    My, Mx = _axis_matrix(H, sh, dh), _axis_matrix(W, sw, dw)
    out = np.einsum('yh,hxc->yxc', My, np.einsum('hwc,xw->hxc', img, Mx, optimize=True), optimize=True)
    return np.clip(out, 0.0, 1.0)


def ref_patchify(img, P=16):
    """[h1 P, w1 P, 3] -> [h1 w1, P P 3]: (block row, block col) x (dy, dx, c)"""
    h1, w1 = img.shape[0] // P, img.shape[1] // P
    return img.reshape(h1, P, w1, P, 3).transpose(0, 2, 1, 3, 4).reshape(h1 * w1, P * P * 3)


def ref_frames_to_patches(frames_u8, grid):
    """uint8 [n, H, W, 3] -> float64 [n, h1 w1, 768]; the pixels are float32(u8) / float32(255), as records.py makes them"""
    dh, dw = 16 * grid[0], 16 * grid[1]
    return np.stack([ref_patchify(ref_resize_pad(f.astype(np.float32) / np.float32(255.0), dh, dw)) for f in frames_u8])


def bf16_bits(x):
    """float32 -> bf16 bit patterns, round to nearest even (finite input)"""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    return ((u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) >> np.uint32(16)).astype(np.uint16)
