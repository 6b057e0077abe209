"""float64 numpy restatements of the two ingest transforms (no product code): the Kaiser-windowed-sinc resampler to 22050 Hz, evaluated from the
continuous filter formula per output sample (it never reads the float32 polyphase table), and the black-bar bounds by numpy max / where."""
import math

import numpy as np

SR = 22050
ZERO_CROSSINGS, CUTOFF, BETA = 16, 0.97, 9.0


def ref_ratio(sr_in):
    g = math.gcd(sr_in, SR)
    L, M = SR // g, sr_in // g
    r = min(1.0, L / M)
    half = -((-ZERO_CROSSINGS * M) // L) if M > L else ZERO_CROSSINGS          # ceil(16 / min(1, L / M))
    return L, M, half, CUTOFF * r


def ref_kernel(t, half, c):
    """w(t) = c sinc(c t) I0(beta sqrt(1 - (t / half)^2)) / I0(beta) for |t| < half, else 0 (not normalised)"""
    t = np.asarray(t, dtype=np.float64)
    w = c * np.sinc(c * t) * np.i0(BETA * np.sqrt(np.maximum(0.0, 1.0 - (t / half) ** 2))) / np.i0(BETA)
    return np.where(np.abs(t) < half, w, 0.0)


def ref_downmix(x, channels_last=False):
    """[N], [C, N] (or [N, C] with channels_last) -> float64 [N]: the mean over channels"""
    x = np.asarray(x, dtype=np.float64)
    if x.ndim == 1:
        return x
    return x.mean(1 if channels_last else 0)


def ref_resample(m, sr_in, chunk=8192):
    """float64 [N] (or a batch [B, N]) at sr_in -> float64 [ceil(N L / M)] (or [B, ...]) at 22050 Hz; input outside [0, N) is 0; every output's
    taps are divided by their sum.  The weights depend on n only through (n M) mod L: with more outputs than phases they are evaluated once per
    phase, from the same formula."""
    m = np.asarray(m, dtype=np.float64)
    single = m.ndim == 1
    m = np.atleast_2d(m)
    N = m.shape[1]
    L, M, half, c = ref_ratio(sr_in)
    K = 2 * half
    n_out = -((-N * L) // M)
    off = np.arange(K) - half + 1
    pad = np.concatenate([np.zeros((m.shape[0], K)), m, np.zeros((m.shape[0], K))], 1)

    def weights(rem):
        w = ref_kernel(off[None, :] - (rem / L)[:, None], half, c)
        return w / w.sum(1, keepdims=True)
    per_phase = weights((np.arange(L, dtype=np.int64) * M) % L) if n_out >= L else None
    out = np.empty((m.shape[0], n_out))
    for a in range(0, n_out, chunk):
        n = np.arange(a, min(a + chunk, n_out), dtype=np.int64)
        w = per_phase[n % L] if per_phase is not None else weights((n * M) % L)
        idx = (n * M) // L
        idx = idx[:, None] + off[None, :] + K                         # into the padded signal
        assert idx.min() >= 0 and idx.max() < pad.shape[1]
        out[:, a:a + n.size] = np.einsum('nk,bnk->bn', w, pad[:, idx])
    return out[0] if single else out


def ref_bounds(frames, threshold):
    """uint8 [n, H, W, 3] -> (first row, last row, first column, last column) with max over frames and channels >= threshold; (H, -1, W, -1) if none"""
    has = frames.max(axis=(0, -1)) >= threshold
    H, W = has.shape
    ys, xs = np.where(has.any(1))[0], np.where(has.any(0))[0]
    if ys.size == 0:
        return H, -1, W, -1
    return int(ys[0]), int(ys[-1]), int(xs[0]), int(xs[-1])


def ref_detect_black_bars(frames, blackbar_threshold=16, max_perc_to_trim=.2):
    """The crop box of mreserve/preprocess.py:34-59 over ref_bounds: each side trimmed by at most int(size * max_perc_to_trim); with no content the
    middle row and column stand in for the content."""
    H, W = frames.shape[1:3]
    ya, yb, xa, xb = ref_bounds(frames, blackbar_threshold)
    if yb < 0:
        ya, yb, xa, xb = H // 2, H // 2, W // 2, W // 2
    return (min(ya, int(H * max_perc_to_trim)), max(yb + 1, int(H * (1 - max_perc_to_trim))),
            min(xa, int(W * max_perc_to_trim)), max(xb + 1, int(W * (1 - max_perc_to_trim))))


def bar_cases(n, H, W, thr=32):
    """{name: (frames uint8 [n, H, W, 3], threshold)}: the patterns of black bar every bounds test runs, host and GPU, scaled to the shape."""
    rng = np.random.default_rng(n * 1000003 + H * 1009 + W)

    def stack(y0, y1, x0, x1):
        f = rng.integers(0, thr, (n, H, W, 3), dtype=np.uint8) if thr > 0 else np.zeros((n, H, W, 3), np.uint8)      # bars are dark noise, not zeros
        f[:, y0:y1, x0:x1] = rng.integers(thr, 256, (n, y1 - y0, x1 - x0, 3), dtype=np.uint8)
        return f
    a, b = max(H // 8, 1 if H > 2 else 0), max(W // 8, 1 if W > 2 else 0)
    at = np.zeros((n, H, W, 3), np.uint8)
    at[n - 1, H // 2, W // 2, 1] = thr                                     # exactly at the threshold: counts
    below = np.full((n, H, W, 3), thr - 1, np.uint8)                       # one below everywhere: does not
    return {'letterbox': (stack(a, H - a, 0, W), thr), 'deep_letterbox': (stack(H // 3, H - H // 3 if H >= 3 else H, 0, W), thr),
            'pillarbox': (stack(0, H, b, W - b), thr), 'full': (stack(0, H, 0, W), thr), 'dark': (np.zeros((n, H, W, 3), np.uint8), thr),
            'at_threshold': (at, thr), 'below_threshold': (below, thr)}
