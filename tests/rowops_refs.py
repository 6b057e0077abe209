"""fp64 references of the row kernels (csrc/layernorm.hip, csrc/rowops.hip) with the magnitude model that util.bound_report wants, and plain
torch-fp32 emulations of the kernels' formulas (tests/test_rowops_exact_checker.py proves the bound on them without a GPU).

Every reference returns (ref64, mag64) pairs.  `mag` is the result's formula with each summed term replaced by its absolute value; where a
sum feeds a later step its error is carried through to first order.  In units of u = 2^-24 an n-term fp32 sum is off by at most n u sum|term|;
bound_report allows n 2^-23 mag = twice that, which also pays for the few single roundings (products, one division) between the sums.

  LayerNorm forward     A = mean|x|, Q = mean x^2, v = Q - mean^2 + eps:  |d mean| <= n u A,  |d v| <= n u (Q + 2 |mean| A) <= 2 n u (Q + A^2),
                        d rstd = rstd d v / (2 v)  ->  mag_rstd = rstd (Q + A^2) / (2 v);   y = (x - mean) rstd gamma + beta  ->
                        mag_y = |gamma| (rstd A + |x - mean| mag_rstd)  +  |x - mean| rstd |gamma| + |beta|      (the last two: the plain roundings)
  LayerNorm backward    g = dy gamma, s1 = mean g, s2 = mean(g xhat):  mag_dx = rstd (|g| + mean|g| + |xhat| mean|g xhat|) + |dx_add|,
                        mag_dgamma = sum_rows |dy xhat|  (n = rows);  dbeta is exact on the integer dy the tests use
  attention pool        s_r = sum_64 (q / 8) k_r, S = max_r sum|q k_r| / 8:  p_r = softmax  ->  |d p_r| <= p_r (2 max|d s| + ...)  ->  mag_p = p_r (2 S + 1);
                        out = sum_r p_r v_r  ->  mag_out = sum_r (mag_p_r + p_r) |v_r|;  n = 64 + R everywhere.  Backward: dp_r = sum_64 dout v_r,
                        dot = sum_r p_r dp_r, ds_r = p_r (dp_r - dot) / 8:  mag_ds = p_r (sum|dout v_r| + sum_r p_r sum|dout v_r|) / 8,
                        mag_dq = sum_r mag_ds_r |k_r|, mag_dk = mag_ds_r |q|, dv = p_r dout is one product (mag = |dv|)
  unit-norm             ss = sum x^2 has positive terms only: inv = (ss + 1e-5)^-1/2 is off by n u / 2 relative, t = x inv by (n u + ...) |t|  ->  mag_t = |t|;
                        backward ndn = sum (x inv) dy:  mag_dx = inv temp (|dy| + |x inv| sum|x inv dy|),  mag_dls = temp / 2 sum_rows sum|x inv dy|
"""
import math

import torch

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
LN100_F32 = float(torch.tensor(4.605170185988092, dtype=F32))         # the kernels' clip of log_scale, as the fp32 constant they hold


# ------------------------------------------------------------------------------------------------------------------------ LayerNorm
def ln_fwd_ref(x, gamma, beta, eps=1e-5):
    """x [rows, H], gamma / beta [H] (bf16 values) -> {'y': [rows, H], 'mean': [1, rows], 'rstd': [1, rows]} of (ref64, mag64); n_terms = H."""
    xd, g, b = x.double(), gamma.double()[None], beta.double()[None]
    mean, Q, A = xd.mean(-1, keepdim=True), (xd * xd).mean(-1, keepdim=True), xd.abs().mean(-1, keepdim=True)
    v = Q - mean * mean + eps
    rstd = v.rsqrt()
    mag_rstd = rstd * (Q + A * A) / (2 * v)
    dev = (xd - mean).abs()
    y = (xd - mean) * (rstd * g) + b
    mag_y = g.abs() * (rstd * A + dev * mag_rstd) + dev * rstd * g.abs() + b.abs()
    return {'y': (y, mag_y), 'mean': (mean.T.contiguous(), A.T.contiguous()), 'rstd': (rstd.T.contiguous(), mag_rstd.T.contiguous())}


def ln_bwd_ref(dy, x, gamma, mean32, rstd32, dx_add=None):
    """mean32 / rstd32 [rows] fp32 are INPUTS of the backward (what the forward saved).  -> {'dx' (n = H), 'dgamma' [1, H] (n = rows), 'dbeta' [1, H]}."""
    d, xd, g = dy.double(), x.double(), gamma.double()[None]
    mu, rs = mean32.double()[:, None], rstd32.double()[:, None]
    xh, gg = (xd - mu) * rs, d * g
    s1, s2 = gg.mean(-1, keepdim=True), (gg * xh).mean(-1, keepdim=True)
    dx = rs * (gg - s1 - xh * s2)
    mag = rs.abs() * (gg.abs() + gg.abs().mean(-1, keepdim=True) + xh.abs() * (gg * xh).abs().mean(-1, keepdim=True))
    if dx_add is not None:
        dx, mag = dx + dx_add.double(), mag + dx_add.double().abs()
    return {'dx': (dx, mag), 'dgamma': ((d * xh).sum(0, keepdim=True), (d * xh).abs().sum(0, keepdim=True)),
            'dbeta': (d.sum(0, keepdim=True), d.abs().sum(0, keepdim=True))}


def ln_fwd_f32(x, gamma, beta, eps=1e-5):
    """The forward kernel's formulas in torch fp32: (y bf16, mean fp32, rstd fp32)."""
    xf, H = x.float(), x.shape[1]
    mean = xf.sum(-1, keepdim=True) / H
    var = (xf * xf).sum(-1, keepdim=True) / H - mean * mean
    rstd = torch.rsqrt(var + eps)
    return ((xf - mean) * (rstd * gamma.float()) + beta.float()).to(BF16), mean[:, 0], rstd[:, 0]


def ln_bwd_f32(dy, x, gamma, mean32, rstd32, dx_add=None):
    """The backward kernels' formulas in torch fp32: (dx bf16, dgamma bf16, dbeta bf16)."""
    d, xf, H = dy.float(), x.float(), x.shape[1]
    xh, gg = (xf - mean32[:, None]) * rstd32[:, None], d * gamma.float()
    s1, s2 = gg.sum(-1, keepdim=True) / H, (gg * xh).sum(-1, keepdim=True) / H
    o = rstd32[:, None] * (gg - s1 - xh * s2)
    if dx_add is not None:
        o = o + dx_add.float()
    return o.to(BF16), (d * xh).sum(0).to(BF16), d.sum(0).to(BF16)


# ------------------------------------------------------------------------------------------------------------------------ rows mean
def rows_mean_fwd_ref(src, rows):
    """src [n, H], rows [G, R] -> (mean of the R named rows [G, H], mag); n_terms = R + 2 (the sum, the rounded 1 / R, the product)."""
    s = src.double()[rows.long()]
    return s.mean(1), s.abs().mean(1)


def rows_mean_bwd_ref(ddst, rows, old):
    """dsrc[rows[g, r]] = old + ddst[g] / R, listed in the order of rows.reshape(-1): (ref [G * R, H], mag); n_terms = 3."""
    R = rows.shape[1]
    add = (ddst.double() / R).repeat_interleave(R, 0)
    o = old.double()[rows.long().reshape(-1)]
    return o + add, o.abs() + add.abs()


def rows_mean_fwd_f32(src, rows):
    R = rows.shape[1]
    return (src.float()[rows.long()].sum(1) * torch.tensor(1.0 / R, dtype=F32)).to(BF16)


# ------------------------------------------------------------------------------------------------------------------------ attention pool
def poolattn_fwd_ref(q, k, v, key_rows, nh):
    """q [G, H], k / v [n, H], key_rows [G, R] -> {'out': [G, H], 'probs': [G, nh * R]} of (ref64, mag64); n_terms = 64 + R."""
    G, R = key_rows.shape
    qd = q.double().reshape(G, 1, nh, 64)
    kd, vd = (t.double()[key_rows.long()].reshape(G, R, nh, 64) for t in (k, v))
    s = (qd * kd).sum(-1) / 8                                        # [G, R, nh]
    S = ((qd * kd).abs().sum(-1) / 8).amax(1, keepdim=True)
    p = torch.softmax(s, 1)
    mag_p = p * (2 * S + 1)
    out = (p[..., None] * vd).sum(1).reshape(G, nh * 64)
    mag_out = ((mag_p + p)[..., None] * vd.abs()).sum(1).reshape(G, nh * 64)
    as_gnr = lambda t: t.permute(0, 2, 1).reshape(G, nh * R)         # noqa: E731   (the kernel's probs layout [G, nh, R])
    return {'out': (out, mag_out), 'probs': (as_gnr(p), as_gnr(mag_p))}


def poolattn_bwd_ref(q, k, v, key_rows, probs32, dout, nh):
    """probs32 [G, nh, R] fp32 is an INPUT.  -> {'dq': [G, H], 'dk', 'dv': [G * R, H] in the order of key_rows.reshape(-1)}; n_terms = 64 + R."""
    G, R = key_rows.shape
    H = nh * 64
    qd, dd = q.double().reshape(G, 1, nh, 64), dout.double().reshape(G, 1, nh, 64)
    kd, vd = (t.double()[key_rows.long()].reshape(G, R, nh, 64) for t in (k, v))
    p = probs32.double().permute(0, 2, 1)[..., None]                 # [G, R, nh, 1]
    dp, dpa = (dd * vd).sum(-1, keepdim=True), (dd * vd).abs().sum(-1, keepdim=True)
    dot, dota = (p * dp).sum(1, keepdim=True), (p * dpa).sum(1, keepdim=True)
    ds, mag_ds = p * (dp - dot) / 8, p * (dpa + dota) / 8
    dv = p * dd
    return {'dq': ((ds * kd).sum(1).reshape(G, H), (mag_ds * kd.abs()).sum(1).reshape(G, H)),
            'dk': ((ds * qd).reshape(G * R, H), (mag_ds * qd.abs()).reshape(G * R, H)),
            'dv': (dv.reshape(G * R, H), dv.abs().reshape(G * R, H))}


def poolattn_fwd_f32(q, k, v, key_rows, nh):
    G, R = key_rows.shape
    qf = (q.float() * 0.125).reshape(G, 1, nh, 64)
    kf, vf = (t.float()[key_rows.long()].reshape(G, R, nh, 64) for t in (k, v))
    s = (qf * kf).sum(-1)
    e = torch.exp(s - s.amax(1, keepdim=True))
    p = e * (1.0 / e.sum(1, keepdim=True))
    return (p[..., None] * vf).sum(1).reshape(G, nh * 64).to(BF16), p.permute(0, 2, 1).contiguous()


def poolattn_bwd_f32(q, k, v, key_rows, probs32, dout, nh):
    G, R = key_rows.shape
    H = nh * 64
    qf, df = q.float().reshape(G, 1, nh, 64), dout.float().reshape(G, 1, nh, 64)
    kf, vf = (t.float()[key_rows.long()].reshape(G, R, nh, 64) for t in (k, v))
    p = probs32.permute(0, 2, 1)[..., None]
    dp = (df * vf).sum(-1, keepdim=True)
    ds = p * (dp - (p * dp).sum(1, keepdim=True)) * 0.125
    return (ds * kf).sum(1).reshape(G, H).to(BF16), (ds * qf).reshape(G * R, H).to(BF16), (p * df).reshape(G * R, H).to(BF16)


# ------------------------------------------------------------------------------------------------------------------------ unit-norm
def temperature(log_scale):
    return math.exp(min(float(log_scale), LN100_F32) / 2)


def unit_norm_fwd_ref(x, log_scale):
    """y = bf16(x inv) temp: the kernel rounds x inv to bf16 first (as unit_normalize does), so does this reference.  Where the fp64 x inv lies
    within the fp32 noise (n 2^-23 + 2^-14) |t| of a bf16 rounding boundary the intermediate may be either neighbour: -> (ref, alt_ref, mag = |ref|
    taken over both, inv [1, rows], mag_inv); n_terms for y is 1 (one product), for inv H."""
    xd, H = x.double(), x.shape[1]
    ss = (xd * xd).sum(-1, keepdim=True)
    inv = (ss + 1e-5).rsqrt()
    t = xd * inv
    tol = (H * 2.0 ** -23 + 2.0 ** -14) * t.abs()
    temp = temperature(log_scale)
    lo, hi = (t - tol).to(BF16).double() * temp, (t + tol).to(BF16).double() * temp
    return lo, hi, torch.maximum(lo.abs(), hi.abs()), inv.T.contiguous(), (inv / 2).T.contiguous()


def unit_norm_bwd_ref(x, log_scale, inv32, dy):
    """inv32 [rows] fp32 is an INPUT.  -> {'dx' (n = H), 'dls' [1, 1] (n = rows * H; exactly 0 at and above the clip)}."""
    xd, d, inv = x.double(), dy.double(), inv32.double()[:, None]
    temp = temperature(log_scale)
    n = xd * inv
    ndn, ndna = (n * d).sum(-1, keepdim=True), (n * d).abs().sum(-1, keepdim=True)
    dx, mag = inv * temp * (d - n * ndn), inv * temp * (d.abs() + n.abs() * ndna)
    on = 1.0 if float(log_scale) < LN100_F32 else 0.0
    return {'dx': (dx, mag), 'dls': (on * 0.5 * temp * ndn.sum().reshape(1, 1), on * 0.5 * temp * ndna.sum().reshape(1, 1))}


def unit_norm_fwd_f32(x, log_scale):
    xf = x.float()
    temp = torch.exp(torch.clamp(torch.tensor(float(log_scale), dtype=F32), max=LN100_F32) * 0.5)
    inv = 1.0 / torch.sqrt((xf * xf).sum(-1, keepdim=True) + 1e-5)
    return ((xf * inv).to(BF16).float() * temp).to(BF16), inv[:, 0]


def unit_norm_bwd_f32(x, log_scale, inv32, dy):
    xf, d, inv = x.float(), dy.float(), inv32[:, None]
    temp = torch.exp(torch.clamp(torch.tensor(float(log_scale), dtype=F32), max=LN100_F32) * 0.5)
    ndn = ((xf * inv) * d).sum(-1, keepdim=True)
    dls = 0.5 * temp * ndn.sum() if float(log_scale) < LN100_F32 else torch.zeros((), dtype=F32)
    return (inv * temp * (d - (xf * inv) * ndn)).to(BF16), dls.reshape(1, 1)


# ------------------------------------------------------------------------------------------------------------------------ shapes and data
# The (rows, H) / (G, R, nh) edges of the GPU file; each takes another path through a kernel (see the GPU file's docstrings).
LN_H = [8, 136, 512, 520, 1024, 1032, 2048]
LN_SMALL_ROWS = [1, 2, 7, 8, 9]
LN_CHECKER_SHAPES = [(9, 8), (7, 136), (2, 512), (9, 520), (8, 1024), (9, 1032), (1, 2048), (17, 136)]
POOL_CHECKER_SHAPES = [(1, 1, 1), (4, 5, 2), (5, 8, 8), (4, 5, 9), (1, 8, 12), (5, 1, 16)]          # (G, R, nh)
UNIT_CHECKER_SHAPES = [(1, 8), (4, 520), (5, 768)]
MEAN_CHECKER_SHAPES = [(1, 8), (4, 520), (5, 520)]                                                  # (G, H), R = 3
LOG_SCALES = [1.0, 4.59375, 4.625]                                                                  # 4.59375 < ln 100 < 4.625: bf16 neighbours


def rnd(shape, seed, scale=1.0, shift=0.0, device='cpu'):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale + shift).to(BF16).to(device)


def ln_inputs(rows, H, seed=0, device='cpu'):
    """x, gamma, beta (bf16 values) and the integer dy the backward tests want (util.sparse_int_rows: dbeta exact, every row visible in it)."""
    from util import sparse_int_rows
    return (rnd((rows, H), seed + 1, 2.0, 0.5, device), rnd((H,), seed + 2, 1.0, 1.0, device), rnd((H,), seed + 3, device=device),
            sparse_int_rows(rows, H, seed + 4, device=device))


def disjoint_rows(G, R, n, seed, device='cpu'):
    """[G, R] int32 row numbers below n, no row named twice (the kernels' contract: groups own their rows)."""
    g = torch.Generator().manual_seed(seed)
    return torch.randperm(n, generator=g)[:G * R].reshape(G, R).to(torch.int32).to(device)
