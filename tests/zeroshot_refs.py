"""float64 numpy restatements of the zero-shot head (no product code): logits from the inputs' exact values, np.argsort(-x, kind='stable'),
log-sum-exp in float64, and the group marginal as the literal walk of zero_shot_ek/zero_shot_eval_ek100.py:155-171 over the sorted list."""
import numpy as np


def exact_rows(rng, n, H):
    """[n, H] float32 with elements in {-4 .. 4} / 16: exact in bf16, and every dot product of up to 2048 terms is exact in fp32 in any order."""
    return (rng.integers(-4, 5, size=(n, H)).astype(np.float32) / np.float32(16.0))


def unit_rows(rng, n, H):
    x = rng.standard_normal((n, H))
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


def to_bf16_values(x):
    """float32 -> the float32 values of its round-to-nearest-even bf16"""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32)


def ref_logits64(queries, labels, scale):
    """float64 scale * queries @ labels.T from the exact values of the (float32-representable) inputs"""
    return np.float64(scale) * (np.asarray(queries, dtype=np.float64) @ np.asarray(labels, dtype=np.float64).T)


def round_f32(x64):
    """The correctly rounded float32 of each value, -0.0 as +0.0"""
    return np.asarray(x64, dtype=np.float64).astype(np.float32) + np.float32(0.0)


def ref_order(x):
    """Per row: the stable descending order, argsort(-logits)"""
    return np.argsort(-np.asarray(x), axis=-1, kind='stable')


def ref_topk(x, k):
    """(values [Q, k] of x's dtype, indices [Q, k] int32): stable descending; the tail for k > L is -inf / -1"""
    x = np.asarray(x)
    Q, L = x.shape
    order = ref_order(x)[:, :k]
    vals = np.full((Q, k), -np.inf, dtype=x.dtype)
    idx = np.full((Q, k), -1, dtype=np.int32)
    n = min(k, L)
    vals[:, :n] = np.take_along_axis(x, order, 1)[:, :n]
    idx[:, :n] = order[:, :n]
    return vals, idx


def ref_lse(x64):
    x64 = np.asarray(x64, dtype=np.float64)
    m = x64.max(-1, keepdims=True)
    return (m + np.log(np.exp(x64 - m).sum(-1, keepdims=True)))[:, 0]


def ref_group_walk(x, groups, k):
    """The reference's walk: go down the sorted label list, keep a label whose group has not been seen, stop at k groups.
    -> (values [Q, k], group ids [Q, k] int32, labels [Q, k] int32), tail -inf / -1 / -1"""
    x = np.asarray(x)
    Q, L = x.shape
    vals = np.full((Q, k), -np.inf, dtype=x.dtype)
    gids = np.full((Q, k), -1, dtype=np.int32)
    labs = np.full((Q, k), -1, dtype=np.int32)
    order = ref_order(x)
    for q in range(Q):
        seen = set()
        for i in order[q]:
            g = int(groups[i])
            if g in seen:
                continue
            r = len(seen)
            seen.add(g)
            vals[q, r], gids[q, r], labs[q, r] = x[q, i], g, i
            if len(seen) == k:
                break
    return vals, gids, labs


def ref_group_max(x, groups, G, k):
    """The definition: a group's score is the maximum of its labels, its representative the lowest-indexed label attaining it; the k best non-empty
    groups by score descending, then by lower representative.  Same return as ref_group_walk."""
    x = np.asarray(x)
    Q, L = x.shape
    vals = np.full((Q, k), -np.inf, dtype=x.dtype)
    gids = np.full((Q, k), -1, dtype=np.int32)
    labs = np.full((Q, k), -1, dtype=np.int32)
    for q in range(Q):
        best = {}
        for i in range(L):
            g = int(groups[i])
            assert 0 <= g < G
            if g not in best or x[q, i] > x[q, best[g]]:
                best[g] = i
        ranked = sorted(best.items(), key=lambda gi: (-x[q, gi[1]], gi[1]))[:k]
        for r, (g, i) in enumerate(ranked):
            vals[q, r], gids[q, r], labs[q, r] = x[q, i], g, i
    return vals, gids, labs


def lse_bound(L, lse64):
    """|lse - lse64| allowed: worst-case fp32 summation of L terms, plus a few ulps for the device exp / log and the final add"""
    return (L + 16) * 2.0 ** -24 + 2.0 ** -22 * np.maximum(1.0, np.abs(lse64))
