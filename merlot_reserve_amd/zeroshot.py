"""The zero-shot head on the GPU (libmreserve_zeroshot.so, include/mreserve_zeroshot.h): what demo/demo_video.py:43-50,
zero_shot_ek/zero_shot_eval_ek100.py:146-192 and zero_shot_qa/inference.py:55-69 all end with --

    logits = 100 * out_h[tokens == MASK] @ get_label_space(options).T;  softmax;  argsort(-logits)

  score_topk          one fused call: the k best labels per query (value descending, lower index first among equal values: a stable
                      argsort), log-sum-exp, optionally every logit, optionally the k best label groups (verb / noun of an action table)
  ZeroShotClassifier  encodes the label table ONCE, embeds videos in batches, scores every <|MASK|> row, keeps the accuracy books of the two
                      evaluation scripts

Determinism: no float atomics, a fixed reduction order, and a split of the labels that depends on their number only -- a query row's
outputs are bit-identical whatever the batch is and wherever the row sits in it."""
import numpy as np
import torch

from . import _zeroshot_lib
from .preprocess import MASK

SLICE_LABELS = _zeroshot_lib.SLICE          # labels per workgroup: L is cut at multiples of this, the partial results merged by a second launch
MAX_K = _zeroshot_lib.MAX_K

_DT = {torch.float32: _zeroshot_lib.DT_F32, torch.bfloat16: _zeroshot_lib.DT_BF16}


class ScoreResult:
    """values / indices [Q, k] (fp32 / int32; tail -inf / -1 for k > L), lse [Q]; logits [Q, L] or None; group_values / group_ids /
    group_labels [Q, k] or None (score, group, representative label).  Probability = exp(value - lse)."""
    __slots__ = ('values', 'indices', 'lse', 'logits', 'group_values', 'group_ids', 'group_labels')

    def __init__(self, values, indices, lse, logits=None, group_values=None, group_ids=None, group_labels=None):
        self.values, self.indices, self.lse, self.logits = values, indices, lse, logits
        self.group_values, self.group_ids, self.group_labels = group_values, group_ids, group_labels

    @property
    def probs(self):
        return torch.exp(self.values - self.lse[:, None])

    @property
    def group_probs(self):
        return None if self.group_values is None else torch.exp(self.group_values - self.lse[:, None])


def _rows(x, name):
    if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dim() == 2):
        raise TypeError(f'{name} must be a 2-d device tensor')
    if x.dtype not in _DT:
        raise TypeError(f'{name} must be float32 or bfloat16, got {x.dtype}')
    if x.stride(1) != 1 or (x.stride(0) * x.element_size()) % 16 or x.data_ptr() % 16 or (x.shape[0] > 1 and x.stride(0) < x.shape[1]):
        x = x.contiguous()
    return x


def score_topk(queries, labels, k, scale=100.0, groups=None, num_groups=None, return_logits=False):
    """queries [Q, H] x labels [L, H] (device tensors, float32 or bfloat16 each) -> ScoreResult.  `groups` [L] int32 (each in [0, num_groups)) adds
    the group outputs; `num_groups` defaults to groups.max() + 1, which reads the device.  Allocates outputs and scratch, launches on the
    current stream, nothing else."""
    q, lab = _rows(queries, 'queries'), _rows(labels, 'labels')
    if q.device != lab.device or q.shape[1] != lab.shape[1]:
        raise ValueError(f'queries {tuple(q.shape)} on {q.device} and labels {tuple(lab.shape)} on {lab.device} do not match')
    dev = q.device
    (Q, H), L, k = q.shape, lab.shape[0], int(k)
    G, gptr = 0, None
    if groups is not None:
        groups = torch.as_tensor(groups).to(device=dev, dtype=torch.int32).contiguous()
        if groups.shape != (L,):
            raise ValueError(f'groups must have shape ({L},), got {tuple(groups.shape)}')
        G = int(num_groups) if num_groups is not None else int(groups.max()) + 1
        gptr = groups.data_ptr()
    lib = _zeroshot_lib.load()
    nbytes = lib.mrz_workspace_bytes(Q, L, G, k)
    if nbytes < 0:
        _zeroshot_lib.check(int(nbytes), 'mrz_workspace_bytes')
    f32 = dict(dtype=torch.float32, device=dev)
    i32 = dict(dtype=torch.int32, device=dev)
    res = ScoreResult(torch.empty((Q, k), **f32), torch.empty((Q, k), **i32), torch.empty((Q,), **f32))
    if return_logits:
        res.logits = torch.empty((Q, L), **f32)
    if groups is not None:
        res.group_values, res.group_ids, res.group_labels = torch.empty((Q, k), **f32), torch.empty((Q, k), **i32), torch.empty((Q, k), **i32)
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev) if nbytes else None

    def ptr(t):
        return None if t is None else t.data_ptr()
    with torch.cuda.device(dev):
        _zeroshot_lib.check(lib.mrz_score_topk(q.data_ptr(), q.stride(0) if Q > 1 else H, _DT[q.dtype], lab.data_ptr(), lab.stride(0) if L > 1 else H,
                                               _DT[lab.dtype], Q, L, H, float(scale), k, res.values.data_ptr(), res.indices.data_ptr(),
                                               res.lse.data_ptr(), ptr(res.logits), gptr, G, ptr(res.group_values), ptr(res.group_ids),
                                               ptr(res.group_labels), ptr(ws), torch.cuda.current_stream(dev).cuda_stream), 'mrz_score_topk')
    return res


# ------------------------------------------------------------------------------------------------ accuracy books (host, no GPU)
def _as_ids(values):
    """A group map given as ids or as strings -> (int32 ids, names or None); strings are numbered in order of first appearance."""
    values = list(values)
    if values and isinstance(values[0], str):
        names = list(dict.fromkeys(values))
        index = {n: i for i, n in enumerate(names)}
        return np.array([index[v] for v in values], dtype=np.int32), names
    return np.asarray(values, dtype=np.int32), None


def topk_accuracy(rankings, golds, ks):
    """rankings: per sample the ranked ids, best first (empty: no prediction); golds: per sample the gold id (-1 or None: not in the table, which
    counts as wrong, inference.py:35-40).  -> {k: fraction of samples whose gold is among the first k}."""
    n = len(golds)
    if len(rankings) != n:
        raise ValueError('one ranking per gold answer')
    out = {}
    for k in ks:
        hits = sum(1 for r, g in zip(rankings, golds) if g is not None and g >= 0 and g in list(r)[:k])
        out[int(k)] = hits / n if n else 0.0
    return out


class ZeroShotClassifier:
    """The label table encoded once, videos embedded in batches, every <|MASK|> row scored by score_topk.

    model       a PretrainedMerlotReserve
    options     the label strings (through model.get_label_space: needs the tokenizer), and / or
    option_ids  [L, 15] token ids, PAD = 0 (through model.embed_text_spans_only: needs nothing)
    groups      {name: [group of every option]}, ids or strings, e.g. {'verb': [...], 'noun': [...]}
    The label space is kept on the device in the model's dtype, `encode_chunk` options per encoder call.
    `scorer(queries, k, return_logits, groups, num_groups)` replaces score_topk on the stored label space (tests)."""

    def __init__(self, model, options=None, option_ids=None, groups=None, scale=100.0, encode_chunk=1024, scorer=None):
        if options is None and option_ids is None:
            raise ValueError('give the label table as options (strings) or option_ids ([L, 15] token ids)')
        self.model, self.scale = model, float(scale)
        self.options = None if options is None else list(options)
        self.option_ids = None if option_ids is None else np.asarray(option_ids, dtype=np.int64)
        if self.option_ids is not None and (self.option_ids.ndim != 2 or self.option_ids.shape[1] != 15):
            raise ValueError(f'option_ids must be [L, 15], got {self.option_ids.shape}')
        self.num_options = len(self.option_ids) if self.option_ids is not None else len(self.options)
        if self.options is not None and len(self.options) != self.num_options:
            raise ValueError('options and option_ids differ in length')
        if self.num_options < 1:
            raise ValueError('empty label table')
        self._option_index = {} if self.options is None else {o: i for i, o in reversed(list(enumerate(self.options)))}
        self.group_ids, self.group_names, self._group_dev = {}, {}, {}
        for name, values in (groups or {}).items():
            ids, names = _as_ids(values)
            if ids.shape != (self.num_options,) or (ids < 0).any():
                raise ValueError(f'group map {name!r} must give one non-negative group per option')
            self.group_ids[name], self.group_names[name] = ids, names
        self._scorer = scorer
        self.label_space = None
        if model is not None:
            self.label_space = self._encode(max(1, int(encode_chunk)))
            for name, ids in self.group_ids.items():
                self._group_dev[name] = torch.from_numpy(ids).to(self.label_space.device)

    def _encode(self, chunk):
        parts = []
        for i in range(0, self.num_options, chunk):
            if self.option_ids is not None:
                parts.append(self.model.embed_text_spans_only(self.option_ids[i:i + chunk]))
            else:
                parts.append(self.model.get_label_space(self.options[i:i + chunk]))
        return torch.cat(parts, 0).contiguous()

    def _score(self, queries, k, return_logits=False, group=None):
        groups = num_groups = None
        if group is not None:
            groups, num_groups = self._group_dev.get(group, self.group_ids[group]), int(self.group_ids[group].max()) + 1
        if self._scorer is not None:
            return self._scorer(queries, k, return_logits, groups, num_groups)
        return score_topk(queries, self.label_space, k, scale=self.scale, groups=groups, num_groups=num_groups, return_logits=return_logits)

    # ---- embedding ---------------------------------------------------------------------------------------------------
    @staticmethod
    def _batches(videos, batch_size):
        """Consecutive runs of videos with equal array shapes, at most batch_size long: [(first index, [videos])]."""
        out = []
        for i, v in enumerate(videos):
            key = (tuple(v['images'].shape), tuple(v['audio_clips'].shape), len(v['tokens']))
            if out and out[-1][2] == key and len(out[-1][1]) < batch_size:
                out[-1][1].append(v)
            else:
                out.append((i, [v], key))
        return [(i, vs) for i, vs, _ in out]

    def _mask_rows(self, vs):
        """(queries [n, H] on the device, MASKs per video): the rows come from the host-side token arrays, no device read."""
        def stack(key):
            xs = [v[key] for v in vs]
            return torch.stack(xs) if isinstance(xs[0], torch.Tensor) else np.stack([np.asarray(x) for x in xs])
        tokens = np.stack([np.asarray(v['tokens']) for v in vs])
        subseg = np.stack([np.asarray(v['subseg_idxs']) for v in vs])
        out_h = self.model.batch_embed_video(stack('images'), stack('audio_clips'), tokens, subseg)
        is_mask = tokens == MASK
        rows = np.flatnonzero(is_mask.reshape(-1))
        counts = is_mask.sum(1).tolist()
        if rows.size == 0:
            return None, counts
        idx = torch.from_numpy(rows).to(out_h.device)
        return out_h.reshape(-1, out_h.shape[-1]).index_select(0, idx), counts

    # ---- public ------------------------------------------------------------------------------------------------------
    def classify(self, videos, k=5, batch_size=8):
        """videos: one preprocess_video dict or a list of them.  -> per video a list with one entry per <|MASK|> (empty without one):
        {'indices': [...], 'probs': [...], 'options': [...] or None, 'groups': {name: {'ids', 'names' or None, 'labels', 'probs'}}}, best first,
        at most k long (shorter when the table or the number of non-empty groups is smaller)."""
        single = isinstance(videos, dict)
        videos = [videos] if single else list(videos)
        k = int(k)
        results = [[] for _ in videos]
        for first, vs in self._batches(videos, max(1, int(batch_size))):
            queries, counts = self._mask_rows(vs)
            if queries is None:
                continue
            names = list(self.group_ids)
            # one launch covers the options and the first group map; every further map is one more
            scored = [self._score(queries, k, group=names[0] if names else None)] + [self._score(queries, k, group=n) for n in names[1:]]
            host = [{f: getattr(s, f).cpu().numpy() for f in ('values', 'indices', 'lse', 'group_values', 'group_ids', 'group_labels')
                     if getattr(s, f) is not None} for s in scored]
            row = 0
            for j, c in enumerate(counts):
                for _ in range(c):
                    results[first + j].append(self._entry(host, names, row))
                    row += 1
        return results[0] if single else results

    def _entry(self, host, names, row):
        h0 = host[0]
        keep = h0['indices'][row] >= 0
        idx = h0['indices'][row][keep]
        lse = np.float64(h0['lse'][row])
        entry = {'indices': idx.tolist(), 'probs': np.exp(h0['values'][row][keep].astype(np.float64) - lse).tolist(),
                 'options': None if self.options is None else [self.options[i] for i in idx], 'groups': {}}
        for n, h in zip(names, host):
            keep = h['group_ids'][row] >= 0
            gid = h['group_ids'][row][keep]
            entry['groups'][n] = {'ids': gid.tolist(), 'names': None if self.group_names[n] is None else [self.group_names[n][g] for g in gid],
                                  'labels': h['group_labels'][row][keep].tolist(),
                                  'probs': np.exp(h['group_values'][row][keep].astype(np.float64) - np.float64(h['lse'][row])).tolist()}
        return entry

    def ranking(self, video):
        """demo_video.py:46-50: per <|MASK|> of the video the full list of (probability, option), most probable first, ties in table order.
        The option is its string when the table has strings, else its index."""
        queries, _ = self._mask_rows([video])
        if queries is None:
            return []
        s = self._score(queries, 1, return_logits=True)
        logits, lse = s.logits.cpu().numpy().astype(np.float64), s.lse.cpu().numpy().astype(np.float64)
        out = []
        for x, z in zip(logits, lse):
            order = np.argsort(-x, kind='stable')
            p = np.exp(x - z)
            out.append([(float(p[i]), self.options[i] if self.options is not None else int(i)) for i in order])
        return out

    def _gold(self, gold):
        """-> {'options': id or -1, group name: id or -1}, only the keys the sample gives"""
        def option(g):
            if isinstance(g, str):
                return self._option_index.get(g, -1)
            g = int(g)
            return g if 0 <= g < self.num_options else -1

        def group(name, g):
            if isinstance(g, str):
                names = self.group_names[name]
                return names.index(g) if names is not None and g in names else -1
            return int(g)
        if not isinstance(gold, dict):
            return {'options': option(gold)}
        out = {}
        for key, g in gold.items():
            if key in ('option', 'options'):
                out['options'] = option(g)
            elif key in self.group_ids:
                out[key] = group(key, g)
            else:
                raise KeyError(f'gold answer names {key!r}, which is neither "option" nor a group map ({sorted(self.group_ids)})')
        return out

    def evaluate(self, samples, ks=(1, 5, 10), batch_size=8, return_predictions=False):
        """samples yields (video, gold); gold: an option index, an option string, or {'option': ..., group name: gold group}.  The first
        <|MASK|> of every video is scored (the scripts' idx[0, i]); a video without one, and a gold answer that is not in the table, count as
        wrong.  -> {'options': {k: accuracy}, group name: {k: accuracy}, 'n': samples} (a key only where some sample gave that gold)."""
        ks = sorted(int(k) for k in ks)
        if not ks or ks[0] < 1 or ks[-1] > MAX_K:
            raise ValueError(f'ks must lie in [1, {MAX_K}]')
        samples = list(samples)
        preds = self.classify([v for v, _ in samples], k=ks[-1], batch_size=batch_size)
        golds = [self._gold(g) for _, g in samples]
        books = {}
        for p, g in zip(preds, golds):
            first = p[0] if p else None
            for key, gid in g.items():
                ranked = [] if first is None else (first['indices'] if key == 'options' else first['groups'][key]['ids'])
                r, gl = books.setdefault(key, ([], []))
                r.append(ranked)
                gl.append(gid)
        acc = {key: topk_accuracy(r, gl, ks) for key, (r, gl) in books.items()}
        acc['n'] = len(samples)
        return (acc, preds) if return_predictions else acc
