"""Finetuning shards without TensorFlow: the reference's finetune/common_dataloader.py (C) restated on numpy + PIL over the container code,
the image loader and the parser pool of records.py.

    shard file --iter_tfrecord--> record bytes --parse_example--> {feature name: values}
               --preprocess_vcr / preprocess_tvqa(config, rng)--> one example's features
               --finetune_input_fn_builder / finetune_val_input_fn_builder--> (ids, batch): what finetune.build_vcr_plan / planner.build_tvqa_plan,
                                                                              the two engines and loader.PrefetchLoader(keys=...) consume

    VCR batch   'image' [B, h w, 768], 'answers' [B, 2, A, T] int32, 'labels' [B, 2] int32
    TVQA batch  'images' [B, nseg, h w, 768], 'audio_clips' [B, nseg, 3, 60, 65], 'textonly_seqs' / 'audio_seqs' [B, A, T, 2] int32, 'labels' [B] int32

Float arrays are CPU torch tensors (bf16 when model.use_bfloat16, as C:285-286), integer arrays numpy (the planners read them on the host).  One process
per GPU, so a batch has no num_devices axis: rank r of `world` gets what the reference's device r gets.

As with the pretraining reader (records.py) the record layout and every integer rule follow the cited lines, and the RANDOM DRAWS come from a numpy
Generator instead of TensorFlow's stateful ops: same distributions, different streams.  The two `singleimg_*` preprocessors have no model in the
reference's finetune/ and are not built.

Of the pool / shared-memory machinery of records.py only the pool (_make_pool / _close_pool, chunked map with one chunk in flight) is reused.  The
record slots (_RecordSlots) and the feeder process (ShardFeeder) are laid out for the pretraining record's 'images' / 'audio_clips' pair and are not
used here: a parsed example returns through the pool's pipe, pickled -- about 0.9 MB per VCR example at the 18 x 32 grid, 2.6 MB per TVQA example at
12 x 20 (bf16 bit patterns).  The pretraining reader was held to 136 records / s by that pipe at 6.3 MB per record before it got the slots; whether the
pipe limits these readers is unmeasured: scripts/finetune_driver_cost.py takes the readers' rate beside the rate the step consumes.
"""
import io
import os

import numpy as np

from .records import (AUDIOSPAN, MASK, _close_pool, _make_pool, bf16_bits, iter_tfrecord, load_and_resize_img, make_example, merged_data_config,
                      parse_example, write_tfrecord, zip_longest_skip)

# encoder.encode('answer: ' / 'rationale: ').ids (C:125, C:184; recorded from the reference tokenizer: tests/golden/tokenizer_ids.json).  The drivers
# pass them explicitly; the preprocessors' own default asks the tokenizer, as the reference does.
SEP_TOKEN_IDS = {'qa': [2216, 35, 149], 'qar': [19283, 1406, 35, 149]}
PREPROCESSORS = ('vcr', 'tvqa')
NOT_BUILT = ('singleimg_linearqaoptions', 'singleimg_jointoptions')
MAX_WORKERS = 16
DEFAULT_WORKERS = 4
FLOAT_KEYS = {'vcr': ('image',), 'tvqa': ('images', 'audio_clips')}


def _resolve_sep_tokens(sep_tokens):
    if sep_tokens is not None:
        return {k: [int(t) for t in v] for k, v in sep_tokens.items()}
    try:
        from .modeling import get_encoder
        enc = get_encoder()
    except FileNotFoundError as e:
        raise FileNotFoundError(f"no tokenizer vocabulary to encode the separators 'answer: ' / 'rationale: ' with ({e}): pass "
                                "sep_tokens={'qa': ids, 'qar': ids} (finetune_records.SEP_TOKEN_IDS holds the reference tokenizer's)") from None
    return {'qa': enc.encode('answer: ').ids, 'qar': enc.encode('rationale: ').ids}


def _example(record):
    return record if isinstance(record, dict) else parse_example(record)


def _ints(ex, key):
    return np.asarray(ex.get(key, []), dtype=np.int64).reshape(-1).astype(np.int32)


def _scalar(ex, key, default):
    v = ex.get(key, [])
    return v[0] if len(v) else default


def _id(ex):
    v = _scalar(ex, 'id', b'')
    return v.decode('utf-8') if isinstance(v, (bytes, bytearray)) else str(v)


def _option(query, choice, T):
    """C:131-133 / C:190-191: query + choice cut to T - 1 tokens, then MASK."""
    return np.concatenate([np.concatenate([query, choice])[:T - 1], [MASK]]).astype(np.int32)


def _pad(x, T):
    out = np.zeros((T,) + x.shape[1:], dtype=np.int32)
    out[:min(len(x), T)] = x[:T]
    return out


def preprocess_vcr(record, config, rng, sep_tokens=None, as_bf16_bits=False):
    """C:86-137 for one serialised record (or a parsed Example dict); `config` is the merged data + model section.  Returns 'image' [h w, 768]
    float32 (uint16 bf16 bit patterns with as_bf16_bits), 'answers' [2, A, T] int32 -- the A qa options, then the A qar options, each
    query + separator + choice cut to T - 1 tokens, MASK, zero padding --, 'labels' [2] int32 and 'id'.
    do_random_scale (default True): `image` or `image_fliplr` with probability 1/2 each, and the image loader's random scale.
    sep_tokens = {'qa': ids, 'qar': ids}; None asks the tokenizer (modeling.get_encoder()) for 'answer: ' / 'rationale: '.
    Random draws come from the numpy `rng`: the streams are not TensorFlow's."""
    config = merged_data_config(config)
    sep = _resolve_sep_tokens(sep_tokens)
    ex = _example(record)
    A, T = config['num_answers'], config['lang_seq_len']
    key = 'image'
    if config.get('do_random_scale', True) and not (rng.random() < 0.5):       # C:112-121: sample_bernoulli(0.5) takes `image`
        key = 'image_fliplr'
    out = {'image': load_and_resize_img(_scalar(ex, key, b''), config, rng, as_bf16_bits=as_bf16_bits), 'id': _id(ex)}
    answers = []
    for prefix in ('qa', 'qar'):
        query = np.concatenate([_ints(ex, f'{prefix}_query'), np.asarray(sep[prefix], dtype=np.int32)])
        for i in range(A):
            answers.append(_pad(_option(query, _ints(ex, f'{prefix}_choice_{i}'), T), T))
    out['answers'] = np.stack(answers).reshape(2, A, T)
    out['labels'] = np.array([int(_scalar(ex, 'qa_label', 1)), int(_scalar(ex, 'qar_label', 1))], dtype=np.int32)
    return out


def preprocess_tvqa(record, config, rng, sep_tokens=None, as_bf16_bits=False):
    """C:139-245 for one serialised record (or a parsed Example dict); `config` is the merged data + model section.  Returns 'images'
    [nseg, h w, 768] and 'audio_clips' [nseg, 3, 60, 65] float32 (uint16 bf16 bit patterns with as_bf16_bits), 'textonly_seqs' / 'audio_seqs'
    [A, T, 2] int32 = (token, segment id), 'labels' (int32 scalar) and 'id'.
    Segment 0 of a sequence is the option (query + 'answer: ' + choice cut to T - 1 tokens, MASK); segment k + 1 is frame k's subtitle in the text
    stream, 3 * audio_token_length AUDIOSPAN tokens in the audio stream; truncated and zero-padded to T.  The reference derives the segment ids
    with tf.where over the ragged values (C:195), which drops id-0 tokens from the ids but not from the values; no shard holds a 0 inside a
    subtitle or an option, which is asserted here instead of reproducing the misalignment.
    Frames and clips beyond num_frames are zero (C:215-216, 239), the last mel column is 1 everywhere (C:242-244).  do_random_scale (default
    True): the valid clips, as one sequence of mel rows, get 4 Gaussian rows in front and 4 + (the invalid clips' rows) behind -- mean and
    standard deviation per mel column of the valid rows -- and a window of the original length is cut at a random start in [0, 4] (C:218-238).
    sep_tokens = {'qa': ids}; None asks the tokenizer for 'answer: '.  Random draws come from the numpy `rng`: the streams are not TensorFlow's."""
    from PIL import Image
    config = merged_data_config(config)
    ex = _example(record)
    A, T, nseg = config['num_answers'], config['lang_seq_len'], config['num_segments']
    sep = (_resolve_sep_tokens(sep_tokens) if sep_tokens is None else sep_tokens)['qa']
    images = np.stack([load_and_resize_img(_scalar(ex, f'c{i:02d}/image_encoded', b''), config, rng) for i in range(nseg)])        # C:174-176
    specs = [np.asarray(Image.open(io.BytesIO(_scalar(ex, f'c{i:02d}/spec_encoded', b''))).convert('L')) for i in range(nseg)]
    audio = np.stack(specs).reshape(nseg, 3, 60, 65).astype(np.float32) / np.float32(_scalar(ex, 'magic_number', 1.0))               # C:178-181
    subs = [_ints(ex, f'c{i:02d}/sub') for i in range(nseg)]
    query = np.concatenate([_ints(ex, 'qa_query'), np.asarray(sep, dtype=np.int32)])                                                  # C:184
    span = np.full(3 * config['audio_token_length'], AUDIOSPAN, dtype=np.int32)
    streams = {'textonly_seqs': [], 'audio_seqs': []}
    for i in range(A):
        option = _option(query, _ints(ex, f'qa_choice_{i}'), T)
        for name, per_seg in (('textonly_seqs', subs), ('audio_seqs', [span] * nseg)):
            rows = [option] + list(per_seg)
            values = np.concatenate(rows)
            assert (values != 0).all(), 'a token id 0 inside an option or a subtitle (the reference would misalign its segment ids, C:195)'
            seg_id = np.concatenate([np.full(len(r), k, dtype=np.int32) for k, r in enumerate(rows)])
            streams[name].append(_pad(np.stack([values, seg_id], -1), T))                                                             # C:196-198
    num_frames = int(_scalar(ex, 'num_frames', 1))
    valid = (np.arange(nseg) < num_frames).astype(np.float32)                                                                         # C:215
    images = images * valid[:, None, None]
    if config.get('do_random_scale', True):                                                                                           # C:218-238
        old_shape = audio.shape
        nwin, nmel = old_shape[0] * old_shape[1] * old_shape[2], old_shape[3]
        giant = audio[:num_frames].reshape(-1, nmel)
        avg, std = giant.mean(0), giant.std(0)
        start = rng.normal(avg, std, size=(4, nmel)).astype(np.float32)
        end = rng.normal(avg, std, size=(4 + nwin - giant.shape[0], nmel)).astype(np.float32)
        s = int(rng.integers(0, 5))
        audio = np.concatenate([start, giant, end], 0)[s:s + nwin].reshape(old_shape)
    audio = audio * valid[:, None, None, None]
    audio[..., -1] = 1.0                                                                                                              # C:242-244
    if as_bf16_bits:
        images, audio = bf16_bits(images), bf16_bits(audio)
    return {'images': images, 'audio_clips': audio, 'textonly_seqs': np.stack(streams['textonly_seqs']), 'audio_seqs': np.stack(streams['audio_seqs']),
            'labels': np.int32(_scalar(ex, 'qa_label', 1)), 'id': _id(ex)}


_PREPROCESS = {'vcr': preprocess_vcr, 'tvqa': preprocess_tvqa}


def _preprocessor(preprocessor_type):
    if preprocessor_type in NOT_BUILT:
        raise NotImplementedError(f"preprocessor {preprocessor_type!r}: the singleimg_linearqaoptions / singleimg_jointoptions preprocessors have no "
                                  "model in the reference's finetune/ and are not built; use 'vcr' or 'tvqa'")
    if preprocessor_type not in _PREPROCESS:
        raise ValueError(f'unknown preprocessor {preprocessor_type!r}: one of {PREPROCESSORS}')
    return _PREPROCESS[preprocessor_type]


def _finetune_job(args):
    """One record in a parser worker (module level: picklable).  The worker reaches this function through the merlot_reserve_amd package, whose
    __init__ is empty; this module and records.py import numpy and PIL only at their top, so the worker loads neither torch nor the native
    library (records.py loads that one lazily, for the container's checksums, which only the parent computes)."""
    rec, seed, merged, kind, sep, as_bf16 = args
    return _PREPROCESS[kind](rec, merged, np.random.default_rng(seed), sep_tokens=sep, as_bf16_bits=as_bf16)


def _float_tensor(x, use_bf16):
    import torch
    x = np.ascontiguousarray(x)
    if x.dtype == np.uint16:                                       # bf16 bit patterns from the preprocessor
        t = torch.from_numpy(x.view(np.int16)).view(torch.bfloat16)
        return t if use_bf16 else t.to(torch.float32)
    return torch.from_numpy(x).to(torch.bfloat16 if use_bf16 else torch.float32)


def collate(examples, kind, use_bf16=True, pad_to=None):
    """(ids, batch) of a list of preprocessed examples; pad_to: zero examples with id 'pad' up to that many (C:349-360)."""
    ids = [e['id'] for e in examples]
    batch = {}
    for k in examples[0]:
        if k == 'id':
            continue
        x = np.stack([np.asarray(e[k]) for e in examples])
        if pad_to is not None and len(examples) < pad_to:
            x = np.concatenate([x, np.zeros((pad_to - len(examples),) + x.shape[1:], dtype=x.dtype)], 0)
        batch[k] = _float_tensor(x, use_bf16) if k in FLOAT_KEYS[kind] else x.astype(np.int32)
    if pad_to is not None:
        ids = ids + ['pad'] * (pad_to - len(ids))
    return ids, batch


def _parsed(jobs, pool, processes, chunk_size):
    """The preprocessed examples of the iterable `jobs`, in order; with a pool, chunk k + 1 is being parsed while chunk k is consumed."""
    if pool is None:
        for job in jobs:
            yield _finetune_job(job)
        return
    pending, chunk = None, []

    def submit(c):
        return pool.map_async(_finetune_job, c) if processes else pool.map(_finetune_job, c)

    def collect(h):
        return h.get() if processes else list(h)
    for job in jobs:
        chunk.append(job)
        if len(chunk) == chunk_size:
            nxt = submit(chunk)
            chunk = []
            if pending is not None:
                yield from collect(pending)
            pending = nxt
    if chunk:
        nxt = submit(chunk)
        if pending is not None:
            yield from collect(pending)
        pending = nxt
    if pending is not None:
        yield from collect(pending)


def _workers(workers):
    return max(0, min(int(workers), MAX_WORKERS))


def finetune_input_fn_builder(config, preprocessor_type, rank=0, world=1, seed=None, workers=DEFAULT_WORKERS, processes=True, sep_tokens=None,
                              epochs=None, skip_batches=0):
    """C:291-302 over C:248-289 for one process per GPU: yields (ids, batch) for training.  File i of data.train_fns belongs to rank i mod world;
    every epoch the rank's files are read in a new order, their records interleaved, passed through a shuffle buffer of
    device.shuffle_buffer_size (256) records, preprocessed with do_random_scale as the config has it (default True) and grouped into batches
    of device.batch_size // world examples, the remainder dropped.  Endless unless `epochs` is given.
    skip_batches: start at that batch of the seed's stream (a resumed run): the records of the skipped batches are drawn but not parsed.
    workers: parser processes (threads with processes=False), at most 16; 0 parses in line.  The record -> random-stream assignment does not
    depend on the pool, so every mode yields the same batches for the same seed."""
    _preprocessor(preprocessor_type)
    d, dev = config['data'], config.get('device', {})
    fns = [d['train_fns'].format(i) for i in range(d['num_train_files']) if i % world == rank]
    if not fns:
        raise ValueError(f'rank {rank} of {world} has no shard among {d["num_train_files"]} files')
    batch_size = max(int(dev.get('batch_size', world)) // world, 1)
    buf_size = int(dev.get('shuffle_buffer_size', 256))
    merged = merged_data_config(config)
    use_bf16 = bool(merged.get('use_bfloat16', True))
    sep = _resolve_sep_tokens(sep_tokens)
    rng = np.random.default_rng(seed)
    workers = _workers(workers)
    pool = _make_pool(workers, processes)

    to_skip = [int(skip_batches)]

    def unskipped(job_iter):
        """Drops the jobs of the first to_skip batches of the stream (whole batches: an epoch's remainder is dropped either way)."""
        n = 0
        for job in job_iter:
            if to_skip[0] > 0:
                n += 1
                if n == batch_size:
                    n, to_skip[0] = 0, to_skip[0] - 1
                continue
            yield job

    def jobs(order):
        buf = []
        for rec in (r for group in zip_longest_skip([iter_tfrecord(fn) for fn in order]) for r in group):
            buf.append(rec)
            if len(buf) >= buf_size:
                yield (buf.pop(int(rng.integers(0, len(buf)))), int(rng.integers(0, 2 ** 63)), merged, preprocessor_type, sep, use_bf16)
        while buf:
            yield (buf.pop(int(rng.integers(0, len(buf)))), int(rng.integers(0, 2 ** 63)), merged, preprocessor_type, sep, use_bf16)
    try:
        epoch = 0
        while epochs is None or epoch < epochs:
            order = [fns[i] for i in rng.permutation(len(fns))]
            done = []
            for ex in _parsed(unskipped(jobs(order)), pool, processes, max(batch_size, 2 * workers)):
                done.append(ex)
                if len(done) == batch_size:
                    yield collate(done, preprocessor_type, use_bf16)
                    done = []
            epoch += 1                                             # (drop_remainder=True)
    finally:
        _close_pool(pool, processes)


def finetune_val_input_fn_builder(config, preprocessor_type, rank=0, world=1, workers=0, processes=True, sep_tokens=None):
    """C:304-363: yields (ids, batch) over data.val_fns.format(i), i < data.num_val_files, in file order, do_random_scale False, in batches of
    device.batch_size examples; the last batch is padded with zero arrays and ids 'pad' to the full batch.  With world > 1 rank r gets its
    contiguous slice of every batch (ids and arrays), the reference's reshape to [num_devices, batch // num_devices]."""
    _preprocessor(preprocessor_type)
    d = config['data']
    batch_size = int(config['device']['batch_size'])
    assert batch_size % world == 0, f'device.batch_size {batch_size} is no multiple of the {world} ranks'
    per = batch_size // world
    fns = [d['val_fns'].format(i) for i in range(d['num_val_files'])]
    merged = dict(merged_data_config(config), do_random_scale=False)
    use_bf16 = bool(merged.get('use_bfloat16', True))
    sep = _resolve_sep_tokens(sep_tokens)
    workers = _workers(workers)
    pool = _make_pool(workers, processes)
    jobs = ((rec, 0, merged, preprocessor_type, sep, use_bf16) for fn in fns for rec in iter_tfrecord(fn))

    def rank_slice(ids, batch):
        lo, hi = rank * per, (rank + 1) * per
        return ids[lo:hi], {k: v[lo:hi] for k, v in batch.items()}
    try:
        done = []
        for ex in _parsed(jobs, pool, processes, max(batch_size, 2 * workers)):
            done.append(ex)
            if len(done) == batch_size:
                yield rank_slice(*collate(done, preprocessor_type, use_bf16))
                done = []
        if done:
            yield rank_slice(*collate(done, preprocessor_type, use_bf16, pad_to=batch_size))
    finally:
        _close_pool(pool, processes)


# ------------------------------------------------------------------------------------------------ fixtures
def _jpeg(arr, mode):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(arr, mode=mode).save(buf, format='JPEG', quality=90)
    return buf.getvalue()


def _smooth_frame(rng, frame_hw):
    from PIL import Image
    h, w = frame_hw
    low = rng.uniform(0, 255, size=(h // 8 + 1, w // 8 + 1, 3)).astype(np.uint8)
    return np.asarray(Image.fromarray(low).resize((w, h), Image.Resampling.BICUBIC))


def make_synthetic_vcr_record(config, rng, index=0, frame_hw=(72, 120), split='val'):
    """A serialised VCR record with every key of C:93-102 and plausible content: a smooth random frame and its mirror image as JPEGs, token
    queries / choices, labels.  The id has the form the leaderboard script splits ('<split>-<index>-qar_0': annotation '<split>-<index>', its
    rationales conditioned on answer 0; the real test shards hold one record per conditionee)."""
    c = merged_data_config(config)
    A, T = c['num_answers'], c['lang_seq_len']
    frame = _smooth_frame(rng, frame_hw)
    qa_label, qar_label = int(rng.integers(0, A)), int(rng.integers(0, A))
    feats = {'image': _jpeg(frame, 'RGB'), 'image_fliplr': _jpeg(np.ascontiguousarray(frame[:, ::-1]), 'RGB'),
             'id': f'{split}-{index}-qar_0'.encode(), 'qa_label': qa_label, 'qar_label': qar_label}
    for prefix in ('qa', 'qar'):
        feats[f'{prefix}_query'] = rng.integers(11, 32768, size=int(rng.integers(3, max(4, T // 3))))
        for i in range(A):
            feats[f'{prefix}_choice_{i}'] = rng.integers(11, 32768, size=int(rng.integers(2, max(3, T // 3))))
    return make_example(feats)


def make_synthetic_tvqa_record(config, rng, index=0, frame_hw=(72, 120), num_frames=None):
    """A serialised TVQA record with every key of C:147-160: per segment a JPEG frame, a 1-channel JPEG spectrogram of 3 x 60 x 65 values and a
    subtitle (some empty), the query, the choices, the label, num_frames (at random in [1, nseg] unless given) and the magic number."""
    c = merged_data_config(config)
    A, T, nseg = c['num_answers'], c['lang_seq_len'], c['num_segments']
    feats = {'id': f'{index}~0'.encode(), 'magic_number': np.float32(25.0), 'qa_label': int(rng.integers(0, A)),
             'num_frames': int(rng.integers(1, nseg + 1)) if num_frames is None else int(num_frames),
             'qa_query': rng.integers(11, 32768, size=int(rng.integers(2, max(3, T // 8))))}
    for i in range(A):
        feats[f'qa_choice_{i}'] = rng.integers(11, 32768, size=int(rng.integers(1, max(2, T // 8))))
    for i in range(nseg):
        feats[f'c{i:02d}/image_encoded'] = _jpeg(_smooth_frame(rng, frame_hw), 'RGB')
        feats[f'c{i:02d}/spec_encoded'] = _jpeg(np.clip(rng.normal(110, 40, size=(180, 65)), 0, 255).astype(np.uint8), 'L')
        n = 0 if rng.random() < 0.2 else int(rng.integers(1, max(2, T // (2 * nseg))))
        feats[f'c{i:02d}/sub'] = rng.integers(11, 32768, size=n) if n else []
    return make_example(feats)


SYNTHETIC_RECORD = {'vcr': make_synthetic_vcr_record, 'tvqa': make_synthetic_tvqa_record}


def write_synthetic_shards(config, kind, directory, seed=0, train=(2, 8), val=(2, 3)):
    """Synthetic train / val shards ((files, records per file) each) under `directory`; returns the data keys that name them
    (train_fns, num_train_files, val_fns, num_val_files).  What `finetune_train --synthetic-shards DIR` and the tests read."""
    os.makedirs(directory, exist_ok=True)
    rng = np.random.default_rng(seed)
    keys, index = {}, 0
    for split, (nfiles, per) in (('train', train), ('val', val)):
        pattern = os.path.join(str(directory), f'{split}{{:03d}}of{nfiles:03d}.tfrecord')
        for i in range(nfiles):
            recs = []
            for _ in range(per):
                kw = {'split': split} if kind == 'vcr' else {}
                recs.append(SYNTHETIC_RECORD[kind](config, rng, index=index, **kw))
                index += 1
            write_tfrecord(pattern.format(i), recs)
        keys[f'{split}_fns'], keys[f'num_{split}_files'] = pattern, nfiles
    return keys
