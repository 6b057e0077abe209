"""Zero-shot evaluation over a directory of preprocessed samples: the EPIC-Kitchens (action / verb / noun top-1 / top-5) and MSRVTT-QA
(top-1 / 5 / 10) numbers of zero_shot_ek/zero_shot_eval_ek100.py and zero_shot_qa/inference.py, with the label table encoded once and the
videos embedded in batches.  The dataset-specific CSV / pickle parsing stays with the user: convert to the manifest below.

    python -m merlot_reserve_amd.zeroshot_eval {base,large} --grid H W --labels labels.json --manifest samples.jsonl --out DIR
        [--ckpt-dir DIR | --random-weights] [--bf16] [-k 1 5 10] [--batch-size N] [--synthetic N | --synthetic-media N]

  labels.json    {"options": [str, ...], "option_ids": [[15 token ids], ...], "groups": {name: [group of every option], ...}}; either of the
                 first two keys is enough (strings need the tokenizer vocabulary)
  samples.jsonl  one line per sample: {"id": ..., "npz": path (relative to the manifest), "answer": option index | option string |
                 {"option": ..., group name: gold group}}; the .npz holds the four preprocess_video arrays.  Or decoded media:
                 {"id": ..., "frames": "x.npy", "wav": "x.wav", "segments": [{"text": [ids] | str, "use_text_as_input": bool}, ...],
                  "time_interval": 5.0, "start": 0.0, "answer": ...} -- x.npy uint8 [n, H, W, 3] (one frame per segment), x.wav 16-bit PCM of
                 any rate and channel count: resampled, trimmed of black bars and preprocessed on the device (preprocess.segments_from_pcm)
  DIR/accuracy.json, DIR/predictions.jsonl
  --synthetic N  writes N random samples and a label file to DIR first and evaluates those: needs neither data nor a tokenizer
  --synthetic-media N  the same with N decoded-media samples (letterboxed frames, 48 kHz stereo int16 audio)"""
import argparse
import json
import os
import sys

import numpy as np

from .preprocess import AUDIOSPAN, MASK

VIDEO_KEYS = ('images', 'audio_clips', 'tokens', 'subseg_idxs')


def read_labels(path):
    """-> (options or None, option_ids or None, groups)"""
    d = json.load(open(path))
    if 'options' not in d and 'option_ids' not in d:
        raise ValueError(f'{path}: needs "options" or "option_ids"')
    ids = None if d.get('option_ids') is None else np.asarray(d['option_ids'], dtype=np.int64)
    return d.get('options'), ids, d.get('groups') or {}


def _media_video(rec, base, grid, device):
    """A decoded-media manifest line -> the four arrays: read_wav, segments_from_pcm, the line's per-segment keys, preprocess_video."""
    from .ingest import read_wav
    from .preprocess import preprocess_video, segments_from_pcm
    if grid is None:
        raise ValueError('a manifest line with "frames" / "wav" needs the image grid: read_manifest(path, grid=(h, w))')
    frames = np.load(os.path.join(base, rec['frames']))
    pcm, sr = read_wav(os.path.join(base, rec['wav']))
    segs = segments_from_pcm(frames, pcm, sr, time_interval=rec.get('time_interval', 5.0), segment_start_time=rec.get('start', 0.0), device=device)
    if len(rec['segments']) != len(segs):
        raise ValueError(f'{rec["id"]}: {len(segs)} frames but {len(rec["segments"])} entries under "segments"')
    for seg, extra in zip(segs, rec['segments']):
        seg.update(extra)
    return preprocess_video(segs, tuple(grid), device=device)


def read_manifest(path, grid=None, device=None):
    """-> [(id, {the four arrays}, answer)].  Lines with "npz" need neither `grid` nor `device`; decoded-media lines are preprocessed for `grid`,
    and with `device` their images and audio clips stay there."""
    base = os.path.dirname(os.path.abspath(path))
    out = []
    for line in open(path):
        if not line.strip():
            continue
        rec = json.loads(line)
        if 'npz' in rec:
            with np.load(os.path.join(base, rec['npz'])) as z:
                video = {key: z[key] for key in VIDEO_KEYS}
        else:
            video = _media_video(rec, base, grid, device)
        out.append((rec['id'], video, rec['answer']))
    return out


def write_synthetic(out_dir, n, grid, num_options=40, num_segments=2, seed=0):
    """n random samples (segment 0 carries text that ends in <|MASK|>, the others audio), a table of `num_options` random token-id options with
    'verb' and 'noun' group maps, and the manifest.  -> (labels path, manifest path)"""
    from .preprocess import preprocess_video
    rng = np.random.default_rng(seed)
    os.makedirs(out_dir, exist_ok=True)
    h, w = grid
    option_ids = np.zeros((num_options, 15), dtype=np.int64)
    for row in option_ids:
        m = int(rng.integers(1, 6))
        row[:m] = rng.integers(10, 32768, size=m)
    groups = {'verb': (np.arange(num_options) % 7).tolist(), 'noun': (np.arange(num_options) // 3).tolist()}
    labels = os.path.join(out_dir, 'labels.json')
    with open(labels, 'w') as f:
        json.dump({'option_ids': option_ids.tolist(), 'groups': groups}, f)
    manifest = os.path.join(out_dir, 'samples.jsonl')
    with open(manifest, 'w') as f:
        for i in range(n):
            segs = []
            for s in range(num_segments):
                spec = (rng.random((3, 60, 65)) * 5).astype(np.float32)
                spec[..., 64] = 1.0
                segs.append({'patches': rng.random((h * w, 768)).astype(np.float32), 'spectrogram': spec, 'use_text_as_input': s == 0})
            segs[0]['text'] = rng.integers(10, 32768, size=int(rng.integers(3, 9))).tolist() + [MASK]
            video = preprocess_video(segs, (h, w))
            assert (video['tokens'] == MASK).sum() == 1 and (video['tokens'] == AUDIOSPAN).sum() == 18 * (num_segments - 1)
            np.savez(os.path.join(out_dir, f'sample_{i:04d}.npz'), **video)
            gold = int(rng.integers(0, num_options))
            f.write(json.dumps({'id': f'sample_{i:04d}', 'npz': f'sample_{i:04d}.npz',
                                'answer': {'option': gold, 'verb': groups['verb'][gold], 'noun': groups['noun'][gold]}}) + '\n')
    return labels, manifest


def write_synthetic_media(out_dir, n, num_options=40, seed=0):
    """n decoded-media samples of 2 segments: letterboxed 96 x 160 uint8 frames (.npy), 10 s of 48 kHz stereo int16 (.wav), segment 0 with
    token-id text that ends in <|MASK|>, segment 1 with audio; the label table of write_synthetic.  -> (labels path, manifest path)"""
    import wave
    rng = np.random.default_rng(seed)
    os.makedirs(out_dir, exist_ok=True)
    option_ids = np.zeros((num_options, 15), dtype=np.int64)
    for row in option_ids:
        m = int(rng.integers(1, 6))
        row[:m] = rng.integers(10, 32768, size=m)
    groups = {'verb': (np.arange(num_options) % 7).tolist(), 'noun': (np.arange(num_options) // 3).tolist()}
    labels = os.path.join(out_dir, 'labels.json')
    with open(labels, 'w') as f:
        json.dump({'option_ids': option_ids.tolist(), 'groups': groups}, f)
    manifest = os.path.join(out_dir, 'samples.jsonl')
    sr, t = 48000, np.arange(10 * 48000) / 48000.0
    with open(manifest, 'w') as f:
        for i in range(n):
            frames = np.zeros((2, 96, 160, 3), dtype=np.uint8)
            frames[:, 12:84] = rng.integers(40, 256, (2, 72, 160, 3), dtype=np.uint8)            # 12 rows of bar above and below
            np.save(os.path.join(out_dir, f'media_{i:04d}.npy'), frames)
            tone = np.sin(2 * np.pi * float(rng.uniform(200, 2000)) * t)
            pcm = np.stack([8000 * tone + 2000 * rng.standard_normal(t.size), 6000 * tone + 2000 * rng.standard_normal(t.size)], 1)
            with wave.open(os.path.join(out_dir, f'media_{i:04d}.wav'), 'wb') as wf:
                wf.setnchannels(2)
                wf.setsampwidth(2)
                wf.setframerate(sr)
                wf.writeframes(np.clip(np.round(pcm), -32768, 32767).astype('<i2').tobytes())
            text = rng.integers(10, 32768, size=int(rng.integers(3, 9))).tolist() + [MASK]
            gold = int(rng.integers(0, num_options))
            f.write(json.dumps({'id': f'media_{i:04d}', 'frames': f'media_{i:04d}.npy', 'wav': f'media_{i:04d}.wav',
                                'segments': [{'text': text, 'use_text_as_input': True}, {'use_text_as_input': False}],
                                'time_interval': 5.0, 'start': 0.0,
                                'answer': {'option': gold, 'verb': groups['verb'][gold], 'noun': groups['noun'][gold]}}) + '\n')
    return labels, manifest


def run(model, labels_path, manifest_path, out_dir, ks=(1, 5, 10), batch_size=8, grid=None, device=None):
    """Evaluates the manifest with `model` (a PretrainedMerlotReserve), writes accuracy.json and predictions.jsonl.  -> the accuracy dict"""
    from .zeroshot import ZeroShotClassifier
    options, option_ids, groups = read_labels(labels_path)
    clf = ZeroShotClassifier(model, options=options, option_ids=option_ids, groups=groups)
    samples = read_manifest(manifest_path, grid=grid, device=device)
    acc, preds = clf.evaluate([(v, a) for _, v, a in samples], ks=ks, batch_size=batch_size, return_predictions=True)
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, 'accuracy.json'), 'w') as f:
        json.dump({key: ({str(k): a for k, a in v.items()} if isinstance(v, dict) else v) for key, v in acc.items()}, f, indent=1, sort_keys=True)
    with open(os.path.join(out_dir, 'predictions.jsonl'), 'w') as f:
        for (sid, _, answer), p in zip(samples, preds):
            f.write(json.dumps({'id': sid, 'answer': answer, 'masks': p}) + '\n')
    return acc


def main(argv=None):
    ap = argparse.ArgumentParser(prog='python -m merlot_reserve_amd.zeroshot_eval', description=__doc__.split('\n\n')[0])
    ap.add_argument('model', choices=['base', 'large'])
    ap.add_argument('--grid', type=int, nargs=2, default=[18, 32], metavar=('H', 'W'))
    ap.add_argument('--labels')
    ap.add_argument('--manifest')
    ap.add_argument('--out', required=True)
    ap.add_argument('--ckpt-dir')
    ap.add_argument('--random-weights', action='store_true')
    ap.add_argument('--bf16', action='store_true')
    ap.add_argument('-k', type=int, nargs='+', default=[1, 5, 10])
    ap.add_argument('--batch-size', type=int, default=8)
    ap.add_argument('--synthetic', type=int, default=0, metavar='N')
    ap.add_argument('--synthetic-media', type=int, default=0, metavar='N')
    ap.add_argument('--device', default='cuda:0')
    args = ap.parse_args(argv)
    if args.synthetic:
        args.labels, args.manifest = write_synthetic(args.out, args.synthetic, tuple(args.grid))
    elif args.synthetic_media:
        args.labels, args.manifest = write_synthetic_media(args.out, args.synthetic_media)
    elif not (args.labels and args.manifest):
        ap.error('--labels and --manifest are required without --synthetic / --synthetic-media')
    if args.random_weights == bool(args.ckpt_dir):
        ap.error('give exactly one of --ckpt-dir and --random-weights')
    from .modeling import PretrainedMerlotReserve
    if args.random_weights:
        model = PretrainedMerlotReserve.from_random(args.model, image_grid_size=tuple(args.grid), device=args.device, use_bfloat16=args.bf16)
    else:
        encoder = None
        if read_labels(args.labels)[1] is not None:
            encoder = False                  # a table of token ids needs no vocabulary file
        model = PretrainedMerlotReserve.from_pretrained(args.model, image_grid_size=tuple(args.grid), cache_dir=args.ckpt_dir, device=args.device,
                                                        use_bfloat16=args.bf16, encoder=encoder)
    acc = run(model, args.labels, args.manifest, args.out, ks=args.k, batch_size=args.batch_size, grid=tuple(args.grid), device=args.device)
    print(json.dumps(acc, sort_keys=True))
    return 0


if __name__ == '__main__':
    sys.exit(main())
