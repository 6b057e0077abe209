"""`mreserve.preprocess` (mreserve/preprocess.py:121-156, 247-271, 463-551): what turns decoded media into the arrays
`MerlotReserve.embed_video` takes.  File decoding (ffmpeg / ffprobe) is out of scope; everything behind it runs on the GPU: PCM of any
rate and channel layout becomes the mono 22050 Hz waveform and black bars are trimmed (merlot_reserve_amd.ingest), uint8 frames of
any size become patches and waveforms become log-mel spectrograms (merlot_reserve_amd.media).  Frames that already are float arrays
at the target resolution, ready patches and ready [3, 60, 65] spectrograms are taken as before.

  make_spectrogram(s)            preprocess.py:121-156   log-mel of a 5 s waveform, three [60, 65] clips
  segments_from_decoded          preprocess.py:247-271   the array half of video_to_segments (mono 22050 Hz waveform, frames as they are)
  segments_from_pcm              preprocess.py:216-271   the same from PCM as decoders give it: downmix, resampling, black-bar trimming
  segments_from_decoded_zero_shot  preprocess.py:312-346 the array half of video_to_segments_zero_shot
  preprocess_image_to_patches    preprocess.py:464-481   resize_and_pad (bilinear, antialiased) + space_to_depth
  patchify                       preprocess.py:478-479   tf.nn.space_to_depth(img, 16) + reshape -> [h*w, 768], patch vector
                                                          order (dy, dx, c) -- the same order as pretrain/dataloader.py:83-84
  preprocess_video               preprocess.py:482-551   token / sub-segment streams, bit-exact
"""
import numpy as np

from .planner import AUDIOSPAN

PADDING, START, END, MASK, MASKAUDIO, LTOVPOOL, RESETCTX = 0, 1, 2, 3, 4, 6, 9


_encoder = None


def __getattr__(name):
    """`from mreserve.preprocess import encoder` (preprocess.py:24): the tokenizer, loaded on first use from the vocabulary
    file the user supplies (modeling.get_encoder)."""
    global _encoder
    if name == 'encoder':
        if _encoder is None:
            from .modeling import get_encoder
            _encoder = get_encoder()
        return _encoder
    raise AttributeError(name)


def video_to_segments(*args, **kwargs):
    """mreserve/preprocess.py:352-460 decodes a video file with ffmpeg / librosa into frames and mel spectrograms: media
    decoding is outside this package -- pass the decoded frames and audio to segments_from_pcm (PCM at the file's own
    rate and channel count) or segments_from_decoded (a mono 22050 Hz waveform)."""
    raise NotImplementedError('video decoding (ffmpeg) is out of scope: decode the frames (uint8 [n, H, W, 3]) and the audio yourself, call '
                              'segments_from_pcm(frames, pcm, sr) with the PCM as decoded, or segments_from_decoded(frames, waveform) with a '
                              'mono 22050 Hz waveform, and then preprocess_video')


def _is_u8(x):
    import torch
    return (x.dtype == torch.uint8) if isinstance(x, torch.Tensor) else (np.asarray(x).dtype == np.uint8)


def _on_device(x):
    import torch
    return isinstance(x, torch.Tensor) and x.is_cuda


def _host(x):
    import torch
    return x.cpu().numpy() if isinstance(x, torch.Tensor) else x


def make_spectrograms(waveforms, playback_speed=1, sr=22050, pad_size=2, device=None):
    """Batched make_spectrogram: waveforms float32 [n, L] -> [n, 3, 60, 65], all rows in one launch.  numpy unless `device` is given (then a
    float32 tensor there)."""
    from . import media
    if playback_speed != 1:
        raise NotImplementedError('only playback_speed=1 (no fast forwarding) is supported')
    if sr != media.SR:
        raise NotImplementedError(f'the spectrogram geometry is fixed to {media.SR} Hz, got sr={sr}')
    shape = tuple(waveforms.shape)
    if len(shape) != 2:
        raise ValueError(f'waveforms must be [n, L], got {shape}')
    seq_size = 60
    T = media.logmel_frames(shape[1])
    if T != seq_size * 3 + pad_size * 4:                                                      # preprocess.py:148-149
        raise ValueError("provided mel spectrogram {}. target size: {}".format((T, 65), (seq_size * 3 + pad_size * 4, 65)))
    if not _on_device(waveforms):
        waveforms = np.asarray(_host(waveforms), dtype=np.float32)
    log_mel = media.logmel(waveforms, playback_speed=float(playback_speed), device=device)
    starts = [pad_size, 2 * pad_size + seq_size, 3 * pad_size + 2 * seq_size]                # preprocess.py:151-155
    import torch
    specs = torch.stack([log_mel[:, a:a + seq_size] for a in starts], 1)
    return specs if device is not None else specs.cpu().numpy()


def make_spectrogram(waveform, playback_speed=1, sr=22050, pad_size=2, device=None):
    """preprocess.py:121-156: the log-mel spectrogram of one segment's waveform with the pretraining parameters, cut into three [60, 65]
    clips with gaps of pad_size rows -> [3, 60, 65]."""
    return make_spectrograms(waveform[None], playback_speed=playback_speed, sr=sr, pad_size=pad_size, device=device)[0]


def preprocess_image_to_patches(img, output_grid_size, device=None):
    """preprocess.py:464-481: a uint8 [H, W, 3] image of any size -> [h1*w1, 768] float32 patches (scaled to fit, zero-padded)."""
    from . import media
    h1, w1 = output_grid_size
    assert h1 <= 24, "we didn't pretrain on anything bigger than 24x24 or 18x32"
    assert w1 <= 32, "we didn't pretrain on anything bigger than 24x24 or 18x32"
    out = media.frames_to_patches(img, (h1, w1), device=device)
    return out if device is not None else out.cpu().numpy()


def segments_from_decoded(frames, waveform, sr=22050, time_interval=5.0, segment_start_time=0.0, device=None):
    """The array half of video_to_segments (preprocess.py:247-271): frames [n, H, W, 3] (one per segment, taken at its middle) and the mono
    waveform of the clip -> the reference's list of dicts ('start_time', 'end_time', 'mid_time', 'frame', 'spectrogram', 'idx').  The waveform
    is cast to float32, divided by max(|w|.max(), 1), zero-padded to the last segment's end and cut at int(sr * start) : int(sr * end); all
    segments' spectrograms come from one launch."""
    n = len(frames)
    times, st = [], segment_start_time
    for _ in range(n):
        et = st + time_interval
        times.append({'start_time': st, 'end_time': et, 'mid_time': (st + et) / 2.0})
        st = et
    if n == 0:
        return times
    waveform = np.asarray(_host(waveform)).astype('float32')
    waveform = waveform / np.float32(max(np.abs(waveform).max() if waveform.size else 0.0, 1.0))
    desired_final_frame = int(sr * max(t['end_time'] for t in times))
    if waveform.size < desired_final_frame:
        waveform = np.concatenate([waveform, np.zeros(desired_final_frame - waveform.size, dtype=np.float32)], 0)
    cuts = [waveform[int(sr * t['start_time']):int(sr * t['end_time'])] for t in times]
    if len({len(c) for c in cuts}) != 1:
        raise ValueError(f'segments of unequal length {sorted({len(c) for c in cuts})}: choose time_interval and segment_start_time so that sr * time is whole')
    specs = make_spectrograms(np.stack(cuts), playback_speed=1, sr=sr, device=device)
    for i, (frame_i, ts_i) in enumerate(zip(frames, times)):
        ts_i['frame'] = frame_i
        ts_i['spectrogram'] = specs[i]
        ts_i['idx'] = i
    return times


def _segment_times(n, time_interval, segment_start_time):
    times, st = [], segment_start_time
    for _ in range(n):
        et = st + time_interval
        times.append({'start_time': st, 'end_time': et, 'mid_time': (st + et) / 2.0})
        st = et
    return times


def _pad_to(wave, length):
    """a 1-D tensor zero-padded at the end to at least `length` samples"""
    import torch
    if wave.numel() >= length:
        return wave
    return torch.cat([wave, torch.zeros(length - wave.numel(), dtype=wave.dtype, device=wave.device)])


def segments_from_pcm(frames, pcm, sr, time_interval=5.0, segment_start_time=0.0, trim_black_bars=True, blackbar_threshold=32,
                      max_perc_to_trim=.2, channels_last=None, device=None):
    """What video_to_segments does with its decoded inputs (preprocess.py:216-271), from media as decoders give it: frames uint8
    [n, H, W, 3] (one per segment, taken at its middle) and `pcm`, int16 or float32 at `sr` Hz, [N], [C, N] or [N, C] (ingest.resample_mono)
    -> the reference's list of dicts, as segments_from_decoded returns it.

      audio    ffmpeg's `-ac 1 -ar 22050` is ingest.resample_mono; the waveform is divided by max(peak, 1) on the device (a float32 division, no
               host round trip), zero-padded to int(22050 * last end), cut at int(22050 * start) : int(22050 * end); one make_spectrograms launch
      frames   ingest.trim_black_bars over the whole stack (extract_frames_from_video, :115-118), or untouched with trim_black_bars=False

    With `device` the frames and spectrograms stay there.  One deviation: the reference's waveform passes through an int16 WAV file between
    ffmpeg and numpy, so its resampled samples are rounded to integers; here they stay float32."""
    import torch
    from . import ingest
    n = len(frames)
    times = _segment_times(n, time_interval, segment_start_time)
    if n == 0:
        return times
    wave, peak = ingest.resample_mono(pcm, sr, channels_last=channels_last, device=device)
    wave = _pad_to(wave / torch.clamp_min(peak, 1.0), int(ingest.SR * max(t['end_time'] for t in times)))
    cuts = [wave[int(ingest.SR * t['start_time']):int(ingest.SR * t['end_time'])] for t in times]
    if len({len(c) for c in cuts}) != 1:
        raise ValueError(f'segments of unequal length {sorted({len(c) for c in cuts})}: choose time_interval and segment_start_time so that sr * time is whole')
    specs = make_spectrograms(torch.stack(cuts), playback_speed=1, sr=ingest.SR, device=device)
    if isinstance(frames, (list, tuple)):
        frames = torch.stack(list(frames)) if isinstance(frames[0], torch.Tensor) else np.stack(frames)
    if device is not None:
        frames = torch.as_tensor(frames).to(device)
    if trim_black_bars:
        frames = ingest.trim_black_bars(frames, blackbar_threshold=blackbar_threshold, max_perc_to_trim=max_perc_to_trim, device=device)
    for i, (frame_i, ts_i) in enumerate(zip(frames, times)):
        ts_i['frame'] = frame_i
        ts_i['spectrogram'] = specs[i]
        ts_i['idx'] = i
    return times


def segments_from_decoded_zero_shot(frames, waveform, times, sr=22050, device=None):
    """The array half of video_to_segments_zero_shot (preprocess.py:312-346; its consumer is demo/zero_shot_ek/extract_ek100_feat.py): `times` is
    a list of {'start_time', 'end_time', 'mid_time'}, frames one per entry, waveform mono at 22050 Hz as for segments_from_decoded -- from raw PCM:

        wave, _ = ingest.resample_mono(pcm, file_rate, device=dev)
        segs = segments_from_decoded_zero_shot(ingest.trim_black_bars(frames), wave, times, device=dev)

    The waveform is divided by max(|w|.max(), 1) and zero-padded to the last end.  A segment shorter than 5 s is centred in zero padding of
    left = int((sr * 5.0 - len) / 2) and right = int(sr * 5.0 - len - left) samples; one of 5 s or more is cut at
    int(sr * (mid - 2.5)) : int(sr * (mid + 2.5)).  A cut whose length does not give 188 spectrogram rows raises the reference's ValueError; cuts
    are grouped by length, one launch per distinct length.  Returns new dicts with 'frame', 'spectrogram' and 'idx' added; frames are not touched."""
    import torch
    times = [dict(t) for t in times]
    if not times:
        return times
    if not isinstance(waveform, torch.Tensor):
        waveform = torch.from_numpy(np.asarray(waveform).astype('float32'))
    w = waveform.to(torch.float32)
    w = w / torch.clamp_min(w.abs().max(), 1.0) if w.numel() else w
    w = _pad_to(w, int(sr * max(t['end_time'] for t in times)))
    window = sr * 5.0                                                     # samples of a 5 s window, a float as in the reference
    cuts = []
    for ts in times:
        if ts['end_time'] - ts['start_time'] < 5.0:                       # shorter than the window: centred in zeros
            cut = w[int(sr * ts['start_time']):int(sr * ts['end_time'])]
            left = int((window - len(cut)) / 2)
            right = int(window - len(cut) - left)
            cut = torch.cat([w.new_zeros(left), cut, w.new_zeros(right)])
        else:                                                             # 5 s or more: the window around the middle
            cut = w[int(sr * (ts['mid_time'] - 2.5)):int(sr * (ts['mid_time'] + 2.5))]
        cuts.append(cut)
    groups = {}
    for i, c in enumerate(cuts):
        groups.setdefault(len(c), []).append(i)
    for idx in groups.values():
        specs = make_spectrograms(torch.stack([cuts[i] for i in idx]), playback_speed=1, sr=sr, device=device)
        for i, spec in zip(idx, specs):
            times[i]['spectrogram'] = spec
    for i, (frame_i, ts_i) in enumerate(zip(frames, times)):
        ts_i['frame'] = frame_i
        ts_i['idx'] = i
    return times


def patchify(img, output_grid_size, P=16):
    """img [h1*P, w1*P, 3] float -> [h1*w1, P*P*3]: space_to_depth in NHWC order (block row, block col, channel)."""
    h1, w1 = output_grid_size
    assert h1 <= 24 and w1 <= 32, "we didn't pretrain on anything bigger than 24x24 or 18x32"      # preprocess.py:474-475
    img = np.asarray(img, dtype=np.float32)
    assert img.shape == (h1 * P, w1 * P, 3), f'expected a {h1 * P}x{w1 * P}x3 frame, got {img.shape}'
    return img.reshape(h1, P, w1, P, 3).transpose(0, 2, 1, 3, 4).reshape(h1 * w1, P * P * 3)


def _images_on_device(video_segments, output_grid_size, dev):
    """[n, h*w, 768] float32 on `dev`: uint8 frames through the resize kernel (one launch per frame size), everything else copied."""
    import torch
    from . import media
    h1, w1 = output_grid_size
    assert h1 <= 24 and w1 <= 32, "we didn't pretrain on anything bigger than 24x24 or 18x32"      # preprocess.py:474-475
    images = torch.empty((len(video_segments), h1 * w1, 768), dtype=torch.float32, device=dev)
    groups = {}
    for i, s in enumerate(video_segments):
        if 'patches' in s:
            images[i] = torch.as_tensor(s['patches']).to(device=dev, dtype=torch.float32)
        elif _is_u8(s['frame']):
            groups.setdefault(tuple(s['frame'].shape), []).append(i)
        else:
            images[i] = torch.from_numpy(patchify(_host(s['frame']), output_grid_size)).to(dev)
    for idx in groups.values():
        fr = [video_segments[i]['frame'] for i in idx]
        batch = torch.stack([f.to(dev) for f in fr]) if isinstance(fr[0], torch.Tensor) else np.stack(fr)
        images[torch.tensor(idx, device=dev)] = media.frames_to_patches(batch, output_grid_size, device=dev)
    return images


def preprocess_video(video_segments, output_grid_size, encoder=None, verbose=False, *, device=None):
    """preprocess.py:482-551.  Each segment: 'frame' (uint8 [H, W, 3] of any size -- resized on the GPU --, or [H, W, 3] float at output
    resolution, or 'patches' [h*w, 768] already patchified), 'spectrogram' [3, 60, 65] or 'waveform' (float32 [110250], 5 s at 22050 Hz --
    log-mel on the GPU), 'text' (str -- needs `encoder` -- or a list of token ids), 'use_text_as_input' (default True).  Returns images
    [n, h*w, 768], audio_clips [3n, 60, 65], tokens [160] int32, subseg_idxs [160] int32; images and audio_clips as numpy arrays, or with
    `device` as float32 tensors there (embed_video takes both)."""
    if len(video_segments) > 8:
        raise ValueError('We only support videos of at most 8 segments right now')             # preprocess.py:497-498
    gpu_images = device is not None or any('patches' not in s and (_is_u8(s['frame']) or _on_device(s['frame'])) for s in video_segments)
    if gpu_images:
        import torch
        dev = torch.device(device) if device is not None else torch.device('cuda', torch.cuda.current_device())
        images = _images_on_device(video_segments, output_grid_size, dev)
        if device is None:
            images = images.cpu().numpy()
    else:
        images = np.stack([np.asarray(s['patches'], dtype=np.float32) if 'patches' in s else patchify(s['frame'], output_grid_size)
                           for s in video_segments])
    subseg_idxs, audio_clips, tokens_out = [], [], []
    for i, segm_i in enumerate(video_segments):
        if segm_i.get('use_text_as_input', True):
            txt = segm_i.get('text', '')
            if isinstance(txt, str):
                if encoder is None:
                    try:
                        encoder = __getattr__('encoder')          # the module-level tokenizer, as in the reference
                    except FileNotFoundError as e:
                        raise ValueError('a tokenizer is needed for string text (pass encoder=..., set MRESERVE_TOKENIZER_JSON, '
                                         'or pass token ids)') from e
                txt_tok = encoder.encode(txt).ids
            else:
                txt_tok = list(txt)
            audio_clips.append(np.zeros([3, 60, 65], dtype=np.float32))       # dummy audio clip
            subseg_idxs.extend([i * 3] * len(txt_tok))
            tokens_out.extend(txt_tok)
        else:
            if 'spectrogram' not in segm_i and 'waveform' in segm_i:
                audio_clips.append(None)                                      # filled below: every waveform of the video in one launch
            elif _on_device(segm_i['spectrogram']):
                audio_clips.append(segm_i['spectrogram'])
            else:
                audio_clips.append(np.asarray(segm_i['spectrogram'], dtype=np.float32))
            tokens_out.extend([AUDIOSPAN] * 18)                               # 6 audio tokens per sub-segment
            subseg_idxs.extend((i * 3 + np.arange(18) // 6).tolist())
    if len(tokens_out) >= 160:
        if verbose:
            print(f'warning -- truncating tokens {len(tokens_out)} to be 160', flush=True)
        tokens_out, subseg_idxs = tokens_out[:160], subseg_idxs[:160]
    while len(tokens_out) < 160:
        tokens_out.append(0)
        subseg_idxs.append(-1)
    waves = [i for i, a in enumerate(audio_clips) if a is None]
    if waves:
        wv = [video_segments[i]['waveform'] for i in waves]
        import torch
        wv = torch.stack(wv) if isinstance(wv[0], torch.Tensor) else np.stack([np.asarray(w, dtype=np.float32) for w in wv])
        for i, spec in zip(waves, make_spectrograms(wv, device=device)):
            audio_clips[i] = spec
    if device is not None or any(_on_device(a) for a in audio_clips):
        import torch
        dev = torch.device(device) if device is not None else torch.device('cuda', torch.cuda.current_device())
        audio = torch.stack([torch.as_tensor(a).to(device=dev, dtype=torch.float32) for a in audio_clips]).reshape(-1, 60, 65)
        audio_clips = audio if device is not None else audio.cpu().numpy()
    else:
        audio_clips = np.stack(audio_clips).reshape(-1, 60, 65)
    return {'images': images, 'audio_clips': audio_clips,
            'tokens': np.array(tokens_out, dtype=np.int32), 'subseg_idxs': np.array(subseg_idxs, dtype=np.int32)}
