"""Torch (CPU) restatement of the reference's TVQA finetuning model -- TEST INFRASTRUCTURE ONLY (may import oracle/).

F = finetune/tvqa/tvqa_finetune.py.  Written from the building blocks of oracle.ref_torch (vision_transformer, audio_transformer,
prepare_multimodal_inputs, transformer_encoder), as oracle.ref_torch.vcr_forward is for VCR; dtype follows the params.  The shared
test configuration, batch and helpers of tests/test_tvqa_plan.py and tests/test_tvqa_gpu.py live here too."""
import numpy as np
import torch

from merlot_reserve_amd.config import tiny_config
from oracle import ref_torch as R


def tvqa_joint_inputs(params, cfg, batch, imgs_enc, audio_enc):
    """F:170-244 + :250: the joint tower's input from the two towers' pooled outputs.  imgs_enc [B, nseg, V, H], audio_enc
    [B, nspans, audio_token_length, H] (any H: only params['token_encoder'] must match it).  Returns x [2 A B, T + nseg V, H], the
    coordinates (numpy), the attention mask and the pool index of every sequence; audio stream first."""
    B, nimg, V, H = imgs_enc.shape
    imgs_enc = torch.cat([torch.zeros(B, 1, V, H, dtype=imgs_enc.dtype), imgs_enc], 1)                      # F:171-174: the "first image"
    nimg += 1                                                                                               # F:177
    B, A, T, _two = batch['textonly_seqs'].shape                                                            # F:178
    imgs_enc = imgs_enc.reshape(B, nimg * V, H).repeat_interleave(A, dim=0)                                 # F:179: repeat-each
    text_toks = batch['textonly_seqs'][..., 0].reshape(B * A, T)                                            # F:182
    text_in = R.prepare_multimodal_inputs(params, cfg, tokens=text_toks, vision_input=imgs_enc,             # F:183-187: no audio pointers
                                          token_segment_idx=batch['textonly_seqs'][..., 1].reshape(B * A, T))
    nspans, a_tok = audio_enc.shape[1], audio_enc.shape[2]                                                  # F:194-195
    audio_enc = audio_enc.repeat_interleave(A, dim=0)                                                       # F:198
    audio_toks = batch['audio_seqs'][..., 0].reshape(B * A, T)                                              # F:200
    ptr = torch.div(torch.cumsum((audio_toks == R.AUDIOSPAN).to(torch.int64), -1) - 1, a_tok, rounding_mode='floor')   # F:201 (jnp // floors)
    ptr = torch.remainder(ptr, nspans)                                                                      # F:202 (jnp % is non-negative)
    audio_in = R.prepare_multimodal_inputs(params, cfg, tokens=audio_toks, vision_input=imgs_enc,           # F:204-210
                                           token_segment_idx=batch['audio_seqs'][..., 1].reshape(B * A, T),
                                           audio_spans=audio_enc, audio_pointers=ptr)
    start = T + V                                                                                           # F:212: cut the "first image" out again
    out = {}
    for k in ('x', 'rotary_coords', 'attention_mask'):                                                      # F:213-224, F:242-244
        cat = np.concatenate if k == 'rotary_coords' else torch.cat
        halves = [cat([t[k][:, :T], t[k][:, start:]], 1) for t in (audio_in, text_in)]
        if k == 'attention_mask':
            halves = [torch.cat([m[:, :, :T], m[:, :, start:]], 2) for m in halves]
        out[k] = cat(halves, 0)
    pool_idx = torch.argmax((torch.cat([audio_toks, text_toks], 0) == R.MASK).to(torch.float32), 1)         # F:250: first MASK, else 0
    return out['x'], out['rotary_coords'], out['attention_mask'], pool_idx


def tvqa_forward(params, config, batch):
    """MerlotReserveTVQA.__call__, F:163-258.  batch: 'images' [B, nseg, hw, 768] float, 'audio_clips' [B, nseg, 3, 60, 65] float,
    'textonly_seqs' / 'audio_seqs' [B, A, T, 2] int64 -> (logits_from_audio, logits_from_text), each [B, A]."""
    cfg = R.Cfg(config)
    H = cfg.hidden_size
    B, nseg, hw, pp3 = batch['images'].shape                                                                # F:166
    imgs_enc = R.vision_transformer(params['vision_encoder'], batch['images'].reshape(B * nseg, hw, pp3), cfg.vit_num_layers, cfg.grid_h,
                                    cfg.grid_w, cfg.vit_pooling_ratio)['seq_attnpool'].reshape(B, nseg, hw // 4, H)     # F:167-168
    _b, _s, nsub, alen, nmel = batch['audio_clips'].shape                                                   # F:191
    audio_enc = R.audio_transformer(params['audio_encoder'], batch['audio_clips'].reshape(-1, alen, nmel), cfg.audio_num_layers,
                                    cfg.audio_pooling_ratio, cfg.audio_patch_size)['seq_attnpool']          # F:192
    audio_enc = audio_enc.reshape(B, nseg * nsub, audio_enc.shape[1], H)                                    # F:197
    x, coords, mask, pool_idx = tvqa_joint_inputs(params, cfg, batch, imgs_enc, audio_enc)
    A, T = batch['textonly_seqs'].shape[1:3]
    joint = R.transformer_encoder(params['joint_transformer'], x, cfg.joint_num_layers, rotary_coords=coords,
                                  attention_mask=mask)['seq'][:, :T]                                        # F:246-247
    pooled_h = joint[torch.arange(2 * A * B), pool_idx]                                                     # F:251
    logits = (pooled_h @ params['proj']['kernel']).squeeze(-1)                                              # F:252
    return logits[:A * B].reshape(B, A), logits[A * B:].reshape(B, A)                                       # F:254-256


def tvqa_train_loss(logits_from_audio, logits_from_text, labels):
    """train_loss_fn, F:277-294."""
    out = {}
    for k, lg in (('audio', logits_from_audio), ('text', logits_from_text)):
        log_p = torch.log_softmax(lg, dim=-1)
        out[f'loss_{k}'] = -(torch.nn.functional.one_hot(labels, lg.shape[-1]).to(log_p.dtype) * log_p).sum(-1).mean()
        out[f'is_right_{k}'] = (torch.argmax(lg, -1) == labels).to(torch.float32).mean()
    return out['loss_audio'] + out['loss_text'], out


def tvqa_pred(logits_from_audio, logits_from_text):
    """pred_step, F:300-310."""
    out = {'logprobs_audio': torch.log_softmax(logits_from_audio, -1), 'preds_audio': torch.argmax(logits_from_audio, -1),
           'logprobs_text': torch.log_softmax(logits_from_text, -1), 'preds_text': torch.argmax(logits_from_text, -1)}
    out['preds_joint'] = torch.argmax(torch.softmax(logits_from_audio, -1) + torch.softmax(logits_from_text, -1), -1)
    return out


# ------------------------------------------------------------------------------------------------ the shared test case
def tvqa_cfg():
    """The smallest shapes at which each indexing rule can fail: B = 2 and A = 3 tell repeat-each from tile, A != 5 catches a hard-coded
    5, nseg = 3 exercises the "+1" of the frame segments, T = 64 < 21 + 54 truncates the last audio span in the middle.
    V = 6, Sj = 82, 12 joint sequences, 6 frames of S = 25, 18 audio clips of S = 31."""
    cfg = tiny_config(hidden_size=128, grid=(4, 6), num_segments=3, lang_seq_len=64)
    cfg['data'].update(num_answers=3)
    cfg['optimizer'] = {'beta_2': 0.98, 'eps': 1e-6, 'learning_rate': 1e-3, 'num_train_steps': 100, 'num_warmup_steps': 2,
                        'use_bfloat16_adam': True, 'weight_decay_rate': 0.1, 'do_bias_correction': True}
    return cfg


def tvqa_batch(cfg, B=2, seed=0, device='cpu'):
    """make_tvqa_batch + the cases the issue asks for by construction."""
    from merlot_reserve_amd.tvqa import TVQADims, make_tvqa_batch
    d = TVQADims(cfg, B)
    batch = make_tvqa_batch(cfg, B, seed=seed, device=device)
    rng = np.random.default_rng(100 + seed)
    span = np.full(d.nas * d.a_tok * d.nseg, R.AUDIOSPAN)
    span_seg = (1 + np.arange(d.nseg)).repeat(d.nas * d.a_tok)
    # (b, a) = (0, 0), audio stream: an option of 20 tokens + MASK, so that T = 64 cuts the last audio span in the middle
    toks = np.concatenate([rng.integers(10, 32768, size=20), [R.MASK], span])[:d.T]
    segs = np.concatenate([np.zeros(21, np.int64), span_seg])[:d.T]
    assert len(toks) == d.T and (d.T - 21) % d.a_tok != 0
    batch['audio_seqs'][0, 0, :, 0], batch['audio_seqs'][0, 0, :, 1] = toks, segs
    # (0, 1), text stream: no MASK (pooled at position 0, a real token)
    t = batch['textonly_seqs'][0, 1, :, 0]
    t[t == R.MASK] = 77
    # (1, 0), both streams: no MASK and a PAD first token -- the pooled position is PAD
    for k in ('textonly_seqs', 'audio_seqs'):
        t = batch[k][1, 0, :, 0]
        t[t == R.MASK] = 78
        t[0] = R.PADDING
    # (1, 2), text stream: token id 5 (AUDIOSPAN) is an ordinary token there
    batch['textonly_seqs'][1, 2, 1, 0] = R.AUDIOSPAN
    batch['textonly_seqs'][1, 2, 4, 0] = R.AUDIOSPAN
    return batch


def ref_batch(batch, dtype=torch.float32):
    return {k: (torch.from_numpy(np.asarray(v).astype(np.int64)) if isinstance(v, np.ndarray) else v.detach().cpu().to(torch.float32).to(dtype))
            for k, v in batch.items()}
