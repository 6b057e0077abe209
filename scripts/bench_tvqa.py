"""TVQA finetuning step timing on one MI355X: python scripts/bench_tvqa.py [steps] [--eager] [--limit SECONDS]
The captured step of the base and of the large model at B = 4 (the reference's per-device batch: 32 examples over 8 devices), at the
released shapes: 7 frames of 12 x 20 patches (ViT S = 241), 21 audio clips (S = 31), 5 answers, T = 256 -> 40 joint sequences of 676.
Both models in one run.  --limit is only looked at before a model starts (one that would start past half of it is left out and said so);
what bounds a run that hangs is the caller's own `timeout`.
Algorithmic FLOPs: 3 x the forward's matrix products (24 H^2 + 4 S H per token and layer, the two embeddings, the two attention pools)."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from merlot_reserve_amd import finetune as F
from merlot_reserve_amd import tvqa as T
from merlot_reserve_amd.config import load_config

args = [a for a in sys.argv[1:] if not a.startswith('--')]
steps = int(args[0]) if args else 10
B = 4
graph = '--eager' not in sys.argv
limit = float(sys.argv[sys.argv.index('--limit') + 1]) if '--limit' in sys.argv else 240.0
t_start = time.perf_counter()
dev = torch.device('cuda:0')
for name in ('base', 'large'):
    if time.perf_counter() - t_start > limit / 2:
        print(f'TVQA {name}: not run, {time.perf_counter() - t_start:.0f} s of the {limit:.0f} s limit were spent')
        continue
    cfg = load_config(name)
    cfg['model']['output_grid'] = [12, 20]
    cfg['data'].update(num_segments=7, lang_seq_len=256, num_answers=5)
    cfg['optimizer'] = {'beta_2': 0.98, 'eps': 1e-6, 'learning_rate': 5e-6, 'num_train_steps': 1000, 'num_warmup_steps': 100,
                        'use_bfloat16_adam': True, 'weight_decay_rate': 0.1, 'do_bias_correction': True}
    model = T.MerlotReserveTVQA.from_config(cfg, device=dev)
    batches = [T.make_tvqa_batch(cfg, B, seed=i, device=dev) for i in range(2)]
    model.init_from_dummy_batch(batches[0])
    state, tx = F.construct_finetuning_train_state(cfg['optimizer'], model)
    d = model.engine.d
    if graph:
        step = T.TVQAGraphStep(state, batches[0])
        plans = [model.engine.build_plan(b) for b in batches]
        run = lambda i: step(batches[i % 2], plans[i % 2])
    else:
        run = lambda i: F.finetune_train_step(state, batches[i % 2])
    for i in range(3):
        run(i)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(steps):
        run(i)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / steps
    info = model.engine.loss_info()
    H = d.H
    enc = lambda n, S, L: n * S * L * (24 * H * H + 4 * S * H)
    fwd = (enc(d.Nv, d.Sv, d.Lv) + enc(d.Na, d.Sa, d.La) + enc(d.n, d.Sj, d.Lj) + d.Nv * d.hw * 2 * d.pp3 * H + d.Na * d.a_len * 2 * 130 * H
           + (d.Nv * d.hw + d.Na * d.a_len) * 4 * H * H + (d.Nv * d.V + d.Na * d.a_tok) * 4 * H * H)
    print(f'TVQA {name} B={B} ({"hipGraph" if graph else "eager"}): {dt * 1e3:.2f} ms/step, {B / dt:.1f} examples/s, loss {info["loss"]:.4f}, '
          f'{3 * fwd / dt / 1e12:.1f} TFLOP/s algorithmic ({3 * fwd / dt / 2.5e15 * 100:.1f} % of bf16 MFMA peak), '
          f'peak memory {torch.cuda.max_memory_allocated() / 2 ** 30:.1f} GiB', flush=True)
    del model, state, batches
    if graph:
        del step, plans
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
