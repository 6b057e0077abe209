"""TVQA finetuning step (finetune/tvqa/tvqa_finetune.py + finetune/optimization.py) on the MI355X against the restatement of
tests/tvqa_ref.py: both logit tensors, the two losses / accuracies, dL/dlogits, every parameter gradient (autograd of the restatement,
the audio tower's included), the optimizer leaf by leaf, the scanned and the captured step, pred_step, the state round trip and one step
at the released shapes.  Tolerances are those of tests/test_vcr_gpu.py (bf16 compute vs the fp32 restatement reading the same
bf16-rounded weights and inputs): logits rel-L2 <= 2e-2, gradients |d| <= 8e-2 |g| + 1.5e-2 max|g| and cos >= 0.995."""
import math

import numpy as np
import pytest
import torch

from oracle import ref_torch as R
from tests.tvqa_ref import ref_batch, tvqa_batch, tvqa_cfg, tvqa_forward, tvqa_pred, tvqa_train_loss
from tests.util import relerr, tree_to

pytestmark = pytest.mark.gpu

ZERO_GRAD = ('audio_encoder/transformer/cls_proj/', 'vision_encoder/transformer/cls_proj/')       # the cls outputs feed nothing (F:167, F:192)


def setup(dev, B=2, seed=0, comm=None):
    from merlot_reserve_amd import tvqa as T
    cfg = tvqa_cfg()
    model = T.MerlotReserveTVQA.from_config(cfg, device=dev, seed=seed, comm=comm)
    batch = tvqa_batch(cfg, B, seed=seed, device=dev)
    params = model.init_from_dummy_batch(batch)
    g = torch.Generator().manual_seed(1)                   # non-trivial biases / LN parameters; a larger Dense(1)
    def jit(t):
        return {k: jit(v) for k, v in t.items()} if isinstance(t, dict) else (t + 0.05 * torch.randn(t.shape, generator=g) if t.dim() == 1 else t)
    params = jit(params)
    params['proj']['kernel'] = torch.randn(128, 1, generator=g) * 0.3
    return T, cfg, model, batch, params


def _leaf(tree, name):
    for part in name.split('/'):
        tree = tree[part]
    return tree


@pytest.fixture(scope='module')
def case(dev):
    """ONE forward + loss + backward of the program and ONE evaluation of the restatement, shared by the tests below."""
    T, cfg, model, batch, params = setup(dev)
    la, lt = model.apply({'params': params}, batch)
    eng, store = model.engine, model.params_store
    eng.loss_and_grad_logits()
    torch.cuda.synchronize()
    out = {'T': T, 'cfg': cfg, 'model': model, 'batch': batch, 'params': params, 'logits': (la.float().cpu().clone(), lt.float().cpu().clone()),
           'info': eng.loss_info(), 'dlogits': eng.dlogits[:, 0].float().cpu().clone()}
    # backward from an INJECTED dL/dlogits, for the reason given in tests/test_vcr_gpu.py: at initialisation the loss gradient is a
    # near-cancelling combination, ill-conditioned in bf16 for the reference as well
    g = torch.Generator().manual_seed(9)
    inj = (torch.randn(eng.d.n, generator=g) * 0.2).to(torch.bfloat16)
    eng.dlogits[:, 0] = inj.to(dev)
    eng.backward()
    torch.cuda.synchronize()
    out['grads'] = store.grad_tree()
    rb = ref_batch(batch)
    wp = R.tree_map(lambda t: t.clone().requires_grad_(True), tree_to(store.work_tree(), torch.float32))
    ra, rt = tvqa_forward(wp, cfg, rb)
    AB = eng.d.A * eng.d.B
    (ra.reshape(-1) * inj[:AB].float()).sum().add((rt.reshape(-1) * inj[AB:].float()).sum()).backward()
    out.update(rb=rb, ref_logits=(ra.detach(), rt.detach()),
               ref_grads=R.tree_map(lambda t: t.grad if t.grad is not None else torch.zeros_like(t), wp))
    return out


def test_tvqa_forward_loss_and_dlogits(case):
    d = case['model'].engine.d
    B, A = d.B, d.A
    for k, mine, ref in zip(('audio', 'text'), case['logits'], case['ref_logits']):
        assert mine.shape == ref.shape == (B, A)
        e = relerr(mine, ref)
        print(f'logits_from_{k} rel err', e, mine.flatten()[:3].tolist(), ref.flatten()[:3].tolist())
        assert e < 2e-2
    loss, info = tvqa_train_loss(*case['ref_logits'], case['rb']['labels'])
    li = case['info']
    print('loss', li, float(loss), {k: float(v) for k, v in info.items()})
    assert abs(li['loss'] - float(loss)) < 2e-2 * abs(float(loss))
    for k in ('loss_audio', 'loss_text'):
        assert abs(li[k] - float(info[k])) < 2e-2 * abs(float(info[k])), k
    for k in ('is_right_audio', 'is_right_text'):
        assert abs(li[k] - float(info[k])) < 1.0 / B + 0.01, k                   # within one example: argmax can flip on near-ties in bf16
    onehot = torch.nn.functional.one_hot(case['rb']['labels'], A).float()
    for s, ref in enumerate(case['ref_logits']):
        want = (torch.softmax(ref, -1) - onehot) / B
        got = case['dlogits'][s * A * B:(s + 1) * A * B].view(B, A)
        e = relerr(got, want)
        print('dlogits rel err', s, e)
        assert e < 1e-2                                                          # the loss gradient (bf16 storage)


def test_tvqa_gradients(case):
    grads, gt = case['ref_grads'], case['grads']
    leaves = list(R.tree_leaves(grads))
    assert {n for n, _ in leaves} == {s[0] for s in case['model'].params_store.specs}
    gmax = max(float(g.norm()) for _, g in leaves)
    bad, zero = [], []
    for name, g in leaves:
        mine = _leaf(gt, name)
        gn, err = float(g.norm()), float((mine.double() - g.double()).norm())
        cos = float((mine.double().flatten() @ g.double().flatten()) / (mine.double().norm() * g.double().norm() + 1e-30))
        if err > 8e-2 * gn + 1.5e-2 * gmax or (gn > 5e-2 * gmax and cos < 0.995):
            bad.append((name, err, gn, cos))
        if float(mine.abs().sum()) == 0.0:
            zero.append(name)
    worst = max(((float((_leaf(gt, n).double() - g.double()).norm()) / (float(g.norm()) + 1e-30), n) for n, g in leaves if float(g.norm()) > 5e-2 * gmax))
    print(f'{len(leaves)} gradient leaves, worst relative error among the large ones {worst}')
    assert not bad, bad
    # the parameters the finetuning graph does not reach get exactly zero gradient, and no others
    assert zero and all(n.startswith(ZERO_GRAD) for n in zero) and len(zero) == 4, zero
    assert all(float(g.abs().sum()) == 0.0 for n, g in leaves if n.startswith(ZERO_GRAD))
    assert float(_leaf(gt, 'audio_encoder/embedding/kernel').abs().sum()) > 0.0, 'the audio tower is trained'


TEXT_FIRST = 500


def _pred_batch(cfg, dev):
    """At initialisation the rows pooled at a MASK token are nearly one vector (their logits differ by 1e-3: near-ties whatever proj is), so
    here every sequence is pooled at position 0 (no MASK: argmax semantics) and starts with a token of its own -- other ones in the two
    streams, so that the two sets of predictions differ."""
    batch = tvqa_batch(cfg, 2, seed=0, device=dev)
    for k, first in (('audio_seqs', 100 + 7 * np.arange(6)), ('textonly_seqs', TEXT_FIRST + 11 * np.arange(6))):
        tok = batch[k][..., 0]
        tok[tok == R.MASK] = 79
        tok[:, :, 0] = first.reshape(2, 3)
    return batch


def test_tvqa_pred_step(case):
    T, cfg, model = case['T'], case['cfg'], case['model']
    model._load({'params': case['params']})
    state, _ = _state(T, cfg, model)
    batch = _pred_batch(cfg, model.device)
    out = T.pred_step(state, batch)
    wp = tree_to(model.params_store.work_tree(), torch.float32)
    with torch.no_grad():
        ra, rt = tvqa_forward(wp, cfg, ref_batch(batch))
    want = tvqa_pred(ra, rt)
    assert set(out) == set(want) == {'logprobs_audio', 'preds_audio', 'logprobs_text', 'preds_text', 'preds_joint'}
    # ties are excluded by construction of proj (std 0.3) and of the batch.  Logits within 2e-2 |ref| (L2, the forward test's bound) have no
    # element further off than ea = 2e-2 |ra| (et likewise); an argmax can only flip where the margin is <= twice that.  A softmax moves by
    # at most half its input's largest error (the rows of |diag(p) - p p^T| sum to 2 p (1 - p) <= 1/2), the sum of the two by (ea + et) / 2.
    ea, et = 2e-2 * float(ra.norm()), 2e-2 * float(rt.norm())
    for v, bound in ((ra, 2 * ea), (rt, 2 * et), (torch.softmax(ra, -1) + torch.softmax(rt, -1), ea + et)):
        top = torch.topk(v, 2, -1).values
        assert float((top[:, 0] - top[:, 1]).min()) > bound, 'a near-tie in the restatement: choose another proj'
    assert not torch.equal(want['preds_audio'], want['preds_text'])
    for k in ('preds_audio', 'preds_text', 'preds_joint'):
        assert torch.equal(out[k], want[k]), k
    for k in ('logprobs_audio', 'logprobs_text'):
        assert out[k].shape == want[k].shape and relerr(out[k], want[k]) < 2e-2, k


def _state(T, cfg, model, params=None):
    from merlot_reserve_amd import finetune as F
    return F.construct_finetuning_train_state(cfg['optimizer'], model, params)


def test_known_answer_with_zero_proj(dev):
    """No reference needed: proj = 0 makes every logit exactly 0, each loss ln A, the prediction class 0; d proj = dlogits^T . pooled_h != 0."""
    T, cfg, model, batch, params = setup(dev, seed=5)
    params['proj']['kernel'] = torch.zeros(128, 1)
    state, _ = _state(T, cfg, model, params)
    loss, info = T.train_loss_fn(state, None, batch)
    eng = model.engine
    assert float(eng.logits[:, 0].abs().max()) == 0.0
    A = eng.d.A
    assert abs(loss - 2 * math.log(A)) < 1e-6 * 2 * math.log(A) and set(info) == {'is_right_audio', 'is_right_text', 'loss_audio', 'loss_text'}
    assert abs(info['loss_audio'] - math.log(A)) < 1e-6 * math.log(A) and info['loss_audio'] == info['loss_text']
    assert info['is_right_audio'] == info['is_right_text'] == float(np.mean(batch['labels'] == 0))
    eng.backward()
    torch.cuda.synchronize()
    assert float(model.params_store.g['proj/kernel'].float().abs().sum()) > 0.0


def test_a_used_engine_computes_what_a_fresh_one_does(dev):
    """Forward + loss + backward twice on one engine, another batch in between: the same gradient bits both times.  (The towers share
    scratch buffers whose CLS rows a backward leaves untouched; whatever one tower leaves there must not reach the next.)"""
    T, cfg, model, batch, params = setup(dev, seed=6)
    model._load({'params': params})
    eng, p = model.engine, model.params_store
    other = tvqa_batch(cfg, 2, seed=12, device=dev)
    got = []
    for b in (batch, other, batch):
        p.grad.zero_()
        eng.forward(b)
        eng.loss_and_grad_logits()
        eng.backward()
        torch.cuda.synchronize()
        got.append(p.grad.clone())
    assert torch.equal(got[0], got[2]) and not torch.equal(got[0], got[1])


def test_tvqa_steps_lower_the_loss_and_match_the_optimizer_chain(dev):
    from merlot_reserve_amd import finetune as F
    T, cfg, model, batch, params = setup(dev, seed=3)
    state, tx = _state(T, cfg, model, params)
    store = model.params_store
    state, info0 = F.finetune_train_step(state, batch, loss_fn=T.train_loss_fn, tx_fns=tx)      # step 0: the warm-up schedule's scale is 0
    torch.cuda.synchronize()
    assert model.engine.bucket_log == [b[0] for b in model.engine.gradient_buckets()[0]] and model.engine.bucket_log[:2] == ['joint', 'audio']
    before = {'p': store.master_tree(), 'mu': store._to_tree(store.mu), 'nu': store._to_tree(store.nu), 'orig': store._to_tree(store.orig)}
    state, info = F.finetune_train_step(state, batch, loss_fn=T.train_loss_fn, tx_fns=tx)
    torch.cuda.synchronize()
    # one step == the finetuning chain on the step's own gradients, leaf by leaf (as tests/test_vcr_gpu.py checks the chain), every bucket
    after = {'p': store.master_tree(), 'mu': store._to_tree(store.mu), 'nu': store._to_tree(store.nu), 'g': store.grad_tree()}
    for name, p0 in R.tree_leaves(before['p']):
        np_, nm, nv = R.finetune_adam_apply(p0, _leaf(before['orig'], name), _leaf(after['g'], name).float(), _leaf(before['mu'], name),
                                            _leaf(before['nu'], name), 1, cfg['optimizer'])
        assert torch.allclose(_leaf(after['p'], name), np_, rtol=2e-6, atol=1e-9), name
        assert float((_leaf(after['mu'], name).float() - nm.float()).abs().max()) <= 2 ** -7 * float(nm.float().abs().max()) + 1e-12, name
        dv = (R.unsigned_bf16_decode(_leaf(after['nu'], name)) - R.unsigned_bf16_decode(nv)).abs()
        assert float((dv / (R.unsigned_bf16_decode(nv).abs() + 1e-30)).max()) < 6e-3, name
    assert not torch.equal(_leaf(after['p'], 'audio_encoder/embedding/kernel'), _leaf(before['p'], 'audio_encoder/embedding/kernel'))
    state, info2 = F.finetune_train_step(state, batch, loss_fn=T.train_loss_fn, tx_fns=tx)
    loss, _ = T.train_loss_fn(state, None, batch)
    hist = [info0['loss'], info['loss'], info2['loss'], loss]
    assert state.step == 3 and np.isfinite(hist).all() and set(info) == set(model.engine.metric_names)
    assert hist[-1] < hist[0], hist


def test_scan_minibatch_sums_per_example_gradients(dev):
    from merlot_reserve_amd import finetune as F
    T, cfg, model, batch, params = setup(dev, seed=7)
    state, _ = _state(T, cfg, model, params)
    eng, p = model.engine, model.params_store
    eng.forward(batch)
    eng.loss_and_grad_logits()
    eng.backward()
    torch.cuda.synchronize()
    full, full_info = p.grad.float().clone(), eng.loss_info()
    state, info = F.finetune_train_step(state, batch, scan_minibatch=True)
    torch.cuda.synchronize()
    B = eng.d.B
    assert state.step == 1 and set(info) == set(full_info)
    assert abs(info['loss'] - full_info['loss']) < 2e-3 * abs(full_info['loss'])
    assert info['is_right_audio'] == full_info['is_right_audio'] and info['is_right_text'] == full_info['is_right_text']
    assert relerr(p.grad.float(), B * full) < 3e-2


@pytest.mark.parametrize('with_comm', [False, True], ids=['plain', 'rccl_world1'])
def test_captured_step_matches_eager(dev, with_comm):
    """TVQAGraphStep (hipGraph replay, with the library's RCCL communicator at world 1 in one variant: its collectives are captured too) and
    finetune_train_step give the same parameters and metrics after the same batches, bit for bit."""
    from merlot_reserve_amd import finetune as F
    comm = None
    if with_comm:
        from merlot_reserve_amd.dist import NativeComm
        comm = NativeComm()
    T, cfg, model_a, batch, params = setup(dev, seed=4)
    _T, _c, model_b, _b, _p = setup(dev, seed=4, comm=comm)
    b2 = tvqa_batch(cfg, 2, seed=11, device=dev)
    sa, _ = _state(T, cfg, model_a, params)
    sb, _ = _state(T, cfg, model_b, params)
    F.finetune_train_step(sa, batch)
    step = T.TVQAGraphStep(sb, batch)                      # runs the first step eagerly, then captures
    eager_order = list(model_b.engine.bucket_log)
    for b in (b2, batch):
        F.finetune_train_step(sa, b)
        step(b)
    torch.cuda.synchronize()
    assert sa.step == sb.step == 3
    assert eager_order == model_a.engine.bucket_log and eager_order[:2] == ['joint', 'audio'] and eager_order[-1] == 'vision_end'
    pa, pb = model_a.params_store, model_b.params_store
    assert torch.equal(pa.master, pb.master) and torch.equal(pa.nu, pb.nu) and torch.equal(pa.mu, pb.mu)
    assert model_a.engine.loss_info() == model_b.engine.loss_info()
    if comm is not None:
        comm.close()


def test_state_round_trip(dev):
    """FinetuneTrainState.state_dict / load_state_dict on a TVQA state: everything (the audio tower's leaves too) comes back bit for bit
    into a model with other initial weights, and the restored run continues bit for bit."""
    from merlot_reserve_amd import finetune as F
    T, cfg, model, batch, params = setup(dev, seed=4)
    state, tx = _state(T, cfg, model, params)
    for _ in range(2):
        state, _ = F.finetune_train_step(state, batch)
    torch.cuda.synchronize()
    sd = state.state_dict()
    assert sd['step'] == 2 and 'audio_encoder' in sd['params'] and 'audio_encoder' in sd['opt_state']['0']['mu'] and 'audio_encoder' in sd['opt_state']['1']['orig_params']
    st = model.params_store
    at2 = {k: getattr(st, k).clone() for k in ('master', 'mu', 'nu', 'orig')}
    F.finetune_train_step(state, batch)
    torch.cuda.synchronize()
    want = {k: getattr(st, k).clone() for k in ('master', 'mu', 'nu', 'orig')}
    _T, cfg2, model2, _b, params2 = setup(dev, seed=9)
    state2, _ = _state(T, cfg2, model2, params2)
    st2 = model2.params_store
    assert not torch.equal(st2.orig, at2['orig'])
    state2.load_state_dict(sd)
    assert state2.step == 2
    a0, a1 = st2.tower_ranges['audio_encoder']
    for k in at2:
        assert torch.equal(getattr(st2, k), at2[k]), k
        assert float(getattr(st2, k)[a0:a1].float().abs().sum()) > 0.0, f'{k}: the audio tower is part of the state'
    F.finetune_train_step(state2, batch)
    torch.cuda.synchronize()
    for k in want:
        assert torch.equal(getattr(st2, k), want[k]), f'{k}: the restored run must continue bit for bit'


def test_real_shape_step_from_a_pretraining_tree(dev):
    """The released shapes (base widths, 7 frames of 12 x 20 patches with audio, 5 answers, T = 256: 10 joint sequences of 676) at B = 1 with
    2 layers per tower, started from a PRETRAINING parameter tree through the reference-named entry points: forward + backward + one
    step complete, every gradient is finite, and the proj = 0 known answer holds.  What this catches: a plan capacity or scratch size
    derived from VCR's dimensions."""
    from finetune.optimization import finetune_train_step
    from merlot_reserve_amd.config import load_config
    from merlot_reserve_amd.finetune import construct_finetuning_train_state
    from merlot_reserve_amd.params import ParamStore
    from merlot_reserve_amd.tvqa import MerlotReserveTVQA, make_tvqa_batch, train_loss_fn
    cfg = load_config('base')
    cfg['model'].update(output_grid=[12, 20], vit_num_layers=2, audio_num_layers=2, joint_num_layers=2, span_num_layers=1)
    cfg['data'].update(num_segments=7, lang_seq_len=256, num_answers=5)
    cfg['optimizer'] = tvqa_cfg()['optimizer']
    pre = ParamStore(cfg, 'cpu', seed=1, with_optimizer=False).master_tree()
    assert 'head' in pre and 'span_encoder' in pre and 'proj' not in pre
    model = MerlotReserveTVQA.from_config(cfg, device=dev)
    batch = make_tvqa_batch(cfg, 1, seed=0, device=dev)
    model.init_from_dummy_batch(batch)
    d = model.engine.d
    assert (d.n, d.Sj, d.Nv, d.Sv, d.Na, d.Sa) == (10, 676, 7, 241, 21, 31)
    state, tx = construct_finetuning_train_state(cfg['optimizer'], model, pre)
    store = model.params_store
    assert torch.equal(store.master_tree()['joint_transformer']['final_ln']['scale'], pre['joint_transformer']['final_ln']['scale'])
    assert float(store.wm['proj/kernel'].abs().sum()) > 0.0, 'a tree without proj keeps the initialised one'
    proj = store.wm['proj/kernel'].clone()
    store.wm['proj/kernel'].zero_()
    store.refresh_work()
    loss, info = train_loss_fn(state, None, batch)
    assert float(model.engine.logits[:, 0].abs().max()) == 0.0 and abs(loss - 2 * math.log(5)) < 1e-6 * 2 * math.log(5)
    assert info['is_right_audio'] == info['is_right_text'] == float(batch['labels'][0] == 0)
    model.engine.backward()
    torch.cuda.synchronize()
    assert float(store.g['proj/kernel'].float().abs().sum()) > 0.0 and bool(torch.isfinite(store.grad.float()).all())
    store.wm['proj/kernel'].copy_(proj)             # (with proj = 0 nothing but proj itself gets gradient)
    store.refresh_work()
    state, info = finetune_train_step(state, batch, loss_fn=train_loss_fn, tx_fns=tx)
    torch.cuda.synchronize()
    assert state.step == 1 and bool(torch.isfinite(store.grad.float()).all()) and bool(torch.isfinite(store.master).all())
    assert float(store.g['proj/kernel'].float().abs().sum()) > 0.0 and float(store.g['audio_encoder/embedding/kernel'].float().abs().sum()) > 0.0
