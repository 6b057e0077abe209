"""The oracle side of tests/test_finetune_eval_gpu.py's prediction checks, on the host: the seeds and batches for which the oracle's own argmax is
clear of the 2 x 2e-2 x max|logits| gap on at least three quarters of the examples.  The batches of the existing VCR / TVQA tests pool every
sequence at its MASK token, where the rows are nearly one vector at initialisation, so most seeds leave more than a quarter of the examples under
the gap: of the seeds 0 ... 59, setup(seed) meets the cap for VCR at seed 31 only and for TVQA at 17 seeds, 3 the first (one example of four
excluded each).  The GPU test uses those two.  It also checks the construction of tests/test_tvqa_gpu.py::_pred_batch (no MASK, pooled at
position 0 at a token of its own) and its VCR twin, which leave at most one of four under the gap with those parameters.  Nothing here touches a GPU."""
import torch

from merlot_reserve_amd import finetune as F
from merlot_reserve_amd.params import ParamStore, decay_finetune, tvqa_param_specs, vcr_param_specs
from oracle import ref_torch as R
from tests.test_finetune_eval_gpu import BOUND, TVQA_SEED, VCR_SEED, vcr_pred_batch
from tests.test_tvqa_gpu import _pred_batch as tvqa_pred_batch
from tests.test_vcr_gpu import oracle_batch, vcr_cfg
from tests.tvqa_ref import ref_batch, tvqa_batch, tvqa_cfg, tvqa_forward
from tests.util import tree_to


def _perturbed(cfg, specs, seed):
    """The parameters of the existing tests' setup(dev, seed=seed), as the bf16 working copy the oracle reads."""
    store = ParamStore(cfg, 'cpu', seed=seed, specs=specs(cfg), decay_rule=decay_finetune, with_orig=True)
    g = torch.Generator().manual_seed(1)

    def jit(t):
        return {k: jit(v) for k, v in t.items()} if isinstance(t, dict) else (t + 0.05 * torch.randn(t.shape, generator=g) if t.dim() == 1 else t)
    params = jit(store.master_tree())
    params['proj']['kernel'] = torch.randn(128, 1, generator=g) * 0.3
    store.load_tree(params)
    return tree_to(store.work_tree(), torch.float32)


def _excluded(rows):
    rows = rows.reshape(-1, rows.shape[-1])
    top = torch.topk(rows, 2, -1).values
    return int(((top[:, 0] - top[:, 1]) <= 2 * BOUND * float(rows.abs().max())).sum()), rows.shape[0]


def _vcr_rows(wp, cfg, batch):
    with torch.no_grad():
        return R.vcr_forward(wp, cfg, oracle_batch(batch))


def _tvqa_rows(wp, cfg, batch):
    with torch.no_grad():
        return torch.cat(tvqa_forward(wp, cfg, ref_batch(batch)))


def test_prediction_batches_meet_the_cap_on_the_oracle_alone():
    cfg = vcr_cfg()
    n, of = _excluded(_vcr_rows(_perturbed(cfg, vcr_param_specs, VCR_SEED), cfg, vcr_pred_batch(cfg, 'cpu')))
    assert of == 4 and 4 * n <= of
    cfg = tvqa_cfg()
    n, of = _excluded(_tvqa_rows(_perturbed(cfg, tvqa_param_specs, TVQA_SEED), cfg, tvqa_pred_batch(cfg, 'cpu')))
    assert of == 4 and 4 * n <= of


def _existing_batches(seed):
    """(VCR rows, TVQA rows) of the oracle on the batches and parameters of the existing tests' setup(dev, seed=seed)."""
    cfg = vcr_cfg()
    batch = F.make_vcr_batch(cfg, 2, seed=seed)
    batch['answers'][0, 1, 2, :] = 0                       # (the edits of tests/test_vcr_gpu.py::setup)
    batch['answers'][1, 0, 1, 5:] = 0
    batch['answers'][1, 0, 1, 2] = 3
    vcr = _vcr_rows(_perturbed(cfg, vcr_param_specs, seed), cfg, batch)
    cfg = tvqa_cfg()
    return vcr, _tvqa_rows(_perturbed(cfg, tvqa_param_specs, seed), cfg, tvqa_batch(cfg, 2, seed=seed))


def test_the_chosen_seeds_meet_the_cap_on_the_existing_tests_batches():
    n, of = _excluded(_existing_batches(VCR_SEED)[0])
    assert of == 4 and n == 1
    n, of = _excluded(_existing_batches(TVQA_SEED)[1])
    assert of == 4 and n == 1


def test_most_seeds_do_not():
    """Why the seeds are not 0: seed 0 leaves all four VCR examples and two of the four TVQA examples under the gap."""
    vcr, tvqa = _existing_batches(0)
    assert _excluded(vcr) == (4, 4) and _excluded(tvqa) == (2, 4)
