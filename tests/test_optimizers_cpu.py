"""``optimizer_name: RAdam / AdaBound`` without a GPU: the restated torch_optimizer rules of ``optim_reference`` (the
oracle of the GPU tests) against what torch itself offers, and the configuration checks ``Trainer`` makes before it
builds the engine."""
import json
import os

import pytest
import torch

from optim_reference import AdaBound, RAdam
from rankaae_amd.parameter import OPTIM_NAMES, Parameters, check_optimizer

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _cfg(**over):
    with open(os.path.join(GOLDEN, "ref_fc_small.json")) as f:
        cfg = dict(json.load(f)["config"])
    cfg.update(over)
    return cfg


def _trainer(cfg):
    from rankaae_amd.trainer import Trainer
    return Trainer(None, None, None, torch.device("cpu"), None, None, verbose=False,
                   config_parameters=Parameters(cfg))


def test_every_reference_optimizer_name_is_accepted():
    assert set(OPTIM_NAMES) == {"Adam", "AdamW", "AdaBound", "RAdam"}
    for name in OPTIM_NAMES:
        check_optimizer(_cfg(optimizer_name=name))


@pytest.mark.skipif(not hasattr(torch.optim, "RAdam") or
                    "decoupled_weight_decay" not in torch.optim.RAdam.__init__.__code__.co_varnames,
                    reason="this torch's RAdam has no decoupled weight decay")
@pytest.mark.parametrize("wd,betas", [(0.0, (0.9, 0.999)), (0.01, (0.9, 0.999)), (0.01, (0.99, 0.9999))])
def test_restated_radam_matches_torch_radam(wd, betas):
    """torch.optim.RAdam(decoupled_weight_decay=True) is the same rule (its threshold is rho_t > 5 where
    torch_optimizer's is N >= 5; no step lands on 5 exactly): 20 steps, through the SGD start and the rectified part."""
    g = torch.Generator().manual_seed(3)
    p0 = torch.randn(300, generator=g)
    a, b = p0.clone().requires_grad_(True), p0.clone().requires_grad_(True)
    mine = RAdam([a], lr=0.01, betas=betas, weight_decay=wd)
    theirs = torch.optim.RAdam([b], lr=0.01, betas=betas, weight_decay=wd, decoupled_weight_decay=True, foreach=False)
    for it in range(20):
        grad = torch.randn(300, generator=g) * (0.0 if it == 7 else 1.0)
        a.grad, b.grad = grad.clone(), grad.clone()
        mine.step()
        theirs.step()
    assert mine.state[a]["step"] == 20 and isinstance(mine.state[a]["step"], int)
    torch.testing.assert_close(a.detach(), b.detach(), rtol=1e-6, atol=1e-6)
    torch.testing.assert_close(mine.state[a]["exp_avg_sq"], theirs.state[b]["exp_avg_sq"], rtol=1e-6, atol=1e-9)


def test_radam_rectification_starts_at_step_six():
    """N_sma misses 5 at step 5 by only 4e-3 (beta2 = 0.999) and 4e-4 (0.9999, the example config's dis_beta 1.1):
    steps 1-5 are SGD with momentum, step 6 is the first rectified one -- for both betas of the engine's optimizers."""
    def n_sma(t, b2):
        nmax = 2 / (1 - b2) - 1
        return nmax - 2 * t * b2 ** t / (1 - b2 ** t)
    for b2, miss in ((0.999, 4.0e-3), (0.9999, 4.0e-4)):
        assert n_sma(4, b2) < n_sma(5, b2) < 5 <= n_sma(6, b2)
        assert abs(5 - n_sma(5, b2) - miss) < 0.05 * miss
    p = torch.zeros(64, requires_grad=True)
    opt = RAdam([p], lr=0.01)
    for t in range(1, 7):
        p.grad = torch.ones(64)
        opt.step()
        assert (opt.param_groups[0]["buffer"][t % 10][1] >= 5) == (t == 6)


def test_trainer_refuses_a_zero_learning_rate_for_radam_and_adabound():
    for name in ("RAdam", "AdaBound"):
        with pytest.raises(ValueError, match=rf"{name}: invalid learning rate 0\.0"):
            _trainer(_cfg(optimizer_name=name, lr_base=0.0))
        with pytest.raises(ValueError, match=rf"{name}: invalid learning rate -"):
            _trainer(_cfg(optimizer_name=name, lr_ratio_Smooth=-1))
    for cls in (RAdam, AdaBound):        # what the reference's classes do
        with pytest.raises(ValueError, match="Invalid learning rate"):
            cls([torch.zeros(1, requires_grad=True)], lr=0.0)


def test_trainer_still_refuses_an_unknown_optimizer_name():
    with pytest.raises(ValueError, match="must be one of"):
        _trainer(_cfg(optimizer_name="SGD"))
