"""``grad_clip_norm`` without a GPU: the key's validation, the float64 reference of the clipped updates pinned against
``torch.nn.utils.clip_grad_norm_`` + ``torch.optim.AdamW``, and the resume fingerprint."""
import numpy as np
import pytest
import torch

import clip_reference
from rankaae_amd import resume
from rankaae_amd.parameter import grad_clip_norm_of


@pytest.mark.parametrize("bad", [0, 0.0, -1.0, float("nan"), float("inf"), "1.0", True])
def test_key_refuses_what_is_not_a_finite_positive_number(bad):
    with pytest.raises(ValueError, match="grad_clip_norm"):
        grad_clip_norm_of({"grad_clip_norm": bad})


def test_null_and_absent_are_the_same_and_numbers_come_back_as_floats():
    assert grad_clip_norm_of({}) is None and grad_clip_norm_of({"grad_clip_norm": None}) is None
    assert grad_clip_norm_of({"grad_clip_norm": 2}) == 2.0 and isinstance(grad_clip_norm_of({"grad_clip_norm": 2}), float)
    assert grad_clip_norm_of({"grad_clip_norm": np.float64(0.5)}) == 0.5


@pytest.mark.parametrize("bad", [0, -0.5, float("nan"), "1.0"])
def test_trainer_refuses_a_bad_key_before_the_gpu(bad):
    """``Trainer.__init__`` raises on the key before it builds the engine: no GPU, no networks, no loaders needed."""
    from rankaae_amd.parameter import Parameters
    from rankaae_amd.trainer import Trainer
    cfg = Parameters({"gradient_reversal": True, "use_cnn_discriminator": False, "optimizer_name": "AdamW",
                      "grad_clip_norm": bad})
    with pytest.raises(ValueError, match="grad_clip_norm"):
        Trainer(None, None, None, torch.device("cpu"), None, None, verbose=False, config_parameters=cfg)


@pytest.mark.parametrize("max_norm", [0.05, 1e3])       # always clipping, never clipping
def test_reference_is_clip_grad_norm_plus_adamw(max_norm):
    g = torch.Generator().manual_seed(3)
    shapes = [(7, 5), (5,), (3, 4, 2)]
    p0 = [torch.randn(s, generator=g, dtype=torch.float64) for s in shapes]
    hyper = dict(lr=0.01, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01)
    mine = [p.clone() for p in p0]
    theirs = [p.clone().requires_grad_(True) for p in p0]
    opt_m, opt_t = clip_reference.make_optimizer("AdamW", mine, **hyper), torch.optim.AdamW(theirs, **hyper)
    for step in range(3):
        grads = [torch.randn(s, generator=g, dtype=torch.float64) * (step + 1) for s in shapes]
        norm, scale = clip_reference.clipped_step(opt_m, mine, grads, max_norm)
        for p, gr in zip(theirs, grads):
            p.grad = gr.clone()
        total = torch.nn.utils.clip_grad_norm_(theirs, max_norm)
        opt_t.step()
        assert abs(norm - float(total)) <= 1e-12 * float(total)
        assert (scale < 1.0) == (max_norm < 1.0)
        for a, b in zip(mine, theirs):
            assert float((a - b.detach()).abs().max()) <= 1e-12
    for a, b in zip(mine, theirs):      # the moments saw the clipped gradient
        assert float((opt_m.state[a]["exp_avg"] - opt_t.state[b]["exp_avg"]).abs().max()) <= 1e-12
        assert float((opt_m.state[a]["exp_avg_sq"] - opt_t.state[b]["exp_avg_sq"]).abs().max()) <= 1e-12


def test_reference_wraps_all_four_rules_and_a_fixed_scale():
    for rule in ("Adam", "AdamW", "RAdam", "AdaBound"):
        p = [torch.ones(4, dtype=torch.float64)]
        q = [torch.ones(4, dtype=torch.float64)]
        grad = [torch.full((4,), 2.0, dtype=torch.float64)]
        a, b = clip_reference.make_optimizer(rule, p, lr=0.01), clip_reference.make_optimizer(rule, q, lr=0.01)
        _, s = clip_reference.clipped_step(a, p, grad, scale=0.25)
        clip_reference.clipped_step(b, q, [grad[0] * 0.25], scale=1.0)
        assert s == 0.25 and torch.equal(p[0], q[0]) and not torch.equal(p[0], torch.ones(4, dtype=torch.float64))


def test_resume_fingerprint_carries_the_key():
    spec = np.ones((4, 8), dtype=np.float32)
    fp = lambda cfg: resume.fingerprint(cfg, 1, 640, 4, 2, spec)       # noqa: E731
    base = {"ae_form": "FC", "nstyle": 2}
    assert fp(base) == fp(dict(base, grad_clip_norm=None))
    assert fp(base) != fp(dict(base, grad_clip_norm=1.0))
    assert fp(dict(base, grad_clip_norm=1.0)) != fp(dict(base, grad_clip_norm=2.0))
    assert fp(dict(base, grad_clip_norm=1)) == fp(dict(base, grad_clip_norm=1.0))
    with pytest.raises(ValueError, match="grad_clip_norm"):
        resume.check_fingerprint(fp(dict(base, grad_clip_norm=1.0)), fp(dict(base, grad_clip_norm=2.0)))
    with pytest.raises(ValueError, match="grad_clip_norm"):
        resume.check_fingerprint(fp(base), fp(dict(base, grad_clip_norm=2.0)))
