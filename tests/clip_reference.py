"""``grad_clip_norm``: the float64 oracle of the clipped updates (``raae_grad_norm`` + ``raae_optim_step_clip``).  Not a
conftest: tests import it.

The scale is ``torch.nn.utils.clip_grad_norm_``'s: ``min(1, max_norm / (norm + 1e-6))`` with ``norm`` the L2 norm of
all gradients of ONE optimizer taken together.  The update rules are not restated here: Adam / AdamW are
``torch.optim``'s, RAdam / AdaBound the classes of ``optim_reference`` (imported, not edited), all stepped on float64
tensors with the scaled gradient -- so the moments see the clipped gradient and a decoupled weight decay does not.
"""
import torch

from optim_reference import OPTIMIZERS

RULES = {"Adam": torch.optim.Adam, "AdamW": torch.optim.AdamW, **OPTIMIZERS}


def clip_scale(grads, max_norm):
    """``(norm, scale)`` of the gradients ``grads`` (tensors, taken together) in float64."""
    norm = torch.sqrt(sum((g.double() ** 2).sum() for g in grads))
    scale = torch.clamp(max_norm / (norm + 1e-6), max=1.0)
    return float(norm), float(scale)


def make_optimizer(rule, params, **hyper):
    """The optimizer class of ``rule`` over ``params`` (float64 leaves)."""
    return RULES[rule](params, **hyper)


def clipped_step(opt, params, grads, max_norm=None, scale=None):
    """One step of ``opt`` with ``grads`` (one per parameter, None: no gradient) times the clip scale of ``max_norm``
    -- or times a given ``scale``.  Returns ``(norm, scale)``."""
    have = [g for g in grads if g is not None]
    norm, s = clip_scale(have, max_norm) if scale is None else (float("nan"), float(scale))
    for p, g in zip(params, grads):
        p.grad = None if g is None else g.double() * s
    opt.step()
    return norm, s
