"""``ema_decay``: the float64 reference of the moving average of the weights (``raae_ema_step``).  Not a test module."""
import torch


def ema_step(ema, p, decay):
    """One step of the recurrence in float64: ``decay * ema + (1 - decay) * p``, element by element; returns a new
    tensor.  ``1 - decay`` is formed in float64 (the kernel rounds it to fp32 once, on the host)."""
    ema, p = torch.as_tensor(ema, dtype=torch.float64), torch.as_tensor(p, dtype=torch.float64)
    decay = float(decay)
    return decay * ema + (1.0 - decay) * p


def ema_run(ema0, snapshots, decay):
    """The averages after each of ``snapshots`` (the parameters as every step left them), starting from ``ema0``."""
    out, ema = [], torch.as_tensor(ema0, dtype=torch.float64)
    for p in snapshots:
        ema = ema_step(ema, p, decay)
        out.append(ema)
    return out


def step_bound(ema, p):
    """Per-element bound of ONE fp32 step against ``ema_step``: ``2^-22 * max(|ema|, |p|)`` -- the roundings of
    ``(float)(1 - decay)``, of the product and of the fused multiply-add, half an ulp (2^-24 relative) each, with the one
    of ``(float)decay`` taken as four and expressed relative to the larger operand (both weights are at most 1)."""
    ema, p = torch.as_tensor(ema, dtype=torch.float64), torch.as_tensor(p, dtype=torch.float64)
    return 2.0 ** -22 * torch.maximum(ema.abs(), p.abs())
