"""Immutable attribute namespace over the YAML configuration -- same surface as the
reference's ``sc/utils/parameter.py:42-94`` (``Parameters``, ``from_yaml``, ``get``,
``update``, ``to_dict``; attribute assignment raises ``TypeError``)."""
import ctypes
import math

import yaml

from .model import AE_CLS_DICT  # noqa: F401  (re-exported like the reference does)

# values of the `optimizer_name` key (the reference's OPTIM_DICT, sc/utils/parameter.py:34-39): torch.optim's Adam and
# AdamW, and AdaBound / RAdam of torch_optimizer 0.1.0 -- all four run as fused HIP updates (rankaae_amd/engine.py)
OPTIM_NAMES = ("Adam", "AdamW", "AdaBound", "RAdam")

# the learning-rate ratios of the optimizers the reference's load_optimizers builds, in its order (trainer.py:333-387)
_LR_RATIOS = ("lr_ratio_Reconn", "lr_ratio_Mutual", "lr_ratio_Smooth", "lr_ratio_Corr", "lr_ratio_dis", "lr_ratio_gen")


def check_optimizer(cfg):
    """Refuse a configuration the reference's optimizer classes refuse at construction: an unknown
    ``optimizer_name``, or for AdaBound / RAdam a learning rate ``lr_ratio_* * lr_base <= 0`` (torch_optimizer raises
    ``ValueError('Invalid learning rate')``; AdaBound also divides by its initial lr)."""
    name = cfg.get("optimizer_name")
    if name not in OPTIM_NAMES:
        raise ValueError(f"optimizer_name must be one of {OPTIM_NAMES}, not {name!r}")
    if name in ("AdaBound", "RAdam"):
        for key in _LR_RATIOS:
            if key in cfg:
                lr = cfg[key] * cfg["lr_base"]
                if not lr > 0.0:
                    raise ValueError(f"{name}: invalid learning rate {lr!r} ({key} * lr_base); {name} needs lr > 0")


def grad_clip_norm_of(cfg):
    """Build-only key ``grad_clip_norm`` (default absent / ``null``: off): a finite float > 0.  Each of the five
    optimizers then multiplies its gradient by ``min(1, grad_clip_norm / (norm + 1e-6))`` before its update, ``norm``
    being the L2 norm of that optimizer's own gradient -- ``torch.nn.utils.clip_grad_norm_`` over the optimizer's
    parameters.  Returns the float, or None."""
    value = cfg.get("grad_clip_norm")
    if value is None:
        return None
    if isinstance(value, bool) or not isinstance(value, (int, float)) or not (0.0 < float(value) < float("inf")):
        raise ValueError(f"grad_clip_norm must be absent, null or a finite number > 0, not {value!r}")
    return float(value)


def ema_decay_of(cfg):
    """Build-only key ``ema_decay`` (default absent / ``null``: off): a finite float with ``0 < x < 1``.  The engine
    then keeps an exponential moving average of the parameter arena, ``ema = x * ema + (1 - x) * p`` after the last
    optimizer update of every step, and ``Trainer`` writes it out as ``final_ema.pt``.  Returns the float, or None."""
    value = cfg.get("ema_decay", None)
    if value is None:
        return None
    if isinstance(value, bool) or not isinstance(value, (int, float)) or not (0.0 < float(value) < 1.0):
        raise ValueError(f"ema_decay must be absent, null or a finite number with 0 < ema_decay < 1, not {value!r}")
    return float(value)


def spec_shift_of(cfg, rng_mode=None):
    """Build-only key ``spec_shift`` (default absent / ``null``: off): a finite float ``s > 0``, the largest shift in
    grid points (it may be fractional).  Every training step then resamples every row of its batch at ``l + delta``,
    ``delta`` uniform in ``[-s, s)`` and drawn per row on the device (linear interpolation, replicated edges), before
    the spectral noise is added; validation and every export see the rows as they are.  The draw lives in the fused
    step head's device random state, so the key needs ``rng_mode: philox`` (``rng_mode``: what the engine was built
    with, default: the config's) and ``fused_step_begin`` on.  Returns the float, or None."""
    value = cfg.get("spec_shift", None)
    if value is None:
        return None
    if isinstance(value, bool) or not isinstance(value, (int, float)) or not (0.0 < float(value) < float("inf")):
        raise ValueError(f"spec_shift must be absent, null or a finite number > 0, not {value!r}")
    if (rng_mode if rng_mode is not None else cfg.get("rng_mode", "philox")) != "philox" or \
            not cfg.get("fused_step_begin", True):
        # (the parity mode exists for comparisons with the reference, which has no such draw to be in parity with)
        raise ValueError("spec_shift: device RNG with the fused step head only")
    return float(value)


SPEC_BROADEN_RMAX = 64      # the largest radius raae_spec_augment2 has LDS for


def _spec_broaden_product(s):
    """``3 s`` as the kernel computes it: ``s`` rounded to fp32, then the fp32 product (Inf for a large finite ``s``)."""
    f = ctypes.c_float(float(s)).value
    return ctypes.c_float(3.0 * f).value                     # (3 f is exact in double: rounded once, as on the device)


def spec_broaden_radius(s):
    """``ceil(3 s)`` as the kernel computes it, for an ``s`` whose product is finite; the range check itself compares
    the product (``ceil(p) <= 64`` is ``p <= 64``), as the entry point does, before any conversion to an integer."""
    return math.ceil(_spec_broaden_product(s))


def spec_broaden_of(cfg, rng_mode=None):
    """Build-only key ``spec_broaden`` (default absent / ``null``: off): a finite float ``s > 0`` with
    ``ceil(3 s) <= 64``, the largest Gaussian sigma in grid points (it may be fractional).  Every training step then
    convolves every row of its batch with a normalised Gaussian of its own width, uniform in ``[0, s)`` and drawn per
    row on the device (replicated edges), before the energy shift (``spec_shift``) and the spectral noise; validation
    and every export see the rows as they are.  Needs ``rng_mode: philox`` and ``fused_step_begin``, like
    ``spec_shift``.  Returns the float, or None."""
    value = cfg.get("spec_broaden", None)
    if value is None:
        return None
    if isinstance(value, bool) or not isinstance(value, (int, float)) or not (0.0 < float(value) < float("inf")) or \
            not _spec_broaden_product(value) <= SPEC_BROADEN_RMAX:
        raise ValueError("spec_broaden must be absent, null or a finite number s with 0 < s and ceil(3 s) <= "
                         f"{SPEC_BROADEN_RMAX} (the largest Gaussian sigma in grid points), not {value!r}")
    if (rng_mode if rng_mode is not None else cfg.get("rng_mode", "philox")) != "philox" or \
            not cfg.get("fused_step_begin", True):
        raise ValueError("spec_broaden: device RNG with the fused step head only")
    return float(value)


def _fp32_of(value):
    """``value`` as the kernel sees it, rounded to fp32 (Inf for a finite number beyond fp32), or None for anything that
    is not a real number (a bool, a string, an integer beyond every float)."""
    if isinstance(value, bool) or not isinstance(value, (int, float)):
        return None
    try:
        return ctypes.c_float(float(value)).value
    except OverflowError:
        return None


def _step_head_rng(cfg, rng_mode):
    return (rng_mode if rng_mode is not None else cfg.get("rng_mode", "philox")) == "philox" and \
        bool(cfg.get("fused_step_begin", True))


def spec_gain_of(cfg, rng_mode=None):
    """Build-only key ``spec_gain`` (default absent / ``null``: off): a finite float ``a`` with ``0 < a < 1``, the
    largest relative error of the normalisation.  Every training step then multiplies row b of its batch by
    ``g_b = 1 + (2 u_b - 1) a``, ``u_b`` uniform in ``[0, 1)`` and drawn per row on the device, behind the broadening
    and the energy shift and before the spectral noise; validation and every export see the rows as they are.  The
    bounds hold for the value as the kernel sees it, in fp32 (``1 - 1e-12`` rounds to 1 and is refused).  Needs
    ``rng_mode: philox`` and ``fused_step_begin``, like ``spec_shift``.  Returns the float, or None."""
    value = cfg.get("spec_gain", None)
    if value is None:
        return None
    f = _fp32_of(value)
    if f is None or not (0.0 < float(value) and f < 1.0):
        raise ValueError(f"spec_gain must be absent, null or a finite number a with 0 < a < 1, not {value!r}")
    if not _step_head_rng(cfg, rng_mode):
        raise ValueError("spec_gain: device RNG with the fused step head only")
    return float(value)


def spec_tilt_of(cfg, rng_mode=None):
    """Build-only key ``spec_tilt`` (default absent / ``null``: off): a finite float ``t > 0``, the largest height of a
    residual linear background at the ends of a row.  Every training step then adds ``c_b r_l`` to row b of its batch,
    ``c_b = (2 u'_b - 1) t`` drawn per row on the device and ``r_l`` running from -1 at the first sample to +1 at the
    last, behind the gain (``spec_gain``) and before the spectral noise; validation and every export see the rows as
    they are.  Finite means finite in fp32, as the kernel sees it.  Needs ``rng_mode: philox`` and
    ``fused_step_begin``, like ``spec_shift``.  Returns the float, or None."""
    value = cfg.get("spec_tilt", None)
    if value is None:
        return None
    f = _fp32_of(value)
    if f is None or not (0.0 < float(value) and f < float("inf")):
        raise ValueError(f"spec_tilt must be absent, null or a finite number > 0, not {value!r}")
    if not _step_head_rng(cfg, rng_mode):
        raise ValueError("spec_tilt: device RNG with the fused step head only")
    return float(value)


def style_decorr_of(cfg):
    """Build-only key ``style_decorr`` (default absent / ``null``: off): a finite float ``w > 0``, the weight of the
    decorrelation penalty.  Phase B of every training step then minimises ``aux_loss + w * D``, ``D`` the mean squared
    off-diagonal Pearson correlation of the styles over the batch: ``w * dD/dstyles`` is added to the rank loss's
    gradient on the device (``raae_style_decorr_fwd_bwd``) before the encoder's backward pass.  ``D`` enters no logged
    loss; ``w`` scales the gradient, not the learning rate.  Returns the float, or None."""
    value = cfg.get("style_decorr", None)
    if value is None:
        return None
    if isinstance(value, bool) or not isinstance(value, (int, float)) or not (0.0 < float(value) < float("inf")):
        raise ValueError(f"style_decorr must be absent, null or a finite number > 0, not {value!r}")
    return float(value)


RANK_LOSS_FORMS = ("linear", "logistic")


def rank_loss_form_of(cfg, world_size=1):
    """Build-only keys ``rank_loss_form`` (``linear``, the default: the reference's ``kendall_constraint``; or
    ``logistic``) and ``rank_temperature`` (a finite float ``T > 0``, default 1.0, with ``logistic`` only).  With
    ``logistic`` phase B of every training step minimises the pairwise logistic (RankNet) loss
    ``T * softplus(-s * (z_i - z_j) / T)`` over the pairs with distinct labelled descriptors (``s`` the sign of the
    descriptor difference), normalised like the linear loss (``raae_rank_logistic_fwd_bwd``): the gradient of a pair is
    the sigmoid of how wrongly it is ordered, the loss is bounded below by 0, and ``kendall_activation`` is not applied
    to it.  The styles leave the style BatchNorm with unit variance, so ``T`` is in style standard deviations; the
    default 1.0 is a convention, not a tuned value.  The validation pass keeps the linear loss.  ``world_size > 1``
    with ``rank_loss_pairs: global`` is refused.  Returns ``(form, T)``, ``T`` None with ``linear``."""
    form = cfg.get("rank_loss_form", None)
    if form is None:
        form = "linear"
    if not isinstance(form, str) or form not in RANK_LOSS_FORMS:
        raise ValueError(f"rank_loss_form must be 'linear' or 'logistic', not {form!r}")
    value = cfg.get("rank_temperature", None)
    if form != "logistic":
        if value is not None:
            raise ValueError("rank_temperature: with rank_loss_form: logistic only")
        return form, None
    if value is None:
        value = 1.0
    # (the kernel works with the value as fp32: that, too, is finite and > 0)
    if isinstance(value, bool) or not isinstance(value, (int, float)) or not (0.0 < float(value) < float("inf")) or \
            not 0.0 < ctypes.c_float(float(value)).value < float("inf"):
        raise ValueError(f"rank_temperature must be a finite number > 0, not {value!r}")
    if world_size > 1 and str(cfg.get("rank_loss_pairs", "local")) == "global":
        raise ValueError("rank_loss_form: logistic: rank_loss_pairs: local only")
    return form, float(value)


REPORT_WEIGHTS = {"final": "final.pt", "ema": "final_ema.pt"}


def report_weights_of(cfg):
    """``generate_report``'s key ``report_weights``: ``final`` (default; every ``job_*/final.pt``) or ``ema`` (every
    ``job_*/final_ema.pt``, the moving average a run with ``ema_decay`` writes).  Returns the value."""
    value = cfg.get("report_weights", "final")
    if not isinstance(value, str) or value not in REPORT_WEIGHTS:
        raise ValueError(f"report_weights must be 'final' or 'ema', not {value!r}")
    return value


def _int_key(cfg, key, least, default):
    value = cfg.get(key, None)
    if value is None:
        return default
    if isinstance(value, bool) or not isinstance(value, int) or value < least:
        raise ValueError(f"{key} must be an integer >= {least}, not {value!r}")
    return value


def apply_keys_of(cfg):
    """The build-only keys of ``rankaae_amd.cmd.apply``: ``apply_top_n`` (an integer >= 1, default ``top_n``: how many of
    the best-ranked trials are applied), ``apply_max_outside`` (an integer >= 0, default 0: how many points of the
    model's energy grid may lie outside the input's range and take its edge value) and ``apply_chunk_rows`` (an integer
    >= 1, default 16384: rows per pass of the models).  Returns ``(apply_top_n, apply_max_outside, apply_chunk_rows)``."""
    top_n = _int_key(cfg, "apply_top_n", 1, None)
    if top_n is None:
        top_n = _int_key(cfg, "top_n", 1, None)
        if top_n is None:
            raise ValueError("apply_top_n: absent, and there is no top_n to default to")
    return top_n, _int_key(cfg, "apply_max_outside", 0, 0), _int_key(cfg, "apply_chunk_rows", 1, 16384)


def detect_anomaly_on(cfg):
    """Build-only key ``detect_anomaly`` (default ``true``: the reference turns on
    ``torch.autograd.set_detect_anomaly(True)`` at import, sc/clustering/trainer.py:11).  On, the optimizer updates
    check every parameter gradient for NaN on the device and ``Trainer.train`` raises ``AnomalyError`` at the end of
    the epoch in which one appeared; ``false`` launches the unchecked updates."""
    value = cfg.get("detect_anomaly", True)
    if not isinstance(value, bool):
        raise ValueError(f"detect_anomaly must be true or false, not {value!r}")
    return value


def rank_metrics_on(cfg):
    """Build-only key ``rank_metrics`` (default ``false``): ``true`` makes every validation also form, on the device,
    Kendall's tau-b of each descriptor against its style over the validation rows labelled for it
    (``raae_kendall_tau``), and ``Trainer`` append them to ``rank_metrics.csv`` every epoch.  A bool and nothing else:
    ``"true"``, ``1`` and the like are a ``ValueError``."""
    value = cfg.get("rank_metrics", False)
    if not isinstance(value, bool):
        raise ValueError(f"rank_metrics must be true or false, not {value!r}")
    return value


def checkpoint_every_of(cfg):
    """Build-only key ``checkpoint_every`` (default 0: off): an integer N >= 0; with N > 0 ``Trainer`` writes the
    trial's resume file (``rankaae_amd/resume.py``) after every N-th epoch, and when a stop request ends the run."""
    value = cfg.get("checkpoint_every", 0)
    if isinstance(value, bool) or not isinstance(value, int) or value < 0:
        raise ValueError(f"checkpoint_every must be an integer >= 0, not {value!r}")
    return value


def resume_on(cfg):
    """Build-only key ``resume`` (default ``false``): ``true`` continues a trial from the resume file in its work
    directory, if there is a usable one."""
    value = cfg.get("resume", False)
    if not isinstance(value, bool):
        raise ValueError(f"resume must be true or false, not {value!r}")
    return value


class Parameters:
    def __init__(self, parameter_dict):
        object.__setattr__(self, "_parameter_dict", parameter_dict)
        self.update(parameter_dict)

    def __setattr__(self, name, value):
        raise TypeError("Parameters object cannot be modified after instantiation")

    def get(self, key, value):
        return self._parameter_dict.get(key, value)

    def update(self, parameter_dict):
        self._parameter_dict.update(parameter_dict)
        self.__dict__.update(self._parameter_dict)

    def to_dict(self):
        return self._parameter_dict

    @classmethod
    def from_yaml(cls, config_file_path):
        with open(config_file_path) as f:
            return cls(yaml.safe_load(f))
