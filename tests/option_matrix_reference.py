"""The training step with every option on at once -- ``grad_clip_norm``, ``ema_decay``, ``spec_shift``, ``spec_broaden``,
an ``optimizer_name`` rule, ``detect_anomaly`` and NaN labels -- as a composition of the float64 references the options
already have (``broaden_reference``, ``augment_reference``, ``partial_label_reference``, ``clip_reference`` /
``optim_reference``, ``ema_reference``).  Nothing is restated here: this module fixes the ORDER in which they meet,

    broaden -> shift -> noise -> (the networks) -> masked rank loss -> clipped update -> moving average,

and the combined configuration ``C`` the tests of ``test_option_matrix_gpu.py`` run.  Not a conftest: tests import it.
numpy and torch on the CPU only; ``test_option_matrix_cpu.py`` pins it without a GPU."""
import numpy as np
import torch

import augment_reference as ar
import broaden_reference as br
import clip_reference
import ema_reference
from partial_label_reference import masked_rank_loss

CLIP = 0.02             # tests/test_grad_clip_gpu.py: clips every optimizer on every step of the small configurations
EMA = 0.999
SHIFT, BROADEN = 2.75, 2.5      # tests/test_spec_broaden_gpu.py
UPDATE_RTOL, UPDATE_ATOL = 2e-6, 2e-7       # tests/test_grad_clip_gpu.py::test_teacher_forced_steps_match_the_clipped_reference
STAT_RTOL = 2.0 ** -23                      # the device's {norm, scale} against float64 on the same fp32 gradient, there
RANK_RTOL, RANK_ATOL = 1e-5, 1e-7           # tests/test_partial_labels_gpu.py::test_masked_rank_loss_is_the_float64_definition
MISSING = 0.3                               # share of NaN cells: that file's "blocked" case


def combined(cfg, **over):
    """``cfg`` with every option of the matrix on top (``over``: changes; a value of ``...`` takes the key out)."""
    out = dict(cfg, grad_clip_norm=CLIP, ema_decay=EMA, spec_shift=SHIFT, spec_broaden=BROADEN, detect_anomaly=True)
    out.update(over)
    return {k: v for k, v in out.items() if v is not ...}


def with_missing_labels(aux, seed=11):
    """``aux`` with ``MISSING`` of its cells NaN, the way ``test_partial_labels_gpu._rank_case("blocked")`` draws them --
    without that case's column that is missing everywhere."""
    aux = np.array(aux, dtype=np.float32, copy=True)
    aux[np.random.default_rng(seed).random(aux.shape) < MISSING] = np.nan
    assert not np.isnan(aux).all(axis=0).any(), "a descriptor is missing everywhere"
    return aux


def every_batch_has_a_gap(aux, perm, b, steps):
    """Whether each of the first ``steps`` batches of ``b`` rows of ``perm`` has a NaN cell and no column without labels."""
    aux, perm = np.asarray(aux), np.asarray(perm)
    for k in range(steps):
        d = aux[perm[b * k:b * (k + 1)]]
        if not np.isnan(d).any() or (np.isfinite(d).sum(axis=0) < 2).any():
            return False
    return True


# ------------------------------------------------------------------------------------------------ the batch
def batch(rows, seed, counter, s_broaden, s_shift, noise_term, order="broaden, shift"):
    """The batch a step trains on, float64: ``rows`` broadened, then shifted (``broaden_reference.augment``), plus the
    head's noise term.  ``order="shift, broaden"`` is the WRONG composition (the CPU twin shows that the bound tells them
    apart)."""
    rows = np.asarray(rows)
    if order == "broaden, shift":
        return br.augment(rows, seed, counter, s_broaden, s_shift) + noise_term
    assert order == "shift, broaden"
    g = ar.shift_rows_by(rows, ar.deltas(rows.shape[0], seed, counter, s_shift))
    return br.broaden_rows_by(g, br.sigmas(rows.shape[0], seed, counter, s_broaden), br.radius(s_broaden)) + noise_term


def batch_bound(rows, seed, counter, s_broaden, s_shift, got, noise_term):
    """``broaden_reference.error_bound`` plus the noise term's two roundings: the tolerance of
    ``test_spec_broaden_gpu.test_engine_batch_is_the_reference_applied_to_the_gathered_rows`` (``_noise_tol`` there: one
    rounding of the sum, at most an ulp of the result, and one of the product ``z sigma``)."""
    rows = np.asarray(rows)
    sigma, delta = br.sigmas(rows.shape[0], seed, counter, s_broaden), ar.deltas(rows.shape[0], seed, counter, s_shift)
    noise = np.spacing(np.abs(np.asarray(got, dtype=np.float32))).astype(np.float64) + br.U * np.abs(noise_term)
    return br.error_bound(rows, sigma, br.radius(s_broaden), delta) + noise


# ------------------------------------------------------------------------------------------------ the update
def make_optimizer(rule, params, hyper):
    """The float64 optimizer of ``rule`` from the engine's hyper block ``{lr, beta1, beta2, eps, weight_decay, base_lr,
    final_lr, gamma}`` through ``clip_reference.make_optimizer``: RAdam's lines on float64 copies, AdaBound's bounds
    from the block's ``final_lr`` / ``gamma`` / ``base_lr``."""
    lr, b1, b2, eps, wd, base_lr, final_lr, gamma = [float(x) for x in hyper[:8]]
    kw = dict(lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd)
    if rule == "AdaBound":
        kw.update(final_lr=final_lr, gamma=gamma)
    opt = clip_reference.make_optimizer(rule, params, **kw)
    if rule == "RAdam":
        opt.compute_dtype = torch.float64
    if rule == "AdaBound":
        opt.base_lrs = [base_lr]
    return opt


def teacher_forced_update(table, name, rule, hyper, p0, m0, v0, grad, max_norm):
    """One clipped float64 update of optimizer ``name`` from the state ``p0, m0, v0`` (the code under test's own, before
    its update) with the fp32 gradient ``grad``.  ``table`` keeps one optimizer per name, so that its step count -- the
    bias corrections, RAdam's rectification term, AdaBound's bounds -- advances once per call, as the device's does.
    Returns ``(params, exp_avg, exp_avg_sq, norm, scale)``."""
    if name not in table:
        par = [p0.double().clone()]
        table[name] = (par, make_optimizer(rule, par, hyper))
    par, opt = table[name]
    par[0].copy_(p0.double())
    if opt.state[par[0]]:
        opt.state[par[0]]["exp_avg"].copy_(m0.double())
        opt.state[par[0]]["exp_avg_sq"].copy_(v0.double())
    norm, scale = clip_reference.clipped_step(opt, par, [grad], max_norm)
    st = opt.state[par[0]]
    return par[0].clone(), st["exp_avg"].double().clone(), st["exp_avg_sq"].double().clone(), norm, scale


def update_ratio(got, want):
    """Largest ``|got - want| / (2e-7 + 2e-6 |want|)``: at most 1 inside the update tolerance."""
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    return float(((got - want).abs() / (UPDATE_ATOL + UPDATE_RTOL * want.abs())).max())


# ------------------------------------------------------------------------------------------------ the composed step
class ToyStep:
    """A whole step around the smallest "network" there is -- styles ``z = batch @ W``, the rank loss its only loss -- so
    that the composition can be checked on the CPU: ``batch`` -> ``masked_rank_loss`` -> gradient of ``W`` -> clipped
    update -> moving average.  ``wrong`` names ONE mistake of composition:

    * ``"average before the update"``: the average takes the weights the step began with;
    * ``"norm over the un-masked gradient"``: the clip scale comes from the gradient of the fully labelled loss
      (``d_full``), the update takes the masked gradient;
    * ``"shift before broaden"``."""

    def __init__(self, W, rule, hyper, max_norm=CLIP, decay=EMA, activate=True):
        self.W = [torch.as_tensor(W, dtype=torch.float64).clone()]
        self.opt = make_optimizer(rule, self.W, hyper)
        self.ema = self.W[0].clone()
        self.max_norm, self.decay, self.activate = max_norm, decay, activate

    def gradient(self, x, d):
        loss, dz = masked_rank_loss(d, x @ self.W[0].numpy(), self.activate)
        return loss, torch.from_numpy(x.T @ dz)

    def step(self, rows, d, seed, counter, noise_term, s_broaden=BROADEN, s_shift=SHIFT, wrong=None, d_full=None):
        order = "shift, broaden" if wrong == "shift before broaden" else "broaden, shift"
        x = batch(rows, seed, counter, s_broaden, s_shift, noise_term, order)
        loss, grad = self.gradient(x, d)
        before = self.W[0].clone()
        if wrong == "norm over the un-masked gradient":
            _, scale = clip_reference.clip_scale([self.gradient(x, d_full)[1]], self.max_norm)
            norm, scale = clip_reference.clipped_step(self.opt, self.W, [grad], scale=scale)
        else:
            norm, scale = clip_reference.clipped_step(self.opt, self.W, [grad], self.max_norm)
        self.ema = ema_reference.ema_step(self.ema, before if wrong == "average before the update" else self.W[0], self.decay)
        return dict(batch=x, loss=loss, grad=grad, norm=norm, scale=scale)
