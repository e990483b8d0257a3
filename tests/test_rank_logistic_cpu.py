"""``rank_loss_form: logistic`` without a GPU: the float64 reference of the pairwise logistic rank loss
(``rank_logistic_reference``) against finite differences, against autograd on the literal formula and on the cases
whose answer is known; the keys' validation, the resume fingerprint and the ``TrialBatch`` agreement check."""
import math
import types

import numpy as np
import pytest
import torch

import rank_logistic_reference as rl
from rankaae_amd import resume
from rankaae_amd.parameter import Parameters, rank_loss_form_of


# ------------------------------------------------------------------------------------------------ the reference
def _inputs(B=23, n_aux=3, seed=0):
    d, z = rl.make_inputs(B, n_aux, n_aux + 1, n_aux + 2, seed)
    z = np.clip(z.astype(np.float64), -3.0, 3.0)         # (finite differences want a smooth neighbourhood)
    return d.astype(np.float64), z


@pytest.mark.parametrize("T", [0.3, 1.0, 20.0])
def test_gradient_is_the_central_finite_difference_of_the_loss(T):
    B, n_aux, h = 23, 3, 1e-6
    d, z = _inputs(B, n_aux)
    g = rl.gradient(d, z, n_aux, T)
    fd = np.zeros((B, n_aux))
    for i in range(B):
        for k in range(n_aux):
            zp, zm = z.copy(), z.copy()
            zp[i, k] += h
            zm[i, k] -= h
            fd[i, k] = (rl.loss(d, zp, n_aux, T) - rl.loss(d, zm, n_aux, T)) / (2.0 * h)
    scale = np.abs(fd).max()
    assert scale > 1e-3                                   # (a gradient worth comparing)
    assert np.abs(g - fd).max() <= 1e-7 * scale, (np.abs(g - fd).max(), scale)


@pytest.mark.parametrize("T", [0.05, 1.0, 20.0])
@pytest.mark.parametrize("B", [9, 600])                  # (600: more than one block of the blockwise pass)
def test_reference_is_autograd_of_the_literal_formula(B, T):
    n_aux = 3
    d, z = rl.make_inputs(B, n_aux, n_aux, n_aux + 1, seed=B)
    ref = rl.evaluate(d, z, n_aux, T)
    dt = torch.tensor(d[:, :n_aux], dtype=torch.float64)
    zt = torch.tensor(z[:, :n_aux], dtype=torch.float64, requires_grad=True)
    total = torch.zeros((), dtype=torch.float64)
    for k in range(n_aux):
        rows = torch.isfinite(dt[:, k])
        m = int(rows.sum())
        dk, zk = dt[rows, k], zt[rows, k]
        s = torch.sign(dk[:, None] - dk[None, :])
        x = -s * (zk[:, None] - zk[None, :]) / T
        # (threshold: torch returns x itself above it -- 1e-13 off in value and slope at 30, 2e-9 at its default 20)
        total = total + T / max(m * m - m, 1) * (torch.nn.functional.softplus(x, threshold=30.0) * (s != 0)).sum()
    total = total / n_aux
    total.backward()
    assert ref["loss"] == pytest.approx(float(total.detach()), rel=1e-12)
    np.testing.assert_allclose(ref["dz"], zt.grad.numpy(), rtol=1e-11, atol=1e-18)
    assert (ref["m"] == np.isfinite(d[:, :n_aux]).sum(axis=0)).all()
    # the bound sums are sums of magnitudes of the same terms
    assert (ref["A"] >= np.abs(ref["dz"]) * n_aux * ref["norm"] / 2.0 * (1.0 - 1e-12)).all()
    assert (ref["E"] >= 4.0 * ref["A"] * (1.0 - 1e-12)).all() and (ref["lossE"] >= 4.0 * ref["lossA"] * (1.0 - 1e-12)).all()


def test_well_ordered_and_widely_separated_styles_have_no_loss_and_no_gradient():
    B, n_aux = 12, 2
    d = np.stack([np.arange(B, dtype=np.float64), -np.arange(B, dtype=np.float64)], axis=1)
    for sep, tol in ((10.0, 1e-3), (50.0, 1e-20)):
        ref = rl.evaluate(d, sep * d, n_aux, 1.0)
        assert 0.0 < ref["loss"] < tol and np.abs(ref["dz"]).max() < tol
    # ... and the same pairs the wrong way round: the hinge, whose gradient is the linear loss's
    ref = rl.evaluate(d, -50.0 * d, n_aux, 1.0)
    norm = B * B - B
    gaps = np.abs(np.arange(B)[:, None] - np.arange(B)[None, :]).sum()
    assert ref["loss"] == pytest.approx(50.0 * gaps / norm, rel=1e-12)
    lin = -2.0 / (n_aux * norm) * np.sign(d[:, None, :] - d[None, :, :]).sum(axis=1)
    np.testing.assert_allclose(ref["dz"], lin, rtol=1e-12)


@pytest.mark.parametrize("T", [0.05, 1.0, 20.0])
def test_equal_styles_give_ln2_per_untied_pair(T):
    B, n_aux = 17, 3
    d, _ = rl.make_inputs(B, n_aux, n_aux, n_aux, seed=5)
    ref = rl.evaluate(d, np.full((B, n_aux), 0.75), n_aux, T)
    assert ref["untied"][:2].min() > 0
    expect = sum(T * math.log(2.0) * u / n for u, n in zip(ref["untied"], ref["norm"])) / n_aux
    assert ref["loss"] == pytest.approx(expect, rel=1e-13)
    # sigma = 1/2 on every such pair: half the linear loss's gradient
    dd = np.where(np.isfinite(d), d, 0.0).astype(np.float64)
    lab = np.isfinite(d)
    s = np.sign(dd[:, None, :] - dd[None, :, :]) * (lab[:, None, :] & lab[None, :, :])
    np.testing.assert_allclose(ref["dz"], -2.0 / (n_aux * ref["norm"]) * 0.5 * s.sum(axis=1), rtol=1e-13, atol=1e-18)


def test_unlabelled_rows_and_descriptors_with_fewer_than_two_labels_give_exact_zeros():
    B, n_aux = 33, 4
    d, z = rl.make_inputs(B, n_aux, n_aux, n_aux, seed=7)
    ref = rl.evaluate(d, z, n_aux, 1.0)
    lab = np.isfinite(d)
    assert ref["m"][n_aux - 1] == 1 and (~lab).all(axis=1).any()
    assert (ref["dz"][~lab] == 0.0).all()
    assert (ref["dz"][:, n_aux - 1] == 0.0).all() and ref["untied"][n_aux - 1] == 0
    only = rl.evaluate(d[:, n_aux - 1:], z[:, n_aux - 1:], 1, 1.0)
    assert only["loss"] == 0.0 and not only["dz"].any()
    assert np.isfinite(ref["loss"]) and np.isfinite(ref["dz"]).all()
    # ties contribute nothing
    tied = rl.evaluate(np.ones((5, 1)), np.arange(5.0)[:, None], 1, 1.0)
    assert tied["loss"] == 0.0 and not tied["dz"].any()


def test_accumulator_terms_follow_the_launch_geometry():
    assert rl.accumulator_terms(2, 1) == 1 + 3 + 1 + 2
    assert rl.accumulator_terms(257, 5) == 33 + 3 + 1 + 2
    import loss_reference as lr
    R, nj, jchunk, nwg = lr.rank_grid(4099, 4099, 5)
    assert nj > 1 and rl.accumulator_terms(4099, 5) == jchunk // 8 + 3 + nj + 2


# ------------------------------------------------------------------------------------------------ the keys
def test_defaults_and_accepted_values():
    assert rank_loss_form_of({}) == ("linear", None) and rank_loss_form_of({"rank_loss_form": None}) == ("linear", None)
    assert rank_loss_form_of({"rank_loss_form": "linear", "rank_temperature": None}) == ("linear", None)
    assert rank_loss_form_of({"rank_loss_form": "logistic"}) == ("logistic", 1.0)
    assert rank_loss_form_of({"rank_loss_form": "logistic", "rank_temperature": 0.05}) == ("logistic", 0.05)
    form, T = rank_loss_form_of(Parameters({"rank_loss_form": "logistic", "rank_temperature": 2}))
    assert form == "logistic" and T == 2.0 and isinstance(T, float)
    # local pairs run the same kernel on every shard
    assert rank_loss_form_of({"rank_loss_form": "logistic"}, world_size=2) == ("logistic", 1.0)
    assert rank_loss_form_of({"rank_loss_form": "logistic", "rank_loss_pairs": "local"}, world_size=4) == ("logistic", 1.0)
    assert rank_loss_form_of({"rank_loss_form": "logistic", "rank_loss_pairs": "global"}, world_size=1) == ("logistic", 1.0)
    assert rank_loss_form_of({"rank_loss_pairs": "global"}, world_size=2) == ("linear", None)


@pytest.mark.parametrize("bad", ["hinge", "Logistic", "", 1, True])
def test_any_other_form_is_refused(bad):
    with pytest.raises(ValueError, match="rank_loss_form must be 'linear' or 'logistic'"):
        rank_loss_form_of({"rank_loss_form": bad})


BAD_T = [0, -1, float("nan"), float("inf"), "1", True, 1e-60, 1e60]      # (the last two: 0 and Inf as fp32)


@pytest.mark.parametrize("bad", BAD_T)
def test_bad_temperatures_are_refused(bad):
    with pytest.raises(ValueError, match="rank_temperature must be a finite number > 0"):
        rank_loss_form_of({"rank_loss_form": "logistic", "rank_temperature": bad})


@pytest.mark.parametrize("cfg", [{"rank_temperature": 1.0}, {"rank_loss_form": "linear", "rank_temperature": 0.5}])
def test_temperature_without_logistic_is_refused(cfg):
    with pytest.raises(ValueError, match="rank_temperature: with rank_loss_form: logistic only"):
        rank_loss_form_of(cfg)


def test_global_pairs_under_data_parallelism_are_refused():
    with pytest.raises(ValueError, match="rank_loss_form: logistic: rank_loss_pairs: local only"):
        rank_loss_form_of({"rank_loss_form": "logistic", "rank_loss_pairs": "global"}, world_size=2)


@pytest.mark.parametrize("cfg", [{"rank_loss_form": "hinge"}, {"rank_loss_form": "logistic", "rank_temperature": 0},
                                 {"rank_loss_form": "logistic", "rank_temperature": "1"}, {"rank_temperature": 1.0}])
def test_engine_and_trainer_refuse_bad_keys_before_the_gpu(cfg, monkeypatch):
    from rankaae_amd.engine import StepEngine
    from rankaae_amd.trainer import Trainer
    with pytest.raises(ValueError, match="rank_loss_form|rank_temperature"):
        StepEngine(None, None, None, cfg, torch.device("cpu"))

    def no_gpu(*a, **kw):
        raise AssertionError("Trainer.from_data was called")
    monkeypatch.setattr(Trainer, "from_data", no_gpu)
    full = Parameters(dict({"gradient_reversal": True, "use_cnn_discriminator": False, "optimizer_name": "AdamW"}, **cfg))
    with pytest.raises(ValueError, match="rank_loss_form|rank_temperature"):
        Trainer(None, None, None, torch.device("cpu"), None, None, verbose=False, config_parameters=full)


def test_engine_refuses_global_pairs_before_the_gpu():
    from rankaae_amd.engine import StepEngine
    with pytest.raises(ValueError, match="rank_loss_form: logistic: rank_loss_pairs: local only"):
        StepEngine(None, None, None, {"rank_loss_form": "logistic", "rank_loss_pairs": "global"}, torch.device("cpu"),
                   world_size=2)


def test_resume_fingerprint_carries_the_keys_only_when_set():
    spec = np.ones((4, 8), dtype=np.float32)
    fp = lambda cfg: resume.fingerprint(cfg, 1, 640, 4, 2, spec)       # noqa: E731
    base = {"ae_form": "FC", "nstyle": 2}
    assert "cfg.rank_loss_form" not in fp(base) and "cfg.rank_temperature" not in fp(base)
    assert fp(base) == fp(dict(base, rank_loss_form=None, rank_temperature=None))
    one = fp(dict(base, rank_loss_form="logistic"))
    assert one["cfg.rank_loss_form"] == "logistic" and "cfg.rank_temperature" not in one
    two = fp(dict(base, rank_loss_form="logistic", rank_temperature=2))
    assert two["cfg.rank_temperature"] == 2.0
    with pytest.raises(ValueError, match="cfg.rank_temperature"):
        resume.check_fingerprint(two, fp(dict(base, rank_loss_form="logistic", rank_temperature=0.5)))
    with pytest.raises(ValueError, match="cfg.rank_loss_form"):
        resume.check_fingerprint(fp(base), one)


def test_trial_batch_wants_its_engines_to_agree_on_the_form():
    from rankaae_amd.trial_batch import TrialBatch
    stream = object()

    def engine(form, T=None):
        return types.SimpleNamespace(rng_mode="philox", world_size=1, bf16=False, tile_mult=1, stream=stream,
                                     aux_missing=False, grad_clip=None, ema_decay=None, spec_shift=None,
                                     spec_broaden=None, rank_metrics=False, style_decorr=None, rank_loss_form=form,
                                     rank_temperature=T, cfg={})
    with pytest.raises(ValueError, match="the engines of a TrialBatch must agree on rank_loss_form"):
        TrialBatch([engine("logistic", 1.0), engine("linear")])
    with pytest.raises(ValueError, match="the engines of a TrialBatch must agree on rank_loss_form"):
        TrialBatch([engine("linear"), engine("logistic", 0.5)])
    assert TrialBatch([engine("logistic", 0.5), engine("logistic", 2.0)]).T == 2     # the temperatures may differ
    assert TrialBatch([engine("linear"), engine("linear")]).T == 2
