"""``style_decorr`` without a GPU: the float64 reference of the penalty and its gradient (``decorr_reference``) against
finite differences and the cases whose answer is known, the key's validation, the resume fingerprint and the
``TrialBatch`` agreement check."""
import types

import numpy as np
import pytest
import torch

import decorr_reference as dr
from rankaae_amd import resume
from rankaae_amd.parameter import Parameters, style_decorr_of


# ------------------------------------------------------------------------------------------------ the reference
def test_gradient_is_the_central_finite_difference_of_the_penalty():
    b, k, h = 7, 3, 1e-6
    z = np.random.default_rng(0).standard_normal((b, k)) @ np.array([[1.0, 0.6, -0.3], [0.0, 1.0, 0.5], [0.0, 0.0, 1.0]])
    z += np.array([2.0, -1.0, 0.5])
    g = dr.gradient(z)
    fd = np.zeros_like(z)
    for r in range(b):
        for i in range(k):
            zp, zm = z.copy(), z.copy()
            zp[r, i] += h
            zm[r, i] -= h
            fd[r, i] = (dr.penalty(zp) - dr.penalty(zm)) / (2.0 * h)
    scale = np.abs(fd).max()
    assert scale > 1e-3                             # (a gradient worth comparing)
    assert np.abs(g - fd).max() <= 1e-7 * scale, (np.abs(g - fd).max(), scale)


def test_orthogonal_columns_have_no_penalty_and_no_gradient():
    # centred, mutually orthogonal columns: rows of a Hadamard matrix without the constant one
    z = np.array([[1, 1, 1], [-1, 1, -1], [1, -1, -1], [-1, -1, 1]], dtype=np.float64) * np.array([1.0, 2.0, 0.5]) + 3.0
    assert dr.penalty(z) == pytest.approx(0.0, abs=1e-30)
    assert np.abs(dr.gradient(z)).max() <= 1e-15


@pytest.mark.parametrize("sign", [1.0, -1.0])
def test_perfectly_correlated_columns_have_penalty_one_and_no_gradient(sign):
    a = np.random.default_rng(1).standard_normal(9)
    z = np.stack([a, sign * 2.5 * a + 4.0], axis=1)
    assert dr.penalty(z) == pytest.approx(1.0, abs=1e-14)
    assert np.abs(dr.gradient(z)).max() <= 1e-14       # D is at its maximum: u_j - C_ij u_i vanishes


def test_constant_column_is_left_out():
    rng = np.random.default_rng(2)
    y = rng.standard_normal((11, 3)) @ rng.standard_normal((3, 3))
    z = np.insert(y, 1, 0.75, axis=1)                   # k = 4, column 1 constant
    d, g = dr.penalty(z), dr.gradient(z)
    assert np.isfinite(d) and np.isfinite(g).all()
    assert not g[:, 1].any()
    # the other columns as if k were 3, up to the 1 / (k (k - 1)) factor: 3 * 2 / (4 * 3)
    assert d == pytest.approx(dr.penalty(y) * 0.5, rel=1e-13)
    np.testing.assert_allclose(g[:, [0, 2, 3]], dr.gradient(y) * 0.5, rtol=1e-12, atol=1e-15)
    assert dr.penalty(np.zeros((5, 3))) == 0.0 and not dr.gradient(np.zeros((5, 3))).any()


def test_penalty_ignores_column_shift_and_positive_scale():
    rng = np.random.default_rng(3)
    z = rng.standard_normal((13, 4)) @ rng.standard_normal((4, 4))
    z2 = z * np.array([0.1, 3.0, 7.5, 1.0]) + np.array([5.0, -2.0, 0.0, 11.0])
    assert dr.penalty(z2) == pytest.approx(dr.penalty(z), rel=1e-12)
    assert 0.0 < dr.penalty(z) < 1.0


def test_one_row_or_one_column_gives_zero():
    for shape in ((1, 4), (9, 1), (1, 1)):
        z = np.random.default_rng(4).standard_normal(shape)
        assert dr.penalty(z) == 0.0
        assert dr.gradient(z).shape == shape and not dr.gradient(z).any()


def test_test_inputs_keep_their_means_within_ten_deviations():
    for b, k in ((63, 5), (257, 64), (4099, 16)):
        z = dr.mixed_gaussian(b, k, seed=b + k).astype(np.float64)
        assert (np.abs(z.mean(axis=0)) <= 10.0 * z.std(axis=0)).all()
        c = np.abs(dr.correlation(z))[~np.eye(k, dtype=bool)]
        assert c.max() > 0.3 and c.min() < 0.1          # correlations of every size


# ------------------------------------------------------------------------------------------------ the key
def test_absent_null_and_positive_numbers_are_accepted():
    assert style_decorr_of({}) is None and style_decorr_of({"style_decorr": None}) is None
    assert style_decorr_of({"style_decorr": 0.5}) == 0.5
    assert style_decorr_of({"style_decorr": 1}) == 1.0 and isinstance(style_decorr_of({"style_decorr": 1}), float)
    assert style_decorr_of({"style_decorr": 1e-3}) == 1e-3
    assert style_decorr_of(Parameters({"style_decorr": 2.0})) == 2.0


BAD = [0, -1, float("nan"), float("inf"), "1", True]


@pytest.mark.parametrize("bad", BAD)
def test_key_refuses_everything_else(bad):
    with pytest.raises(ValueError, match="style_decorr must be absent, null or a finite number > 0"):
        style_decorr_of({"style_decorr": bad})


@pytest.mark.parametrize("bad", BAD)
def test_engine_and_trainer_refuse_a_bad_key_before_the_gpu(bad, monkeypatch):
    from rankaae_amd.engine import StepEngine
    from rankaae_amd.trainer import Trainer
    with pytest.raises(ValueError, match="style_decorr"):
        StepEngine(None, None, None, {"style_decorr": bad}, torch.device("cpu"))

    def no_gpu(*a, **kw):
        raise AssertionError("Trainer.from_data was called")
    monkeypatch.setattr(Trainer, "from_data", no_gpu)
    cfg = Parameters({"gradient_reversal": True, "use_cnn_discriminator": False, "optimizer_name": "AdamW",
                      "style_decorr": bad})
    with pytest.raises(ValueError, match="style_decorr"):
        Trainer(None, None, None, torch.device("cpu"), None, None, verbose=False, config_parameters=cfg)


def test_resume_fingerprint_carries_the_key_only_when_set():
    spec = np.ones((4, 8), dtype=np.float32)
    fp = lambda cfg: resume.fingerprint(cfg, 1, 640, 4, 2, spec)       # noqa: E731
    base = {"ae_form": "FC", "nstyle": 2}
    assert "cfg.style_decorr" not in fp(base) and fp(base) == fp(dict(base, style_decorr=None))
    assert fp(dict(base, style_decorr=1))["cfg.style_decorr"] == 1.0
    with pytest.raises(ValueError, match="cfg.style_decorr"):
        resume.check_fingerprint(fp(dict(base, style_decorr=0.5)), fp(dict(base, style_decorr=1.0)))
    with pytest.raises(ValueError, match="cfg.style_decorr"):
        resume.check_fingerprint(fp(base), fp(dict(base, style_decorr=0.5)))


def test_trial_batch_wants_its_engines_to_agree_on_whether_the_key_is_set():
    from rankaae_amd.trial_batch import TrialBatch
    stream = object()

    def engine(style_decorr):
        return types.SimpleNamespace(rng_mode="philox", world_size=1, bf16=False, tile_mult=1, stream=stream,
                                     aux_missing=False, grad_clip=None, ema_decay=None, spec_shift=None,
                                     spec_broaden=None, rank_metrics=False, style_decorr=style_decorr, cfg={})
    with pytest.raises(ValueError, match="the engines of a TrialBatch must agree on whether style_decorr is set"):
        TrialBatch([engine(0.5), engine(None)])
    with pytest.raises(ValueError, match="the engines of a TrialBatch must agree on whether style_decorr is set"):
        TrialBatch([engine(None), engine(2.0)])
    assert TrialBatch([engine(0.5), engine(2.0)]).T == 2          # the values may differ
    assert TrialBatch([engine(None), engine(None)]).T == 2
