"""``spec_shift`` without a GPU: the key's validation and the modes it needs, the resume fingerprint, and the properties
of the float64 reference of the draw and the resampling (``augment_reference``)."""
import numpy as np
import pytest
import torch

import augment_reference as ar
from rankaae_amd import resume
from rankaae_amd.parameter import Parameters, spec_shift_of

BAD = [0, 0.0, -1, -0.5, float("nan"), float("inf"), float("-inf"), "2", True, False]


def test_absent_null_and_positive_numbers_are_accepted():
    assert spec_shift_of({}) is None and spec_shift_of({"spec_shift": None}) is None
    assert spec_shift_of({"spec_shift": 0.5}) == 0.5 and spec_shift_of({"spec_shift": 3}) == 3.0
    assert isinstance(spec_shift_of({"spec_shift": np.float64(2.75)}), float)
    assert spec_shift_of(Parameters({"spec_shift": 2.0, "rng_mode": "philox", "fused_step_begin": True})) == 2.0


@pytest.mark.parametrize("bad", BAD)
def test_key_refuses_what_is_not_a_finite_number_above_zero(bad):
    with pytest.raises(ValueError, match="spec_shift"):
        spec_shift_of({"spec_shift": bad})


@pytest.mark.parametrize("bad", BAD)
def test_trainer_refuses_a_bad_key_before_the_gpu(bad, monkeypatch):
    from rankaae_amd.trainer import Trainer

    def no_gpu(*a, **kw):
        raise AssertionError("Trainer.from_data was called")
    monkeypatch.setattr(Trainer, "from_data", no_gpu)
    cfg = Parameters({"gradient_reversal": True, "use_cnn_discriminator": False, "optimizer_name": "AdamW",
                      "spec_shift": bad})
    with pytest.raises(ValueError, match="spec_shift"):
        Trainer(None, None, None, torch.device("cpu"), None, None, verbose=False, config_parameters=cfg)


@pytest.mark.parametrize("bad", [0, -2.0, "2", True])
def test_engine_refuses_a_bad_key_before_the_gpu(bad):
    from rankaae_amd.engine import StepEngine
    with pytest.raises(ValueError, match="spec_shift"):
        StepEngine(None, None, None, {"spec_shift": bad}, torch.device("cpu"))


MODES = "spec_shift: device RNG with the fused step head only"


def test_key_needs_the_device_rng_and_the_fused_step_head():
    with pytest.raises(ValueError, match=MODES):
        spec_shift_of({"spec_shift": 1.0, "rng_mode": "host"})
    with pytest.raises(ValueError, match=MODES):
        spec_shift_of({"spec_shift": 1.0, "fused_step_begin": False})
    with pytest.raises(ValueError, match=MODES):
        spec_shift_of({"spec_shift": 1.0}, rng_mode="host")           # (what the engine was built with wins)
    # without the key neither mode is anybody's business here
    assert spec_shift_of({"rng_mode": "host", "fused_step_begin": False}) is None
    assert spec_shift_of({"spec_shift": None, "rng_mode": "host"}) is None


def test_engine_and_trainer_refuse_the_modes_before_the_gpu():
    from rankaae_amd.engine import StepEngine
    from rankaae_amd.trainer import Trainer
    with pytest.raises(ValueError, match=MODES):
        StepEngine(None, None, None, {"spec_shift": 1.0}, torch.device("cpu"), rng_mode="host")
    with pytest.raises(ValueError, match=MODES):
        StepEngine(None, None, None, {"spec_shift": 1.0, "fused_step_begin": False}, torch.device("cpu"))
    for over in ({"rng_mode": "host"}, {"fused_step_begin": False}):
        cfg = Parameters({"gradient_reversal": True, "use_cnn_discriminator": False, "optimizer_name": "AdamW",
                          "spec_shift": 1.0, **over})
        with pytest.raises(ValueError, match=MODES):
            Trainer(None, None, None, torch.device("cpu"), None, None, verbose=False, config_parameters=cfg)


def test_resume_fingerprint_carries_the_key_only_when_set():
    spec = np.ones((4, 8), dtype=np.float32)
    fp = lambda cfg: resume.fingerprint(cfg, 1, 640, 4, 2, spec)       # noqa: E731
    base = {"ae_form": "FC", "nstyle": 2}
    assert "cfg.spec_shift" not in fp(base) and fp(base) == fp(dict(base, spec_shift=None))
    assert fp(dict(base, spec_shift=2))["cfg.spec_shift"] == 2.0
    with pytest.raises(ValueError, match="cfg.spec_shift"):
        resume.check_fingerprint(fp(dict(base, spec_shift=2.0)), fp(dict(base, spec_shift=2.5)))
    with pytest.raises(ValueError, match="cfg.spec_shift"):
        resume.check_fingerprint(fp(base), fp(dict(base, spec_shift=2.0)))


# ------------------------------------------------------------------------------------------------ the reference
def test_lowbias32_and_the_keys_follow_the_written_out_arithmetic():
    """Python integers, masked by hand, against the ``np.uint32`` forms."""
    def lb(x):
        x ^= x >> 16
        x = (x * 0x7feb352d) & 0xFFFFFFFF
        x ^= x >> 15
        x = (x * 0x846ca68b) & 0xFFFFFFFF
        return x ^ (x >> 16)
    for x in (0, 1, 0x80000000, 0xFFFFFFFF, 123456789):
        assert int(ar.lowbias32(np.uint32(x))) == lb(x)
    assert lb(0) == 0 and lb(1) != 1
    for seed, ctr in ((0, 1), (711, 5), ((3 << 32) | 9, (1 << 32) | 7)):
        k1 = lb((seed & 0xFFFFFFFF) ^ lb(((ctr & 0xFFFFFFFF) + 0x9E3779B9) & 0xFFFFFFFF))
        k2 = lb(((seed >> 32) + 0x85EBCA6B + lb((ctr >> 32) ^ k1)) & 0xFFFFFFFF)
        assert tuple(int(k) for k in ar.step_keys(seed, ctr)) == (k1, k2)
        h0 = lb(lb((0 + ar.OFF + k1) & 0xFFFFFFFF) ^ k2)
        assert float(ar.uniforms(3, seed, ctr)[0]) == (h0 >> 8) / 2.0 ** 24


@pytest.mark.parametrize("s", [0.5, 2.75, 4.0, 300.0])
def test_every_shift_is_inside_the_interval_and_rows_differ(s):
    d = ar.deltas(4096, 711, 3, s)
    assert d.dtype == np.float32 and np.all(np.abs(d) <= np.float32(s)) and np.all(d < np.float32(s))
    assert len(np.unique(d)) > 4000                       # per-row draws
    assert d.min() < -0.9 * s and d.max() > 0.9 * s and abs(float(d.mean())) < 0.05 * s      # uniform over [-s, s)
    u = ar.uniforms(4096, 711, 3)
    assert u.dtype == np.float32 and np.all((u >= 0) & (u < 1))


def test_shifts_change_with_the_counter_and_with_the_seed():
    a, b, c = ar.deltas(64, 711, 3, 2.0), ar.deltas(64, 711, 4, 2.0), ar.deltas(64, 712, 3, 2.0)
    assert not np.array_equal(a, b) and not np.array_equal(a, c) and not np.array_equal(b, c)
    assert np.mean(a == b) < 0.1 and np.mean(a == c) < 0.1
    assert np.array_equal(a, ar.deltas(64, 711, 3, 2.0))                        # and with nothing else
    assert np.array_equal(a[:16], ar.deltas(16, 711, 3, 2.0))                   # (not with the number of rows)
    hi = (5 << 32) | 711                                                        # the seed's and counter's high words count
    assert not np.array_equal(a, ar.deltas(64, hi, 3, 2.0)) and not np.array_equal(a, ar.deltas(64, 711, (1 << 32) | 3, 2.0))


@pytest.mark.parametrize("delta", [0.0, 0.25, -0.25, 1.0, -3.5, 2.75, 0.3])
def test_ramp_shifted_stays_a_ramp_away_from_the_clamped_ends(delta):
    L = 64
    ramp = 0.5 * np.arange(L, dtype=np.float64)[None, :] + 3.0
    out = ar.shift_rows_by(ramp, np.array([delta], dtype=np.float32))
    lo, hi = int(np.ceil(max(0.0, -delta))), int(np.floor(min(L - 1, L - 1 - delta)))
    inner = np.arange(lo, hi + 1)
    want = 0.5 * (inner + float(np.float32(delta))) + 3.0
    assert inner.size >= L - 5
    np.testing.assert_allclose(out[0, inner], want, rtol=0, atol=1e-5)       # (x = l + delta is rounded to fp32)
    # the clamped ends replicate the end samples
    assert np.all(out[0, :lo] == ramp[0, 0]) and np.all(out[0, hi + 1:] == ramp[0, -1])


def test_constant_row_is_unchanged_and_zero_shift_is_the_identity():
    rows = np.full((5, 33), 1.625)
    assert np.array_equal(ar.shift_rows(rows, 9, 2, 4.0), rows)
    g = np.random.default_rng(0).standard_normal((5, 33))
    assert np.array_equal(ar.shift_rows(g, 9, 2, 0.0), g)
    assert np.array_equal(ar.shift_rows_by(g, np.zeros(5, dtype=np.float32)), g)


def test_edges_are_replicated_at_both_ends():
    L = 16
    g = np.random.default_rng(1).standard_normal((2, L))
    out = ar.shift_rows_by(g, np.array([-float(L), float(L)], dtype=np.float32))
    assert np.all(out[0] == g[0, 0]) and np.all(out[1] == g[1, -1])
    out = ar.shift_rows_by(g, np.array([-2.5, 2.5], dtype=np.float32))
    assert np.all(out[0, :3] == g[0, 0]) and out[0, 3] == g[0, 0] + 0.5 * (g[0, 1] - g[0, 0])
    assert np.all(out[1, -3:] == g[1, -1]) and out[1, -4] == g[1, -2] + 0.5 * (g[1, -1] - g[1, -2])
    i0, i1, f = ar.positions(np.array([-2.5, 2.5, 0.0], dtype=np.float32), L)
    assert i0.min() == 0 and i1.max() == L - 1 and np.all(i1 - i0 <= 1) and np.all((f >= 0) & (f < 1))
    assert np.all(f[2] == 0) and np.array_equal(i0[2], np.arange(L))


def test_whole_number_shift_moves_the_samples():
    g = np.random.default_rng(2).standard_normal((1, 20))
    out = ar.shift_rows_by(g, np.array([3.0], dtype=np.float32))
    assert np.array_equal(out[0, :17], g[0, 3:]) and np.all(out[0, 17:] == g[0, -1])
