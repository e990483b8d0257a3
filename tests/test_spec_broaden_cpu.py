"""``spec_broaden`` without a GPU: the properties of the float64 reference of the draw and the convolution
(``broaden_reference``), the key's validation and the modes it needs, and the resume fingerprint."""
import math

import numpy as np
import pytest
import torch

import augment_reference as ar
import broaden_reference as br
from rankaae_amd import resume
from rankaae_amd.parameter import Parameters, spec_broaden_of

BAD = [0, 0.0, -1, -0.5, float("nan"), float("inf"), float("-inf"), "1", True, False, 21.5, 22, 1e9, 715827883,
       1e10, 3e38, 1e39, 1e300]       # (3e38: finite in fp32, its product is not; 1e39, 1e300: Inf in fp32)


# ------------------------------------------------------------------------------------------------ the reference
@pytest.mark.parametrize("sigma", [0.3, 1.7, 4.0])
def test_reference_is_scipys_gaussian_filter(sigma):
    """``gaussian_filter1d(row, sigma, mode="nearest", radius=R)``: the same truncated, normalised kernel and the same
    replicated edges, to 1e-12 (the fp32 value of sigma on both sides)."""
    from scipy import ndimage
    R = 12
    rows = np.random.default_rng(3).standard_normal((4, 50)) + np.linspace(0.0, 3.0, 50)[None, :]
    s32 = np.float32(sigma)
    got = br.broaden_rows_by(rows, np.full(4, s32), R)
    for b in range(4):
        want = ndimage.gaussian_filter1d(rows[b], float(s32), mode="nearest", radius=R)
        assert np.abs(got[b] - want).max() <= 1e-12
    assert np.abs(got - rows).max() > 1e-3


@pytest.mark.parametrize("sigma", [0.05, 0.4, 2.5, 21.0])
def test_constant_row_is_unchanged(sigma):
    rows = np.full((3, 33), 1.625)
    out = br.broaden_rows_by(rows, np.full(3, sigma, dtype=np.float32), br.radius(sigma))
    assert np.abs(out - rows).max() <= 4e-16 * 1.625


def test_zero_sigma_is_the_identity():
    g = np.random.default_rng(0).standard_normal((5, 33))
    g[1, 4] = -0.0
    out = br.broaden_rows_by(g, np.zeros(5, dtype=np.float32), 12)
    assert np.array_equal(out, g) and np.signbit(out[1, 4])
    assert np.array_equal(br.augment(g, 9, 2, 0.0, 0.0), g)
    # rows with sigma == 0 among rows with sigma > 0 stay themselves
    mixed = br.broaden_rows_by(g, np.array([0, 1.5, 0, 0.5, 0], dtype=np.float32), 5)
    assert np.array_equal(mixed[[0, 2, 4]], g[[0, 2, 4]]) and not np.array_equal(mixed[1], g[1])


@pytest.mark.parametrize("sigma,R", [(0.4, 2), (2.5, 8), (4.0, 12)])
def test_spike_keeps_its_mass_away_from_the_ends(sigma, R):
    L = 64
    rows = np.zeros((2, L))
    rows[0, R + 1], rows[1, L - R - 2] = 3.0, -2.0        # more than R points from both ends
    out = br.broaden_rows_by(rows, np.full(2, sigma, dtype=np.float32), R)
    assert abs(out[0].sum() - 3.0) <= 1e-14 and abs(out[1].sum() + 2.0) <= 1e-14
    near = np.zeros((1, L))
    near[0, 0] = 1.0                                      # at the end the replicated halo repeats it: 1 + sum_(j>0) (j - 1) w_j / W
    w = br.weights(np.float32(sigma), R)
    extra = (np.arange(0, R) * w[R + 1:]).sum() / w.sum()
    assert abs(br.broaden_rows_by(near, np.full(1, sigma, dtype=np.float32), R)[0].sum() - (1.0 + extra)) <= 1e-14 and extra > 1e-6


@pytest.mark.parametrize("sigma", [1.0, 2.5, 4.0])
def test_second_moment_rises_by_sigma_squared_within_the_truncation(sigma):
    """A spike broadened by the kernel truncated at ``R = ceil(3 sigma)`` has the truncated Gaussian's variance
    ``V_R = sum_{|j|<=R} j^2 w_j / sum_{|j|<=R} w_j`` exactly, and that is below ``sigma^2`` by the missing tail:

        sigma^2 - V_R = (sum_{|j|>R} (j^2 - V_R) w_j) / W_inf <= (2 / W_R) * sum_{j>R} j^2 exp(-j^2 / (2 sigma^2)).

    ``j^2 exp(-j^2 / 2 sigma^2)`` decreases for ``j > sqrt(2) sigma``, so the sum is below the integral from ``R``:
    ``I(R) = sigma^2 R exp(-R^2 / 2 sigma^2) + sigma^3 sqrt(pi / 2) erfc(R / (sqrt(2) sigma))``.  (The discrete
    Gaussian's full variance differs from ``sigma^2`` by ``O(exp(-2 pi^2 sigma^2))``: 3e-9 at ``sigma = 1``, added.)"""
    s32 = float(np.float32(sigma))
    R, L = br.radius(sigma), 101
    rows = np.zeros((1, L))
    rows[0, 50] = 1.0
    out = br.broaden_rows_by(rows, np.array([sigma], dtype=np.float32), R)[0]
    x = np.arange(L) - 50.0
    assert abs(out.sum() - 1.0) <= 1e-14 and abs((out * x).sum()) <= 1e-13
    var = (out * x * x).sum()
    W_R = br.weights(np.float32(sigma), R).sum()
    tail = s32 ** 2 * R * math.exp(-R * R / (2 * s32 ** 2)) + s32 ** 3 * math.sqrt(math.pi / 2) * math.erfc(R / (math.sqrt(2) * s32))
    slack = 2.0 * tail / W_R + 4.0 * s32 ** 2 * math.exp(-2 * math.pi ** 2 * s32 ** 2) * (1 + 4 * math.pi ** 2 * s32 ** 2) + 1e-12
    print(f"sigma {sigma}: variance {var:.6f}, sigma^2 {s32 ** 2:.6f}, allowed deficit {slack:.4f}")
    assert s32 ** 2 - slack <= var <= s32 ** 2 + 1e-12
    assert slack < 0.15 * s32 ** 2                        # (the bound says something: R >= 3 sigma)


def test_edges_are_replicated_not_zero_padded():
    g = np.random.default_rng(1).standard_normal((1, 16)) + 5.0
    sig = np.array([2.0], dtype=np.float32)
    edge, zero = br.broaden_rows_by(g, sig, 6), br.broaden_rows_by(g, sig, 6, pad="constant")
    assert np.allclose(edge[0, 6:10], zero[0, 6:10], rtol=0, atol=1e-15)
    assert edge[0, 0] > zero[0, 0] + 1.0 and edge[0, -1] > zero[0, -1] + 1.0
    w = br.weights(sig[0], 6)
    want0 = (w[:6].sum() * g[0, 0] + (w[6:] * g[0, :7]).sum()) / w.sum()
    assert abs(edge[0, 0] - want0) <= 1e-14
    # R > L: every tap beyond the row is an end sample
    tiny = np.array([[1.0, 2.0, 4.0, 8.0]])
    t = br.taps(tiny, 8)
    assert t.shape == (1, 4, 17) and np.all(t[0, 0, :8] == 1.0) and np.all(t[0, 3, 9:] == 8.0)


# ------------------------------------------------------------------------------------------------ the draw
@pytest.mark.parametrize("s", [0.4, 2.0, 21.0])
def test_every_sigma_is_inside_the_interval_and_rows_differ(s):
    d = br.sigmas(4096, 711, 3, s)
    assert d.dtype == np.float32 and np.all(d >= 0) and np.all(d < np.float32(s))
    assert len(np.unique(d)) > 4000
    assert d.min() < 0.05 * s and d.max() > 0.95 * s and abs(float(d.mean()) - 0.5 * s) < 0.03 * s
    v = br.unit_draws(4096, 711, 3)
    assert v.dtype == np.float32 and np.all((v >= 0) & (v < 1))


def test_draw_follows_the_written_out_arithmetic():
    def lb(x):
        x ^= x >> 16
        x = (x * 0x7feb352d) & 0xFFFFFFFF
        x ^= x >> 15
        x = (x * 0x846ca68b) & 0xFFFFFFFF
        return x ^ (x >> 16)
    for seed, ctr in ((0, 1), (711, 5), ((3 << 32) | 9, (1 << 32) | 7)):
        k1, k2 = (int(k) for k in ar.step_keys(seed, ctr))
        for b in (0, 1, 77):
            g = lb(lb((b + 0xC0000000 + k1) & 0xFFFFFFFF) ^ k2)
            assert float(br.unit_draws(78, seed, ctr)[b]) == (g >> 8) / 2.0 ** 24
            assert br.sigmas(78, seed, ctr, 2.5)[b] == np.float32((g >> 8) / 2.0 ** 24) * np.float32(2.5)
    assert br.OFF == 0xC0000000 and br.radius(21.0) == 63 and br.radius(21.5) == 65 and br.radius(0.4) == 2 and br.radius(0.0) == 0


def test_sigmas_change_with_the_counter_and_the_seed_and_are_not_the_shifts_draws():
    a, b, c = br.sigmas(64, 711, 3, 2.0), br.sigmas(64, 711, 4, 2.0), br.sigmas(64, 712, 3, 2.0)
    assert np.mean(a == b) < 0.1 and np.mean(a == c) < 0.1 and np.mean(b == c) < 0.1
    assert np.array_equal(a, br.sigmas(64, 711, 3, 2.0)) and np.array_equal(a[:16], br.sigmas(16, 711, 3, 2.0))
    hi = (5 << 32) | 711
    assert not np.array_equal(a, br.sigmas(64, hi, 3, 2.0)) and not np.array_equal(a, br.sigmas(64, 711, (1 << 32) | 3, 2.0))
    # the hash index range of the widths is not the shifts': the unit draws of the same rows differ
    v, u = br.unit_draws(4096, 711, 3), ar.uniforms(4096, 711, 3)
    assert np.mean(v == u) < 0.01 and abs(float(np.corrcoef(v, u)[0, 1])) < 0.05
    assert br.OFF != ar.OFF and br.OFF - ar.OFF == 2 ** 30


def test_augment_is_broadening_followed_by_the_shift():
    rows = np.random.default_rng(5).standard_normal((6, 40))
    g = br.broaden_rows_by(rows, br.sigmas(6, 9, 2, 2.5), br.radius(2.5))
    assert np.array_equal(br.augment(rows, 9, 2, 2.5, 0.0), g)
    assert np.array_equal(br.augment(rows, 9, 2, 2.5, 2.75), ar.shift_rows(g, 9, 2, 2.75))
    assert np.array_equal(br.augment(rows, 9, 2, 0.0, 2.75), ar.shift_rows(rows, 9, 2, 2.75))


# ------------------------------------------------------------------------------------------------ the key
def test_absent_null_and_numbers_in_range_are_accepted():
    assert spec_broaden_of({}) is None and spec_broaden_of({"spec_broaden": None}) is None
    assert spec_broaden_of({"spec_broaden": 0.5}) == 0.5 and spec_broaden_of({"spec_broaden": 3}) == 3.0
    assert spec_broaden_of({"spec_broaden": 21}) == 21.0
    assert isinstance(spec_broaden_of({"spec_broaden": np.float64(2.75)}), float)
    assert spec_broaden_of(Parameters({"spec_broaden": 2.0, "rng_mode": "philox", "fused_step_begin": True})) == 2.0
    assert spec_broaden_of({"spec_broaden": 2.0, "spec_shift": 1.0}) == 2.0


def test_host_radius_is_the_kernels():
    from rankaae_amd.parameter import spec_broaden_radius
    for s in (0.1, 0.4, 1.0 / 3.0, 2.0, 2.5, 21.0, 21.3, 64.0 / 3.0, 21.333333333, 21.34, 21.5):
        assert spec_broaden_radius(s) == br.radius(s), s


@pytest.mark.parametrize("bad", BAD)
def test_key_refuses_what_is_outside_the_range(bad):
    with pytest.raises(ValueError, match=r"spec_broaden must be .*0 < s and ceil\(3 s\) <= 64"):
        spec_broaden_of({"spec_broaden": bad})


@pytest.mark.parametrize("bad", BAD)
def test_trainer_refuses_a_bad_key_before_the_gpu(bad, monkeypatch):
    from rankaae_amd.trainer import Trainer

    def no_gpu(*a, **kw):
        raise AssertionError("Trainer.from_data was called")
    monkeypatch.setattr(Trainer, "from_data", no_gpu)
    cfg = Parameters({"gradient_reversal": True, "use_cnn_discriminator": False, "optimizer_name": "AdamW",
                      "spec_broaden": bad})
    with pytest.raises(ValueError, match="spec_broaden"):
        Trainer(None, None, None, torch.device("cpu"), None, None, verbose=False, config_parameters=cfg)


@pytest.mark.parametrize("bad", [0, -2.0, "1", True, 21.5])
def test_engine_refuses_a_bad_key_before_the_gpu(bad):
    from rankaae_amd.engine import StepEngine
    with pytest.raises(ValueError, match="spec_broaden"):
        StepEngine(None, None, None, {"spec_broaden": bad}, torch.device("cpu"))


MODES = "spec_broaden: device RNG with the fused step head only"


def test_key_needs_the_device_rng_and_the_fused_step_head():
    with pytest.raises(ValueError, match=MODES):
        spec_broaden_of({"spec_broaden": 1.0, "rng_mode": "host"})
    with pytest.raises(ValueError, match=MODES):
        spec_broaden_of({"spec_broaden": 1.0, "fused_step_begin": False})
    with pytest.raises(ValueError, match=MODES):
        spec_broaden_of({"spec_broaden": 1.0}, rng_mode="host")
    assert spec_broaden_of({"rng_mode": "host", "fused_step_begin": False}) is None
    assert spec_broaden_of({"spec_broaden": None, "rng_mode": "host"}) is None


def test_engine_and_trainer_refuse_the_modes_before_the_gpu():
    from rankaae_amd.engine import StepEngine
    from rankaae_amd.trainer import Trainer
    with pytest.raises(ValueError, match=MODES):
        StepEngine(None, None, None, {"spec_broaden": 1.0}, torch.device("cpu"), rng_mode="host")
    with pytest.raises(ValueError, match=MODES):
        StepEngine(None, None, None, {"spec_broaden": 1.0, "fused_step_begin": False}, torch.device("cpu"))
    for over in ({"rng_mode": "host"}, {"fused_step_begin": False}):
        cfg = Parameters({"gradient_reversal": True, "use_cnn_discriminator": False, "optimizer_name": "AdamW",
                          "spec_broaden": 1.0, **over})
        with pytest.raises(ValueError, match=MODES):
            Trainer(None, None, None, torch.device("cpu"), None, None, verbose=False, config_parameters=cfg)


def test_resume_fingerprint_carries_the_key_only_when_set():
    spec = np.ones((4, 8), dtype=np.float32)
    fp = lambda cfg: resume.fingerprint(cfg, 1, 640, 4, 2, spec)       # noqa: E731
    base = {"ae_form": "FC", "nstyle": 2}
    assert "cfg.spec_broaden" not in fp(base) and fp(base) == fp(dict(base, spec_broaden=None))
    assert fp(dict(base, spec_broaden=2))["cfg.spec_broaden"] == 2.0
    assert "cfg.spec_shift" not in fp(dict(base, spec_broaden=2))
    with pytest.raises(ValueError, match="cfg.spec_broaden"):
        resume.check_fingerprint(fp(dict(base, spec_broaden=2.0)), fp(dict(base, spec_broaden=2.5)))
    with pytest.raises(ValueError, match="cfg.spec_broaden"):
        resume.check_fingerprint(fp(base), fp(dict(base, spec_broaden=2.0)))
