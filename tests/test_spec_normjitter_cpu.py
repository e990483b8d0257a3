"""``spec_gain`` and ``spec_tilt`` without a GPU: the keys' validation and the modes they need, the fp32 emulation of
the stage (``normjitter_reference``) against its float64 form, the statistics of the draws and the separation of the
four hash index ranges, the resume fingerprint and the ``TrialBatch`` agreement check."""
import types

import numpy as np
import pytest
import torch

import augment_reference as ar
import broaden_reference as br
import normjitter_reference as nj
from rankaae_amd import resume
from rankaae_amd.parameter import Parameters, spec_gain_of, spec_tilt_of

OF = {"spec_gain": spec_gain_of, "spec_tilt": spec_tilt_of}
BAD_BOTH = [0, 0.0, -1, -0.5, -1e-9, float("nan"), float("inf"), float("-inf"), "0.1", "1", True, False, [0.1]]
# spec_gain: 1 and above; 1 - 1e-12 is 1 as the kernel sees it (fp32).  spec_tilt: beyond fp32 (Inf there), beyond float
BAD = {"spec_gain": BAD_BOTH + [1, 1.0, 1.5, 2, 1e9, 1.0 - 1e-12], "spec_tilt": BAD_BOTH + [1e39, 1e300, 10 ** 400]}
GOOD = {"spec_gain": [0.03, 0.5, 0.999, 1e-6, np.float64(0.25)], "spec_tilt": [0.02, 1, 3, 250.0, 1e30, np.float64(0.25)]}
MUST = {"spec_gain": r"spec_gain must be .*0 < a < 1", "spec_tilt": r"spec_tilt must be .*finite number > 0"}


# ------------------------------------------------------------------------------------------------ the keys
@pytest.mark.parametrize("key", list(OF))
def test_absent_null_and_numbers_in_range_are_accepted(key):
    of = OF[key]
    assert of({}) is None and of({key: None}) is None
    for v in GOOD[key]:
        got = of({key: v})
        assert isinstance(got, float) and got == float(v)
    assert of(Parameters({key: 0.25, "rng_mode": "philox", "fused_step_begin": True})) == 0.25


def test_each_key_may_be_set_without_the_other_and_beside_its_siblings():
    assert spec_gain_of({"spec_gain": 0.05}) == 0.05 and spec_tilt_of({"spec_gain": 0.05}) is None
    assert spec_tilt_of({"spec_tilt": 0.02}) == 0.02 and spec_gain_of({"spec_tilt": 0.02}) is None
    both = {"spec_gain": 0.05, "spec_tilt": 0.02, "spec_shift": 1.0, "spec_broaden": 2.0}
    assert spec_gain_of(both) == 0.05 and spec_tilt_of(both) == 0.02


@pytest.mark.parametrize("key,bad", [(k, b) for k in BAD for b in BAD[k]])
def test_key_refuses_what_is_outside_the_range(key, bad):
    with pytest.raises(ValueError, match=MUST[key]):
        OF[key]({key: bad})


@pytest.mark.parametrize("key,bad", [(k, b) for k in BAD for b in BAD[k]])
def test_trainer_refuses_a_bad_key_before_the_gpu(key, bad, monkeypatch):
    from rankaae_amd.trainer import Trainer

    def no_gpu(*a, **kw):
        raise AssertionError("Trainer.from_data was called")
    monkeypatch.setattr(Trainer, "from_data", no_gpu)
    cfg = Parameters({"gradient_reversal": True, "use_cnn_discriminator": False, "optimizer_name": "AdamW", key: bad})
    with pytest.raises(ValueError, match=key):
        Trainer(None, None, None, torch.device("cpu"), None, None, verbose=False, config_parameters=cfg)


@pytest.mark.parametrize("key,bad", [(k, b) for k in BAD for b in (0, -2.0, "1", True, float("nan"))] + [("spec_gain", 1.0)])
def test_engine_refuses_a_bad_key_before_the_gpu(key, bad):
    from rankaae_amd.engine import StepEngine
    with pytest.raises(ValueError, match=key):
        StepEngine(None, None, None, {key: bad}, torch.device("cpu"))


@pytest.mark.parametrize("key", list(OF))
def test_key_needs_the_device_rng_and_the_fused_step_head(key):
    from rankaae_amd.engine import StepEngine
    from rankaae_amd.trainer import Trainer
    of, modes = OF[key], f"{key}: device RNG with the fused step head only"
    with pytest.raises(ValueError, match=modes):
        of({key: 0.25, "rng_mode": "host"})
    with pytest.raises(ValueError, match=modes):
        of({key: 0.25, "fused_step_begin": False})
    with pytest.raises(ValueError, match=modes):
        of({key: 0.25}, rng_mode="host")
    assert of({"rng_mode": "host", "fused_step_begin": False}) is None
    assert of({key: None, "rng_mode": "host"}) is None
    with pytest.raises(ValueError, match=modes):
        StepEngine(None, None, None, {key: 0.25}, torch.device("cpu"), rng_mode="host")
    with pytest.raises(ValueError, match=modes):
        StepEngine(None, None, None, {key: 0.25, "fused_step_begin": False}, torch.device("cpu"))
    for over in ({"rng_mode": "host"}, {"fused_step_begin": False}):
        cfg = Parameters({"gradient_reversal": True, "use_cnn_discriminator": False, "optimizer_name": "AdamW",
                          key: 0.25, **over})
        with pytest.raises(ValueError, match=modes):
            Trainer(None, None, None, torch.device("cpu"), None, None, verbose=False, config_parameters=cfg)


# ------------------------------------------------------------------------------------------------ the emulation
def _rows(B, L, seed=0):
    g = np.random.default_rng(1000 * B + L + seed)
    x = (g.standard_normal((B, L)) + np.linspace(0.0, 4.0, L)[None, :]).astype(np.float32)
    x[0, 0] = 0.0
    x[B - 1, L - 1] = -37.5
    return x


@pytest.mark.parametrize("a,t", [(0.05, 0.02), (0.9, 3.0), (0.3, 0.0), (0.0, 0.7)])
@pytest.mark.parametrize("B,L", [(3, 256), (1, 5), (2, 1), (1025, 8), (4, 8192)])
def test_emulation_is_the_float64_stage_within_one_spacing_per_rounding(B, L, a, t):
    """``|stage32 - stage64| <= stage_bound``: one fp32 spacing for each of the eight roundings of the stage, each
    weighted by what it scales (the bound's docstring); nothing in it comes from the emulation's output."""
    x = _rows(B, L)
    got, want = nj.stage32(x, 711, 3, a, t), nj.stage64(x, 711, 3, a, t)
    assert got.dtype == np.float32 and got.shape == (B, L)
    err, bound = np.abs(got.astype(np.float64) - want), nj.stage_bound(x, 711, 3, a, t)
    print(f"B {B} L {L} a {a} t {t}: max |err| {err.max():.3e}, max err / bound {(err / bound).max():.3f}")
    assert np.all(err <= bound)
    if L > 1 and (a or t):
        assert not np.array_equal(got, x)


def test_emulation_follows_the_written_out_arithmetic():
    """The hash in Python integers, the stage in ``np.float32`` scalars, one operation per line."""
    def lb(x):
        x ^= x >> 16
        x = (x * 0x7feb352d) & 0xFFFFFFFF
        x ^= x >> 15
        x = (x * 0x846ca68b) & 0xFFFFFFFF
        return x ^ (x >> 16)
    F = np.float32
    a, t, L = 0.3, 0.7, 7
    x = _rows(78, L)
    for seed, ctr in ((0, 1), (711, 5), ((3 << 32) | 9, (1 << 32) | 7)):
        k1, k2 = (int(k) for k in ar.step_keys(seed, ctr))
        out = nj.stage32(x, seed, ctr, a, t)
        for b in (0, 1, 77):
            u = F((lb(lb((b + 0xA0000000 + k1) & 0xFFFFFFFF) ^ k2) >> 8) / 2.0 ** 24)
            w = F((lb(lb((b + 0xE0000000 + k1) & 0xFFFFFFFF) ^ k2) >> 8) / 2.0 ** 24)
            assert nj.uniforms(78, seed, ctr, nj.GAIN_OFF)[b] == u and nj.uniforms(78, seed, ctr, nj.TILT_OFF)[b] == w
            g = F(F(1) + F(F(F(2) * u - F(1)) * F(a)))
            c = F(F(F(2) * w - F(1)) * F(t))
            assert nj.gains(78, seed, ctr, a)[b] == g and nj.tilts(78, seed, ctr, t)[b] == c
            for l in (0, 3, 6):
                r = F(F(2 * l - (L - 1)) / F(L - 1))
                assert out[b, l] == F(F(g * x[b, l]) + F(c * r))
    assert nj.GAIN_OFF == 0xA0000000 and nj.TILT_OFF == 0xE0000000 and nj.BMAX == 2 ** 29


def test_ramp_runs_from_minus_one_to_plus_one_and_is_zero_for_one_sample():
    for L in (2, 3, 5, 8, 256, 8192):
        r = nj.ramp(L)
        assert r.dtype == np.float32 and r[0] == -1.0 and r[-1] == 1.0 and np.all(np.diff(r) > 0)
        assert np.array_equal(r, -r[::-1])                                   # odd about the middle, bit for bit
        assert np.abs(r.astype(np.float64) - nj.ramp64(L)).max() <= 2.0 ** -24
    assert np.array_equal(nj.ramp(1), np.zeros(1, dtype=np.float32)) and np.array_equal(nj.ramp64(1), np.zeros(1))
    assert nj.ramp(3)[1] == 0.0


def test_each_value_zero_leaves_its_stage_out_up_to_the_sign_of_a_zero():
    x = _rows(6, 9)
    x[2, 3] = -0.0
    only_gain, only_tilt, none = nj.stage32(x, 9, 2, 0.3, 0.0), nj.stage32(x, 9, 2, 0.0, 0.7), nj.stage32(x, 9, 2, 0.0, 0.0)
    assert np.all(nj.gains(6, 9, 2, 0.0) == 1.0) and np.all(nj.tilts(6, 9, 2, 0.0) == 0.0)
    assert np.array_equal(none, x)                                           # (== : -0.0 equals +0.0)
    assert np.array_equal(only_gain, (x * nj.gains(6, 9, 2, 0.3)[:, None]).astype(np.float32))
    assert np.array_equal(only_tilt, (x + (nj.tilts(6, 9, 2, 0.7)[:, None] * nj.ramp(9)[None, :]).astype(np.float32)).astype(np.float32))
    assert not np.array_equal(only_gain, x) and not np.array_equal(only_tilt, x)


# ------------------------------------------------------------------------------------------------ the draws
@pytest.mark.parametrize("a,t", [(0.03, 0.02), (0.5, 1.0), (0.999, 250.0)])
def test_draws_stay_inside_their_intervals_and_rows_differ(a, t):
    B = 4096
    g, c = nj.gains(B, 711, 3, a), nj.tilts(B, 711, 3, t)
    assert g.dtype == np.float32 and c.dtype == np.float32
    lo, hi = np.float32(1.0) - np.float32(a), np.float32(1.0) + np.float32(a)
    assert np.all(g >= lo) and np.all(g < hi)
    assert np.all(np.abs(c) <= np.float32(t))
    g64, c64 = nj.gains64(B, 711, 3, a), nj.tilts64(B, 711, 3, t)
    a32, t32 = float(np.float32(a)), float(np.float32(t))
    assert np.all(g64 >= 1.0 - a32) and np.all(g64 < 1.0 + a32) and np.all(c64 >= -t32) and np.all(c64 < t32)
    assert len(np.unique(g64)) > 4000 and len(np.unique(c)) > 4000
    assert g64.min() < 1.0 - 0.95 * a32 and g64.max() > 1.0 + 0.95 * a32 and abs(float(g64.mean()) - 1.0) < 0.03 * a32
    assert c.min() < -0.95 * t32 and c.max() > 0.95 * t32 and abs(float(c.mean())) < 0.03 * t32


def test_the_four_streams_of_a_row_are_pairwise_different():
    """The gain, tilt, shift and broaden hashes of the same 4096 rows: no two of the streams agree on more than a
    handful of rows, none is correlated with another, and the four index ranges do not meet for any row count the
    entry point admits (nor reach the dropout elements below 2^31, nor wrap past 2^32)."""
    B = 4096
    u = {"gain": nj.uniforms(B, 711, 3, nj.GAIN_OFF), "tilt": nj.uniforms(B, 711, 3, nj.TILT_OFF),
         "shift": ar.uniforms(B, 711, 3), "broaden": br.unit_draws(B, 711, 3)}
    h = {"gain": nj.hashes(B, 711, 3, nj.GAIN_OFF), "tilt": nj.hashes(B, 711, 3, nj.TILT_OFF),
         "shift": nj.hashes(B, 711, 3, ar.OFF), "broaden": nj.hashes(B, 711, 3, br.OFF)}
    assert np.array_equal(h["shift"] >> np.uint32(8), (u["shift"] * 2.0 ** 24).astype(np.uint32))
    assert np.array_equal(h["broaden"] >> np.uint32(8), (u["broaden"] * 2.0 ** 24).astype(np.uint32))
    names = list(u)
    for i, p in enumerate(names):
        for q in names[i + 1:]:
            assert np.mean(h[p] == h[q]) < 0.01, (p, q)
            assert abs(float(np.corrcoef(u[p], u[q])[0, 1])) < 0.05, (p, q)
    ranges = sorted((off, off + nj.BMAX - 1) for off in (ar.OFF, nj.GAIN_OFF, br.OFF, nj.TILT_OFF))
    assert ranges[0][0] >= 2 ** 31 and ranges[-1][1] <= 2 ** 32 - 1
    for (_, end), (start, _) in zip(ranges, ranges[1:]):
        assert end < start


def test_draws_change_with_the_counter_and_the_seed_and_depend_on_the_row_alone():
    for f, m in ((nj.gains, 0.3), (nj.tilts, 0.7)):
        a, b, c = f(64, 711, 3, m), f(64, 711, 4, m), f(64, 712, 3, m)
        assert np.mean(a == b) < 0.1 and np.mean(a == c) < 0.1 and np.mean(b == c) < 0.1
        assert np.array_equal(a, f(64, 711, 3, m)) and np.array_equal(a[:16], f(16, 711, 3, m))


# ------------------------------------------------------------------------------------------------ resume, TrialBatch
def test_resume_fingerprint_carries_each_key_only_when_set():
    spec = np.ones((4, 8), dtype=np.float32)
    fp = lambda cfg: resume.fingerprint(cfg, 1, 640, 4, 2, spec)       # noqa: E731
    base = {"ae_form": "FC", "nstyle": 2}
    for key, other in (("spec_gain", "spec_tilt"), ("spec_tilt", "spec_gain")):
        assert "cfg." + key not in fp(base) and fp(base) == fp(dict(base, **{key: None}))
        one = fp(dict(base, **{key: 0.25}))
        assert one["cfg." + key] == 0.25 and isinstance(one["cfg." + key], float) and "cfg." + other not in one
        assert {k: v for k, v in one.items() if k != "cfg." + key} == fp(base)
        with pytest.raises(ValueError, match="cfg." + key):
            resume.check_fingerprint(one, fp(dict(base, **{key: 0.5})))
        with pytest.raises(ValueError, match="cfg." + key):
            resume.check_fingerprint(fp(base), one)
        with pytest.raises(ValueError, match="cfg." + key):
            resume.check_fingerprint(one, fp(base))
    both = fp(dict(base, spec_gain=0.05, spec_tilt=0.02))
    assert both["cfg.spec_gain"] == 0.05 and both["cfg.spec_tilt"] == 0.02


def test_trial_batch_wants_its_engines_to_agree_on_whether_each_key_is_set():
    from rankaae_amd.trial_batch import TrialBatch
    stream = object()

    def engine(gain=None, tilt=None):
        return types.SimpleNamespace(rng_mode="philox", world_size=1, bf16=False, tile_mult=1, stream=stream,
                                     aux_missing=False, grad_clip=None, ema_decay=None, spec_shift=None,
                                     spec_broaden=None, spec_gain=gain, spec_tilt=tilt, rank_metrics=False,
                                     style_decorr=None, rank_loss_form="linear", rank_temperature=None, cfg={})
    with pytest.raises(ValueError, match="the engines of a TrialBatch must agree on whether spec_gain is set"):
        TrialBatch([engine(gain=0.05), engine()])
    with pytest.raises(ValueError, match="the engines of a TrialBatch must agree on whether spec_gain is set"):
        TrialBatch([engine(tilt=0.1), engine(gain=0.05, tilt=0.1)])
    with pytest.raises(ValueError, match="the engines of a TrialBatch must agree on whether spec_tilt is set"):
        TrialBatch([engine(gain=0.05), engine(gain=0.05, tilt=0.1)])
    with pytest.raises(ValueError, match="the engines of a TrialBatch must agree on whether spec_tilt is set"):
        TrialBatch([engine(tilt=0.1), engine()])
    assert TrialBatch([engine(gain=0.05, tilt=0.1), engine(gain=0.5, tilt=2.0)]).T == 2      # the values may differ
    assert TrialBatch([engine(gain=0.05), engine(gain=0.5)]).T == 2
    assert TrialBatch([engine(), engine()]).T == 2
