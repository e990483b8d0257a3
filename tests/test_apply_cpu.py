"""Host side of ``rankaae_amd.apply``: the resampling plan against ``np.interp``, the calibration rows from hand-built
``raae_select_scores`` blocks, the three config keys, and the numpy reference of the ensemble statistics
(``tests/apply_reference.py``) against ``np.mean`` / ``np.std(ddof=1)``.  No GPU."""
import os

import numpy as np
import pytest

import apply_reference as ar
from rankaae_amd import _lib, apply
from rankaae_amd._lib import SEL_HEAD, SEL_STRIDE
from rankaae_amd.parameter import Parameters, apply_keys_of


def _grid(rng, n, lo, hi):
    g = np.sort(rng.uniform(lo, hi, n))
    assert np.all(np.diff(g) > 0)
    return g


# ------------------------------------------------------------------------------------------------ resample_plan
@pytest.mark.parametrize("seed,Ls,L", [(0, 2, 1), (1, 7, 64), (2, 257, 256), (3, 1000, 300)])
def test_plan_agrees_with_np_interp(seed, Ls, L):
    """One rounding of w to fp32 moves ``a + w (b - a)`` by at most ``2^-25 |b - a| <= 2^-24 max|row|``; the float64
    arithmetic on either side adds ~1e-16."""
    rng = np.random.default_rng(seed)
    src, dst = _grid(rng, Ls, 100.0, 200.0), _grid(rng, L, 90.0, 210.0)       # some points outside on either side
    idx, w, outside = apply.resample_plan(src, dst)
    assert idx.dtype == np.int32 and w.dtype == np.float32 and outside.dtype == np.bool_
    assert idx.shape == w.shape == outside.shape == (L,)
    assert idx.min() >= 0 and idx.max() <= Ls - 2 and w.min() >= 0.0 and w.max() <= 1.0
    assert np.array_equal(outside, (dst < src[0]) | (dst > src[-1]))
    rows = rng.standard_normal((3, Ls))
    want = np.stack([np.interp(dst, src, r) for r in rows])                   # (np.interp clamps outside points, too)
    got = ar.resample(rows, idx, w)
    assert np.max(np.abs(got - want)) <= 2.0 ** -24 * np.max(np.abs(rows)) + 1e-15
    # outside points: the edge value itself
    assert np.array_equal(got[:, dst < src[0]], np.repeat(rows[:, :1], int((dst < src[0]).sum()), axis=1))
    assert np.array_equal(got[:, dst > src[-1]], np.repeat(rows[:, -1:], int((dst > src[-1]).sum()), axis=1))


def test_plan_on_coinciding_points():
    src = np.array([1.0, 1.5, 2.25, 4.0, 4.125])
    idx, w, outside = apply.resample_plan(src, src)
    assert idx.tolist() == [0, 1, 2, 3, 3] and w.tolist() == [0.0, 0.0, 0.0, 0.0, 1.0] and not outside.any()
    idx, w, outside = apply.resample_plan(src, src[::2])
    assert idx.tolist() == [0, 2, 3] and w.tolist() == [0.0, 0.0, 1.0] and not outside.any()
    idx, w, outside = apply.resample_plan(src, np.array([0.5, 1.0, 3.125, 4.125, 5.0]))
    assert idx.tolist() == [0, 0, 2, 3, 3] and w.tolist() == [0.0, 0.0, 0.5, 1.0, 1.0]
    assert outside.tolist() == [True, False, False, False, True]


@pytest.mark.parametrize("src,dst", [
    ([1.0, 3.0, 2.0], [1.5]), ([1.0, 1.0, 2.0], [1.5]), ([1.0, 2.0], [2.0, 1.0]), ([1.0, 2.0], [1.0, 1.0]),
    ([1.0, np.nan, 2.0], [1.5]), ([1.0, np.inf], [1.5]), ([1.0, 2.0], [np.nan]), ([1.0], [1.0]), ([], [1.0]),
    ([1.0, 2.0], [])])
def test_plan_refuses_bad_grids(src, dst):
    with pytest.raises(ValueError):
        apply.resample_plan(np.array(src, dtype=np.float64), np.array(dst, dtype=np.float64))


# ------------------------------------------------------------------------------------------------ calibration
def _block(n_aux):
    b = np.zeros(SEL_HEAD + SEL_STRIDE * n_aux)
    for i in range(n_aux):
        o = b[SEL_HEAD + SEL_STRIDE * i:SEL_HEAD + SEL_STRIDE * (i + 1)]
        if i == 1:
            o[:6] = [1.0, 0.8, 300.0, 420.0, -0.49356223175965663, 0.7081545064377681]
        else:
            o[:4] = [0.9, 0.123456789 * (i + 1), -0.0987654321 * (i + 1), 0.7]
    return b


def test_calibration_kinds():
    b = _block(5)
    c = apply.calibration(b, 5)
    assert c.shape == (5, 4) and c.dtype == np.float64
    for i in (0, 2, 3, 4):
        assert c[i].tolist() == [1.0, 0.123456789 * (i + 1), -0.0987654321 * (i + 1), 0.0]     # unrounded
    assert c[1].tolist() == [2.0, -0.49356223175965663, 0.7081545064377681, 0.0]
    # fewer than 3 labelled rows: none, whatever the block holds
    c = apply.calibration(b, 5, labelled=np.array([100, 2, 3, 0, 100]))
    assert c[:, 0].tolist() == [1.0, 0.0, 1.0, 0.0, 1.0] and not c[1, 1:].any() and not c[3, 1:].any()
    # the coordination number's valid == 0 (more than three classes)
    b2 = b.copy()
    b2[SEL_HEAD + SEL_STRIDE] = 0.0
    assert apply.calibration(b2, 5)[1].tolist() == [0.0, 0.0, 0.0, 0.0]
    # a slope of 0 or NaN
    for bad in (0.0, np.nan):
        b3 = b.copy()
        b3[SEL_HEAD + SEL_STRIDE * 2 + 1] = bad
        c = apply.calibration(b3, 5)
        assert c[2].tolist() == [0.0, 0.0, 0.0, 0.0] and c[0, 0] == 1.0
    assert apply.calibration(b[:SEL_HEAD], 0).shape == (0, 4)


def test_calibration_is_none_where_the_report_is():
    from rankaae_amd import report
    b = _block(5)
    b[SEL_HEAD + SEL_STRIDE] = 0.0
    labelled = np.array([5, 5, 2, 5, 5])
    res = report.result_from_block(b, 5, labelled)["Style-descriptor Corr"]
    c = apply.calibration(b, 5, labelled)
    assert [res[i] is None for i in range(5)] == [c[i, 0] == 0.0 for i in range(5)] == [False, True, True, False, False]


# ------------------------------------------------------------------------------------------------ config keys
def test_apply_keys():
    assert apply_keys_of(Parameters({"top_n": 5})) == (5, 0, 16384)
    assert apply_keys_of({"top_n": 5, "apply_top_n": 2, "apply_max_outside": 3, "apply_chunk_rows": 1}) == (2, 3, 1)
    assert apply_keys_of({"apply_top_n": 1}) == (1, 0, 16384)
    for bad in ({"top_n": 5, "apply_top_n": 0}, {"top_n": 5, "apply_top_n": 1.0}, {"top_n": 5, "apply_top_n": True},
                {"top_n": 5, "apply_top_n": "2"}, {"top_n": 5, "apply_max_outside": -1},
                {"top_n": 5, "apply_max_outside": 0.5}, {"top_n": 5, "apply_chunk_rows": 0},
                {"top_n": 5, "apply_chunk_rows": False}, {"top_n": 0}, {}):
        with pytest.raises(ValueError):
            apply_keys_of(bad)


# ------------------------------------------------------------------------------------------------ the reference
def test_reference_statistics_written_out():
    z = np.array([[[1.0, 2.0]], [[3.0, 2.5]], [[8.0, 3.0]]], dtype=np.float32)            # J = 3, n = 1, k = 2
    spec = np.array([[1.0, 2.0, 3.0, 4.0]], dtype=np.float32)
    recon = np.stack([spec + 0.5, spec - 0.25, spec]).astype(np.float32)
    calib = np.array([[[1.0, 2.0, 1.0, 0.0], [2.0, 2.25, 2.75, 0.0], [0.0, 0.0, 0.0, 0.0]],
                      [[0.0, 0.0, 0.0, 0.0], [2.0, 2.25, 2.75, 0.0], [0.0, 0.0, 0.0, 0.0]],
                      [[1.0, -1.0, 0.0, 0.0], [2.0, 2.25, 2.75, 0.0], [0.0, 0.0, 0.0, 0.0]]])
    r = ar.ensemble_stats(z, spec, recon, calib)
    assert r["z_mean"].tolist() == [[4.0, 2.5]]
    assert np.allclose(r["z_std"], [[np.sqrt(13.0), 0.5]], rtol=1e-15)
    assert r["mae"].tolist() == [[0.5], [0.25], [0.0]] and r["mae_mean"].tolist() == [0.25]
    assert r["d_used"].tolist() == [2.0, 3.0, 0.0]
    # descriptor 0: (1 - 1) / 2 = 0 and (8 - 0) / -1 = -8; descriptor 1: classes 4, 5, 6; descriptor 2 has no style
    assert r["d_mean"][0, :2].tolist() == [-4.0, 5.0] and np.isnan(r["d_mean"][0, 2]) and np.isnan(r["d_std"][0, 2])
    assert np.allclose(r["d_std"][0, :2], [np.sqrt(32.0), 1.0], rtol=1e-15)
    one = ar.ensemble_stats(z[:1], spec, recon[:1], calib[:1])
    assert one["z_std"].tolist() == [[0.0, 0.0]] and one["d_std"][0, :2].tolist() == [0.0, 0.0]


@pytest.mark.parametrize("J,n_aux", [(2, 3), (5, 5), (5, 3)])
def test_reference_against_numpy_and_the_spread_of_the_inputs(J, n_aux):
    """The reference against ``np.mean`` / ``np.std(ddof=1)``, and the premise of the GPU test's ``rtol = 1e-10`` on the
    standard deviations: every column's spread over the models is at least 1e-3 of its mean's magnitude, under which a
    two-pass double computation stays below ``J 2^-53 1e3 ~ 1e-11`` relative."""
    z, spec, recon, calib = ar.stats_inputs(7, J, 67, 5, n_aux, 256)
    r = ar.ensemble_stats(z, spec, recon, calib)
    z64 = z.astype(np.float64)
    assert np.allclose(r["z_mean"], z64.mean(axis=0), rtol=1e-14, atol=0.0)
    assert np.allclose(r["z_std"], z64.std(axis=0, ddof=1), rtol=1e-11, atol=0.0)
    assert np.all(r["z_std"] >= 1e-3 * np.abs(r["z_mean"]))
    want_mae = np.abs(recon.astype(np.float64) - spec.astype(np.float64)[None]).mean(axis=2)
    assert np.allclose(r["mae"], want_mae, rtol=2.0 ** -20, atol=0.0)       # (the reference's difference is fp32)
    assert np.allclose(r["mae_mean"], r["mae"].mean(axis=0), rtol=1e-14, atol=0.0)
    for i in range(min(5, n_aux)):
        d = np.stack([ar.predict(calib[j, i], z64[j, :, i]) for j in range(J) if calib[j, i, 0] != 0.0])
        assert r["d_used"][i] == len(d) >= 1
        assert np.allclose(r["d_mean"][:, i], d.mean(axis=0), rtol=1e-14, atol=0.0)
        if len(d) > 1:
            sd = d.std(axis=0, ddof=1)
            assert np.allclose(r["d_std"][:, i], sd, rtol=1e-11, atol=0.0)
            if i != 1:      # (classes may agree between the models: their spread may be 0, which two passes give exactly)
                assert np.all(sd >= 1e-3 * np.abs(d.mean(axis=0)))
        else:
            assert not r["d_std"][:, i].any()


def test_symbols_are_bound_and_refuse_bad_shapes():
    """The two entry points validate on the host and return -1 without touching a GPU."""
    assert os.path.exists(_lib.LIB_PATH), "run rankaae_amd/csrc/build.sh (or __graft_entry__.build())"
    lib = _lib.load()
    assert _lib.ABI_VERSION == 34
    assert lib.raae_resample_rows(None, 1, 2, 2, None, None, 1, None, 1, None) == -1
    one = 8      # (any non-NULL address: nothing is launched)
    assert lib.raae_resample_rows(one, 1, 1, 1, one, one, 1, one, 1, None) == -1          # Ls < 2
    assert lib.raae_resample_rows(one, 1, 65537, 65537, one, one, 1, one, 1, None) == -1
    assert lib.raae_resample_rows(one, 1, 8, 8, one, one, 4097, one, 4097, None) == -1
    assert lib.raae_resample_rows(one, 1, 8, 7, one, one, 4, one, 4, None) == -1          # ld_src < Ls
    assert lib.raae_resample_rows(one, 0, 8, 8, one, one, 4, one, 4, None) == -1
    args = [one, one, one, one, 2, 3, 5, 3, 16, one, one, one, one, one, one, 3, one, None]
    for pos, bad in ((4, 0), (4, 65), (5, 0), (6, 0), (6, 17), (7, -1), (7, 17), (8, 0), (15, 2), (0, None), (3, None)):
        a = list(args)
        a[pos] = bad
        assert lib.raae_ensemble_stats(*a) == -1, (pos, bad)
