"""The numpy reference of ``raae_kendall_tau`` (tests/kendall_reference.py) against ``scipy.stats.kendalltau(x, y,
variant="b")`` on the labelled rows, |dtau| <= 1e-12 -- the bound of the project's other scipy-pinned metrics; the two
differ by a handful of double roundings -- and the ``rank_metrics`` key's validation.  No GPU."""
import numpy as np
import pytest
from scipy import stats

import kendall_reference as kr
from rankaae_amd.parameter import rank_metrics_on


@pytest.mark.parametrize("n", [2, 7, 200])
@pytest.mark.parametrize("kind", kr.KINDS)
def test_reference_matches_scipy(kind, n):
    d, z = kr.make_column(kind, n, seed=3)
    counts = kr.kendall_counts(d, z)
    tau = kr.tau_from_counts(counts)
    keep = np.isfinite(d)
    m = int(keep.sum())
    assert counts[kr.M] == m and counts[:5].sum() == m * (m - 1) // 2
    want = stats.kendalltau(d[keep], z[keep], variant="b").statistic
    if kind in ("one_labelled", "constant"):
        assert np.isnan(want) and np.isnan(tau)
    elif np.isnan(want):
        assert np.isnan(tau)
    else:
        assert abs(tau - want) <= 1e-12, (tau, want)
    if kind == "ulp_1e-38" and n > 2:
        assert counts[kr.TX] == counts[kr.TY] == counts[kr.TXY] == 0        # ordered, never tied
    if kind == "signed_zeros" and n == 200:
        assert counts[kr.TXY] > 0 and counts[kr.TX] > 0 and counts[kr.TY] > 0


def test_scipy_returns_nan_for_a_constant_column():
    assert np.isnan(stats.kendalltau(np.ones(5), np.arange(5.), variant="b").statistic)
    tau, counts = kr.kendall_reference(np.ones((5, 1)), np.arange(5.).reshape(5, 1), 1)
    assert np.isnan(tau[0]) and counts[0].tolist() == [0, 0, 10, 0, 0, 5]


def test_hand_counted_pairs():
    d = np.array([1, 2, 2, 3, np.nan, 3], dtype=np.float32)
    z = np.array([1, 3, 3, 2, 9, 2], dtype=np.float32)
    # labelled rows (1,1) (2,3) (2,3) (3,2) (3,2): 10 pairs; Txy: the two doubles; C: row 0 with the other four;
    # D: the (2,3) rows against the (3,2) rows
    tau, counts = kr.kendall_reference(d[:, None], z[:, None], 1)
    assert counts[0].tolist() == [4, 4, 0, 0, 2, 5]
    assert tau[0] == 0.0


def test_matrix_leaves_padding_columns_unread():
    d, z = kr.make_matrix(40, 5, seed=1, ldd=7, ldz=6)
    assert np.isnan(d[:, 5:]).all() and np.isnan(z[:, 5:]).all()
    tau, counts = kr.kendall_reference(d, z, 5)
    d2, z2 = kr.make_matrix(40, 5, seed=1)
    tau2, counts2 = kr.kendall_reference(d2, z2, 5)
    kr.assert_matches(tau, counts, tau2, counts2, tol=0.0)


@pytest.mark.parametrize("value", [True, False])
def test_rank_metrics_accepts_bools(value):
    assert rank_metrics_on({"rank_metrics": value}) is value


def test_rank_metrics_defaults_to_off():
    assert rank_metrics_on({}) is False


@pytest.mark.parametrize("value", ["true", "false", 1, 0, 1.0, None, "yes", [True]])
def test_rank_metrics_refuses_everything_else(value):
    with pytest.raises(ValueError, match="rank_metrics"):
        rank_metrics_on({"rank_metrics": value})
