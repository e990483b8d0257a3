"""Brute-force numpy reference for ``raae_kendall_tau`` (config key ``rank_metrics``), and the data its tests share.

Per descriptor ``k``, over the unordered pairs ``i < j`` of the rows labelled for ``k`` (a finite descriptor cell), the
six int64 counts ``C, D, Tx, Ty, Txy, m`` -- concordant, discordant, tied in the descriptor only, tied in the style
only, tied in both, labelled rows -- by comparing the stored float32 values (``<``, ``>``, ``==``; no differences, no
products), and tau-b from them in float64 in scipy's order of operations::

    tot = m (m - 1) / 2
    tau = (C - D) / sqrt(tot - (Tx + Txy)) / sqrt(tot - (Ty + Txy))        # NaN: m < 2, or a factor is zero

``tests/test_kendall_reference_cpu.py`` pins this to ``scipy.stats.kendalltau(x, y, variant="b")``.
"""
import numpy as np

C, D, TX, TY, TXY, M = range(6)


def kendall_counts(x, y):
    """The six counts of one descriptor column ``x`` against one style column ``y`` (float32 as stored)."""
    x, y = np.asarray(x, dtype=np.float32), np.asarray(y, dtype=np.float32)
    keep = np.isfinite(x)
    x, y = x[keep], y[keep]
    # the whole m x m table of ordered pairs (i, j), the diagonal struck out: every unordered pair stands in it twice,
    # once each way round, and each of the five classes is symmetric, so every count is an even number halved
    xl, xg, xe = x[:, None] < x[None, :], x[:, None] > x[None, :], x[:, None] == x[None, :]
    yl, yg, ye = y[:, None] < y[None, :], y[:, None] > y[None, :], y[:, None] == y[None, :]
    np.fill_diagonal(xe, False)
    np.fill_diagonal(ye, False)
    twice = np.array([np.count_nonzero((xl & yl) | (xg & yg)), np.count_nonzero((xl & yg) | (xg & yl)),
                      np.count_nonzero(xe & (yl | yg)), np.count_nonzero(ye & (xl | xg)), np.count_nonzero(xe & ye)],
                     dtype=np.int64)
    assert not (twice & 1).any()
    out = np.zeros(6, dtype=np.int64)
    out[:5] = twice // 2
    out[M] = len(x)
    return out


def tau_from_counts(c):
    c = [int(v) for v in c]
    m = c[M]
    tot = m * (m - 1) // 2
    fx, fy = tot - (c[TX] + c[TXY]), tot - (c[TY] + c[TXY])
    if m < 2 or fx == 0 or fy == 0:
        return np.float64(np.nan)
    return np.float64(c[C] - c[D]) / np.sqrt(np.float64(fx)) / np.sqrt(np.float64(fy))


def kendall_reference(d, z, n_aux):
    """``(tau float64[n_aux], counts int64[n_aux, 6])`` of columns ``k < n_aux`` of ``d`` and ``z``."""
    d, z = np.asarray(d, dtype=np.float32), np.asarray(z, dtype=np.float32)
    counts = np.stack([kendall_counts(d[:, k], z[:, k]) for k in range(n_aux)])
    return np.array([tau_from_counts(c) for c in counts], dtype=np.float64), counts


def assert_matches(tau, counts, want_tau, want_counts, tol=1e-12, what=""):
    """Counts exactly; tau within ``tol``, NaN exactly where the reference is NaN."""
    assert counts.dtype == np.int64 and tau.dtype == np.float64
    assert np.array_equal(counts, want_counts), f"{what}: counts\n{counts}\nwant\n{want_counts}"
    nan = np.isnan(want_tau)
    assert np.array_equal(np.isnan(tau), nan), f"{what}: tau {tau}, want {want_tau}"
    err = np.abs(tau[~nan] - want_tau[~nan])
    assert (err <= tol).all(), f"{what}: tau {tau}, want {want_tau}, |diff| {err}"


# ---- data: one (descriptor, style) column pair per kind -----------------------------------------------------------------
KINDS = ("continuous", "integer_ties", "style_duplicates", "both_ties", "nan30", "one_labelled", "constant",
         "ulp_1e-38", "signed_zeros")


def _ulp_column(n, rng):
    """Float32 neighbours one ulp apart around 1e-38 (subnormal: the smallest normal is 1.18e-38), shuffled."""
    base = int(np.float32(1e-38).view(np.uint32))
    bits = (base + np.arange(n, dtype=np.int64)).astype(np.uint32)
    return rng.permutation(bits).view(np.float32)


def make_column(kind, n, seed):
    """``(d, z)``: float32 ``[n]`` each."""
    rng = np.random.default_rng([seed, KINDS.index(kind), n])
    t = rng.normal(size=n)
    d = t.astype(np.float32)
    z = (0.6 * t + 0.8 * rng.normal(size=n)).astype(np.float32)
    if kind == "integer_ties":              # coordination numbers: a few classes
        d = rng.integers(0, 4, size=n).astype(np.float32)
        z = (d + rng.normal(size=n)).astype(np.float32)
    elif kind == "style_duplicates":
        z = np.round(z, 1).astype(np.float32)
    elif kind == "both_ties":
        d = rng.integers(0, 3, size=n).astype(np.float32)
        z = np.round(d - 1 + 0.7 * rng.normal(size=n)).astype(np.float32)
    elif kind == "nan30":
        d[rng.random(n) < 0.3] = np.nan
    elif kind == "one_labelled":
        keep = int(rng.integers(0, n))
        d[np.arange(n) != keep] = np.nan
    elif kind == "constant":
        d[:] = np.float32(2.5)
    elif kind == "ulp_1e-38":
        d, z = _ulp_column(n, rng), _ulp_column(n, rng)
    elif kind == "signed_zeros":            # runs of +0.0 and -0.0 (ties) among a few other values
        d = rng.choice(np.array([0.0, -0.0, 1.0, -1.0], dtype=np.float32), size=n)
        z = rng.choice(np.array([0.0, -0.0, 0.5], dtype=np.float32), size=n)
    return d, z


def make_matrix(n, n_aux, seed, ldd=None, ldz=None, shift=0):
    """``d [n, ldd]``, ``z [n, ldz]`` float32: column ``k < n_aux`` is of kind ``KINDS[(k + shift) % 9]``; the columns
    behind ``n_aux`` hold NaN -- they are not data and must never be read as such."""
    ldd, ldz = ldd or n_aux, ldz or n_aux
    d = np.full((n, ldd), np.nan, dtype=np.float32)
    z = np.full((n, ldz), np.nan, dtype=np.float32)
    for k in range(n_aux):
        d[:, k], z[:, k] = make_column(KINDS[(k + shift) % len(KINDS)], n, seed + k)
    return d, z
