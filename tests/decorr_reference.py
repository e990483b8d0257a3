"""numpy float64 reference of the style decorrelation penalty (config key ``style_decorr``, ``raae_style_decorr_fwd_bwd``).

For styles ``z [b, k]``: ``x_i`` column ``i`` minus its mean, ``s_i = |x_i|``, ``u_i = x_i / s_i``, ``C_ij = u_i . u_j``,

    D(z) = 1 / (k (k - 1)) * sum_{i != j} C_ij^2

    dD/dz[r, i] = 4 / (k (k - 1) s_i) * sum_{j != i} C_ij (u[r, j] - C_ij u[r, i])

A column whose centred sum of squares is exactly zero has ``C_i. = 0``: it adds nothing to ``D`` and has no gradient.
``b == 1`` or ``k == 1``: ``D = 0``, no gradient.  ``penalty`` and ``gradient`` are written independently of each other --
the first from the definition, the second from the closed form -- and ``test_style_decorr_cpu.py`` holds the second
against central finite differences of the first."""
import numpy as np


def _unit_columns(z):
    """``(u [b, k], s [k])``: the centred columns scaled to unit length (zero for a column without variance)."""
    z = np.asarray(z, dtype=np.float64)
    x = z - z.mean(axis=0, keepdims=True)
    s = np.sqrt((x * x).sum(axis=0))
    u = np.divide(x, s, out=np.zeros_like(x), where=s > 0.0)
    return u, s


def correlation(z):
    """``C [k, k]``; rows and columns of a column without variance are zero (the diagonal included)."""
    u, _ = _unit_columns(z)
    return u.T @ u


def penalty(z):
    """``D(z)`` as a Python float."""
    z = np.asarray(z, dtype=np.float64)
    b, k = z.shape
    if b == 1 or k == 1:
        return 0.0
    c = correlation(z)
    off = c - np.diag(np.diag(c))
    return float((off * off).sum() / (k * (k - 1)))


def gradient(z):
    """``dD/dz [b, k]`` (float64), exact through the centring and the normalisation."""
    z = np.asarray(z, dtype=np.float64)
    b, k = z.shape
    g = np.zeros((b, k))
    if b == 1 or k == 1:
        return g
    u, s = _unit_columns(z)
    c = u.T @ u
    for i in range(k):
        if not s[i] > 0.0:
            continue
        acc = np.zeros(b)
        for j in range(k):
            if j != i:
                acc += c[i, j] * (u[:, j] - c[i, j] * u[:, i])
        g[:, i] = 4.0 / (k * (k - 1) * s[i]) * acc
    return g


def mixed_gaussian(b, k, seed):
    """Test styles ``[b, k]`` (float32): Gaussian columns mixed by a random matrix (so that ``C`` has entries of every
    size), each column then given its own scale and a mean of at most ten of its standard deviations."""
    rng = np.random.default_rng(seed)
    y = rng.standard_normal((b, k)) @ (rng.standard_normal((k, k)) * rng.uniform(0.05, 1.0, size=(1, k)) + np.eye(k))
    sd = y.std(axis=0)
    sd = np.where(sd > 0.0, sd, 1.0)
    y = y / sd * rng.uniform(0.1, 3.0, size=k)
    col_sd = np.where(y.std(axis=0) > 0.0, y.std(axis=0), 1.0)
    y = y - y.mean(axis=0) + rng.uniform(-9.0, 9.0, size=k) * col_sd
    return np.ascontiguousarray(y, dtype=np.float32)
