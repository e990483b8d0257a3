"""The arithmetic of ``raae_resample_rows`` and ``raae_ensemble_stats`` (``rankaae_amd/csrc/raae_apply.hip``) restated in
numpy float64: what ``tests/test_apply_cpu.py`` checks against ``np.interp`` / ``np.mean`` / ``np.std`` and what
``tests/test_apply_gpu.py`` holds the kernels to.  No torch on these lines."""
import numpy as np


def resample(rows, idx, w):
    """``a + w (b - a)`` in float64 on the rows as given (fp32 rows are promoted exactly), ``w`` the plan's fp32
    weights: the value the kernel approximates with one fp32 subtraction and one fp32 fmaf.  ``w == 0`` is ``a`` and
    ``w == 1`` is ``b`` themselves, as in the kernel (``a + 1 (b - a)`` rounds)."""
    rows = np.asarray(rows, dtype=np.float64)
    idx = np.asarray(idx, dtype=np.int64)
    w = np.asarray(w, dtype=np.float64)[None, :]
    a, b = rows[:, idx], rows[:, idx + 1]
    return np.where(w == 0.0, a, np.where(w == 1.0, b, a + w * (b - a)))


def predict(calib_row, z):
    """The descriptor a calibration row ``{kind, p0, p1, 0}`` reads off the styles ``z`` (float64); kind 0 has none."""
    kind, p0, p1 = calib_row[0], calib_row[1], calib_row[2]
    z = np.asarray(z, dtype=np.float64)
    if kind == 1.0:
        return (z - p1) / p0
    if kind == 2.0:
        return 4.0 + (z > p0).astype(np.float64) + (z > p1).astype(np.float64)
    raise ValueError("kind 0 predicts nothing")


def _mean_std(values):
    """Two-pass mean and sample standard deviation over axis 0, summed in order; exactly 0 for one value."""
    values = np.asarray(values, dtype=np.float64)
    m = values.shape[0]
    s = np.zeros(values.shape[1:], dtype=np.float64)
    for v in values:
        s = s + v
    mean = s / m
    q = np.zeros_like(s)
    for v in values:
        q = q + (v - mean) * (v - mean)
    return mean, (np.sqrt(q / (m - 1)) if m > 1 else np.zeros_like(s))


def ensemble_stats(z, spec, recon, calib):
    """``z [J, n, k]``, ``spec [n, L]`` and ``recon [J, n, L]`` fp32, ``calib [J, n_aux, 4]`` float64 -> dict of
    float64 arrays named as ``apply_models`` names them.  The error is ``mean_l |recon - spec|`` with the difference
    in fp32 (exactly what the fp32 arrays give) and the sum in float64."""
    z, spec, recon = np.asarray(z, dtype=np.float32), np.asarray(spec, dtype=np.float32), np.asarray(recon, dtype=np.float32)
    calib = np.asarray(calib, dtype=np.float64)
    J, n, k = z.shape
    n_aux = calib.shape[1]
    z_mean, z_std = _mean_std(z.astype(np.float64))
    mae = np.abs(recon - spec[None]).astype(np.float64).sum(axis=2) / spec.shape[1]
    d_mean, d_std = np.full((n, n_aux), np.nan), np.full((n, n_aux), np.nan)
    d_used = np.zeros(n_aux)
    for i in range(min(k, n_aux)):
        d = [predict(calib[j, i], z[j, :, i]) for j in range(J) if calib[j, i, 0] != 0.0]
        d_used[i] = len(d)
        if d:
            d_mean[:, i], d_std[:, i] = _mean_std(np.stack(d))
    return dict(z_mean=z_mean, z_std=z_std, d_mean=d_mean, d_std=d_std, d_used=d_used, mae=mae,
                mae_mean=_mean_std(mae)[0])


def stats_inputs(seed, J, n, k, n_aux, L, kinds="mixed"):
    """Inputs of the statistics tests (the GPU tests use them, too): fp32 styles ``level * f_j`` with the models'
    factors at least 0.06 apart (``f_j = 1 + 0.1 j`` and a jitter of 0.02), so that every column's standard deviation
    is above 1e-2 of its mean's magnitude; calibration rows of every kind (``kinds="mixed"``: model j has no fit for
    descriptor (j + 2) % n_aux; descriptor 1 is the class kind), or with descriptor ``kinds`` (an int) kind 0 in every
    model.  The linear rows' slopes alternate in sign over the models and their intercepts lie at least 2 away from any
    style, so the predicted descriptors are of magnitude >= 1 with both signs among them: a spread of their own size."""
    rng = np.random.default_rng(seed)
    level = rng.uniform(0.5, 2.0, (1, n, k)) * rng.choice([-1.0, 1.0], (1, n, k))
    factor = 1.0 + 0.1 * np.arange(J)[:, None, None] + rng.uniform(-0.02, 0.02, (J, n, k))
    z = (level * factor).astype(np.float32)
    spec = rng.uniform(0.0, 1.5, (n, L)).astype(np.float32)
    recon = (spec[None] + rng.normal(0.0, 0.05, (J, n, L))).astype(np.float32)
    calib = np.zeros((J, n_aux, 4))
    for j in range(J):
        for i in range(n_aux):
            if i == 1:
                calib[j, i] = [2.0, rng.uniform(-1.2, -0.6), rng.uniform(0.6, 1.2), 0.0]
            else:
                calib[j, i] = [1.0, rng.uniform(0.5, 2.0) * (-1.0) ** (i + j), rng.uniform(5.0, 8.0), 0.0]
            if (kinds == "mixed" and J > 1 and (j + 2) % n_aux == i) or kinds == i:
                calib[j, i] = 0.0
    return z, spec, recon, calib
