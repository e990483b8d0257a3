"""Float64 reference of the resolution augmentation (config key ``spec_broaden``, ``raae_spec_augment2``; DESIGN.md
section 2, "Resolution augmentation").

The draw is followed rounding for rounding in ``np.uint32`` / ``np.float32`` arithmetic (``g_b``, ``v_b``, and
``sigma_b = v_b * s``, one fp32 product), so ``sigma_b`` is exact.  The convolution itself is float64, from that exact
fp32 ``sigma_b``: weights ``exp(-j^2 / (2 sigma^2))``, ``j = -R .. R``, normalised, replicated edges.  What the kernel
is compared against differs from it by the kernel's own fp32 roundings only (``error_bound``)."""
import numpy as np

import augment_reference as ar

OFF = 0xC0000000        # hash index of row 0's width draw: beyond every dropout element and every shift draw of a step
RMAX = 64
U = 2.0 ** -24          # unit roundoff of fp32


def radius(s):
    """``R = ceil(3 s)`` as the kernel computes it: ``s`` in fp32, the fp32 product, then the ceiling."""
    return int(np.ceil(np.float32(3.0) * np.float32(s)))


def unit_draws(n_rows, seed, counter):
    """``v_b`` of rows ``0 .. n_rows - 1``, fp32, in ``[0, 1)`` (24 bits: exact)."""
    return ar.row_uniforms(n_rows, seed, counter, OFF)


def sigmas(n_rows, seed, counter, s):
    """``sigma_b = v_b * s`` in fp32: the product is the only rounding."""
    return (unit_draws(n_rows, seed, counter) * np.float32(s)).astype(np.float32)


def weights(sigma, R):
    """The ``2 R + 1`` unnormalised float64 weights of one row (``sigma > 0``, the exact fp32 value), ``w_0 = 1``."""
    j = np.arange(-R, R + 1, dtype=np.float64)
    return np.exp(-(j * j) / (2.0 * float(sigma) * float(sigma)))


def taps(rows, R, pad="edge"):
    """``[B][L][2 R + 1]``: sample ``clamp(l + j, 0, L - 1)`` of every row (``pad="constant"``: zeros beyond the ends)."""
    rows = np.asarray(rows, dtype=np.float64)
    padded = np.pad(rows, ((0, 0), (R, R)), mode=pad)
    return np.lib.stride_tricks.sliding_window_view(padded, 2 * R + 1, axis=1)


def broaden_rows_by(rows, sigma, R, pad="edge"):
    """``rows`` [B][L], row b convolved with the normalised Gaussian of width ``sigma[b]`` truncated at ``R``;
    replicated edges; ``sigma == 0`` gives the row itself.  float64."""
    rows = np.asarray(rows, dtype=np.float64)
    sigma = np.asarray(sigma, dtype=np.float32)
    assert rows.ndim == 2 and sigma.shape == (rows.shape[0],) and R >= 0
    out = rows.copy()
    t = taps(rows, R, pad)
    for b in np.nonzero(sigma != 0)[0]:
        w = weights(sigma[b], R)
        out[b] = t[b] @ w / w.sum()
    return out


def augment(rows, seed, counter, s_broaden, s_shift):
    """The augmented batch without its noise term: row b broadened by its own ``sigma_b``, then shifted by its own
    ``delta_b`` (``s_shift = 0``: not shifted)."""
    rows = np.asarray(rows)
    g = broaden_rows_by(rows, sigmas(rows.shape[0], seed, counter, s_broaden), radius(s_broaden))
    return ar.shift_rows_by(g, ar.deltas(rows.shape[0], seed, counter, s_shift))


def error_bound(rows, sigma, R, delta):
    """What the kernel's fp32 arithmetic may differ from ``shift_rows_by(broaden_rows_by(rows, sigma, R), delta)`` by,
    per element, before the noise ("Resolution augmentation: the error bound").  With ``u = 2^-24``,
    ``n = 2 R + 1``, ``w_j`` the true weights, ``W`` their sum, ``x_j`` the taps of an output and ``t_j = j^2 / (2
    sigma^2)``:

    * the computed weight is ``w_j (1 + eta_j)``, ``|eta_j| <= 3 u t_j + 2 u`` for ``j != 0`` (three roundings in the
      argument, which enter as ``t_j w_j <= 1 / e``, and ``expf``'s 1 ulp = ``2 u``), 0 for ``j = 0``, plus ``2^-126``
      absolute where the weight leaves the normal range;
    * the fused sum of ``n`` terms: ``gamma_n sum |w_j x_j|``; the plain sum ``W``: ``gamma_(n-1) W``; the division: ``u``;
    * the shift: the errors of its two samples interpolate, and its difference, product and sum round once each:
      ``u (2 f |g1 - g0| + |out|)``.

    ``sigma == 0`` rows carry the shift's part only.  Second-order terms are below ``2 n u`` of the first-order ones
    and are covered by the factor ``1 + 1e-4``."""
    rows = np.asarray(rows, dtype=np.float64)
    B, L = rows.shape
    n = 2 * R + 1
    gam = lambda k: k * U / (1.0 - k * U)           # noqa: E731
    g = broaden_rows_by(rows, sigma, R)
    e = np.zeros_like(rows)
    t_abs = np.abs(taps(rows, R))
    j = np.arange(-R, R + 1, dtype=np.float64)
    for b in np.nonzero(np.asarray(sigma) != 0)[0]:
        w = weights(sigma[b], R)
        W = w.sum()
        tj = (j * j) / (2.0 * float(sigma[b]) ** 2)
        dw = np.where(j == 0, 0.0, (3.0 * U * tj + 2.0 * U) * w + 2.0 ** -126)       # |computed w_j - w_j|
        A = t_abs[b] @ w / W                        # sum w_j |x_j| / W
        e[b] = gam(n) * A + t_abs[b] @ dw / W + (gam(n - 1) + dw.sum() / W) * A + U * np.abs(g[b])
    i0, i1, f = ar.positions(delta, L)
    f = f.astype(np.float64)
    take = lambda a, i: np.take_along_axis(a, i, axis=1)        # noqa: E731
    g0, g1 = take(g, i0), take(g, i1)
    out = g0 + f * (g1 - g0)
    bound = (1.0 - f) * take(e, i0) + f * take(e, i1) + np.where(f == 0, 0.0, U * (2.0 * f * np.abs(g1 - g0) + np.abs(out)))
    return (1.0 + 1e-4) * bound
