"""Reference of the normalisation augmentation (config keys ``spec_gain``, ``spec_tilt``; ``raae_spec_augment3``;
DESIGN.md section 2, "Normalisation augmentation").

Two forms of the one stage ``v = g_b x + c_b r_l``:

* ``stage32``: the kernel's own arithmetic in ``np.uint32`` / ``np.float32``, rounding for rounding -- the hash, the
  24-bit uniforms, ``(2 u - 1) a`` (one rounding), ``1 + ...`` (one), ``(2 u' - 1) t`` (one), the integer
  ``2 l - (L - 1)`` (exact), its division by ``float(L - 1)`` (one), ``g x`` (one), ``c r`` (one) and the sum (one).
  numpy's fp32 operations are IEEE and round once each, like the device's with contraction off: the result is the
  kernel's, bit for bit.
* ``stage64``: the same stage in float64 from the exact 24-bit uniforms, no fp32 rounding anywhere."""
import numpy as np

from augment_reference import row_hashes as hashes, row_uniforms as uniforms      # (at index range ``off``)

GAIN_OFF = 0xA0000000       # hash index of row 0's gain draw
TILT_OFF = 0xE0000000       # hash index of row 0's tilt draw
BMAX = 2 ** 29              # the most rows the entry point takes
U = 2.0 ** -24              # unit roundoff of fp32
_F = np.float32


def _signed(n_rows, seed, counter, off):
    return _F(2.0) * uniforms(n_rows, seed, counter, off) - _F(1.0)          # exact: a multiple of 2^-23 in [-1, 1)


def gains(n_rows, seed, counter, a):
    """``g_b = 1 + (2 u_b - 1) a`` in fp32: the product rounds, the sum rounds."""
    d = (_signed(n_rows, seed, counter, GAIN_OFF) * _F(a)).astype(_F)
    return (_F(1.0) + d).astype(_F)


def tilts(n_rows, seed, counter, t):
    """``c_b = (2 u'_b - 1) t`` in fp32: the product is the only rounding."""
    return (_signed(n_rows, seed, counter, TILT_OFF) * _F(t)).astype(_F)


def ramp(L):
    """``r_l = float(2 l - (L - 1)) / float(L - 1)`` in fp32 (the integer is exact, the division rounds); ``L == 1``: 0."""
    if L == 1:
        return np.zeros(1, dtype=_F)
    return ((2 * np.arange(L, dtype=np.int64) - (L - 1)).astype(_F) / _F(L - 1)).astype(_F)


def apply32(x, g, c):
    """``fl(fl(g_b x) + fl(c_b r_l))`` on fp32 rows ``x`` [B][L] with the fp32 per-row ``g``, ``c``."""
    x = np.asarray(x)
    assert x.dtype == np.float32 and x.ndim == 2
    with np.errstate(invalid="ignore", over="ignore"):
        v = (x * np.asarray(g, dtype=_F)[:, None]).astype(_F)
        p = (np.asarray(c, dtype=_F)[:, None] * ramp(x.shape[1])[None, :]).astype(_F)
        return (v + p).astype(_F)


def stage32(x, seed, counter, a, t):
    """The kernel's gain and tilt stage on the fp32 rows ``x`` (what its shift stage hands on), bit for bit."""
    B = np.asarray(x).shape[0]
    return apply32(x, gains(B, seed, counter, a), tilts(B, seed, counter, t))


def gains64(n_rows, seed, counter, a):
    """``1 + (2 u_b - 1) a`` in float64, from the exact uniforms and ``a`` as the kernel sees it (rounded to fp32)."""
    return 1.0 + (2.0 * uniforms(n_rows, seed, counter, GAIN_OFF).astype(np.float64) - 1.0) * float(_F(a))


def tilts64(n_rows, seed, counter, t):
    return (2.0 * uniforms(n_rows, seed, counter, TILT_OFF).astype(np.float64) - 1.0) * float(_F(t))


def ramp64(L):
    if L == 1:
        return np.zeros(1)
    return (2.0 * np.arange(L) - (L - 1)) / (L - 1)


def stage64(x, seed, counter, a, t):
    """``g_b x + c_b r_l`` in float64."""
    x = np.asarray(x, dtype=np.float64)
    B, L = x.shape
    return gains64(B, seed, counter, a)[:, None] * x + tilts64(B, seed, counter, t)[:, None] * ramp64(L)[None, :]


def stage_bound(x, seed, counter, a, t):
    """What ``stage32`` may differ from ``stage64`` by, per element, one fp32 spacing (``2 u`` relative, at most) for
    each of the listed roundings, propagated to first order (second-order terms: the factor ``1 + 1e-5``):

    * ``g``: the product ``(2 u - 1) a`` (at most ``2u |d|``, ``|d| <= a``) and the sum (``2u |g|``), both times ``|x|``;
    * ``g x``: ``2u |g x|``;
    * ``c``, ``r`` and ``c r``: three roundings of the tilt term, ``3 * 2u |c r|``;
    * the sum: ``2u |v|``."""
    x = np.abs(np.asarray(x, dtype=np.float64))
    B, L = x.shape
    g, c, r = np.abs(gains64(B, seed, counter, a))[:, None], np.abs(tilts64(B, seed, counter, t))[:, None], np.abs(ramp64(L))[None, :]
    sp = 2.0 * U
    return (1.0 + 1e-5) * (sp * (float(_F(a)) + g) * x + sp * g * x + 3.0 * sp * c * r + sp * (g * x + c * r)) + 2.0 ** -126
