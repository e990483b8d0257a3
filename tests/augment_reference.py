"""Float64 reference of the energy-shift augmentation (config key ``spec_shift``, ``raae_spec_augment``; DESIGN.md
section 2, "Energy-shift augmentation").

The draw is followed rounding for rounding, in ``np.uint32`` / ``np.float32`` arithmetic: the step's hash keys
``k1, k2`` (``mask_gen_make`` of ``raae_common.h``), ``h_b``, ``u_b``, ``delta_b`` (one fp32 product), ``x`` (one fp32
sum, clamped), ``i0`` and ``f = x - i0`` (exact).  The interpolation itself is float64: what the kernel is compared
against differs from it by the kernel's three fp32 roundings only."""
import numpy as np

OFF = 0x80000000        # hash index of row 0's draw: beyond every dropout element of a step
_M32 = 0xFFFFFFFF


def lowbias32(x):
    """C. Wellons' hash on ``np.uint32`` (scalar or array), wrapping like the device's unsigned arithmetic."""
    x = np.asarray(x, dtype=np.uint32).copy()
    with np.errstate(over="ignore"):
        x ^= x >> np.uint32(16)
        x *= np.uint32(0x7feb352d)
        x ^= x >> np.uint32(15)
        x *= np.uint32(0x846ca68b)
        x ^= x >> np.uint32(16)
    return x


def step_keys(seed, counter):
    """``(k1, k2)`` as the step head stores them behind ``{counter, seed}``; ``counter`` is the ADVANCED counter."""
    seed, counter = int(seed) & 0xFFFFFFFFFFFFFFFF, int(counter) & 0xFFFFFFFFFFFFFFFF
    u32 = lambda v: np.uint32(v & _M32)       # noqa: E731
    with np.errstate(over="ignore"):
        k1 = lowbias32(u32(seed) ^ lowbias32(u32(counter) + np.uint32(0x9E3779B9)))
        k2 = lowbias32(u32(seed >> 32) + np.uint32(0x85EBCA6B) + lowbias32(u32(counter >> 32) ^ k1))
    return np.uint32(k1), np.uint32(k2)


def row_hashes(n_rows, seed, counter, off):
    """``lowbias32(lowbias32(b + off + k1) ^ k2)`` of rows ``0 .. n_rows - 1``: the 32-bit stream at index range ``off``
    (every per-row draw of the augmentation kernels: shift, width, gain, tilt)."""
    k1, k2 = step_keys(seed, counter)
    with np.errstate(over="ignore"):
        b = np.arange(n_rows, dtype=np.uint32) + np.uint32(off) + k1
    return lowbias32(lowbias32(b) ^ k2)


def row_uniforms(n_rows, seed, counter, off):
    """``float(h_b >> 8) * 2^-24`` of that stream, fp32, in ``[0, 1)`` (24 bits: exact)."""
    return (row_hashes(n_rows, seed, counter, off) >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)


def uniforms(n_rows, seed, counter):
    """``u_b`` of rows ``0 .. n_rows - 1``: the shift's draw."""
    return row_uniforms(n_rows, seed, counter, OFF)


def deltas(n_rows, seed, counter, s):
    """``delta_b = (2 u_b - 1) * s`` in fp32: ``2 u - 1`` is exact, the product is the only rounding."""
    t = np.float32(2.0) * uniforms(n_rows, seed, counter) - np.float32(1.0)
    return (t * np.float32(s)).astype(np.float32)


def positions(delta, L):
    """``(i0, i1, f)`` of every ``(b, l)``: ``x = min(max(float(l) + delta_b, 0), L - 1)`` in fp32, ``i0 = floor(x)``,
    ``f = x - i0`` (fp32, exact), ``i1 = min(i0 + 1, L - 1)``."""
    delta = np.asarray(delta, dtype=np.float32)
    x = (np.arange(L, dtype=np.float32)[None, :] + delta[:, None]).astype(np.float32)
    x = np.minimum(np.maximum(x, np.float32(0.0)), np.float32(L - 1))
    fl = np.floor(x)
    f = (x - fl).astype(np.float32)
    i0 = fl.astype(np.int64)
    assert np.all(fl.astype(np.float64) + f.astype(np.float64) == x.astype(np.float64))      # (f is exact)
    return i0, np.minimum(i0 + 1, L - 1), f


def shift_rows_by(rows, delta):
    """``rows`` [B][L] resampled at ``l + delta_b``, linear with replicated edges; float64."""
    rows = np.asarray(rows, dtype=np.float64)
    i0, i1, f = positions(delta, rows.shape[1])
    v0, v1 = np.take_along_axis(rows, i0, axis=1), np.take_along_axis(rows, i1, axis=1)
    return v0 + f.astype(np.float64) * (v1 - v0)


def shift_rows(rows, seed, counter, s):
    """The augmented batch without its noise term: row b of ``rows`` shifted by its own ``delta_b``."""
    rows = np.asarray(rows)
    return shift_rows_by(rows, deltas(rows.shape[0], seed, counter, s))
