"""Float64 / Python-integer reference of ``csrc/raae_optim.hip`` with ``raae_optim_body.inc``: the four update rules
(``OptRule<R>::scalars`` / ``::update`` under ``update_body``), the slab sum (``slab_sum`` / ``slab_sum_wide``), the random tape (Philox4x32-10, ``u01``, Box-Muller; the mask kinds through ``dense_reference.mask_hash``),
``raae_step_tick`` and ``raae_step_begin`` -- with a mirror of the dispatch (which kernel shape and grid a call takes).
Plain numpy, no autograd, nothing imported from the package.  The oracle of ``test_step_kernels_gpu.py``;
``test_step_reference_cpu.py`` pins it to ``torch.optim`` / ``optim_reference`` in float64 and to the Random123
known-answer vectors.  Not a conftest: tests import it.

Update rules (``hyper`` = {lr, beta1, beta2, eps, weight_decay, base_lr, final_lr, gamma}, ``t`` the 1-based step
count, the per-step scalars formed in Python floats in the order of the kernels' ``scalars``)::

    Adam / AdamW   g += wd p (Adam) | p *= 1 - lr wd (AdamW);  m += (1 - b1)(g - m);  v = b2 v + (1 - b2) g g
                   p -= lr / bc1 * m / (sqrt(v) / sqrt(bc2) + eps)
    RAdam          v, m as above (m = b1 m + (1 - b1) g);  p += -wd lr p;  N = Nmax - 2 t b2^t / (1 - b2^t)
                   N >= 5: p -= ss m / (sqrt(v) + eps), else p -= lr / bc1 * m
    AdaBound       g += wd p;  m, v;  x = clamp(lr sqrt(bc2) / bc1 / (sqrt(v) + eps), lo, hi) m;  p -= x
                   lo, hi = final_lr lr / base_lr * (1 - 1 / (gamma t + 1)), ... * (1 + 1 / (gamma t))

``g`` is the sum of the first ``seg_nslab[i / 64]`` slab rows of element ``i`` (times the clip scale, before weight
decay and the moments); a segment with 0 slabs is left untouched.

Random tape.  ``u01`` is the exact ``((x >> 8) + 0.5) / 2^24``; the kernel forms it in fp32, where ``k + 0.5`` is not
representable from ``k = 2^23`` on and rounds to the even neighbour (``u01_f32``; ``u01_f32(0xffffffff) == 1.0``, a
radius of 0).  ``normal4`` starts from the values the kernel holds -- ``u01_f32`` and the fp32 angle
``float32(2 pi) * u`` -- and takes ``log``, ``sqrt``, ``cos`` and ``sin`` in float64.
"""
import functools
import math

import numpy as np

from dense_reference import gen_params, mask_hash, step_keys

ADAM, ADAMW, RADAM, ADABOUND = 0, 1, 2, 3           # _lib.OPT_*
RULE_NAMES = {ADAM: "Adam", ADAMW: "AdamW", RADAM: "RAdam", ADABOUND: "AdaBound"}
HYPER = (0.01, 0.9, 0.999, 1e-8, 0.01, 0.01, 0.1, 1e-3)
GRID_CAP, LANES8_ABOVE = 4096, 16
M32 = 0xFFFFFFFF


# ------------------------------------------------------------------------------------------------------ dispatch mirror
def update_form(n, max_nslab):
    """(shape, grid) of every update kernel and of ``raae_slab_reduce`` (``optim_grid``): one thread per element, or 8
    lanes per element (32 elements per workgroup) above 16 slabs; at most 4096 workgroups."""
    if max_nslab > LANES8_ABOVE:
        return "lanes8", min(GRID_CAP, (n + 31) // 32)
    return "thread", min(GRID_CAP, (n + 255) // 256)


def rng_fill_grid(total):
    return max(1, min(GRID_CAP, (total // 4 + 255) // 256))


def step_begin_grid(B, L, total):
    """~16 quads per thread over the larger of the gather and the fill; 64 ... 1024 workgroups."""
    work = max(B * L // 4, total // 4)
    return max(64, min(1024, (work + 4095) // 4096))


def step_begin_form(B, L, spec_noise, noise_from_tape, nseg):
    return ("vector" if L % 4 == 0 else "scalar",
            "none" if spec_noise == 0 else ("tape" if noise_from_tape else "generated"),
            "nofill" if nseg == 0 else ("lds" if nseg <= 256 else "global"))


# ------------------------------------------------------------------------------------------------------ update rules
def radam_scalars(hyper, t):
    """(N, rectified, step size) of torch_optimizer.RAdam at step ``t``."""
    lr, b1, b2 = hyper[0], hyper[1], hyper[2]
    b2t = b2 ** t
    nmax = 2.0 / (1.0 - b2) - 1.0
    nsma = nmax - 2.0 * t * b2t / (1.0 - b2t)
    if nsma >= 5.0:
        ss = lr * math.sqrt((1.0 - b2t) * (nsma - 4.0) / (nmax - 4.0) * (nsma - 2.0) / nsma * nmax / (nmax - 2.0)) / \
            (1.0 - b1 ** t)
        return nsma, True, ss
    return nsma, False, lr / (1.0 - b1 ** t)


def adabound_scalars(hyper, t):
    """(step size, lower bound, upper bound) of torch_optimizer.AdaBound at step ``t``."""
    lr, b1, b2, _, _, base_lr, final_lr, gamma = hyper[:8]
    ss = lr * math.sqrt(1.0 - b2 ** t) / (1.0 - b1 ** t)
    flr = final_lr * lr / base_lr
    return ss, flr * (1.0 - 1.0 / (gamma * t + 1.0)), flr * (1.0 + 1.0 / (gamma * t))


def update(rule, p, m, v, g, hyper, t, scale=None, info=None):
    """One step of ``rule`` in float64 on arrays ``p, m, v, g`` (not modified); returns ``(p, m, v)``.  ``info`` (a
    dict) receives AdaBound's clamp hits ``lo`` / ``hi`` (bool arrays)."""
    p, m, v, g = (np.array(a, dtype=np.float64) for a in (p, m, v, g))
    lr, b1, b2, eps, wd = (float(x) for x in hyper[:5])
    t = int(t)
    if scale is not None:
        g = g * float(scale)
    if rule in (ADAM, ADAMW):
        bc1, bc2 = 1.0 - b1 ** t, 1.0 - b2 ** t
        if rule == ADAMW:
            p = p * (1.0 - lr * wd)
        elif wd != 0.0:
            g = g + wd * p
        m = m + (1.0 - b1) * (g - m)
        v = v * b2 + (1.0 - b2) * g * g
        p = p - (lr / bc1) * m / (np.sqrt(v) / math.sqrt(bc2) + eps)
    elif rule == RADAM:
        _, rect, ss = radam_scalars(hyper, t)
        v = v * b2 + (1.0 - b2) * g * g
        m = m * b1 + (1.0 - b1) * g
        if wd != 0.0:
            p = p + (-wd * lr) * p
        p = p - ss * m / (np.sqrt(v) + eps) if rect else p - ss * m
    elif rule == ADABOUND:
        ss, lo, hi = adabound_scalars(hyper, t)
        if wd != 0.0:
            g = g + wd * p
        m = m * b1 + (1.0 - b1) * g
        v = v * b2 + (1.0 - b2) * g * g
        x = ss / (np.sqrt(v) + eps)
        if info is not None:
            info["lo"], info["hi"] = x < lo, x > hi
        p = p - np.clip(x, lo, hi) * m
    else:
        raise ValueError(rule)
    return p, m, v


def slab_sum(slabs, counts):
    """``(g, has)``: float64 sum of the first ``counts[i / 64]`` rows of ``slabs`` [rows, n] per element, and whether
    the element's segment has a slab at all.  Rows at and beyond a segment's count are never read."""
    slabs = np.asarray(slabs)
    n = slabs.shape[1]
    g = np.zeros(n)
    for s, c in enumerate(counts):
        if c > 0:
            g[64 * s:64 * s + 64] = slabs[:c, 64 * s:64 * s + 64].astype(np.float64).sum(0)
    return g, np.repeat(np.asarray(counts) > 0, 64)


def slab_abs_sum(slabs, counts):
    """Sum of the magnitudes of the rows ``slab_sum`` adds: the scale of the fp32 summation bound."""
    return slab_sum(np.abs(np.asarray(slabs)), counts)[0]


def step(rule, p, m, v, slabs, counts, hyper, t, scale=None, info=None):
    """``update`` on the slab sum; elements of a segment without slabs keep ``p, m, v``."""
    g, has = slab_sum(slabs, counts)
    pn, mn, vn = update(rule, p, m, v, g, hyper, t, scale, info)
    keep = lambda new, old: np.where(has, new, np.asarray(old, dtype=np.float64))
    return keep(pn, p), keep(mn, m), keep(vn, v)


# ------------------------------------------------------------------------------------------------------ Philox4x32-10
PHILOX_M0, PHILOX_M1 = 0xD2511F53, 0xCD9E8D57
PHILOX_W0, PHILOX_W1 = 0x9E3779B9, 0xBB67AE85


def philox4x32_10_int(counter, key):
    """Scalar form in Python integers: 4 counter words, 2 key words -> 4 output words."""
    c0, c1, c2, c3 = (int(x) & M32 for x in counter)
    k0, k1 = (int(x) & M32 for x in key)
    for _ in range(10):
        p0, p1 = PHILOX_M0 * c0, PHILOX_M1 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & M32, (p0 >> 32) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + PHILOX_W0) & M32, (k1 + PHILOX_W1) & M32
    return c0, c1, c2, c3


def philox4x32_10(counter, key):
    """Vectorised over numpy ``uint64``: ``counter`` four arrays (or scalars) of 32-bit words, ``key`` two scalars."""
    c = [np.atleast_1d(np.asarray(x, dtype=np.uint64)) & np.uint64(M32) for x in counter]
    shape = np.broadcast(*c).shape
    c = [np.broadcast_to(x, shape) for x in c]
    k0, k1 = int(key[0]) & M32, int(key[1]) & M32
    m32, s32 = np.uint64(M32), np.uint64(32)
    for _ in range(10):
        p0, p1 = np.uint64(PHILOX_M0) * c[0], np.uint64(PHILOX_M1) * c[2]      # < 2^64: no wrap
        c = [(p1 >> s32) ^ c[1] ^ np.uint64(k0), p1 & m32, (p0 >> s32) ^ c[3] ^ np.uint64(k1), p0 & m32]
        k0, k1 = (k0 + PHILOX_W0) & M32, (k1 + PHILOX_W1) & M32
    return c


def u01(x):
    """``((x >> 8) + 0.5) / 2^24`` exactly (float64): strictly inside (0, 1)."""
    return ((np.asarray(x, dtype=np.uint64) >> np.uint64(8)).astype(np.float64) + 0.5) / 16777216.0


def u01_f32(x):
    """``u01`` as the kernel forms it: ``(float(x >> 8) + 0.5f) * 2^-24`` in fp32.  Equal to ``u01`` below
    ``x >> 8 = 2^23``; from there ``k + 0.5`` rounds to the even neighbour, and ``k = 2^24 - 1`` gives exactly 1.0."""
    k = (np.asarray(x, dtype=np.uint64) >> np.uint64(8)).astype(np.float32)
    return (k + np.float32(0.5)) * np.float32(1.0 / 16777216.0)


TWO_PI_F32 = np.float32(6.283185307179586)


def _gauss_words(qg, ctr, seed):
    qg = np.atleast_1d(np.asarray(qg, dtype=np.int64)).astype(np.uint64)
    ctr, seed = int(ctr) % 2 ** 64, int(seed) % 2 ** 64
    return philox4x32_10([qg & np.uint64(M32), qg >> np.uint64(32), ctr & M32, ctr >> 32], [seed & M32, seed >> 32])


def normal4(qg, ctr, seed):
    """Philox blocks ``qg`` (array) of step ``ctr``: ``(z [len, 4], r [len, 4])`` in float64 -- the four N(0, 1) values
    {r0 cos a0, r0 sin a0, r1 cos a1, r1 sin a1} (words 0 and 2 the radii, 1 and 3 the angles) and the radius of each."""
    w = _gauss_words(qg, ctr, seed)
    out, rad = [], []
    for wr, wa in ((w[0], w[1]), (w[2], w[3])):
        r = np.sqrt(-2.0 * np.log(u01_f32(wr).astype(np.float64))) + 0.0        # (+ 0.0: no negative zero)
        a = (TWO_PI_F32 * u01_f32(wa)).astype(np.float64)                        # the fp32 product the kernel holds
        out += [r * np.cos(a), r * np.sin(a)]
        rad += [r, r]
    return np.stack(out, 1), np.stack(rad, 1)


def normal4_f32(qg, ctr, seed):
    """The same chain evaluated in numpy float32 on the CPU: NOT the reference, the yardstick of the Gaussian
    tolerance (module docstring of ``test_step_kernels_gpu.py``)."""
    w = _gauss_words(qg, ctr, seed)
    out = []
    for wr, wa in ((w[0], w[1]), (w[2], w[3])):
        r = np.sqrt(np.float32(-2.0) * np.log(u01_f32(wr)))
        a = TWO_PI_F32 * u01_f32(wa)
        out += [r * np.cos(a), r * np.sin(a)]
    z = np.stack(out, 1)
    assert z.dtype == np.float32
    return z


@functools.lru_cache(maxsize=8)
def gauss_slot(goff, count, ctr, seed):
    """Elements 0 .. count - 1 of a Gaussian slot whose numbering starts at ``goff``: element ``i`` is lane ``i & 3`` of
    block ``(goff + 4 (i / 4)) >> 2`` (``fill_quad``; ``step_begin``, whose ``goff`` is a multiple of 4: block
    ``(goff + i) >> 2``, lane ``(goff + i) & 3`` -- the same).  Returns ``(z, r)``, read-only."""
    q = (int(goff) + 4 * np.arange((count + 3) // 4, dtype=np.int64)) >> 2
    z, r = normal4(q, ctr, seed)
    z, r = z.reshape(-1)[:count], r.reshape(-1)[:count]
    z.setflags(write=False)
    r.setflags(write=False)
    return z, r


def ulp32(x):
    """Spacing of the fp32 grid at ``|x|`` (float64)."""
    return np.spacing(np.abs(np.asarray(x, dtype=np.float64)).astype(np.float32)).astype(np.float64)


def gauss_f32_error_ulps(goff, count, ctr, seed):
    """Largest error of ``normal4_f32`` against ``normal4`` over a slot, in fp32 ulps of the radius."""
    z, r = gauss_slot(int(goff), int(count), int(ctr), int(seed))
    q = (int(goff) + 4 * np.arange((count + 3) // 4, dtype=np.int64)) >> 2
    z32 = normal4_f32(q, ctr, seed).astype(np.float64).reshape(-1)[:count]
    ok = r > 0
    return float((np.abs(z32 - z)[ok] / ulp32(r[ok])).max()) if ok.any() else 0.0


# ------------------------------------------------------------------------------------------------------ tape
def fill(seg_desc, seg_scale, total, seed, ctr, sentinel):
    """The whole tape after ``raae_rng_fill`` / the fill of ``raae_step_begin``: dict of ``tape`` (float64 [total]; the
    mask kinds hold their exact fp32 values, kind 2 as the float whose bits are the two bf16 flags), ``kind`` (int8,
    -1: owned by no segment, keeps ``sentinel``) and ``radius`` (float64, the Gaussian elements' radii, else 0).
    ``seg_desc`` rows {offset, count, kind, hash offset | start in the Gaussian numbering}, ``seg_scale`` = keep."""
    tape = np.full(total, float(sentinel))
    kind = np.full(total, -1, dtype=np.int8)
    radius = np.zeros(total)
    k1, k2 = step_keys(int(seed) % 2 ** 64, int(ctr) % 2 ** 64)
    for (off, cnt, kd, hoff), keep in zip(np.asarray(seg_desc).reshape(-1, 4).tolist(), np.asarray(seg_scale).tolist()):
        cnt = max(0, min(cnt, total - off))
        if cnt == 0:
            continue
        sl = slice(off, off + cnt)
        kind[sl] = kd
        if kd == 0:
            tape[sl], radius[sl] = gauss_slot(int(hoff), int(cnt), int(ctr) % 2 ** 64, int(seed) % 2 ** 64)
        elif kd == 1:
            thr, inv = gen_params(keep)
            tape[sl] = mask_hash(k1, k2, hoff, thr, cnt).astype(np.float32) * inv
        else:
            thr, _ = gen_params(keep)
            flags = mask_hash(k1, k2, hoff, thr, 2 * cnt).astype(np.uint32) * np.uint32(0x3F80)
            tape[sl] = (flags[0::2] | (flags[1::2] << np.uint32(16))).view(np.float32)
    return dict(tape=tape, kind=kind, radius=radius)


# ------------------------------------------------------------------------------------------------------ step head
def tick(steps, n, mask, ctr=None, seed=0, cursor=None, cursor_inc=0):
    """``raae_step_tick``: dict of ``steps`` (the first ``n`` advanced under ``mask``), ``ctr`` / ``keys`` (None without
    a counter block) and ``cursor`` (None without one)."""
    steps = [int(s) + (1 if (i < n and (mask >> i) & 1) else 0) for i, s in enumerate(steps)]
    out = dict(steps=steps, ctr=None, keys=None, cursor=None if cursor is None else int(cursor) + int(cursor_inc))
    if ctr is not None:
        out["ctr"] = (int(ctr) + 1) % 2 ** 64
        out["keys"] = step_keys(int(seed) % 2 ** 64, out["ctr"])
    return out


def step_begin(steps, nsteps, mask, ctr, seed, cursor, stride, spec, aux, idx, B, spec_noise=0.0, noise=None,
               noise_goff=0, fill_args=None):
    """``raae_step_begin`` from the state the previous step left: works with ``ctr + 1`` and ``cursor + stride``,
    gathers rows ``idx[cursor + stride - B, cursor + stride)``.  ``noise``: the fp32 values of a tape slot [B * L], or
    None: generated at ``noise_goff`` of the Gaussian numbering (when ``spec_noise != 0``).  ``fill_args`` =
    (seg_desc, seg_scale, total, sentinel) or None.  Returns the ``tick`` dict plus ``rows`` (the gathered spectra),
    ``spec_out`` (float64), ``z`` / ``radius`` (the noise and, when generated, its radii), ``aux_out``, ``tape``."""
    out = tick(steps, nsteps, mask, ctr, seed, cursor, stride)
    spec, aux = np.asarray(spec), np.asarray(aux)
    L = spec.shape[1]
    sel = np.asarray(idx)[out["cursor"] - B:out["cursor"]]
    rows = spec[sel]
    out.update(rows=rows, aux_out=aux[sel], z=None, radius=None, tape=None, spec_out=rows.astype(np.float64))
    if spec_noise != 0.0:
        if noise is not None:
            z, r = np.asarray(noise, dtype=np.float64).reshape(B, L), None
        else:
            z, r = gauss_slot(int(noise_goff), B * L, out["ctr"], int(seed) % 2 ** 64)
            z, r = z.reshape(B, L), r.reshape(B, L)
        out.update(z=z, radius=r, spec_out=rows.astype(np.float64) + z * float(np.float32(spec_noise)))
    if fill_args is not None:
        desc, scale, total, sentinel = fill_args
        out["tape"] = fill(desc, scale, total, seed, out["ctr"], sentinel)
    return out
