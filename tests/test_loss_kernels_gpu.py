"""Every kernel form of ``csrc/raae_loss.hip`` (style BatchNorm, the rank loss in all its forms, the recon, smoothness,
MSE and BCE losses, ``raae_loss_finalize``, ``raae_disc_input``, ``raae_scale_by_dev``, ``raae_gather_batch``) and of
``csrc/raae_disc.hip`` (``raae_disc_fused``) against the float64 reference of ``loss_reference``, one launch at a time.

* INPUTS are rounded to fp32 before the reference sees them (``f32``): both sides compute on the same numbers.
* ROUTE: ``test_loss_reference_cpu.py`` holds the case tables below to the mirrored dispatch of ``loss_reference``; here
  the partial / slab counts the library returns equal the mirror's, and the rank pair pass must have written exactly
  the mirror's number of ``RankWork`` records and column blocks into a work buffer that starts as sentinel bytes.  The
  module is skipped when ``RAAE_DISC_MFMA`` is set (the mirror holds the defaults).
* HYGIENE: outputs, partials beyond the returned count, slab rows beyond ``nslab`` and four guard elements behind each
  written tensor start at a sentinel and keep it outside what the call owns; a second identical launch is bitwise
  equal; a ticket reads 0 afterwards; the loss-only form (NULL gradient) gives the same loss bits.
* TOLERANCES are those of ``test_ops_gpu.py`` with its fixed 1e-9 gradient floors replaced by derived ones:
    rank dz     1e-5 |ref| + 4 u (|c| |g+| + |g-|) 2 / norm: ``f (c g+ + g-)`` is three fp32 operations on exact integers
                g+- (u = 2^-24), the fourth u covers the rounding of f and c.  Loss 1e-5 |ref| + 1e-7.
    recon dy    1e-4 |ref| + 4 u (|y| + |x| c) 2 / (B L) for the cancellation in ``y - x c`` (product, difference, the
                factor 2 / (B L), the final sum: four roundings of operands of that size), plus for the ``gscale`` term
                0.2 dr / (|mx| L B) + 4 u |gscale| with dr = r (e_x + e_y + 3 u) the error of ``r - 1``: an fp32 mean over
                L terms -- ceil(L / 64) sequential additions per lane and a 6-level tree -- is within
                e = (ceil(L / 64) + 6) u mean|v| / |mean v| of the mean, and r takes two such means, a division and two
                conversions.  Loss 1e-5 relative.
    smooth dx   1e-4 |ref| + (ntaps + 2) u max|x| 2 / (B L): ntaps multiply-adds and two differences on operands of size
                max|x|.  Loss 2e-5 relative.
    MSE da 1e-5 + 1e-9, loss 1e-6; BCE dlogits 1e-5 + 1e-9, loss 1e-6; finalize and the glue kernels one fp32 ulp.
    style BN    forward 1e-5 + 1e-5, dz 1e-4 + 2e-5, running statistics 1e-4 + 1e-6.
    disc_fused  loss 1e-5 + 1e-6, gradients 1e-7 + 2e-4 max|ref| + 2e-4 |ref|; a row may miss only if the float64 forward
                has a hidden pre-activation with |z| < 1e-5 max|z| in it (a tensor then misses in at most 130 entries per
                such row, by at most 5 % of its largest entry); the cases up to 63 rows have no such row.

FORM -> CASE (the table test of ``test_loss_reference_cpu.py`` recomputes this map and fails on a gap):
  rank pairs   KA 1..16, R = 1, unmasked / masked: ka{K}_u / ka{K}_m (B = 37); tile edges tile{B}_k3 / _k7
               KA 1..16, R = 4, column blocks, unmasked / masked: r4_1025_k{K}_{u,m}; KA {1,3,7,11,16} also at 1030
               rows: r4_1030_k{K}_{u,m}; the empty last column block: r4_1030_k1_* (the 64 instances are KA x R x
               masked: every one has a case of its own)
               R = 4, nj = 1: big_8192; nj = 2: big_8184; grid stride: big_16392_u / big_16392_m
               R = 1 with nj > 1 (rows form only): rows_1030_515_*; one-row and R = 4 shares rows_1030_1_1029_* /
               rows_1030_1029_1_*; small splits rows_40_*
  recon        plain / flexible target: rc_{B}x{L}_{p,s}; rows stride: rc_2049x8_*
  smooth       17 taps: sm17_{L}, sm17_2049x20, sm17_L2048; generic: smg_{taps}_{L}; last: L = 4096
  mse, bce, finalize, glue: one kernel each; the grid-stride shapes are mse_524291, di_stride, sc_stride, ga_stride
  style BN     forward sf_*; backward sb_{C}_{B}
  disc_fused   VALU dv_*; matrix core dm_*
  batched      pl_* (one two-plane program per entry point with a ``_m`` twin)
"""
import collections
import ctypes as C
import functools
import os
import time
import zlib

import numpy as np
import pytest
import torch

import loss_reference as lr
from loss_reference import f32, U32

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif("RAAE_DISC_MFMA" in os.environ, reason="RAAE_DISC_MFMA is set: the mirror holds the defaults")]

if torch.cuda.is_available():
    from rankaae_amd import ops, _lib
    DEV = torch.device("cuda:0")

MAXP = 512
SENT = -777.25
SENT_BYTE = 0xA5
WORST = collections.defaultdict(float)       # quantity class -> largest share of its bound over the session


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


# ======================================================================================================= case tables
# ---------------------------------------------------------------------------------------------------------- rank loss
RankCase = collections.namedtuple("RankCase", "name B K masked scaled")
RANK_CASES = ([RankCase(f"ka{K}_{'m' if m else 'u'}", 37, K, m, False) for K in range(1, 17) for m in (False, True)] +
              [RankCase(f"tile{B}_k{K}_{'m' if m else 'u'}", B, K, m, False)
               for B in (2, 255, 256, 257, 513) for K in (3, 7) for m in (False, True)] +
              [RankCase(f"r4_{B}_k{K}_{'m' if m else 'u'}", B, K, m, False)
               for B in (1025, 1030) for K in (1, 3, 7, 11, 16) for m in (False, True)] +
              # the other eleven descriptor counts at R = 4 (any run above 1024 rows with 2, 4, 5, 6, ... descriptors)
              [RankCase(f"r4_1025_k{K}_{'m' if m else 'u'}", 1025, K, m, False)
               for K in (2, 4, 5, 6, 8, 9, 10, 12, 13, 14, 15) for m in (False, True)])
BIG_RANK_CASES = [RankCase("big_8192", 8192, 16, False, True), RankCase("big_8184", 8184, 16, False, True),
                  RankCase("big_16392_u", 16392, 16, False, True), RankCase("big_16392_m", 16392, 16, True, True)]
RANK_BY_NAME = {c.name: c for c in RANK_CASES + BIG_RANK_CASES}

RowsCase = collections.namedtuple("RowsCase", "name n_all K split masked")
ROWS_CASES = [RowsCase(f"rows_{n}_{'_'.join(map(str, s))}_{'m' if m else 'u'}", n, K, s, m)
              for n, K, s in ((1030, 3, (515, 515)), (1030, 3, (1, 1029)), (1030, 3, (1029, 1)), (40, 5, (13, 27)),
                              (40, 5, (1, 2, 37)))
              for m in (False, True)]
ROWS_BY_NAME = {c.name: c for c in ROWS_CASES}

# exact in fp32 on styles that are multiples of 2^-10 below 8: (1 + k / 16) 2^e has five mantissa bits
BIG_FACTORS = [(-1.0 if k % 3 == 1 else 1.0) * (1.0 + k / 16.0) * 2.0 ** (k % 3 - 1) for k in range(16)]


@functools.lru_cache(maxsize=None)
def rank_data(name, B, K, masked, scaled):
    """``(d [B, K] float64 on the fp32 grid, NaN = no label; z [B, K + 1])``.  Plain cases: one descriptor column is
    integer-valued (ties in d); about 5 % of style columns 0 and 1 is duplicated (p == 0 while d differs: the pair counts in
    neither sum); masked: about 25 % of the cells are NaN and from K >= 3 one column has m = 0 and one m = 1."""
    g = _rng(name.rsplit("_", 1)[0] if name.startswith("rows_") else name)
    if scaled:
        d0 = np.round(g.standard_normal(B) * 16) / 16
        z0 = np.clip(np.round(g.standard_normal(B) * 1024) / 1024, -7.5, 7.5)
        if masked:
            d0[g.random(B) < 0.25] = np.nan
        d = np.repeat(d0[:, None], K, 1)
        z = np.concatenate([z0[:, None] * np.array(BIG_FACTORS[:K])[None, :], g.standard_normal((B, 1))], 1)
        return f32(d), f32(z)
    d = f32(g.standard_normal((B, K)))
    d[:, min(1, K - 1)] = g.integers(4, 7, size=B)
    z = f32(g.standard_normal((B, K + 1)))
    ndup = max(1, B // 20)
    for col in sorted({0, min(1, K - 1)}):                      # also in the integer-valued column, which stays labelled
        z[g.choice(B, ndup, replace=False), col] = z[g.choice(B, ndup), col]
    if masked:
        gone = g.random((B, K)) < 0.25
        if K >= 3:
            gone[:, 2] = True                                   # m = 0
            one = 3 if K >= 4 else 0                            # never the integer-valued column 1: it keeps its labels
            gone[:, one] = True
            gone[B // 2, one] = False                           # m = 1
        d[gone] = np.nan
    return d, z


@functools.lru_cache(maxsize=None)
def rank_ref(name):
    """``(d, z, Pairs, seconds the reference took)`` of a whole-batch case; shared by every test that needs it."""
    c = RANK_BY_NAME[name]
    d, z = rank_data(*c)
    t0 = time.perf_counter()
    if c.scaled:
        P = lr.rank_pairs_scaled(d[:, 0], z[:, 0] / BIG_FACTORS[0], BIG_FACTORS[:c.K], c.masked)
    else:
        P = lr.rank_pairs(d, z[:, :c.K], c.masked)
    return d, z, P, time.perf_counter() - t0


# ------------------------------------------------------------------------------------------------------ recon, smooth
ReconCase = collections.namedtuple("ReconCase", "name B L scale")
RECON_CASES = ([ReconCase("rc_1x1_p", 1, 1, False)] +
               [ReconCase(f"rc_{B}x{L}_{'s' if s else 'p'}", B, L, s)
                for B, L in ((3, 63), (4, 64), (5, 65), (7, 1000), (2049, 8)) for s in (False, True)])


@functools.lru_cache(maxsize=None)
def recon_data(c):
    """Flexible-target rows by ``row % 5``: 0 ratio > 1.3, 1 ratio < 0.7, 2 a negative output mean (ratio inside),
    3 a negative input mean, 4 strictly inside."""
    g = _rng(c.name)
    x = g.random((c.B, c.L)) + 0.2
    y = x + 0.3 * g.standard_normal((c.B, c.L)) / max(1.0, (8.0 / c.L) ** 0.5 * 2)
    r = np.arange(c.B) % 5
    y[r == 0] *= 2.0
    y[r == 1] *= 0.3
    y[r == 2] *= -1.0
    x[r == 3] *= -1.0
    return f32(x), f32(y)


SmoothCase = collections.namedtuple("SmoothCase", "name B L taps")
SMOOTH_CASES = ([SmoothCase(f"sm17_{L}", 5, L, "g17") for L in (2, 5, 8, 9, 16, 17, 20, 64, 65, 256)] +
                [SmoothCase("sm17_2049x20", 2049, 20, "g17"), SmoothCase("sm17_L2048", 5, 2048, "g17")] +
                [SmoothCase(f"smg_{t}_{L}", 5, L, t) for t in ("g1", "g3", "g15", "g33", "asym5") for L in (2, 7, 40, 70)])


def taps_of(kind):
    if kind == "asym5":                                          # not symmetric: a flipped tap index shows
        w = _rng("asym5").random(5) + 0.1
        return f32(w / w.sum())
    from oracle.ref_model import gaussian_taps
    return gaussian_taps(int(kind[1:]), 3.0).double().numpy()


@functools.lru_cache(maxsize=None)
def smooth_data(c):
    g = _rng(c.name)
    return f32(g.random((c.B, c.L)) + 0.1 * g.standard_normal((c.B, c.L)))


# ---------------------------------------------------------------------------------------------------- style BatchNorm
StyleF = collections.namedtuple("StyleF", "name B C nparts mode")
_MODES, _NP = ("train_u", "train", "eval"), (1, 3, 512)
STYLE_FWD = ([StyleF(f"sf_{C}_{B}", B, C, _NP[i % 3], _MODES[(i + i // 3) % 3])
              for i, (C, B) in enumerate((C, B) for C in (1, 6, 13, 16, 64) for B in (2, 37))] +
             [StyleF("sf_stride", 1100, 64, 512, "train_u"), StyleF("sf_stride_eval", 1100, 64, 3, "eval")])
StyleB = collections.namedtuple("StyleB", "name B C")
STYLE_BWD = ([StyleB(f"sb_{C}_{B}", B, C) for C in (6, 13, 64) for B in
              (4 * (1024 // C) - 1, 4 * (1024 // C), 4 * (1024 // C) + 1)] + [StyleB("sb_6_2", 2, 6), StyleB("sb_13_2", 2, 13)])


@functools.lru_cache(maxsize=None)
def style_data(name, B, Cc, nparts):
    g = _rng(name)
    z = f32(g.standard_normal((B, Cc)) * 2 + 0.5)
    rows = lr.partial_rows(z, nparts)
    run = (f32(g.standard_normal(Cc) * 0.3), f32(g.random(Cc) + 0.5))
    dy = f32(g.standard_normal((B, Cc)))
    return z, rows, run, dy


# ------------------------------------------------------------------------------------------------------- discriminator
DiscCase = collections.namedtuple("DiscCase", "name n_real n_fake ns noise masks seed")
DISC_CASES = [
    DiscCase("dv_1_1_1", 1, 1, 1, True, True, 0), DiscCase("dv_16_16_16", 16, 16, 16, True, True, 0),
    DiscCase("dv_40_23_6", 40, 23, 6, True, True, 0), DiscCase("dv_17_15_13_bare", 17, 15, 13, False, False, 0),
    DiscCase("dv_1000_1047_6", 1000, 1047, 6, True, True, 0),
    DiscCase("dm_1000_1048_6", 1000, 1048, 6, True, True, 0), DiscCase("dm_1_2047_16", 1, 2047, 16, True, True, 0),
    DiscCase("dm_2056_2057_3", 2056, 2057, 3, True, True, 0),
]
DISC_BY_NAME = {c.name: c for c in DISC_CASES}
DISC_PARAMS = ("w1", "b1", "s1", "w2", "b2", "s2", "w3", "b3")
SIGMA, ALPHA, DROP = 0.56, 0.37, 0.056


@functools.lru_cache(maxsize=None)
def disc_data(name, variant=0):
    """Inputs of a case (float64 on the fp32 grid) and the reference's result.  ``variant``: other inputs of the same
    geometry (the second plane of a batched launch)."""
    c = DISC_BY_NAME[name]
    g = _rng(f"{name}/{c.seed}/{variant}")
    n, H, ns = c.n_real + c.n_fake, 64, c.ns
    t = dict(z_real=f32(g.standard_normal((c.n_real, ns))), styles=f32(g.standard_normal((c.n_fake, ns))),
             noise=f32(g.standard_normal((n, ns))) if c.noise else None)
    for i in (1, 2):
        t[f"m{i}"] = f32((g.random((n, H)) > DROP) / (1 - DROP)) if c.masks else None
    t["w1"], t["b1"] = f32((g.random((H, ns)) * 2 - 1) / ns ** 0.5), f32((g.random(H) * 2 - 1) / ns ** 0.5)
    t["w2"], t["b2"] = f32((g.random((H, H)) * 2 - 1) / 8), f32((g.random(H) * 2 - 1) / 8)
    t["w3"], t["b3"] = f32((g.random((1, H)) * 2 - 1) / 8), f32((g.random(1) * 2 - 1) / 8)
    t["s1"], t["s2"] = f32(0.1 + 0.3 * g.random(H)), f32(0.1 + 0.3 * g.random(H))
    alpha = float(f32(ALPHA))
    t["ref"] = lr.disc_fused(t["z_real"], t["styles"], t["noise"], float(f32(SIGMA)), t["m1"], t["m2"],
                             *[t[k] for k in DISC_PARAMS], alpha)
    t["near"] = lr.near_zero_rows(t["ref"]["z1"], t["ref"]["z2"])
    return t


# =================================================================================================== device plumbing
class Report:
    def __init__(self, case):
        self.case, self.bad = case, []

    def close(self, kind, what, got, want, tol):
        """``|got - want| <= tol`` element-wise (``tol`` an array or a number)."""
        got = got.detach().double().cpu().numpy() if torch.is_tensor(got) else np.asarray(got, np.float64)
        want = np.asarray(want, np.float64).reshape(got.shape)
        tol = np.broadcast_to(np.asarray(tol, np.float64), got.shape)
        err = np.abs(got - want)
        finite = bool(np.isfinite(got).all())
        with np.errstate(divide="ignore", invalid="ignore"):
            share = np.where(err == 0, 0.0, err / tol)
        ratio = float(share.max()) if finite and got.size else (0.0 if finite else float("inf"))
        WORST[kind] = max(WORST[kind], ratio)
        print(f"CMP {self.case} {what}: max err {float(err.max()) if got.size else 0.0:.3e} "
              f"(max |ref| {float(np.abs(want).max()) if got.size else 0.0:.3e}), {ratio:.3f} of the bound [{kind}]")
        if not (ratio <= 1.0):
            i = int(np.nan_to_num(share, nan=np.inf).argmax())
            self.bad.append(f"{what}: {ratio:.2f} x bound at flat index {i}: ref {want.flat[i]:.9e} got {got.flat[i]:.9e}")
        return ratio <= 1.0

    def check(self, cond, what):
        if not cond:
            self.bad.append(what)

    def done(self):
        assert not self.bad, f"{self.case}:\n" + "\n".join(self.bad)


class Buf:
    """A device tensor, sentinel-filled unless ``src``, with four guard elements behind it."""

    def __init__(self, shape, dtype=torch.float32, src=None):
        self.n = int(np.prod(shape))
        self.fill = SENT_BYTE if dtype == torch.uint8 else (-777 if dtype in (torch.int32, torch.int64) else SENT)
        self.whole = torch.full((self.n + 4,), self.fill, dtype=dtype, device=DEV)
        self.t = self.whole[:self.n].view(*shape)
        self.src = None if src is None else torch.as_tensor(np.asarray(src)).to(dtype).contiguous().to(DEV)
        self.reset()

    def reset(self):
        if self.src is not None:
            self.t.copy_(self.src.view(self.t.shape))
        else:
            self.t.fill_(self.fill)

    def guard_ok(self):
        return bool((self.whole[self.n:] == self.fill).all())

    def untouched(self):
        return bool((self.t == self.fill).all())


def _dev(a, dtype=torch.float32):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a)).to(dtype).contiguous().to(DEV)


def _snap(bufs):
    torch.cuda.synchronize()
    return [b.whole.clone() for b in bufs]


def _same(a, b):
    return all(torch.equal(x.view(torch.uint8), y.view(torch.uint8)) for x, y in zip(a, b))


def _bits(t):
    return t.detach().contiguous().view(torch.uint8).cpu()


def _twice(rep, bufs, launch):
    """Run ``launch`` on reset buffers twice; the results must be bitwise equal.  Returns the launch's value."""
    for b in bufs:
        b.reset()
    n = launch()
    first = _snap(bufs)
    for b in bufs:
        b.reset()
    n2 = launch()
    rep.check(n == n2 and _same(first, _snap(bufs)), "second identical launch differs")
    rep.check(all(b.guard_ok() for b in bufs), "a guard was overwritten")
    return n


def _ulp(want):
    return np.spacing(np.abs(np.asarray(want, np.float64)).astype(np.float32)).astype(np.float64)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _two_planes(rep, calls, bufs):
    """``calls[i]()`` writes ``bufs[i]``: record each, build one two-plane program, launch it once; each plane must hold
    the bits of its single launch."""
    lib = _lib.load()
    handles, single = [], []
    for i in range(2):
        for b in bufs[i]:
            b.reset()
        assert lib.raae_record_begin() == 0
        try:
            calls[i]()
        finally:
            h, n = C.c_void_p(), C.c_int(0)
            rc = lib.raae_record_end(C.byref(h), C.byref(n))
        assert rc == 0 and n.value >= 1, (rep.case, rc, n.value)
        handles.append(h)
        single.append(_snap(bufs[i]))
    prog = C.c_void_p()
    rc = lib.raae_multi_build((C.c_void_p * 2)(*[h.value for h in handles]), 2, C.byref(prog))
    for h in handles:
        lib.raae_record_free(h)
    assert rc == 0, (rep.case, "raae_multi_build", rc)
    try:
        for i in range(2):
            for b in bufs[i]:
                b.reset()
        assert lib.raae_multi_launch(prog, _stream()) == 0
        for i in range(2):
            rep.check(_same(single[i], _snap(bufs[i])), f"plane {i} differs from its single launch")
            rep.check(all(b.guard_ok() for b in bufs[i]), f"plane {i}: a guard was overwritten")
    finally:
        torch.cuda.synchronize()
        lib.raae_multi_free(prog)


# ========================================================================================================== rank loss
class RankDev:
    """Device side of a rank launch over rows ``[row0, row0 + nrows)`` of ``d [n_all, K]`` / ``z [n_all, K + 1]``:
    ``ldd = K + 2`` with NaN in the two padding columns (an over-read poisons the result), ``ldz = K + 1``."""

    def __init__(self, d, z, K, masked, nrows=None):
        B = len(d)
        self.B, self.K, self.masked, self.nrows = B, K, masked, B if nrows is None else nrows
        dd = np.full((B, K + 2), np.nan)
        dd[:, :K] = d
        self.d, self.z = _dev(dd), _dev(z)
        wb = (ops.rank_loss_masked_work_bytes if masked else ops.rank_loss_work_bytes)(self.nrows, K)
        self.work = Buf((wb,), torch.uint8)
        self.loss, self.dz = Buf((1,)), Buf((self.nrows, K + 1))
        self.totals = Buf((80 if masked else 64,), torch.float64)

    def whole(self, activate, dz=True):
        fn = ops.rank_loss_masked_fwd_bwd if self.masked else ops.rank_loss_fwd_bwd
        fn(self.d, self.K + 2, self.z, self.K + 1, self.B, self.K, activate, self.work.t, self.loss.t,
           self.dz.t if dz else None)

    def pairs(self, row0):
        fn = ops.rank_rows_masked_pairs if self.masked else ops.rank_rows_pairs
        fn(self.d, self.K + 2, self.z, self.K + 1, self.B, row0, self.nrows, self.K, self.work.t, self.totals.t)

    def finish(self, totals, activate, scale, dz=True):
        fn = ops.rank_rows_masked_finish if self.masked else ops.rank_rows_finish
        fn(totals, self.B, self.nrows, self.K, activate, scale, self.work.t, self.loss.t, self.dz.t if dz else None,
           self.K + 1)

    def route(self, rep, P=None):
        """The work buffer against the mirror: ``nwg`` RankWork records at offset 0, ``nj`` column blocks of g+-."""
        form = lr.rank_form(self.B, self.nrows, self.K, self.masked)
        w = self.work.t.cpu().numpy()
        rec = (w[:lr.RANK_PART_BYTES].reshape(lr.RANK_MAXWG, lr.RANK_WORK_RECORD) != SENT_BYTE).any(1)
        rep.check(int(rec.sum()) == form["nwg"] and bool(rec[:form["nwg"]].all()),
                  f"{int(rec.sum())} RankWork records written, the mirror gives nwg = {form['nwg']}")
        blk = self.nrows * self.K
        sent = np.frombuffer(bytes([SENT_BYTE] * 4), np.uint32)[0]
        for which in (0, 1):
            off = lr.RANK_PART_BYTES + which * lr.RANK_MAXNJ * blk * 4
            g = w[off:off + lr.RANK_MAXNJ * blk * 4].view(np.uint32).reshape(lr.RANK_MAXNJ, blk)
            full, none = (g != sent).all(1), (g == sent).all(1)
            rep.check(bool(full[:form["nj"]].all()) and bool(none[form["nj"]:].all()),
                      f"{'g-' if which else 'g+'}: blocks written {full.tolist()}, the mirror gives nj = {form['nj']}")
            if form["empty_block"]:
                rep.check(not g[form["nj"] - 1].view(np.float32).any(), "the empty last column block is not all zeros")
            if P is not None:
                tot = g[:form["nj"]].view(np.float32).astype(np.float64).sum(0).reshape(self.nrows, self.K)
                rep.check(np.array_equal(tot, P.gneg if which else P.gpos), f"{'g-' if which else 'g+'} differ from the reference's integers")
        if self.masked:
            off = lr.RANK_PART_BYTES + ((2 * lr.RANK_MAXNJ * blk * 4 + 255) & ~255)
            lab = (w[off:off + lr.RANK_MAXWG * 64].reshape(lr.RANK_MAXWG, 64) != SENT_BYTE).any(1)
            rep.check(int(lab.sum()) == form["nwg"], f"{int(lab.sum())} labelled-count records, nwg = {form['nwg']}")
        return form


def _check_rank(rep, dv, P, n_all, activate, totals, scale, masked, K):
    r = lr.rank_finish(totals, P, n_all, activate, masked, scale)
    rep.close("rank loss", f"loss act={int(activate)}", dv.loss.t, [r["loss"]], 1e-5 * abs(r["loss"]) + 1e-7)
    dz = dv.dz.t.cpu().double().numpy()
    rep.close("rank dz", f"dz act={int(activate)}", dz[:, :K], r["dz"],
              1e-5 * np.abs(r["dz"]) + lr.rank_dz_floor(P, r["c"], r["norm"], scale))
    rep.check(not dz[:, K].any(), "the extra column of dz is not 0")


def _run_rank_whole(c):
    rep = Report(c.name)
    d, z, P, _ = rank_ref(c.name)
    dv = RankDev(d, z, c.K, c.masked)
    bufs = [dv.work, dv.loss, dv.dz]
    for act in (False, True):
        _twice(rep, bufs, lambda: dv.whole(act))
        _check_rank(rep, dv, P, c.B, act, P.totals(c.masked), 1.0, c.masked, c.K)
        form = dv.route(rep, P)
        bits = _bits(dv.loss.t)
        dv.dz.reset()
        dv.whole(act, dz=False)
        rep.check(torch.equal(bits, _bits(dv.loss.t)), "the loss-only form gives other loss bits")
        rep.check(dv.dz.untouched(), "the loss-only form wrote dz")
    rep.done()
    return form


@pytest.mark.parametrize("name", [c.name for c in RANK_CASES])
def test_rank_loss(name):
    _run_rank_whole(RANK_BY_NAME[name])


def test_rank_empty_column_block():
    """1030 rows at n_aux = 1: the mirror gives nj = 4 column blocks of 512, so block 3 starts beyond the rows; its
    slice of g+- is written as zeros (``route``), not left stale."""
    for name in ("r4_1030_k1_u", "r4_1030_k1_m"):
        c = RANK_BY_NAME[name]
        form = lr.rank_form(c.B, c.B, c.K, c.masked)
        assert form["empty_block"] and form["nj"] == 4 and lr.rank_grid(c.B, c.B, c.K)[2] == 512


@pytest.mark.parametrize("name", [c.name for c in BIG_RANK_CASES])
def test_rank_loss_big(name):
    """R = 4 with nj = 1 (8192 rows), nj = 2 (8184) and the pair pass's grid stride (16392 rows: 2049 row groups).
    Descriptor column k is column 0 and style column k is column 0 times BIG_FACTORS[k] (exact products; negative
    factors swap n+ and n-), so the float64 reference is one column's pair pass."""
    c = RANK_BY_NAME[name]
    _, z, _, secs = rank_ref(name)
    assert np.array_equal(z[:, :c.K], (z[:, :1] / BIG_FACTORS[0]) * np.array(BIG_FACTORS[:c.K])[None, :]), "products not exact"
    t0 = time.perf_counter()
    form = _run_rank_whole(c)
    torch.cuda.synchronize()
    print(f"TIME {name}: reference {secs:.2f} s on the CPU, device part {time.perf_counter() - t0:.2f} s; form {form}")
    want = {"big_8192": (1, False), "big_8184": (2, False), "big_16392_u": (1, True), "big_16392_m": (1, True)}[name]
    assert (form["nj"], form["stride"]) == want and form["R"] == 4


@pytest.mark.parametrize("name", [c.name for c in ROWS_CASES])
def test_rank_rows(name):
    """The rows-against-all pair per emulated rank: counts exact, sums to the loss tolerance, one loss for all ranks
    after the totals are summed, dz with scale = the number of ranks, and the loss-only finish."""
    c = ROWS_BY_NAME[name]
    rep = Report(name)
    d, z = rank_data(name, c.n_all, c.K, c.masked, False)
    nr = len(c.split)
    row0s = np.concatenate([[0], np.cumsum(c.split)[:-1]])
    devs, Ps = [], []
    for row0, nrows in zip(row0s, c.split):
        dv = RankDev(d, z, c.K, c.masked, nrows)
        P = lr.rank_pairs(d, z[:, :c.K], c.masked, int(row0), nrows)
        _twice(rep, [dv.work, dv.totals], lambda: dv.pairs(int(row0)))
        form = dv.route(rep, P)
        rep.check((form["R"] == 4) == (nrows > 1024), f"R = {form['R']} at {nrows} rows")
        got = dv.totals.t.cpu().numpy().reshape(-1, 16)
        want = P.totals(c.masked)
        for row, what in ((0, "n+"), (1, "n-")) + (((4, "m"),) if c.masked else ()):
            rep.check(np.array_equal(got[row], want[row]), f"rank at row {row0}: {what} {got[row, :c.K]} != {want[row, :c.K]}")
        for row, what in ((2, "S+"), (3, "S-")):
            rep.close("rank sums", f"{what} rank at row {row0}", got[row], want[row], 1e-5 * np.abs(want[row]) + 1e-7)
        devs.append(dv)
        Ps.append(P)
    tot_ref = sum(P.totals(c.masked) for P in Ps)
    whole = lr.rank_pairs(d, z[:, :c.K], c.masked)
    assert np.array_equal(tot_ref[[0, 1] + ([4] if c.masked else [])], whole.totals(c.masked)[[0, 1] + ([4] if c.masked else [])])
    summed = torch.stack([dv.totals.t for dv in devs]).sum(0).contiguous()
    for act in (False, True):
        bits = []
        for dv, P in zip(devs, Ps):
            _twice(rep, [dv.loss, dv.dz], lambda: dv.finish(summed, act, float(nr)))
            _check_rank(rep, dv, P, c.n_all, act, tot_ref, float(nr), c.masked, c.K)
            b = _bits(dv.loss.t)
            dv.dz.reset()
            dv.finish(summed, act, float(nr), dz=False)
            rep.check(torch.equal(b, _bits(dv.loss.t)) and dv.dz.untouched(), "the loss-only finish differs or wrote dz")
            bits.append(b)
        rep.check(all(torch.equal(bits[0], b) for b in bits), "the ranks' losses differ in bits")
    rep.done()


@pytest.mark.parametrize("B", [33, 1027])
def test_rank_rows_single_split_is_the_whole_batch(B):
    """One rank that owns every row: ``raae_rank_rows_pairs`` + ``raae_rank_rows_finish`` (scale 1) and
    ``raae_rank_loss_fwd_bwd`` run one pair pass, one reduction of its records, one set of coefficients and one dz loop,
    and the counts pass through the totals exactly, so loss and dz have the same bits.  33 rows: one column block and
    fewer than 16 records; 1027 rows: R = 4, several column blocks, more than 16 records (the slice loop takes more than
    one trip)."""
    K = 5
    d, z = rank_data(f"one_{B}", B, K, False, False)
    form = lr.rank_form(B, B, K, False)
    assert (form["nwg"] > 16, form["nj"] > 1, form["R"]) == ((True, True, 4) if B == 1027 else (False, False, 1)), form
    whole, rows = RankDev(d, z, K, False), RankDev(d, z, K, False, B)
    for act in (False, True):
        whole.whole(act)
        rows.pairs(0)
        rows.finish(rows.totals.t, act, 1.0)
        torch.cuda.synchronize()
        assert torch.equal(_bits(whole.loss.t), _bits(rows.loss.t)), f"activate={act}: loss bits differ"
        assert torch.equal(_bits(whole.dz.t), _bits(rows.dz.t)), f"activate={act}: dz bits differ"
        assert all(b.guard_ok() for b in (rows.totals, rows.loss, rows.dz, rows.work))


# ============================================================================================ recon, smooth, MSE, BCE
def _loss_of(part, n, scale=1.0):
    out = torch.zeros(8, device=DEV)
    ops.loss_finalize(part, n, scale, out, 2)
    return out[2:3]


def _recon_tol(c, x, y, r):
    B, L = x.shape
    tol = 1e-4 * np.abs(r["dy"]) + 4 * U32 * (np.abs(y) + np.abs(x) * r["c"][:, None]) * 2.0 / (B * L)
    if c.scale:
        e_mean = (-(-L // 64) + 6) * U32
        ex = e_mean * np.abs(x).mean(1) / np.abs(r["mx"])
        ey = e_mean * np.abs(y).mean(1) / np.abs(r["my"])
        dr = r["r"] * (ex + ey + 3 * U32)
        gs = 0.2 * (r["r"] - 1.0) / (np.abs(r["mx"]) * L * B)
        tol = tol + (0.2 * dr / (np.abs(r["mx"]) * L * B) + 4 * U32 * np.abs(gs))[:, None]
    return tol


@pytest.mark.parametrize("c", RECON_CASES, ids=lambda c: c.name)
def test_recon_loss(c):
    rep = Report(c.name)
    x, y = recon_data(c)
    r = lr.recon_loss(x, y, c.scale)
    xd, yd = _dev(x), _dev(y)
    part, dy = Buf((MAXP,), torch.float64), Buf((c.B, c.L))
    n = _twice(rep, [part, dy], lambda: ops.recon_loss_fwd_bwd(xd, yd, c.B, c.L, c.scale, part.t, dy.t))
    rep.check(n == lr.recon_nparts(c.B), f"{n} partials, the mirror gives {lr.recon_nparts(c.B)}")
    rep.check(bool((part.t[n:] == SENT).all()), "partials beyond the count touched")
    rep.close("recon loss", "loss", _loss_of(part.t, n), [r["loss"]], 1e-5 * abs(r["loss"]))
    rep.close("recon dy", "dy", dy.t, r["dy"], _recon_tol(c, x, y, r))
    bits = _bits(part.t)
    part.reset()
    ops.recon_loss_fwd_bwd(xd, yd, c.B, c.L, c.scale, part.t, None)
    rep.check(torch.equal(bits, _bits(part.t)), "the loss-only form gives other partial bits")
    rep.done()


def _check_smooth(rep, c, x, taps, part, dx, n):
    """One finished launch (``n`` partials in ``part``, gradient in ``dx``) against the reference."""
    want_loss, want_dx = lr.smooth_loss(x, taps)
    rep.check(n == lr.smooth_nparts(c.B), f"{n} partials, the mirror gives {lr.smooth_nparts(c.B)}")
    rep.check(bool((part.t[n:] == SENT).all()), "partials beyond the count touched")
    kind = lr.smooth_instance(len(taps))
    if len(taps) == 1:
        rep.check(float(_loss_of(part.t, n)) == 0.0 and not dx.t.any(), "one tap: loss and dx are not exactly 0")
    rep.close(f"smooth loss {kind}", "loss", _loss_of(part.t, n), [want_loss], 2e-5 * abs(want_loss))
    rep.close(f"smooth dx {kind}", "dx", dx.t, want_dx,
              1e-4 * np.abs(want_dx) + (len(taps) + 2) * U32 * np.abs(x).max() * 2.0 / (c.B * c.L))
    rep.check(part.guard_ok() and dx.guard_ok(), "a guard was overwritten")


def _run_smooth(rep, c, x, taps):
    xd = _dev(x)
    part, dx = Buf((MAXP,), torch.float64), Buf((c.B, c.L))
    n = _twice(rep, [part, dx], lambda: ops.smooth_loss_fwd_bwd(xd, c.B, c.L, list(taps), part.t, dx.t))
    _check_smooth(rep, c, x, taps, part, dx, n)
    bits = _bits(part.t)
    part.reset()
    ops.smooth_loss_fwd_bwd(xd, c.B, c.L, list(taps), part.t, None)
    rep.check(torch.equal(bits, _bits(part.t)), "the loss-only form gives other partial bits")


@pytest.mark.parametrize("c", SMOOTH_CASES, ids=lambda c: c.name)
def test_smooth_loss(c):
    rep = Report(c.name)
    _run_smooth(rep, c, smooth_data(c), taps_of(c.taps))
    rep.done()


MSE_SIZES = (1, 255, 257, 512 * 1024 + 3)


@pytest.mark.parametrize("n", MSE_SIZES)
def test_mse(n):
    rep = Report(f"mse_{n}")
    g = _rng(f"mse{n}")
    a, b = f32(g.standard_normal(n)), f32(g.standard_normal(n))
    want_loss, want_da = lr.mse(a, b)
    ad, bd = _dev(a), _dev(b)
    part, da = Buf((MAXP,), torch.float64), Buf((n,))
    k = _twice(rep, [part, da], lambda: ops.mse_fwd_bwd(ad, bd, n, part.t, da.t))
    rep.check(k == lr.mse_nparts(n), f"{k} partials, the mirror gives {lr.mse_nparts(n)}")
    rep.check(bool((part.t[k:] == SENT).all()), "partials beyond the count touched")
    rep.close("mse loss", "loss", _loss_of(part.t, k), [want_loss], 1e-6 * abs(want_loss))
    rep.close("mse da", "da", da.t, want_da, 1e-5 * np.abs(want_da) + 1e-9)
    bits = _bits(part.t)
    part.reset()
    ops.mse_fwd_bwd(ad, bd, n, part.t, None)
    rep.check(torch.equal(bits, _bits(part.t)), "the loss-only form gives other partial bits")
    rep.done()


BCE_CASES = ((1, 1), (3, 1030), (256, 36))
BCE_EDGE = (0.0, 30.0, -30.0, 88.0, -88.0, 104.0, -104.0)


def bce_data(n_real, n_fake):
    """Logits of both halves: the edge values first (as many as fit), then 3 N(0, 1)."""
    g = _rng(f"bce{n_real}_{n_fake}")
    o = g.standard_normal(n_real + n_fake) * 3
    if n_real == 1:
        o[:] = (-104.0, 104.0)            # both terms 104: (104, -104) would make the loss 1.4e-45, below fp32
    else:
        o[:min(n_real, 7)] = BCE_EDGE[:min(n_real, 7)]
        o[n_real:n_real + min(n_fake, 7)] = BCE_EDGE[:min(n_fake, 7)]
    return f32(o)


@pytest.mark.parametrize("n_real,n_fake", BCE_CASES)
def test_bce_pair(n_real, n_fake):
    rep = Report(f"bce_{n_real}_{n_fake}")
    o = bce_data(n_real, n_fake)
    want_loss, want_d = lr.bce_pair(o, n_real)
    od = _dev(o)
    loss, d = Buf((1,)), Buf((n_real + n_fake,))
    _twice(rep, [loss, d], lambda: ops.bce_pair_fwd_bwd(od, n_real, n_fake, loss.t, d.t))
    rep.close("bce loss", "loss", loss.t, [want_loss], 1e-6 * abs(want_loss))
    rep.close("bce dlogits", "dlogits", d.t, want_d, 1e-5 * np.abs(want_d) + 1e-9)
    got = d.t.cpu().numpy()
    rep.check(bool(np.isfinite(got).all()), "a gradient is not finite")
    for i in np.flatnonzero(np.abs(o) >= 104.0):           # expf overflows: exactly 0 or +-1/n
        n = n_real if i < n_real else n_fake
        want = np.float32((0.0 if o[i] > 0 else -1.0) if i < n_real else (1.0 if o[i] > 0 else 0.0)) / np.float32(n)
        rep.check(got[i] == want, f"logit {o[i]} at {i}: gradient {got[i]!r}, exactly {want!r} expected")
    bits = _bits(loss.t)
    loss.reset()
    ops.bce_pair_fwd_bwd(od, n_real, n_fake, loss.t, None)
    rep.check(torch.equal(bits, _bits(loss.t)), "the loss-only form gives other loss bits")
    rep.done()


@pytest.mark.parametrize("n", (1, 256, 257, 512))
def test_loss_finalize(n):
    rep = Report(f"fin_{n}")
    g = _rng(f"fin{n}")
    p = g.standard_normal(n) * 10.0 ** g.integers(-3, 3, n)
    scale = 0.37
    part = _dev(p, torch.float64)
    out = Buf((8,), src=np.zeros(8))
    _twice(rep, [out], lambda: (ops.loss_finalize(part, n, scale, out.t, 3, 5), ops.loss_finalize(part, n, scale, out.t, 3, 5)) and None)
    want = lr.finalize(p, float(f32(scale)))
    got = out.t.cpu().double().numpy()
    rep.close("finalize", "slot", got[3:4], [want], _ulp(want))
    rep.check(got[5] == 2 * got[3], "the accumulating slot is not twice the value after two calls")
    rep.check(not got[[0, 1, 2, 4, 6, 7]].any(), "another slot was written")
    rep.done()


def test_in_kernel_finish():
    """``fin=``: the last workgroup adds the partials inside the loss kernel.  Same bits as the separate
    raae_loss_finalize launch, with and without an accumulating slot, three calls in a row; the ticket reads 0."""
    rep = Report("fin_in_kernel")
    g = _rng("fin_in_kernel")
    B, L = 1031, 70                                                    # ragged: 258 workgroups, the last one row short
    x, y = _dev(f32(g.random((B, L)) + 0.2)), _dev(f32(g.random((B, L)) + 0.2))
    part = Buf((MAXP,), torch.float64)
    ticket = torch.zeros(1, dtype=torch.int32, device=DEV)
    ref, got = Buf((8,), src=np.zeros(8)), Buf((8,), src=np.zeros(8))
    t17, t5 = list(taps_of("g17")), list(taps_of("asym5"))
    n_el = B * L - 5
    for it in range(3):
        for slot, acc, launch in (
                (0, -1, lambda fin: ops.recon_loss_fwd_bwd(x, y, B, L, True, part.t, None, fin=fin)),
                (1, 6, lambda fin: ops.smooth_loss_fwd_bwd(y, B, L, t17, part.t, None, fin=fin)),
                (2, -1, lambda fin: ops.smooth_loss_fwd_bwd(y, B, L, t5, part.t, None, fin=fin)),
                (3, 7, lambda fin: ops.mse_fwd_bwd(x, y, n_el, part.t, None, fin=fin)),
                (4, -1, lambda fin: ops.mse_fwd_bwd(x, y, n_el, part.t, None, fin=fin))):
            part.reset()
            n = launch(None)
            ops.loss_finalize(part.t, n, 0.5, ref.t, slot, acc)
            part.reset()
            launch((0.5, got.t, slot, acc, ticket))
            rep.check(int(ticket) == 0, f"slot {slot}: the ticket reads {int(ticket)}")
            rep.check(bool((part.t[n:] == SENT).all()), "partials beyond the count touched")
        rep.check(torch.equal(_bits(ref.t), _bits(got.t)), f"call {it}: {ref.t.tolist()} != {got.t.tolist()}")
    rep.check(ref.guard_ok() and got.guard_ok() and part.guard_ok(), "a guard was overwritten")
    rep.check(float(got.t[6]) > 2.5 * float(got.t[1]) > 0, "the accumulating slot did not accumulate")
    rep.done()


# =============================================================================================================== glue
DISC_INPUT_CASES = (("di_noise", 8, 5, 6, True), ("di_bare", 8, 5, 6, False), ("di_c1", 1, 1, 1, True),
                    ("di_stride", 9000, 7400, 16, True))             # 262400 elements > 1024 workgroups x 256


def disc_input_data(name, n_real, n_fake, Cc, noise, variant=0):
    g = _rng(f"{name}/{variant}")
    return (f32(g.standard_normal((n_real, Cc))), f32(g.standard_normal((n_fake, Cc))),
            f32(g.standard_normal((n_real + n_fake, Cc))) if noise else None)


@pytest.mark.parametrize("name,n_real,n_fake,Cc,noise", DISC_INPUT_CASES)
def test_disc_input(name, n_real, n_fake, Cc, noise):
    rep = Report(name)
    assert (name == "di_stride") == ((n_real + n_fake) * Cc > lr.GLUE_CAPS["disc_input"] * 256)
    zr, st, nz = disc_input_data(name, n_real, n_fake, Cc, noise)
    out = Buf((n_real + n_fake, Cc))
    a = (_dev(zr), _dev(st), _dev(nz))
    _twice(rep, [out], lambda: ops.disc_input(*a, SIGMA, n_real, n_fake, Cc, out.t))
    want = lr.disc_input(zr, st, nz, float(f32(SIGMA)))
    if noise:
        rep.close("glue", "out", out.t, want, _ulp(want))
    else:
        rep.check(np.array_equal(out.t.cpu().double().numpy(), want), "noise = NULL is not a bitwise copy")
    rep.done()


@pytest.mark.parametrize("n,sign", [(30, -1.0), (1, 1.0), (1024 * 256 + 77, -1.0)])
def test_scale_by_dev(n, sign):
    rep = Report(f"sc_{n}")
    g = _rng(f"sc{n}")
    src, s = f32(g.standard_normal(n)), f32(g.random(1) + 0.1)
    dst = Buf((n,))
    a = (_dev(src), _dev(s))
    _twice(rep, [dst], lambda: ops.scale_by_dev(a[0], a[1], sign, n, dst.t))
    want = sign * s[0] * src
    rep.close("glue", "dst", dst.t, want, _ulp(want))
    rep.done()


@pytest.mark.parametrize("name,B,L,n_aux,cursor,noise", [("ga_cursor", 16, 32, 5, 48, True), ("ga_null", 16, 32, 5, None, True),
                                                         ("ga_bare", 7, 3, 1, 7, False), ("ga_stride", 2050, 256, 3, None, True)])
def test_gather_batch(name, B, L, n_aux, cursor, noise):
    rep = Report(name)
    assert (name == "ga_stride") == (B * L > lr.GLUE_CAPS["gather_batch"] * 256)
    g = _rng(name)
    rows = 100
    spec, aux = f32(g.standard_normal((rows, L))), f32(g.standard_normal((rows, n_aux)))
    idx = g.integers(0, rows, size=max(B, cursor or 0) + 3)             # repeated indices
    idx[1] = idx[0]
    nz = f32(g.standard_normal((B, L))) if noise else None
    so, ao = Buf((B, L)), Buf((B, n_aux))
    cur = None if cursor is None else torch.tensor([cursor], dtype=torch.int32, device=DEV)
    a = (_dev(spec), _dev(aux), _dev(idx, torch.int64), cur, _dev(nz))
    _twice(rep, [so, ao], lambda: ops.gather_batch(*a, 0.02, B, L, n_aux, so.t, ao.t))
    take = idx[:B] if cursor is None else idx[cursor - B:cursor]
    rep.check(np.array_equal(ao.t.cpu().double().numpy(), aux[take]), "the aux copy is not bitwise")
    if noise:
        want = spec[take] + float(f32(0.02)) * nz
        rep.close("glue", "spec", so.t, want, _ulp(want))
    else:
        rep.check(np.array_equal(so.t.cpu().double().numpy(), spec[take]), "noise = NULL is not a bitwise copy")
    rep.done()


# =================================================================================================== style BatchNorm
def _style_bn(rows, count, rm, rv, update):
    prt = Buf((MAXP, rows.shape[1], 2), torch.float64)
    prt.t[:len(rows)] = _dev(rows, torch.float64)
    return prt, ops.make_bn(prt.t, len(rows), count, rm.t, rv.t, update_running=update)


@pytest.mark.parametrize("c", STYLE_FWD, ids=lambda c: c.name)
def test_style_bn_fwd(c):
    rep = Report(c.name)
    z, rows, run, _ = style_data(c.name, c.B, c.C, c.nparts)
    rm, rv = Buf((c.C,), src=run[0]), Buf((c.C,), src=run[1])
    update = c.mode == "train_u"
    if c.mode == "eval":
        bn = ops.make_bn(None, 0, 0, rm.t, rv.t)
        want, new = lr.style_bn_fwd(z, None, 0, run)
    else:
        prt, bn = _style_bn(rows, c.B, rm, rv, update)
        want, new = lr.style_bn_fwd(z, rows, c.B, run if update else None)
    zd, out = _dev(z), Buf((c.B, c.C))
    _twice(rep, [out, rm, rv], lambda: ops.style_bn_fwd(zd, c.B, c.C, bn, out.t))
    rep.close("style forward", "styles", out.t, want, 1e-5 * np.abs(want) + 1e-5)
    if update:
        rep.close("running", "running_mean", rm.t, new[0], 1e-4 * np.abs(new[0]) + 1e-6)
        rep.close("running", "running_var", rv.t, new[1], 1e-4 * np.abs(new[1]) + 1e-6)
    else:
        rep.check(torch.equal(rm.t, rm.src) and torch.equal(rv.t, rv.src), "the running statistics moved")
    rep.done()


@pytest.mark.parametrize("c", STYLE_BWD, ids=lambda c: c.name)
def test_style_bn_bwd(c):
    rep = Report(c.name)
    z, rows, run, dy = style_data(c.name, c.B, c.C, 3)
    _, rstd, _ = lr.bn_stats(rows, c.B)
    y = f32(lr.style_bn_fwd(z, rows, c.B)[0])
    rm, rv = Buf((c.C,), src=run[0]), Buf((c.C,), src=run[1])
    prt, bn = _style_bn(rows, c.B, rm, rv, False)
    dyd, yd, dz = _dev(dy), _dev(y), Buf((c.B, c.C))
    for scale in (1.0, 2.0):
        want = lr.style_bn_bwd(dy, y, rstd, scale)
        _twice(rep, [dz, rm, rv], lambda: ops.style_bn_bwd(dyd, yd, c.B, c.C, bn, dz.t, scale))
        rep.close("style dz", f"dz scale={scale}", dz.t, want, 1e-4 * np.abs(want) + 2e-5)
    rep.check(torch.equal(rm.t, rm.src) and torch.equal(rv.t, rv.src), "the running statistics moved")
    rep.done()


# ====================================================================================================== disc_fused
class DiscDev:
    def __init__(self, c, t):
        self.c = c
        class Obj:
            pass
        self.p = {k: _dev(t[k]) for k in DISC_PARAMS}
        self.layers = []
        for i, (w, b, s) in enumerate((("w1", "b1", "s1"), ("w2", "b2", "s2"), ("w3", "b3", None))):
            l = Obj()
            l.w, l.b, l.N = self.p[w], self.p[b], t[w].shape[0]
            l.prelu = Obj()
            l.prelu.weight = self.p[s] if s else None
            self.layers.append(l)
        self.offs, tot = {}, 0
        for k in DISC_PARAMS:
            self.offs[k] = tot
            tot += (t[k].size + 63) // 64 * 64
        self.stride = tot
        self.by_ptr = {self.p[k].data_ptr(): k for k in DISC_PARAMS}
        self.inp = [_dev(t[k]) for k in ("z_real", "styles", "noise", "m1", "m2")]
        self.alpha = _dev(f32([ALPHA]))
        self.slabs, self.dstyles = Buf((lr.DISC_MAXWG, tot)), Buf((c.n_fake, c.ns))
        self.partial, self.loss = Buf((lr.DISC_MAXWG,), torch.float64), Buf((1,))
        self.ticket = torch.zeros(1, dtype=torch.int32, device=DEV)
        self.bufs = [self.slabs, self.dstyles, self.partial, self.loss]

    def launch(self):
        c = self.c
        zr, st, nz, m1, m2 = self.inp
        return ops.disc_fused(zr, st, nz, SIGMA, m1, m2, self.layers, self.alpha, c.n_real, c.n_fake, c.ns,
                              lambda q: self.slabs.t[0, self.offs[self.by_ptr[q.data_ptr()]]:], self.stride,
                              self.dstyles.t, self.partial.t, self.ticket, self.loss.t)


def run_disc_fused(name, force=None):
    """One case against float64.  ``force``: the value of ``RAAE_DISC_MFMA`` the library was loaded under (None: unset),
    which the mirror follows; returns (instance, nslab)."""
    c = DISC_BY_NAME[name]
    rep = Report(name)
    t = disc_data(name)
    ref, near = t["ref"], t["near"]
    dv = DiscDev(c, t)
    nsl = _twice(rep, dv.bufs, dv.launch)
    inst, want_n = lr.disc_instance(c.n_real, c.n_fake, force)
    rep.check(nsl == want_n, f"nslab {nsl}, the mirror of the {inst} instance gives {want_n}")
    rep.check(int(dv.ticket) == 0, f"the ticket reads {int(dv.ticket)}")
    rep.check(bool((dv.slabs.t[nsl:] == SENT).all()), "slab rows beyond nslab touched")
    rep.check(bool((dv.partial.t[nsl:] == SENT).all()), "loss partials beyond nslab touched")
    rep.close(f"disc loss {inst}", "loss", dv.loss.t, [ref["loss"]], 1e-5 * abs(ref["loss"]) + 1e-6)
    n_near = int(near.sum())
    small = c.n_real + c.n_fake <= 63
    rep.check(n_near == 0 if small else n_near <= 0.01 * len(near), f"{n_near} near-zero rows of {len(near)}")
    near_fake = set(int(i) - c.n_real for i in np.flatnonzero(near) if i >= c.n_real)
    want = ref["dstyles"]
    got = dv.dstyles.t.cpu().double().numpy()
    err = np.abs(got - want)
    tol = 1e-7 + 2e-4 * float(np.abs(want).max()) + 2e-4 * np.abs(want)
    bad_rows = set(int(i) for i in np.unique(np.nonzero(err > tol)[0]))
    good = np.array([i not in near_fake for i in range(c.n_fake)])
    rep.close(f"disc grads {inst}", "dstyles (rows without a near-zero unit)", got[good], want[good], tol[good])
    rep.check(bad_rows <= near_fake, f"dstyles rows {sorted(bad_rows - near_fake)} miss without a near-zero unit")
    rep.check(all((err[r] <= 0.5 * np.abs(want).max()).all() for r in bad_rows), "an excused dstyles row is far off")
    slabs = dv.slabs.t[:nsl].cpu().double().numpy()
    for k in DISC_PARAMS:
        w = ref["d" + k].reshape(-1)
        g = slabs[:, dv.offs[k]:dv.offs[k] + w.size].sum(0)
        tol = 1e-7 + 2e-4 * float(np.abs(w).max()) + 2e-4 * np.abs(w)
        e = np.abs(g - w)
        n_bad = int((e > tol).sum())
        if n_near == 0:
            rep.close(f"disc grads {inst}", "d" + k, g, w, tol)
        else:
            print(f"CMP {name} d{k}: max err {e.max():.3e}, {float((e / tol).max()):.3f} of the bound, {n_bad} entries miss, "
                  f"{n_near} near-zero rows")
            rep.check(n_bad <= n_near * 130 and (n_bad == 0 or e.max() <= 0.05 * np.abs(w).max() + 1e-7),
                      f"d{k}: {n_bad} entries miss (max err {e.max():.3e}) with {n_near} near-zero rows")
    rep.done()
    return inst, nsl


@pytest.mark.parametrize("name", [c.name for c in DISC_CASES])
def test_disc_fused(name):
    run_disc_fused(name)


# ==================================================================================================== batched planes
def _plane_style(i):
    z, rows, run, dy = style_data(f"pl_style{i}", 37, 13, 3)
    rm, rv = Buf((13,), src=run[0]), Buf((13,), src=run[1])
    prt, bn = _style_bn(rows, 37, rm, rv, True)
    prt2, bn2 = _style_bn(rows, 37, rm, rv, False)
    zd, dyd, out, dz = _dev(z), _dev(dy), Buf((37, 13)), Buf((37, 13))
    yd = _dev(f32(lr.style_bn_fwd(z, rows, 37)[0]))
    keep = (prt, prt2, bn, bn2)

    def call():
        ops.style_bn_fwd(zd, 37, 13, bn, out.t)
        ops.style_bn_bwd(dyd, yd, 37, 13, bn2, dz.t, 2.0)
        return keep
    return call, [out, dz, rm, rv]


def _plane_rank(B, K, masked_rows):
    def make(i):
        name = f"pl_rank{B}_{K}_{int(masked_rows)}_{i}"
        d, z = rank_data(name, B, K, masked_rows, False)
        if masked_rows:                                  # the masked rows finish: rows [5, 5 + 20) of 37
            dv = RankDev(d, z, K, True, 20)
            dv.pairs(5)
            totals = dv.totals.t.clone()
            return (lambda: dv.finish(totals, True, 2.0)), [dv.loss, dv.dz]
        dv = RankDev(d, z, K, False)
        return (lambda: dv.whole(True)), [dv.work, dv.loss, dv.dz]
    return make


def _plane_recon(i):
    c = ReconCase(f"pl_recon{i}", 7, 65, True)
    x, y = recon_data(c)
    xd, yd, part, dy = _dev(x), _dev(y), Buf((MAXP,), torch.float64), Buf((7, 65))
    return (lambda: ops.recon_loss_fwd_bwd(xd, yd, 7, 65, True, part.t, dy.t)), [part, dy]


def _plane_smooth(kind):
    def make(i):
        c = SmoothCase(f"pl_smooth_{kind}{i}", 5, 70, kind)
        taps = list(taps_of(kind))
        xd, part, dx = _dev(smooth_data(c)), Buf((MAXP,), torch.float64), Buf((5, 70))
        return (lambda: ops.smooth_loss_fwd_bwd(xd, 5, 70, taps, part.t, dx.t)), [part, dx]
    return make


def _plane_mse(i):
    g = _rng(f"pl_mse{i}")
    a, b, part, da = _dev(f32(g.standard_normal(1500))), _dev(f32(g.standard_normal(1500))), Buf((MAXP,), torch.float64), Buf((1500,))
    return (lambda: ops.mse_fwd_bwd(a, b, 1500, part.t, da.t)), [part, da]


def _plane_bce(i):
    od, loss, d = _dev(f32(_rng(f"pl_bce{i}").standard_normal(40) * 3)), Buf((1,)), Buf((40,))
    return (lambda: ops.bce_pair_fwd_bwd(od, 17, 23, loss.t, d.t)), [loss, d]


def _plane_disc_input(i):
    zr, st, nz = disc_input_data("pl_di", 8, 5, 6, True, i)
    a, out = (_dev(zr), _dev(st), _dev(nz)), Buf((13, 6))
    return (lambda: ops.disc_input(*a, SIGMA, 8, 5, 6, out.t)), [out]


def _plane_disc(name):
    def make(i):
        dv = DiscDev(DISC_BY_NAME[name], disc_data(name, i))
        return dv.launch, dv.bufs
    return make


PLANES = {"pl_style_bn": _plane_style, "pl_rank_r1": _plane_rank(37, 5, False), "pl_rank_r4": _plane_rank(1030, 3, False),
          "pl_rank_rows_masked_finish": _plane_rank(37, 5, True), "pl_recon": _plane_recon,
          "pl_smooth_17": _plane_smooth("g17"), "pl_smooth_generic": _plane_smooth("asym5"), "pl_mse": _plane_mse,
          "pl_bce": _plane_bce, "pl_disc_input": _plane_disc_input, "pl_disc_valu": _plane_disc("dv_40_23_6"),
          "pl_disc_mfma": _plane_disc("dm_1000_1048_6")}


@pytest.mark.parametrize("name", list(PLANES))
def test_batched_planes(name):
    """Two calls on different inputs of one geometry, recorded and launched once as a two-plane program
    (``gridDim.z`` = 2): each plane has the bits of its single launch."""
    rep = Report(name)
    made = [PLANES[name](i) for i in range(2)]
    _two_planes(rep, [m[0] for m in made], [m[1] for m in made])
    rep.done()


# ================================================================================================= reporting, L = 4096
def test_zy_worst_ratios():
    """Prints the largest share of each bound over the cases this session ran (figures for DESIGN.md); asserts nothing
    the cases have not asserted already."""
    for k, v in sorted(WORST.items()):
        print(f"WORST {k}: {v:.4f} of its bound")


def test_zz_smooth_largest_row():
    """LAST, and launched exactly once: L = 4096 -- the argument check's limit -- needs 8 L floats = 128 KiB of dynamic
    LDS beside the kernel's static LDS, and the launch sets no attribute.  The one call either returns 0 and its
    outputs meet the reference, or returns non-zero and leaves every output at its sentinel (no repeat, no loss-only
    form here: ``sm17_L2048`` has those)."""
    rep = Report("sm17_L4096")
    c = SmoothCase("sm17_L4096", 4, 4096, "g17")
    info = (C.c_int(0), C.c_int(0))
    assert _lib.load().raae_device_info(C.byref(info[0]), C.byref(info[1]), None, 0) == 0
    print(f"device LDS limit {info[1].value} bytes; the launch needs {lr.smooth_lds_bytes(c.L)}")
    x, taps = smooth_data(c), taps_of(c.taps)
    xd, part, dx = _dev(x), Buf((MAXP,), torch.float64), Buf((c.B, c.L))
    arr = (C.c_float * len(taps))(*[float(t) for t in taps])
    n = C.c_int(-5)
    rc = _lib.load().raae_smooth_loss_fwd_bwd(C.c_void_p(xd.data_ptr()), c.B, c.L, arr, len(taps), C.c_void_p(part.t.data_ptr()),
                                             C.byref(n), C.c_void_p(dx.t.data_ptr()), None, _stream())
    torch.cuda.synchronize()
    if rc == 0:
        assert lr.smooth_lds_bytes(c.L) <= info[1].value, "launched beyond the device's LDS limit?"
        _check_smooth(rep, c, x, taps, part, dx, n.value)
    else:
        rep.check(part.untouched() and dx.untouched(), f"return code {rc} but an output was written")
        rep.check(lr.smooth_lds_bytes(c.L) > info[1].value, f"return code {rc} although the LDS fits")
        rep.check(rc == -1 and n.value == -5, f"refused by the runtime (code {rc}), not by the argument check")
    rep.done()
