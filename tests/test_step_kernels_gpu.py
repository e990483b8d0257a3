"""Every kernel form of ``csrc/raae_optim.hip`` with ``raae_optim_body.inc`` -- the 32 update instances (4 rules x
{one thread per element, 8 lanes per element} x {plain, checked, clipped, checked + clipped}: ``update_body<RULE, WIDE,
CHK, SC>`` under ``update_kernel``, Adam and AdamW sharing a family) and their ``_m`` twins,
``raae_slab_reduce``, the Gaussian half of ``raae_rng_fill``, ``raae_step_tick`` and ``raae_step_begin`` -- against the
float64 / Python-integer reference of ``step_reference``, one launch at a time, teacher-forced.

* INPUTS are fp32 values; the reference computes on the same numbers in float64.  Every launch starts from fresh
  ``p, m, v``; every written buffer has four sentinel floats behind its count; a second launch from the same inputs
  must be bitwise the first.
* ROUTE: ``test_step_reference_cpu.py`` recomputes FORM -> CASE below from the dispatch mirror of ``step_reference``
  (``update_form``, ``rng_fill_grid``, ``step_begin_grid`` / ``step_begin_form``) and fails on a gap or on a case whose
  expected grid is not the mirror's.  The instance a case runs is its ``form`` field.
* NaN ROWS: slab rows at and beyond a segment's own count hold NaN (both shapes): a row of another segment that
  entered a sum would poison the result.
* TOLERANCES of the update kernels are the project's (``test_adam_matches_torch`` / ``test_optimizers_gpu.py``):
  2e-6 |ref| + 2e-7, for ``m`` and ``v`` in units of the segment's gradient scale (2e-7 s, 2e-7 s^2).  There is no fixed
  gradient floor; the fp32 slab sum adds a derived one: every term passes through at most ``d`` additions (``d = ns``
  for one thread per element; ``ceil(ns / 8) + 3`` with 8 lanes and the three-level shuffle tree), so the summed
  gradient is within ``e_g = d u sum|slab|`` (u = 2^-24) of the float64 sum, times the clip scale; the reference is
  evaluated at ``g +- e_g`` and the larger movement of each of ``p, m, v`` is added to its bound.
  ``raae_slab_reduce``: ``e_g`` itself.
* A GAUSSIAN VALUE is compared with the float64 evaluation from the kernel's own fp32 uniform and fp32 angle, relative
  to its radius ``r``: ``|got - ref| <= G ulp32(r)``.  No document of the HIP math library's error bounds (``logf``,
  ``sqrtf``, ``sinf``, ``cosf``) is installed, so by the issue's second rule ``G`` = four times the largest error, in
  ulps of ``r``, of numpy's own float32 evaluation of the same chain over the test's elements, and at least 4
  (``step_reference.gauss_f32_error_ulps``).  numpy measures 0.7 to 2.6 ulps over the layouts here, so ``G`` lies
  between 4 and 10.6; the kernels' largest error is 2.3 ulps of ``r``.  A wrong integer stream misses by O(1) =
  millions of ulps.  Noise multiply-add of ``step_begin``: one ulp of the largest of ``|row|``, ``|z s|`` and the
  result (the form may contract), plus ``G ulp32(r) s`` for noise generated in the kernel.
* EPS: at gradients of order 1 the bound on ``p`` cannot see ``eps`` = 1e-8.  The tiny_* cases run gradients and
  moments of scale 1e-8 (``sqrt(v)`` ~ 1e-8, the size of ``eps``; the test itself asserts that the reference without
  ``eps`` moves ``p`` by more than five bounds (10 to 60 measured), and ``(sqrt(v) + eps) / sqrt(bc2)`` for ``sqrt(v) / sqrt(bc2) + eps``
  moves it further still; AdaBound's step sits at its upper
  clamp at that scale, so for it the case pins the clamp, not eps), and zero_t1_* an all-zero gradient on all-zero
  moments: 0 / (0 + eps), ``p`` must come back bit for bit.
* NOT PINNED: the high word of the Philox block number ``qg`` (a slot of 2^34 floats); the 8-deep body of the thread
  shape beyond 16 slabs (unreachable: above 16 the 8-lane shape runs); which of the two kernel symbols of an instance
  ran is taken from the mirror, not read back from the device; the update riding in ``co_kernel`` is run here
  at the two table pairs with a backward phase A as host (beside a forward block, at the capped grid and as a
  two-plane program: ``test_co_kernels_gpu.py``).  Already held elsewhere and only
  cited here: a clip scale of exactly 1.0 is bitwise the plain instance and a fixed scale meets the rule
  (``test_grad_clip_gpu.py``); kinds 1 and 2 of the tape alone (``test_dense_kernels_gpu.py``).

FORM -> CASE
  update        (rule, shape, checked, clipped) -> u_{rule}_{thread|lanes8}_{p|c|s|cs}; grid stride gs_{rule}_{shape};
                steps t1_*, radam_t{5,6}_b{999,9999}, t100000_*, zero_*, zero_t1_*, tiny_*, decades_adabound (lr cut:
                base_lr != lr); the Adam half riding in co_kernel beside bwd_a of dec3 / enc2 at 37 rows: co_*
  slab_reduce   thread / lanes8 -> sr_thread / sr_lanes8
  rng_fill      floor grid f_one4 / f_six / f_gmg / f_total; capped grid f_big
  step_begin    (vector | scalar, generated | tape | none, nofill | lds | global) -> sb_*
"""
import collections
import ctypes as C
import functools
import time
import types
import zlib

import numpy as np
import pytest
import torch

import step_reference as sr

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    import test_block_kernels_gpu as blocks
    from rankaae_amd import ops, _lib
    DEV = torch.device("cuda:0")

SENT = -777.25
U = 2.0 ** -24
WORST = collections.defaultdict(float)       # quantity class -> largest share of its bound over the session
SLOW = {}                                    # test -> (wall seconds, CPU reference seconds), above one second


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


# ======================================================================================================= case tables
LAYOUTS = {                                   # name -> (slab counts per 64-element segment, slab rows, max_nslab hint)
    "thread": ([3, 0, 1, 8, 16], 16, 16),
    "lanes8": ([17, 0, 64, 65, 200, 1], 200, 200),
    "stride_thread": ([2] * ((1048576 + 64) // 64), 2, 2),
    "stride_lanes8": ([17] * ((131072 + 64) // 64), 17, 17),
    "decades": ([3] * 9, 4, 3),
}
UCase = collections.namedtuple("UCase", "name rule layout chk clip t betas wd kind form grid")
VARIANTS = {"p": (False, False), "c": (True, False), "s": (False, True), "cs": (True, True)}
CLIP_SCALE = 0.37


def _ucase(name, rule, layout, chk=False, clip=False, t=7, betas=(0.9, 0.999), wd=0.01, kind="normal"):
    counts, _, hint = LAYOUTS[layout]
    shape, grid = sr.update_form(64 * len(counts), hint)
    return UCase(name, rule, layout, chk, clip, t, betas, wd, kind, (rule, shape, chk, clip), grid)


RULES = (sr.ADAM, sr.ADAMW, sr.RADAM, sr.ADABOUND)
_RN = {r: sr.RULE_NAMES[r].lower() for r in RULES}
INSTANCE_CASES = [_ucase(f"u_{_RN[r]}_{lay}_{vn}", r, lay, chk, clip)
                  for r in RULES for lay in ("thread", "lanes8") for vn, (chk, clip) in VARIANTS.items()]
STRIDE_CASES = [_ucase(f"gs_{_RN[r]}_{lay[7:]}", r, lay) for r in RULES for lay in ("stride_thread", "stride_lanes8")]
STEP_CASES = ([_ucase(f"t1_{_RN[r]}", r, "thread", t=1) for r in RULES] +
              [_ucase(f"radam_t{t}_b{str(b2)[2:]}", sr.RADAM, "thread", t=t, betas=(0.99 if b2 == 0.9999 else 0.9, b2))
               for t in (5, 6) for b2 in (0.999, 0.9999)] +
              [_ucase(f"t100000_{_RN[r]}", r, lay, t=100000) for r, lay in zip(RULES, ("thread", "lanes8") * 2)] +
              [_ucase(f"zero_{_RN[r]}", r, "thread", kind="zero") for r in RULES] +
              [_ucase(f"zero_t1_{_RN[r]}", r, "thread", t=1, wd=0.0, kind="zero") for r in RULES] +
              [_ucase(f"tiny_{_RN[r]}", r, lay, wd=0.0, kind="tiny") for r, lay in zip(RULES, ("lanes8", "thread") * 2)] +
              [_ucase("decades_adabound", sr.ADABOUND, "decades", wd=0.0, kind="decades")])
UPDATE_CASES = INSTANCE_CASES + STRIDE_CASES + STEP_CASES

FCase = collections.namedtuple("FCase", "name segs total grid")      # segs: (offset, count, kind, numbering / hash offset, keep)
_BIG = 4194304 + 4096 + 8
FILL_CASES = [FCase(n, s, t, sr.rng_fill_grid(t)) for n, s, t in (
    ("f_one4", [(0, 4, 0, 0, 1.0)], 4),
    ("f_six", [(0, 6, 0, 0, 1.0)], 8),
    ("f_gmg", [(0, 40, 0, 0, 1.0), (40, 24, 1, 1000, 0.9), (64, 50, 0, 40, 1.0)], 114),
    ("f_total", [(0, 12, 0, 8, 1.0)], 10),
    ("f_big", [(0, _BIG, 0, 0, 1.0)], _BIG))]
FILL_STATES = [(1234, 0), (1234, 1), (1234, 2 ** 32 + 5), (0xABCDEF0123456789, 0), (0xABCDEF0123456789, 2 ** 32 + 5),
               (1234, None)]                                         # (seed, counter; None: counter = NULL)

SBCase = collections.namedtuple("SBCase", "name B L noise goff fill form grid")
_SEG3 = [(0, 40, 0, 4096, 1.0), (40, 24, 1, 1000, 0.9), (64, 16, 2, 77, 0.5)]
_SEG257 = [(4 * i, 4, i % 3, 8 * i, 0.8) for i in range(257)]
_SEGMID = [(0, 65 * 4096 * 4 - 4096, 0, 0, 1.0), (65 * 4096 * 4 - 4096, 4096, 1, 5, 0.9)]
SB_FILLS = {"none": ([], 0), "seg3": (_SEG3, 80), "seg257": (_SEG257, 4 * 257), "mid": (_SEGMID, 65 * 4096 * 4)}


def _sbcase(name, B, L, noise, goff, fill):
    segs, total = SB_FILLS[fill]
    return SBCase(name, B, L, noise, goff, fill, sr.step_begin_form(B, L, 0.0 if noise == "none" else 0.3, noise == "tape", len(segs)),
                  sr.step_begin_grid(B, L, total))


SB_CASES = [_sbcase(*a) for a in (
    ("sb_v8_gen0_nofill", 2, 8, "gen", 0, "none"), ("sb_v256_gen148_seg3", 37, 256, "gen", 148, "seg3"),
    ("sb_v8_gen148_seg257", 37, 8, "gen", 148, "seg257"),
    ("sb_s6_gen0_nofill", 37, 6, "gen", 0, "none"), ("sb_s7_gen148_seg257", 2, 7, "gen", 148, "seg257"),
    ("sb_s7_gen148_seg3", 37, 7, "gen", 148, "seg3"),
    ("sb_v8_tape_seg3", 37, 8, "tape", 0, "seg3"), ("sb_v256_tape_nofill", 2, 256, "tape", 0, "none"),
    ("sb_v8_tape_seg257", 2, 8, "tape", 0, "seg257"),
    ("sb_s7_tape_nofill", 37, 7, "tape", 0, "none"), ("sb_s6_tape_seg3", 2, 6, "tape", 0, "seg3"),
    ("sb_s6_tape_seg257", 37, 6, "tape", 0, "seg257"),
    ("sb_v256_none_nofill", 37, 256, "none", 0, "none"), ("sb_v8_none_seg3", 2, 8, "none", 0, "seg3"),
    ("sb_v8_none_seg257", 37, 8, "none", 0, "seg257"),
    ("sb_s6_none_nofill", 2, 6, "none", 0, "none"), ("sb_s7_none_seg3", 37, 7, "none", 0, "seg3"),
    ("sb_s7_none_seg257", 2, 7, "none", 0, "seg257"),
    ("sb_mid65", 2, 8, "gen", 0, "mid"))]
SB_CAP = _sbcase("sb_cap1024", 16400, 1024, "none", 0, "none")        # a pure gather past the 1024-workgroup cap

FORM_CASES = {
    "update": {c.name: c.form for c in UPDATE_CASES},
    "slab_reduce": {f"sr_{lay}": sr.update_form(64 * len(LAYOUTS[lay][0]), LAYOUTS[lay][2])[0] for lay in ("thread", "lanes8")},
    "rng_fill": {c.name: ("floor" if c.total // 4 <= 256 else "capped" if (c.total // 4 + 255) // 256 > sr.GRID_CAP else "mid")
                 for c in FILL_CASES},
    "step_begin": {c.name: c.form for c in SB_CASES + [SB_CAP]},
}


# ============================================================================================================ helpers
class Buf:
    """A device tensor of ``n`` elements with four guard elements behind it; ``reset`` restores the initial values."""

    def __init__(self, init, dtype=torch.float32, fill=None):
        if isinstance(init, int):
            init = np.full(init, SENT if fill is None else fill)
        self.init = torch.as_tensor(np.asarray(init)).to(dtype).reshape(-1)
        self.n = self.init.numel()
        self.guard = torch.full((4,), 77 if dtype in (torch.int32, torch.int64, torch.int16) else SENT).to(dtype)
        self.whole = torch.empty(self.n + 4, dtype=dtype, device=DEV)
        self.t = self.whole[:self.n]
        self.reset()

    def reset(self):
        self.whole.copy_(torch.cat([self.init, self.guard]))

    def guard_ok(self):
        return torch.equal(self.whole[self.n:].cpu(), self.guard)

    def np(self):
        return self.t.cpu().numpy()


def _bits(bufs):
    torch.cuda.synchronize()
    return [b.whole.clone().view(torch.uint8) for b in bufs]


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


def _twice(bufs, launch):
    for b in bufs:
        b.reset()
    launch()
    first = _bits(bufs)
    for b in bufs:
        b.reset()
    launch()
    assert _same(first, _bits(bufs)), "second identical launch differs"
    assert all(b.guard_ok() for b in bufs), "a guard was overwritten"
    return first


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _two_planes(calls, bufs):
    """``calls[i]()`` writes ``bufs[i]``: record each, build ONE two-plane program (the ``_m`` twin, gridDim.z = 2) and
    launch it once; each plane must hold the bits of its single launch."""
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
        assert rc == 0 and n.value == 1, (rc, n.value)
        handles.append(h)
        single.append(_bits(bufs[i]))
    prog = C.c_void_p()
    rc = lib.raae_multi_build((C.c_void_p * 2)(*[h.value for h in handles]), 2, C.byref(prog))
    for h in handles:
        lib.raae_record_free(h)
    assert rc == 0, ("raae_multi_build", rc)
    try:
        for i in range(2):
            for b in bufs[i]:
                b.reset()
        assert lib.raae_multi_launch(prog, _stream()) == 0
        for i in range(2):
            assert _same(single[i], _bits(bufs[i])), f"plane {i} differs from its single launch"
            assert all(b.guard_ok() for b in bufs[i]), f"plane {i}: a guard was overwritten"
    finally:
        torch.cuda.synchronize()
        lib.raae_multi_free(prog)


def _share(cls, err, tol):
    s = float((err / tol).max()) if np.size(err) else 0.0
    WORST[cls] = max(WORST[cls], s)
    return s


def _timed(name, t0, cpu):
    wall = time.perf_counter() - t0
    if wall > 1.0:
        SLOW[name] = (wall, cpu)


# ===================================================================================================== update kernels
def _hyper(c, plane=0):
    lr, base = (0.001, 0.01) if c.kind == "decades" else (0.01, 0.01)
    h = [lr, c.betas[0], c.betas[1], 1e-8, c.wd, base, 0.1, 1e-3]
    if plane == 1:                      # the second plane of the batched form: another hyper block
        h = [0.5 * lr, 0.8, 0.99, 1e-7, 0.5 * c.wd, base, 0.2, 2e-3]
    return h


@functools.lru_cache(maxsize=4)
def update_data(name, layout, kind, t):
    """fp32 inputs of a case: ``slabs`` [rows, n] (NaN at and beyond a segment's count), ``p0, m0, v0``, the
    per-element gradient scale ``gs`` and the depth ``d`` of the fp32 slab sum."""
    counts, rows, hint = LAYOUTS[layout]
    g = _rng(name)
    n = 64 * len(counts)
    seg_scale = 10.0 ** np.arange(-4, 5) if kind == "decades" else np.full(len(counts), 1e-8 if kind == "tiny" else 1.0)
    gs = np.repeat(seg_scale, 64)
    slabs = (g.standard_normal((rows, n)) * gs * (0.0 if kind == "zero" else 1.0)).astype(np.float32)
    cnt = np.repeat(np.asarray(counts), 64)
    slabs[np.arange(rows)[:, None] >= cnt[None, :]] = np.nan
    p0 = g.standard_normal(n).astype(np.float32)
    first = t == 1
    m0 = (0.0 if first else 0.1) * (g.standard_normal(n) * gs).astype(np.float32)
    v0 = (0.0 if first else 1.0) * (g.random(n) * gs * gs).astype(np.float32)
    shape = sr.update_form(n, hint)[0]
    depth = np.where(cnt > 0, cnt if shape == "thread" else -(-cnt // 8) + 3, 0).astype(np.float64)
    return types.SimpleNamespace(counts=counts, rows=rows, hint=hint, n=n, slabs=slabs, p0=p0, m0=m0, v0=v0, gs=gs,
                                 depth=depth, cnt=cnt)


class UpdateDev:
    def __init__(self, c, d, plane=0, slabs=None, counts=None):
        self.c, self.d = c, d
        self.p, self.m, self.v = Buf(d.p0), Buf(d.m0), Buf(d.v0)
        self.slabs = torch.from_numpy(d.slabs if slabs is None else slabs).to(DEV).contiguous()
        self.seg = torch.tensor(d.counts if counts is None else counts, dtype=torch.int16, device=DEV)
        self.t = c.t if plane == 0 else 3
        self.h = _hyper(c, plane)
        self.hyper = torch.tensor(self.h, dtype=torch.float64, device=DEV)
        self.step = torch.tensor([self.t], dtype=torch.int32, device=DEV)
        self.nan = Buf(np.zeros(1), torch.int32)
        self.scale = torch.tensor([CLIP_SCALE], device=DEV)
        self.bufs = [self.p, self.m, self.v, self.nan]

    def launch(self, chk=None, clip=None):
        c, d = self.c, self.d
        chk, clip = c.chk if chk is None else chk, c.clip if clip is None else clip
        a = (self.p.t, self.m.t, self.v.t, self.slabs, d.n, self.seg, d.n, c.rule, self.hyper, self.step)
        if clip:
            ops.optim_step_clip(*a, max_nslab=d.hint, nan_step=self.nan.t if chk else None, scale=self.scale)
        else:
            ops.optim_step(*a, max_nslab=d.hint, nan_step=self.nan.t if chk else None)


def _check_update(c, d, dev, info=None):
    """p, m, v of ``dev`` against the reference, each within its own bound; the shares go to WORST."""
    scale = CLIP_SCALE if c.clip else None
    g, has = sr.slab_sum(d.slabs, d.counts)
    eg = d.depth * U * sr.slab_abs_sum(d.slabs, d.counts)
    ref = sr.update(c.rule, d.p0, d.m0, d.v0, g, dev.h, dev.t, scale, info)
    moved = [sr.update(c.rule, d.p0, d.m0, d.v0, g + s * eg, dev.h, dev.t, scale) for s in (1.0, -1.0)]
    cls = f"{sr.RULE_NAMES[c.rule]} {c.form[1]}"
    for k, (what, buf, old, unit) in enumerate((("p", dev.p, d.p0, np.ones(d.n)), ("m", dev.m, d.m0, d.gs),
                                                ("v", dev.v, d.v0, d.gs ** 2))):
        got = buf.np().astype(np.float64)
        assert np.isfinite(got).all(), f"{c.name} {what}: not finite (a row at or beyond a segment's count entered a sum?)"
        want = np.where(has, ref[k], old.astype(np.float64))
        assert np.array_equal(got[~has], old[~has].astype(np.float64)), f"{c.name} {what}: a segment without slabs moved"
        tol = 2e-6 * np.abs(want) + 2e-7 * unit + np.maximum(np.abs(moved[0][k] - ref[k]), np.abs(moved[1][k] - ref[k]))
        err = np.abs(got - want)
        s = _share(f"update {what}: {cls}", err[has], tol[has])
        print(f"{c.name} {what}: largest share of the bound {s:.3f}")
        assert s <= 1.0, f"{c.name} {what}: {s:.3f} of the bound at {int((err / tol).argmax())}"
    return ref, has


@pytest.mark.parametrize("c", INSTANCE_CASES + STEP_CASES, ids=lambda c: c.name)
def test_update_instance(c):
    """One launch of the instance ``c.form`` against ``step_reference.update`` on p, m and v separately; a checked
    instance on finite gradients is bitwise its plain one and leaves ``nan_step`` 0."""
    d = update_data(c.name, c.layout, c.kind, c.t)
    dev = UpdateDev(c, d)
    first = _twice(dev.bufs, dev.launch)
    info = {}
    _, has = _check_update(c, d, dev, info)
    if c.chk:
        assert int(dev.nan.t[0]) == 0, "nan_step moved on finite gradients"
        plain = _twice(dev.bufs, lambda: dev.launch(chk=False))
        assert _same(first, plain), "checked instance differs from the plain one"
    if c.kind == "decades":
        lo, hi = int((info["lo"] & has).sum()), int((info["hi"] & has).sum())
        print(f"{c.name}: clamp hits lower {lo}, upper {hi}")
        assert lo >= 64 and hi >= 32, f"the clamp did not bind at both ends: {lo}, {hi}"
        assert dev.h[0] != dev.h[5], "the case runs behind an lr cut"
    if c.kind == "zero":
        assert not np.any(d.slabs[~np.isnan(d.slabs)]), "an all-zero gradient"
        if c.t == 1:
            assert not d.m0.any() and not d.v0.any() and np.array_equal(dev.p.np().view(np.uint32), d.p0.view(np.uint32)), \
                "0 / (0 + eps): p must come back bit for bit"
    if c.kind == "tiny" and c.rule != sr.ADABOUND:
        h0 = list(dev.h)
        h0[3] = 0.0
        g, has = sr.slab_sum(d.slabs, d.counts)
        moved = np.abs(sr.update(c.rule, d.p0, d.m0, d.v0, g, h0, dev.t)[0] - sr.update(c.rule, d.p0, d.m0, d.v0, g, dev.h, dev.t)[0])
        tolp = 2e-6 * np.abs(d.p0) + 2e-7
        assert np.median((moved / tolp)[has]) > 5, "eps does not matter in this case: it would not notice eps dropped"
    if c.rule == sr.RADAM and c.t in (5, 6):
        assert sr.radam_scalars(dev.h, c.t)[1] == (c.t == 6), "t = 6 is the first rectified step"


@pytest.mark.parametrize("c", STRIDE_CASES, ids=lambda c: c.name)
def test_update_grid_stride(c):
    """More elements than 4096 workgroups cover in one pass: the last segment is updated, the sentinel behind it is
    not."""
    t0 = time.perf_counter()
    assert c.grid == sr.GRID_CAP
    d = update_data(c.name, c.layout, c.kind, c.t)
    dev = UpdateDev(c, d)
    _twice(dev.bufs, dev.launch)
    t1 = time.perf_counter()
    _check_update(c, d, dev)
    cpu = time.perf_counter() - t1
    assert not np.array_equal(dev.p.np()[-64:], d.p0[-64:]), "the last segment was not updated"
    _timed(f"test_update_grid_stride[{c.name}]", t0, cpu)


@pytest.mark.parametrize("c", INSTANCE_CASES, ids=lambda c: c.name)
def test_update_two_planes(c):
    """The ``_m`` twin of every instance: two planes with different data, hyper blocks and step counts in one launch,
    each bitwise its single launch."""
    d = [update_data(c.name, c.layout, c.kind, c.t), update_data(c.name + "/plane1", c.layout, c.kind, c.t)]
    devs = [UpdateDev(c, d[i], plane=i) for i in range(2)]
    _two_planes([dv.launch for dv in devs], [dv.bufs for dv in devs])
    assert not torch.equal(devs[0].p.t, devs[1].p.t)


# ============================================================================================ Adam riding in co_kernel
CO_CASES = [("dec3", sr.ADAMW, False), ("dec3", sr.ADAM, True), ("enc2", sr.ADAM, False), ("enc2", sr.ADAMW, True)]


@pytest.mark.parametrize("host,rule,chk", CO_CASES, ids=[f"co_{h}_{_RN[r]}_{'c' if k else 'p'}" for h, r, k in CO_CASES])
def test_adam_riding_in_co_kernel_is_bitwise_the_update_alone(host, rule, chk):
    """``raae_co_launch`` of phase A of a block's backward pass (37 rows) with an Adam / AdamW update of the 8-lane
    shape (``ops.adam_part_args``, with and without ``nan_step``) is ONE launch, and ``p, m, v, nan_step`` hold the
    bits of ``raae_adam_step`` / ``raae_optim_step_chk`` alone from the same inputs (NaN rows included)."""
    c = _ucase(f"co_{host}_{_RN[rule]}", rule, "lanes8", chk=chk)
    d = update_data(c.name, c.layout, c.kind, c.t)
    dev = UpdateDev(c, d)
    alone = _twice(dev.bufs, dev.launch)
    _check_update(c, d, dev)
    for b in dev.bufs:
        b.reset()
    item = types.SimpleNamespace(co_args=ops.adam_part_args(dev.p.t, dev.m.t, dev.v.t, dev.slabs, d.n, dev.seg, d.n, rule,
                                                            dev.hyper, dev.step, d.hint, dev.nan.t if chk else None))
    rig = blocks._launched(host, 37, "fwd_a", "fwd_b", "bwd_b")
    ax = rig.args_bwd_a()
    assert ops.co_pairable("bwd_a", ax, "adam", item), "the pair has a row in the table"
    n = blocks._launches(lambda: ops.co_launch("bwd_a", ax, "adam", item))
    assert n == 1, f"{n} launches"
    assert _same(alone, _bits(dev.bufs)), "the update riding in co_kernel differs from the update alone"
    assert all(b.guard_ok() for b in dev.bufs) and int(dev.nan.t[0]) == 0


# ======================================================================================================= slab_reduce
@pytest.mark.parametrize("lay", ["thread", "lanes8"])
def test_slab_reduce(lay):
    """``out`` within the fp32 summation bound of the float64 sum, NaN rows behind every segment's count, a 0-slab
    segment gives 0; the ``_m`` twin is bitwise the single launches."""
    d = [update_data(f"sr_{lay}", lay, "normal", 7), update_data(f"sr_{lay}/plane1", lay, "normal", 7)]
    outs = [Buf(dd.n) for dd in d]
    slabs = [torch.from_numpy(dd.slabs).to(DEV) for dd in d]
    seg = torch.tensor(d[0].counts, dtype=torch.int16, device=DEV)
    calls = [functools.partial(ops.slab_reduce, slabs[i], d[i].n, seg, d[i].n, outs[i].t, d[i].hint) for i in range(2)]
    _twice([outs[0]], calls[0])
    got = outs[0].np().astype(np.float64)
    g, has = sr.slab_sum(d[0].slabs, d[0].counts)
    assert np.isfinite(got).all() and not got[~has].any(), "a 0-slab segment gives 0"
    tol = d[0].depth * U * sr.slab_abs_sum(d[0].slabs, d[0].counts)
    s = _share(f"slab_reduce {lay}", np.abs(got - g)[has], tol[has])
    print(f"sr_{lay}: largest share of the summation bound {s:.3f}")
    assert s <= 1.0
    _two_planes(calls, [[o] for o in outs])


@pytest.mark.parametrize("clip", [False, True], ids=["plain", "clipped"])
@pytest.mark.parametrize("lay", ["thread", "lanes8"])
@pytest.mark.parametrize("rule", RULES, ids=lambda r: _RN[r])
def test_reduced_gradient_as_one_slab_is_bitwise_the_slabs(rule, lay, clip):
    """What the clipping path rests on: ``raae_slab_reduce``'s flat gradient, read by the update as ONE slab through
    ``min(seg, 1)`` with the same slab hint, gives bit for bit the update from the slabs themselves."""
    c = _ucase(f"flat_{_RN[rule]}_{lay}", rule, lay, clip=clip)
    d = update_data(c.name, c.layout, c.kind, c.t)
    dev = UpdateDev(c, d)
    want = _twice(dev.bufs, dev.launch)
    flat = torch.full((1, d.n), float("nan"), device=DEV)
    ops.slab_reduce(dev.slabs, d.n, dev.seg, d.n, flat[0], d.hint)
    one = UpdateDev(c, d, slabs=flat.cpu().numpy(), counts=[min(x, 1) for x in d.counts])
    got = _twice(one.bufs, one.launch)
    assert _same(want, got), "the update from the reduced gradient differs from the update from the slabs"


# ==================================================================================================== rng_fill kind 0
@functools.lru_cache(maxsize=None)
def gauss_bound(segs, total, seed, ctr):
    """``G`` of the module docstring for the Gaussian slots of a layout: max(4, 4 x numpy's float32 error)."""
    worst = 0.0
    for off, cnt, kind, goff, _ in segs:
        if kind == 0:
            worst = max(worst, sr.gauss_f32_error_ulps(goff, max(0, min(cnt, total - off)), ctr, seed))
    return max(4.0, 4.0 * worst), worst


def _check_tape(name, got, ref, G, cls="rng_fill"):
    kind = ref["kind"]
    assert np.isfinite(got).all(), f"{name}: a value is NaN or infinite"
    free = kind == -1
    assert np.array_equal(got[free], np.full(int(free.sum()), np.float32(SENT))), f"{name}: a float no segment owns was written"
    mk = kind > 0
    assert np.array_equal(got[mk].view(np.uint32), ref["tape"][mk].astype(np.float32).view(np.uint32)), f"{name}: mask kinds"
    ga = kind == 0
    err = np.abs(got[ga].astype(np.float64) - ref["tape"][ga])
    s = _share(f"{cls} Gaussian, of G ulp(r)", err, G * sr.ulp32(ref["radius"][ga]))
    WORST[f"{cls} Gaussian, ulps of r"] = max(WORST[f"{cls} Gaussian, ulps of r"], s * G)
    assert s <= 1.0, f"{name}: a Gaussian value misses by {s * G:.1f} ulps of its radius (bound {G:.1f})"


def _desc(segs):
    desc = torch.tensor([[o, n, k, h] for o, n, k, h, _ in segs], dtype=torch.int32, device=DEV)
    return desc, torch.tensor([s[4] for s in segs], dtype=torch.float32, device=DEV)


FILL_RUNS = [(c, s) for c in FILL_CASES for s in (FILL_STATES if c.name != "f_big" else FILL_STATES[4:5])]


@pytest.mark.parametrize("c,state", FILL_RUNS, ids=lambda v: v.name if isinstance(v, FCase) else f"{v[0]:x}_{v[1]}")
def test_rng_fill_gaussian(c, state):
    """The whole tape against ``step_reference.fill``: Philox word order, Box-Muller pairing, the numbering of a second
    Gaussian segment, padding and a ragged ``total``; ``counter = NULL`` is counter 0."""
    seed, ctr = state                    # (the grid-stride layout runs once, with both high words set)
    t0 = time.perf_counter()
    desc, scale = _desc(c.segs)
    tape = Buf(c.total)
    cdev = None if ctr is None else torch.tensor([ctr], dtype=torch.int64, device=DEV)
    _twice([tape], lambda: ops.rng_fill(tape.t, desc, scale, len(c.segs), c.total, seed, cdev))
    t1 = time.perf_counter()
    ref = sr.fill([s[:4] for s in c.segs], [s[4] for s in c.segs], c.total, seed, ctr or 0, SENT)
    G, worst = gauss_bound(tuple(c.segs), c.total, seed, ctr or 0)
    cpu = time.perf_counter() - t1
    print(f"{c.name}: numpy float32 chain {worst:.2f} ulps of r, G = {G:.2f}")
    _check_tape(c.name, tape.np(), ref, G)
    _timed(f"test_rng_fill_gaussian[{c.name}]", t0, cpu)


# ========================================================================================================= step_tick
@pytest.mark.parametrize("n,mask,has_rng,has_cur", [(32, 0, True, True), (4, 0b0101, True, True), (32, 0xFFFFFFFF, True, True),
                                                    (0, 0b1, True, True), (4, 0b0101, False, True), (4, 0b0101, True, False)])
def test_step_tick(n, mask, has_rng, has_cur):
    seed, ctr0 = 0x1234567890ABCDEF, 2 ** 32 - 1
    steps = Buf(np.arange(32) * 3, torch.int32)
    state = Buf(np.array([ctr0, seed, 0], dtype=np.uint64).view(np.int64), torch.int64)
    cur = Buf(np.array([100]), torch.int32)
    _twice([steps, state, cur], lambda: ops.step_tick(steps.t, n, mask, state.t if has_rng else None,
                                                       cur.t if has_cur else None, 256))
    ref = sr.tick(list(range(0, 96, 3)), n, mask, ctr0 if has_rng else None, seed, 100 if has_cur else None, 256)
    assert steps.np().tolist() == ref["steps"]
    st = state.np().view(np.uint64)
    if has_rng:
        assert int(st[0]) == ref["ctr"] and int(st[1]) == seed
        assert tuple(int(x) for x in st[2:3].view(np.uint32)) == ref["keys"], "the stored keys are dense_reference.step_keys"
    else:
        assert st.tolist() == [ctr0, seed, 0]
    assert int(cur.t[0]) == (ref["cursor"] if has_cur else 100)


# ======================================================================================================== step_begin
NSRC, NAUX, CUR0, NOISE_S = 9, 3, 5, 0.3


@functools.lru_cache(maxsize=4)
def sb_data(name, B, L, with_noise):
    g = _rng(name)
    spec = g.standard_normal((NSRC, L)).astype(np.float32)
    aux = g.standard_normal((NSRC, NAUX)).astype(np.float32)
    idx = g.integers(0, NSRC, size=CUR0 + 2 * B).astype(np.int64)
    noise = g.standard_normal(B * L).astype(np.float32) if with_noise else None
    return spec, aux, idx, noise


class StepBeginDev:
    NSTEPS, MASK = 5, 0b10110

    def __init__(self, c, seed=0x9E3779B97F4A7C15, ctr0=2 ** 32 - 1):
        self.c, self.seed, self.ctr0 = c, seed, ctr0
        spec, aux, idx, noise = self.data = sb_data(c.name, c.B, c.L, c.noise == "tape")
        self.spec, self.aux, self.idx = (torch.from_numpy(a).to(DEV) for a in (spec, aux, idx))
        self.noise = torch.from_numpy(noise).to(DEV) if c.noise == "tape" else None
        self.steps = Buf(np.array([7, 0, 3, 9, 11, 13]), torch.int32)                 # the sixth is beyond nsteps
        self.state = Buf(np.array([ctr0, seed, 0], dtype=np.uint64).view(np.int64), torch.int64)
        self.cursor, self.ticket = Buf(np.array([CUR0]), torch.int32), Buf(np.array([0]), torch.int32)
        self.spec_out, self.aux_out = Buf(c.B * c.L), Buf(c.B * NAUX)
        segs, total = SB_FILLS[c.fill]
        self.segs, self.total = segs, total
        self.tape = Buf(max(total, 1))
        self.fill = None
        if segs:
            desc, scale = _desc(segs)
            self.fill = types.SimpleNamespace(buf=self.tape.t, seg_desc=desc, seg_scale=scale, segs=segs, total=total)
        self.bufs = [self.steps, self.state, self.cursor, self.ticket, self.spec_out, self.aux_out, self.tape]
        self.sn = 0.0 if c.noise == "none" else NOISE_S

    def launch(self):
        c = self.c
        ops.step_begin(self.steps.t, self.NSTEPS, self.MASK, self.state.t, self.cursor.t, c.B, self.ticket.t, self.spec,
                       self.aux, self.idx, c.B, c.L, NAUX, self.sn, self.noise, c.goff, self.spec_out.t, self.aux_out.t,
                       tape=self.fill)

    def reference(self, steps, ctr, cursor):
        spec, aux, idx, noise = self.data
        fa = ([s[:4] for s in self.segs], [s[4] for s in self.segs], self.total, SENT) if self.segs else None
        return sr.step_begin(steps, self.NSTEPS, self.MASK, ctr, self.seed, cursor, self.c.B, spec, aux, idx, self.c.B,
                             self.sn, noise if self.c.noise == "tape" else None, self.c.goff, fa)

    def check(self, ref, what):
        c = self.c
        assert self.steps.np().tolist() == ref["steps"], what
        st = self.state.np().view(np.uint64)
        assert (int(st[0]), int(st[1])) == (ref["ctr"], self.seed), what
        assert tuple(int(x) for x in st[2:3].view(np.uint32)) == ref["keys"], what
        assert int(self.cursor.t[0]) == ref["cursor"] and int(self.ticket.t[0]) == 0, what
        assert np.array_equal(self.aux_out.np().view(np.uint32), ref["aux_out"].reshape(-1).view(np.uint32)), f"{what}: aux_out"
        got = self.spec_out.np()
        G = 0.0
        if c.noise == "none":
            assert np.array_equal(got.view(np.uint32), ref["rows"].reshape(-1).view(np.uint32)), f"{what}: spec_out"
        else:
            want, rows, z = ref["spec_out"].reshape(-1), ref["rows"].reshape(-1).astype(np.float64), ref["z"].reshape(-1)
            tol = sr.ulp32(np.maximum(np.maximum(np.abs(rows), np.abs(z * self.sn)), np.abs(want)))
            if c.noise == "gen":
                G = gauss_bound(((0, c.B * c.L, 0, c.goff, 1.0),), c.B * c.L, self.seed, ref["ctr"])[0]
                tol = tol + G * sr.ulp32(ref["radius"].reshape(-1)) * self.sn
            s = _share(f"step_begin noise ({c.noise})", np.abs(got.astype(np.float64) - want), tol)
            assert np.isfinite(got).all() and s <= 1.0, f"{what}: spec_out {s:.3f} of the bound"
        if self.segs:
            Gt = gauss_bound(tuple(self.segs), self.total, self.seed, ref["ctr"])[0]
            _check_tape(what, self.tape.np()[:self.total], ref["tape"], Gt, cls="step_begin fill")
        else:
            assert float(self.tape.t[0]) == SENT


@pytest.mark.parametrize("c", SB_CASES, ids=lambda c: c.name)
def test_step_begin(c):
    """One launch from the state of the previous step against ``step_reference.step_begin``; a second launch WITHOUT a
    reset gives the state of step 2, not a repeat of step 1."""
    t0 = time.perf_counter()
    dev = StepBeginDev(c)
    _twice(dev.bufs, dev.launch)
    t1 = time.perf_counter()
    ref = dev.reference([7, 0, 3, 9, 11, 13], dev.ctr0, CUR0)
    dev.check(ref, f"{c.name} step 1")
    dev.launch()
    torch.cuda.synchronize()
    ref2 = dev.reference(ref["steps"], ref["ctr"], ref["cursor"])
    dev.check(ref2, f"{c.name} step 2")
    assert ref2["ctr"] == 2 ** 32 + 1 and all(b.guard_ok() for b in dev.bufs)
    _timed(f"test_step_begin[{c.name}]", t0, time.perf_counter() - t1)


def test_step_begin_gather_at_the_grid_cap():
    """A pure gather past 1024 workgroups (a few source rows indexed repeatedly), compared on the device."""
    c = SB_CAP
    assert c.grid == 1024 and c.B * c.L // 4 > 1024 * 4096
    dev = StepBeginDev(c)
    dev.launch()
    rows = dev.idx[CUR0:CUR0 + c.B]
    assert torch.equal(dev.spec_out.t.view(c.B, c.L), dev.spec[rows]) and torch.equal(dev.aux_out.t.view(c.B, NAUX), dev.aux[rows])
    assert all(b.guard_ok() for b in dev.bufs) and int(dev.cursor.t[0]) == CUR0 + c.B and int(dev.ticket.t[0]) == 0


def test_step_begin_two_planes():
    c = next(x for x in SB_CASES if x.name == "sb_v256_gen148_seg3")
    devs = [StepBeginDev(c, seed=0x9E3779B97F4A7C15), StepBeginDev(c, seed=77)]
    _two_planes([d.launch for d in devs], [d.bufs for d in devs])
    assert not torch.equal(devs[0].spec_out.t, devs[1].spec_out.t)


@pytest.mark.parametrize("what", ["null_steps", "null_rng", "null_cursor", "null_ticket", "null_spec", "null_aux", "null_idx",
                                  "null_spec_out", "null_aux_out", "nsteps33", "goff2", "goff_negative", "fill_without_tape"])
def test_step_begin_rejections(what):
    """Host-side argument checks: the invalid-argument code, nothing launched, every buffer still at its initial
    values."""
    dev = StepBeginDev(next(x for x in SB_CASES if x.name == "sb_v8_tape_seg3"))
    a = _lib.StepBeginT()
    p = lambda t: t.data_ptr()
    a.steps, a.nsteps, a.step_mask, a.rng_state = p(dev.steps.t), 5, 0b10110, p(dev.state.t)
    a.cursor, a.stride, a.ticket = p(dev.cursor.t), 37, p(dev.ticket.t)
    a.spec, a.aux, a.idx, a.B, a.L, a.n_aux = p(dev.spec), p(dev.aux), p(dev.idx), 37, 8, NAUX
    a.spec_noise, a.noise_tape, a.noise_goff = 0.3, p(dev.noise), 0
    a.spec_out, a.aux_out = p(dev.spec_out.t), p(dev.aux_out.t)
    a.tape, a.seg_desc, a.seg_scale, a.nseg, a.total = p(dev.fill.buf), p(dev.fill.seg_desc), p(dev.fill.seg_scale), 3, 80
    if what.startswith("null_"):
        setattr(a, {"rng": "rng_state"}.get(what[5:], what[5:]), None)
    elif what == "nsteps33":
        a.nsteps = 33
    elif what == "goff2":
        a.noise_goff = 2
    elif what == "goff_negative":
        a.noise_goff = -4
    else:
        a.tape = None
    before = _bits(dev.bufs)
    rc = _lib.load().raae_step_begin(C.byref(a), _stream())
    assert rc == -1, f"{what}: not RAAE_EINVAL ({rc})"
    assert _same(before, _bits(dev.bufs)), f"{what}: something was written"


# =========================================================================================================== summary
def test_zz_largest_share_of_each_bound():
    """Printed last: the largest share of each bound per class, and every test above one second with the CPU
    (reference) share of its time."""
    for k in sorted(WORST):
        print(f"{k}: {WORST[k]:.3f}")
    for k, (wall, cpu) in sorted(SLOW.items()):
        print(f"slow: {k} {wall:.1f} s, of which {cpu:.1f} s CPU reference")
    assert all(v <= 1.0 or "ulps of r" in k for k, v in WORST.items())
