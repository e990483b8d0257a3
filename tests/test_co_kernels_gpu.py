"""Every two-body launch of the conv networks (the 35 ``co_kernel<X, Y>`` rows of ``co_pair``, csrc/raae_conv.hip) and
the batched (``_m``) twins of the five fused block kernels, one launch at a time.

* BIT FOR BIT: the two bodies run alone through their own entry points; on fresh, identically filled buffers they run
  through ``ops.co_launch`` (``raae_co_launch``), ``ops.block_fwd_pair`` (``raae_block_fwd_a2`` / ``_b2``) or
  ``ops.block_bwd_b_launch`` (``raae_block_bwd_b_wgrad``).  Every tensor of BOTH sides -- outputs, partial rows, slabs,
  running statistics, the update's ``p, m, v, nan_step`` with their guards -- holds the bits of the single launches, the
  returned counts are the singles', and ``raae_co_instance`` and the recorder's launch count are what the mirror
  ``co_reference.instance`` says: one launch where it names a row, two where it names none.
* AGAINST FLOAT64: the co-launched outputs meet the references and tolerances of the sibling modules, none new:
  ``block_reference`` through the ``_check_*`` helpers of ``test_block_kernels_gpu.py`` (teacher-forced: every body
  reads the reference's tensors), ``step_reference`` through ``_check_update`` of ``test_step_kernels_gpu.py``,
  ``conv_reference`` for the head (2e-5 |ref| + 2e-5) and for the lone head-conv weight-gradient task (5e-4 |ref| +
  5e-5 mean|g| sqrt(B L)).  Those helpers also assert that rows beyond a returned count hold the sentinel.  The forward
  bodies run with ``update_running`` on: the running statistics move once, by the body's OWN workgroup 0.
* ENTRY ROWS AT 1027 ROWS run the plain bodies where the single entry points run BIG instances.  There bit equality
  with the singles is asserted only where neither single is a BIG instance (per the mirror); for the others the
  co-launch is held to float64 alone and the test prints whether the bits agree and the largest difference in units of
  the bound (``PLAINvBIG`` lines).  Nothing promises bit equality between a plain and a BIG instance.
* TWO PLANES: every row, and every ``KERNEL_m<KIND, BIG>`` twin of the block kernels that the default dispatch can
  select (the 18 twins behind the ``RAAE_BIG_MASK_*`` overrides: ``test_tuning_overrides_gpu.py``), as a two-plane program (``raae_multi_build`` of two recorded trials with other seeds, and for the update
  another hyper block and step count): each plane holds the bits of its own single (co-)launch.

FORM -> CASE (``test_co_reference_cpu.py`` recomputes it and fails on a gap)
  plain row i    p{i}@{37+40, 1023}: one launch; p{i}@1027: one launch for the four rows whose sides stay plain,
                 else two; cap_*: the update's grid capped at 4096 workgroups; head_{raw, softplus, relu}, head_unal,
                 head8
  entry row i    e{i}@{37+40, 256, 1027}; e18@4099, e22@4099: the y body loops over 513 sample groups on 512 workgroups
  tile_hint(4)   tile_* (five plain rows, one per x kind, two entry rows) at 256 rows
  graph replay   graph_* (one plain row per x kind)
  two planes     pl{i} for all 35 rows; blk_{kind}_{shape}@37 (plain twins), blk_{kind}_{shape}@1027 (BIG twins)
"""
import collections
import ctypes as C
import functools
import os
import time
import types

import pytest
import torch

import block_reference as br
import co_reference as co
import conv_reference as cr
import step_reference as sr
import test_block_kernels_gpu as blocks
import test_step_kernels_gpu as step

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from rankaae_amd import ops, _lib
    DEV = torch.device("cuda:0")

SENT, MAXP = blocks.SENT, blocks.MAXP
WIDE, CAPPED = 200, 17                          # max_nslab of the step module's "lanes8" / "stride_lanes8" layouts: both wide
WORST = collections.defaultdict(float)          # quantity class -> largest share of its bound over the session
MASK_ENV = ("FWD_A", "FWD_B", "BWD_B", "BWD_A", "WGRAD")
# kBigMask as the library was loaded: the default unless a child process of test_tuning_overrides_gpu.py, started with the
# RAAE_BIG_MASK_* overrides in its environment, says otherwise before it calls the runners below
MASK = [co.BIG_MASK]
PLAIN_V_BIG = []                                # (case, bits agree, largest difference in units of the bound)
SLOW = {}
T_START = [None]

# ======================================================================================================== case tables
Case = collections.namedtuple("Case", "name kind row x y rows via want opt")
X_KIND_ROWS = (3, 2, 14, 15, 17)                # one plain row per x kind: bwd_a, bwd_b + wgrad, wgrad, adam, fwd_a


def _via(i):
    if co.CO_ROWS[i][0] == "plain":
        return "co"
    return "pair" if co.CO_ROWS[i][1] in ("a", "b") else "bwdb"


def _case(name, kind, i, rows, x=None, y=None, **opt):
    sx, sy = co.row_sides(i, CAPPED if opt.get("cap") else WIDE)
    x, y = x or sx, y or sy
    if y[0] == "head" and opt.get("off"):
        y = y + (False,)
    via = _via(i)
    return Case(name, kind, i, x, y, rows, via, co.instance(x, y, rows, via != "co"), opt)


def _rows2(r):
    return (37, 40) if r == 37 else (r, r)      # at 37 rows the y side gets 40: the two grids differ


PLAIN = range(co.N_PLAIN)
# 1023: the last row count below the gate.  With 2 and 256 rows as well the module took longer on an MI355X than the block
# module (42.4 s against 40.4 s), so those two row counts of the plain rows were dropped, as agreed for that event; 256
# rows stay with the tile_* cases and the entry rows, 2 rows with the block module's own cases.
PLAIN_ROWS = (37, 1023)
ENTRY = range(co.N_PLAIN, len(co.CO_ROWS))
HEAD_ACTS = {"raw": cr.OUT_RAW, "softplus": cr.OUT_SOFTPLUS, "relu": cr.OUT_RELU}
VALUE_CASES = sorted(
    [_case(f"p{i}@{r}", "value", i, _rows2(r)) for i in PLAIN for r in PLAIN_ROWS + (1027,)] +
    [_case(f"e{i}@{r}", "value", i, _rows2(r)) for i in ENTRY for r in (37, 256, 1027)] +
    # 4099 rows of the 4 x 256 block are 513 sample groups on 512 workgroups (test_grid_cap_loops_over_groups of the block
    # module): only there does a forward body walk its groups with the workgroup count it was GIVEN
    [_case(f"e{i}@4099", "value", i, (4099, 4099), groups=True) for i in (18, 22)] +
    [_case("cap_bwd_a_adam", "value", 1, _rows2(37), cap=True), _case("cap_adam_fwd_b", "value", 15, _rows2(37), cap=True)] +
    [_case(f"head_{n}", "value", 17, _rows2(37), act=a) for n, a in HEAD_ACTS.items()] +
    [_case("head_unal", "value", 17, _rows2(37), act=cr.OUT_SOFTPLUS, off=1),
     _case("head8", "value", 17, _rows2(37), y=("head", 8), act=cr.OUT_RELU)],
    key=lambda c: (c.rows[0], c.name))            # by row count: the float64 references are shared through a small cache
TILE_CASES = [_case(f"tile_p{i}", "tile", i, (256, 256)) for i in X_KIND_ROWS] + \
             [_case(f"tile_e{i}", "tile", i, (256, 256)) for i in (20, 28)]
GRAPH_CASES = [_case(f"graph_p{i}", "graph", i, _rows2(37)) for i in X_KIND_ROWS]
PLANE_CASES = [_case(f"pl{i}", "planes", i, _rows2(37)) for i in range(len(co.CO_ROWS))]
# (kernel, shape, rows): the plain twin of every table shape and of one generic shape, the BIG twin wherever the default
# mask selects it
BLOCK_PLANE_CASES = [(k, n, 37) for k in co.FAMILY for n in list(br.TABLE_SHAPES) + ["gen_b"]] + \
                    [(k, n, 1027) for k in co.FAMILY for n in list(br.TABLE_SHAPES) + ["gen_c"] if co.use_big(1027, k, n)]
ALL_CASES = VALUE_CASES + TILE_CASES + GRAPH_CASES + PLANE_CASES


def _timed(name, t0):
    wall = time.perf_counter() - t0
    if wall > 1.0:
        SLOW[name] = wall


# =========================================================================================================== the sides
@functools.lru_cache(maxsize=12)
def _reference(name, rows, gy_bn, seed):
    """One float64 reference per (shape, rows, seed), shared by every row that uses it (``gy_bn`` follows the rows)."""
    return blocks._reference.__wrapped__(name, rows, gy_bn, True, seed)[5:]


class Rep(blocks.Report):
    """``Report`` that also keeps the largest share of each bound per quantity class."""

    def close(self, what, got, want, rtol, atol, arbiter=None):
        nbad = len(self.bad)
        super().close(what, got, want, rtol, atol, arbiter)
        g, w = got.detach().double().cpu(), want.detach().double().cpu()
        if len(self.bad) == nbad and bool(torch.isfinite(g).all()):
            cls = ("running statistics" if "running" in what else "forward sums" if what.startswith("stats") else
                   "backward sums" if what.startswith("pairs") else "parameter gradients" if what.startswith("d ") else
                   "data gradients" if what.startswith("d") else "forward tensors")
            s = float(((g - w).abs() / (atol + rtol * w.abs())).max())
            cls += " (through the fp32 arbiter)" if s > 1.0 else ""
            WORST[cls] = max(WORST[cls], s)


class BlockSide:
    """One of the five block kernels on one block, teacher-forced as ``run_teacher_forced`` forces it; with ``tasks``
    backward phase B beside the weight-gradient tasks of block ``tasks`` (RAAE_CO_BWD_B_WGRAD)."""

    def __init__(self, kind, name, rows, seed=0, tasks=None):
        self.kind, self.name, self.rows = kind, name, rows
        gy_bn = rows % 2 == 1
        self.r = r = blocks.Rig(name, rows, gy_bn=gy_bn, seed=seed, reference=False)
        r.f, r.b, r.g32 = _reference(name, rows, gy_bn, seed)
        self.nxt = BlockSide("wgrad", tasks, rows, seed) if tasks else None
        ex, sh = r.excit, r.short
        if kind != "a":
            r.force("T1", "E2", *(("Sh",) if sh else ()))
            r.force_stats("T1", *(("E2",) if ex else ()))
        if kind == "bwd_b":
            r.force("T2", "Y", *(("E3",) if ex else ()))
            if gy_bn:
                r.force_stats("Y", "G")
        if kind == "bwd_a":
            r.force("dBn2", "dSh", "E1", *(("dBnE",) if ex else ("dEx",)))
            r.force_stats("dBn2", *(("dBnE",) if ex else ()))
        if kind == "wgrad":
            r.force("E1", "dT2", "dT1", "dE1", "dEx", "dSh", *(("dE2",) if ex else ()))
        self.a = self.n = None

    def spec(self):
        return (self.kind, self.name) + ((self.nxt.name,) if self.nxt else ())

    def args(self):
        r = self.r
        if self.kind == "bwd_b":
            self.a = r.args_bwd_b(wgrad=self.nxt.args() if self.nxt else None)
        else:
            self.a = {"a": lambda: r.args_fwd_a(update=True), "b": lambda: r.args_fwd_b(update=True),
                      "bwd_a": r.args_bwd_a, "wgrad": r.args_wgrad}[self.kind]()
        return self.a

    def single(self):
        a = self.args()
        ret = {"a": ops.block_fwd_a, "b": ops.block_fwd_b, "bwd_a": ops.block_bwd_a_launch, "bwd_b": ops.block_bwd_b_launch,
               "wgrad": lambda a_: ops.block_wgrad(self.rows, None, None, self.r.stride, args=a_)}[self.kind](a)
        self.note(ret)
        return ret

    def note(self, ret):
        r, w, kind = self.r, self.r.w, self.kind
        if kind == "bwd_b" and self.nxt:
            ret, ns = ret
            self.nxt.note(ns)
        self.n = ret
        if kind == "a":
            w.nT1 = w.nE2 = ret
        elif kind == "b":
            w.nY = ret
        elif kind == "bwd_b":
            w.nB = ret
            for n in ["relu2"] + (["relu_short"] if r.short else []) + ["relu_excit_3" if r.excit else "relu_excit_2"]:
                r.nslab[n + ".weight"] = ret
        elif kind == "bwd_a":
            for n in ["relu1", "relu_excit_1"] + (["relu_excit_2"] if r.excit else []):
                r.nslab[n + ".weight"] = ret
        else:
            r.note_wgrad(self.a, ret)

    def tensors(self):
        r = self.r
        d = {n: v for n, v in vars(r.w).items() if torch.is_tensor(v)}
        d["slabs"] = r.slabs
        d.update({"buffer " + k: v for k, v in r.md.named_buffers()})
        if self.nxt:
            d.update({"tasks: " + k: v for k, v in self.nxt.tensors().items()})
        return d

    def check(self, rep):
        r = self.r
        if self.kind == "a":
            blocks._check_fwd_a(r, rep, r.f, True)
        elif self.kind == "b":
            blocks._check_fwd_b(r, rep, r.f, True)
        elif self.kind == "bwd_b":
            blocks._check_bwd_b(r, rep, r.b)
            if self.nxt:
                self.nxt.check(rep)
        elif self.kind == "bwd_a":
            blocks._check_bwd_a(r, rep, r.b, self.n)
        else:
            blocks._check_wgrad(r, rep, r.b)


class AdamSide:
    """An Adam (checked) / AdamW (plain) update of the 8-lane shape on the step module's data: NaN in every slab row at
    and beyond a segment's count, ``n`` = 384 (``cap``: 131072 + 64, the grid capped at 4096 workgroups) -- no size of
    the block side; plane 1 has another hyper block and step count."""
    kind = "adam"

    def __init__(self, chk, cap=False, seed=0, tag=""):
        self.rule = sr.ADAM if chk else sr.ADAMW
        lay = "stride_lanes8" if cap else "lanes8"
        self.c = step._ucase(f"co_{tag}_{lay}_{seed}", self.rule, lay, chk=chk)
        self.d = step.update_data(self.c.name, lay, self.c.kind, self.c.t)
        self.dev = step.UpdateDev(self.c, self.d, plane=seed)
        assert self.d.hint > co.WIDE_ABOVE and self.c.form[1] == "lanes8"
        assert (self.c.grid == sr.GRID_CAP and self.d.n > 32 * sr.GRID_CAP) if cap else self.c.grid < sr.GRID_CAP

    def spec(self):
        return ("adam", self.d.hint, self.c.chk)

    def args(self):
        v, d = self.dev, self.d
        self.a = types.SimpleNamespace(co_args=ops.adam_part_args(
            v.p.t, v.m.t, v.v.t, v.slabs, d.n, v.seg, d.n, self.rule, v.hyper, v.step, d.hint, v.nan.t if self.c.chk else None))
        return self.a

    def single(self):
        self.dev.launch()

    def note(self, ret):
        assert ret is None

    def tensors(self):
        return {"adam " + n: b.whole for n, b in zip(("p", "m", "v", "nan_step"), self.dev.bufs)}

    def check(self, rep):
        keep, step.WORST = step.WORST, WORST
        try:
            step._check_update(self.c, self.d, self.dev)
        finally:
            step.WORST = keep
        rep.check(all(b.guard_ok() for b in self.dev.bufs), "update: a guard was overwritten")
        rep.check(int(self.dev.nan.t[0]) == 0, "nan_step moved on finite gradients")


class HeadSide:
    """The decoder's head, Conv1d(C, 1, 1) on [rows, C, L] behind a train-mode BatchNorm, ``out`` ``off`` floats into
    its allocation with NaN around it."""
    kind = "head"

    def __init__(self, rows, Cc=4, act=0, off=0, seed=0):
        g = torch.Generator().manual_seed(500 + seed + rows)
        L = 256 if Cc == 4 else 64
        self.rows, self.Cc, self.L, self.act, self.off = rows, Cc, L, act, off
        self.X = cr.f32(torch.randn(rows, Cc, L, generator=g) * 1.3 + 0.2)
        self.w, self.b = cr.f32(torch.randn(1, Cc, 1, generator=g) * 0.5), cr.f32(torch.randn(1, generator=g) * 0.2)
        self.P, self.np_ = blocks._stat_rows(self.X)
        self.rm, self.rv = torch.zeros(Cc, device=DEV), torch.ones(Cc, device=DEV)
        self.whole = torch.full((rows * L + 8,), float("nan"), device=DEV)
        self.out = self.whole[off:off + rows * L].view(rows, 1, L)
        self.dX, self.dw, self.db = (t.float().to(DEV) for t in (self.X, self.w, self.b))
        self.view = ops.make_view(self.dX, None, ops.make_bn(self.P, self.np_, rows * L, self.rm, self.rv, 0.1, 1e-5, False))
        self.cv = ops.make_conv(Cc, L, 1, L, 1, 1, 0, 0, 1, 0)
        self.a = ops.conv_fwd_item(self.view, rows, self.cv, self.dw, self.db, self.out, act)

    def spec(self):
        return ("head", self.Cc) + ((False,) if self.off else ())

    def args(self):
        return self.a

    def single(self):
        self.a()

    def note(self, ret):
        assert ret is None

    def tensors(self):
        return {"head out": self.whole, "head running_mean": self.rm, "head running_var": self.rv}

    def check(self, rep):
        bn = dict(rows=self.P[:self.np_].cpu(), count=self.rows * self.L)
        ref = cr.layer_fwd(cr.Conv(self.Cc, self.L, 1, 1), self.X, self.w, self.b, bn=bn, act=self.act)
        rep.close("head out", self.out, ref["out"], 2e-5, 2e-5)
        n = self.rows * self.L
        rep.check(bool(torch.isnan(self.whole[:self.off]).all() and torch.isnan(self.whole[self.off + n:]).all()),
                  "head: written outside out")


class HeadTaskSide:
    """The weight-gradient task of the decoder's head conv alone: one conv task of no block shape (generic)."""
    kind, name, STRIDE = "wgrad", "head_task", 128

    def __init__(self, rows, seed=0):
        g = torch.Generator().manual_seed(900 + seed + rows)
        self.rows = rows
        self.X, self.G = cr.f32(torch.randn(rows, 4, 256, generator=g) * 1.3 + 0.2), cr.f32(torch.randn(rows, 1, 256, generator=g))
        self.P, self.np_ = blocks._stat_rows(self.X)
        self.rm, self.rv = torch.zeros(4, device=DEV), torch.ones(4, device=DEV)
        self.slabs = torch.full((MAXP, self.STRIDE), SENT, device=DEV)
        self.dX, self.dG = self.X.float().to(DEV), self.G.float().to(DEV)
        view = ops.make_view(self.dX, None, ops.make_bn(self.P, self.np_, rows * 256, self.rm, self.rv, 0.1, 1e-5, False))
        cv = ops.make_conv(4, 256, 1, 256, 1, 1, 0, 0, 1, 0)
        self.a = ops.block_wgrad_args(rows, [(ops.make_grad(self.dG), cv, view, self.slabs[0, 0:4], self.slabs[0, 64:65])],
                                      [], self.STRIDE)
        self.a.keep = (view, cv)
        self.ns = None

    def spec(self):
        return ("wgrad", "head_task")

    def args(self):
        return self.a

    def single(self):
        ret = ops.block_wgrad(self.rows, None, None, self.STRIDE, args=self.a)
        self.note(ret)
        return ret

    def note(self, ret):
        self.ns = list(ret)

    def tensors(self):
        return {"head task slabs": self.slabs}

    def check(self, rep):
        ns = self.ns[0]
        rep.check(len(self.ns) == 1 and 1 <= ns <= MAXP, f"head task: slab counts {self.ns}")
        v = cr.view(self.X, None, dict(rows=self.P[:self.np_].cpu(), count=self.rows * 256))[0]
        _, dw, db = cr.Conv(4, 256, 1, 1).bwd(v, torch.zeros(1, 4, 1, dtype=torch.float64), self.G)
        floor = 5e-5 * float(self.G.abs().mean()) * (self.rows * 256) ** 0.5
        s = self.slabs.cpu()
        rep.close("d head conv weight", s[:ns, 0:4].double().sum(0).view(1, 4, 1), dw, 5e-4, floor)
        rep.close("d head conv bias", s[:ns, 64:65].double().sum(0), db, 5e-4, floor)
        used = torch.zeros(self.STRIDE, dtype=torch.bool)
        used[0:4] = used[64:65] = True
        rep.check(bool((s[ns:] == SENT).all()) and bool((s[:ns][:, ~used] == SENT).all()), "head task: slabs outside dw / dbias written")


def make_side(spec, rows, seed=0, opt=None, tag=""):
    opt = opt or {}
    if spec[0] == "adam":
        return AdamSide(spec[2], opt.get("cap", False), seed, tag)
    if spec[0] == "head":
        return HeadSide(rows, spec[1], opt.get("act", cr.OUT_SOFTPLUS), opt.get("off", 0), seed)
    if spec == ("wgrad", "head_task"):
        return HeadTaskSide(rows, seed)
    return BlockSide(spec[0], spec[1], rows, seed, tasks=spec[2] if len(spec) == 3 else None)


def _snap(*sides):
    torch.cuda.synchronize()
    return [{k: v.clone() for k, v in s.tensors().items()} for s in sides]


def _restore(sides, snaps):
    for s, snap in zip(sides, snaps):
        for k, v in s.tensors().items():
            v.copy_(snap[k])


def _differ(a, b):
    """Names of the tensors that differ in bits (NaN equals NaN)."""
    assert a.keys() == b.keys()
    return [k for k in a if not bool(((a[k] == b[k]) | ((a[k] != a[k]) & (b[k] != b[k]))).all())]


def _pair(c, seed=0):
    tag = c.name.split("@")[0]
    return make_side(c.x, c.rows[0], seed, c.opt, tag), make_side(c.y, c.rows[1], seed, c.opt, tag)


def _together(c, X, Y):
    """The pair through the entry point the row belongs to; the sides take note of the counts.  Returns the counts."""
    if c.via == "co":
        rx, ry = ops.co_launch(X.kind, X.args(), Y.kind, Y.args())
    elif c.via == "pair":
        rx, ry = ops.block_fwd_pair(X.kind, X.args(), Y.args())
    else:
        X.a = X.r.args_bwd_b(wgrad=Y.args())
        rx, ry = ops.block_bwd_b_launch(X.a)
    X.note(rx)
    Y.note(ry)
    return rx, (list(ry) if isinstance(ry, (list, tuple)) else ry)


def _count(fn):
    """(launches ``fn()`` makes, None) through the recorder, or (None, the recorder's refusal) where a launch has no
    batched form (the per-layer conv kernels: a head that does not take the head kernel)."""
    lib = _lib.load()
    assert lib.raae_record_begin() == 0
    try:
        out = fn()
    finally:
        h, n = C.c_void_p(), C.c_int(0)
        rc = lib.raae_record_end(C.byref(h), C.byref(n))
    torch.cuda.synchronize()
    if rc == 0:
        lib.raae_record_free(h)
        return n.value, None, out
    buf = C.create_string_buffer(256)
    lib.raae_record_refusal(buf, 256)
    return None, buf.value.decode(), out


def _mask_is_the_environments():
    if MASK[0] == co.BIG_MASK:
        assert not [k for k in os.environ if k.startswith("RAAE_BIG_MASK_")], "RAAE_BIG_MASK_* overrides are set"
    env = tuple(int(os.environ.get("RAAE_BIG_MASK_" + n, str(d)), 0) for n, d in zip(MASK_ENV, co.BIG_MASK))
    assert env == tuple(MASK[0]), f"RAAE_BIG_MASK_* overrides {env}, the cases were built for {MASK[0]}"


def _mirror_holds(c, X, Y):
    """The case's sides are the mirror's, no tuning override moves the answers (in a child process of
    test_tuning_overrides_gpu.py: the overrides are exactly the mask the case was built with), and ``raae_co_instance``
    agrees."""
    _mask_is_the_environments()
    assert (X.spec(), Y.spec()) == (c.x, c.y), (X.spec(), Y.spec(), c.x, c.y)
    if c.via == "co":
        assert bool(ops.co_pairable(X.kind, X.args(), Y.kind, Y.args())) == (c.want is not None), \
            f"{c.name}: raae_co_instance disagrees with the mirror ({c.want})"


def _run_pair(c, check=True):
    """The singles, then the pair on fresh buffers: counts, launches, bits, sentinels, float64."""
    X1, Y1 = _pair(c)
    rx1, ry1 = X1.single(), Y1.single()
    alone = _snap(X1, Y1)
    X, Y = _pair(c)
    _mirror_holds(c, X, Y)
    n, refused, (rx, ry) = _count(lambda: _together(c, X, Y))
    want_n = 1 if c.want is not None else 2
    if refused is None:
        assert n == want_n, f"{c.name}: {n} launches, the mirror says {want_n} (row {c.want})"
    else:
        assert want_n == 2 and "conv_fwd" in refused, f"{c.name}: the recorder refused `{refused}`"
    norm = lambda v: list(v) if isinstance(v, (list, tuple)) else v
    assert (norm(rx), norm(ry)) == (norm(rx1), norm(ry1)), f"{c.name}: counts {(rx, ry)}, alone {(rx1, ry1)}"
    got = _snap(X, Y)
    rep = Rep(c.name)
    if check:
        X.check(rep)
        Y.check(rep)
    big = [co.single_is_big(s, r, MASK[0]) for s, r in zip((c.x, c.y), c.rows)]
    diff = [_differ(g, a) for g, a in zip(got, alone)]
    for i, what in enumerate("xy"):
        if c.want is None or not big[i]:
            rep.check(not diff[i], f"side {what} differs from its single launch: {diff[i]}")
    if c.want is not None and any(big):
        # plain bodies here, a BIG instance alone: float64 holds both (the checks above; the singles below); report the bits
        rep1 = Rep(c.name + " (singles)")
        X1.check(rep1)
        Y1.check(rep1)
        rep1.done()
        worst = 0.0
        for g, a, s, s1 in zip(got, alone, (X, Y), (X1, Y1)):
            for k, (rt, at) in _diff_bounds(s).items():
                if g.get(k) is not None:
                    d = (g[k].double() - a[k].double()).abs() / (at + rt * a[k].double().abs())
                    worst = max(worst, float(torch.nan_to_num(d, nan=0.0).max()))
            worst = max(worst, _param_diff(s, s1))
        PLAIN_V_BIG.append((c.name, not any(diff), worst))
        print(f"PLAINvBIG {c.name}: BIG alone {big}; bits {'agree' if not any(diff) else 'differ in ' + str(diff)}; "
              f"largest difference {worst:.3f} of the bound")
    rep.done()
    return X, Y


def _param_diff(s, s1):
    """Largest difference of a summed parameter gradient between two runs of a block side, in units of its bound."""
    if not isinstance(s, BlockSide):
        return 0.0
    worst = max([_param_diff(s.nxt, s1.nxt)] if s.nxt else [0.0])
    for key in s.r.nslab:
        if isinstance(key, str):
            a, b = s.r.grad_of(key).cpu(), s1.r.grad_of(key).cpu()
            worst = max(worst, float(((a - b).abs() / (s.r.tol_param(key, s.r.b) + 5e-4 * b.abs())).max()))
    return worst


def _diff_bounds(side):
    """Per tensor name, the (rtol, atol) of the module for element-wise quantities (forward 2e-5 + 2e-5, data gradients
    5e-4 + 5e-5): the unit in which a plain-versus-BIG difference is printed."""
    fwd = dict.fromkeys(("T1", "Sh", "E1", "E2", "T2", "E3", "Y"), (2e-5, 2e-5))
    bwd = dict.fromkeys(("dT2", "dSh", "dEx", "dBn2", "dBnE", "dT1", "dE2", "dE1", "dR"), (5e-4, 5e-5))
    kind = getattr(side, "kind", None)
    return fwd if kind in ("a", "b") else bwd if kind in ("bwd_a", "bwd_b") else {}


# ============================================================================================================== tests
@pytest.mark.parametrize("c", VALUE_CASES, ids=lambda c: c.name)
def test_pair_is_the_two_launches_and_meets_float64(c):
    """See the module docstring: mirror, launch count, returned counts, every tensor of both sides bit for bit, rows
    beyond the counts, and the float64 references."""
    t0 = time.perf_counter()
    T_START[0] = T_START[0] or t0
    X, Y = _run_pair(c)
    if c.opt.get("groups"):
        assert Y.n == MAXP and all(-(-4099 // S) != MAXP for S in range(1, 4100)), f"{c.name}: y returned {Y.n} rows, no group loop"
    _timed(c.name, t0)


@pytest.mark.parametrize("c", TILE_CASES, ids=lambda c: c.name)
def test_pair_under_tile_hint(c):
    """``raae_tile_hint(4)``: the pair is one launch and holds the bits of the singles under the same hint."""
    assert c.want is not None
    ops.tile_hint(4)
    try:
        _run_pair(c)
    finally:
        ops.tile_hint(1)


@pytest.mark.parametrize("c", GRAPH_CASES, ids=lambda c: c.name)
def test_pair_replayed_from_a_graph(c):
    """The co-launch captured with ``raae_graph_begin / _end`` and replayed twice on re-filled inputs holds the bits of
    the eager launch."""
    X, Y = _pair(c)
    stream = torch.cuda.Stream(device=DEV)
    stream.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(stream):
        pre = _snap(X, Y)
        _together(c, X, Y)
        eager = _snap(X, Y)
        _restore((X, Y), pre)
        g = ops.Graph()
        g.begin()
        try:
            _together(c, X, Y)
        finally:
            g.end()
        for i in range(2):
            _restore((X, Y), pre)
            g.launch()
            got = _snap(X, Y)
            assert not any(_differ(a, b) for a, b in zip(got, eager)), f"{c.name}: replay {i} differs from the eager launch"
    assert any(_differ(a, b) for a, b in zip(eager, pre)), "the launch wrote nothing"
    torch.cuda.current_stream(DEV).wait_stream(stream)


def _two_planes(name, build, launch):
    """``build(seed)`` -> sides, ``launch(sides)`` one launch: record each trial (it runs: its bits are the plane's
    expectation), restore its buffers, build ONE two-plane program, launch it once."""
    lib = _lib.load()
    trials, handles = [], []
    for seed in (0, 1):
        sides = build(seed)
        pre = _snap(*sides)
        assert lib.raae_record_begin() == 0
        try:
            launch(sides)
        finally:
            h, n = C.c_void_p(), C.c_int(0)
            rc = lib.raae_record_end(C.byref(h), C.byref(n))
        assert rc == 0 and n.value == 1, (name, rc, n.value)
        handles.append(h)
        single = _snap(*sides)
        assert any(_differ(a, b) for a, b in zip(single, pre)), "the launch wrote nothing"
        _restore(sides, pre)
        trials.append((sides, single))
    prog = C.c_void_p()
    rc = lib.raae_multi_build((C.c_void_p * 2)(*[h.value for h in handles]), 2, C.byref(prog))
    for h in handles:
        lib.raae_record_free(h)
    assert rc == 0, (name, "raae_multi_build", rc)
    try:
        assert lib.raae_multi_launch(prog, step._stream()) == 0
        for i, (sides, single) in enumerate(trials):
            diff = [_differ(a, b) for a, b in zip(_snap(*sides), single)]
            assert not any(diff), f"{name}: plane {i} differs from its single launch in {diff}"
    finally:
        torch.cuda.synchronize()
        lib.raae_multi_free(prog)
    a, b = trials[0][1], trials[1][1]
    assert any(not torch.equal(a[0][k], b[0][k]) for k in a[0]), "the two planes hold the same data"


@pytest.mark.parametrize("c", PLANE_CASES, ids=lambda c: c.name)
def test_pair_two_planes(c):
    """``co_kernel_m`` of every row: two trials with other seeds (the update: another hyper block and step count) in
    one launch, each plane bit for bit its own single co-launch."""
    assert c.want == c.row
    _two_planes(c.name, lambda seed: _pair(c, seed), lambda s: _together(c, *s))


@pytest.mark.parametrize("kind,name,rows", BLOCK_PLANE_CASES, ids=lambda v: str(v))
def test_block_kernel_two_planes(kind, name, rows):
    """``KERNEL_m<KIND, BIG>`` of the five block kernels alone: the plain twins at 37 rows, at 1027 rows every twin the
    default mask sends to BIG (the other BIG twins: ``test_tuning_overrides_gpu.py``)."""
    _mask_is_the_environments()
    _two_planes(f"blk_{kind}_{name}@{rows}", lambda seed: (BlockSide(kind, name, rows, seed),), lambda s: s[0].single())


# =========================================================================================================== refusals
def _record(fn):
    lib = _lib.load()
    assert lib.raae_record_begin() == 0
    try:
        fn()
    finally:
        h, n = C.c_void_p(), C.c_int(0)
        rc = lib.raae_record_end(C.byref(h), C.byref(n))
    assert rc == 0 and n.value == 1
    return h


@pytest.mark.parametrize("what,second", [("rows", ("a", "enc0", 40)), ("shape", ("a", "enc1", 37))])
def test_batching_refusals(what, second):
    """``raae_multi_build`` of a log of ``fwd_a`` enc0 at 37 rows with one at another row count, or with one of enc1:
    RAAE_EINVAL, and ``raae_record_refusal`` names the launch."""
    lib = _lib.load()
    sides = [BlockSide("a", "enc0", 37), BlockSide(*second)]
    handles = [_record(s.single) for s in sides]
    prog = C.c_void_p()
    rc = lib.raae_multi_build((C.c_void_p * 2)(*[h.value for h in handles]), 2, C.byref(prog))
    for h in handles:
        lib.raae_record_free(h)
    buf = C.create_string_buffer(256)
    n = lib.raae_record_refusal(buf, 256)
    print(f"REFUSAL {what}: rc {rc}, `{buf.value.decode()}`")
    assert rc == -1 and not prog.value, (rc, prog.value)
    assert n > 0 and "launch 0 of trial 1" in buf.value.decode(), buf.value


REJECTIONS = ["kind_x_range", "kind_y_range", "kind_x_negative", "head_as_x", "null_x", "null_y", "adam_n_mod_64", "adam_n_zero",
              "adam_rule", "adam_null_p", "bwd_b_null_nslab", "invalid_second_side"]


@pytest.mark.parametrize("what", REJECTIONS)
def test_argument_rejections(what):
    """``raae_co_launch`` and ``raae_co_instance`` return the invalid-argument code, nothing is launched (counted
    through the recorder) and every buffer keeps its bits.  ``invalid_second_side``: ``co_prep`` writes the first side's
    ``*nparts_x`` before the second side is checked, so after the refused call ``*nparts_x`` holds the first side's
    row count (not the value it had) and ``*nparts_y`` is untouched; ``raae_co_instance`` passes no count pointers and
    writes nothing.  That is pinned here as it stands."""
    lib = _lib.load()
    X, Y = BlockSide("bwd_a", "dec3", 37), AdamSide(True, tag="rej")
    if what == "bwd_b_null_nslab":
        X, Y = BlockSide("bwd_b", "dec2", 37, tasks="dec3"), BlockSide("a", "enc0", 40)
    kx, px, _, _, ns = ops._co_side(X.kind, X.args())
    ky, py, _, _, _ = ops._co_side(Y.kind, Y.args())
    ax, ay = C.cast(C.pointer(px), C.c_void_p), C.cast(C.pointer(py), C.c_void_p)
    first_written = False
    if what == "kind_x_range":
        kx = 7
    elif what == "kind_y_range":
        ky = 7
    elif what == "kind_x_negative":
        kx = -1
    elif what == "head_as_x":
        H = HeadSide(37)
        kx, hx, _, _, _ = ops._co_side("head", H.args())
        ax = C.cast(C.pointer(hx), C.c_void_p)
    elif what == "null_x":
        ax = None
    elif what == "null_y":
        ay, first_written = None, True
    elif what == "adam_n_mod_64":
        py.n = Y.d.n - 32
        first_written = True
    elif what == "adam_n_zero":
        py.n = 0
        first_written = True
    elif what == "adam_rule":
        py.rule = sr.RADAM
        first_written = True
    elif what == "adam_null_p":
        py.p = None
        first_written = True
    elif what == "bwd_b_null_nslab":
        px.nslab = None
    else:
        assert what == "invalid_second_side"
        py.max_nslab = -1
        first_written = True
    before = _snap(X, Y)
    n1, n2 = C.c_int(-5), C.c_int(-5)
    n, refused, rc = _count(lambda: lib.raae_co_launch(kx, ax, ky, ay, C.byref(n1), C.byref(n2), step._stream()))
    assert rc == -1, f"{what}: raae_co_launch returned {rc}"
    assert (n, refused) == (0, None), f"{what}: {n} launches, refusal {refused}"
    assert not any(_differ(a, b) for a, b in zip(_snap(X, Y), before)), f"{what}: a refused call wrote something"
    if what == "head_as_x":
        assert lib.raae_co_instance(kx, ax, ky, ay) in (0, 1), "raae_co_instance takes the head as x (it launches nothing)"
    else:
        assert lib.raae_co_instance(kx, ax, ky, ay) == -1, f"{what}: raae_co_instance"
    alone = BlockSide("bwd_a", "dec3", 37).single()
    assert n2.value == -5, f"{what}: *nparts_y written ({n2.value})"
    assert n1.value == (alone if first_written else -5), f"{what}: *nparts_x = {n1.value}"


# ============================================================================================================ summary
def test_zz_largest_share_of_each_bound():
    """Printed last: the largest share of each bound per quantity class, the plain-versus-BIG answers of the entry rows
    at 1027 rows, the module's wall time and the slowest tests."""
    for k in sorted(WORST):
        print(f"{k}: {WORST[k]:.3f}")
    for name, same, worst in PLAIN_V_BIG:
        print(f"plain v BIG {name}: bits {'agree' if same else 'differ'}, {worst:.3f} of the bound")
    if T_START[0]:
        print(f"wall time since the first value case: {time.perf_counter() - T_START[0]:.1f} s")
    for k, wall in sorted(SLOW.items(), key=lambda kv: -kv[1])[:3]:
        print(f"slow: {k} {wall:.1f} s")
    assert all(v <= 1.0 or "arbiter" in k for k, v in WORST.items())
