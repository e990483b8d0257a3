"""Every kernel form of the per-layer conv-network entry points -- ``raae_conv_fwd``, ``raae_conv_bwd_data``,
``raae_conv_bwd_weight``, ``raae_lenlin_fwd``, ``raae_lenlin_bwd_data``, ``raae_lenlin_bwd_weight``, ``raae_sum3_fwd``,
``raae_grad_materialize``, ``raae_head_bwd`` (``csrc/raae_conv.hip``, ``raae_conv_tiled.inc``, ``raae_conv_strip.inc``,
``raae_head.inc``) -- against the float64 reference of ``conv_reference``, one launch at a time.

* TEACHER-FORCED: a kernel receives the reference's tensors rounded to fp32 and float64 partial rows.  The raw tensor
  behind a PReLU / softplus / ReLU derivative is the reference's own (rounded), and the reference differentiates at that
  rounded tensor: no branch can differ and no entry is excused.
* ROUTE: every case names the form it expects per entry point (``forms``: forward, data gradient, weight gradient);
  ``test_conv_reference_cpu.py`` holds the table to the mirrored dispatch of ``conv_reference``, and here the row /
  slab count the library returns must equal the mirror's.  The module is skipped when a ``RAAE_PICK_*``,
  ``RAAE_BIG_MASK_*`` or ``RAAE_WGRAD_*`` tuning variable is set (the mirror holds the defaults).
* HYGIENE: rows and slabs beyond the returned count keep a sentinel, so do four guard floats behind every written
  tensor; a second identical launch is bitwise equal; running statistics move only when asked.
* Tolerances are those of ``test_block_kernels_gpu.py``: forward tensors 2e-5 relative + 2e-5; data gradients 5e-4 +
  5e-5; weight, bias and slope gradients 5e-4 + 5e-5 * mean|G| * sqrt(B * Lout); forward statistic sums 1e-5 and
  backward partial sums 1e-4 relative, both + max(1e-3, 5e-5 * sqrt(B * L)); running statistics 1e-4 + 1e-6.  From
  1024 rows a parameter gradient may instead lie within 3x the distance of fp32 CPU autograd of the same composition
  from the float64 reference, plus the same floor.

FORM -> CASE (the table test of ``test_conv_reference_cpu.py`` recomputes this map and fails on a gap):
  conv forward    head4 h4_*; head8 h8_*; strip(4,4,11,1) s11_1 / s11_1_m; strip(1,4,11,2) s11_2 / s11_2_m;
                  strip(4,4,5,1) s5_1 / s5_1_m (each unmasked / masked, zero and replicate pad, a ragged last group);
                  strip(4,4,11,2), strip(4,4,7,2), strip(4,4,5,2): compiled, not selectable
                  (``conv_reference.UNSELECTABLE``), their layers run tiled: s11_2x, s7_2x, s5_2x;
                  tiled t_* / g_c13_8 / g_ct13_8; tiled_big tb_* and the strip shapes below the threshold or off
                  alignment (s_below is plain tiled at 1023 rows, s_unal tiled_big); generic g_*
  conv data grad  tiled t_*; tiled_big tb_*; generic g_* (replicate edge loop: g_1024 stride 1, g_rep_s2 stride 2)
  conv weight grad tiled t_*; tiled_big tb_*; generic g_* and t_wide (Cout = 12)
  lenlin          tiled l_t*; generic l_c13* l_wfl (no BIG instance is dispatched for the length-axis Linear)
  sum3, grad_materialize: one kernel each; the count follows the slice rule (x_*)
  head backward   hb4_* hb8_*
"""
import collections
import ctypes as C
import functools
import os
import zlib

import numpy as np
import pytest
import torch

import conv_reference as cr
from conv_reference import OUT_RAW, OUT_STATS_PRELU, OUT_STATS_RAW, OUT_SOFTPLUS, OUT_RELU, f32

TUNED = [k for k in os.environ if k.startswith(("RAAE_PICK_", "RAAE_BIG_MASK_", "RAAE_WGRAD_"))]
pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(bool(TUNED), reason=f"dispatch tuning variables are set: {TUNED}")]

if torch.cuda.is_available():
    from rankaae_amd import ops, _lib
    DEV = torch.device("cuda:0")

MAXP = 512                      # RAAE_MAX_PARTS
SENT = -777.25
WORST = collections.defaultdict(float)       # quantity class -> largest share of its bound over the session

# view: s = PReLU, b = train BatchNorm, e = eval BatchNorm, m = mask, u = update the running statistics
# go:   s = PReLU of the output, b = BatchNorm behind it, u = `u` given, p = softplus, r = ReLU
# bwd:  a = accumulate onto din, p = din_partials, d = dslope; "" = no backward launches
Case = collections.namedtuple("Case", "name op B Cin Lin Cout K s p rep g view stats act go bwd forms off")


def Cv(name, B, Cin, Lin, Cout, K, s=1, p=0, rep=False, g=1, view="", stats=OUT_RAW, act=OUT_RAW, go="", bwd="",
       forms=(None, None, None), off=0, T=False):
    return Case(name, "convT" if T else "conv", B, Cin, Lin, Cout, K, s, p, rep, g, view, stats, act, go, bwd, forms, off)


def Ll(name, B, Cc, Lin, E, view="", stats=OUT_RAW, go="", bwd="", forms=(None, None, None)):
    return Case(name, "lenlin", B, Cc, Lin, Cc, E, 1, 0, False, 1, view, stats, OUT_RAW, go, bwd, forms, 0)


T_, TB, GEN = "tiled", "tiled_big", "generic"
P, PR, RAWS = OUT_STATS_PRELU, OUT_STATS_RAW, OUT_RAW

CASES = [
    # ---- generic, every entry point: 9 / 13 channels at 2 and 37 rows, > 1024 weights, a tile over the LDS budget
    Cv("g_ct13_8_b2", 2, 13, 1, 8, 2, 2, T=True, view="sbu", stats=P, go="sb", bwd="pd", forms=(T_, GEN, T_)),
    Cv("g_ct13_8", 37, 13, 1, 8, 2, 2, T=True, view="sbm", stats=P, go="sb", bwd="apd", forms=(T_, GEN, T_)),
    Cv("g_c13_8", 37, 13, 8, 8, 1, view="sbm", stats=P, go="sb", bwd="pd", forms=(T_, GEN, T_)),
    Cv("g_c13_8_b2", 2, 13, 8, 8, 1, view="b", stats=PR, go="bu", bwd="ap", forms=(T_, GEN, T_)),
    Cv("g_c4_13", 37, 4, 8, 13, 1, view="sem", stats=P, go="sb", bwd="pd", forms=(GEN, T_, GEN)),
    Cv("g_c9_9", 37, 9, 24, 9, 3, 1, 1, view="sbmu", stats=P, go="sbu", bwd="apd", forms=(GEN, GEN, GEN)),
    Cv("g_c9_9_b2", 2, 9, 24, 9, 3, 1, 1, view="", stats=PR, go="", bwd="", forms=(GEN, None, None)),
    Cv("g_plain", 37, 16, 24, 16, 5, 1, 2, view="", stats=PR, go="", bwd="a", forms=(GEN, GEN, GEN)),
    Cv("g_1024", 37, 16, 24, 16, 5, 1, 2, rep=True, view="sbm", stats=P, go="sb", bwd="pd", forms=(GEN, GEN, GEN)),
    Cv("g_1024_sp", 2, 16, 24, 16, 5, 1, 2, rep=True, view="se", stats=RAWS, act=OUT_SOFTPLUS, go="p", bwd="a",
       forms=(GEN, GEN, GEN)),
    Cv("g_rep_s2", 37, 16, 25, 16, 5, 2, 2, rep=True, view="sbm", stats=P, go="s", bwd="pd", forms=(GEN, GEN, GEN)),
    Cv("g_rep_s2_k7", 2, 12, 19, 12, 7, 2, 3, rep=True, view="b", stats=PR, act=OUT_RELU, go="r", bwd="p",
       forms=(GEN, GEN, GEN)),
    Cv("g_grouped", 37, 16, 12, 12, 4, 4, 0, g=4, view="sbm", stats=P, go="sb", bwd="apd", forms=(GEN, GEN, GEN)),
    Cv("g_ct_grouped", 37, 12, 6, 12, 4, 4, g=3, T=True, view="sbm", stats=P, go="sb", bwd="pd", forms=(GEN, GEN, GEN)),
    Cv("g_budget", 2, 24, 512, 2, 3, 1, 1, view="sb", stats=P, go="sb", bwd="pd", forms=(GEN, GEN, GEN)),
    # ---- tiled small: power-of-two and other lengths, groups, transposed, every view / gradient form
    Cv("t_k11", 37, 4, 64, 4, 11, 2, 5, rep=True, view="sbmu", stats=P, go="sb", bwd="apd", forms=(T_, T_, T_)),
    Cv("t_k7_np2", 37, 4, 48, 6, 7, 2, 3, g=2, view="sem", stats=PR, go="bu", bwd="p", forms=(T_, T_, T_)),
    Cv("t_plain", 37, 3, 20, 5, 3, 1, 1, view="", stats=RAWS, go="", bwd="", forms=(T_, None, None)),
    Cv("t_plain_bwd", 37, 3, 20, 5, 3, 1, 1, view="", stats=PR, go="", bwd="a", forms=(T_, T_, T_)),
    Cv("t_softplus", 37, 4, 16, 2, 5, 1, 2, rep=True, view="sb", stats=RAWS, act=OUT_SOFTPLUS, go="p", bwd="p",
       forms=(T_, T_, T_)),
    Cv("t_relu", 2, 8, 64, 4, 1, 1, 0, g=4, view="sbm", stats=RAWS, act=OUT_RELU, go="r", bwd="ap", forms=(T_, T_, T_)),
    Cv("t_sbu", 37, 4, 16, 4, 5, 1, 2, view="sbm", stats=P, go="sbu", bwd="pd", forms=(T_, T_, T_)),
    Cv("t_nods", 37, 4, 16, 4, 5, 1, 2, view="sbm", stats=P, go="sb", bwd="", forms=(T_, None, None)),
    Cv("t_nods_bwd", 37, 4, 16, 4, 5, 1, 2, view="sbm", stats=P, go="sb", bwd="a", forms=(T_, T_, T_)),
    Cv("t_ct6_8", 37, 6, 1, 8, 8, 8, g=2, T=True, view="sbm", stats=P, go="sb", bwd="pd", forms=(T_, T_, T_)),
    Cv("t_ct8_4", 2, 8, 8, 4, 8, 8, g=4, T=True, view="se", stats=PR, go="b", bwd="ap", forms=(T_, T_, T_)),
    Cv("t_wide", 37, 4, 24, 12, 3, 1, 1, view="sbm", stats=RAWS, go="s", bwd="pd", forms=(T_, T_, GEN)),
    Cv("t_c13_nop", 37, 13, 8, 8, 1, view="sbm", stats=P, go="sb", bwd="d", forms=(T_, T_, T_)),
    # ---- tiled BIG (>= 1024 rows): the 16-byte staging and its scalar fall-backs, the capped grid
    Cv("tb_k5", 1027, 4, 40, 4, 5, 1, 2, rep=True, view="sbmu", stats=P, go="sb", bwd="apd", forms=(TB, TB, TB)),
    Cv("tb_k5_off", 1027, 4, 64, 4, 5, 1, 2, view="sbm", stats=P, go="sb", bwd="pd", forms=(TB, TB, TB), off=1),
    Cv("tb_l70", 1027, 4, 35, 4, 2, 2, T=True, view="sem", stats=PR, go="bu", bwd="ap", forms=(TB, TB, TB)),
    Cv("tb_ct8_4", 1027, 8, 8, 4, 8, 8, T=True, view="sbm", stats=RAWS, act=OUT_RELU, go="r", bwd="p", forms=(TB, TB, TB)),
    Cv("tb_cap", 4100, 1, 64, 4, 3, 1, 1, view="", stats=PR, go="", bwd="", forms=(TB, None, None)),
    # ---- strip: the three selectable instances at the least row count with 2^20 outputs, masked and not
    Cv("s11_1_m", 1024, 4, 256, 4, 11, 1, 5, rep=True, view="sbmu", stats=P, forms=("strip(4,4,11,1,mask)", None, None)),
    Cv("s11_1", 1027, 4, 256, 4, 11, 1, 5, view="", stats=RAWS, act=OUT_SOFTPLUS, forms=("strip(4,4,11,1)", None, None)),
    Cv("s11_2_m", 2051, 1, 256, 4, 11, 2, 5, view="sbm", stats=PR, forms=("strip(1,4,11,2,mask)", None, None)),
    Cv("s11_2", 2048, 1, 256, 4, 11, 2, 5, rep=True, view="e", stats=P, forms=("strip(1,4,11,2)", None, None)),
    Cv("s5_1_m", 1027, 4, 256, 4, 5, 1, 2, view="sem", stats=P, forms=("strip(4,4,5,1,mask)", None, None)),
    Cv("s5_1", 1024, 4, 256, 4, 5, 1, 2, rep=True, view="s", stats=RAWS, act=OUT_RELU, forms=("strip(4,4,5,1)", None, None)),
    Cv("s_below", 1023, 4, 256, 4, 11, 1, 5, rep=True, view="sbm", stats=P, forms=(T_, None, None)),
    Cv("s_unal", 1024, 4, 256, 4, 11, 1, 5, rep=True, view="sbm", stats=P, forms=(TB, None, None), off=1),
    Cv("s11_2x", 2050, 4, 256, 4, 11, 2, 5, view="sbm", stats=P, forms=(TB, None, None)),
    Cv("s7_2x", 8200, 4, 64, 4, 7, 2, 3, rep=True, view="b", stats=P, forms=(TB, None, None)),
    Cv("s5_2x", 4100, 4, 128, 4, 5, 2, 2, view="", stats=PR, forms=(TB, None, None)),
    # ---- the head: Conv1d(C, 1, 1) behind a plain BatchNorm view (forward inside raae_conv_fwd), and its fall-backs
    Cv("h4_softplus", 37, 4, 256, 1, 1, view="bu", act=OUT_SOFTPLUS, forms=("head4", None, None)),
    Cv("h4_relu", 37, 4, 256, 1, 1, view="b", act=OUT_RELU, forms=("head4", None, None)),
    Cv("h4_raw", 2, 4, 8, 1, 1, view="e", forms=("head4", None, None)),
    Cv("h4_big", 2051, 4, 256, 1, 1, view="b", act=OUT_SOFTPLUS, forms=("head4", None, None)),
    Cv("h8_raw", 130, 8, 64, 1, 1, view="b", forms=("head8", None, None)),
    Cv("h8_softplus", 37, 8, 64, 1, 1, view="e", act=OUT_SOFTPLUS, forms=("head8", None, None)),
    Cv("h8_relu", 1027, 8, 64, 1, 1, view="bu", act=OUT_RELU, forms=("head8", None, None)),
    Cv("h4_unal", 37, 4, 256, 1, 1, view="b", act=OUT_SOFTPLUS, go="p", bwd="p", forms=(T_, T_, T_), off=1),
    Cv("h4_mask", 37, 4, 256, 1, 1, view="bm", act=OUT_SOFTPLUS, forms=(T_, None, None)),
    # ---- length-axis Linear
    Ll("l_c13", 37, 13, 8, 3, view="sbm", stats=P, go="sb", bwd="apd", forms=(GEN, GEN, GEN)),
    Ll("l_c13_b2", 2, 13, 1, 1, view="bu", stats=PR, go="bu", bwd="p", forms=(GEN, GEN, GEN)),
    Ll("l_c9_plain", 37, 9, 8, 8, view="", stats=P, go="s", bwd="ad", forms=(GEN, T_, GEN)),
    Ll("l_wfl", 37, 1, 256, 9, view="se", stats=RAWS, go="", bwd="a", forms=(GEN, GEN, GEN)),
    Ll("l_t_sub", 37, 4, 64, 2, view="sbmu", stats=P, go="sb", bwd="apd", forms=(T_, T_, T_)),
    Ll("l_t_e64", 37, 8, 2, 64, view="sem", stats=PR, go="bu", bwd="p", forms=(T_, T_, T_)),
    Ll("l_t_np2", 2, 6, 12, 3, view="", stats=RAWS, go="", bwd="a", forms=(T_, T_, T_)),
    Ll("l_t_1027", 1027, 4, 64, 2, view="sbm", stats=P, go="sb", bwd="pd", forms=(T_, T_, T_)),
    Ll("l_t_raw13", 37, 13, 8, 3, view="sbm", stats=RAWS, go="s", bwd="d", forms=(T_, T_, GEN)),
]
BY_NAME = {c.name: c for c in CASES}

# sum3 / grad_materialize: (name, B, C, L, spec flags)
Elem = collections.namedtuple("Elem", "name B C L go acc draw")
ELEM_CASES = [
    Elem("x_c4", 37, 4, 64, "sbu", False, True),
    Elem("x_c13", 2, 13, 8, "sb", True, True),
    Elem("x_nodraw", 37, 4, 64, "sbu", False, False),
    Elem("x_plain", 37, 5, 7, "", True, True),
    Elem("x_relu", 37, 4, 16, "r", False, True),
    Elem("x_softplus", 37, 4, 16, "bp", False, True),
    Elem("x_cap", 1027, 4, 256, "sbu", False, True),
]

# raae_head_bwd: (name, B, C, L, act, view)
HeadB = collections.namedtuple("HeadB", "name B C L act")
HEAD_BWD = [HeadB("hb4_softplus", 37, 4, 256, OUT_SOFTPLUS), HeadB("hb4_relu", 2, 4, 8, OUT_RELU),
            HeadB("hb4_raw", 1027, 4, 256, OUT_RAW), HeadB("hb8_softplus", 130, 8, 64, OUT_SOFTPLUS),
            HeadB("hb8_relu", 37, 8, 64, OUT_RELU), HeadB("hb8_raw", 1027, 8, 64, OUT_RAW)]


def make_op(c):
    if c.op == "lenlin":
        return cr.LenLin(c.Cin, c.Lin, c.K)
    return cr.Conv(c.Cin, c.Lin, c.Cout, c.K, c.s, c.p, c.rep, c.g, c.op == "convT")


def expected(c):
    """What the mirrored dispatch says of case ``c``: ((form, count) | None) x (forward, data, weight)."""
    op = make_op(c)
    v = c.view
    has_bn = "b" in v or "e" in v
    if c.op == "lenlin":
        f = cr.lenlin_fwd_form(c.B, c.Cin, c.Lin, c.K, c.stats)
        d = cr.lenlin_bwd_data_form(c.B, c.Cin, c.Lin, c.K, "p" in c.bwd)
        w = cr.lenlin_bwd_weight_form(c.B, c.Cin, c.Lin, c.K, "d" in c.bwd)
    else:
        f = cr.conv_fwd_form(c.B, op, c.stats, has_bn, "s" in v, "m" in v, aligned=not c.off)
        d = cr.conv_bwd_data_form(c.B, op, "p" in c.bwd)
        w = cr.conv_bwd_weight_form(c.B, op, "d" in c.bwd)
    return f, (d if c.bwd else None), (w if c.bwd else None)


# ------------------------------------------------------------------------------------- case data (CPU, cached)
def _gen(name):
    return torch.Generator().manual_seed(zlib.crc32(name.encode()))


def _view_data(flags, B, Cc, L, g):
    t = {"raw": f32(torch.randn(B, Cc, L, generator=g) * 1.3 + 0.2), "slope": None, "bn": None, "mask": None}
    if "s" in flags:
        t["slope"] = f32(torch.rand(Cc, generator=g) * 0.5 - 0.1)
    if "m" in flags:
        t["mask"] = f32((torch.rand(B, Cc, L, generator=g) < 0.8).double() / 0.8)
    run = (f32(torch.randn(Cc, generator=g) * 0.3), f32(torch.rand(Cc, generator=g) + 0.5))
    if "b" in flags:
        a = cr.prelu(t["raw"], t["slope"]) if t["slope"] is not None else t["raw"]
        t["bn"] = dict(rows=cr.partial_rows([a, a * a], 3), count=B * L, running=run if "u" in flags else None)
    elif "e" in flags:
        t["bn"] = dict(rows=None, running=run)
    t["running0"] = run
    return t


def _go_data(flags, raw, g, act=OUT_RAW):
    """A gradient spec over ``raw`` [B, C, L] (float64 on the fp32 grid): keyword dict of ``cr.grad_spec``."""
    B, Cc, L = raw.shape
    go = dict(g=f32(torch.randn(B, Cc, L, generator=g)), raw=raw, slope=None, bn=None, g_rows=None, u=None, act=act)
    if "s" in flags:
        go["slope"] = f32(torch.rand(Cc, generator=g) * 0.5 - 0.1)
    uu = cr.prelu(raw, go["slope"]) if go["slope"] is not None else raw
    if "u" in flags:
        go["u"] = uu = f32(uu + torch.randn(B, Cc, L, generator=g))
    if "b" in flags:
        go["bn"] = dict(rows=cr.partial_rows([uu, uu * uu], 2), count=B * L)
        mean, rstd, _ = cr.bn_stats(go["bn"]["rows"], B * L)
        y = (uu - mean.view(1, -1, 1)) * rstd.view(1, -1, 1)
        go["g_rows"] = cr.partial_rows([go["g"], go["g"] * y], 3)
    return go


@functools.lru_cache(maxsize=4)
def make(c):
    g = _gen(c.name)
    op = make_op(c)
    t = _view_data(c.view, c.B, c.Cin, c.Lin, g)
    t["w"] = f32(torch.randn(*op.wshape, generator=g) / op.fan ** 0.5)
    t["bias"] = f32(torch.randn(op.wshape[0] if c.op == "lenlin" else c.Cout, generator=g) * 0.2)
    t["oslope"] = f32(torch.rand(c.Cout, generator=g) * 0.5 - 0.1)
    t["fwd"] = cr.layer_fwd(op, t["raw"], t["w"], t["bias"], t["slope"], t["bn"], t["mask"], c.stats, t["oslope"], c.act)
    if c.bwd:
        act = {"p": OUT_SOFTPLUS, "r": OUT_RELU}.get(c.go[-1:] if c.go else "", OUT_RAW)
        t["go"] = _go_data(c.go, f32(t["fwd"]["out"]), g, act)       # raw = the reference's own output, rounded
        t["din0"] = f32(torch.randn(c.B, c.Cin, c.Lin, generator=g)) if "a" in c.bwd else None
        t["bwd"] = cr.layer_bwd(op, t["go"], t["w"], t["raw"], t["slope"], t["bn"], t["mask"], t["din0"])
        t["arbiter"] = None
        if c.B >= cr.BIG_ROWS:
            t["arbiter"] = _arbiter(c, op, t)
    return t


def _arbiter(c, op, t):
    """fp32 CPU autograd of the same composition: (dw, db, dslope)."""
    go = t["go"]
    bn = "train" if "b" in c.view else ((t["bn"]["running"]) if "e" in c.view else None)
    u_add = None
    if go["u"] is not None:
        base = cr.prelu(go["raw"], go["slope"]) if go["slope"] is not None else go["raw"]
        u_add = go["u"] - base
    a = cr.layer_autograd(op, go["g"], t["raw"], t["w"], t["bias"], t["slope"], bn, t["mask"],
                          go["slope"], go["bn"] is not None, u_add, go["act"], dtype=torch.float32)
    return a["dw"], a["db"], a["dslope"]


# ------------------------------------------------------------------------------------- device plumbing
class Report:
    def __init__(self, case):
        self.case, self.bad = case, []

    def close(self, kind, what, got, want, rtol, atol, arbiter=None):
        got, want = got.detach().double().cpu(), want.detach().double().cpu()
        assert got.shape == want.shape, (self.case, what, got.shape, want.shape)
        err, tol = (got - want).abs(), atol + rtol * want.abs()
        finite = bool(torch.isfinite(got).all())
        worst = float(err.max()) if finite else float("inf")
        ratio = float((err / tol).max()) if finite else float("inf")
        ok, note = finite and ratio <= 1.0, ""
        if not ok and finite and arbiter is not None:
            e_ref = float((arbiter.detach().double().cpu() - want).abs().max())
            ok = worst <= 3.0 * e_ref + atol
            note = f"  arbiter: fp32 autograd is {e_ref:.3e} from float64 -> {'ok' if ok else 'FAIL'}"
        else:
            WORST[kind] = max(WORST[kind], ratio)
        print(f"ERR {self.case} {what}: max err {worst:.3e} (max |ref| {float(want.abs().max()):.3e}), "
              f"{ratio:.3f} of the bound [{kind}]{note}")
        if not ok:
            i = int(torch.nan_to_num(err / tol, nan=float("inf")).argmax())
            self.bad.append(f"{what}: max err {worst:.3e} = {ratio:.2f} x bound at flat index {i}: "
                            f"ref {float(want.flatten()[i]):.6e} got {float(got.flatten()[i]):.6e}{note}")

    def check(self, cond, what):
        if not cond:
            self.bad.append(what)

    def done(self):
        assert not self.bad, f"{self.case}:\n" + "\n".join(self.bad)


class Buf:
    """A device tensor (sentinel-filled unless ``src``) ``off`` floats into its allocation, four guard elements behind."""

    def __init__(self, shape, dtype=torch.float32, src=None, off=0):
        self.n, self.off = int(np.prod(shape)), off
        self.whole = torch.full((off + self.n + 4,), SENT, dtype=dtype, device=DEV)
        self.t = self.whole[off:off + self.n].view(*shape)
        self.src = None if src is None else src.to(dtype).contiguous().to(DEV)
        self.reset()

    def reset(self):
        if self.src is not None:
            self.t.copy_(self.src.view(self.t.shape))
        else:
            self.t.fill_(SENT)

    def guard_ok(self):
        return bool((self.whole[self.off + self.n:] == SENT).all()) and bool((self.whole[:self.off] == SENT).all())


def _dev(t, off=0):
    if t is None:
        return None
    if not off:
        return t.float().contiguous().to(DEV)
    return Buf(t.shape, src=t, off=off).t


def _rows(rows, Cc):
    buf = torch.full((MAXP, Cc, 2), SENT, dtype=torch.float64, device=DEV)
    buf[:rows.shape[0]] = rows.to(DEV)
    return buf, rows.shape[0]


class DevView:
    """A reference view on the device; ``rm`` / ``rv`` are reset by ``reset()``."""

    def __init__(self, t, Cc, update, off=0):
        self.raw, self.slope, self.mask = _dev(t["raw"], off), _dev(t["slope"]), _dev(t["mask"], 0)
        self.rm, self.rv = Buf((Cc,), src=t["running0"][0]), Buf((Cc,), src=t["running0"][1])
        self.bn = None
        if t["bn"] is not None and t["bn"].get("rows") is not None:
            self.rows, n = _rows(t["bn"]["rows"], Cc)
            self.bn = ops.make_bn(self.rows, n, t["bn"]["count"], self.rm.t, self.rv.t, update_running=update)
        elif t["bn"] is not None:
            self.bn = ops.make_bn(None, 0, 0, self.rm.t, self.rv.t)
        self.v = ops.make_view(self.raw, self.slope, self.bn, self.mask)

    def reset(self):
        self.rm.reset()
        self.rv.reset()


class DevGrad:
    def __init__(self, go, off=0):
        Cc = go["g"].shape[1]
        self.g, self.raw, self.slope, self.u = _dev(go["g"], off), _dev(go["raw"], off), _dev(go["slope"]), _dev(go["u"], off)
        bn, gp, gn = None, None, 0
        if go["bn"] is not None:
            self.rows, n = _rows(go["bn"]["rows"], Cc)
            bn = ops.make_bn(self.rows, n, go["bn"]["count"])
            gp, gn = _rows(go["g_rows"], Cc)
        self.gp = gp
        self.s = ops.make_grad(self.g, self.raw, self.slope, bn, gp, gn, self.u, go["act"])


def _snap(bufs):
    torch.cuda.synchronize()
    return [b.whole.clone() for b in bufs]


def _same(a, b):
    return all(torch.equal(x.view(torch.uint8), y.view(torch.uint8)) for x, y in zip(a, b))


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


def _tail(B, L):
    return max(1e-3, 5e-5 * (B * L) ** 0.5)


def _cv(c, op):
    return ops.make_conv(c.Cin, c.Lin, c.Cout, op.Lout, c.K, c.s, c.p, c.rep, c.g, c.op == "convT")


def _run_forward(c, t, rep, want):
    op = make_op(c)
    ref = t["fwd"]
    dv = DevView(t, c.Cin, "u" in c.view, c.off)
    out = Buf((c.B, c.Cout, op.Lout), off=c.off)
    parts = Buf((MAXP, c.Cout, 2), torch.float64)
    w, bias, osl = _dev(t["w"]), _dev(t["bias"]), _dev(t["oslope"])
    stats = c.stats != OUT_RAW

    def launch():
        a = (osl if c.stats == OUT_STATS_PRELU else None, parts.t if stats else None)
        if c.op == "lenlin":
            return ops.lenlin_fwd(dv.v, c.B, c.Cin, c.Lin, w, bias, c.K, out.t, c.stats, *a)
        return ops.conv_fwd(dv.v, c.B, _cv(c, op), w, bias, out.t, c.stats, *a, act=c.act)
    n = _twice(rep, [out, parts, dv.rm, dv.rv], launch)
    rep.check(n == want[1], f"forward: {n} partial rows returned, the mirror of `{want[0]}` gives {want[1]}")
    rep.close("forward", "out", out.t, ref["out"], 2e-5, 2e-5)
    rows = parts.t.cpu()
    if stats:
        rep.close("forward sums", "{sum, sumsq}", rows[:n].sum(0), ref["stats"], 1e-5, _tail(c.B, op.Lout))
    rep.check(bool((rows[n if stats else 0:] == SENT).all()), "partial rows beyond the count (or all, without statistics) touched")
    if ref["running"] is not None:
        rep.close("running", "running_mean", dv.rm.t, ref["running"][0], 1e-4, 1e-6)
        rep.close("running", "running_var", dv.rv.t, ref["running"][1], 1e-4, 1e-6)
    else:
        rep.check(torch.equal(dv.rm.t, dv.rm.src) and torch.equal(dv.rv.t, dv.rv.src), "running statistics moved")


def _run_backward(c, t, rep, want_d, want_w):
    op = make_op(c)
    ref, arb = t["bwd"], t["arbiter"] or (None, None, None)
    dv = DevView(t, c.Cin, False, c.off)
    dg = DevGrad(t["go"], c.off)
    w = _dev(t["w"])
    nw = t["w"].numel()
    nb = t["bias"].numel()
    r64 = lambda v: (v + 63) // 64 * 64
    o_db, o_ds = r64(nw), r64(nw) + r64(nb)
    stride = o_ds + r64(c.Cout)
    nslabs = 130
    slabs = Buf((nslabs, stride))
    din = Buf((c.B, c.Cin, c.Lin), src=t["din0"], off=c.off)
    dparts = Buf((MAXP, c.Cin, 2), torch.float64)
    acc, wantp, wantds = "a" in c.bwd, "p" in c.bwd, "d" in c.bwd
    s = slabs.t

    def launch_w():
        a = (s[0, 0:], s[0, o_db:], s[0, o_ds:] if wantds else None, stride)
        if c.op == "lenlin":
            return ops.lenlin_bwd_weight(dg.s, c.B, c.Cin, c.K, dv.v, c.Lin, *a)
        return ops.conv_bwd_weight(dg.s, c.B, _cv(c, op), dv.v, *a)

    def launch_d():
        if c.op == "lenlin":
            return ops.lenlin_bwd_data(dg.s, c.B, c.Cin, c.K, w, dv.v, c.Lin, din.t, acc, dparts.t if wantp else None)
        return ops.conv_bwd_data(dg.s, c.B, _cv(c, op), w, dv.v, din.t, acc, dparts.t if wantp else None)
    ns = _twice(rep, [slabs, dv.rm, dv.rv], launch_w)
    rep.check(ns == want_w[1], f"weight gradient: {ns} slabs returned, the mirror of `{want_w[0]}` gives {want_w[1]}")
    sc = slabs.t.cpu()
    floor = 5e-5 * float(t["go"]["g"].abs().mean()) * (c.B * op.Lout) ** 0.5
    rep.close("parameter", "dw", sc[:ns, :nw].double().sum(0).view(ref["dw"].shape), ref["dw"], 5e-4, floor, arb[0])
    rep.close("parameter", "dbias", sc[:ns, o_db:o_db + nb].double().sum(0), ref["db"], 5e-4, floor, arb[1])
    used = torch.zeros(stride, dtype=torch.bool)
    used[:nw] = True
    used[o_db:o_db + nb] = True
    if wantds:
        rep.close("parameter", "dslope", sc[:ns, o_ds:o_ds + c.Cout].double().sum(0), ref["dslope"], 5e-4, floor, arb[2])
        used[o_ds:o_ds + c.Cout] = True
    rep.check(bool((sc[ns:] == SENT).all()), "slabs beyond the count touched")
    rep.check(bool((sc[:ns][:, ~used] == SENT).all()), "columns of a slab outside dw / dbias / dslope touched")
    rep.check(not bool((sc[:ns][:, used] == SENT).any()), "an element of a slab was left unwritten")
    nd = _twice(rep, [din, dparts, dv.rm, dv.rv], launch_d)
    rep.check(nd == want_d[1], f"data gradient: {nd} partial rows returned, the mirror of `{want_d[0]}` gives {want_d[1]}")
    rep.close("data gradient", "din", din.t, ref["din"], 5e-4, 5e-5)
    rows = dparts.t.cpu()
    if wantp:
        rep.close("backward sums", "{sum din, sum din*y}", rows[:nd].sum(0), ref["pairs"], 1e-4, _tail(c.B, c.Lin))
    rep.check(bool((rows[nd if wantp else 0:] == SENT).all()), "din partial rows beyond the count (or all, unasked) touched")
    rep.check(torch.equal(dv.rm.t, dv.rm.src) and torch.equal(dv.rv.t, dv.rv.src), "a backward launch moved running statistics")


@pytest.mark.parametrize("c", CASES, ids=lambda c: c.name)
def test_layer(c):
    """Forward, data gradient and weight gradient of one layer: every written tensor, the route, the hygiene."""
    t = make(c)
    rep = Report(c.name)
    want = expected(c)
    assert tuple(None if w is None else w[0] for w in want) == tuple(f if (i == 0 or c.bwd) else None for i, f in enumerate(c.forms)), \
        (c.name, want, c.forms)
    _run_forward(c, t, rep, want[0])
    if c.bwd:
        _run_backward(c, t, rep, want[1], want[2])
    rep.done()


# ------------------------------------------------------------------------------------- sum3, grad_materialize
@pytest.mark.parametrize("e", ELEM_CASES, ids=lambda e: e.name)
def test_sum3_and_grad_materialize(e):
    g = _gen(e.name)
    rep = Report(e.name)
    B, Cc, L = e.B, e.C, e.L
    va, vb, vc = _view_data("s", B, Cc, L, g), _view_data("bu", B, Cc, L, g), _view_data("sem" if Cc != 5 else "", B, Cc, L, g)
    y64, st64, run64 = cr.sum3([{k: v[k] for k in ("raw", "slope", "bn", "mask")} for v in (va, vb, vc)])
    da, db_, dc = DevView(va, Cc, False), DevView(vb, Cc, True), DevView(vc, Cc, False)
    y, parts = Buf((B, Cc, L)), Buf((MAXP, Cc, 2), torch.float64)
    n = _twice(rep, [y, parts, db_.rm, db_.rv, dc.rm, dc.rv], lambda: ops.sum3_fwd(da.v, db_.v, dc.v, B, Cc, L, y.t, parts.t))
    rep.check(n == cr.sum3_form(B, L)[1], f"sum3: {n} rows, the slice rule gives {cr.sum3_form(B, L)[1]}")
    rep.close("forward", "Y", y.t, y64, 2e-5, 2e-5)
    rows = parts.t.cpu()
    rep.close("forward sums", "{sum, sumsq} of Y", rows[:n].sum(0), st64, 1e-5, _tail(B, L))
    rep.check(bool((rows[n:] == SENT).all()), "partial rows beyond the count touched")
    rep.close("running", "running_mean (middle view)", db_.rm.t, run64[0], 1e-4, 1e-6)
    rep.close("running", "running_var (middle view)", db_.rv.t, run64[1], 1e-4, 1e-6)
    rep.check(torch.equal(dc.rm.t, dc.rm.src), "an eval-mode view's running statistics moved")
    # the gradient spec over term A of the sum (u = Y when asked), materialised
    act = {"p": OUT_SOFTPLUS, "r": OUT_RELU}.get(e.go[-1:], OUT_RAW)
    raw = f32(cr.activation(va["raw"], act)) if act else va["raw"]
    go = _go_data(e.go, raw, g, act)
    want_dr, want_ds = cr.grad_materialize(go, None)
    draw0 = f32(torch.randn(B, Cc, L, generator=g)) if e.acc else None
    dg = DevGrad(go)
    draw = Buf((B, Cc, L), src=draw0)
    slabs = Buf((66, 64))
    has_s = "s" in e.go
    if not e.draw and not has_s:
        pytest.fail("a case without draw needs a slope")
    ns = _twice(rep, [draw, slabs], lambda: ops.grad_materialize(dg.s, B, Cc, L, draw.t if e.draw else None, e.acc,
                                                                 slabs.t[0] if has_s else None, 64))
    rep.check(ns == cr.grad_materialize_form(B, L)[1], f"grad_materialize: {ns} slabs, the rule gives {cr.grad_materialize_form(B, L)[1]}")
    if e.draw:
        rep.close("data gradient", "draw", draw.t, want_dr + draw0 if e.acc else want_dr, 5e-4, 5e-5)
    else:
        rep.check(bool((draw.t == SENT).all()), "draw written although NULL was passed")   # (the buffer was not passed)
    sc = slabs.t.cpu()
    if has_s:
        floor = 5e-5 * float(go["g"].abs().mean()) * (B * L) ** 0.5
        rep.close("parameter", "dslope", sc[:ns, :Cc].double().sum(0), want_ds, 5e-4, floor)
        rep.check(bool((sc[ns:] == SENT).all()) and bool((sc[:, Cc:] == SENT).all()), "slab elements outside dslope touched")
    else:
        rep.check(bool((sc == SENT).all()), "dslope slabs written without a slope")
    rep.done()


# ------------------------------------------------------------------------------------- raae_head_bwd
@pytest.mark.parametrize("h", HEAD_BWD, ids=lambda h: h.name)
def test_head_backward(h):
    g = _gen(h.name)
    rep = Report(h.name)
    B, Cc, L = h.B, h.C, h.L
    op = cr.Conv(Cc, L, 1, 1)
    t = _view_data("b", B, Cc, L, g)
    t["w"], t["bias"] = f32(torch.randn(1, Cc, 1, generator=g) / Cc ** 0.5), f32(torch.randn(1, generator=g) * 0.2)
    fwd = cr.layer_fwd(op, t["raw"], t["w"], t["bias"], bn=t["bn"], act=h.act)
    go = _go_data("", f32(fwd["out"]), g, h.act)
    bn = dict(t["bn"], running=t["running0"])
    ref = cr.layer_bwd(op, go, t["w"], t["raw"], bn=bn)
    dv, dg = DevView(t, Cc, False), DevGrad(go)
    cv = ops.make_conv(Cc, L, 1, L, 1, 1, 0, False, 1, False)
    rep.check(ops.head_bwd_supported(dg.s, B, cv, dv.v), "raae_head_bwd_supported refuses the head shape")
    din, dparts, slabs = Buf((B, Cc, L)), Buf((MAXP, Cc, 2), torch.float64), Buf((258, 128))
    w = _dev(t["w"])
    nd, ns = _twice(rep, [din, dparts, slabs, dv.rm, dv.rv],
                    lambda: ops.head_bwd(dg.s, B, cv, w, dv.v, din.t, dparts.t, slabs.t[0, 0:], slabs.t[0, 64:], 128))
    form, grid = cr.head_bwd_form(B, op)
    rep.check((nd, ns) == (grid, grid), f"{form}: counts {(nd, ns)}, head_grid gives {grid}")
    rep.close("data gradient", "din", din.t, ref["din"], 5e-4, 5e-5)
    rows, sc = dparts.t.cpu(), slabs.t.cpu()
    rep.close("backward sums", "{sum din, sum din*y}", rows[:nd].sum(0), ref["pairs"], 1e-4, _tail(B, L))
    floor = 5e-5 * float(go["g"].abs().mean()) * (B * L) ** 0.5
    arb = (None, None)
    if B >= cr.BIG_ROWS:
        a = cr.layer_autograd(op, go["g"], t["raw"], t["w"], t["bias"], bn="train", act=h.act, dtype=torch.float32)
        arb = (a["dw"], a["db"])
    rep.close("parameter", "dw", sc[:ns, :Cc].double().sum(0).view(1, Cc, 1), ref["dw"], 5e-4, floor, arb[0])
    rep.close("parameter", "dbias", sc[:ns, 64:65].double().sum(0), ref["db"], 5e-4, floor, arb[1])
    rep.check(bool((rows[nd:] == SENT).all()) and bool((sc[ns:] == SENT).all()), "rows or slabs beyond the count touched")
    rep.check(bool((sc[:ns, Cc:64] == SENT).all()) and bool((sc[:ns, 65:] == SENT).all()), "slab columns outside dw / dbias touched")
    # a gradient 4 bytes into its allocation is refused, and so is one behind a BatchNorm or a PReLU
    off = DevGrad(go, off=1)
    rep.check(not ops.head_bwd_supported(off.s, B, cv, dv.v), "an unaligned gradient is not refused")
    if h.act == OUT_RAW:
        sl = DevGrad(dict(go, slope=f32(torch.rand(1, generator=g))))
        rep.check(not ops.head_bwd_supported(sl.s, B, cv, dv.v), "a gradient behind a PReLU is not refused")
        before = _snap([din, dparts, slabs])
        n1, n2 = C.c_int(-5), C.c_int(-5)
        rc = _lib.load().raae_head_bwd(C.byref(off.s), B, C.byref(cv), C.c_void_p(w.data_ptr()), C.byref(dv.v),
                                       C.c_void_p(din.t.data_ptr()), C.c_void_p(dparts.t.data_ptr()), C.byref(n1),
                                       C.c_void_p(slabs.t.data_ptr()), C.c_void_p(slabs.t[0, 64:].data_ptr()), 128,
                                       C.byref(n2), C.c_void_p(torch.cuda.current_stream().cuda_stream))
        rep.check(rc == -1 and (n1.value, n2.value) == (-5, -5) and _same(before, _snap([din, dparts, slabs])),
                  "raae_head_bwd on an unaligned gradient: not RAAE_EINVAL, or something was written")
    rep.done()


# ------------------------------------------------------------------------------------- argument rejections
def test_rejections_launch_nothing():
    """``conv_ok`` / ``view_ok`` / ``grad_ok`` refusals: RAAE_EINVAL, the count untouched, no output written.  Every
    buffer is sized for the larger of the declared and the consistent shape, and every refused shape stays inside the
    kernels' own limits apart from the one refused property (K = 17 with 4 x 4 channels is 272 weights; 65 channels
    would index one float past a 64-entry LDS table, never global memory)."""
    rep = Report("einval")
    lib = _lib.load()
    st = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda x: None if x is None else C.c_void_p(x.data_ptr())
    g = _gen("einval")

    def rig(Cin, Lin, Cout, Lout, B=4):
        t = _view_data("sb", B, Cin, Lin, g)
        dv = DevView(t, Cin, False)
        raw = f32(torch.randn(B, Cout, Lout, generator=g))
        dg = DevGrad(_go_data("sb", raw, g))
        w = torch.zeros(70 * 70 * 17, device=DEV)
        bufs = [Buf((B, 70, max(Lout, Lin) * 4)), Buf((MAXP, 70, 2), torch.float64), Buf((130, 8192))]
        return dv, dg, w, bufs

    def expect(what, cv_args, dslope_without_slope=False, stats_without_rows=False, lenlin=False):
        Cin, Lin, Cout, Lout = cv_args[0], cv_args[1], cv_args[2], cv_args[3]
        dv, dg, w, (out, parts, slabs) = rig(Cin, Lin, Cout, Lout)
        if dslope_without_slope:
            dg.s.slope = None
        cv = ops.make_conv(*cv_args)
        before = _snap([out, parts, slabs])
        n = C.c_int(-5)
        rcs = []
        if not dslope_without_slope:
            rcs.append(lib.raae_conv_fwd(C.byref(dv.v), 4, C.byref(cv), p(w), p(w), p(out.t), OUT_STATS_RAW,
                                         None, None if stats_without_rows else p(parts.t), C.byref(n), 0, st()))
        if not stats_without_rows:
            rcs.append(lib.raae_conv_bwd_weight(C.byref(dg.s), 4, C.byref(cv), C.byref(dv.v), p(slabs.t), p(slabs.t[0, 4096:]),
                                                p(slabs.t[0, 6144:]), 8192, C.byref(n), st()))
        if not dslope_without_slope and not stats_without_rows:
            rcs.append(lib.raae_conv_bwd_data(C.byref(dg.s), 4, C.byref(cv), p(w), C.byref(dv.v), p(out.t), 0, p(parts.t),
                                              C.byref(n), st()))
        rep.check(all(rc == -1 for rc in rcs) and n.value == -5, f"{what}: return codes {rcs}, count {n.value}")
        rep.check(_same(before, _snap([out, parts, slabs])), f"{what}: an output was written")

    expect("K = 17", (4, 32, 4, 32, 17, 1, 8, 0, 1, 0))
    expect("65 input channels", (65, 8, 4, 8, 1, 1, 0, 0, 1, 0))
    expect("65 output channels", (4, 8, 65, 8, 1, 1, 0, 0, 1, 0))
    expect("transposed with K != stride", (4, 8, 4, 16, 3, 2, 0, 0, 1, 1))
    expect("wrong Lout", (4, 32, 4, 31, 3, 1, 1, 0, 1, 0))
    expect("channels not divisible by groups", (6, 8, 4, 8, 1, 1, 0, 0, 4, 0))
    expect("dslope without a slope", (4, 32, 4, 32, 3, 1, 1, 0, 1, 0), dslope_without_slope=True)
    expect("statistics without out_partials", (4, 32, 4, 32, 3, 1, 1, 0, 1, 0), stats_without_rows=True)
    # the length-axis Linear and the element-wise kernels share view_ok / grad_ok
    dv, dg, w, (out, parts, slabs) = rig(4, 8, 4, 8)
    before = _snap([out, parts, slabs])
    n = C.c_int(-5)
    rcs = [lib.raae_lenlin_fwd(C.byref(dv.v), 4, 4, 8, p(w), p(w), 8, p(out.t), OUT_STATS_RAW, None, None, C.byref(n), st()),
           lib.raae_lenlin_fwd(C.byref(dv.v), 4, 65, 8, p(w), p(w), 8, p(out.t), OUT_RAW, None, None, C.byref(n), st()),
           lib.raae_sum3_fwd(C.byref(dv.v), C.byref(dv.v), C.byref(dv.v), 4, 65, 8, p(out.t), p(parts.t), C.byref(n), st()),
           lib.raae_grad_materialize(C.byref(dg.s), 4, 4, 8, None, 0, None, 64, C.byref(n), st())]
    dg.s.slope = None
    rcs.append(lib.raae_lenlin_bwd_weight(C.byref(dg.s), 4, 4, 8, C.byref(dv.v), 8, p(slabs.t), p(slabs.t[0, 4096:]),
                                          p(slabs.t[0, 6144:]), 8192, C.byref(n), st()))
    rcs.append(lib.raae_grad_materialize(C.byref(dg.s), 4, 4, 8, p(out.t), 0, p(slabs.t), 64, C.byref(n), st()))
    rep.check(all(rc == -1 for rc in rcs) and n.value == -5, f"lenlin / sum3 / grad_materialize: return codes {rcs}")
    rep.check(_same(before, _snap([out, parts, slabs])), "lenlin / sum3 / grad_materialize: an output was written")
    rep.done()


def test_zz_worst_ratios():
    """Prints the largest share of each bound over the cases this session ran (figures for DESIGN.md); asserts nothing
    the cases have not asserted already."""
    for k, v in sorted(WORST.items()):
        print(f"WORST {k}: {v:.4f} of its bound")
