"""``conv_reference`` against float64 torch autograd of the same composition (1e-10), and the case table of
``test_conv_kernels_gpu.py`` against the mirrored dispatch: every case runs the form it names, every form the dispatch
can select has a forward case and (where one exists) a backward case, every strip instance a masked and an unmasked
one; forms that are compiled but cannot be selected are listed with the reason."""
import re

import pytest
import torch
import torch.nn.functional as F

import conv_reference as cr
import test_conv_kernels_gpu as tk
from conv_reference import OUT_RAW, OUT_STATS_PRELU, OUT_STATS_RAW, OUT_SOFTPLUS, OUT_RELU

TOL = 1e-10


def close(a, b, what):
    assert a.shape == b.shape, (what, a.shape, b.shape)
    err = float((a - b).abs().max())
    assert err <= TOL * (1.0 + float(b.abs().max())), f"{what}: {err:.3e}"


OPS = {
    "conv_k11_s2_rep": lambda: cr.Conv(4, 64, 4, 11, 2, 5, True),
    "conv_k7_s2_g2": lambda: cr.Conv(4, 48, 6, 7, 2, 3, False, 2),
    "conv_k5_rep": lambda: cr.Conv(16, 24, 16, 5, 1, 2, True),
    "conv_k5_s2_rep_odd": lambda: cr.Conv(16, 25, 16, 5, 2, 2, True),
    "conv_k7_s2_rep_odd": lambda: cr.Conv(12, 19, 12, 7, 2, 3, True),
    "conv_k4_s4_g4": lambda: cr.Conv(16, 12, 12, 4, 4, 0, False, 4),
    "conv_k3_zero_floor": lambda: cr.Conv(3, 20, 5, 3, 2, 1),
    "conv_1x1_head": lambda: cr.Conv(4, 16, 1, 1),
    "convT_13_8": lambda: cr.Conv(13, 1, 8, 2, 2, transposed=True),
    "convT_g3": lambda: cr.Conv(12, 6, 12, 4, 4, groups=3, transposed=True),
    "lenlin_c13": lambda: cr.LenLin(13, 8, 3),
    "lenlin_e64": lambda: cr.LenLin(8, 2, 64),
}
# (view flags, gradient-spec flags, accumulate): see test_conv_kernels_gpu.Case
COMBOS = [("sbm", "sb", True), ("sem", "bu", False), ("", "", True), ("b", "sbu", False), ("sm", "s", False),
          ("sb", "p", False), ("e", "r", True), ("sbm", "bp", False)]


@pytest.mark.parametrize("combo", COMBOS, ids=lambda c: "-".join(x or "none" for x in c[:2]))
@pytest.mark.parametrize("name", list(OPS))
def test_layer_reference_is_float64_autograd(name, combo):
    """Forward, data gradient, {sum, sum*y}, weight / bias / slope gradients and the running-statistic update of every
    layer kind under every view and gradient-spec form."""
    vflags, gflags, acc = combo
    op = OPS[name]()
    B = 5
    g = tk._gen(name + vflags + gflags)
    t = tk._view_data(vflags + "u", B, op.Cin, op.Lin, g)
    if "b" in vflags:
        t["bn"]["running"] = (torch.zeros(op.Cin, dtype=torch.float64), torch.ones(op.Cin, dtype=torch.float64))
    w = torch.randn(*op.wshape, generator=g).double() / op.fan ** 0.5
    bias = torch.randn(op.Lout if isinstance(op, cr.LenLin) else op.Cout, generator=g).double()
    act = {"p": OUT_SOFTPLUS, "r": OUT_RELU}.get(gflags[-1:], OUT_RAW)
    oslope = torch.rand(op.Cout, generator=g).double() * 0.5 - 0.1
    kind = OUT_STATS_PRELU if "s" in gflags else OUT_STATS_RAW
    fwd = cr.layer_fwd(op, t["raw"], w, bias, t["slope"], t["bn"], t["mask"], kind, oslope, act)
    go = tk._go_data(gflags, fwd["out"], g, act)        # raw = the reference's own output, not rounded here
    din0 = torch.randn(B, op.Cin, op.Lin, generator=g).double() if acc else None
    bwd = cr.layer_bwd(op, go, w, t["raw"], t["slope"], t["bn"], t["mask"], din0)
    base = cr.prelu(fwd["out"], go["slope"]) if "s" in gflags else fwd["out"]
    a = cr.layer_autograd(op, go["g"], t["raw"], w, bias, t["slope"],
                          "train" if "b" in vflags else t["bn"]["running"] if "e" in vflags else None, t["mask"],
                          go["slope"], "b" in gflags, go["u"] - base if go["u"] is not None else None, act)
    close(fwd["out"], a["out"], "out")
    v = cr.prelu(fwd["z"], oslope) if kind == OUT_STATS_PRELU else fwd["z"]
    close(fwd["stats"], cr.chan_stats(v), "forward statistics")
    close(bwd["din"], a["din"] + (din0 if acc else 0), "din")
    close(bwd["dw"], a["dw"], "dw")
    close(bwd["db"], a["db"], "dbias")
    if "s" in gflags:
        close(bwd["dslope"], a["dslope"], "dslope")
    y = cr.view(t["raw"], t["slope"], t["bn"])[1]
    close(bwd["pairs"], torch.stack([bwd["din"].sum((0, 2)), (bwd["din"] * y).sum((0, 2))], 1), "pairs")
    if "b" in vflags:
        close(fwd["running"][0], a["running"][0], "running mean")
        close(fwd["running"][1], a["running"][1], "running var")
    else:
        assert fwd["running"] is None


def test_sum3_and_grad_materialize_are_float64_autograd():
    g = tk._gen("sum3")
    B, Cc, L = 6, 5, 7
    va, vb, vc = tk._view_data("s", B, Cc, L, g), tk._view_data("bu", B, Cc, L, g), tk._view_data("sem", B, Cc, L, g)
    vb["bn"]["running"] = (torch.zeros(Cc, dtype=torch.float64), torch.ones(Cc, dtype=torch.float64))
    y, st, run = cr.sum3([{k: v[k] for k in ("raw", "slope", "bn", "mask")} for v in (va, vb, vc)])
    A = va["raw"].clone().requires_grad_(True)
    sa = va["slope"].clone().requires_grad_(True)
    rm, rv = torch.zeros(Cc, dtype=torch.float64), torch.ones(Cc, dtype=torch.float64)
    Y = F.prelu(A, sa) + F.batch_norm(vb["raw"], rm, rv, training=True, momentum=0.1, eps=1e-5) + \
        F.batch_norm(F.prelu(vc["raw"], vc["slope"]), vc["running0"][0].clone(), vc["running0"][1].clone(), training=False,
                     eps=1e-5) * vc["mask"]
    close(y, Y.detach(), "Y")
    close(st, cr.chan_stats(Y.detach()), "statistics of Y")
    close(run[0], rm, "running mean")
    close(run[1], rv, "running var")
    G = torch.randn(B, Cc, L, generator=g).double()
    (F.batch_norm(Y, None, None, training=True, eps=1e-5) * G).sum().backward()
    go = tk._go_data("b", y, g)
    go.update(g=G, raw=va["raw"], slope=va["slope"], u=y)
    mean, rstd, _ = cr.bn_stats(go["bn"]["rows"], B * L)
    go["g_rows"] = cr.partial_rows([G, G * (y - mean.view(1, -1, 1)) * rstd.view(1, -1, 1)], 2)
    d0 = torch.randn(B, Cc, L, generator=g).double()
    dr, ds = cr.grad_materialize(go, d0)
    close(dr, A.grad + d0, "draw (accumulated)")
    close(ds, sa.grad, "dslope")
    z = torch.randn(B, Cc, L, generator=g).double().requires_grad_(True)
    for act, fn in ((OUT_SOFTPLUS, lambda t: F.softplus(t, beta=2)), (OUT_RELU, torch.relu)):
        o = fn(z)
        (grad,) = torch.autograd.grad((o * G).sum(), z)
        close(cr.activation(z.detach(), act), o.detach(), "activation")
        close(cr.grad_spec(G, raw=o.detach(), act=act)[0], grad, "activation derivative from the activated output")


# ------------------------------------------------------------------------------------------------ the case table
def _forms():
    """form -> [case names] per entry point, as the mirror routes the GPU file's cases."""
    m = {"fwd": {}, "data": {}, "weight": {}, "lenlin_fwd": {}, "lenlin_data": {}, "lenlin_weight": {}}
    for c in tk.CASES:
        pre = "lenlin_" if c.op == "lenlin" else ""
        for key, w in zip(("fwd", "data", "weight"), tk.expected(c)):
            if w is not None:
                m[pre + key].setdefault(w[0], []).append(c.name)
    return m


def test_every_case_runs_the_form_it_names():
    names = [c.name for c in tk.CASES] + [e.name for e in tk.ELEM_CASES] + [h.name for h in tk.HEAD_BWD]
    assert len(names) == len(set(names))
    for c in tk.CASES:
        want = tk.expected(c)
        got = tuple(None if w is None else w[0] for w in want)
        named = tuple(f if (i == 0 or c.bwd) else None for i, f in enumerate(c.forms))
        assert got == named, (c.name, got, named)
        for w in want:
            assert w is None or 0 <= w[1] <= cr.MAX_PARTS
        op = tk.make_op(c)
        assert c.op == "lenlin" or cr.conv_ok(op)


def test_every_selectable_form_has_a_case():
    m = _forms()
    strips = {f"strip({','.join(map(str, s))}{mk})" for s in cr.STRIP_INSTANCES for mk in ("", ",mask")}
    dead = {s for s in strips if re.sub(",mask", "", s) in cr.UNSELECTABLE}
    assert len(dead) == 6 and len(cr.UNSELECTABLE) == 3
    assert set(m["fwd"]) == {"head4", "head8", "tiled", "tiled_big", "generic"} | (strips - dead), sorted(m["fwd"])
    for key in ("data", "weight"):
        assert set(m[key]) == {"tiled", "tiled_big", "generic"}, (key, sorted(m[key]))
    for key in ("lenlin_fwd", "lenlin_data", "lenlin_weight"):        # lenlin launches <false> at every row count
        assert set(m[key]) == {"tiled", "generic"}, (key, sorted(m[key]))
    assert {cr.head_bwd_form(h.B, cr.Conv(h.C, h.L, 1, 1))[0] for h in tk.HEAD_BWD} == {"head4", "head8"}
    assert {h.act for h in tk.HEAD_BWD if h.C == 4} == {h.act for h in tk.HEAD_BWD if h.C == 8} == {OUT_RAW, OUT_SOFTPLUS, OUT_RELU}
    by = tk.BY_NAME
    # the generic kernels a user configuration reaches (nstyle 9..64: the first decoder block is nstyle -> 8 channels)
    assert tk.expected(by["g_ct13_8"])[1][0] == "generic" and tk.expected(by["l_c13"]) [0][0] == "generic"
    assert tk.expected(by["l_c13"])[2][0] == "generic"
    # view / gradient-spec forms, each on a tiled and on a generic kernel of the data gradient
    for what, pred in (("eval BatchNorm", lambda c: "e" in c.view), ("plain view", lambda c: c.view == "" and c.go == ""),
                       ("go.u", lambda c: "u" in c.go), ("softplus", lambda c: "p" in c.go), ("relu", lambda c: "r" in c.go),
                       ("accumulate with partials", lambda c: "a" in c.bwd and "p" in c.bwd),
                       ("no accumulate with partials", lambda c: "a" not in c.bwd and "p" in c.bwd),
                       ("NULL dslope", lambda c: "d" not in c.bwd), ("NULL din_partials", lambda c: "p" not in c.bwd)):
        hit = {tk.expected(c)[1][0].replace("_big", "") for c in tk.CASES if c.bwd and pred(c)}
        assert hit >= {"tiled", "generic"}, (what, hit)
    hit = {tk.expected(c)[0][0].replace("_big", "") for c in tk.CASES if "u" in c.view and "b" in c.view}
    assert hit >= {"tiled", "generic", "head4", "head8"} and any(h.startswith("strip") for h in hit), hit
    # the grid caps: RAAE_MAX_PARTS forward, 128 slabs of the conv weight gradient, 64 of the lenlin one and of
    # grad_materialize, 256 of the head
    assert tk.expected(by["tb_cap"])[0] == ("tiled_big", 512) and cr.cdiv(4100, 8) == 513
    assert tk.expected(by["tb_k5"])[2][1] == 128 and tk.expected(by["l_t_1027"])[2][1] == 64
    assert cr.grad_materialize_form(1027, 256)[1] == 64 and cr.sum3_form(1027, 256)[1] == 512
    assert cr.head_fwd_grid(2051, cr.Conv(4, 256, 1, 1)) == 256 and cr.head_bwd_form(1027, cr.Conv(4, 256, 1, 1))[1] == 256


def test_unselectable_strip_instances():
    """The three stride-2 instances with four input channels fail the 72 KB test at every length the other tests of
    ``conv_fwd_strip`` admit, at any row count; the other three instances are selectable."""
    reach = set()
    for (ci, co, k, s) in cr.STRIP_INSTANCES:
        for lout in range(4, 1025, 4):
            cv = cr.Conv(ci, lout * s, co, k, s, (k - 1) // 2)
            assert cv.Lout == lout
            if cr.strip_form(1 << 22, cv, False):
                reach.add(f"strip({ci},{co},{k},{s})")
    all_ = {f"strip({','.join(map(str, s))})" for s in cr.STRIP_INSTANCES}
    assert all_ - reach == set(cr.UNSELECTABLE), (reach, cr.UNSELECTABLE)
    # the strip shapes the engine's layers have at 256 points: the stride-2 4 -> 4 layers run the tiled kernels
    for name in ("s11_2x", "s7_2x", "s5_2x"):
        assert tk.expected(tk.BY_NAME[name])[0][0] == "tiled_big"


def test_pick_S_and_slices_mirror_known_geometry():
    """Spot values worked out by hand from ``pick_S`` / ``slices_for`` / ``head_grid`` of csrc/raae_conv.hip."""
    assert cr.pick_S(1040, 1024, 256, cr.TILE_BUDGET, 256) == 1          # small sample, 256 rows: one per group
    assert cr.pick_S(1040, 1024, 4096, cr.TILE_BUDGET, 256) == 8         # ceil(4096/256) = 16 > 8 * 1
    assert cr.pick_S(1040, 1024, 1500, cr.TILE_BUDGET, 256) == 4         # 6 groups wanted: over 4 S, under 8 S -> 4 S
    assert cr.pick_S(4096, 1024, 8192, cr.TILE_BUDGET, 256) == 2         # large sample: capped by the LDS budget
    assert cr.pick_S(13, 8, 2, cr.TILE_BUDGET, 256) == 2                 # never more than the batch
    assert cr.slices_for(1) == 1 and cr.slices_for(257) == 2 and cr.slices_for(10 ** 7) == 512
    assert cr.head_grid(37 * 64, 4) == 10 and cr.head_grid(1 << 17, 4) == 256 and cr.head_grid(1 << 17, 2) == 256
