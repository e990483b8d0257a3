"""Pins ``step_reference`` (the oracle of ``test_step_kernels_gpu.py``) without a GPU: Philox4x32-10 to the Random123
known-answer vectors, the update rules to float64 ``torch.optim`` / ``optim_reference`` with state loaded, the tape
layout rules, and the GPU module's FORM -> CASE table to the dispatch mirror."""
import itertools

import numpy as np
import pytest
import torch

import step_reference as sr
import test_step_kernels_gpu as gpu
from dense_reference import step_keys
from optim_reference import OPTIMIZERS

KAT = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
       ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
       ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
        (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]


# ------------------------------------------------------------------------------------------------------------ Philox
@pytest.mark.parametrize("ctr,key,want", KAT)
def test_philox_known_answers(ctr, key, want):
    assert sr.philox4x32_10_int(ctr, key) == want
    assert tuple(int(w[0]) for w in sr.philox4x32_10(ctr, key)) == want


def test_philox_vectorised_is_the_scalar_form():
    g = np.random.default_rng(3)
    n = 300
    c = g.integers(0, 2 ** 32, size=(4, n), dtype=np.uint64)
    c[0, :50] = np.arange(50)                       # small block numbers, high words set in the others
    c[1, 50:100] = 0
    c[:, 100] = 0xFFFFFFFF
    key = (0x89ABCDEF, 0xFFFFFFFE)
    got = np.stack(sr.philox4x32_10(list(c), key), 1)
    for i in range(n):
        assert tuple(int(x) for x in got[i]) == sr.philox4x32_10_int([int(x) for x in c[:, i]], key), i


def test_u01_and_the_fp32_form_the_kernel_holds():
    lo, hi = float(sr.u01(0)), float(sr.u01(0xFFFFFFFF))
    assert 0.0 < lo < hi < 1.0 and lo == 0.5 / 2 ** 24 and hi == 1.0 - 0.5 / 2 ** 24
    x = (np.arange(0, 2 ** 24, 4099, dtype=np.uint64) << np.uint64(8)) | np.uint64(0xAB)
    k = x >> np.uint64(8)
    f = sr.u01_f32(x).astype(np.float64)
    small = k < 2 ** 23
    assert small.any() and (~small).any()
    assert np.array_equal(f[small], sr.u01(x)[small]), "below 2^23 the fp32 form is exact"
    d = (f - sr.u01(x))[~small] * 2 ** 24
    assert set(np.unique(d)) == {-0.5, 0.5}, "from 2^23 on k + 0.5 rounds to the even neighbour"
    assert float(sr.u01_f32(0)) == lo and float(sr.u01_f32(0xFFFFFFFF)) == 1.0      # the one value that leaves (0, 1)


def test_normal4_word_order_and_finiteness():
    z, r = sr.normal4(np.array([0, 1, 2 ** 32 + 7]), 2 ** 32 + 5, 0xABCDEF0123456789)
    assert np.isfinite(z).all() and (r >= 0).all()
    w = sr.philox4x32_10_int([7, 1, 5, 1], [0x23456789, 0xABCDEF01])     # block 2^32 + 7 -> {low, high}, counter likewise
    r0 = np.sqrt(-2.0 * np.log(float(sr.u01_f32(w[0]))))
    a0 = float(np.float32(6.283185307179586) * sr.u01_f32(w[1]))
    assert z[2, 0] == r0 * np.cos(a0) and z[2, 1] == r0 * np.sin(a0) and r[2, 0] == r[2, 1] == r0
    r1 = np.sqrt(-2.0 * np.log(float(sr.u01_f32(w[2]))))
    a1 = float(np.float32(6.283185307179586) * sr.u01_f32(w[3]))
    assert z[2, 2] == r1 * np.cos(a1) and z[2, 3] == r1 * np.sin(a1)
    big = sr.gauss_slot(0, 200000, 1, 1234)[0]
    assert abs(big.mean()) < 0.01 and abs(big.std() - 1) < 0.01 and abs((big ** 4).mean() - 3) < 0.1
    assert 0.5 < sr.gauss_f32_error_ulps(0, 20000, 1, 1234) < 8.0       # numpy's float32 chain: a few ulps of r


def test_fill_layout_rules():
    segs = [(0, 6, 0, 0), (8, 8, 1, 1000), (16, 5, 0, 8), (24, 4, 2, 77)]
    ref = sr.fill(segs, [1.0, 0.9, 1.0, 0.5], 27, 1234, 9, -5.0)
    kind, tape = ref["kind"], ref["tape"]
    assert kind.tolist() == [0] * 6 + [-1] * 2 + [1] * 8 + [0] * 5 + [-1] * 3 + [2] * 3     # total cuts the last segment
    assert (tape[kind == -1] == -5.0).all()
    z = sr.normal4(np.arange(4), 9, 1234)[0].reshape(-1)
    assert np.array_equal(tape[:6], z[:6]) and np.array_equal(tape[16:21], z[8:13]), "the numbering continues at 8"
    assert set(np.unique(tape[8:16])) <= {0.0, float(np.float32(1.0) / np.float32(0.9))}
    bits = tape[24:27].astype(np.float32).view(np.uint32)
    assert all(b in (0, 0x3F80, 0x3F800000, 0x3F803F80) for b in bits.tolist())


def test_tick_and_step_begin_state():
    t = sr.tick([1, 2, 3, 4], 3, 0b1101, 2 ** 64 - 1, 5, 10, 7)
    assert t["steps"] == [2, 2, 4, 4] and t["ctr"] == 0 and t["cursor"] == 17 and t["keys"] == step_keys(5, 0)
    assert sr.tick([1], 0, 1)["steps"] == [1] and sr.tick([1], 1, 1)["ctr"] is None
    spec, aux = np.arange(12, dtype=np.float32).reshape(4, 3), np.arange(8, dtype=np.float32).reshape(4, 2)
    idx = np.array([3, 3, 0, 2, 1])
    o = sr.step_begin([0, 0], 2, 0b10, 4, 9, 1, 2, spec, aux, idx, 2)
    assert o["steps"] == [0, 1] and o["ctr"] == 5 and o["cursor"] == 3
    assert np.array_equal(o["rows"], spec[[3, 0]]) and np.array_equal(o["aux_out"], aux[[3, 0]]) and o["tape"] is None
    o = sr.step_begin([0, 0], 2, 0b10, 4, 9, 1, 2, spec, aux, idx, 2, 0.5, None, 8)
    z = sr.normal4(np.array([2, 3]), 5, 9)[0].reshape(-1)[:6].reshape(2, 3)
    assert np.array_equal(o["spec_out"], spec[[3, 0]] + 0.5 * z)


# ------------------------------------------------------------------------------------------------------ update rules
class RAdam64(OPTIMIZERS["RAdam"]):
    """The restated class computes on fp32 copies, as torch_optimizer's does; the same lines on float64 copies."""
    compute_dtype = torch.float64


def _torch_step(rule, p, m, v, g, h, t):
    ref = torch.tensor(p, dtype=torch.float64, requires_grad=True)
    kw = dict(lr=h[0], betas=(h[1], h[2]), eps=h[3], weight_decay=h[4])
    if rule in (sr.ADAM, sr.ADAMW):
        opt = (torch.optim.AdamW if rule == sr.ADAMW else torch.optim.Adam)([ref], **kw)
        step = torch.tensor(float(t - 1))
    elif rule == sr.RADAM:
        opt, step = RAdam64([ref], **kw), t - 1
    else:
        opt, step = OPTIMIZERS["AdaBound"]([ref], final_lr=h[6], gamma=h[7], **kw), t - 1
        opt.base_lrs = [h[5]]
    opt.state[ref] = {"step": step, "exp_avg": torch.tensor(m, dtype=torch.float64),
                      "exp_avg_sq": torch.tensor(v, dtype=torch.float64)}
    ref.grad = torch.tensor(g, dtype=torch.float64)
    opt.step()
    st = opt.state[ref]
    return ref.detach().numpy(), st["exp_avg"].numpy(), st["exp_avg_sq"].numpy()


CLAMPED = {"lo": 0, "hi": 0}


@pytest.mark.parametrize("t", [1, 5, 6, 7, 1000, 100000])
@pytest.mark.parametrize("rule", gpu.RULES, ids=lambda r: sr.RULE_NAMES[r])
def test_update_is_the_float64_optimizer(rule, t):
    """Both beta pairs x weight decay 0 / 0.01 x {lr as constructed, behind an lr cut} x {no clip scale, 0.37}, one
    test per rule and step count (the cases of one test share nothing but the data)."""
    g_ = np.random.default_rng(t)
    n = 9 * 32
    gs = np.repeat(10.0 ** np.arange(-4, 5), 32)                       # gradients over eight decades
    p, grad = g_.standard_normal(n), g_.standard_normal(n) * gs
    m, v = (0.1 * g_.standard_normal(n) * gs, g_.random(n) * gs * gs) if t > 1 else (np.zeros(n), np.zeros(n))
    for betas, wd, lr_cut, scale in itertools.product([(0.9, 0.999), (0.99, 0.9999)], [0.0, 0.01], [False, True], [None, 0.37]):
        h = [0.001 if lr_cut else 0.01, betas[0], betas[1], 1e-8, wd, 0.01, 0.1, 1e-3]
        info = {}
        got = sr.update(rule, p, m, v, grad, h, t, scale, info)
        want = _torch_step(rule, p, m, v, grad * (1.0 if scale is None else scale), h, t)
        for a, b, unit, what in zip(got, want, (1.0, gs, gs * gs), "pmv"):
            assert np.all(np.abs(a - b) <= 1e-12 * (np.abs(b) + unit)), (what, betas, wd, lr_cut, scale, float(np.abs(a - b).max()))
        if rule == sr.RADAM:
            assert sr.radam_scalars(h, t)[1] == (t >= 6), "t = 6 is the first rectified step at both beta2"
        if rule == sr.ADABOUND and wd == 0.0:
            CLAMPED["lo"] += int(info["lo"].sum())
            CLAMPED["hi"] += int(info["hi"].sum())


def test_zz_adabound_clamp_bound_at_both_ends():
    assert CLAMPED["lo"] > 100 and CLAMPED["hi"] > 100, CLAMPED


def test_step_leaves_a_segment_without_slabs():
    g_ = np.random.default_rng(1)
    slabs = g_.standard_normal((4, 192)).astype(np.float32)
    slabs[2:, :64] = np.nan
    p, m, v = g_.standard_normal(192), g_.standard_normal(192), g_.random(192)
    pn, mn, vn = sr.step(sr.ADAMW, p, m, v, slabs, [2, 0, 4], sr.HYPER, 3)
    assert np.isfinite(pn).all() and np.array_equal(pn[64:128], p[64:128]) and np.array_equal(vn[64:128], v[64:128])
    assert not np.array_equal(pn[:64], p[:64])
    g, has = sr.slab_sum(slabs, [2, 0, 4])
    assert np.array_equal(g[:64], slabs[0, :64].astype(np.float64) + slabs[1, :64]) and not has[64:128].any()


# -------------------------------------------------------------------------------------------------------- case table
def test_dispatch_mirror_edges():
    assert sr.update_form(64, 16) == ("thread", 1) and sr.update_form(64, 17) == ("lanes8", 2)
    assert sr.update_form(1048576, 2) == ("thread", 4096) and sr.update_form(1048576 + 64, 2) == ("thread", 4096)
    assert sr.update_form(131072 + 64, 17) == ("lanes8", 4096) and sr.update_form(131072 - 32, 17)[1] == 4095
    assert sr.rng_fill_grid(3) == 1 and sr.rng_fill_grid(4 * 256 * 4096) == 4096 and sr.rng_fill_grid(4 * 256 * 4095) == 4095
    assert sr.step_begin_grid(2, 8, 0) == 64 and sr.step_begin_grid(2, 8, 65 * 4096 * 4) == 65
    assert sr.step_begin_grid(16400, 1024, 0) == 1024


def test_every_form_has_a_case():
    """FORM -> CASE recomputed from the mirror: all 32 update instances, both slab_reduce shapes, both fill grids, every
    ``step_begin`` form; and every case's expected grid is the mirror's."""
    forms = {}
    for c in gpu.UPDATE_CASES:
        counts, rows, hint = gpu.LAYOUTS[c.layout]
        shape, grid = sr.update_form(64 * len(counts), hint)
        assert c.form == (c.rule, shape, c.chk, c.clip) and c.grid == grid, c.name
        assert max(counts) <= rows and max(counts) == hint, c.name
        forms.setdefault(c.form, []).append(c.name)
    want = {(r, s, chk, clip) for r in gpu.RULES for s in ("thread", "lanes8") for chk in (False, True) for clip in (False, True)}
    assert set(forms) == want and len(want) == 32, sorted(want - set(forms))
    assert gpu.FORM_CASES["update"] == {c.name: c.form for c in gpu.UPDATE_CASES}
    assert {c.layout for c in gpu.STRIDE_CASES} == {"stride_thread", "stride_lanes8"}
    assert all(c.grid == sr.GRID_CAP and 64 * len(gpu.LAYOUTS[c.layout][0]) > (1048576 if c.form[1] == "thread" else 131072)
               for c in gpu.STRIDE_CASES)
    assert gpu.LAYOUTS["thread"][0] == [3, 0, 1, 8, 16] and gpu.LAYOUTS["lanes8"][0] == [17, 0, 64, 65, 200, 1]
    assert set(gpu.FORM_CASES["slab_reduce"].values()) == {"thread", "lanes8"}
    for c in gpu.FILL_CASES:
        assert c.grid == sr.rng_fill_grid(c.total), c.name
    assert {"floor", "capped"} <= set(gpu.FORM_CASES["rng_fill"].values())
    assert any(c.grid == sr.GRID_CAP and c.total > 4 * 256 * sr.GRID_CAP for c in gpu.FILL_CASES)
    sb = {}
    for c in gpu.SB_CASES + [gpu.SB_CAP]:
        segs, total = gpu.SB_FILLS[c.fill]
        assert c.form == sr.step_begin_form(c.B, c.L, 0.0 if c.noise == "none" else gpu.NOISE_S, c.noise == "tape", len(segs)), c.name
        assert c.grid == sr.step_begin_grid(c.B, c.L, total), c.name
        sb.setdefault(c.form, []).append(c.name)
    want = {(g, n, f) for g in ("vector", "scalar") for n in ("generated", "tape", "none") for f in ("nofill", "lds", "global")}
    assert set(sb) == want, sorted(want - set(sb))
    grids = {c.grid for c in gpu.SB_CASES + [gpu.SB_CAP]}
    assert 64 in grids and 65 in grids and 1024 in grids
    assert {c.B for c in gpu.SB_CASES} == {2, 37} and {c.L for c in gpu.SB_CASES} == {6, 7, 8, 256}
    assert {c.goff for c in gpu.SB_CASES if c.noise == "gen"} == {0, 4 * 37}
    assert len(gpu.SB_FILLS["seg257"][0]) == 257 and {s[2] for s in gpu.SB_FILLS["seg3"][0]} == {0, 1, 2}
