"""``loss_reference`` against float64 torch autograd of the same composition (1e-12 relative), the masked rank loss
against ``partial_label_reference`` / ``partial_label_rows_reference``, the case tables of ``test_loss_kernels_gpu.py``
against the mirrored dispatch (every form named under "FORM -> CASE" there is reached by a case; a gap fails), and the
two input conditions the GPU tests rely on, checked on the reference alone."""
import collections
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import loss_reference as lr
import partial_label_reference as plref
import partial_label_rows_reference as plrows
import test_loss_kernels_gpu as tk
from oracle import ref_train
from oracle.ref_model import gaussian_taps

TOL = 1e-12


def close(a, b, what):
    a, b = np.asarray(a, np.float64), np.asarray(b.detach().numpy() if torch.is_tensor(b) else b, np.float64)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    err = float(np.abs(a - b).max()) if a.size else 0.0
    assert err <= TOL * (1.0 + float(np.abs(b).max() if b.size else 0.0)), f"{what}: {err:.3e}"


def T(a):
    return torch.tensor(np.asarray(a, np.float64), dtype=torch.float64)


# ---------------------------------------------------------------------------------------------------------- rank loss
@pytest.mark.parametrize("B,K", [(2, 1), (37, 3), (37, 16), (130, 5)])
@pytest.mark.parametrize("activate", [False, True])
def test_rank_reference_is_the_oracle(B, K, activate):
    d, z = tk.rank_data(f"cpu{B}", B, K, False, False)
    r = lr.rank_loss(d, z[:, :K], activate)
    zt = T(z[:, :K]).requires_grad_(True)
    loss = ref_train.kendall_constraint(T(d), zt, activate=activate)
    loss.backward()
    close([r["loss"]], [float(loss.detach())], "loss vs kendall_constraint")
    # ties (equal styles, different descriptors): autograd has the pair's sign, the closed form and the kernels do not
    assert B < 20 or r["P"].gzero.any(), "the data holds no tie"
    close(r["dz"] + lr.rank_tie_term(r["P"], r["norm"]), zt.grad, "dz + tie term vs autograd of kendall_constraint")
    l2, g2 = ref_train.kendall_closed_form(T(d), T(z[:, :K]), activate=activate)
    close([r["loss"]], [float(l2)], "loss vs kendall_closed_form")
    close(r["dz"], g2, "dz vs kendall_closed_form")
    # the counts are those of the definition, and the row blocks do not matter
    p = (z[:, None, :K] - z[None, :, :K]) * np.sign(d[:, None, :] - d[None, :, :])
    assert np.array_equal(r["P"].npos, (p > 0).sum((0, 1))) and np.array_equal(r["P"].nneg, (p < 0).sum((0, 1)))
    Q = lr.rank_pairs(d, z[:, :K], block=7)
    assert np.array_equal(Q.gpos, r["P"].gpos) and np.array_equal(Q.gneg, r["P"].gneg) and np.array_equal(Q.npos, r["P"].npos)
    assert np.array_equal(Q.gzero, r["P"].gzero)
    close(Q.spos, r["P"].spos, "S+ in other row blocks")


@pytest.mark.parametrize("B,K", [(37, 5), (130, 3), (2, 3)])
@pytest.mark.parametrize("activate", [False, True])
def test_masked_rank_reference(B, K, activate):
    d, z = tk.rank_data(f"cpum{B}", B, K, True, False)
    r = lr.rank_loss(d, z[:, :K], activate, masked=True)
    loss, grad = plref.masked_rank_loss(d, z[:, :K], activate)
    close([r["loss"]], [loss], "loss vs partial_label_reference")
    tie = lr.rank_tie_term(r["P"], r["norm"])
    close(r["dz"] + tie, grad, "dz + tie term vs partial_label_reference")
    assert np.array_equal(r["P"].m, np.isfinite(d).sum(0))
    # autograd of the same composition on the compacted rows of each descriptor
    zt = T(z[:, :K]).requires_grad_(True)
    tot = 0.0
    for k in range(K):
        rows = np.flatnonzero(np.isfinite(d[:, k]))
        if len(rows) >= 2:
            tot = tot + ref_train.kendall_constraint(T(d[rows, k:k + 1]), zt[rows, k:k + 1], activate=activate) / K
    if torch.is_tensor(tot):
        tot.backward()
        close([r["loss"]], [float(tot)], "loss vs autograd per descriptor")
        close(r["dz"] + tie, zt.grad, "dz + tie term vs autograd per descriptor")


@pytest.mark.parametrize("masked", [False, True])
def test_rank_rows_reference(masked):
    """The rows form: the ranks' totals add up to the whole batch's, and each rank's finish is its slice of the whole."""
    n, K, split = 40, 5, (1, 2, 37)
    d, z = tk.rank_data("cpurows", n, K, masked, False)
    whole = lr.rank_loss(d, z[:, :K], True, masked)
    row0, tot, Ps = 0, 0.0, []
    for nrows in split:
        P = lr.rank_pairs(d, z[:, :K], masked, row0, nrows)
        if masked:
            close(P.totals(True)[:, :K], plrows.masked_rank_rows(d, z[:, :K], row0, nrows), "totals vs partial_label_rows_reference")
        tot = tot + P.totals(masked)
        Ps.append((row0, nrows, P))
        row0 += nrows
    assert np.array_equal(tot[:2], whole["P"].totals(masked)[:2])
    for row0, nrows, P in Ps:
        r = lr.rank_finish(tot, P, n, True, masked, scale=3.0)
        close([r["loss"]], [whole["loss"]], "every rank's loss is the whole batch's")
        close(r["dz"], 3.0 * whole["dz"][row0:row0 + nrows], "a rank's dz is its slice")
        if masked:
            l2, g2 = plrows.finish(tot[:, :K], d, z[:, :K], row0, nrows, True)
            close([r["loss"]], [l2], "loss vs partial_label_rows_reference.finish")
            close(r["dz"] + lr.rank_tie_term(P, r["norm"], 3.0), 3.0 * g2, "dz + tie term vs partial_label_rows_reference.finish")


@pytest.mark.parametrize("masked", [False, True])
def test_scaled_columns_reference(masked):
    """``rank_pairs_scaled`` (one column's pair pass for the 8184 .. 16392-row cases) is ``rank_pairs`` on such a batch."""
    d, z = tk.rank_data("cpuscaled", 300, 16, masked, True)
    assert len(set(abs(f) for f in tk.BIG_FACTORS)) == 16 and any(f < 0 for f in tk.BIG_FACTORS)
    assert np.array_equal(z[:, :16], (z[:, :1] / tk.BIG_FACTORS[0]) * np.array(tk.BIG_FACTORS)[None, :])
    P = lr.rank_pairs(d, z[:, :16], masked)
    Q = lr.rank_pairs_scaled(d[:, 0], z[:, 0] / tk.BIG_FACTORS[0], tk.BIG_FACTORS, masked, block=64)
    for a in ("npos", "nneg", "m", "gpos", "gneg", "gzero"):
        assert np.array_equal(getattr(P, a), getattr(Q, a)), a
    close(Q.spos, P.spos, "S+")
    close(Q.sneg, P.sneg, "S-")
    assert (P.npos[0] != P.nneg[0]) and P.npos[1] == P.nneg[0], "a negative factor swaps n+ and n-"


# ------------------------------------------------------------------------------------------------- recon, smooth, MSE
@pytest.mark.parametrize("c", tk.RECON_CASES[:7], ids=lambda c: c.name)
def test_recon_reference(c):
    x, y = tk.recon_data(c)
    r = lr.recon_loss(x, y, c.scale)
    yt = T(y).requires_grad_(True)
    loss = ref_train.recon_loss(T(x), yt, scale=c.scale)
    loss.backward()
    close([r["loss"]], [float(loss)], "loss")
    close(r["dy"], yt.grad, "dy")


@pytest.mark.parametrize("kind,L", [("g17", 2), ("g17", 5), ("g17", 9), ("g17", 20), ("g17", 70), ("g3", 2), ("g33", 7),
                                    ("g33", 40), ("g1", 7)])
def test_smooth_reference(kind, L):
    x = tk.smooth_data(tk.SmoothCase(f"cpu{kind}{L}", 5, L, kind))
    taps = tk.taps_of(kind)
    loss, dx = lr.smooth_loss(x, taps)
    xt = T(x).requires_grad_(True)
    want = ref_train.smoothness_loss(xt, len(taps))
    want.backward()
    assert np.array_equal(taps, gaussian_taps(len(taps), 3.0).double().numpy())
    close([loss], [float(want)], "loss")
    close(dx, xt.grad, "dx")


def test_smooth_reference_asymmetric_taps():
    """Taps that are not symmetric, against F.pad / F.conv1d (cross-correlation: tap t meets x[l + t - half])."""
    taps = tk.taps_of("asym5")
    assert not np.allclose(taps, taps[::-1])
    for L in (2, 7, 40):
        x = tk.smooth_data(tk.SmoothCase(f"cpuasym{L}", 5, L, "asym5"))
        loss, dx = lr.smooth_loss(x, taps)
        xt = T(x).requires_grad_(True)
        sm = F.conv1d(F.pad(xt.unsqueeze(1), (2, 2), mode="replicate"), T(taps).view(1, 1, -1)).squeeze(1)
        want = F.mse_loss(xt, sm)
        want.backward()
        close([loss], [float(want)], "loss")
        close(dx, xt.grad, "dx")


def test_mse_bce_finalize_reference():
    g = np.random.default_rng(3)
    a, b = g.standard_normal(301), g.standard_normal(301)
    at = T(a).requires_grad_(True)
    want = F.mse_loss(at, T(b))
    want.backward()
    loss, da = lr.mse(a, b)
    close([loss], [float(want)], "mse")
    close(da, at.grad, "mse da")
    for n_real, n_fake in tk.BCE_CASES:
        o = tk.bce_data(n_real, n_fake)
        ot = T(o).requires_grad_(True)
        want = F.binary_cross_entropy_with_logits(ot[:n_real], torch.ones(n_real, dtype=torch.float64)) + \
            F.binary_cross_entropy_with_logits(ot[n_real:], torch.zeros(n_fake, dtype=torch.float64))
        want.backward()
        loss, d = lr.bce_pair(o, n_real)
        close([loss], [float(want)], "bce")
        close(d, ot.grad, "bce dlogits")
        assert set(np.abs(o)) >= ({104.0} if n_real == 1 else set(np.abs(tk.BCE_EDGE[:3])))
    assert set(np.abs(tk.bce_data(256, 36))) >= set(np.abs(tk.BCE_EDGE)), "every edge logit is in a case"
    p = [1e16, 1.0, -1e16, 1e-3]
    assert lr.finalize(p, 2.0) == 2.002 and float(np.sum(p)) != 1.001


# ---------------------------------------------------------------------------------------------------- style BatchNorm
@pytest.mark.parametrize("B,Cc,nparts", [(2, 1, 1), (37, 13, 3), (37, 64, 512)])
def test_style_bn_reference(B, Cc, nparts):
    z, rows, run, dy = tk.style_data(f"cpu{B}", B, Cc, nparts)
    y, new = lr.style_bn_fwd(z, rows, B, run)
    zt = T(z).requires_grad_(True)
    rm, rv = T(run[0]).clone(), T(run[1]).clone()
    yt = F.batch_norm(zt, rm, rv, training=True, momentum=lr.MOMENTUM, eps=lr.EPS)
    (yt * 2.0 * T(dy)).sum().backward()
    close(y, yt, "train forward")
    close(new[0], rm, "running mean")
    close(new[1], rv, "running var")
    rstd = lr.bn_stats(rows, B)[1]
    close(lr.style_bn_bwd(dy, y, rstd, 2.0), zt.grad, "backward with scale")
    ye, none = lr.style_bn_fwd(z, None, 0, run)
    assert none is None and lr.style_bn_fwd(z, rows, B)[1] is None
    close(ye, F.batch_norm(T(z), T(run[0]), T(run[1]), training=False, eps=lr.EPS), "eval forward")


# ------------------------------------------------------------------------------------------------------ discriminator
@pytest.mark.parametrize("name", ["dv_1_1_1", "dv_40_23_6", "dv_17_15_13_bare"])
def test_disc_reference(name):
    c = tk.DISC_BY_NAME[name]
    t = tk.disc_data(name)
    lin = [torch.nn.Linear(c.ns, 64), torch.nn.Linear(64, 64), torch.nn.Linear(64, 1)]
    pre = [torch.nn.PReLU(64), torch.nn.PReLU(64)]
    for m in lin + pre:
        m.double()
    with torch.no_grad():
        for i, l in enumerate(lin):
            l.weight.copy_(T(t[f"w{i + 1}"]))
            l.bias.copy_(T(t[f"b{i + 1}"]))
        for i, q in enumerate(pre):
            q.weight.copy_(T(t[f"s{i + 1}"]))
    styles = T(t["styles"]).requires_grad_(True)
    x = torch.cat([T(t["z_real"]), styles])
    if t["noise"] is not None:
        x = x + float(lr.f32(tk.SIGMA)) * T(t["noise"])
    h = x
    for i in range(2):
        h = pre[i](lin[i](h))
        if t[f"m{i + 1}"] is not None:
            h = h * T(t[f"m{i + 1}"])
    o = lin[2](h).squeeze(1)
    loss = F.binary_cross_entropy_with_logits(o[:c.n_real], torch.ones(c.n_real, dtype=torch.float64)) + \
        F.binary_cross_entropy_with_logits(o[c.n_real:], torch.zeros(c.n_fake, dtype=torch.float64))
    loss.backward()
    r = t["ref"]
    close([r["loss"]], [float(loss)], "loss")
    close(r["dstyles"], -float(lr.f32(tk.ALPHA)) * styles.grad, "dstyles")
    for k, p in zip(tk.DISC_PARAMS, (lin[0].weight, lin[0].bias, pre[0].weight, lin[1].weight, lin[1].bias, pre[1].weight,
                                     lin[2].weight, lin[2].bias)):
        close(r["d" + k].reshape(p.shape), p.grad, "d" + k)


# ------------------------------------------------------------------------------------------------ input conditions
def test_disc_cases_near_zero_cap():
    """The cases up to 63 rows have no row with a near-zero hidden pre-activation (nothing is excused there); the
    larger ones at most 1 %."""
    for c in tk.DISC_CASES:
        near = tk.disc_data(c.name)["near"]
        if c.n_real + c.n_fake <= 63:
            assert not near.any(), (c.name, np.flatnonzero(near))
        else:
            assert near.sum() <= 0.01 * len(near), (c.name, int(near.sum()))


def test_recon_cases_keep_the_means_away_from_zero():
    """sign(mean) is discontinuous at 0: no flexible-target case has a row mean with |mean| < 0.05; and the rows the
    issue names are there: ratio below 0.7, above 1.3, strictly inside, a negative output mean, a negative input mean."""
    seen = set()
    for c in tk.RECON_CASES + [tk.ReconCase(f"pl_recon{i}", 7, 65, True) for i in range(2)]:
        if not c.scale:
            continue
        x, y = tk.recon_data(c)
        r = lr.recon_loss(x, y, True)
        assert np.abs(r["mx"]).min() >= 0.05 and np.abs(r["my"]).min() >= 0.05, (c.name, np.abs(r["mx"]).min(), np.abs(r["my"]).min())
        if c.B >= 5:
            have = {"low": (r["r"] < 0.7).any(), "high": (r["r"] > 1.3).any(), "inside": ((r["r"] > 0.7) & (r["r"] < 1.3)).any(),
                    "neg_out": (r["my"] < 0).any(), "neg_in": (r["mx"] < 0).any()}
            assert all(have.values()), (c.name, have)
            seen |= set(have)
    assert len(seen) == 5


# ------------------------------------------------------------------------------------------------ mirror and table
def test_mirror_of_the_dispatch():
    assert lr.rank_grid(1030, 1030, 1) == (4, 4, 512, 36)
    assert lr.rank_grid(4096, 4096, 5) == (4, 6, 768, 171 * 6)          # the figures in raae_loss.hip's comment
    assert lr.rank_grid(8192, 8192, 16) == (4, 1, 8192, 1024)
    assert lr.rank_grid(8184, 8184, 16) == (4, 2, 4096, 2046)
    assert lr.rank_grid(16392, 16392, 16) == (4, 1, 16640, 2048)
    assert lr.rank_grid(1030, 515, 3) == (1, 4, 512, 52 * 4)
    assert lr.rank_grid(37, 37, 7) == (1, 1, 256, 10)
    assert (lr.recon_nparts(1), lr.recon_nparts(2049), lr.mse_nparts(512 * 1024 + 3), lr.mse_nparts(1)) == (1, 512, 512, 1)
    assert lr.disc_instance(1000, 1047) == ("valu", 128) and lr.disc_instance(1000, 1048) == ("mfma", 128)
    assert lr.disc_instance(2056, 2057) == ("mfma", 256) and lr.disc_instance(1, 1) == ("valu", 1)
    assert lr.disc_instance(1, 1, force=1) == ("mfma", 1) and lr.disc_instance(2056, 2057, force=0) == ("valu", 256)
    assert lr.disc_instance(1000, 1048, force=-1) == ("mfma", 128)
    assert lr.smooth_instance(17) == "taps17" and lr.smooth_instance(33) == "generic"
    assert lr.smooth_lds_bytes(2048) > 65536 and lr.smooth_lds_bytes(4096) < 163840


def test_case_table_reaches_every_form():
    """Recomputes FORM -> CASE from the mirror and fails on a gap."""
    forms = {}
    for c in tk.RANK_CASES + tk.BIG_RANK_CASES:
        forms[c.name] = lr.rank_form(c.B, c.B, c.K, c.masked)
    for c in tk.ROWS_CASES:
        for i, nrows in enumerate(c.split):
            forms[f"{c.name}#{i}"] = lr.rank_form(c.n_all, nrows, c.K, c.masked)
    have = collections.defaultdict(list)
    for name, f in forms.items():
        have[(f["KA"], f["R"], f["masked"])].append(name)
    # R = 1: all 16 KA, masked and not
    for K in range(1, 17):
        for m in (False, True):
            assert have[(K, 1, m)], f"rank_pairs_body<{K}, 1, {m}> has no case"
    # R = 4: all 16 KA, masked and not, each with column blocks
    for K in range(1, 17):
        for m in (False, True):
            names = have[(K, 4, m)]
            assert any(forms[n]["multi_block"] for n in names), f"rank_pairs_body<{K}, 4, {m}> has no case with column blocks"
    r4 = [f for f in forms.values() if f["R"] == 4]
    r1 = [f for f in forms.values() if f["R"] == 1]
    assert any(f["nj"] == 1 for f in r4) and any(f["nj"] == 2 for f in r4), "R = 4 with nj = 1 and nj = 2"
    assert any(f["stride"] and not f["masked"] for f in r4) and any(f["stride"] and f["masked"] for f in r4), "grid stride"
    assert any(f["empty_block"] and f["KA"] == 1 for f in r4), "an empty column block"
    assert forms["r4_1030_k1_u"]["empty_block"] and forms["r4_1030_k1_m"]["empty_block"]
    assert any(f["multi_block"] for f in r1), "R = 1 with nj > 1 (the rows form)"
    assert any(f["idle_slots"] == 4 for f in forms.values()) and any(f["idle_slots"] == 2 for f in forms.values())
    for B in (2, 255, 256, 257, 513):
        for K in (3, 7):
            assert f"tile{B}_k{K}_u" in forms and f"tile{B}_k{K}_m" in forms
    assert forms["big_8192"]["nj"] == 1 and forms["big_8184"]["nj"] == 2 and forms["big_16392_u"]["stride"]
    assert not forms["big_8192"]["stride"] and not forms["big_8184"]["stride"]
    # recon / smooth / mse / disc / style
    assert {(c.scale, lr.recon_nparts(c.B) * 4 < c.B) for c in tk.RECON_CASES} == {(False, False), (True, False), (False, True), (True, True)}
    inst = {(lr.smooth_instance(len(tk.taps_of(c.taps))), lr.smooth_nparts(c.B) * 4 < c.B) for c in tk.SMOOTH_CASES}
    assert ("taps17", True) in inst and ("taps17", False) in inst and ("generic", False) in inst
    assert {len(tk.taps_of(c.taps)) for c in tk.SMOOTH_CASES} == {1, 3, 5, 15, 17, 33}
    assert any(c.L < 8 for c in tk.SMOOTH_CASES if c.taps == "g17"), "L shorter than the half window"
    assert any(n > lr.MAX_PARTS * 1024 for n in tk.MSE_SIZES), "mse grid stride"
    d = {lr.disc_instance(c.n_real, c.n_fake)[0]: [] for c in tk.DISC_CASES}
    for c in tk.DISC_CASES:
        d[lr.disc_instance(c.n_real, c.n_fake)[0]].append(c)
        assert c.name.startswith("dm_") == (lr.disc_instance(c.n_real, c.n_fake)[0] == "mfma"), c.name
    assert any(c.n_real + c.n_fake == 2047 for c in d["valu"]) and any(c.n_real + c.n_fake == 2048 for c in d["mfma"])
    assert any((c.n_real + c.n_fake + 15) // 16 > lr.DISC_MAXWG for c in d["mfma"]), "tiles stride"
    assert any(c.n_real % 16 for c in d["mfma"]), "the real / fake boundary inside a tile"
    assert any(c.B * c.C > 65536 for c in tk.STYLE_FWD) and {c.mode for c in tk.STYLE_FWD} == {"train", "train_u", "eval"}
    assert {c.nparts for c in tk.STYLE_FWD} == {1, 3, 512} and {c.C for c in tk.STYLE_FWD} == {1, 6, 13, 16, 64}
    for Cc in (6, 13, 64):
        n = 1024 // Cc
        assert {4 * n - 1, 4 * n, 4 * n + 1} <= {c.B for c in tk.STYLE_BWD if c.C == Cc}
    # every case name pattern of the docstring's table matches a case, and every case is named by a pattern
    table = tk.__doc__.split("FORM -> CASE")[1]
    names = ([c.name for c in tk.RANK_CASES + tk.BIG_RANK_CASES + tk.ROWS_CASES + tk.RECON_CASES + tk.SMOOTH_CASES +
              tk.STYLE_FWD + tk.STYLE_BWD + tk.DISC_CASES] + list(tk.PLANES))
    for prefix in ("ka", "tile", "r4_", "big_", "rows_", "rc_", "sm17_", "smg_", "sf_", "sb_", "dv_", "dm_", "pl_"):
        assert re.search(r"\b" + prefix, table), prefix
        assert any(n.startswith(prefix) for n in names), prefix
    assert all(re.match(r"(ka|tile|r4_|big_|rows_|rc_|sm17_|smg_|sf_|sb_|dv_|dm_|pl_)", n) for n in names)
    assert len(set(names)) == len(names)

