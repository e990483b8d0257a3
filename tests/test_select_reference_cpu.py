"""``select_reference`` against the libraries the reference calls (scipy, numpy, scikit-learn), the golden fixtures of
the real reference, the case table of ``test_select_kernels_gpu.py`` against the mirrored dispatch (a form without a case
fails), and -- before anything runs on a GPU -- that the float64 restatement alone sits inside every bound the GPU tests
apply."""
import itertools
import json
import os
import re
import warnings

import numpy as np
import pytest
from numpy.polynomial import Polynomial
from scipy import stats

import select_reference as sr
import test_select_kernels_gpu as tk

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "selection_ref.json")
FLOAT_CASES = [c.name for c in tk.CASES]


def _xy(n, seed, ties=True):
    g = np.random.default_rng(seed)
    x = g.standard_normal(n)
    if ties:
        x = np.round(x * 4.0) / 4.0
    y = (x + 0.2 * x * x + 0.5 * g.standard_normal(n)).astype(np.float32)
    return x, y


# ------------------------------------------------------------------------------------------------ pieces vs libraries
@pytest.mark.parametrize("n", [3, 37, 2049, 4099])
def test_ranks_are_rankdata(n):
    x, y = _xy(n, n)
    assert np.array_equal(sr.avg_rank(x), stats.rankdata(x, method="average"))
    assert np.array_equal(sr.avg_rank(y), stats.rankdata(y, method="average"))
    m = x.copy()
    m[::3] = np.inf                                   # unlabelled rows stand above every labelled one
    lab = np.isfinite(m)
    assert np.array_equal(sr.avg_rank(m)[lab], stats.rankdata(m[lab], method="average"))


@pytest.mark.parametrize("n", [3, 37, 2049, 4099])
def test_descriptor_stats_are_scipy_and_numpy(n):
    x, y = _xy(n, 100 + n, ties=n > 3)
    st = sr.descriptor_stats(x, y)
    f, y64 = st["f64"], y.astype(np.float64)
    assert abs(f[0] - stats.spearmanr(x, y64).correlation) <= 1e-13
    lin = stats.linregress(x, y64)
    assert abs(f[1] - lin.slope) <= 1e-13 and abs(f[2] - lin.intercept) <= 1e-13 and abs(f[3] - lin.rvalue ** 2) <= 1e-13
    p, info = Polynomial.fit(x, y64, 2, full=True)
    assert np.abs(np.array([f[4], f[5], f[6]]) - p.convert().coef).max() <= 1e-13 and info[1] == st["rank"] == 3
    if n > 3:                                         # (lstsq returns no residual for a square system)
        assert abs(f[7] - info[0][0] / n) <= 1e-13
    assert abs(f[8] - stats.linregress(p(x), y64).rvalue ** 2) <= 1e-13
    for s in range(9):                                # the high-precision form is the same quantity
        assert abs(f[s] - st["hp"][s]) <= 1e-11 * max(1.0, sr.slot_scale(s, f)), (s, f[s], st["hp"][s])


def test_two_valued_descriptor_is_the_rank_two_fit():
    """What the reference does there: rank 2, an EMPTY residual array, the minimum-norm coefficients -- on the mapped
    variable a1 = (mean_hi - mean_lo) / 2, a0 = a2 = (mean_hi + mean_lo) / 4."""
    g = np.random.default_rng(5)
    x = (g.random(37) < 0.4).astype(np.float64)
    y = (0.7 * x + g.standard_normal(37)).astype(np.float32)
    y64 = y.astype(np.float64)
    p, info = Polynomial.fit(x, y64, 2, full=True)
    assert info[1] == 2 and info[0].size == 0
    hi, lo = y64[x == 1].mean(), y64[x == 0].mean()
    assert np.abs(p.coef - [(hi + lo) / 4, (hi - lo) / 2, (hi + lo) / 4]).max() <= 1e-14
    st = sr.descriptor_stats(x, y)
    assert st["rank"] == 2
    assert np.abs(np.array([st["f64"][s] for s in (4, 5, 6)]) - p.convert().coef).max() <= 1e-13
    assert np.abs(np.array([st["hp"][s] for s in (4, 5, 6)]) - p.convert().coef).max() <= 1e-13
    assert abs(st["f64"][0] - stats.spearmanr(x, y64).correlation) <= 1e-13
    assert abs(st["f64"][8] - stats.linregress(p(x), y64).rvalue ** 2) <= 1e-13
    assert abs(st["f64"][7] - np.mean((y64 - p(x)) ** 2)) <= 1e-13 and abs(st["hp"][7] - st["f64"][7]) <= 1e-13


def test_constant_columns_as_scipy_sees_them():
    g = np.random.default_rng(6)
    y = g.standard_normal(37).astype(np.float32)
    x = np.full(37, 1.25)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        assert np.isnan(stats.spearmanr(x, y).correlation)
        with pytest.raises(ValueError):
            stats.linregress(x, y.astype(np.float64))
    st = sr.descriptor_stats(x, y)
    assert st["rank"] == 1 and np.isnan(st["f64"][0]) and np.isnan(st["hp"][0])
    # a constant style: its rho against the last style is NaN and does not take part in the maximum
    z = g.standard_normal((37, 4)).astype(np.float32)
    z[:, 1] = 0.5
    rk = np.stack([sr.avg_rank(z[:, c]) for c in range(4)])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        rho = [stats.spearmanr(z[:, c], z[:, 3]).correlation for c in range(3)]
    assert np.isnan(rho[1])
    assert abs(sr.inter_style(rk)[0] - max(abs(rho[0]), abs(rho[2]))) <= 1e-13


@pytest.mark.parametrize("kind", ["three", "two", "outside", "frac", "four"])
def test_confusion_and_f1_are_sklearn(kind):
    from sklearn.metrics import confusion_matrix, f1_score
    name = {"three": "sw_257", "two": "cls_two", "outside": "cls_outside", "frac": "cls_frac", "four": "cls_four"}[kind]
    z, aux, si, so, th = tk.case_data(name)
    R = tk.case_ref(name)
    cls = (aux[:, 1] - 4).astype(int)
    assert np.array_equal(cls, sr.cn_class(aux[:, 1]))
    o = R["block"][sr.HEAD + sr.STRIDE:sr.HEAD + 2 * sr.STRIDE]
    if kind == "four":
        assert len(set(cls)) == 4 and R["distinct"] == 4 and not o.any()
        return
    assert len(set(cls)) == R["distinct"] <= 3
    if kind == "outside":
        assert cls.min() < 0 and cls.max() > 2
    if kind == "frac":
        assert {3.5, 4.5} <= set(aux[:, 1]) and set(cls[(aux[:, 1] == 3.5) | (aux[:, 1] == 4.5)]) == {0}
    z1 = z[:, 1].astype(np.float64)
    f4 = [f1_score(z1 < t, cls < 1, zero_division=0) for t in th]
    f6 = [f1_score(z1 > t, cls > 1, zero_division=0) for t in th]
    for s, f in enumerate((f4, f6)):
        assert np.array_equal(np.array([float(q) for q in sr.quotients(R["sweep"][s])]), np.array(f))
    i45, i56 = int(np.argmax(f4)), int(np.argmax(f6))
    assert (o[2], o[3], o[4], o[5]) == (i45, i56, th[i45], th[i56])
    pred = (z1 > th[i45]).astype(int) + (z1 > th[i56]).astype(int)
    assert np.array_equal(o[6:15].reshape(3, 3), confusion_matrix(cls, pred, labels=[0, 1, 2]))
    want = f1_score(cls, pred, average="weighted", zero_division=0)
    assert abs(o[1] - want) <= 1e-15 and abs(R["block_hp"][sr.HEAD + sr.STRIDE + 1] - want) <= 1e-15


def test_argmax_tables_hold_what_they_are_built_for():
    """Exact ties of the maximum in different threads' strides and different halves of the reduction tree, zero
    denominators, and two different fractions of one value; ``first_argmax`` is ``numpy.argmax`` of the quotients."""
    seen = set()
    for c in tk.CASES:
        if c.n_aux < 2 or c.masked:
            continue
        R = tk.case_ref(c.name)
        for s in range(2):
            q = sr.quotients(R["sweep"][s])
            assert sr.first_argmax(R["sweep"][s]) == int(np.argmax([float(v) for v in q])), (c.name, s)
            top = [t for t, v in enumerate(q) if v == max(q)]
            if len(top) > 1:
                seen.add("tie")
                if len({t % 256 for t in top}) > 1:
                    seen.add("strides")
                if len({(t % 256) < 128 for t in top}) > 1:
                    seen.add("halves")
                if len({t // 256 for t in top}) > 1:
                    seen.add("within a stride")
                if len({tuple(R["sweep"][s][t]) for t in top}) > 1 and max(q) > 0:
                    seen.add("2/4 = 4/8")
            if (R["sweep"][s][:, 1] == 0).any():
                seen.add("0/0")
    assert seen == {"tie", "strides", "halves", "within a stride", "2/4 = 4/8", "0/0"}, seen
    o = tk.case_ref("sw_craft")["sweep"][0]
    top = {tuple(o[t]) for t in range(len(o)) if sr.quotients(o)[t] == max(sr.quotients(o))}
    assert top == {(2, 4), (4, 8)}, top


@pytest.mark.parametrize("n,k,extra", [(3, 2, ""), (37, 3, ""), (258, 2, ""), (2049, 2, ""), (37, 3, "const"), (257, 3, "tiny")])
def test_style_metrics_reference_is_scipy(n, k, extra):
    from rankaae_amd.metrics import shapiro_coefficients
    z = tk.sm_data(n, k, extra)
    R = sr.style_metrics_ref(z, shapiro_coefficients(n))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        W = np.array([stats.shapiro(z[:, c]).statistic for c in range(k)])
        rho = np.array([stats.spearmanr(z[:, p], z[:, q]).correlation for p, q in itertools.combinations(range(k), 2)])
    assert np.abs(R["W"] - W).max() <= 1e-13 and np.abs(R["W_hp"] - W).max() <= 1e-11
    assert np.array_equal(np.isnan(R["rho"]), np.isnan(rho)) and np.array_equal(np.isnan(R["rho_hp"]), np.isnan(rho))
    ok = ~np.isnan(rho)
    assert ok.all() or extra == "const"
    if ok.any():
        assert np.abs(R["rho"][ok] - rho[ok]).max() <= 1e-13 and np.abs(R["rho_hp"][ok] - rho[ok]).max() <= 1e-13
    if extra == "const":
        assert R["W"][1] == 1.0 and W[1] == 1.0
    for c in range(k):
        assert np.array_equal(R["rank"][c], stats.rankdata(z[:, c], method="average"))
        assert np.array_equal(R["sorted"][c], np.sort(z[:, c].astype(np.float64) - float(z[n // 2, c])))


def test_mae_cases_tell_an_fp32_difference_from_a_double_one():
    """sklearn's mean_absolute_error sees fp32 arrays: the difference is an fp32 one.  Every MAE case has rows where that
    rounds, so a difference taken in double gives another per-row value, far outside the bound."""
    from sklearn.metrics import mean_absolute_error
    for c in tk.CASES:
        z, aux, si, so, th = tk.case_data(c.name)
        mae, exact = sr.mae_rows(si, so)
        dbl = np.abs(so.astype(np.float64) - si.astype(np.float64)).mean(axis=1)
        far = np.abs(dbl - mae) > 1e3 * np.array([sr.bound(m, m, float(e)) for m, e in zip(mae, exact)])
        assert (far.any() or c.n * c.L < 64) and (c.L < 32 or far.mean() > 0.5), (c.name, far.mean())
        for r in range(min(c.n, 5)):
            assert abs(mae[r] - float(mean_absolute_error(si[r], so[r]))) <= 2.0 ** -22 * mae[r]     # (sklearn's mean is an fp32 one)


def test_group_mean_reference():
    x = tk.gm_data(37, 7, 65)
    want = x.astype(np.float64).mean(axis=1)
    assert np.abs(sr.group_mean_exact(x, 37, 7, 65) - want).max() <= 1e-15 * np.abs(want).max()
    assert sr.ulp32(1.0) == 2.0 ** -23 and sr.ulp32(-3.0) == 2.0 ** -22


# ------------------------------------------------------------------------------------------------------- masked form
@pytest.mark.parametrize("name", [c.name for c in tk.CASES if c.masked])
def test_masked_reference_is_the_unmasked_one_on_the_labelled_rows(name):
    z, aux, si, so, th = tk.case_data(name)
    R = tk.case_ref(name)
    c = tk.BY_NAME[name]
    full = np.where(np.isnan(aux), 5.0, aux)
    assert np.array_equal(R["block"][:sr.HEAD], sr.select_ref(z, full, si, so, th)["block"][:sr.HEAD]), "the head uses all rows"
    counts = set()
    for i in range(c.n_aux):
        rows = np.flatnonzero(np.isfinite(aux[:, i]))
        counts.add(len(rows))
        sl = slice(sr.HEAD + sr.STRIDE * i, sr.HEAD + sr.STRIDE * (i + 1))
        if len(rows) < 3:
            assert not R["block"][sl].any()
            continue
        a2 = np.zeros((len(rows), c.n_aux))
        a2[:, i] = aux[rows, i]
        if c.n_aux > 1 and i != 1:
            a2[:, 1] = 5.0
        U = sr.select_ref(z[rows], a2, si[rows], so[rows], th)
        assert np.array_equal(R["block"][sl], U["block"][sl], equal_nan=True), i
        if i == 1:
            assert np.array_equal(R["sweep"], U["sweep"])
        else:
            assert np.array_equal(R["rank_d"][i][rows], U["rank_d"][i]) and np.array_equal(R["rank_zs"][i][rows], U["rank_z"][i])
    if c.n_aux >= 5:
        assert {2, 3} <= counts
    elif c.n_aux >= 3:
        assert 3 in counts
    if c.n > 2048:
        assert (~np.isfinite(aux[2040:2048])).any() and (~np.isfinite(aux[2048:2060])).any(), "unlabelled rows on both sides of index 2048"


# ---------------------------------------------------------------------------------------------------- golden fixtures
@pytest.mark.parametrize("name", ["main", "small"])
def test_restatement_reproduces_the_reference_fixtures(name):
    """All 8 + n jobs of both cases of ``selection_ref.json`` through ``report.result_from_block`` and the comparison
    rule of ``test_report_gpu.py``."""
    from rankaae_amd import report
    from rankaae_amd.synthetic import selection_inputs
    import test_report_gpu as tr
    with open(GOLDEN) as f:
        case = {c["name"]: c for c in json.load(f)["cases"]}[name]
    inputs = selection_inputs(case["seed"], case["n_jobs"], case["n_rows"], case["nstyle"], case["n_aux"], case["n_points"],
                              case["four_class_job"])
    assert np.array_equal(tk.THRESH_GRID, report.THRESH_GRID)
    blocks = [sr.select_ref(*x, report.THRESH_GRID)["block"] for x in inputs]
    tr._check_blocks(case, blocks)


# ------------------------------------------------------------------------------------------------ bounds, before the GPU
@pytest.mark.parametrize("name", FLOAT_CASES)
def test_restatement_alone_is_inside_every_bound(name):
    """A case too ill-conditioned to pin would be thrown out HERE (none is): the float64 restatement's distance from the
    high-precision form is at most 1/16 of its bound by construction, so what this asserts is that the bound is a
    usable one -- no slot's bound above 1e-9 of its scale -- and that both forms are finite where a number is due."""
    R = tk.case_ref(name)
    c = tk.BY_NAME[name]
    for j, cls in enumerate(R["cls"]):
        if cls is None:
            assert R["block"][j] == R["block_hp"][j]
            continue
        d = (j - sr.HEAD) // sr.STRIDE
        if j >= sr.HEAD and R["lstsq_rank"].get(d) == 1:
            assert c.deg == "constdesc" and d == 0
            continue
        if np.isnan(R["block"][j]):
            assert c.deg == "conststyle" and np.isnan(R["block_hp"][j]), (name, j, cls)
            continue
        assert abs(R["block"][j] - R["block_hp"][j]) <= R["tol"][j], (name, j, cls)
        assert R["tol"][j] <= 1e-9 * max(R["scale"][j], 1e-300), \
            f"{name}: slot {j} ({cls}) is too ill-conditioned to pin: bound {R['tol'][j]:.2e} at scale {R['scale'][j]:.2e}"
        if cls == "residue" and R["m"][d] > 3:
            y = tk.case_data(name)[0][:, d].astype(np.float64)
            assert R["block"][j] >= 2.0 ** -20 * np.mean(y * y), \
                f"{name}: the residue of descriptor {d} is rounding noise of an exact fit, not a number to pin"


def test_degenerate_cases_are_what_they_claim():
    assert tk.case_ref("deg_two37")["lstsq_rank"][0] == 2 and tk.case_ref("deg_two2049")["lstsq_rank"][0] == 2
    assert tk.case_ref("deg_constdesc")["lstsq_rank"][0] == 1 and np.isnan(tk.case_ref("deg_constdesc")["block"][sr.HEAD])
    z = tk.case_data("deg_conststyle")[0]
    assert np.ptp(z[:, 4]) == 0.0 and tk.case_ref("deg_conststyle")["block"][2] > 0.0
    for name in ("tile2049", "tile4099"):
        z, aux = tk.case_data(name)[:2]
        assert np.ptp(z[2040:2060, 0]) == 0.0 and np.ptp(aux[2040:2060, 0]) == 0.0, "a run of equal values across 2048"


# ------------------------------------------------------------------------------------------------ mirror and table
def test_mirror_of_the_host_side():
    assert sr.select_work_bytes(1000, 6, 5, 700) == sr.align256(8 * 1000 * 12) + sr.align256(16 * 700) == 96000 + 11264
    assert sr.select_masked_work_bytes(40, 6, 5, 700) == sr.align256(8 * 40 * 17) + 11264
    lay = sr.work_layout(37, 3, 3, 5)
    assert lay["rank_z"][0] == 0 and lay["rank_d"][0] == 8 * 37 * 3 and lay["mae"][0] == 8 * 37 * 6
    assert lay["sweep"][0] == sr.align256(8 * 37 * 7) and lay["bytes"] == sr.select_work_bytes(37, 3, 3, 5)
    laym = sr.work_layout(37, 3, 3, 5, masked=True)
    assert laym["rank_zs"][0] == 8 * 37 * 7 and laym["bytes"] == sr.select_masked_work_bytes(37, 3, 3, 5)
    w = sr.written_bytes(37, 3, 3, 5)
    assert not w[8 * 37 * 4:8 * 37 * 5].any() and w[:8 * 37 * 4].all() and w[8 * 37 * 5:8 * 37 * 7].all()
    assert not sr.written_bytes(5, 2, 1, 0).reshape(-1)[8 * 5 * 4:].any()
    assert sr.grids(2049, 3, 3, 5) == {"rank": (9, 6, 1), "mae": (513, 1, 1), "sweep": (5, 2, 1), "stat": (5, 1, 1)}
    assert sr.grids(41, 64, 1, 0)["sweep"] is None and sr.grids(41, 6, 5, 5, masked=True)["rank"] == (1, 16, 1)
    assert (sr.HEAD, sr.STRIDE) == (4, 16)
    assert sr.group_mean_grid(2049, 257) == 2048 and sr.group_mean_grid(37, 65) == 10
    assert sr.style_metrics_grids(41, 64)["stat"] == (2080, 1, 1) and sr.style_metrics_grids(41, 1)["stat"] == (1, 1, 1)


def test_case_table_reaches_every_form():
    """Recomputes FORM -> CASE from the mirror and fails on a gap."""
    forms = {c.name: sr.form(c.n, c.k, c.n_aux, c.L, c.th, c.masked) for c in tk.CASES}
    un = [f for n, f in forms.items() if not f["masked"]]
    ma = [f for n, f in forms.items() if f["masked"]]
    assert {c.n for c in tk.CASES if c.name.startswith("tile") and not c.masked} == {3, 4, 37, 255, 256, 257, 1027, 2047, 2048, 2049, 4099}
    for fs in (un, ma):
        assert {f["tiles"] for f in fs} >= {1, 2, 3}, "one tile, one over, two tiles plus a tail"
        assert any(f["odd_tail"] for f in fs) and any(not f["odd_tail"] for f in fs)
        assert any(f["sweep"] for f in fs)
    assert any(f["tiles"] == 1 and f["full_tile"] for f in un), "exactly one tile"
    assert {f["float4_tail"] for f in un} == {0, 1, 2, 3}
    assert {f["mae_last_rows"] for f in un} == {1, 2, 3, 4}
    assert {c.L for c in tk.CASES} >= {1, 32, 63, 64, 65, 256}
    assert {f["L_loops"] for f in un} >= {1, 2, 4} and {f["L_mod_64"] for f in un} >= {0, 1, 63, 32}
    assert {c.k for c in tk.CASES} >= {2, 6, 13, 64} and {c.n_aux for c in tk.CASES} >= {1, 2, 5, 13, 64}
    assert any(f["n_aux_eq_k"] and f["sweep"] for f in un) and any(not f["sweep"] for f in un)
    assert {c.th for c in tk.CASES if c.n_aux >= 2} >= {1, 255, 256, 257, 700, 4097}
    assert {f["th_per_thread"] for f in un} >= {1, 2, 3, 17}
    assert {c.cn for c in tk.CASES} == {"three", "two", "four", "outside", "frac", "craft"}
    assert {c.deg for c in tk.CASES} == {None, "two", "constdesc", "conststyle"}
    assert any(c.masked and c.n > 2048 for c in tk.CASES) and any(c.masked and c.n_aux == c.k == 64 for c in tk.CASES)
    assert set(tk.PLANES.values()) | set(tk.CAPTURES.values()) <= set(tk.BY_NAME)
    assert any(tk.BY_NAME[v].masked for v in tk.PLANES.values()) and any(not tk.BY_NAME[v].masked for v in tk.PLANES.values())
    assert {tk.BY_NAME[v].deg for v in tk.PLANES.values()} >= {"two", "constdesc", "conststyle"}
    assert {tk.BY_NAME[v].masked for v in tk.CAPTURES.values()} == {False, True}
    assert all(tk.BY_NAME[v].n == 2049 for v in tk.CAPTURES.values())
    # raae_style_metrics and raae_group_mean
    ns, ks = {n for n, _ in tk.SM_NK}, {k for _, k in tk.SM_NK}
    assert ns >= {3, 4, 37, 255, 256, 257, 1027, 2047, 2048, 2049, 4099} and ks == {1, 2, 13, 64}
    assert {n % 4 for n in ns if 256 < n < 262} >= {1, 2, 3}, "the float4 tail just above a multiple of 256"
    assert set(tk.GM_CASES) == {(1, 1, 1), (3, 20, 256), (37, 7, 65), (2049, 3, 257)}
    assert [g * L > 2048 * 256 for g, _, L in tk.GM_CASES] == [False, False, False, True], "the grid stride"
    # every case name pattern of the docstring's table matches a case, and every case is named by a pattern
    table = tk.__doc__.split("FORM -> CASE")[1]
    names = [c.name for c in tk.CASES] + list(tk.PLANES) + list(tk.CAPTURES)
    for prefix in ("tile", "mae_", "shape_", "sw_", "cls_", "deg_", "pl_", "cap_", "sm_", "smx_", "gm_"):
        assert re.search(r"\b" + prefix, table), prefix
    for prefix in ("tile", "mae_", "shape_", "sw_", "cls_", "deg_", "pl_", "cap_"):
        assert any(n.startswith(prefix) for n in names), prefix
    assert all(re.match(r"(tile|mae_|shape_|sw_|cls_|deg_|pl_|cap_)", n) for n in names) and len(set(names)) == len(names)
