"""Float64 restatement of what ``rankaae_amd/csrc/raae_select.hip`` and ``raae_metrics.hip`` compute -- every
intermediate included -- plus a mirror of their host side (work-buffer layout, grids, block layout).  Plain numpy, no
scipy, no scikit-learn: ``tests/test_select_reference_cpu.py`` holds it to those libraries where they are installed,
``tests/test_select_kernels_gpu.py`` holds the kernels to it.

The restatement is written from the definitions, not from the kernels: ranks by sorting (the kernels count), the
degree-2 fit by ``numpy.linalg.lstsq`` on the mapped, column-scaled basis as ``Polynomial.fit`` does it (the kernel
eliminates the normal equations), sums by numpy's pairwise summation (the kernels stride and tree).

Every floating scalar also comes in a HIGHER-PRECISION form (``mpmath`` at 60 digits from exact raw moments, or exact
``fractions``), used only to size tolerances: ``bound(scale, ref64, ref_hp) = max(64 eps scale, 16 |ref64 - ref_hp|)``.
"""
import itertools
import math
from fractions import Fraction

import mpmath
import numpy as np

HEAD, STRIDE, TILE = 4, 16, 2048        # RAAE_SEL_HEAD, RAAE_SEL_STRIDE; kTile of both files
EPS = 2.0 ** -52
MP = mpmath.mp.clone()
MP.dps = 60

# slot -> quantity class of a descriptor's slice (descriptor != 1) and of the head; everything else is exact
SLOT_CLASS = {0: "Spearman", 1: "slope", 2: "intercept", 3: "r2", 4: "quadratic coefficient", 5: "quadratic coefficient",
              6: "quadratic coefficient", 7: "residue", 8: "quadratic r2"}
HEAD_CLASS = {0: "MAE mean", 1: "MAE std", 2: "inter-style rho"}


def bound(scale, ref64, ref_hp):
    return max(64.0 * EPS * abs(scale), 16.0 * abs(ref64 - ref_hp))


# ----------------------------------------------------------------------------------------------- mirror of the host side
def align256(b):
    return (b + 255) & ~255


def select_work_bytes(n, k, n_aux, n_th):
    return align256(8 * n * (k + n_aux + 1)) + align256(4 * 4 * n_th)


def select_masked_work_bytes(n, k, n_aux, n_th):
    return align256(8 * n * (k + 2 * n_aux + 1)) + align256(4 * 4 * n_th)


def work_layout(n, k, n_aux, n_th, masked=False):
    """``{name: (byte offset, dtype, shape)}`` as ``sel_fill`` lays the work buffer out, and its size under "bytes"."""
    lay, off = {}, 0
    for name, cols in (("rank_z", k), ("rank_d", n_aux), ("mae", 1)) + ((("rank_zs", n_aux),) if masked else ()):
        lay[name] = (off, np.float64, (cols, n))
        off += 8 * cols * n
    lay["sweep"] = (align256(off), np.int32, (2, n_th, 2))
    lay["bytes"] = align256(off) + align256(16 * n_th)
    return lay


def written_bytes(n, k, n_aux, n_th, masked=False):
    """Boolean mask over the work buffer's bytes: what a call writes.  Not written: the rank column of descriptor 1 (the
    coordination number is classified, never ranked; ``rank_zs`` likewise), the slack before and behind the sweep table,
    and the whole table when ``n_aux == 1`` (no sweep launch)."""
    lay = work_layout(n, k, n_aux, n_th, masked)
    w = np.zeros(lay["bytes"], dtype=bool)
    for name in ("rank_z", "rank_d", "mae") + (("rank_zs",) if masked else ()):
        off, _, (cols, _) = lay[name]
        for c in range(cols):
            if not (name in ("rank_d", "rank_zs") and c == 1):
                w[off + 8 * n * c:off + 8 * n * (c + 1)] = True
    if n_aux >= 2:
        w[lay["sweep"][0]:lay["sweep"][0] + 16 * n_th] = True
    return w


def grids(n, k, n_aux, n_th, masked=False):
    """Grid of each of the four launches (None: not launched); every block is 256 threads."""
    cdiv = lambda a, b: (a + b - 1) // b      # noqa: E731
    return {"rank": (cdiv(n, 256), k + (2 if masked else 1) * n_aux, 1), "mae": (cdiv(n, 4), 1, 1),
            "sweep": (n_th, 2, 1) if n_aux >= 2 else None, "stat": (2 + n_aux, 1, 1)}


def form(n, k, n_aux, L, n_th, masked=False):
    """What a case reaches inside the kernels (the FORM -> CASE table is recomputed from this)."""
    return {"masked": masked, "tiles": -(-n // TILE), "full_tile": n >= TILE, "odd_tail": n % TILE % 2 == 1,
            "float4_tail": n % TILE % 4, "mae_last_rows": (n - 1) % 4 + 1, "L_mod_64": L % 64, "L_loops": -(-L // 64),
            "sweep": n_aux >= 2, "n_aux_eq_k": n_aux == k, "th_per_thread": -(-n_th // 256) if n_aux >= 2 else 0,
            "rank_grid_x": -(-n // 256), "stat_strides": -(-n // 256)}


def group_mean_grid(groups, L):
    return min((groups * L + 255) // 256, 2048)


def style_metrics_grids(n, k):
    return {"rank": (-(-n // 256), k, 1), "stat": (k + k * (k - 1) // 2, 1, 1)}


# ---------------------------------------------------------------------------------------------------------- the pieces
def avg_rank(x):
    """Average ranks (1-based) by sorting; ``+inf`` entries rank above everything and tie with each other."""
    x = np.asarray(x, np.float64)
    _, inv, cnt = np.unique(x, return_inverse=True, return_counts=True)
    less = np.cumsum(cnt) - cnt
    return less[inv] + 0.5 * (cnt[inv] + 1)


def labelled(x):
    return np.isfinite(x)


def mae_rows(spec_in, spec_out):
    """mean |out - in| of each row: the difference and its absolute value in fp32, the sum in double."""
    d = np.abs(np.asarray(spec_out, np.float32) - np.asarray(spec_in, np.float32))
    assert d.dtype == np.float32
    return d.astype(np.float64).sum(axis=1) / d.shape[1], [Fraction(math.fsum(r.tolist())) / d.shape[1] for r in d]


def cn_class(cn):
    return np.trunc(np.asarray(cn, np.float64) - 4.0)          # (cn - 4).astype(int): toward zero


def sweep_counts(z1, cls, th):
    """``[2][n_th][2]`` integers ``{2 TP, 2 TP + FP + FN}``: sweep 0 is ``z < th`` against ``class < 1``, sweep 1 is
    ``z > th`` against ``class > 1``; the fp32 style is promoted to double before it meets the threshold."""
    z = np.asarray(z1, np.float32).astype(np.float64)
    out = np.zeros((2, len(th), 2), dtype=np.int64)
    for s, (p, q) in enumerate(((z[None, :] < th[:, None], cls < 1.0), (z[None, :] > th[:, None], cls > 1.0))):
        out[s, :, 0] = 2 * (p & q[None, :]).sum(1)
        out[s, :, 1] = p.sum(1) + q.sum()
    return out


def quotients(counts):
    """The fractions of one sweep as exact ``Fraction``s, 0 where the denominator is 0 (``zero_division=0``)."""
    return [Fraction(int(a), int(b)) if b > 0 else Fraction(0) for a, b in counts]


def first_argmax(counts):
    best, bi = None, 0
    for t, q in enumerate(quotients(counts)):
        if best is None or q > best:
            best, bi = q, t
    return bi


def confusion(z1, cls, t45, t56):
    """``(cm[true 0..2][predicted 0..2], predicted counts[3])``; true classes outside 0..2 appear only in the latter."""
    z = np.asarray(z1, np.float32).astype(np.float64)
    pred = (z > t45).astype(int) + (z > t56).astype(int)
    cm = np.array([[int(((cls == r) & (pred == q)).sum()) for q in range(3)] for r in range(3)], dtype=np.int64)
    return cm, np.array([int((pred == q).sum()) for q in range(3)], dtype=np.int64)


def weighted_f1(cm, npred, m):
    """Support-weighted F1 over the labels 0..2 with divisor ``m`` (every row's support counts): float64 and exact."""
    acc, exact = 0.0, Fraction(0)
    for l in range(3):
        support, den = int(cm[l].sum()), int(cm[l].sum() + npred[l])
        if den > 0:
            acc += (2.0 * cm[l, l] / den) * support
            exact += Fraction(2 * int(cm[l, l]), den) * support
    return acc / m, exact / m


def pearson(u, v):
    """numpy.corrcoef's arithmetic: centre, divide by each deviation, clip."""
    u, v = u - u.mean(), v - v.mean()
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.float64(np.dot(u, v)) / np.sqrt(np.dot(u, u)) / np.sqrt(np.dot(v, v))
    return float(np.clip(r, -1.0, 1.0)) if r == r else float("nan")


def _moments_hp(*cols):
    """Exact column lists for ``MP.fdot``."""
    return [[MP.mpf(float(v)) for v in c] for c in cols]


def pearson_hp(u, v):
    n = len(u)
    U, V = _moments_hp(u, v)
    su, sv = MP.fsum(U), MP.fsum(V)
    cuu, cvv, cuv = MP.fdot(U, U) - su * su / n, MP.fdot(V, V) - sv * sv / n, MP.fdot(U, V) - su * sv / n
    if cuu == 0 or cvv == 0:
        return float("nan")
    return float(cuv / MP.sqrt(cuu * cvv))


def descriptor_stats(x, y):
    """One descriptor's slice from ``x`` (descriptor, float64) and ``y`` (style, fp32 promoted) on its labelled rows:
    float64 values and the high-precision ones, both as ``{slot: value}`` for slots 0..8, plus "rank" (lstsq's) and the
    two rank vectors."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float32).astype(np.float64)
    n = len(x)
    rx, ry = avg_rank(x), avg_rank(y)
    res = {"rx": rx, "ry": ry}
    nan = float("nan")
    if x.max() == x.min():
        # a constant descriptor: scipy's spearmanr gives NaN, its linregress raises; nothing else is defined
        res["rank"], res["f64"], res["hp"] = 1, {s: nan for s in range(9)}, {s: nan for s in range(9)}
        return res
    f64, hp = {}, {}
    f64[0], hp[0] = pearson(rx, ry), pearson_hp(rx, ry)
    # scipy.stats.linregress
    xm, ym = x.mean(), y.mean()
    ssxm, ssym, ssxym = np.dot(x - xm, x - xm) / n, np.dot(y - ym, y - ym) / n, np.dot(x - xm, y - ym) / n
    r = 0.0 if ssxm == 0.0 or ssym == 0.0 else float(np.clip(ssxym / np.sqrt(ssxm * ssym), -1.0, 1.0))
    slope = ssxym / ssxm
    f64[1], f64[2], f64[3] = slope, ym - slope * xm, r * r
    # Polynomial.fit(x, y, 2, full=True): map [min, max] onto [-1, 1], scale the columns, SVD least squares
    lo, hi = x.min(), x.max()
    off, scl = (-hi - lo) / (hi - lo), 2.0 / (hi - lo)
    u = off + scl * x
    lhs = np.stack([np.ones(n), u, u * u], axis=1)
    col = np.sqrt(np.square(lhs).sum(0))
    c, _, rank, _ = np.linalg.lstsq(lhs / col, y, rcond=n * np.finfo(np.float64).eps)
    a = c / col
    f64[4], f64[5], f64[6] = a[0] + a[1] * off + a[2] * off * off, a[1] * scl + 2.0 * a[2] * off * scl, a[2] * scl * scl
    fit = lhs @ a
    f64[7] = float(np.dot(y - fit, y - fit)) / n
    f64[8] = pearson(fit, y) ** 2 if np.ptp(fit) > 0.0 and ssym > 0.0 else 0.0
    res["rank"] = int(rank)
    # ---- high precision, from exact raw moments
    X, Y = _moments_hp(x, y)
    X2 = [v * v for v in X]
    N = MP.mpf(n)
    sx, sy, sxx, sxy, syy = MP.fsum(X), MP.fsum(Y), MP.fsum(X2), MP.fdot(X, Y), MP.fdot(Y, Y)
    cxx, cyy, cxy = sxx - sx * sx / N, syy - sy * sy / N, sxy - sx * sy / N
    hslope = cxy / cxx
    hp[1], hp[2] = float(hslope), float(sy / N - hslope * sx / N)
    hp[3] = 0.0 if cyy == 0 else float(cxy * cxy / (cxx * cyy))
    sx3, sx4, sx2y = MP.fdot(X2, X), MP.fdot(X2, X2), MP.fdot(X2, Y)
    if rank == 3:
        M = MP.matrix([[N, sx, sxx], [sx, sxx, sx3], [sxx, sx3, sx4]])
        b = MP.matrix([sy, sxy, sx2y])
        q = MP.lu_solve(M, b)
        q0, q1, q2 = q[0], q[1], q[2]
    else:
        # two distinct values: u = -1 / +1, the line through the two group means, its constant shared by 1 and u^2
        assert rank == 2 and len(np.unique(x)) == 2, (rank, np.unique(x)[:5])
        mlo, mhi = [MP.fsum([MP.mpf(float(v)) for v in y[x == e]]) / int((x == e).sum()) for e in (lo, hi)]
        a1, a02 = (mhi - mlo) / 2, (mhi + mlo) / 4
        hoff, hscl = (-MP.mpf(float(hi)) - MP.mpf(float(lo))) / (MP.mpf(float(hi)) - MP.mpf(float(lo))), 2 / (MP.mpf(float(hi)) - MP.mpf(float(lo)))
        q0, q1, q2 = a02 + a1 * hoff + a02 * hoff * hoff, a1 * hscl + 2 * a02 * hoff * hscl, a02 * hscl * hscl
    hp[4], hp[5], hp[6] = float(q0), float(q1), float(q2)
    # sum (y - q0 - q1 x - q2 x^2)^2 and the correlation of the fitted values with y, expanded in the moments
    sff = q0 * q0 * N + q1 * q1 * sxx + q2 * q2 * sx4 + 2 * (q0 * q1 * sx + q0 * q2 * sxx + q1 * q2 * sx3)
    sfy, sf = q0 * sy + q1 * sxy + q2 * sx2y, q0 * N + q1 * sx + q2 * sxx
    hp[7] = float((syy - 2 * sfy + sff) / N)
    cff, cfy = sff - sf * sf / N, sfy - sf * sy / N
    hp[8] = 0.0 if f64[8] == 0.0 else float(cfy * cfy / (cff * cyy))
    res["f64"], res["hp"] = f64, hp
    return res


def slot_scale(slot, f64):
    """The natural magnitude of a slice's slot for one case."""
    if slot in (1, 2):
        return max(abs(f64[1]), abs(f64[2]))
    if slot in (4, 5, 6):
        return max(abs(f64[4]), abs(f64[5]), abs(f64[6]))
    if slot == 7:
        return abs(f64[7])
    return 1.0


def mean_std(v, exact):
    """np.mean / np.std (population) and the same from exact fractions."""
    m = Fraction(sum(exact)) / len(exact)
    var = sum((e - m) ** 2 for e in exact) / len(exact)
    return (float(np.mean(v)), float(np.std(v))), (float(m), float(MP.sqrt(MP.mpf(var.numerator) / var.denominator)))


def inter_style(rank_z):
    """``max_i |rho(style_i, style_last)|``, ``i < k - 1``, as the kernel states it: ``fmax`` drops a NaN, so a constant
    column among the first ``k - 1`` does not take part (and a constant last column gives 0)."""
    best, best_hp = 0.0, 0.0
    for c in range(len(rank_z) - 1):
        r, h = pearson(rank_z[c], rank_z[-1]), pearson_hp(rank_z[c], rank_z[-1])
        if r == r and abs(r) > best:
            best, best_hp = abs(r), abs(h)
    return best, best_hp


# ----------------------------------------------------------------------------------------------------- the whole block
def select_ref(styles, aux, spec_in, spec_out, th, masked=False):
    """Everything ``raae_select_scores`` (or ``_masked``) forms for one model.  Returns a dict:

    ``rank_z [k][n]``, ``rank_d [n_aux][n]`` (row 1: None), ``rank_zs`` (masked), ``mae [n]``, ``sweep [2][n_th][2]``,
    ``block`` (float64 restatement, laid out as the kernel's), ``block_hp`` (the high-precision form, rounded to
    float64), ``scale`` and ``cls`` per slot (``cls`` None: compared exactly), ``tol`` (the bound per slot), ``m``
    (rows per descriptor), ``distinct`` (classes of descriptor 1), ``lstsq_rank`` per descriptor."""
    z = np.ascontiguousarray(styles, np.float32)
    aux = np.ascontiguousarray(aux, np.float64)
    n, k = z.shape
    n_aux = aux.shape[1]
    th = np.asarray(th, np.float64)
    if not masked:
        assert np.isfinite(aux).all()
    lab = labelled(aux)
    R = {"m": lab.sum(0), "lstsq_rank": {}}
    R["rank_z"] = np.stack([avg_rank(z[:, c]) for c in range(k)])
    R["rank_d"] = [None if i == 1 else avg_rank(np.where(lab[:, i], aux[:, i], np.inf)) for i in range(n_aux)]
    if masked:
        R["rank_zs"] = [None if i == 1 else avg_rank(np.where(lab[:, i], z[:, i].astype(np.float64), np.inf))
                        for i in range(n_aux)]
    R["mae"], mae_exact = mae_rows(spec_in, spec_out)
    size = HEAD + STRIDE * n_aux
    block, hp, scale = np.zeros(size), np.zeros(size), np.ones(size)
    cls = [None] * size
    (block[0], block[1]), (hp[0], hp[1]) = mean_std(R["mae"], mae_exact)
    block[2], hp[2] = inter_style(R["rank_z"])
    scale[0], scale[1] = abs(block[0]), abs(block[1])
    for s, name in HEAD_CLASS.items():
        cls[s] = name
    for i in range(n_aux):
        o = HEAD + STRIDE * i
        rows = np.flatnonzero(lab[:, i])
        if len(rows) < 3:
            continue                                     # the slice is zeros
        if i == 1:
            c = cn_class(aux[rows, 1])
            R["sweep"] = sweep_counts(z[rows, 1], c, th)
            R["distinct"] = len(np.unique(c))
            if R["distinct"] > 3:
                continue                                 # o[0] == 0: no result
            i45, i56 = first_argmax(R["sweep"][0]), first_argmax(R["sweep"][1])
            cm, npred = confusion(z[rows, 1], c, th[i45], th[i56])
            f1, f1_exact = weighted_f1(cm, npred, len(rows))
            block[o:o + 6] = hp[o:o + 6] = [1.0, f1, i45, i56, th[i45], th[i56]]
            hp[o + 1] = float(f1_exact)
            block[o + 6:o + 15] = hp[o + 6:o + 15] = cm.reshape(-1)
            cls[o + 1] = "F1"
            R["cm"], R["npred"] = cm, npred
        else:
            st = descriptor_stats(aux[rows, i], z[rows, i])
            R["lstsq_rank"][i] = st["rank"]
            for s in range(9):
                block[o + s], hp[o + s], cls[o + s] = st["f64"][s], st["hp"][s], SLOT_CLASS[s]
                scale[o + s] = slot_scale(s, st["f64"])
            if len(rows) == 3:
                # three rows, three coefficients: the fit interpolates, and the residue is the rounding noise of y - f
                # (lstsq itself reports none for a square system).  Its natural magnitude is that of y^2, not its own
                y = z[rows, i].astype(np.float64)
                scale[o + 7] = float(np.mean(y * y))
    if n_aux >= 2 and "sweep" not in R:                  # the sweep runs whatever the slice becomes
        rows = np.flatnonzero(lab[:, 1])
        R["sweep"] = sweep_counts(z[rows, 1], cn_class(aux[rows, 1]), th)
    with np.errstate(invalid="ignore"):
        tol = np.array([0.0 if c is None else bound(sc, b, h) for c, sc, b, h in zip(cls, scale, block, hp)])
    R.update(block=block, block_hp=hp, scale=scale, cls=cls, tol=tol)
    return R


# ------------------------------------------------------------------------------------------------- raae_style_metrics
def shapiro_w(x, a):
    """W of one column with AS R94's arithmetic as scipy 1.15.3 runs it: pivot ``x[n // 2]``, range scaling, squared
    correlation with the antisymmetric coefficient vector, reported as ``1 - (1 - W)``; float64 and high precision.  Also
    returns the sorted, pivoted column."""
    x = np.asarray(x, np.float32).astype(np.float64)
    n = len(x)
    y = np.sort(x - x[n // 2])
    rng = y[-1] - y[0]
    if rng < 1e-19:
        return 1.0, 1.0, y
    coef = np.zeros(n)
    coef[:n // 2] = -np.asarray(a, np.float64)
    coef[n - n // 2:] = np.asarray(a, np.float64)[::-1]
    xx = y / rng
    sa, sx = coef.sum() / n, xx.sum() / n
    ssa, ssx, sax = np.dot(coef - sa, coef - sa), np.dot(xx - sx, xx - sx), np.dot(coef - sa, xx - sx)
    ssassx = np.sqrt(ssa * ssx)
    w64 = 1.0 - (ssassx - sax) * (ssassx + sax) / (ssa * ssx)
    A, Y = _moments_hp(coef, y)
    sA, sY = MP.fsum(A), MP.fsum(Y)
    caa, cyy, cay = MP.fdot(A, A) - sA * sA / n, MP.fdot(Y, Y) - sY * sY / n, MP.fdot(A, Y) - sA * sY / n
    return float(w64), float(cay * cay / (caa * cyy)), y


def style_metrics_ref(z, a):
    """``W [k]``, ``rho [k (k - 1) / 2]`` in ``itertools.combinations`` order (NaN where a column is constant), each
    float64 and high precision, the rank matrix and the sorted columns."""
    z = np.ascontiguousarray(z, np.float32)
    n, k = z.shape
    rank = np.stack([avg_rank(z[:, c]) for c in range(k)])
    W = [shapiro_w(z[:, c], a) for c in range(k)]
    pairs = list(itertools.combinations(range(k), 2))
    rho = np.array([pearson(rank[p], rank[q]) for p, q in pairs])
    rho_hp = np.array([pearson_hp(rank[p], rank[q]) for p, q in pairs])
    return {"W": np.array([w[0] for w in W]), "W_hp": np.array([w[1] for w in W]), "rho": rho, "rho_hp": rho_hp,
            "rank": rank, "sorted": np.stack([w[2] for w in W])}


# ------------------------------------------------------------------------------------------------------ raae_group_mean
def group_mean_exact(x, groups, per, L):
    """``mean_s x[g][s][l]`` with ``math.fsum`` (the exactly rounded sum) divided by ``per``: float64 ``[groups, L]``."""
    x = np.asarray(x, np.float32).reshape(groups, per, L).astype(np.float64)
    cols = x.transpose(0, 2, 1).reshape(groups * L, per).tolist()
    return (np.array([math.fsum(c) for c in cols]) / per).reshape(groups, L)


def ulp32(v):
    v = np.abs(np.asarray(v, np.float64)).astype(np.float32)
    return (np.nextafter(v, np.float32(np.inf)) - v).astype(np.float64)
