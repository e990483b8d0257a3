"""Float64 reference of the pairwise logistic rank loss (``raae_rank_logistic_fwd_bwd``), blockwise over the pairs, with
the sums that bound an fp32 evaluation of it.

``S_k``: the rows whose descriptor ``k`` is finite, ``m_k`` their number, ``norm_k = max(m_k^2 - m_k, 1)``; with
``s_ij = sign(d_ik - d_jk)`` and ``x_ij = -s_ij (z_ik - z_jk) / T``::

    L     = (1 / n_aux) sum_k T / norm_k sum_{i,j in S_k, s_ij != 0} softplus(x_ij)
    dz_ik = -2 / (n_aux norm_k) sum_{j in S_k, s_ij != 0} s_ij sigma(x_ij)

Error model of the kernel (``bounds``).  Every fp32 operation is rounded once, relative error ``u = 2^-24``; ``expf`` and
``log1pf`` are good to one ulp, ``2 u``.  The argument ``x`` carries two roundings (the difference, the divide), which
``sigma`` amplifies by its relative sensitivity ``(1 - sigma) |x| <= |x|`` and softplus by ``sigma |x| / softplus <=
|x|`` (``sigma <= softplus`` everywhere): ``2 |x| u``.  ``sigma = (x >= 0 ? 1 : e) / (1 + e)`` adds ``expf`` (2), the add
(1) and the divide (1): ``(2 |x| + 4) u`` per term.  ``softplus = max(x, 0) + log1pf(e)`` adds ``expf`` (2, passed on by
``log1p`` with a factor <= 1), ``log1pf`` (2) on the ``log1p`` part and the add (1) on the whole, which is exact for
``x <= 0``: again within ``(2 |x| + 4) u`` of the term.  An fp32 accumulator that adds ``J`` terms adds ``J u`` times
the sum of their magnitudes.  With ``t = s sigma``, ``A = sum |t|`` and ``E = sum (2 |x| + 4) |t|``::

    |dz - ref| <= f 2^-24 (E_ik + J A_ik) + spacing(ref),    f = 2 / (n_aux norm_k)

and the same for the loss with its own sums and ``f = T / (n_aux norm_k)``.  ``spacing`` is fp32's at the reference
value (the store), which also covers terms below fp32's range.  ``T`` is the temperature as the kernel uses it: the
caller's value rounded to fp32 once (``temperature_f32``)."""
import numpy as np

import loss_reference as lr

U = 2.0 ** -24
RANK_JC = 8                  # lanes that split the columns of one (row, descriptor)


def temperature_f32(t):
    """The temperature every pair and the loss use: the caller's double rounded to fp32 once."""
    return float(np.float32(t))


def evaluate(d, z, n_aux, T, block=512):
    """``d [B, >= n_aux]`` descriptors (NaN: no label), ``z [B, >= n_aux]`` styles, float64 arithmetic throughout.
    Returns a dict: ``loss``, ``dz [B, n_aux]``, ``A``/``E [B, n_aux]`` (the gradient's bound sums), ``lossA``/``lossE
    [n_aux]`` (the loss's, per descriptor, unnormalised), ``norm [n_aux]``, ``m [n_aux]``, ``untied [n_aux]`` (ordered
    pairs with ``s != 0``)."""
    d = np.asarray(d, dtype=np.float64)[:, :n_aux]
    z = np.asarray(z, dtype=np.float64)[:, :n_aux]
    B = d.shape[0]
    T = float(T)
    lab = np.isfinite(d)
    m = lab.sum(axis=0).astype(np.int64)
    norm = np.maximum(m * m - m, 1).astype(np.float64)
    G = np.zeros((B, n_aux))
    A = np.zeros((B, n_aux))
    E = np.zeros((B, n_aux))
    lsum, lA, lE = np.zeros(n_aux), np.zeros(n_aux), np.zeros(n_aux)
    untied = np.zeros(n_aux, dtype=np.int64)
    dd = np.where(lab, d, 0.0)
    for k in range(n_aux):
        for i0 in range(0, B, block):
            i1 = min(B, i0 + block)
            # x_ji = x_ij and s_ji = -s_ij: the blocks below the diagonal are the transposes of those above it
            for j0 in range(i0, B, block):
                j1 = min(B, j0 + block)
                s = np.sign(dd[i0:i1, k, None] - dd[None, j0:j1, k])
                s = s * (lab[i0:i1, k, None] & lab[None, j0:j1, k])
                on = s != 0.0
                x = -s * (z[i0:i1, k, None] - z[None, j0:j1, k]) / T
                e = np.exp(-np.abs(x))
                at = np.where(x >= 0.0, 1.0, e) / (1.0 + e) * on       # |t|, t = s sigma(x)
                t = s * at
                w = 2.0 * np.abs(x) + 4.0
                sp = (np.maximum(x, 0.0) + np.log1p(e)) * on
                wat, wsp = w * at, w * sp
                G[i0:i1, k] += t.sum(axis=1)
                A[i0:i1, k] += at.sum(axis=1)
                E[i0:i1, k] += wat.sum(axis=1)
                both = 2.0 if j0 > i0 else 1.0
                if j0 > i0:
                    G[j0:j1, k] -= t.sum(axis=0)
                    A[j0:j1, k] += at.sum(axis=0)
                    E[j0:j1, k] += wat.sum(axis=0)
                lsum[k] += both * sp.sum()
                lE[k] += both * wsp.sum()
                untied[k] += int(both) * int(on.sum())
    lA = lsum.copy()
    loss = float((T * lsum / norm).sum() / n_aux)
    dz = -2.0 / (n_aux * norm) * G
    return dict(loss=loss, dz=dz, A=A, E=E, lossA=lA, lossE=lE, norm=norm, m=m, untied=untied, T=T, n_aux=n_aux)


def loss(d, z, n_aux, T):
    return evaluate(d, z, n_aux, T)["loss"]


def gradient(d, z, n_aux, T):
    return evaluate(d, z, n_aux, T)["dz"]


def accumulator_terms(B, n_aux):
    """``J``: the most additions that one fp32 value of the kernel goes through, from the launch geometry
    (``loss_reference.rank_grid``): a lane's share of the columns of its column block, the three shuffle steps of the
    eight lanes, the column blocks added by the finish, and the rounded factor with its product."""
    R, nj, jchunk, nwg = lr.rank_grid(B, B, n_aux)
    cols = min(jchunk, B)
    return (cols + RANK_JC - 1) // RANK_JC + 3 + nj + 2


def spacing32(v):
    return np.spacing(np.abs(np.asarray(v, dtype=np.float64)).astype(np.float32)).astype(np.float64)


def bounds(ref, B):
    """``(dz_bound [B, n_aux], loss_bound)`` of an fp32 evaluation against ``ref = evaluate(...)``."""
    n_aux = ref["n_aux"]
    J = accumulator_terms(B, n_aux)
    f = 2.0 / (n_aux * ref["norm"])
    dz_bound = f * U * (ref["E"] + J * ref["A"]) + spacing32(ref["dz"])
    fl = ref["T"] / (n_aux * ref["norm"])
    loss_bound = float((fl * U * (ref["lossE"] + J * ref["lossA"])).sum() + spacing32(ref["loss"]))
    return dz_bound, loss_bound


def make_inputs(B, n_aux, ldd, ldz, seed, missing=True):
    """The test inputs: Gaussian styles with a few duplicated values and a few at +-1e4, descriptors with ties, and
    with ``missing`` about 30 % NaN cells, one all-NaN row and (from two descriptors on) one descriptor with a single
    labelled row.  The padding columns of ``z`` are NaN.  float32 arrays ``d [B, ldd]``, ``z [B, ldz]``."""
    rng = np.random.default_rng(seed)
    d = np.round(rng.standard_normal((B, ldd)) * 4.0) / 4.0            # a grid of values: many ties
    z = rng.standard_normal((B, ldz))
    ndup = max(1, B // 16)
    for k in range(n_aux):
        src, dst = rng.integers(0, B, ndup), rng.integers(0, B, ndup)
        z[dst, k] = z[src, k]                                          # duplicated style values
    if B >= 8:
        big = rng.choice(B, size=min(4, B // 4), replace=False)
        z[big, rng.integers(0, n_aux, big.size)] = np.where(rng.random(big.size) < 0.5, 1e4, -1e4)
    z[:, n_aux:] = np.nan
    if missing:
        d[rng.random((B, ldd)) < 0.3] = np.nan
        r = int(rng.integers(0, B))
        if n_aux >= 2:
            d[:, n_aux - 1] = np.nan                                   # a descriptor with one labelled row
            d[(r + 1) % B, n_aux - 1] = 0.5
        d[r, :] = np.nan                                               # a row without any label
    return d.astype(np.float32), z.astype(np.float32)
