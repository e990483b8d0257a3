"""Float64 restatement of the masked rank loss split over the ranks of a data-parallel run (numpy only).

Rank r owns rows ``[row0, row0 + nrows)`` of the gathered batch and pairs them with all rows.  A pair ``(i, j)`` of
descriptor ``k`` counts only where both ``d_ik`` and ``d_jk`` are finite.  With ``p = (z_ik - z_jk) sign(d_ik - d_jk)``
a rank's totals are, per descriptor,

    n+ = #{p > 0},  n- = #{p < 0},  S+ = sum of the positive p,  S- = sum of the negative p,  m = labelled rows it owns.

The ranks' rows partition the batch, so the totals summed over the ranks are those of the whole batch, and with
``c_k = 1`` (no ``activate``) or ``max(n-, 1) / max(max(n+, 1), max(n-, 1))``

    loss = -(1 / n_aux) sum_k (c_k S+_k + S-_k) / max(m_k^2 - m_k, 1)        (a descriptor with m_k < 2 contributes 0)

which is ``partial_label_reference.masked_rank_loss`` on the whole batch; ``tests/test_partial_labels_rows_cpu.py`` pins
that.  The cases and splits below are the ones the GPU test runs the kernels on."""
import numpy as np

TILE = 256                  # RANK_TJ, the pair pass's tile of j rows (raae_loss.hip)

# case -> the ranks' row counts, in rank order
SPLITS = {"b7": [(4, 3), (3, 2, 2)], "tile": [(128, 129), (256, 1)], "blocked": [(550, 550), (1050, 50)]}


def rank_case(name, labelled=False):
    """``(d [B, K] with NaN, z [B, K + 1], K)``; column 1 holds 4 / 5 / 6: ties.  ``labelled``: the same batch without
    the NaNs."""
    B, K = {"b7": (7, 5), "tile": (TILE + 1, 2), "blocked": (1100, 5)}[name]
    g = np.random.default_rng(B * 31 + K)
    d = g.standard_normal((B, K)).astype(np.float32)
    d[:, 1] = g.integers(4, 7, size=B)
    z = g.standard_normal((B, K + 1)).astype(np.float32)
    gone = np.zeros((B, K), dtype=bool)
    if name == "b7":                                               # m = 5, 3, 0, 1, 6
        gone[[1, 5], 0] = True
        gone[[0, 1, 2, 6], 1] = True                               # 3 labelled, of the tied column; split 3+2+2: rank 0 owns none
        gone[:, 2] = True
        gone[np.arange(7) != 4, 3] = True
        gone[3, 4] = True
    elif name == "tile":                                           # unlabelled rows on both sides of row 256
        gone[[0, 7, 100, TILE - 2, TILE], 0] = True
        gone[[3, 50, TILE - 1], 1] = True
    else:                                                          # several column blocks; 1050 rows: four rows per thread
        gone[g.random((B, K)) < 0.3] = True
        gone[:, 3] = True
    if not labelled:
        d[gone] = np.nan
    return d, z, K


def masked_rank_rows(d_all, z_all, row0, nrows, activate=False):
    """This rank's totals ``[5][n_aux]`` = ``{n+, n-, S+, S-, m}`` in float64 (``activate`` does not enter them: the
    weights are formed from the SUMMED counts, in ``finish``)."""
    d = np.asarray(d_all, dtype=np.float64)
    z = np.asarray(z_all, dtype=np.float64)
    n_aux = d.shape[1]
    totals = np.zeros((5, n_aux))
    for k in range(n_aux):
        lab = np.isfinite(d[:, k])
        mine = row0 + np.flatnonzero(lab[row0:row0 + nrows])
        cols = np.flatnonzero(lab)
        totals[4, k] = len(mine)
        if len(mine) == 0:
            continue
        p = (z[mine, k][:, None] - z[cols, k][None, :]) * np.sign(d[mine, k][:, None] - d[cols, k][None, :])
        totals[0, k], totals[1, k] = (p > 0).sum(), (p < 0).sum()
        totals[2, k], totals[3, k] = p[p > 0].sum(), p[p < 0].sum()
    return totals


def finish(totals_sum, d_all, z_all, row0, nrows, activate=False):
    """``(loss, dloss/dz of rows [row0, row0 + nrows) as [nrows, n_aux])`` from the totals summed over the ranks."""
    d = np.asarray(d_all, dtype=np.float64)
    z = np.asarray(z_all, dtype=np.float64)
    n_aux = d.shape[1]
    loss, grad = 0.0, np.zeros((nrows, n_aux))
    for k in range(n_aux):
        n_same, n_opp, s_pos, s_neg, m = (float(v) for v in np.asarray(totals_sum)[:, k])
        if m < 2:
            continue
        c = max(n_opp, 1.0) / max(max(n_same, 1.0), max(n_opp, 1.0)) if activate else 1.0
        norm = max(m * m - m, 1.0) * n_aux
        loss -= (c * s_pos + s_neg) / norm
        lab = np.isfinite(d[:, k])
        mine = row0 + np.flatnonzero(lab[row0:row0 + nrows])
        cols = np.flatnonzero(lab)
        sign = np.sign(d[mine, k][:, None] - d[cols, k][None, :])
        p = (z[mine, k][:, None] - z[cols, k][None, :]) * sign
        w = np.where(p > 0, c, 1.0)
        # z_i enters pair (i, j) with + and pair (j, i), which has the same p and the opposite sign, with -
        grad[mine - row0, k] = -2.0 * (w * sign).sum(axis=1) / norm
    return loss, grad
