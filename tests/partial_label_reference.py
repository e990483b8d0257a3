"""Float64 restatement of the rank loss on a batch with missing labels, written from its definition (numpy only).

A NaN in column ``k`` of the descriptors means the row has no label for descriptor ``k``.  With ``S_k`` the rows whose
descriptor ``k`` is finite and ``m_k = |S_k|``

    loss = -(1 / n_aux) * sum_k [ sum_{i,j in S_k} w_k(i,j) (z_ik - z_jk) sign(d_ik - d_jk) ] / max(m_k^2 - m_k, 1)

``w_k`` is 1 without ``activate``; with it, the pairs whose product ``(z_ik - z_jk) sign(d_ik - d_jk)`` is positive are
weighted by ``n_opp / max(n_same, n_opp)``, ``n_same`` / ``n_opp`` the numbers of positive / negative products among
the pairs inside ``S_k``, each at least 1 (a constant of the batch: no gradient flows through it).  The gradient is the
derivative of that expression in ``z``; it is 0 wherever the row is outside ``S_k``."""
import numpy as np


def masked_rank_loss(d, z, activate=False):
    """``(loss, dloss/dz [B, n_aux])`` in float64 for descriptors ``d [B, n_aux]`` (NaN: no label) and styles
    ``z [B, n_aux]``."""
    d = np.asarray(d, dtype=np.float64)
    z = np.asarray(z, dtype=np.float64)
    n, n_aux = z.shape
    loss, grad = 0.0, np.zeros((n, n_aux))
    for k in range(n_aux):
        rows = np.flatnonzero(np.isfinite(d[:, k]))
        m = len(rows)
        if m < 2:
            continue
        dk, zk = d[rows, k], z[rows, k]
        sign = np.sign(dk[:, None] - dk[None, :])
        prod = (zk[:, None] - zk[None, :]) * sign
        w = np.ones_like(prod)
        if activate:
            n_same, n_opp = max(int((prod > 0).sum()), 1), max(int((prod < 0).sum()), 1)
            w[prod > 0] = n_opp / max(n_same, n_opp)
        norm = max(m * m - m, 1) * n_aux
        loss -= (w * prod).sum() / norm
        ws = w * sign
        grad[rows, k] = -(ws.sum(axis=1) - ws.sum(axis=0)) / norm       # z_i enters pair (i, j) with +, pair (j, i) with -
    return loss, grad


def compact(d, z, k=0):
    """The rows labelled for descriptor ``k``: ``(row indices, d[rows], z[rows])``."""
    rows = np.flatnonzero(np.isfinite(np.asarray(d)[:, k]))
    return rows, np.asarray(d)[rows], np.asarray(z)[rows]
