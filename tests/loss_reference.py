"""Float64 restatement, without autograd, of every entry point of ``csrc/raae_loss.hip`` and ``csrc/raae_disc.hip``
(numpy only), and a pure-Python mirror of their launch dispatch.

Each function is written from the definition of the operation, not from the kernel: ``test_loss_reference_cpu.py`` holds
every one of them to float64 torch autograd of the same composition (1e-12 relative), and the masked rank loss to
``partial_label_reference.masked_rank_loss`` / ``partial_label_rows_reference``, which state the same loss.
``test_loss_kernels_gpu.py`` runs the kernels against them, one launch at a time."""
import math

import numpy as np

EPS, MOMENTUM = 1e-5, 0.1
U32 = 2.0 ** -24                    # unit roundoff of fp32


def f32(a):
    """Round to fp32 and return as float64: what a kernel reads of a reference tensor."""
    return np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)


# ------------------------------------------------------------------------------------------------------ rank loss
class Pairs:
    """The pair pass of rows ``[row0, row0 + nrows)`` against all rows, per descriptor ``k``: the exact integer counts
    ``npos`` / ``nneg`` of the products ``p = (z_ik - z_jk) sign(d_ik - d_jk)`` that are > 0 / < 0, their float64 sums
    ``spos`` / ``sneg``, ``m`` the labelled rows among the owned rows, and per owned row ``gpos`` / ``gneg`` = the sum of
    ``sign(d_ik - d_jk)`` over the pairs with ``p > 0`` / ``p < 0`` (integers held as float64).

    TIES: a pair with equal styles and different descriptors has ``p == 0`` and counts in neither n, S nor g+-: the
    convention of ``oracle.ref_train.kendall_closed_form`` and of the kernels.  Autograd of the literal loss differs
    there: the pair's term ``(z_ik - z_jk) sign`` has the derivative ``sign`` (weight 1) also at ``p == 0``.  ``gzero``
    holds the sign sum over those pairs, so that ``rank_tie_term`` states the difference exactly (the CPU test pins
    reference + tie term to autograd, and the reference itself to the closed form)."""

    def __init__(self, nrows, K):
        self.npos, self.nneg, self.m = np.zeros(K, np.int64), np.zeros(K, np.int64), np.zeros(K, np.int64)
        self.spos, self.sneg = np.zeros(K), np.zeros(K)
        self.gpos, self.gneg, self.gzero = np.zeros((nrows, K)), np.zeros((nrows, K)), np.zeros((nrows, K))

    def totals(self, masked):
        """``[4 | 5][16]`` doubles as the kernels lay them out: {n+, n-, S+, S-, (m)}."""
        t = np.zeros((5 if masked else 4, 16))
        K = len(self.m)
        t[0, :K], t[1, :K], t[2, :K], t[3, :K] = self.npos, self.nneg, self.spos, self.sneg
        if masked:
            t[4, :K] = self.m
        return t


def _pair_column(dk, zk, lab, row0, nrows, block):
    """One descriptor: ``(n+, n-, S+, S-, m, g+ [nrows], g- [nrows], g0 [nrows])``, g0 the sign sum over the pairs
    with ``p == 0``; memory ``block x B``."""
    cols = np.flatnonzero(lab)
    dc, zc = dk[cols], zk[cols]
    npos = nneg = 0
    sp, sn = [], []
    gp, gn, g0 = np.zeros(nrows), np.zeros(nrows), np.zeros(nrows)
    m = 0
    for i0 in range(row0, row0 + nrows, block):
        idx = np.arange(i0, min(i0 + block, row0 + nrows))
        mine = idx[lab[idx]]
        m += len(mine)
        if len(mine) == 0 or len(cols) == 0:
            continue
        s = np.sign(dk[mine][:, None] - dc[None, :])
        p = (zk[mine][:, None] - zc[None, :]) * s
        pos, neg = p > 0, p < 0
        npos += int(pos.sum())
        nneg += int(neg.sum())
        sp.append(float(np.where(pos, p, 0.0).sum()))
        sn.append(float(np.where(neg, p, 0.0).sum()))
        gp[mine - row0] = np.where(pos, s, 0.0).sum(1)
        gn[mine - row0] = np.where(neg, s, 0.0).sum(1)
        g0[mine - row0] = np.where(p == 0, s, 0.0).sum(1)
    return npos, nneg, math.fsum(sp), math.fsum(sn), m, gp, gn, g0


def rank_pairs(d, z, masked=False, row0=0, nrows=None, block=512):
    """``Pairs`` of descriptors ``d [B, K]`` and styles ``z [B, K]``, computed per descriptor column (memory B^2, not
    B^2 K).  ``masked``: a cell of ``d`` that is not finite takes its row out of that descriptor's pairs."""
    d, z = np.asarray(d, np.float64), np.asarray(z, np.float64)
    B, K = z.shape
    nrows = B - row0 if nrows is None else nrows
    P = Pairs(nrows, K)
    for k in range(K):
        lab = np.isfinite(d[:, k]) if masked else np.ones(B, bool)
        (P.npos[k], P.nneg[k], P.spos[k], P.sneg[k], P.m[k], P.gpos[:, k], P.gneg[:, k], P.gzero[:, k]) = \
            _pair_column(d[:, k], z[:, k], lab, row0, nrows, block)
    return P


def rank_pairs_scaled(d0, z0, factors, masked=False, row0=0, nrows=None, block=512):
    """``rank_pairs`` for the batch whose descriptor columns are all ``d0`` and whose style column ``k`` is
    ``factors[k] * z0`` (``factors[k] != 0``, the products exact): one column's pair pass.  ``p_k = factors[k] p_0``, so a
    negative factor swaps the two classes: n+ <-> n-, S+ = f S-_0, g+ <-> g-."""
    d0, z0 = np.asarray(d0, np.float64), np.asarray(z0, np.float64)
    B, K = len(z0), len(factors)
    nrows = B - row0 if nrows is None else nrows
    lab = np.isfinite(d0) if masked else np.ones(B, bool)
    npos, nneg, sp, sn, m, gp, gn, g0 = _pair_column(d0, z0, lab, row0, nrows, block)
    P = Pairs(nrows, K)
    for k, f in enumerate(factors):
        assert f != 0
        P.m[k], P.gzero[:, k] = m, g0
        if f > 0:
            P.npos[k], P.nneg[k], P.spos[k], P.sneg[k], P.gpos[:, k], P.gneg[:, k] = npos, nneg, f * sp, f * sn, gp, gn
        else:
            P.npos[k], P.nneg[k], P.spos[k], P.sneg[k], P.gpos[:, k], P.gneg[:, k] = nneg, npos, f * sn, f * sp, gn, gp
    return P


def rank_finish(totals, P, n_all, activate=False, masked=False, scale=1.0):
    """``dict(loss, dz [nrows, K], c [K], norm [K])`` from the totals ``[4 | 5][16]`` of the WHOLE batch (summed over
    the ranks) and one rank's ``Pairs`` (its g+-):

        c_k = max(n-, 1) / max(max(n+, 1), max(n-, 1)) with ``activate``, else 1
        norm_k = (n_all^2 - n_all) K, masked: max(m_k^2 - m_k, 1) K
        loss = -sum_k (c_k S+_k + S-_k) / norm_k,  dz[i][k] = -scale (2 / norm_k) (c_k g+_ik + g-_ik)."""
    K = P.gpos.shape[1]
    t = np.asarray(totals, np.float64)
    c, norm = np.ones(K), np.zeros(K)
    loss = []
    for k in range(K):
        if activate:
            n_same, n_opp = max(t[0, k], 1.0), max(t[1, k], 1.0)
            c[k] = n_opp / max(n_same, n_opp)
        norm[k] = (max(t[4, k] * t[4, k] - t[4, k], 1.0) if masked else float(n_all) * n_all - n_all) * K
        loss.append(-(c[k] * t[2, k] + t[3, k]) / norm[k])
    dz = -scale * (2.0 / norm)[None, :] * (c[None, :] * P.gpos + P.gneg)
    return dict(loss=math.fsum(loss), dz=dz, c=c, norm=norm)


def rank_tie_term(P, norm, scale=1.0):
    """What autograd of the literal loss has beyond ``rank_finish``'s dz: ``-scale (2 / norm_k) gzero`` (see ``Pairs``)."""
    return -scale * (2.0 / norm)[None, :] * P.gzero


def rank_loss(d, z, activate=False, masked=False, P=None):
    """The loss on one whole batch: ``rank_finish`` of its own totals.  Returns the dict plus ``P``."""
    P = rank_pairs(d, z, masked) if P is None else P
    r = rank_finish(P.totals(masked), P, len(P.gpos), activate, masked)
    r["P"] = P
    return r


def rank_dz_floor(P, c, norm, scale=1.0):
    """The kernel forms ``f (c g+ + g-)`` in three fp32 operations on exact integers g+-: an absolute error of at most
    ``4 u (|c| |g+| + |g-|) 2 scale / norm`` per element (u = 2^-24; the fourth u is the rounding of f and c)."""
    return 4 * U32 * (np.abs(c)[None, :] * np.abs(P.gpos) + np.abs(P.gneg)) * 2.0 * scale / norm[None, :]


# ------------------------------------------------------------------------------------------------- recon, smooth, MSE
def recon_loss(x, y, scale):
    """``dict(loss, dy, mx, my, r, c)``.  Plain: ``mean((y - x)^2)``.  ``scale``: with the row means ``mx``, ``my`` and
    ``r = |my| / |mx|``, ``loss = 0.1 mean((r - 1)^2) + mean((y - x c)^2)``, ``c`` the DETACHED ``r`` clamped to
    [0.7, 1.3]; the gradient of the first term reaches ``y`` through ``|my|``: ``0.2 (r - 1) sign(my) / (|mx| L B)``."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    B, L = x.shape
    N = B * L
    if not scale:
        e = y - x
        return dict(loss=float((e * e).sum() / N), dy=2.0 * e / N, mx=None, my=None, r=None, c=np.ones(B))
    mx, my = x.mean(1), y.mean(1)
    r = np.abs(my) / np.abs(mx)
    c = np.clip(r, 0.7, 1.3)
    e = y - x * c[:, None]
    loss = 0.1 * float(((r - 1.0) ** 2).sum()) / B + float((e * e).sum()) / N
    gs = 0.2 * (r - 1.0) * np.sign(my) / (np.abs(mx) * L * B)
    return dict(loss=loss, dy=2.0 * e / N + gs[:, None], mx=mx, my=my, r=r, c=c)


def smooth_matrix(taps, L):
    """The L x L replicate-pad smoothing matrix: ``(G x)_l = sum_t w_t x[clamp(l + t - half, 0, L - 1)]``."""
    w = np.asarray(taps, np.float64)
    half = (len(w) - 1) // 2
    G = np.zeros((L, L))
    for l in range(L):
        for t in range(len(w)):
            G[l, min(max(l + t - half, 0), L - 1)] += w[t]
    return G


def smooth_loss(x, taps):
    """``(loss, dx)``: ``loss = mean((x - G x)^2)``, ``dx = (2 / N) (I - G)^T (x - G x)`` per row."""
    x = np.asarray(x, np.float64)
    B, L = x.shape
    G = smooth_matrix(taps, L)
    e = x - x @ G.T
    return float((e * e).sum()) / (B * L), (2.0 / (B * L)) * (e - e @ G)


def mse(a, b):
    a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    e = a - b
    return float((e * e).sum()) / len(e), 2.0 * e / len(e)


def softplus(v):
    v = np.asarray(v, np.float64)
    return np.maximum(v, 0.0) + np.log1p(np.exp(-np.abs(v)))


def sigmoid(v):
    v = np.asarray(v, np.float64)
    e = np.exp(-np.abs(v))
    return np.where(v >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def bce_pair(o, n_real):
    """``(loss, dlogits)``: mean softplus(-o) over the first ``n_real`` logits + mean softplus(o) over the rest."""
    o = np.asarray(o, np.float64)
    n_fake = len(o) - n_real
    loss = float(softplus(-o[:n_real]).sum()) / n_real + float(softplus(o[n_real:]).sum()) / n_fake
    s = sigmoid(o)
    return loss, np.concatenate([(s[:n_real] - 1.0) / n_real, s[n_real:] / n_fake])


def finalize(partials, scale=1.0):
    """``raae_loss_finalize``: the exactly rounded sum of the partials times ``scale``."""
    return math.fsum(float(p) for p in np.asarray(partials).ravel()) * float(scale)


# ---------------------------------------------------------------------------------------------------- style BatchNorm
def bn_stats(rows=None, count=0, running=None):
    """``(mean, rstd, updated running (mean, var) | None)``: train mode from partial rows ``[n][C][2]`` = {sum, sum of
    squares}, eval mode (``rows is None``) from the running buffers."""
    if rows is None:
        return running[0], 1.0 / np.sqrt(running[1] + EPS), None
    tot = np.asarray(rows, np.float64).sum(0)
    mean = tot[:, 0] / count
    var = np.maximum(tot[:, 1] / count - mean * mean, 0.0)
    new = None
    if running is not None:
        unb = var * count / (count - 1) if count > 1 else var
        new = ((1 - MOMENTUM) * running[0] + MOMENTUM * mean, (1 - MOMENTUM) * running[1] + MOMENTUM * unb)
    return mean, 1.0 / np.sqrt(var + EPS), new


def partial_rows(z, nrows):
    """``[nrows][C][2]`` float64 {sum, sum of squares} of ``z [B, C]`` split along the batch (empty slices give 0)."""
    z = np.asarray(z, np.float64)
    return np.stack([np.stack([s.sum(0), (s * s).sum(0)], 1) for s in np.array_split(z, nrows)])


def style_bn_fwd(z, rows=None, count=0, running=None):
    """``(styles, updated running | None)``."""
    mean, rstd, new = bn_stats(rows, count, running)
    return (np.asarray(z, np.float64) - mean[None, :]) * rstd[None, :], new


def style_bn_bwd(dy, y, rstd, scale=1.0):
    """``dz = rstd (g - mean(g) - y mean(g y))``, ``g = scale dy``, the means over the batch."""
    g = scale * np.asarray(dy, np.float64)
    y = np.asarray(y, np.float64)
    return rstd[None, :] * (g - g.mean(0)[None, :] - y * (g * y).mean(0)[None, :])


# ------------------------------------------------------------------------------------------------------ discriminator
def disc_input(z_real, styles, noise=None, sigma=0.0):
    x = np.concatenate([np.asarray(z_real, np.float64), np.asarray(styles, np.float64)])
    return x if noise is None else x + float(sigma) * np.asarray(noise, np.float64)


def _prelu(z, s):
    return np.where(z > 0, z, z * s[None, :])


def disc_fused(z_real, styles, noise, sigma, m1, m2, w1, b1, s1, w2, b2, s2, w3, b3, alpha):
    """The adversarial branch: ``x = [z_real; styles] + sigma noise`` -> Linear / PReLU / Dropout (multipliers ``m1``,
    ``m2`` or None) twice -> Linear -> BCE-with-logits against ones for the first rows and zeros for the rest.  Returns
    ``dict(loss, dw1, db1, ds1, dw2, db2, ds2, dw3, db3, dstyles, z1, z2)``; ``dstyles = -alpha dL/dstyles``."""
    n_real = len(z_real)
    x = disc_input(z_real, styles, noise, sigma)
    z1 = x @ w1.T + b1[None, :]
    a1 = _prelu(z1, s1) * (1.0 if m1 is None else m1)
    z2 = a1 @ w2.T + b2[None, :]
    a2 = _prelu(z2, s2) * (1.0 if m2 is None else m2)
    o = a2 @ w3.reshape(-1) + float(np.asarray(b3).reshape(-1)[0])
    loss, dl = bce_pair(o, n_real)
    r = dict(loss=loss, z1=z1, z2=z2)
    r["dw3"], r["db3"] = (dl @ a2).reshape(1, -1), np.array([dl.sum()])
    da2 = dl[:, None] * w3.reshape(1, -1) * (1.0 if m2 is None else m2)
    g2 = np.where(z2 > 0, da2, da2 * s2[None, :])
    r["ds2"] = np.where(z2 > 0, 0.0, da2 * z2).sum(0)
    r["dw2"], r["db2"] = g2.T @ a1, g2.sum(0)
    da1 = (g2 @ w2) * (1.0 if m1 is None else m1)
    g1 = np.where(z1 > 0, da1, da1 * s1[None, :])
    r["ds1"] = np.where(z1 > 0, 0.0, da1 * z1).sum(0)
    r["dw1"], r["db1"] = g1.T @ x, g1.sum(0)
    r["dstyles"] = -float(alpha) * (g1 @ w1)[n_real:]
    return r


def near_zero_rows(z1, z2, rel=1e-5):
    """Rows with a hidden pre-activation that is pure rounding residue: ``|z| < rel max|z|`` in either hidden layer.
    Only there may an fp32 evaluation take the other PReLU slope."""
    return (np.abs(z1) < rel * np.abs(z1).max()).any(1) | (np.abs(z2) < rel * np.abs(z2).max()).any(1)


# ------------------------------------------------------------------------------------------- mirror of the dispatch
RANK_TJ, RANK_MAXWG, RANK_MAXNJ, RANK_JC, MAX_PARTS = 256, 2048, 16, 8, 512
RANK_WORK_RECORD = 512                      # sizeof(RankWork): 2 x 16 int64 + 2 x 16 doubles
RANK_PART_BYTES = RANK_MAXWG * RANK_WORK_RECORD
DISC_TILE, DISC_MAXWG, DISC_MFMA_ROWS = 16, 256, 2048
# static LDS of a smoothness kernel, an UPPER ESTIMATE read off the source, not taken from the code object: block_sum
# scratch 128 + the in-kernel finish's flag 4 and scratch 128 + the table (_m) kernels' SmoothArgs copy of about 200
# bytes (33 taps) + alignment.  Used only to compare 8 L floats of dynamic LDS with the device limit.
SMOOTH_STATIC_LDS = 512


def grid_for(n, per_block, cap):
    return int(min(max((n + per_block - 1) // per_block, 1), cap))


def rank_grid(n_all, nrows, n_aux):
    """``(R, nj, jchunk, nwg)`` of the pair pass: rows per thread, column blocks, columns per block, workgroups."""
    ipb = 32 // n_aux
    R = 4 if nrows > 1024 else 1
    groups = (nrows + ipb * R - 1) // (ipb * R)
    nj = 1
    if n_all > 1024 and groups < 1024:
        nj = max(min((1024 + groups - 1) // groups, RANK_MAXNJ, n_all // RANK_TJ), 1)
    jchunk = ((n_all + nj - 1) // nj + RANK_TJ - 1) // RANK_TJ * RANK_TJ
    ni = min(groups, RANK_MAXWG // nj)
    return R, nj, jchunk, ni * nj


def rank_form(n_all, nrows, n_aux, masked):
    """The pair-pass form of a launch: the template instance and the edges of its geometry."""
    R, nj, jchunk, nwg = rank_grid(n_all, nrows, n_aux)
    ipb = 32 // n_aux
    groups = (nrows + ipb * R - 1) // (ipb * R)
    return dict(KA=n_aux, R=R, masked=bool(masked), nj=nj, nwg=nwg, multi_block=nj > 1,
                empty_block=(nj - 1) * jchunk >= n_all, stride=groups > nwg // nj,
                idle_slots=32 - ipb * n_aux, ragged_tile=n_all % RANK_TJ != 0)


def recon_nparts(B):
    return grid_for(B, 4, MAX_PARTS)


smooth_nparts = recon_nparts


def mse_nparts(n):
    return grid_for(n, 1024, MAX_PARTS)


def smooth_instance(ntaps):
    return "taps17" if ntaps == 17 else "generic"


def smooth_lds_bytes(L):
    """Dynamic LDS of a smoothness launch (four waves x {row, residual} x L floats) plus the estimate of the static."""
    return 8 * L * 4 + SMOOTH_STATIC_LDS


def disc_instance(n_real, n_fake, force=None):
    """``(instance, nslab)``: the matrix-core form from 2048 rows; one slab per workgroup, 256 at most.  ``force``: the
    value of the ``RAAE_DISC_MFMA`` tuning override (read once when the library loads): 0 / non-zero forces a form."""
    n = n_real + n_fake
    mm = n >= DISC_MFMA_ROWS if force is None or force < 0 else force != 0
    return ("mfma" if mm else "valu"), min((n + DISC_TILE - 1) // DISC_TILE, DISC_MAXWG)


def style_fwd_grid(B, C):
    return grid_for(B * C, 256, 256)


GLUE_CAPS = dict(disc_input=1024, scale_by_dev=1024, gather_batch=2048)      # workgroups of 256 threads
