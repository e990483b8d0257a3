"""Float64 reference of one fused dense layer (``csrc/raae_dense.hip``: ``raae_dense_fwd*`` / ``raae_dense_bwd*``),
forward and backward, written out with plain torch operations on the CPU -- its own formulas, no autograd.  The oracle
of ``test_dense_kernels_gpu.py``; ``test_dense_reference_cpu.py`` pins it to float64 autograd of ``nn.Linear`` /
``nn.PReLU`` / ``nn.BatchNorm1d(affine=False)``.  Not a conftest: tests import it.

One layer (``include/rankaae_hip.h``)::

    a    = PReLU(x, slope)                          in_kind != IN_NONE
    y    = (a - mean) * rstd                        in_kind == IN_PRELU_BN_DROP
    xin  = y * mult                                 mult: dropout multipliers {0, 1/keep} or None
    z    = xin @ W^T + bias
    out  = z | softplus_beta2(z) | relu(z)          what is stored
    {sum, sumsq} of PReLU(z, out_slope) | z         OUT_STATS_PRELU | OUT_STATS_RAW

BatchNorm is ``affine=False``.  Train mode: mean and BIASED variance from the float64 partial rows
``[nparts][C][{sum, sumsq}]`` a producer emitted, ``rstd = 1 / sqrt(var + eps)``; the running statistics move by
``momentum`` towards {mean, UNBIASED variance}.  Eval mode (no partial rows): the running statistics.

bf16 storage (``RAAE_ST_*``).  ``ST_X`` and ``ST_MASK`` change nothing here: the caller passes the values the tensors
hold, already on the bf16 grid (a bf16 mask holds {0, 1} and ``mult`` is that times the fp32 ``mask_scale``).
``ST_Z`` rounds at the points where ``dense_fwd_tiles``' epilogue rounds:

1. ``z = round_bf16(acc + bias)`` BEFORE the output activation and BEFORE the statistics, so the activation and the
   ``{sum, sumsq}`` describe the rounded value -- what the next layer will read;
2. with a softplus or relu output, the activation of that rounded z is rounded A SECOND TIME at the store (relu of a
   bf16 value is a bf16 value, so only softplus moves there).

``raw`` of the result is the value before every rounding: what the per-element bf16 bound of the GPU suite is centred
on.

Backward of the same layer: ``dz`` from ``g`` by ``g_kind`` (``zout``: the layer's STORED output)::

    G_DIRECT    dz = g
    G_SOFTPLUS  dz = g * (1 - exp(-2 zout))         zout = softplus(z): 1 - exp(-2 softplus(z)) = sigmoid(2 z)
    G_RELU      dz = g [zout > 0]
    G_PRELU     da = g;                                         dz = da [z > 0] + slope * da [z <= 0]
    G_PRELU_BN  y = (PReLU(z) - mean) * rstd;  da = rstd * (g - m1 - y * m2),   m1 = sum g / n,  m2 = sum g y / n
    dslope = sum_rows da * z [z <= 0];  db = sum_rows dz;  dW = dz^T xin
    dx = (dz @ W) * mult  -- dL/d(BatchNorm output of the input transform);  dx_partials = {sum dx, sum dx * y_in}

``mask_hash`` is the counter-based dropout hash of ``csrc/raae_common.h`` in numpy ``uint32``.
"""
import numpy as np
import torch

IN_NONE, IN_PRELU_BN_DROP, IN_PRELU_DROP = 0, 1, 2
OUT_RAW, OUT_STATS_PRELU, OUT_STATS_RAW, OUT_SOFTPLUS, OUT_RELU = 0, 1, 2, 3, 4
G_DIRECT, G_SOFTPLUS, G_PRELU_BN, G_PRELU, G_RELU = 0, 1, 2, 3, 4
ST_X, ST_MASK, ST_Z = 1, 2, 4
EPS, MOMENTUM = 1e-5, 0.1


# ------------------------------------------------------------------------------------------------------ bf16 grid
def ulp_bf16(t):
    """Spacing of the bf16 grid at ``t`` (8 significant bits; subnormal spacing 2^-133 below 2^-126), float64."""
    a = np.abs(np.asarray(t, dtype=np.float64))
    e = np.frexp(a)[1] - 1                                   # a = f * 2^(e + 1), 0.5 <= f < 1
    return torch.from_numpy(np.atleast_1d(np.ldexp(1.0, np.maximum(e, -126) - 7)).reshape(np.shape(a)))


def round_bf16(t):
    """``t`` (any float tensor) rounded to the nearest bf16 value, ties to even, as float64: ONE rounding from the
    given precision (for float32 input: what ``v_cvt_pk_bf16_f32`` and ``tensor.to(torch.bfloat16)`` do).  Values that
    round past the largest finite bf16 become infinite; the sign of a zero is kept; NaN stays NaN."""
    x = t.detach().double().numpy()
    u = ulp_bf16(x).numpy()
    with np.errstate(invalid="ignore", over="ignore"):
        r = np.rint(x / u) * u                               # np.rint: half to even; x / u is exact (u a power of two)
    big = float(np.ldexp(1.0, 128))
    r = np.where(np.abs(r) >= big, np.copysign(np.inf, x), r)
    r = np.where(np.isfinite(x), r, x)
    return torch.from_numpy(np.asarray(r, dtype=np.float64)).reshape(t.shape)


# ------------------------------------------------------------------------------------------------------ dropout hash
def lowbias32(x):
    x = np.asarray(x, dtype=np.uint32).copy()
    x ^= x >> np.uint32(16)
    x *= np.uint32(0x7feb352d)
    x ^= x >> np.uint32(15)
    x *= np.uint32(0x846ca68b)
    x ^= x >> np.uint32(16)
    return x


def gen_params(keep):
    """(thr, inv) of a keep probability, as ``ops.make_gen`` forms them: from the FLOAT keep."""
    k32 = np.float32(keep)
    return min(0xFFFFFFFF, int(float(k32) * 4294967296.0)), np.float32(1.0) / k32


def mask_hash(k1, k2, offset, thr, n):
    """Keep flags (bool [n]) of elements 0..n-1 of a slot at ``offset``:
    ``lowbias32(lowbias32(e + offset + k1) ^ k2) < thr``, all sums modulo 2^32."""
    e = (np.arange(n, dtype=np.uint64) + np.uint64(int(offset) % 2 ** 32) + np.uint64(int(k1))).astype(np.uint32)
    return lowbias32(lowbias32(e) ^ np.uint32(k2)) < np.uint32(thr)


def step_keys(seed, ctr):
    """(k1, k2) that ``raae_step_tick`` / ``raae_step_begin`` store for a 64-bit seed and step counter."""
    m = 0xFFFFFFFF
    one = lambda v: int(lowbias32(np.array([v & m], dtype=np.uint32))[0])
    k1 = one((seed & m) ^ one((ctr & m) + 0x9E3779B9))
    k2 = one(((seed >> 32) & m) + 0x85EBCA6B + one(((ctr >> 32) & m) ^ k1))
    return k1, k2


# ------------------------------------------------------------------------------------------------------ pieces
def prelu(x, slope):
    return torch.where(x > 0, x, slope.view(1, -1) * x)


def softplus2(x):
    """torch.nn.Softplus(beta=2, threshold=20)."""
    return torch.where(2 * x > 20, x, 0.5 * torch.log1p(torch.exp(torch.clamp(2 * x, max=40.0))))


def col_stats(a):
    """{sum, sum of squares} per column of ``a`` [B, C] -> [C, 2]."""
    return torch.stack([a.sum(0), (a * a).sum(0)], 1)


def partial_rows(cols, nrows=2):
    """What a producer emits: ``nrows`` float64 partial rows [nrows, C, len(cols)], row r summing the r-th run of
    batch rows of every [B, C] tensor of ``cols``."""
    B = cols[0].shape[0]
    edges = [B * r // nrows for r in range(nrows + 1)]
    return torch.stack([torch.stack([c[edges[r]:edges[r + 1]].sum(0) for c in cols], 1) for r in range(nrows)])


def bn_from_rows(rows, count, eps=EPS):
    """(mean, rstd, unbiased variance) from partial rows [nparts, C, 2] of ``count`` elements per column."""
    tot = rows.double().sum(0)
    mean = tot[:, 0] / count
    var = torch.clamp(tot[:, 1] / count - mean * mean, min=0.0)
    unb = var * count / (count - 1.0) if count > 1 else var
    return mean, 1.0 / torch.sqrt(var + eps), unb


def running_update(running, mean, unb, momentum=MOMENTUM):
    rm, rv = running
    return (1.0 - momentum) * rm.double() + momentum * mean, (1.0 - momentum) * rv.double() + momentum * unb


def in_transform(x, in_kind, slope=None, rows=None, count=None, running=None, eps=EPS):
    """(y, mean, unbiased variance): the input after PReLU and BatchNorm, BEFORE the dropout multiplier."""
    x = x.double()
    if in_kind == IN_NONE:
        return x, None, None
    a = prelu(x, slope.double())
    if in_kind == IN_PRELU_DROP:
        return a, None, None
    if rows is not None:
        mean, rstd, unb = bn_from_rows(rows, count, eps)
    else:
        mean, rstd, unb = running[0].double(), 1.0 / torch.sqrt(running[1].double() + eps), None
    return (a - mean) * rstd, mean, unb


# ------------------------------------------------------------------------------------------------------ forward
def fwd(x, w, bias, in_kind=IN_NONE, slope=None, rows=None, count=None, running=None, mult=None, out_kind=OUT_RAW,
        out_slope=None, storage=0, eps=EPS, momentum=MOMENTUM):
    """One fused layer.  ``rows``/``count``: partial rows of PReLU(x) (train mode); ``running`` = (mean, var): read in
    eval mode (``rows is None``), updated in train mode.  Returns a dict:
    ``stored`` what the kernel writes; ``raw`` the same before every bf16 rounding; ``z`` the (rounded) pre-activation
    the statistics describe; ``stats`` [N, 2] or None; ``running`` the updated (mean, var) or None; ``y`` / ``xin``."""
    y, mean, unb = in_transform(x, in_kind, slope, rows, count, running, eps)
    xin = y if mult is None or in_kind == IN_NONE else y * mult.double()
    z_raw = xin @ w.double().t() + bias.double()
    z = round_bf16(z_raw) if storage & ST_Z else z_raw
    act = {OUT_SOFTPLUS: softplus2, OUT_RELU: lambda v: torch.clamp(v, min=0.0)}.get(out_kind, lambda v: v)
    stored = act(z)
    if storage & ST_Z:
        stored = round_bf16(stored)
    stats = None
    if out_kind == OUT_STATS_PRELU:
        stats = col_stats(prelu(z, out_slope.double()))
    elif out_kind == OUT_STATS_RAW:
        stats = col_stats(z)
    new_running = None
    if in_kind == IN_PRELU_BN_DROP and rows is not None and running is not None:
        new_running = running_update(running, mean, unb, momentum)
    return dict(stored=stored, raw=act(z_raw), z_raw=z_raw, z=z, stats=stats, running=new_running, y=y, xin=xin)


# ------------------------------------------------------------------------------------------------------ backward
def bwd(g, g_kind, x, w, zout=None, out_slope=None, out_rows=None, g_rows=None, count=None, in_kind=IN_NONE,
        slope=None, rows=None, mult=None, need_dx=True, eps=EPS):
    """Backward of the layer.  ``zout``: its stored output; ``out_rows``: partial rows of PReLU(zout) and ``g_rows``:
    partial rows {sum g, sum g y} (G_PRELU_BN); ``count``: batch rows.  Returns ``dw`` [N, K], ``db`` [N], ``dslope``
    [N] or None, ``dx`` [B, K] or None, ``dx_stats`` [K, 2] = {sum dx, sum dx * y_in} or None, ``dz``."""
    g = g.double()
    B = g.shape[0]
    count = B if count is None else count
    dslope = None
    if g_kind == G_DIRECT:
        dz = g
    elif g_kind == G_SOFTPLUS:
        dz = g * (1.0 - torch.exp(-2.0 * zout.double()))
    elif g_kind == G_RELU:
        dz = torch.where(zout.double() > 0, g, torch.zeros_like(g))
    else:
        z, s = zout.double(), out_slope.double()
        da = g
        if g_kind == G_PRELU_BN:
            mean, rstd, _ = bn_from_rows(out_rows, count, eps)
            yo = (prelu(z, s) - mean) * rstd
            tot = g_rows.double().sum(0)
            da = rstd * (g - tot[:, 0] / count - yo * (tot[:, 1] / count))
        pos = z > 0
        dz = torch.where(pos, da, da * s.view(1, -1))
        dslope = torch.where(pos, torch.zeros_like(da), da * z).sum(0)
    y, _, _ = in_transform(x, in_kind, slope, rows, count, None, eps)
    m = None if mult is None or in_kind == IN_NONE else mult.double()
    xin = y if m is None else y * m
    out = dict(dw=dz.t() @ xin, db=dz.sum(0), dslope=dslope, dz=dz, dx=None, dx_stats=None)
    if need_dx:
        dx = dz @ w.double()
        if m is not None:
            dx = dx * m
        out["dx"] = dx
        if in_kind == IN_PRELU_BN_DROP:
            out["dx_stats"] = torch.stack([dx.sum(0), (dx * y).sum(0)], 1)
    return out


# ------------------------------------------------------------------------------------------------------ autograd twin
def layer_autograd(g, g_kind, x, w, bias, out_slope=None, in_kind=IN_NONE, slope=None, mult=None, dtype=torch.float64,
                   eps=EPS):
    """NOT part of the reference: the same layer through torch autograd in ``dtype`` (train-mode BatchNorm on both
    sides), for the CPU cross-check (float64) and as the fp32 arbiter of the long gradient sums.  ``g`` is
    dL/d softplus(z) | relu(z) | z | PReLU(z) | BN(PReLU(z)) by ``g_kind``.  Returns ``dw, db, dslope, dx, z`` with
    ``dx`` taken at the BatchNorm output of the input transform (what the kernel calls dx)."""
    import torch.nn.functional as F
    c = lambda t: None if t is None else t.detach().to(dtype)
    x, g, mult = c(x), c(g), c(mult)
    wl, bl = c(w).requires_grad_(True), c(bias).requires_grad_(True)
    sl = c(out_slope).requires_grad_(True) if out_slope is not None else None
    with torch.enable_grad():
        y = x
        if in_kind != IN_NONE:
            y = F.prelu(x, c(slope))
            if in_kind == IN_PRELU_BN_DROP:
                y = F.batch_norm(y, None, None, training=True, eps=eps)
        y = y.detach().requires_grad_(True)
        xin = y * mult if (mult is not None and in_kind != IN_NONE) else y
        z = F.linear(xin, wl, bl)
        if g_kind == G_SOFTPLUS:
            o = F.softplus(z, beta=2)
        elif g_kind == G_RELU:
            o = torch.relu(z)
        elif g_kind == G_PRELU:
            o = F.prelu(z, sl)
        elif g_kind == G_PRELU_BN:
            o = F.batch_norm(F.prelu(z, sl), None, None, training=True, eps=eps)
        else:
            o = z
        (o * g).sum().backward()
    return wl.grad, bl.grad, (sl.grad if sl is not None else None), y.grad, z.detach()
