"""Float64 reference of the per-layer conv-network kernels (``csrc/raae_conv.hip``, ``raae_conv_tiled.inc``,
``raae_conv_strip.inc``, ``raae_head.inc``) written out without autograd, and a pure-Python mirror of their dispatch.
The oracle of ``test_conv_kernels_gpu.py``; ``test_conv_reference_cpu.py`` pins it to float64 torch autograd of the
same composition.  Not a conftest: tests import it.

A VIEW is ``mask * BatchNorm(PReLU(raw))`` with every stage optional; BatchNorm (affine=False) reads partial rows
``[n][C]{sum, sumsq}`` and a count in train mode, the running buffers in eval mode.  A GRADIENT SPEC turns the incoming
gradient ``g`` into the gradient at a layer's raw output: BatchNorm backward from partial rows ``{sum g, sum g*y}`` (y
from ``u`` when given, else from PReLU(raw) / raw), then the PReLU, softplus(beta=2) or ReLU derivative; the latter two
read the ACTIVATED output as ``raw`` (``1 - exp(-2 out)`` is sigmoid(2 z)).
"""
import torch
import torch.nn.functional as F

from block_reference import chan_stats, prelu

OUT_RAW, OUT_STATS_PRELU, OUT_STATS_RAW, OUT_SOFTPLUS, OUT_RELU = 0, 1, 2, 3, 4
MAX_PARTS, BIG_ROWS, TILE_BUDGET, CT_MAXCH, CV_MAXC = 512, 1024, 10 * 1024, 8, 64
EPS, MOMENTUM = 1e-5, 0.1


def f32(t):
    """Round to fp32 and return as float64: what a kernel reads of a reference tensor."""
    return t.float().double()


def partial_rows(pairs, nrows):
    """[n][C][2] float64 rows of per-channel sums of the two [B, C, L] tensors, split along the batch."""
    a, b = pairs
    n = max(1, min(nrows, a.shape[0]))
    return torch.stack([torch.stack([x.sum((0, 2)), y.sum((0, 2))], 1)
                        for x, y in zip(a.tensor_split(n), b.tensor_split(n))])


# ------------------------------------------------------------------------------------------------ view, gradient spec
def bn_stats(rows=None, count=0, running=None):
    """(mean, rstd, updated running (mean, var) or None): train from partial rows, eval from the running buffers."""
    if rows is None:
        return running[0], 1.0 / torch.sqrt(running[1] + EPS), None
    tot = rows.sum(0)
    mean = tot[:, 0] / count
    var = (tot[:, 1] / count - mean * mean).clamp_min(0.0)
    new = None
    if running is not None:
        unb = var * count / (count - 1) if count > 1 else var
        new = ((1 - MOMENTUM) * running[0] + MOMENTUM * mean, (1 - MOMENTUM) * running[1] + MOMENTUM * unb)
    return mean, 1.0 / torch.sqrt(var + EPS), new


def view(raw, slope=None, bn=None, mask=None):
    """(value, y, updated running statistics): y = the BatchNorm output before the mask (``view_y`` of the kernels).
    ``bn``: dict(rows=, count=, running=) or None."""
    x, new = raw, None
    if slope is not None:
        x = prelu(x, slope)
    if bn is not None:
        mean, rstd, new = bn_stats(bn.get("rows"), bn.get("count", 0), bn.get("running"))
        x = (x - mean.view(1, -1, 1)) * rstd.view(1, -1, 1)
    return (x * mask if mask is not None else x), x, new


def grad_spec(g, raw=None, slope=None, bn=None, g_rows=None, u=None, act=OUT_RAW):
    """(d raw, d slope per channel or None, d at the activation output).  ``bn``: dict(rows=, count=) of the tensor the
    BatchNorm normalised (u, else PReLU(raw), else raw)."""
    da = g
    if bn is not None:
        uu = u if u is not None else (prelu(raw, slope) if slope is not None else raw)
        mean, rstd, _ = bn_stats(bn["rows"], bn["count"])
        y = (uu - mean.view(1, -1, 1)) * rstd.view(1, -1, 1)
        m = g_rows.sum(0) / bn["count"]
        da = rstd.view(1, -1, 1) * (g - m[:, 0].view(1, -1, 1) - y * m[:, 1].view(1, -1, 1))
    dr, ds = da, None
    if slope is not None:
        dr = torch.where(raw > 0, da, da * slope.view(1, -1, 1))
        ds = torch.where(raw > 0, torch.zeros_like(da), da * raw).sum((0, 2))
    elif act == OUT_SOFTPLUS:
        dr = da * (1.0 - torch.exp(-2.0 * raw))
    elif act == OUT_RELU:
        dr = torch.where(raw > 0, da, torch.zeros_like(da))
    return dr, ds, da


def activation(z, act):
    if act == OUT_SOFTPLUS:
        return torch.where(2 * z > 20, z, 0.5 * torch.log1p(torch.exp(torch.clamp(2 * z, max=20.0))))
    return z.clamp_min(0.0) if act == OUT_RELU else z


def out_stats(z, stats_kind, out_slope=None):
    """{sum, sumsq} per channel of what a forward kernel's statistics describe (always the pre-activation)."""
    if stats_kind == OUT_RAW:
        return None
    return chan_stats(prelu(z, out_slope) if stats_kind == OUT_STATS_PRELU else z)


# ------------------------------------------------------------------------------------------------ the linear layers
class Conv:
    """Conv1d (zero or replicate pad, stride, groups) or ConvTranspose1d with K == stride, in torch's weight layout."""

    def __init__(self, Cin, Lin, Cout, K, stride=1, pad=0, rep=False, groups=1, transposed=False):
        self.Cin, self.Lin, self.Cout, self.K, self.stride, self.pad = Cin, Lin, Cout, K, stride, pad
        self.rep, self.groups, self.transposed = bool(rep), groups, bool(transposed)
        self.Lout = Lin * stride if transposed else (Lin + 2 * pad - K) // stride + 1
        self.cig, self.cog = Cin // groups, Cout // groups
        self.wshape = (Cin, self.cog, K) if transposed else (Cout, self.cig, K)
        self.fan = self.cig * K

    def _windows(self, x):
        p = self.pad
        if p:
            xp = torch.cat([x[:, :, :1].expand(-1, -1, p), x, x[:, :, -1:].expand(-1, -1, p)], 2) if self.rep else \
                torch.cat([x.new_zeros(x.shape[0], x.shape[1], p), x, x.new_zeros(x.shape[0], x.shape[1], p)], 2)
        else:
            xp = x
        win = xp.unfold(2, self.K, self.stride)[:, :, :self.Lout]              # [B, Cin, Lout, K]
        return win.reshape(x.shape[0], self.groups, self.cig, self.Lout, self.K)

    def fwd(self, x, w, b):
        B, G = x.shape[0], self.groups
        if self.transposed:
            o = torch.einsum("bgcl,gcot->bgolt", x.reshape(B, G, self.cig, self.Lin), w.reshape(G, self.cig, self.cog, self.K))
        else:
            o = torch.einsum("bgclk,gock->bgol", self._windows(x), w.reshape(G, self.cog, self.cig, self.K))
        return o.reshape(B, self.Cout, self.Lout) + b.view(1, -1, 1)

    def bwd(self, x, w, g):
        """(d x, d w, d bias) for the output gradient ``g`` at input ``x``."""
        B, G, K, s, p = x.shape[0], self.groups, self.K, self.stride, self.pad
        db = g.sum((0, 2))
        if self.transposed:
            gg = g.reshape(B, G, self.cog, self.Lin, K)
            wg = w.reshape(G, self.cig, self.cog, K)
            dx = torch.einsum("bgolt,gcot->bgcl", gg, wg).reshape(B, self.Cin, self.Lin)
            dw = torch.einsum("bgolt,bgcl->gcot", gg, x.reshape(B, G, self.cig, self.Lin)).reshape(self.wshape)
            return dx, dw, db
        gg = g.reshape(B, G, self.cog, self.Lout)
        wg = w.reshape(G, self.cog, self.cig, K)
        dw = torch.einsum("bgol,bgclk->gock", gg, self._windows(x)).reshape(self.wshape)
        dxp = x.new_zeros(B, G, self.cig, self.Lin + 2 * p)
        for k in range(K):
            dxp[:, :, :, k:k + s * (self.Lout - 1) + 1:s] += torch.einsum("bgol,goc->bgcl", gg, wg[:, :, :, k])
        dxp = dxp.reshape(B, self.Cin, -1)
        dx = dxp[:, :, p:p + self.Lin].clone()
        if p and self.rep:
            dx[:, :, 0] += dxp[:, :, :p].sum(2)
            dx[:, :, -1] += dxp[:, :, p + self.Lin:].sum(2)
        return dx, dw, db

    def torch_fn(self):
        """The same layer through torch's own operators (any dtype): what the CPU test differentiates."""
        if self.transposed:
            return lambda x, w, b: F.conv_transpose1d(x, w, b, stride=self.stride, groups=self.groups)
        if self.pad and self.rep:
            return lambda x, w, b: F.conv1d(F.pad(x, (self.pad, self.pad), mode="replicate"), w, b, stride=self.stride,
                                            groups=self.groups)
        return lambda x, w, b: F.conv1d(x, w, b, stride=self.stride, padding=self.pad, groups=self.groups)


class LenLin:
    """Linear along the length axis: out[b][c][e] = bias[e] + sum_l w[e][l] x[b][c][l]."""

    def __init__(self, C, Lin, E):
        self.Cin = self.Cout = C
        self.Lin, self.Lout, self.E, self.wshape, self.fan = Lin, E, E, (E, Lin), Lin

    def fwd(self, x, w, b):
        return x @ w.t() + b

    def bwd(self, x, w, g):
        return g @ w, torch.einsum("bce,bcl->el", g, x), g.sum((0, 1))

    def torch_fn(self):
        return lambda x, w, b: F.linear(x, w, b)


def layer_fwd(op, raw, w, b, slope=None, bn=None, mask=None, stats_kind=OUT_RAW, out_slope=None, act=OUT_RAW):
    """dict(z = pre-activation, out = what the kernel stores, stats, running) of one forward launch."""
    v, _, run = view(raw, slope, bn, mask)
    z = op.fwd(v, w, b)
    return dict(z=z, out=activation(z, act), stats=out_stats(z, stats_kind, out_slope), running=run)


def layer_bwd(op, go, w, raw, slope=None, bn=None, mask=None, din0=None):
    """Backward of one layer for the gradient spec ``go`` (keyword dict of ``grad_spec``): ``din`` = gradient at the
    view's BatchNorm output (mask applied, ``din0`` added when accumulating), ``pairs`` = {sum din, sum din*y}, ``dw``
    ``db`` ``dslope`` (of the spec's PReLU, None without one)."""
    v, y, _ = view(raw, slope, bn, mask)
    dr, ds, _ = grad_spec(**go)
    dx, dw, db = op.bwd(v, w, dr)
    if mask is not None:
        dx = dx * mask
    if din0 is not None:
        dx = dx + din0
    return dict(din=dx, pairs=torch.stack([dx.sum((0, 2)), (dx * y).sum((0, 2))], 1), dw=dw, db=db, dslope=ds, dr=dr)


def sum3(views):
    """y = the sum of three views, its {sum, sumsq}, the running statistics the middle view's BatchNorm updates."""
    vals = [view(**v) for v in views]
    y = vals[0][0] + vals[1][0] + vals[2][0]
    return y, chan_stats(y), vals[1][2]


def grad_materialize(go, draw0=None):
    dr, ds, _ = grad_spec(**go)
    return (dr + draw0 if draw0 is not None else dr), ds


def layer_autograd(op, G, X, w, b, slope=None, bn=None, mask=None, out_slope=None, out_bn=False, u_add=None,
                   act=OUT_RAW, dtype=torch.float64):
    """The same composition through torch autograd in ``dtype``: value = mask * BN(PReLU(X)); z = layer(value);
    uu = PReLU(z) | act(z) (+ ``u_add``); loss = sum(G * BN(uu) | G * uu).  BatchNorm: batch statistics for
    ``bn="train"`` / ``out_bn``, running buffers for ``bn=(mean, var)``.  Returns dict(out, din = gradient at the
    BatchNorm output of the view, dw, db, dslope, running = buffers after the train-mode forward)."""
    c = lambda t: None if t is None else t.detach().to(dtype)
    Xl, wl, bl = (c(t).clone().requires_grad_(True) for t in (X, w, b))
    a = Xl if slope is None else F.prelu(Xl, c(slope))
    run = None
    if isinstance(bn, str):
        run = (torch.zeros(X.shape[1], dtype=dtype), torch.ones(X.shape[1], dtype=dtype))
        y = F.batch_norm(a, run[0], run[1], training=True, momentum=MOMENTUM, eps=EPS)
    elif bn is not None:
        y = F.batch_norm(a, c(bn[0]), c(bn[1]), training=False, eps=EPS)
    else:
        y = a * 1.0
    y.retain_grad()
    z = op.torch_fn()(y * c(mask) if mask is not None else y, wl, bl)
    so = None
    if out_slope is not None:
        so = c(out_slope).clone().requires_grad_(True)
        uu = F.prelu(z, so)
    else:
        uu = F.softplus(z, beta=2) if act == OUT_SOFTPLUS else torch.relu(z) if act == OUT_RELU else z
    out = z if out_slope is not None else uu
    if u_add is not None:
        uu = uu + c(u_add)
    t = F.batch_norm(uu, None, None, training=True, eps=EPS) if out_bn else uu
    (t * c(G)).sum().backward()
    return dict(out=out.detach(), uu=uu.detach(), din=y.grad, dw=wl.grad, db=bl.grad,
                dslope=None if so is None else so.grad, running=run)


# ------------------------------------------------------------------------------------------------ the dispatch, mirrored
# Environment defaults (no RAAE_PICK_* / RAAE_BIG_MASK_* / RAAE_WGRAD_* set) and raae_tile_hint = 1.
STRIP_INSTANCES = ((4, 4, 11, 1), (4, 4, 11, 2), (1, 4, 11, 2), (4, 4, 7, 2), (4, 4, 5, 1), (4, 4, 5, 2))
# Compiled, never selected: conv_fwd_strip refuses a launch whose two LDS tiles exceed 72 KB.  A tile holds S = 512 /
# (Lout / 4) samples of Cin rows of Lin + 16 floats, so the pair is 16384 * Cin * (stride + 16 / Lout) bytes: with Cin =
# 4 and stride 2 more than 128 KB at every length.  Such layers run the tiled kernels.
UNSELECTABLE = {
    "strip(4,4,11,2)": "two LDS tiles need 65536 * (2 + 16 / Lout) bytes > 72 KB at every Lout",
    "strip(4,4,7,2)": "two LDS tiles need 65536 * (2 + 16 / Lout) bytes > 72 KB at every Lout",
    "strip(4,4,5,2)": "two LDS tiles need 65536 * (2 + 16 / Lout) bytes > 72 KB at every Lout",
}


def cdiv(a, b):
    return (a + b - 1) // b


def slices_for(per_channel):
    return max(1, min(MAX_PARTS, cdiv(per_channel, 256)))


def pick_S(floats_per_sample, outputs_per_sample, B, budget, min_out, small_floats=2200, small_mult=8, small_div=256):
    S = max(1, cdiv(min_out, outputs_per_sample))
    cap = budget // max(floats_per_sample, 1)
    want = cdiv(B, 1024)
    if floats_per_sample <= small_floats:
        want = cdiv(B, small_div)
    if want > small_mult * S and floats_per_sample <= small_floats:
        want = small_mult * S
    elif want > 4 * S:
        want = 4 * S
    return max(1, min(max(S, want), cap, B))


def head_grid(nq, unroll):
    per_trip = max(1, min(unroll, nq // (256 * 256)))
    return max(1, min(256, cdiv(nq, 256 * per_trip)))


def conv_nw(cv):
    return cv.Cin * cv.cog * cv.K if cv.transposed else cv.Cout * cv.cig * cv.K


def conv_ok(cv, Lout=None):
    Lout = cv.Lout if Lout is None else Lout
    if min(cv.Cin, cv.Cout, cv.K, cv.stride, cv.groups) < 1 or cv.K > 16:
        return False
    if cv.Cin % cv.groups or cv.Cout % cv.groups or cv.Cin > CV_MAXC or cv.Cout > CV_MAXC:
        return False
    if cv.transposed:
        return cv.K == cv.stride and cv.pad == 0 and Lout == cv.Lin * cv.stride
    return Lout == (cv.Lin + 2 * cv.pad - cv.K) // cv.stride + 1


def head_shape_ok(cv, has_bn, has_slope, has_mask, raw_aligned=True):
    return (cv.K == 1 and cv.stride == 1 and cv.pad == 0 and cv.groups == 1 and not cv.transposed and cv.Cout == 1 and
            cv.Cin in (4, 8) and cv.Lin == cv.Lout and cv.Lin % 4 == 0 and has_bn and not has_slope and not has_mask and
            raw_aligned)


def strip_form(B, cv, has_mask, aligned=True):
    """The strip instance ``raae_conv_fwd`` selects and its row count, or None."""
    if cv.transposed or cv.groups != 1 or cv.pad != (cv.K - 1) // 2 or cv.K % 2 == 0:
        return None
    if cv.Lin % 4 or cv.Lout % 4 or cv.Lout > 1024 or cv.Lout * cv.stride != cv.Lin:
        return None
    if B * cv.Cout * cv.Lout < 1 << 20 or not aligned:
        return None
    S = 512 // (cv.Lout // 4)
    if 2 * S * cv.Cin * (cv.Lin + 16) * 4 > 72 * 1024:
        return None
    if (cv.Cin, cv.Cout, cv.K, cv.stride) not in STRIP_INSTANCES:
        return None
    l4 = cv.Lin >> 2
    if l4 & (l4 - 1):
        return None
    return f"strip({cv.Cin},{cv.Cout},{cv.K},{cv.stride}{',mask' if has_mask else ''})", min(cdiv(B, S), MAX_PARTS)


def _tiled(B, S, cap=MAX_PARTS, big=True):
    return ("tiled_big" if big and B >= BIG_ROWS else "tiled"), min(cdiv(B, S), cap)


def conv_fwd_form(B, cv, stats_kind=OUT_RAW, has_bn=False, has_slope=False, has_mask=False, aligned=True):
    """(form, partial rows returned) of ``raae_conv_fwd``.  ``aligned``: raw, mask and out start on 16 bytes."""
    if stats_kind == OUT_RAW and head_shape_ok(cv, has_bn, has_slope, has_mask, aligned) and aligned:
        return f"head{cv.Cin}", 0
    s = strip_form(B, cv, has_mask, aligned)
    if s:
        return s
    per_in = cv.Cin * (cv.Lin + 2 * (0 if cv.transposed else cv.pad))
    if conv_nw(cv) <= 1024 and (stats_kind == OUT_RAW or cv.Cout <= CT_MAXCH) and per_in <= TILE_BUDGET:
        return _tiled(B, pick_S(per_in, cv.Cout * cv.Lout, B, TILE_BUDGET, 256))
    return "generic", slices_for(B * cv.Lout)


def conv_bwd_data_form(B, cv, partials):
    per_g = cv.Cout * cv.Lout
    if conv_nw(cv) <= 1024 and (not partials or cv.Cin <= CT_MAXCH) and per_g <= TILE_BUDGET:
        return _tiled(B, pick_S(per_g, cv.Cin * cv.Lin, B, TILE_BUDGET, 256))
    return "generic", slices_for(B * cv.Lin)


def conv_bwd_weight_form(B, cv, dslope):
    per = (2 if dslope else 1) * cv.Cout * cv.Lout + cv.Cin * (cv.Lin + 2 * (0 if cv.transposed else cv.pad))
    if conv_nw(cv) <= 1024 and cv.Cout <= 8 and per <= TILE_BUDGET:
        S = min(pick_S(per, cv.Lin if cv.transposed else cv.Lout, B, TILE_BUDGET, 256), cdiv(B, 128))
        return _tiled(B, S, 128)
    return "generic", 1


def lenlin_fwd_form(B, C, Lin, E, stats_kind=OUT_RAW):
    wfl, per = E * Lin + E, C * Lin
    if (stats_kind == OUT_RAW or C <= CT_MAXCH) and wfl <= 2048 and per <= TILE_BUDGET - wfl:
        return _tiled(B, pick_S(per, C * E, B, TILE_BUDGET - wfl, 16 if Lin >= 64 else 256), big=False)
    return "generic", slices_for(B * E)


def lenlin_bwd_data_form(B, C, Lin, E, partials):
    wfl, per = E * Lin, C * E
    if (not partials or C <= CT_MAXCH) and wfl <= 2048 and per <= TILE_BUDGET - wfl:
        return _tiled(B, pick_S(per, C * Lin, B, TILE_BUDGET - wfl, 16 if E >= 64 else 256), big=False)
    return "generic", slices_for(B * Lin)


def lenlin_bwd_weight_form(B, C, Lin, E, dslope):
    per = (2 if dslope else 1) * C * E + C * Lin
    if E * Lin <= 1024 and E <= 256 and C <= CT_MAXCH and per <= TILE_BUDGET:
        return _tiled(B, pick_S(per, C, B, TILE_BUDGET, 64), 64, big=False)
    return "generic", 1


def sum3_form(B, L):
    return "generic", slices_for(B * L)


def grad_materialize_form(B, L):
    return "generic", max(1, min(64, cdiv(B * L, 1024)))


def head_fwd_grid(B, cv):
    return head_grid(B * (cv.Lin >> 2), 4 if cv.Cin <= 4 else 2)


def head_bwd_form(B, cv):
    g = head_grid(B * (cv.Lin >> 2), 2)
    return f"head{cv.Cin}", g
