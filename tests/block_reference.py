"""Float64 reference of one residual block (``rankaae_amd.model.EncodingBlock`` / ``DecodingBlock``), stage by stage:
every tensor the fused block kernels (``csrc/raae_block_fused.inc``) store or emit, forward and backward.  The oracle
of ``test_block_kernels_gpu.py``; ``test_block_reference_cpu.py`` pins it to the module's own forward and to float64
autograd.  Not a conftest: tests import it.

Dataflow (``rankaae_amd/nets_conv.py``)::

    R  = bn1(X)                                   T1 = conv1(R);  T2 = conv2(bn2(PReLU1(T1)))
    Sh = conv_short(R)  (or the identity)         E1 = fc1(mask * R);  E2 = fc2(PReLU(E1))
    E3 = conv_excit(bn_excit(PReLU(E2)))          (only when Cin != Cout)
    Y  = PReLU2(T2) + PReLUs(Sh) | R + PReLU(E3 | E2)

BatchNorm (affine=False) is written out: batch statistics (biased variance) in train mode, the running buffers in eval
mode.  PReLU and BatchNorm backward are written out too; only the vector-Jacobian product of a single linear layer
(conv / transposed conv / fc) is taken from torch, one layer at a time.  The PReLU branch of every backward stage is
read from ``sides[name]`` when given (a raw tensor of the same shape), from the reference's own raw tensor otherwise.
"""
import torch
import torch.nn.functional as F
from torch import nn


def _d(t):
    return None if t is None else t.detach().double()


def prelu(x, slope):
    """Per-channel (dim 1) PReLU."""
    return torch.where(x > 0, x, slope.view(1, -1, 1) * x)


def chan_stats(a):
    """{sum, sum of squares} per channel of ``a`` [B, C, L] -> [C, 2]."""
    return torch.stack([a.sum((0, 2)), (a * a).sum((0, 2))], 1)


def _layer_fn(mod):
    """(x, weight, bias) -> output of one linear layer of the block, in whatever precision the operands have."""
    if isinstance(mod, nn.Linear):
        return lambda x, w, b: F.linear(x, w, b)
    if isinstance(mod, nn.ConvTranspose1d):
        return lambda x, w, b: F.conv_transpose1d(x, w, b, stride=mod.stride[0], groups=mod.groups)
    p, rep = mod.padding[0], mod.padding_mode == "replicate"

    def conv(x, w, b):
        if p and rep:
            return F.conv1d(F.pad(x, (p, p), mode="replicate"), w, b, stride=mod.stride[0], groups=mod.groups)
        return F.conv1d(x, w, b, stride=mod.stride[0], padding=p, groups=mod.groups)
    return conv


def _layer(mod, x):
    return _layer_fn(mod)(x, _d(mod.weight), _d(mod.bias))


def _layer_vjp(mod, x, g):
    """(d input, d weight, d bias) of one linear layer at input ``x`` for the output gradient ``g``."""
    ops = [t.detach().clone().requires_grad_(True) for t in (x, _d(mod.weight), _d(mod.bias))]
    with torch.enable_grad():
        y = _layer_fn(mod)(*ops)
    return torch.autograd.grad(y, ops, g)


def _bn_forward(bn, a, train):
    """y, (mean, rstd), (new running mean, new running var) of BatchNorm1d(affine=False) on ``a`` [B, C, L]."""
    rm, rv = _d(bn.running_mean), _d(bn.running_var)
    if train:
        n = a.shape[0] * a.shape[2]
        mean = a.mean((0, 2))
        var = ((a - mean.view(1, -1, 1)) ** 2).mean((0, 2))
        unb = var * n / (n - 1) if n > 1 else var
        run = ((1 - bn.momentum) * rm + bn.momentum * mean, (1 - bn.momentum) * rv + bn.momentum * unb)
    else:
        mean, var, run = rm, rv, (rm, rv)
    rstd = 1.0 / torch.sqrt(var + bn.eps)
    return (a - mean.view(1, -1, 1)) * rstd.view(1, -1, 1), (mean, rstd), run


def _bn_backward(g, y, rstd):
    """Train-mode BatchNorm backward: (d input, {sum g, sum g*y} per channel)."""
    n = g.shape[0] * g.shape[2]
    s1, s2 = g.sum((0, 2)), (g * y).sum((0, 2))
    dx = rstd.view(1, -1, 1) * (g - (s1 / n).view(1, -1, 1) - y * (s2 / n).view(1, -1, 1))
    return dx, torch.stack([s1, s2], 1)


def _prelu_backward(g, raw, slope, side):
    """(d raw, d slope per channel); the branch is taken where ``side`` > 0."""
    side = raw if side is None else side
    pos = side > 0
    return torch.where(pos, g, slope.view(1, -1, 1) * g), torch.where(pos, torch.zeros_like(g), g * raw).sum((0, 2))


def forward(m, x, mask=None, train=True):
    """Forward of block ``m`` on ``x`` [B, Cin, Lin] (``mask``: the dropout-scale multipliers of ``dropout_1``'s input,
    or None).  Returns a dict of float64 tensors: raw ``T1 Sh E1 E2 T2 E3 Y`` (None where the block has no such
    layer), the views between them, ``stats`` = {sum, sumsq} of ``X``, ``PReLU1(T1)``, ``PReLU(E2)``, ``Y`` and
    ``running`` = the updated (mean, var) of ``bn1 bn2 bn_excit``."""
    o = {"stats": {}, "bn": {}, "running": {}}
    X = _d(x)
    mk = _d(mask)
    o["X"], o["stats"]["X"] = X, chan_stats(X)
    if m.bn1 is not None:
        R, o["bn"]["bn1"], o["running"]["bn1"] = _bn_forward(m.bn1, X, train)
    else:
        R = X
    o["R"] = R
    T1 = _layer(m.conv1, R)
    A1 = prelu(T1, _d(m.relu1.weight))
    N1, o["bn"]["bn2"], o["running"]["bn2"] = _bn_forward(m.bn2, A1, train)
    T2 = _layer(m.conv2, N1)
    Sh = _layer(m.conv_short, R) if m.conv_short is not None else None
    Rm = R * mk if mk is not None else R
    E1 = _layer(m.fc1, Rm)
    P1 = prelu(E1, _d(m.relu_excit_1.weight))
    E2 = _layer(m.fc2, P1)
    AE2 = prelu(E2, _d(m.relu_excit_2.weight))
    if m.conv_excit is not None:
        NE, o["bn"]["bn_excit"], o["running"]["bn_excit"] = _bn_forward(m.bn_excit, AE2, train)
        E3 = _layer(m.conv_excit, NE)
        ex = prelu(E3, _d(m.relu_excit_3.weight))
    else:
        NE, E3, ex = None, None, AE2
    sh = prelu(Sh, _d(m.relu_short.weight)) if Sh is not None else R
    Y = prelu(T2, _d(m.relu2.weight)) + sh + ex
    o.update(T1=T1, A1=A1, N1=N1, T2=T2, Sh=Sh, Rm=Rm, E1=E1, P1=P1, E2=E2, AE2=AE2, NE=NE, E3=E3, Y=Y)
    o["stats"].update(T1=chan_stats(A1), E2=chan_stats(AE2), Y=chan_stats(Y))
    return o


def backward(m, f, g, mask=None, gy_bn=False, sides=None):
    """Backward of a train-mode ``forward`` result ``f`` for the upstream gradient ``g``: the gradient of the loss
    with respect to ``Y``, or -- ``gy_bn`` -- with respect to ``BatchNorm(Y)`` (the next block's ``bn1``, batch
    statistics).  Returns ``dY dT2 dSh dEx dBn2 dBnE dT1 dE2 dE1 dR dX``, the gradients at the PReLU outputs ``dA1 dAE2
    dP1``, ``pairs`` = {sum g, sum g*y} of the upstream gradient, ``dBn2``, ``dBnE`` and ``dR``, and ``params`` = gradient of every parameter by ``named_parameters`` key."""
    sides = sides or {}
    side = lambda name: _d(sides.get(name))
    G, mk = _d(g), _d(mask)
    o = {"pairs": {}, "params": {}}
    P = o["params"]
    if gy_bn:
        mean = f["Y"].mean((0, 2))
        rstd = 1.0 / torch.sqrt(((f["Y"] - mean.view(1, -1, 1)) ** 2).mean((0, 2)) + 1e-5)
        dY, o["pairs"]["gy"] = _bn_backward(G, (f["Y"] - mean.view(1, -1, 1)) * rstd.view(1, -1, 1), rstd)
    else:
        dY = G
    o["dY"] = dY
    dT2, P["relu2.weight"] = _prelu_backward(dY, f["T2"], _d(m.relu2.weight), side("T2"))
    if m.conv_short is not None:
        dSh, P["relu_short.weight"] = _prelu_backward(dY, f["Sh"], _d(m.relu_short.weight), side("Sh"))
    else:
        dSh = dY
    if m.conv_excit is not None:
        dEx, P["relu_excit_3.weight"] = _prelu_backward(dY, f["E3"], _d(m.relu_excit_3.weight), side("E3"))
    else:
        dEx, P["relu_excit_2.weight"] = _prelu_backward(dY, f["E2"], _d(m.relu_excit_2.weight), side("E2"))
    dBn2, P["conv2.weight"], P["conv2.bias"] = _layer_vjp(m.conv2, f["N1"], dT2)
    dA1, o["pairs"]["dBn2"] = _bn_backward(dBn2, f["N1"], f["bn"]["bn2"][1])
    dT1, P["relu1.weight"] = _prelu_backward(dA1, f["T1"], _d(m.relu1.weight), side("T1"))
    if m.conv_excit is not None:
        dBnE, P["conv_excit.weight"], P["conv_excit.bias"] = _layer_vjp(m.conv_excit, f["NE"], dEx)
        dAE2, o["pairs"]["dBnE"] = _bn_backward(dBnE, f["NE"], f["bn"]["bn_excit"][1])
        dE2, P["relu_excit_2.weight"] = _prelu_backward(dAE2, f["E2"], _d(m.relu_excit_2.weight), side("E2"))
    else:
        dBnE, dE2 = None, dEx
    dP1, P["fc2.weight"], P["fc2.bias"] = _layer_vjp(m.fc2, f["P1"], dE2)
    dE1, P["relu_excit_1.weight"] = _prelu_backward(dP1, f["E1"], _d(m.relu_excit_1.weight), side("E1"))
    dRm, P["fc1.weight"], P["fc1.bias"] = _layer_vjp(m.fc1, f["Rm"], dE1)
    dR = dRm * mk if mk is not None else dRm
    d1, P["conv1.weight"], P["conv1.bias"] = _layer_vjp(m.conv1, f["R"], dT1)
    dR = dR + d1
    if m.conv_short is not None:
        ds, P["conv_short.weight"], P["conv_short.bias"] = _layer_vjp(m.conv_short, f["R"], dSh)
        dR = dR + ds
    else:
        dR = dR + dSh
    if m.bn1 is not None:
        dX, o["pairs"]["dR"] = _bn_backward(dR, f["R"], f["bn"]["bn1"][1])
    else:
        dX = dR
    o.update(dT2=dT2, dSh=dSh, dEx=dEx, dBn2=dBn2, dBnE=dBnE, dT1=dT1, dE2=dE2, dE1=dE1, dR=dR, dX=dX)
    # gradients with respect to the PReLU outputs (what the slope gradients are sums of)
    o.update(dA1=dA1, dAE2=dAE2 if m.conv_excit is not None else dY, dP1=dP1)
    return o


class MaskMul(nn.Module):
    """``dropout_1`` with its multipliers spelled out."""

    def __init__(self, mask):
        super().__init__()
        self.mask = mask

    def forward(self, x):
        return x * self.mask


def module_autograd(m, x, g, mask=None, gy_bn=False, dtype=torch.float64):
    """The project's own module in ``dtype`` with ``dropout_1`` replaced by the mask multiply, train mode, through torch
    autograd.  Returns (Y, dR, dX, parameter gradients by name); the module itself is left untouched."""
    import copy
    mm = copy.deepcopy(m).to(dtype).train()
    if mm.dropout_1 is not None:
        mm.dropout_1 = MaskMul(mask.detach().to(dtype)) if mask is not None else nn.Identity()
    xx = x.detach().to(dtype).clone().requires_grad_(True)
    kept = {}
    if mm.bn1 is not None:
        def keep(_mod, _inp, out):
            out.retain_grad()
            kept["R"] = out
        mm.bn1.register_forward_hook(keep)
    y = mm(xx)
    out = F.batch_norm(y, None, None, training=True, eps=1e-5) if gy_bn else y
    (out * g.detach().to(dtype)).sum().backward()
    dR = kept["R"].grad if "R" in kept else xx.grad
    return y.detach(), dR, xx.grad, {k: p.grad for k, p in mm.named_parameters()}


# the seven block shapes the fused kernels are specialised for (csrc/raae_block_shapes.inc, in its order) and the
# shapes only the generic instance takes: name -> (constructor name, args, kwargs, Lin)
TABLE_SHAPES = {
    "enc0": ("EncodingBlock", (1, 4, 256, 64), dict(kernel_size=11, stride=2, excitation=4), 256),
    "enc1": ("EncodingBlock", (4, 4, 64, 16), dict(kernel_size=7, stride=2, excitation=2), 64),
    "enc2": ("EncodingBlock", (4, 4, 16, 8), dict(kernel_size=5, stride=2, excitation=1), 16),
    "dec0": ("DecodingBlock", (6, 8, 1), dict(excitation=1, out_len=8), 1),
    "dec1": ("DecodingBlock", (8, 4, 8), dict(excitation=2, out_len=64), 8),
    "dec2": ("DecodingBlock", (4, 4, 64), dict(excitation=4), 64),
    "dec3": ("EncodingBlock", (4, 4, 256, 256), dict(kernel_size=11, stride=1, excitation=2), 256),
}
GENERIC_SHAPES = {
    "gen_a": ("DecodingBlock", (5, 8, 1), dict(excitation=1, out_len=8), 1),                  # the nstyle: 5 shape
    "gen_b": ("EncodingBlock", (4, 4, 48, 12), dict(kernel_size=7, stride=2, excitation=3), 48),   # no power of two
    "gen_c": ("DecodingBlock", (3, 6, 6), dict(excitation=3, out_len=24), 6),       # grouped shortcut + conv_excit
    "gen_d": ("EncodingBlock", (4, 4, 40, 40), dict(kernel_size=5, stride=1, excitation=2), 40),   # identity shortcut
    "gen_e": ("DecodingBlock", (4, 4, 35), dict(excitation=2, out_len=70), 35),     # Lout = 70: not a multiple of 4
}
SHAPES = dict(TABLE_SHAPES, **GENERIC_SHAPES)


def make_block(name, seed=0):
    """Block ``name`` of ``SHAPES`` -- or an ad-hoc shape given as its (constructor name, args, kwargs or their sorted
    items, Lin) tuple -- with every parameter and running buffer drawn away from its initial value (PReLU slopes of
    both signs, non-trivial running statistics).  Returns (module in fp32, Lin)."""
    from rankaae_amd import model
    cls, args, kw, Lin = SHAPES[name] if isinstance(name, str) else name
    kw = dict(kw)
    g = torch.Generator().manual_seed(1000 + seed)
    with torch.random.fork_rng():
        torch.manual_seed(seed)
        m = getattr(model, cls)(*args, **kw)
    with torch.no_grad():
        for k, p in m.named_parameters():
            if isinstance(m.get_submodule(k.rsplit(".", 1)[0]), nn.PReLU):
                p.copy_(torch.rand(p.shape, generator=g) * 0.5 - 0.1)
            elif k.endswith("bias"):
                p.copy_(torch.randn(p.shape, generator=g) * 0.2)
        for k, b in m.named_buffers():
            if k.endswith("running_mean"):
                b.copy_(torch.randn(b.shape, generator=g) * 0.3)
            elif k.endswith("running_var"):
                b.copy_(torch.rand(b.shape, generator=g) + 0.5)
    return m, Lin


def make_inputs(m, Lin, rows, seed=0):
    """(x, dropout-scale mask or None, upstream gradient) in fp32 for ``rows`` samples."""
    g = torch.Generator().manual_seed(77 + seed + rows)
    ci, co = m.conv1.in_channels, m.conv1.out_channels
    x = torch.randn(rows, ci, Lin, generator=g) * 1.3 + 0.2
    mask = None
    if m.dropout_1 is not None:
        keep = 1.0 - m.dropout_1.p
        mask = (torch.rand(rows, ci, Lin, generator=g) < keep).float() / keep
    gy = torch.randn(rows, co, m.fc2.out_features, generator=g)
    return x, mask, gy
