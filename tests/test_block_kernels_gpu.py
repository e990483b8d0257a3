"""The five fused residual-block kernels (``raae_block_fwd_a``, ``raae_block_fwd_b``, ``raae_block_bwd_b``,
``raae_block_bwd_a``, ``raae_block_wgrad``; ``csrc/raae_block_fused.inc`` and the dispatch in ``csrc/raae_conv.hip``)
against the float64 reference of ``block_reference``, one kernel at a time.

The entry points are driven directly through ``ops.block_*_args`` with ``nets_conv.Block(m, Lin)`` and a small
workspace object that carries the attributes ``CompactNet.alloc`` sets; no ``StepEngine`` is involved.

* TEACHER-FORCED: every kernel receives the reference's tensors (rounded to fp32) as its stored inputs and float64
  partial rows as its input statistics, so kernel and reference read the same pre-activations, no PReLU branch can
  differ and no entry is excused.  Every stored or emitted tensor is compared; the returned row / slab counts lie in
  1..RAAE_MAX_PARTS, rows beyond them are untouched, a second identical launch is bitwise equal.
* CHAINED: fwd_a -> fwd_b -> bwd_b -> bwd_a -> wgrad on the kernels' own outputs against the reference of the same
  block.  In backward the reference takes the kernel's PReLU side only where its own pre-activation lies within 1e-5
  of that tensor's largest magnitude (the band of ``test_disc_fused_matches_autograd``); a sign disagreement
  outside the band fails, the number of entries inside is printed.
* THE PAIR TABLE (``co_pair`` of csrc/raae_conv.hip, behind every two-body launch): which pairs are one launch at
  which row counts, as the library answers (``raae_co_instance``) and as the recorder counts the launches.
* SELF-CONSISTENCY, bit for bit: ``raae_block_fwd_a2`` / ``_b2`` against the two single calls, and
  ``raae_block_bwd_b_wgrad`` against ``raae_block_bwd_b`` followed by ``raae_block_wgrad``.  The ``_m``
  (trial-batched) forms stay with the trial-batch suites (``test_trial_batch_large_gpu.py`` and the trial-mode tests
  of ``test_engine_gpu.py``), which already hold them bitwise to the single launches pinned here.

Code paths reached by name: generic instance small and ``BIG`` (``gen_*`` at 37 and 1027 rows), the division
fallback of ``split`` (``gen_b``, ``gen_c``, ``gen_d``, ``gen_e``: no power-of-two length or width), the scalar
fallback of the ``BIG`` 16-byte paths (``gen_e``: Lout = 70; ``test_unaligned_big``: tensors 4 bytes into their
allocation) and the grid-capped group loop (``dec3`` at 4099 rows: 513 sample groups on 512 workgroups).

Which of the 16 instances per kernel run here: all eight plain ones (seven table shapes + generic), and the ``BIG``
ones the dispatch selects from 1024 rows (``kBigMask`` of csrc/raae_conv.hip): ``enc0``, ``dec2``, ``dec3`` and
generic in every family, ``dec1`` too in ``bwd_a`` and ``wgrad``.  For the other table shapes the 1027- and
4099-row cases run the PLAIN instance, as the package does; their compiled ``BIG`` instances (``enc1``, ``enc2``,
``dec0`` everywhere, ``dec1`` in ``fwd_a`` / ``fwd_b`` / ``bwd_b``) are reachable only through the
``RAAE_BIG_MASK_*`` tuning overrides, which are read once when the library loads: ``test_tuning_overrides_gpu.py`` runs
the runners of this module on them (and on the plain instances at 1027 rows, and under the other tuning overrides) in
child processes that load the library with the overrides set.

Tolerances are those ``test_conv_family_fwd_bwd`` applies to the same quantities of the per-layer kernels: forward
tensors 2e-5 relative + 2e-5; data gradients 5e-4 + 5e-5; weight, bias and slope gradients 5e-4 +
5e-5 * mean|G| * sqrt(B * L), G and L those of the parameter's own layer (``Rig.tol_param``); forward statistic
sums 1e-5 and backward partial sums 1e-4 relative, both +
max(1e-3, 5e-5 * sqrt(B * L)); running statistics 1e-4 + 1e-6.  From 1024 rows the parameter gradients (long
cancelling sums) may instead lie within 3x the distance of fp32 CPU autograd of the module (same inputs) from the
float64 reference, plus the same absolute floor -- the arbiter rule of ``test_p2_teacher_forced_steps``.
"""
import copy
import ctypes as C
import functools
import os
import types

import numpy as np
import pytest
import torch

import block_reference as br

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from rankaae_amd import ops, _lib, nets_conv
    DEV = torch.device("cuda:0")

MAXP = 512                     # RAAE_MAX_PARTS
SENT = -777.25                 # what a row no kernel may touch holds
BIG_ROWS = 1024                # RAAE_BIG_ROWS
RAW = ("T1", "T2", "Sh", "E1", "E2", "E3")
ROWS = (2, 37, 256, 1027, 4099)


# ---------------------------------------------------------------------------------------------- reference (cached)
@functools.lru_cache(maxsize=4)
def _reference(name, rows, gy_bn, masked, seed=0):
    m, Lin = br.make_block(name, seed)
    x, mask, g = br.make_inputs(m, Lin, rows, seed)
    if not masked:
        mask = None
    f = br.forward(m, x, mask, train=True)
    b = br.backward(m, f, g, mask, gy_bn=gy_bn)
    g32 = None
    if rows >= BIG_ROWS:
        g32 = br.module_autograd(m, x, g, mask, gy_bn=gy_bn, dtype=torch.float32)[3]
    return m, Lin, x, mask, g, f, b, g32


def _inputs(name, rows, masked, seed=0):
    """The same block and inputs without the reference's forward and backward (tests that compare launches only)."""
    m, Lin = br.make_block(name, seed)
    x, mask, g = br.make_inputs(m, Lin, rows, seed)
    return m, Lin, x, mask if masked else None, g, None, None, None


# ---------------------------------------------------------------------------------------------- comparisons
class Report:
    """Collects every comparison of a case: prints the largest error per quantity, asserts at the end."""

    def __init__(self, case):
        self.case, self.bad = case, []

    def close(self, what, got, want, rtol, atol, arbiter=None):
        got = got.detach().double().cpu()
        want = want.detach().double().cpu()
        assert got.shape == want.shape, (self.case, what, got.shape, want.shape)
        err = (got - want).abs()
        tol = atol + rtol * want.abs()
        finite = bool(torch.isfinite(got).all())
        worst = float(err.max()) if finite else float("inf")
        ratio = float((err / tol).max()) if finite else float("inf")
        note = ""
        ok = finite and bool((err <= tol).all())
        if not ok and finite and arbiter is not None:
            e_ref = float((arbiter.detach().double().cpu() - want).abs().max())
            ok = worst <= 3.0 * e_ref + atol
            note = f"  arbiter: fp32 autograd is {e_ref:.3e} from float64 -> {'ok' if ok else 'FAIL'}"
        print(f"ERR {self.case} {what}: max err {worst:.3e} (max |ref| {float(want.abs().max()):.3e}), "
              f"{ratio:.3f} of the bound{note}")
        if not ok:
            i = int(torch.nan_to_num(err / tol, nan=float("inf")).argmax())
            self.bad.append(f"{what}: max err {worst:.3e} = {ratio:.2f} x bound at flat index {i}: "
                            f"ref {float(want.flatten()[i]):.6e} got {float(got.flatten()[i]):.6e}{note}")

    def check(self, cond, what):
        if not cond:
            self.bad.append(what)

    def done(self):
        assert not self.bad, f"{self.case}:\n" + "\n".join(self.bad)


def _alloc(shape, off, fill=float("nan")):
    """fp32 device tensor that starts ``off`` floats into its (16-byte aligned) allocation."""
    n = int(np.prod(shape))
    return torch.full((n + 4,), fill, device=DEV)[off:off + n].view(*shape)


def _put(t, off):
    out = _alloc(tuple(t.shape), off)
    out.copy_(t.to(torch.float32))
    return out


def _rows(cols):
    """Two float64 partial rows (first / second half of the batch, like ``_partials_of`` of test_ops_gpu.py) from
    per-sample column sums ``cols`` = list of [B, C] tensors -> (buffer [MAXP, C, len(cols)], 2)."""
    B, C = cols[0].shape
    h = max(B // 2, 1)
    P = torch.full((MAXP, C, 2), SENT, dtype=torch.float64)
    for i, sl in enumerate((slice(0, h), slice(h, B))):
        for j, c in enumerate(cols):
            P[i, :, j] = c[sl].sum(0)
    return P.to(DEV), 2


def _stat_rows(a):
    a = a.double()
    return _rows([a.sum(2), (a * a).sum(2)])


def _pair_rows(g, y):
    g, y = g.double(), y.double()
    return _rows([g.sum(2), (g * y).sum(2)])


def _r(t):
    """A reference tensor as the kernels store it: rounded to fp32."""
    return t.float().double()


# ---------------------------------------------------------------------------------------------- the rig
class Rig:
    """One block on the device: module, static description, workspace, gradient slabs and the five launches."""

    def __init__(self, name, rows, gy_bn=False, need_dx=True, masked=True, off=0, seed=0, reference=True):
        self.name, self.B, self.gy_bn, self.need_dx, self.off = name, rows, gy_bn, need_dx, off
        (self.m, self.Lin, self.x, self.mask, self.g, self.f, self.b, self.g32) = (
            _reference(name, rows, gy_bn, masked, seed) if reference else _inputs(name, rows, masked, seed))
        self.md = copy.deepcopy(self.m).to(DEV)
        self.k = k = nets_conv.Block(self.md, self.Lin)
        self.excit, self.short, self.bn1 = k.cve is not None, k.cvs is not None, self.md.bn1 is not None
        self.offs, o = {}, 0
        for key, p in self.md.named_parameters():
            self.offs[key] = (o, p.numel(), tuple(p.shape))
            self.offs[id(p)] = self.offs[key]
            o += (p.numel() + 63) // 64 * 64
        self.stride = o
        self.slabs = torch.full((MAXP, o), SENT, device=DEV)
        self.nslab = {}
        B = rows
        w = self.w = types.SimpleNamespace(b=B)
        t = lambda *s: _alloc(s, off)
        parts = lambda C: torch.full((MAXP, C, 2), SENT, dtype=torch.float64, device=DEV)
        w.X, w.pX, w.nX = _put(self.x, off), None, 0
        w.maskd = _put(self.mask, off) if self.mask is not None else None
        w.G = _put(self.g, off)
        w.T1, w.T2 = t(B, k.Cout, k.L1), t(B, k.Cout, k.Lout)
        w.Sh = t(B, k.Cout, k.Lout) if self.short else None
        w.E1, w.E2 = t(B, k.Cin, k.E), t(B, k.Cin, k.Lout)
        w.E3 = t(B, k.Cout, k.Lout) if self.excit else None
        w.Y = t(B, k.Cout, k.Lout)
        w.pT1, w.pE2, w.pY = parts(k.Cout), parts(k.Cin), parts(k.Cout)
        w.nT1 = w.nE2 = w.nY = 0
        w.dBn2, w.pdBn2 = t(B, k.Cout, k.L1), parts(k.Cout)
        w.dR, w.pdR = t(B, k.Cin, k.Lin), parts(k.Cin)
        w.dBnE, w.pdBnE = t(B, k.Cin, k.Lout), parts(k.Cin)
        w.dT2, w.dSh, w.dEx = t(B, k.Cout, k.Lout), t(B, k.Cout, k.Lout), t(B, k.Cout, k.Lout)
        w.dT1, w.dE2, w.dE1 = t(B, k.Cout, k.L1), t(B, k.Cin, k.Lout), t(B, k.Cin, k.E)
        w.pG, w.nG, w.nB = None, 0, 0
        if self.bn1:
            w.pX, w.nX = _stat_rows(self.x)

    # ---- argument pieces
    def gslab(self, p):
        o, n, _ = self.offs[id(p)]
        return self.slabs[0, o:o + n]

    def _bn(self, bn, partials, nparts, count, train=True, update=False):
        if train:
            return ops.make_bn(partials, nparts, count, bn.running_mean, bn.running_var, bn.momentum, bn.eps, update)
        return ops.make_bn(None, 0, 0, bn.running_mean, bn.running_var, bn.momentum, bn.eps, False)

    def vR(self, train=True, update=False, mask=None):
        w, k = self.w, self.k
        bn = self._bn(self.md.bn1, w.pX, w.nX, self.B * k.Lin, train, update) if self.bn1 else None
        return ops.make_view(w.X, None, bn, mask)

    def v1(self, train=True, update=False):
        w, k, m = self.w, self.k, self.md
        return ops.make_view(w.T1, m.relu1.weight, self._bn(m.bn2, w.pT1, w.nT1, self.B * k.L1, train, update))

    def ve2(self, train=True, update=False):
        w, k, m = self.w, self.k, self.md
        if not self.excit:
            return ops.make_view(w.E2, m.relu_excit_2.weight)
        return ops.make_view(w.E2, m.relu_excit_2.weight,
                             self._bn(m.bn_excit, w.pE2, w.nE2, self.B * k.Lout, train, update))

    # ---- argument blocks (what nets_conv.CompactNet builds)
    def args_fwd_a(self, train=True, update=False):
        w, k, m = self.w, self.k, self.md
        return ops.block_fwd_a_args(self.vR(train, update), w.maskd if train else None, self.B, k, m, w.T1, w.Sh, w.E1,
                                    w.E2, w.pT1, w.pE2 if self.excit else None)

    def args_fwd_b(self, train=True, update=False):
        w, k, m = self.w, self.k, self.md
        return ops.block_fwd_b_args(self.v1(train, update), self.ve2(train, update),
                                    self.vR(train) if not self.short else None, self.B, k, m, w.Sh, w.T2, w.E3, w.Y, w.pY)

    def args_bwd_b(self, wgrad=None):
        w, k, m = self.w, self.k, self.md
        if self.gy_bn:
            ybn = ops.make_bn(w.pY, w.nY, self.B * k.Lout, None, None, 0.1, 1e-5, False)
            gy = ops.make_grad(w.G, bn=ybn, g_partials=w.pG, g_nparts=w.nG, u=w.Y)
        else:
            gy = ops.make_grad(w.G)
        return ops.block_bwd_b_args(gy, self.v1(), self.ve2() if self.excit else None, self.B, k, m, w, self.stride,
                                    self.gslab, wgrad=wgrad)

    def args_bwd_a(self):
        w, k, m = self.w, self.k, self.md
        bn2v = self._bn(m.bn2, w.pT1, w.nT1, self.B * k.L1)
        g1 = ops.make_grad(w.dBn2, raw=w.T1, slope=m.relu1.weight, bn=bn2v, g_partials=w.pdBn2, g_nparts=w.nB)
        ge = None
        if self.excit:
            bne = self._bn(m.bn_excit, w.pE2, w.nE2, self.B * k.Lout)
            ge = ops.make_grad(w.dBnE, raw=w.E2, slope=m.relu_excit_2.weight, bn=bne, g_partials=w.pdBnE, g_nparts=w.nB)
        dE2 = w.dE2 if self.excit else w.dEx
        return ops.block_bwd_a_args(g1, ge, self.vR(), w.maskd, self.B, k, m, w, dE2, w.dR if self.need_dx else None,
                                    w.pdR if (self.need_dx and self.bn1) else None, self.stride, self.gslab)

    def wgrad_tasks(self):
        w, k, m = self.w, self.k, self.md
        convs = [(ops.make_grad(w.dT2), k.cv2, self.v1(), m.conv2), (ops.make_grad(w.dT1), k.cv1, self.vR(), m.conv1)]
        if self.excit:
            convs.append((ops.make_grad(w.dEx), k.cve, self.ve2(), m.conv_excit))
        if self.short:
            convs.append((ops.make_grad(w.dSh), k.cvs, self.vR(), m.conv_short))
        dE2 = w.dE2 if self.excit else w.dEx
        lins = [(ops.make_grad(dE2), k.Cin, k.Lout, k.E, ops.make_view(w.E1, m.relu_excit_1.weight), m.fc2),
                (ops.make_grad(w.dE1), k.Cin, k.E, k.Lin, self.vR(mask=w.maskd), m.fc1)]
        return convs, lins

    def args_wgrad(self):
        convs, lins = self.wgrad_tasks()
        G = self.gslab
        a = ops.block_wgrad_args(self.B, [(g_, cv_, v_, G(mod.weight), G(mod.bias)) for g_, cv_, v_, mod in convs],
                                 [(g_, c_, e_, l_, v_, G(mod.weight), G(mod.bias)) for g_, c_, e_, l_, v_, mod in lins],
                                 self.stride)
        a.keep = (convs, lins)
        a.mods = [t[-1] for t in convs] + [t[-1] for t in lins]
        return a

    # ---- launches; each records the counts the next one needs
    def fwd_a(self, **kw):
        n = ops.block_fwd_a(self.args_fwd_a(**kw))
        self.w.nT1 = self.w.nE2 = n
        return n

    def fwd_b(self, **kw):
        self.w.nY = ops.block_fwd_b(self.args_fwd_b(**kw))
        return self.w.nY

    def bwd_b(self):
        self.w.nB = ops.block_bwd_b_launch(self.args_bwd_b())
        for name in ["relu2"] + (["relu_short"] if self.short else []) + ["relu_excit_3" if self.excit else "relu_excit_2"]:
            self.nslab[name + ".weight"] = self.w.nB
        return self.w.nB

    def bwd_a(self):
        n = ops.block_bwd_a_launch(self.args_bwd_a())
        for name in ["relu1", "relu_excit_1"] + (["relu_excit_2"] if self.excit else []):
            self.nslab[name + ".weight"] = n
        return n

    def note_wgrad(self, a, ns):
        names = {id(mod): key for key, mod in self.md.named_modules()}
        for mod, n in zip(a.mods, ns):
            self.nslab[names[id(mod)] + ".weight"] = self.nslab[names[id(mod)] + ".bias"] = n

    def wgrad(self):
        a = self.args_wgrad()
        ns = ops.block_wgrad(self.B, None, None, self.stride, args=a)
        self.note_wgrad(a, ns)
        return ns

    # ---- reading results
    def grad_of(self, key):
        """Parameter gradient ``key``: its slabs summed in float64; the rows beyond the slab count must be untouched."""
        o, n, shape = self.offs[key]
        ns = self.nslab[key]
        assert 1 <= ns <= MAXP, (key, ns)
        assert bool((self.slabs[ns:, o:o + n] == SENT).all()), f"{key}: slabs beyond the returned count {ns} were written"
        return self.slabs[:ns, o:o + n].double().sum(0).view(shape)

    def part_sum(self, buf, n, what):
        assert 1 <= n <= MAXP, (what, n)
        assert bool((buf[n:] == SENT).all()), f"{what}: partial rows beyond the returned count {n} were written"
        return buf[:n].sum(0)

    def snapshot(self, names):
        return {n: getattr(self.w, n).clone() for n in names if getattr(self.w, n) is not None}

    # ---- teacher forcing: the reference's tensors as the stored inputs of the next kernel
    def force(self, *names):
        f, b, w = self.f, self.b, self.w
        for n in names:
            src = f[n] if n in f else b[n]
            getattr(w, n).copy_(src.float())

    def force_stats(self, *names):
        f, b, w, m = self.f, self.b, self.w, self.m
        for n in names:
            if n == "T1":
                w.pT1, w.nT1 = _stat_rows(br.prelu(_r(f["T1"]), m.relu1.weight.detach().double()))
            elif n == "E2":
                w.pE2, w.nE2 = _stat_rows(br.prelu(_r(f["E2"]), m.relu_excit_2.weight.detach().double()))
            elif n == "Y":
                w.pY, w.nY = _stat_rows(_r(f["Y"]))
            elif n == "G":
                Y = _r(f["Y"])
                mean = Y.mean((0, 2), keepdim=True)
                yhat = (Y - mean) / torch.sqrt(((Y - mean) ** 2).mean((0, 2), keepdim=True) + 1e-5)
                w.pG, w.nG = _pair_rows(self.g, yhat)
            elif n == "dBn2":
                w.pdBn2, w.nB = _pair_rows(_r(b["dBn2"]), f["N1"])
            elif n == "dBnE":
                w.pdBnE, _ = _pair_rows(_r(b["dBnE"]), f["NE"])

    # ---- tolerances
    def tol_param(self, key, b):
        """5e-5 * mean|G| * sqrt(B * L) with G and L of the layer whose parameter ``key`` is, as
        ``test_conv_family_fwd_bwd`` takes them: for a conv / fc the gradient at its output and that output's length,
        for a PReLU slope the gradient at the activation's output and its length (``b``: the reference's backward)."""
        k = self.k
        G, L = {"conv2": ("dT2", k.Lout), "conv1": ("dT1", k.L1), "conv_short": ("dSh", k.Lout),
                "conv_excit": ("dEx", k.Lout), "fc2": ("dE2", k.Lout), "fc1": ("dE1", k.E),
                "relu2": ("dY", k.Lout), "relu_short": ("dY", k.Lout), "relu_excit_3": ("dY", k.Lout),
                "relu_excit_2": ("dAE2", k.Lout), "relu1": ("dA1", k.L1), "relu_excit_1": ("dP1", k.E)}[key.split(".")[0]]
        return 5e-5 * float(b[G].abs().mean()) * (self.B * L) ** 0.5

    def tol_sum(self, L):
        return max(1e-3, 5e-5 * (self.B * L) ** 0.5)

def _case_id(name, rows, **kw):
    return f"{name}@{rows}" + "".join(f",{a}={b}" for a, b in kw.items() if b not in (False, 0, None))


# ---------------------------------------------------------------------------------------------- the three groups
def _check_fwd_a(r, rep, f, update):
    w, k, m = r.w, r.k, r.md
    for n in ("T1", "Sh", "E1", "E2"):
        if f[n] is not None:
            rep.close(n, getattr(w, n), f[n], 2e-5, 2e-5)
    tot = r.part_sum(w.pT1, w.nT1, "pT1")
    rep.close("stats PReLU1(T1)", tot, f["stats"]["T1"], 1e-5, r.tol_sum(k.L1))
    if r.excit:
        rep.close("stats PReLU(E2)", r.part_sum(w.pE2, w.nE2, "pE2"), f["stats"]["E2"], 1e-5, r.tol_sum(k.Lout))
    else:
        rep.check(bool((w.pE2 == SENT).all()), "pE2 written although the block has no bn_excit")
    if r.bn1:
        want = f["running"]["bn1"] if update else (r.m.bn1.running_mean, r.m.bn1.running_var)
        rep.close("bn1.running_mean", m.bn1.running_mean, want[0], 1e-4, 1e-6)
        rep.close("bn1.running_var", m.bn1.running_var, want[1], 1e-4, 1e-6)


def _check_fwd_b(r, rep, f, update):
    w, k, m = r.w, r.k, r.md
    for n in ("T2", "E3", "Y"):
        if f[n] is not None:
            rep.close(n, getattr(w, n), f[n], 2e-5, 2e-5)
    rep.close("stats Y", r.part_sum(w.pY, w.nY, "pY"), f["stats"]["Y"], 1e-5, r.tol_sum(k.Lout))
    for bn in ("bn2",) + (("bn_excit",) if r.excit else ()):
        want = f["running"][bn] if update else (getattr(r.m, bn).running_mean, getattr(r.m, bn).running_var)
        rep.close(bn + ".running_mean", getattr(m, bn).running_mean, want[0], 1e-4, 1e-6)
        rep.close(bn + ".running_var", getattr(m, bn).running_var, want[1], 1e-4, 1e-6)


def _param(r, rep, b, key):
    arb = r.g32[key] if r.g32 is not None else None
    rep.close("d " + key, r.grad_of(key), b["params"][key], 5e-4, r.tol_param(key, b), arbiter=arb)


def _check_bwd_b(r, rep, b):
    w, k = r.w, r.k
    for n in ("dT2", "dSh", "dEx", "dBn2") + (("dBnE",) if r.excit else ()):
        rep.close(n, getattr(w, n), b[n], 5e-4, 5e-5)
    rep.close("pairs dBn2", r.part_sum(w.pdBn2, w.nB, "pdBn2"), b["pairs"]["dBn2"], 1e-4, r.tol_sum(k.L1))
    if r.excit:
        rep.close("pairs dBnE", r.part_sum(w.pdBnE, w.nB, "pdBnE"), b["pairs"]["dBnE"], 1e-4, r.tol_sum(k.Lout))
    for key in ["relu2"] + (["relu_short"] if r.short else []) + ["relu_excit_3" if r.excit else "relu_excit_2"]:
        _param(r, rep, b, key + ".weight")


def _check_bwd_a(r, rep, b, n):
    w, k = r.w, r.k
    for name in ("dT1", "dE1") + (("dE2",) if r.excit else ()) + (("dR",) if r.need_dx else ()):
        rep.close(name, getattr(w, name), b[name], 5e-4, 5e-5)
    if not r.need_dx:
        rep.check(bool(torch.isnan(w.dR).all()), "dR written although no input gradient was asked for")
    if r.need_dx and r.bn1:
        rep.close("pairs dR", r.part_sum(w.pdR, n, "pdR"), b["pairs"]["dR"], 1e-4, r.tol_sum(k.Lin))
    else:
        rep.check(bool((w.pdR == SENT).all()), "pdR written although none was asked for")
    for key in ["relu1", "relu_excit_1"] + (["relu_excit_2"] if r.excit else []):
        _param(r, rep, b, key + ".weight")


def _check_wgrad(r, rep, b):
    for key in sorted(b["params"]):
        if key.startswith(("conv", "fc")):
            _param(r, rep, b, key)


def _twice(rep, what, launch, read):
    """A second identical launch is bitwise equal."""
    n1 = launch()
    first = read()
    n2 = launch()
    second = read()
    rep.check(n1 == n2, f"{what}: counts {n1} then {n2}")
    for key in first:
        rep.check(torch.equal(first[key], second[key]) or
                  bool(((first[key] == second[key]) | (torch.isnan(first[key]) & torch.isnan(second[key]))).all()),
                  f"{what}: {key} differs between two identical launches")
    return n1


def run_teacher_forced(name, rows, gy_bn=False, need_dx=True, masked=True, off=0, update=False, tile=0, slabs_out=None):
    """Returns the row count each of the four row-writing launches reported; ``slabs_out`` (a dict) receives the slab
    counts of the weight-gradient tasks under "wgrad", in task order."""
    r = Rig(name, rows, gy_bn=gy_bn, need_dx=need_dx, masked=masked, off=off)
    rep = Report("forced " + _case_id(name, rows, gy_bn=gy_bn, no_dx=not need_dx, nomask=not masked, off=off,
                                      update=update, tile=tile))
    w, f, b, md = r.w, r.f, r.b, r.md
    counts = {}

    def buffers(*names):
        return lambda: dict(r.snapshot(names), slabs=r.slabs.clone())

    # fwd_a: reads X (+ its float64 statistics), the mask
    # (running statistics move once per launch: the bitwise repeat runs with the update off)
    n = _twice(rep, "fwd_a", lambda: r.fwd_a(update=False), buffers("T1", "Sh", "E1", "E2", "pT1", "pE2"))
    if update:
        r.fwd_a(update=True)
    counts["fwd_a"] = n
    _check_fwd_a(r, rep, f, update)
    # fwd_b: reads T1, E2, Sh | X
    r.force("T1", "E2", *(("Sh",) if r.short else ()))
    r.force_stats("T1", *(("E2",) if r.excit else ()))
    n = _twice(rep, "fwd_b", lambda: r.fwd_b(update=False), buffers("T2", "E3", "Y", "pY"))
    if update:
        r.fwd_b(update=True)
    counts["fwd_b"] = n
    _check_fwd_b(r, rep, f, update)
    # bwd_b: reads the upstream gradient (+ Y behind a BatchNorm), T2, Sh, E3 | E2, T1, E2
    r.force("T2", "Y", *(("E3",) if r.excit else ()))
    if gy_bn:
        r.force_stats("Y", "G")
    n = _twice(rep, "bwd_b", r.bwd_b, buffers("dT2", "dSh", "dEx", "dBn2", "dBnE", "pdBn2", "pdBnE"))
    counts["bwd_b"] = n
    _check_bwd_b(r, rep, b)
    # bwd_a: reads dBn2, T1, dSh, dBnE + E2 | dE2, E1, the mask, X
    r.force("dBn2", "dSh", "E1", *(("dBnE",) if r.excit else ("dEx",)))
    r.force_stats("dBn2", *(("dBnE",) if r.excit else ()))
    n = _twice(rep, "bwd_a", r.bwd_a, buffers("dT1", "dE2", "dE1", "dR", "pdR"))
    counts["bwd_a"] = n
    _check_bwd_a(r, rep, b, n)
    # wgrad: reads the materialised gradients and the views they multiply
    r.force("dT2", "dT1", "dE1", "dEx", *(("dE2",) if r.excit else ()))
    ns = _twice(rep, "wgrad", lambda: tuple(r.wgrad()), lambda: dict(slabs=r.slabs.clone()))
    if slabs_out is not None:
        slabs_out["wgrad"] = tuple(ns)
    _check_wgrad(r, rep, b)
    rep.done()
    return counts


def run_chained(name, rows, gy_bn=False, need_dx=True, masked=True, off=0, tile=0):
    r = Rig(name, rows, gy_bn=gy_bn, need_dx=need_dx, masked=masked, off=off)
    rep = Report("chained " + _case_id(name, rows, gy_bn=gy_bn, no_dx=not need_dx, nomask=not masked, off=off,
                                       tile=tile))
    w, f, m = r.w, r.f, r.m
    r.fwd_a(update=True)
    _check_fwd_a(r, rep, f, True)
    r.fwd_b(update=True)
    _check_fwd_b(r, rep, f, True)
    # PReLU sides: the kernel's where the reference's own pre-activation is rounding noise around zero, and only there
    sides, inside = {}, 0
    for n in RAW:
        if f[n] is None:
            continue
        mine = getattr(w, n).double().cpu()
        band = f[n].abs() <= 1e-5 * float(f[n].abs().max())
        flip = (mine > 0) != (f[n] > 0)
        rep.check(not bool((flip & ~band).any()),
                  f"{n}: {int((flip & ~band).sum())} pre-activations outside the 1e-5 band on the other side of zero")
        inside += int(band.sum())
        sides[n] = torch.where(band, mine, f[n])
    print(f"ERR {rep.case} entries inside the 1e-5 PReLU band: {inside} "
          f"({sum(int(((getattr(w, n).double().cpu() > 0) != (f[n] > 0)).sum()) for n in RAW if f[n] is not None)} "
          f"of them on the other side)")
    b = br.backward(m, f, r.g, r.mask, gy_bn=gy_bn, sides=sides)
    if gy_bn:
        Y = w.Y.double().cpu()
        mean = Y.mean((0, 2), keepdim=True)
        yhat = (Y - mean) / torch.sqrt(((Y - mean) ** 2).mean((0, 2), keepdim=True) + 1e-5)
        w.pG, w.nG = _pair_rows(r.g, yhat)
    r.bwd_b()
    _check_bwd_b(r, rep, b)
    n = r.bwd_a()
    _check_bwd_a(r, rep, b, n)
    r.wgrad()
    _check_wgrad(r, rep, b)
    rep.done()


# (shape, rows, gy behind a BatchNorm of its own): the table shapes alternate by row parity, teacher-forced and chained
# the other way round, so that every table shape meets both forms in both groups; the generic shapes run at two odd
# row counts only, so they take both forms explicitly
FORCED_CASES = ([(n, rows, rows % 2 == 1) for n in br.TABLE_SHAPES for rows in ROWS] +
                [(n, rows, bn) for n in br.GENERIC_SHAPES for rows in (37, 1027) for bn in (True, False)])
CHAINED_CASES = [(n, rows, not bn if n in br.TABLE_SHAPES else bn) for n, rows, bn in FORCED_CASES]


@pytest.mark.parametrize("name,rows,gy_bn", FORCED_CASES)
def test_teacher_forced(name, rows, gy_bn):
    """Every kernel alone on the reference's tensors.  ``gy`` carries a BatchNorm of its own (an inner block) or none
    (a network's last block); the dropout mask is there wherever the block has ``dropout_1``; the input gradient and
    its sums are asked for wherever the block has ``bn1`` (``pdR`` = NULL with ``dR`` for ``enc0`` -- one input channel
    -- and ``dec0`` / ``gen_a`` -- length 1)."""
    run_teacher_forced(name, rows, gy_bn=gy_bn)


@pytest.mark.parametrize("name,rows,gy_bn", CHAINED_CASES)
def test_chained(name, rows, gy_bn):
    run_chained(name, rows, gy_bn=gy_bn)


def test_grid_cap_loops_over_groups():
    """``ngroups > RAAE_MAX_PARTS``: a workgroup walks several sample groups.  4099 rows of the 4 x 256 block are today
    513 groups of 8 samples (forward, backward phase B) and 1025 of 4 (backward phase A) on 512 workgroups.  That the
    loop runs is read off the returned count alone: a launch has ceil(B / S) groups of S samples (an integer) and
    returns min(groups, RAAE_MAX_PARTS) rows; no S gives ceil(4099 / S) = 512 (S = 8 gives 513, S = 9 gives 456), so
    a returned 512 means more than 512 groups, whatever group size the host picks.  A retuned host that no longer
    reaches the cap at this row count fails here instead of silently dropping the case."""
    assert all(-(-4099 // S) != MAXP for S in range(1, 4100))
    counts = run_teacher_forced("dec3", 4099, gy_bn=True)
    for kernel, n in counts.items():
        assert n == MAXP, (kernel, n)


def run_first_block(name, rows):
    run_teacher_forced(name, rows, need_dx=False)
    run_chained(name, rows, need_dx=False)


def run_running_statistics(name, rows):
    run_teacher_forced(name, rows, update=True)


@pytest.mark.parametrize("name,rows", [("enc1", 37), ("dec1", 1027), ("gen_d", 37), ("dec3", 256)])
def test_first_block_of_a_network(name, rows):
    """``dR`` = NULL: nothing upstream wants the input gradient; neither ``dR`` nor ``pdR`` is written."""
    run_first_block(name, rows)


@pytest.mark.parametrize("name,rows", [("enc1", 37), ("dec1", 256), ("dec2", 1027), ("gen_c", 37)])
def test_running_statistics_move_as_batchnorm1d(name, rows):
    """``update_running`` on: the buffers move as ``torch.nn.BatchNorm1d`` moves them (momentum 0.1, unbiased
    variance), once, by workgroup 0 only."""
    run_running_statistics(name, rows)


def run_eval_forward(name, rows):
    r = Rig(name, rows, masked=False)
    rep = Report("eval " + _case_id(name, rows))
    f = br.forward(r.m, r.x, None, train=False)
    before = {k: v.clone() for k, v in r.md.state_dict().items()}
    r.fwd_a(train=False)
    for n in ("T1", "Sh", "E1", "E2"):
        if f[n] is not None:
            rep.close(n, getattr(r.w, n), f[n], 2e-5, 2e-5)
    rep.close("stats PReLU1(T1)", r.part_sum(r.w.pT1, r.w.nT1, "pT1"), f["stats"]["T1"], 1e-5, r.tol_sum(r.k.L1))
    for n in ("T1", "E2") + (("Sh",) if r.short else ()):          # teacher-forced with the EVAL reference's tensors
        getattr(r.w, n).copy_(f[n].float())
    r.fwd_b(train=False)
    for n in ("T2", "E3", "Y"):
        if f[n] is not None:
            rep.close(n, getattr(r.w, n), f[n], 2e-5, 2e-5)
    rep.close("stats Y", r.part_sum(r.w.pY, r.w.nY, "pY"), f["stats"]["Y"], 1e-5, r.tol_sum(r.k.Lout))
    for k, v in r.md.state_dict().items():
        rep.check(torch.equal(v, before[k]), f"{k} changed in an eval-mode forward")
    rep.done()


@pytest.mark.parametrize("name,rows", [("enc1", 37), ("dec1", 37), ("dec3", 1027), ("gen_c", 1027), ("gen_d", 37)])
def test_eval_mode_forward(name, rows):
    """Eval mode: running statistics normalise, there is no mask, and the running buffers stay as they were."""
    run_eval_forward(name, rows)


@pytest.mark.parametrize("name,rows", [("enc0", 1027), ("dec2", 1027), ("dec3", 1027), ("dec3", 37), ("gen_d", 1027),
                                       ("gen_c", 1027)])
def test_unaligned_big(name, rows):
    """Activations, gradients and mask that start 4 bytes into their allocation: every 16-byte path must step aside
    for its scalar form.  The ``BIG`` instances test the alignment of what they move in quads inside the kernel.
    The strip paths of the 4 x 256 instance (``dec3``) move quads at EVERY row count and do not test: for them the
    host entry points look at the pointers and send an off-boundary launch to the generic instance (so ``dec3`` here
    is also the generic instance on a strip-capable convolution, halo 8 around a pad of 5)."""
    r = Rig(name, rows, off=1)
    assert r.w.T1.data_ptr() % 16 == 4 and r.w.X.data_ptr() % 16 == 4 and r.w.dR.data_ptr() % 16 == 4
    run_teacher_forced(name, rows, gy_bn=True, off=1)
    run_chained(name, rows, off=1)


@pytest.mark.parametrize("name,rows", [("enc1", 37), ("dec1", 37), ("gen_b", 37)])
def test_tile_hint(name, rows):
    """``raae_tile_hint(4)`` (a caller that batches four trials) sizes the sample groups for four times the rows."""
    ops.tile_hint(4)
    try:
        run_teacher_forced(name, rows, gy_bn=True, tile=4)
        run_chained(name, rows, tile=4)
    finally:
        ops.tile_hint(1)


# ---------------------------------------------------------------------------------------------- refusals
def _refused(launch, rig):
    before = {n: v.clone() for n, v in vars(rig.w).items() if torch.is_tensor(v)}
    with pytest.raises(_lib.HipCallError, match="error -1:"):       # RAAE_EINVAL
        launch()
    torch.cuda.synchronize()
    for n, v in before.items():
        now = getattr(rig.w, n)
        assert bool(((now == v) | (torch.isnan(now) & torch.isnan(v))).all()), f"{n} written by a refused call"
    assert bool((rig.slabs == SENT).all())


@pytest.mark.parametrize("what,cls,args,kw,Lin", [
    ("Cin = 9", "EncodingBlock", (9, 4, 16, 8), dict(kernel_size=5, stride=2, excitation=1), 16),
    ("weights over 4096 floats", "EncodingBlock", (4, 4, 256, 256), dict(kernel_size=11, stride=1, excitation=9), 256),
    ("tile over the LDS budget", "EncodingBlock", (8, 8, 1536, 1536), dict(kernel_size=7, stride=1, excitation=1), 1536),
])
def test_refusals_are_host_side(what, cls, args, kw, Lin):
    """Shapes the fused kernels cannot take return RAAE_EINVAL from the argument checks: nothing is launched, nothing
    is written.  (``CompactNet`` sends blocks of more than 8 channels down its per-layer path.)"""
    r = Rig((cls, args, tuple(sorted(kw.items())), Lin), 2)        # an ad-hoc shape, given as its tuple
    _refused(lambda: ops.block_fwd_a(r.args_fwd_a()), r)
    r.w.nT1 = r.w.nE2 = r.w.nB = 2
    for p in (r.w.pT1, r.w.pE2, r.w.pdBn2, r.w.pdBnE):
        p[:2] = 1.0
    r.w.pT1[:2, :, 1] = 4.0
    _refused(lambda: ops.block_bwd_a_launch(r.args_bwd_a()), r)
    if what != "weights over 4096 floats":       # (the phase B kernels stage no fc weights: they take that shape)
        _refused(lambda: ops.block_fwd_b(r.args_fwd_b()), r)
        _refused(lambda: ops.block_bwd_b_launch(r.args_bwd_b()), r)


# ---------------------------------------------------------------------------------------------- self-consistency
def _fwd_outputs(r):
    return r.snapshot(("T1", "Sh", "E1", "E2", "T2", "E3", "Y", "pT1", "pE2", "pY"))


def _same(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        assert bool(((a[k] == b[k]) | (torch.isnan(a[k]) & torch.isnan(b[k]))).all()), f"{what}: {k} differs"


@pytest.mark.parametrize("first,second,rows", [("enc0", "dec0", 37), ("enc1", "dec1", 256), ("enc1", "gen_c", 37),
                                               ("gen_b", "dec2", 37)])
def test_fwd_pair_is_bitwise_the_two_single_calls(first, second, rows):
    """``raae_block_fwd_a2`` / ``_b2`` (two independent blocks in one launch) on a table pair with an instance of
    its own and on pairs with a generic shape."""
    x, y = Rig(first, rows), Rig(second, rows + 3)
    for r in (x, y):
        r.fwd_a()
        r.fwd_b()
    alone = [_fwd_outputs(r) for r in (x, y)]
    nalone = [(r.w.nT1, r.w.nY) for r in (x, y)]
    x2, y2 = Rig(first, rows), Rig(second, rows + 3)
    n1, n2 = ops.block_fwd_pair("a", x2.args_fwd_a(), y2.args_fwd_a())
    x2.w.nT1 = x2.w.nE2 = n1
    y2.w.nT1 = y2.w.nE2 = n2
    m1, m2 = ops.block_fwd_pair("b", x2.args_fwd_b(), y2.args_fwd_b())
    assert [(n1, m1), (n2, m2)] == nalone
    _same(_fwd_outputs(x2), alone[0], first)
    _same(_fwd_outputs(y2), alone[1], second)


def _through_bwd_a(name, rows):
    r = Rig(name, rows)
    r.fwd_a()
    r.fwd_b()
    r.bwd_b()
    r.bwd_a()
    return r


@pytest.mark.parametrize("phase_b,tasks,rows", [("enc0", "enc1", 37), ("dec1", "dec2", 256), ("gen_c", "gen_b", 37),
                                                ("enc1", "gen_d", 37)])
def test_bwd_b_wgrad_is_bitwise_the_two_launches(phase_b, tasks, rows):
    """``raae_block_bwd_b_wgrad`` (phase B of one block beside the weight-gradient tasks of the block after it) on
    table pairs with an instance of their own and on pairs with a generic shape."""
    outs = ("dT2", "dSh", "dEx", "dBn2", "dBnE", "pdBn2", "pdBnE")
    res = []
    for fused in (False, True):
        nxt = _through_bwd_a(tasks, rows)            # the block whose weight gradients are pending
        r = Rig(phase_b, rows)
        r.fwd_a()
        r.fwd_b()
        wa = nxt.args_wgrad()
        if fused:
            a = r.args_bwd_b(wgrad=wa)
            nB, ns = ops.block_bwd_b_launch(a)
        else:
            nB = ops.block_bwd_b_launch(r.args_bwd_b())
            ns = ops.block_wgrad(nxt.B, None, None, nxt.stride, args=wa)
        res.append((nB, list(ns), dict(r.snapshot(outs), slabs=r.slabs.clone(), slabs_next=nxt.slabs.clone())))
    assert res[0][:2] == res[1][:2]
    _same(res[0][2], res[1][2], f"{phase_b} + {tasks}")


# ---------------------------------------------------------------------------------------------- the pair table
def _ready(name, rows):
    """A block whose argument blocks pass the host checks without a launch: two statistic rows everywhere."""
    r = Rig(name, rows, reference=False)
    r.w.nT1 = r.w.nE2 = r.w.nY = r.w.nB = 2
    return r


def _adam_item(max_nslab, chk, n=256):
    """What the engine yields for an Adam update that may ride (``StepEngine``: a launch with ``co_args``)."""
    z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device=DEV)
    keep = [z(n), z(n), z(n), z(max_nslab, n), torch.ones(n // 64, dtype=torch.int16, device=DEV),
            z(8, dt=torch.float64), z(1, dt=torch.int32), z(1, dt=torch.int32) if chk else None]
    p, m, v, g, seg, hyper, step, nan = keep
    return types.SimpleNamespace(co_args=ops.adam_part_args(p, m, v, g, n, seg, n, _lib.OPT_ADAM, hyper, step, max_nslab,
                                                            nan), keep=keep)


def _head_item(rows, C_=4, L=256):
    """The decoder's head on a [rows, C_, L] tensor behind a BatchNorm (``CompactNet.forward_steps``)."""
    X, P = torch.zeros(rows, C_, L, device=DEV), torch.zeros(MAXP, C_, 2, dtype=torch.float64, device=DEV)
    rm, rv = torch.zeros(C_, device=DEV), torch.ones(C_, device=DEV)
    w, b, out = torch.zeros(1, C_, 1, device=DEV), torch.zeros(1, device=DEV), torch.zeros(rows, 1, L, device=DEV)
    view = ops.make_view(X, None, ops.make_bn(P, 2, rows * L, rm, rv, 0.1, 1e-5, False))
    item = ops.conv_fwd_item(view, rows, ops.make_conv(C_, L, 1, L, 1, 1, 0, 0, 1, 0), w, b, out, 1)
    item.keep = (item.keep, X, P, rm, rv, w, b, out)
    return item


def _side(spec, rows, rigs):
    """(kind, argument block) as a generator of launches yields it, from a row of ``CO_TABLE``; ``rigs``: one block per
    shape name, shared by the rows (nothing is launched)."""
    kind, what = spec[0], spec[1:]
    if kind == "adam":
        return kind, _adam_item(*what)
    if kind == "head":
        return kind, _head_item(rows, *what)
    for name in what:
        if name not in rigs:
            rigs[name] = _ready(name, rows)
    r = rigs[what[0]]
    if kind == "bwd_b":
        a = r.args_bwd_b(wgrad=rigs[what[1]].args_wgrad())
    else:
        a = {"a": r.args_fwd_a, "b": r.args_fwd_b, "bwd_a": r.args_bwd_a, "wgrad": r.args_wgrad}[kind]()
    return kind, a


WIDE, NARROW = 40, 16          # max_nslab of an Adam update: above 16 the wide kernel, which has a body in co_kernel
# (x, y, one launch at 256 rows, one launch at 1027 rows) -- the answers of raae_co_instance, read off the build BEFORE
# the forward pairs and bwd_b + wgrad moved into the same table, not off the code under test.  The first 18 are the
# table's rows for the phase boundaries of the 256-row step; each applies where neither body would run a large-batch
# (BIG) instance alone, so four of them also hold at 1027 rows: bwd_a of enc1 / enc2 / dec0 and fwd_b of enc2 / dec0 run
# their plain instance at every row count (kBigMask), and an Adam update has no large-batch form.
CO_TABLE = [
    (("bwd_a", "dec3"), ("adam", WIDE, True), 1, 0),
    (("bwd_a", "dec3"), ("adam", WIDE, False), 1, 0),
    (("bwd_b", "dec2", "dec3"), ("a", "enc0"), 1, 0),
    (("bwd_a", "dec2"), ("b", "enc0"), 1, 0),
    (("bwd_b", "dec1", "dec2"), ("a", "enc1"), 1, 0),
    (("bwd_a", "dec1"), ("b", "enc1"), 1, 0),
    (("bwd_b", "dec0", "dec1"), ("a", "enc2"), 1, 0),
    (("bwd_a", "dec0"), ("b", "enc2"), 1, 1),
    (("bwd_a", "enc2"), ("adam", WIDE, True), 1, 1),
    (("bwd_a", "enc2"), ("adam", WIDE, False), 1, 1),
    (("bwd_b", "enc1", "enc2"), ("a", "dec0"), 1, 0),
    (("bwd_a", "enc1"), ("b", "dec0"), 1, 1),
    (("bwd_b", "enc0", "enc1"), ("a", "dec1"), 1, 0),
    (("bwd_a", "enc0"), ("b", "dec1"), 1, 0),
    (("wgrad", "enc0"), ("a", "dec2"), 1, 0),
    (("adam", WIDE, True), ("b", "dec2"), 1, 0),
    (("adam", WIDE, False), ("b", "dec2"), 1, 0),
    (("a", "enc1"), ("head", 4), 1, 0),
    # pairs without a row
    (("bwd_a", "enc1"), ("b", "dec1"), 0, 0),
    (("bwd_a", "dec3"), ("adam", NARROW, True), 0, 0),
    (("bwd_a", "dec2"), ("a", "enc0"), 0, 0),
    (("bwd_b", "dec2", "dec3"), ("a", "enc1"), 0, 0),
    (("bwd_b", "dec3", "dec2"), ("a", "enc0"), 0, 0),
    (("wgrad", "enc1"), ("a", "dec2"), 0, 0),
    (("a", "enc1"), ("head", 8), 0, 0),
    (("a", "enc0"), ("head", 4), 0, 0),
    (("bwd_a", "gen_d"), ("adam", WIDE, False), 0, 0),
    # the forward pairs' rows belong to raae_block_fwd_a2 / _b2 alone: raae_co_launch runs such a pair as two launches
    (("a", "enc0"), ("a", "dec3"), 0, 0),
    (("a", "enc1"), ("b", "dec1"), 0, 0),
]


@pytest.mark.parametrize("rows,col", [(256, 2), (1027, 3)])
def test_pair_table_answers(rows, col):
    """``ops.co_pairable`` (``raae_co_instance``) for every row of the cross-phase table and for pairs without one.
    The answers at 1027 rows are those of the default ``kBigMask``; the ``RAAE_BIG_MASK_*`` tuning overrides, read once
    when the library loads, would move them, so the test insists that none is set."""
    assert not [k for k in os.environ if k.startswith("RAAE_BIG_MASK_")], "RAAE_BIG_MASK_* overrides are set"
    got, rigs = [], {}
    for row in CO_TABLE:
        (kx, ax), (ky, ay) = _side(row[0], rows, rigs), _side(row[1], rows, rigs)
        got.append(int(ops.co_pairable(kx, ax, ky, ay)))
        print(f"PAIR {rows} rows: {row[0]} + {row[1]}: {got[-1]} (expected {row[col]})")
    assert got == [row[col] for row in CO_TABLE]


def _launches(fn):
    """How many launches ``fn()`` makes, read through the recorder (as ``TrialBatch`` uses it)."""
    lib = _lib.load()
    assert lib.raae_record_begin() == 0
    try:
        fn()
    finally:
        h, n = C.c_void_p(), C.c_int(0)
        rc = lib.raae_record_end(C.byref(h), C.byref(n))
    assert rc == 0
    lib.raae_record_free(h)
    torch.cuda.synchronize()
    return n.value


def _launched(name, rows, *launches):
    """A block without a reference (only launches are counted) after the named launches."""
    r = Rig(name, rows, reference=False)
    for step in launches:
        getattr(r, step)()
    return r


@pytest.mark.parametrize("first,second,rows,want", [("enc0", "dec0", 37, 1), ("enc0", "dec0", 1027, 1),
                                                    ("enc1", "gen_c", 37, 2)])
def test_fwd_pair_launch_counts(first, second, rows, want):
    """``raae_block_fwd_a2`` / ``_b2``: a pair with a row of the table is ONE launch at every row count (the row is not
    gated by the large-batch instances: it runs the plain bodies), a pair without one is two."""
    x, y = _launched(first, rows, "fwd_a"), _launched(second, rows, "fwd_a")
    na = _launches(lambda: ops.block_fwd_pair("a", x.args_fwd_a(), y.args_fwd_a()))
    nb = _launches(lambda: ops.block_fwd_pair("b", x.args_fwd_b(), y.args_fwd_b()))
    print(f"LAUNCHES fwd pair {first} + {second} at {rows} rows: a {na}, b {nb} (expected {want})")
    assert (na, nb) == (want, want)


@pytest.mark.parametrize("phase_b,tasks", [("enc0", "enc1"), ("gen_c", "gen_b")])
@pytest.mark.parametrize("rows", [37, 1027])
def test_bwd_b_wgrad_launch_counts(phase_b, tasks, rows):
    """``raae_block_bwd_b_wgrad`` is ONE launch for a table pair and for any other pair (the generic instance), below
    and above 1024 rows."""
    nxt = _launched(tasks, rows, "fwd_a", "fwd_b", "bwd_b", "bwd_a")
    r = _launched(phase_b, rows, "fwd_a", "fwd_b")
    a = r.args_bwd_b(wgrad=nxt.args_wgrad())
    n = _launches(lambda: ops.block_bwd_b_launch(a))
    print(f"LAUNCHES bwd_b {phase_b} + wgrad {tasks} at {rows} rows: {n} (expected 1)")
    assert n == 1


def test_co_launch_without_an_instance_is_two_launches():
    """``raae_co_launch`` of a pair the table has no row for: the two bodies' own launches, x first."""
    x, y = _launched("enc1", 37, "fwd_a", "fwd_b", "bwd_b"), _launched("dec1", 37, "fwd_a")
    ax, ay = x.args_bwd_a(), y.args_fwd_b()
    assert not ops.co_pairable("bwd_a", ax, "b", ay)
    n = _launches(lambda: ops.co_launch("bwd_a", ax, "b", ay))
    print(f"LAUNCHES co_launch bwd_a enc1 + fwd_b dec1: {n} (expected 2)")
    assert n == 2
