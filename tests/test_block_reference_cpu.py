"""Pins ``block_reference`` (the float64 oracle of the fused block kernels) without a GPU: its ``Y`` is the forward of
the project's own module in float64 with ``dropout_1`` replaced by the mask multiply, and its ``dR``, input gradient
and parameter gradients are float64 autograd of that module -- to 1e-12 relative, at every table shape and every
generic shape of the GPU test."""
import pytest
import torch

import block_reference as br

RTOL = 1e-12


def _close(got, want, what):
    scale = float(want.abs().max())
    err = float((got - want).abs().max())
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert err <= RTOL * max(scale, 1e-300), f"{what}: max err {err:.3e} against max |ref| {scale:.3e}"


@pytest.mark.parametrize("gy_bn", [False, True])
@pytest.mark.parametrize("rows", [2, 37])
@pytest.mark.parametrize("name", sorted(br.SHAPES))
def test_reference_is_float64_autograd_of_the_module(name, rows, gy_bn):
    m, Lin = br.make_block(name, seed=3)
    x, mask, g = br.make_inputs(m, Lin, rows, seed=3)
    assert (mask is not None) == (m.dropout_1 is not None)
    f = br.forward(m, x, mask, train=True)
    b = br.backward(m, f, g, mask, gy_bn=gy_bn)
    y, dR, dX, grads = br.module_autograd(m, x, g, mask, gy_bn=gy_bn)
    _close(f["Y"], y, "Y")
    _close(b["dR"], dR, "dR")
    _close(b["dX"], dX, "dX")
    assert set(b["params"]) == set(grads), (sorted(b["params"]), sorted(grads))
    for k in sorted(grads):
        _close(b["params"][k], grads[k], k)


@pytest.mark.parametrize("name", ["enc1", "dec1", "gen_c", "gen_d"])
def test_reference_eval_mode_and_running_statistics(name):
    """Eval mode normalises with the running buffers and leaves them alone; train mode moves them as
    ``torch.nn.BatchNorm1d`` does (momentum 0.1, unbiased variance)."""
    import copy
    m, Lin = br.make_block(name, seed=5)
    x, mask, _ = br.make_inputs(m, Lin, 9, seed=5)
    f = br.forward(m, x, None, train=False)
    mm = copy.deepcopy(m).double().eval()
    _close(f["Y"], mm(x.double()).detach(), "eval Y")
    for k, (rm, rv) in f["running"].items():
        _close(rm, getattr(m, k).running_mean.double(), k + ".running_mean (eval)")
        _close(rv, getattr(m, k).running_var.double(), k + ".running_var (eval)")
    f = br.forward(m, x, mask, train=True)
    mm = copy.deepcopy(m).double().train()
    if mm.dropout_1 is not None:
        mm.dropout_1 = br.MaskMul(mask.double())
    mm(x.double())
    assert set(f["running"]) == {k for k in ("bn1", "bn2", "bn_excit") if getattr(m, k) is not None}
    for k, (rm, rv) in f["running"].items():
        _close(rm, getattr(mm, k).running_mean, k + ".running_mean")
        _close(rv, getattr(mm, k).running_var, k + ".running_var")


def test_prelu_side_is_taken_from_the_supplied_tensor():
    """With ``sides`` the backward follows the supplied tensor's sign, element by element."""
    m, Lin = br.make_block("enc1", seed=1)
    x, mask, g = br.make_inputs(m, Lin, 5, seed=1)
    f = br.forward(m, x, mask)
    own = br.backward(m, f, g, mask)
    same = br.backward(m, f, g, mask, sides={k: f[k] for k in ("T1", "T2", "Sh", "E1", "E2")})
    assert torch.equal(own["dR"], same["dR"])
    flipped = br.backward(m, f, g, mask, sides={"T2": -f["T2"]})
    slope = m.relu2.weight.detach().double().view(1, -1, 1)
    want = torch.where(f["T2"] > 0, slope * g.double(), g.double())
    assert torch.equal(flipped["dT2"], want)
    assert torch.equal(flipped["dSh"], own["dSh"])
