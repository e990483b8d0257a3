"""The composed reference of ``option_matrix_reference`` without a GPU: the toy step against PyTorch in float64
(``torch.nn.utils.clip_grad_norm_``, the optimizer classes ``clip_reference`` wraps, a hand-rolled moving average), and
three WRONG compositions, each of which the tolerance ``test_option_matrix_gpu.py`` asserts tells from the right one --
the margins are printed.  Also: the NaN pattern of the GPU tests' data, and the resume fingerprint of ``C``."""
import numpy as np
import pytest
import torch

import clip_reference
import ema_reference
import option_matrix_reference as om
from oracle import ref_train
from partial_label_reference import masked_rank_loss
from rankaae_amd import resume
from rankaae_amd.synthetic import make_spectra

RULES = ["AdamW", "RAdam", "AdaBound"]
HYPER = [0.01, 0.9, 0.999, 1e-8, 0.01, 0.01, 0.1, 1e-3]
B, L, K, STEPS, SEED = 16, 64, 3, 3, 712


def _inputs():
    """Spiked rows (the kind ``test_spec_broaden_gpu._rows`` draws), descriptors with and without NaN cells, a noise
    term of the configurations' size, initial weights."""
    g = np.random.default_rng(5)
    rows = (g.standard_normal((STEPS, B, L)) + np.linspace(0.0, 4.0, L)).astype(np.float32)
    for k in range(STEPS):
        for r in range(B):
            rows[k, r, g.integers(0, L, 2)] += 40.0 * (1.0 if r % 2 else -1.0)
    d_full = g.standard_normal((STEPS, B, K)).astype(np.float32)
    d = d_full.copy()
    d[g.random(d.shape) < om.MISSING] = np.nan
    term = (0.02 * g.standard_normal((STEPS, B, L))).astype(np.float32).astype(np.float64)
    W = 0.1 * g.standard_normal((L, K))
    return rows, d, d_full, term, W


def _run(rule, wrong=None):
    rows, d, d_full, term, W = _inputs()
    toy = om.ToyStep(W, rule, HYPER)
    out = []
    for k in range(STEPS):
        info = toy.step(rows[k], d[k], SEED, k + 1, term[k], wrong=wrong, d_full=d_full[k])
        out.append(dict(info, W=toy.W[0].clone(), ema=toy.ema.clone(), m=toy.opt.state[toy.W[0]]["exp_avg"].clone()))
    return out


@pytest.mark.parametrize("rule", RULES)
def test_composed_step_is_pytorch_in_float64(rule):
    rows, d, d_full, term, W = _inputs()
    mine = _run(rule)
    p = torch.tensor(W, dtype=torch.float64, requires_grad=True)
    kw = dict(lr=HYPER[0], betas=(HYPER[1], HYPER[2]), eps=HYPER[3], weight_decay=HYPER[4])
    if rule == "AdaBound":
        kw.update(final_lr=HYPER[6], gamma=HYPER[7])
    opt = clip_reference.RULES[rule]([p], **kw)
    if rule == "RAdam":
        opt.compute_dtype = torch.float64
    ema = p.detach().clone()
    for k in range(STEPS):
        x = om.batch(rows[k], SEED, k + 1, om.BROADEN, om.SHIFT, term[k])
        z = torch.from_numpy(x) @ p
        loss, dz = masked_rank_loss(d[k], z.detach().numpy(), True)
        z.backward(torch.from_numpy(dz))                    # autograd carries d(loss)/dz to the weights
        total = float(torch.nn.utils.clip_grad_norm_([p], om.CLIP))
        opt.step()
        opt.zero_grad()
        ema = om.EMA * ema + (1.0 - om.EMA) * p.detach()
        got = mine[k]
        assert abs(got["loss"] - loss) <= 1e-12 * abs(loss) and abs(got["norm"] - total) <= 1e-12 * total
        assert got["scale"] < 1.0, "the toy step does not clip"
        assert float((got["W"] - p.detach()).abs().max()) <= 1e-12
        assert float((got["m"] - opt.state[p]["exp_avg"]).abs().max()) <= 1e-12
        assert float((got["ema"] - ema).abs().max()) <= 1e-14
    assert np.isnan(d).any() and not np.isnan(d).all(axis=1).all(axis=0).any()


@pytest.mark.parametrize("rule", RULES)
def test_tolerances_separate_three_wrong_compositions(rule):
    """For each mistake, the largest ratio of its difference from the right composition to the tolerance the GPU test
    asserts for that quantity, over the steps: above 1 means a step engine with that mistake fails.  Asserted at 4, so
    that the code under test's own rounding (at most the tolerance) cannot close the gap."""
    rows, d, d_full, term, W = _inputs()
    right = _run(rule)
    margins = {}
    # the average: k accumulated single-step bounds of ema_reference, as tests/test_ema_gpu.py asserts after step k
    wrong = _run(rule, "average before the update")
    big, worst = torch.as_tensor(W).abs(), 0.0
    for k in range(STEPS):
        assert torch.equal(wrong[k]["W"], right[k]["W"])
        big = torch.maximum(big, right[k]["W"].abs())
        bound = (k + 1) * ema_reference.step_bound(big, big)
        worst = max(worst, float(((wrong[k]["ema"] - right[k]["ema"]).abs() / bound).max()))
    margins["average before the update"] = worst
    # the update: the parameters after step 1 (teacher forcing: every step starts from the code's own state)
    wrong = _run(rule, "norm over the un-masked gradient")
    diff = (wrong[0]["W"] - right[0]["W"]).abs() / (om.UPDATE_ATOL + om.UPDATE_RTOL * right[0]["W"].abs())
    stat = abs(wrong[0]["scale"] - right[0]["scale"]) / (om.STAT_RTOL * right[0]["scale"])
    margins["norm over the un-masked gradient"] = min(float(diff.max()), stat)
    # the batch: broaden_reference.error_bound plus the noise term's roundings
    worst = 0.0
    for k in range(STEPS):
        x = om.batch(rows[k], SEED, k + 1, om.BROADEN, om.SHIFT, term[k], "shift, broaden")
        bound = om.batch_bound(rows[k], SEED, k + 1, om.BROADEN, om.SHIFT, right[k]["batch"], term[k])
        worst = max(worst, float((np.abs(x - right[k]["batch"]) / bound).max()))
    margins["shift before broaden"] = worst
    print(f"{rule}: difference / tolerance of each wrong composition: " + ", ".join(f"{n} {m:.3g}" for n, m in margins.items()))
    assert all(m > 4.0 for m in margins.values()), margins


def test_teacher_forced_update_follows_the_free_running_optimizer():
    """``teacher_forced_update`` fed its own results step after step is the optimizer left alone -- for every rule, so
    the step count behind RAdam's rectification and AdaBound's bounds advances as it should."""
    g = torch.Generator().manual_seed(2)
    for rule in RULES:
        p0 = torch.randn(40, generator=g)
        free = [p0.double().clone()]
        opt = om.make_optimizer(rule, free, HYPER)
        table, p, m, v = {}, p0.double(), torch.zeros(40, dtype=torch.float64), torch.zeros(40, dtype=torch.float64)
        for _ in range(7):                                  # (RAdam's rectified form begins at step 6)
            grad = torch.randn(40, generator=g)
            p, m, v, norm, scale = om.teacher_forced_update(table, "x", rule, HYPER, p, m, v, grad, om.CLIP)
            clip_reference.clipped_step(opt, free, [grad], om.CLIP)
            assert scale < 1.0 and float((p - free[0]).abs().max()) <= 1e-15, rule
            assert float((v - opt.state[free[0]]["exp_avg_sq"]).abs().max()) <= 1e-18


def test_gpu_tests_data_has_a_gap_in_every_batch():
    for n, seed, b, steps, perms in ((700, 3, 64, 4, (1, 2, 50, 51)), (1600, 8, 256, 4, (3, 50, 51))):
        spec, aux, _ = make_spectra(n, 256, 5, seed=seed)
        n_train = ref_train.split_rows(n)[0]
        part = om.with_missing_labels(aux)
        assert 0.25 < np.isnan(part).mean() < 0.35
        for ps in perms:
            perm = torch.randperm(n_train, generator=torch.Generator().manual_seed(ps)).numpy()
            assert om.every_batch_has_a_gap(part[:n_train], perm, b, steps), (n, ps)
        assert not om.every_batch_has_a_gap(aux[:n_train], np.arange(n_train), b, 1)


def test_resume_fingerprint_refuses_c_without_any_one_key():
    """What the engine's own state does not carry (the augmentation keys) the resume file's fingerprint does: ``C``
    against ``C`` without any one of the four keys is refused, naming the key."""
    spec = np.ones((4, 8), dtype=np.float32)
    fp = lambda cfg: resume.fingerprint(cfg, 1, 640, 4, 2, spec)       # noqa: E731
    c = om.combined({"ae_form": "FC", "nstyle": 2})
    for key in ("grad_clip_norm", "ema_decay", "spec_shift", "spec_broaden"):
        with pytest.raises(ValueError, match=key):
            resume.check_fingerprint(fp(c), fp(om.combined(c, **{key: ...})))
    resume.check_fingerprint(fp(c), fp(dict(c)))
