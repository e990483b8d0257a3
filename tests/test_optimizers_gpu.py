"""``optimizer_name: RAdam / AdaBound`` on the GPU: the fused updates of ``raae_optim_step`` against the restated
torch_optimizer 0.1.0 rules of ``optim_reference``, from the kernel up to ``Trainer``.

ops      ``ops.optim_step`` over 14 steps: both kernel shapes, an all-zero gradient step, a segment without slabs, an lr
         cut mid-run (AdaBound's bounds move with lr / base_lr, base_lr stays), gradients spanning eight decades so
         that AdaBound's clamp binds at both ends; tolerance of ``test_adam_matches_torch``.
engine   P2 of ``test_engine_gpu`` (teacher-forced phases, its gradient bounds and escape-hatch ceilings) with the oracle
         trainer's optimizers replaced by the restated rules, through step 6: RAdam's first rectified step.
trials   a ``TrialBatch`` (kernels with gridDim.z = trials) is bit for bit the trials stepped alone.
trainer  two epochs through ``Trainer.from_data``: files written, losses finite, weights not AdamW's.
"""
import json
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from optim_reference import OPTIMIZERS
from rankaae_amd.synthetic import make_spectra, write_csv

if torch.cuda.is_available():
    import test_engine_gpu as p2
    from oracle import ref_train
    from rankaae_amd import _lib, model as pm, ops
    from rankaae_amd.engine import StepEngine
    DEV = torch.device("cuda:0")
    RULES = {"RAdam": _lib.OPT_RADAM, "AdaBound": _lib.OPT_ADABOUND}

NAMES = ["RAdam", "AdaBound"]


def _close(a, b, rtol, atol, what):
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    err = (a - b).abs() - (atol + rtol * b.abs())
    assert float(err.max()) <= 0, f"{what}: max excess {float(err.max()):.3e} at {int(err.argmax())}"


@pytest.mark.parametrize("wd", [0.0, 0.01])
@pytest.mark.parametrize("name", NAMES)
def test_optim_step_matches_the_restated_rule(name, wd):
    g = torch.Generator().manual_seed(11)
    n, nslab = 64 * 40, 3
    # AdaBound: per-segment gradient scales 5e-4, 1, 100 -- its step lr*sqrt(bc2)/bc1/sqrt(v) then meets the upper
    # bound, neither, the lower bound (without weight decay: wd*p outweighs the smallest gradients)
    scale = torch.ones(n)
    if name == "AdaBound":
        scale = torch.tensor([5e-4, 1.0, 100.0]).repeat(n // 64)[:n // 64].repeat_interleave(64)
    p0 = torch.randn(n, generator=g)
    ref = p0.clone().requires_grad_(True)
    opt = OPTIMIZERS[name]([ref], lr=0.01, betas=(0.9, 0.999), weight_decay=wd)
    p, m, v = p0.to(DEV), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    hyper = torch.tensor([0.01, 0.9, 0.999, 1e-8, wd, 0.01, 0.1, 1e-3], dtype=torch.float64, device=DEV)
    step = torch.zeros(2, dtype=torch.int32, device=DEV)
    seg = torch.full((n // 64,), nslab, dtype=torch.int16, device=DEV)
    seg[5] = 0          # one segment "without gradient": must be left untouched
    clamped = [0, 0]
    for it in range(14):
        if it == 9:     # ReduceLROnPlateau's cut: only the lr moves (engine: OptState.push)
            opt.param_groups[0]["lr"] = 0.001
            hyper[0] = 0.001
        slabs = torch.randn(nslab, n, generator=g) * scale * (0.0 if it == 3 else 1.0)     # one all-zero gradient step
        ref.grad = (slabs[0] + slabs[1]) + slabs[2]
        opt.step()
        step[1:].add_(1)
        ops.optim_step(p, m, v, slabs.to(DEV), n, seg, n, RULES[name], hyper, step[1:],
                       max_nslab=(3 if it % 2 else 40))          # per-thread and 8-lanes-per-element kernels
        if name == "AdaBound" and wd == 0.0 and it > 3:
            st, lr, t = opt.state[ref], opt.param_groups[0]["lr"], it + 1
            ratio = lr * math.sqrt(1 - 0.999 ** t) / (1 - 0.9 ** t) / (st["exp_avg_sq"].sqrt() + 1e-8)
            flr = 0.1 * lr / 0.01
            clamped[0] += int((ratio < flr * (1 - 1 / (1e-3 * t + 1))).sum())
            clamped[1] += int((ratio > flr * (1 + 1 / (1e-3 * t))).sum())
    torch.cuda.synchronize()
    assert step.tolist() == [0, 14] and opt.state[ref]["step"] == 14
    assert float(hyper[5]) == 0.01, "base_lr stays"
    if name == "AdaBound" and wd == 0.0:
        assert min(clamped) > 1000, f"the clamp did not bind at both ends: {clamped}"
    pr, mr, vr = ref.detach().clone(), opt.state[ref]["exp_avg"].clone(), opt.state[ref]["exp_avg_sq"].clone()
    pr[5 * 64:6 * 64] = p0[5 * 64:6 * 64]
    mr[5 * 64:6 * 64] = 0
    vr[5 * 64:6 * 64] = 0
    _close(p, pr, 2e-6, 2e-7, f"{name} params after 14 steps")
    _close(m.cpu() / scale, mr / scale, 2e-6, 2e-7, f"{name} exp_avg (in units of the segment's gradient scale)")
    _close(v.cpu() / scale ** 2, vr / scale ** 2, 2e-6, 2e-7, f"{name} exp_avg_sq (same)")


@pytest.mark.parametrize("name", NAMES)
def test_optim_step_many_slabs_lane_split(name):
    """Ranges with many gradient slabs take the 8-lanes-per-element kernel: same update as one thread per element,
    and both as the rule on the host sum of the slabs."""
    g = torch.Generator().manual_seed(5)
    n, rows = 64 * 6, 200
    slabs = torch.randn(rows, n, generator=g)
    counts = [200, 37, 0, 8, 65, 1]
    seg = torch.tensor(counts, dtype=torch.int16, device=DEV)
    p0 = torch.randn(n, generator=g)
    hyper = torch.tensor([0.01, 0.9, 0.999, 1e-8, 0.01, 0.01, 0.1, 1e-3], dtype=torch.float64, device=DEV)
    step = torch.full((1,), 7, dtype=torch.int32, device=DEV)     # RAdam: a rectified step
    out = []
    m0 = torch.randn(n, generator=g) * 0.1
    v0 = torch.rand(n, generator=g)
    for hint in (8, 200):
        p, m, v = p0.to(DEV), m0.to(DEV), v0.to(DEV)
        ops.optim_step(p, m, v, slabs.to(DEV), n, seg, n, RULES[name], hyper, step, max_nslab=hint)
        out.append((p.cpu(), m.cpu(), v.cpu()))
    grad = torch.stack([slabs[:c, 64 * i:64 * (i + 1)].double().sum(0) for i, c in enumerate(counts)]).reshape(-1)
    ref = p0.clone().requires_grad_(True)
    opt = OPTIMIZERS[name]([ref], lr=0.01, weight_decay=0.01)
    opt.state[ref] = {"step": 6, "exp_avg": m0.clone(), "exp_avg_sq": v0.clone()}
    ref.grad = grad.float()
    opt.step()
    keep = torch.tensor(counts).repeat_interleave(64) > 0
    for got, want, what in zip(out[1], (ref.detach(), opt.state[ref]["exp_avg"], opt.state[ref]["exp_avg_sq"]),
                               ("p", "m", "v")):
        _close(got[keep], want[keep], 1e-5, 1e-6, f"{name} lane-split {what} vs the rule on the host sum")
    for a, b in zip(out[0], out[1]):
        _close(a, b, 1e-5, 1e-6, f"{name} lane-split vs per-thread")
    assert torch.equal(out[1][0][128:192], p0[128:192]), "segment without slabs untouched"


def test_optim_step_rejects_a_short_hyper_block():
    t = torch.zeros(64, device=DEV)
    with pytest.raises(ValueError, match="reads 8"):
        ops.optim_step(t, t, t, t, 64, torch.ones(1, dtype=torch.int16, device=DEV), 64, _lib.OPT_RADAM,
                       torch.zeros(5, dtype=torch.float64, device=DEV), torch.ones(1, dtype=torch.int32, device=DEV))


# ---------------------------------------------------------------------------------------------------- engine (P2)
def _oracle_with(name):
    """The oracle trainer with the optimizers of ``Trainer.load_optimizers`` (trainer.py:333-387) built from the
    restated class: weight decay and betas where the reference passes them, the class defaults elsewhere."""
    cls = OPTIMIZERS[name]

    class Oracle(ref_train.OracleTrainer):
        def _load_optimizers(self):
            c = self.cfg
            enc, dec, dis = self.encoder, self.decoder, self.discriminator
            lr = c["lr_base"]
            betas_d = (c["dis_beta"] * 0.9, c["dis_beta"] * 0.009 + 0.99)
            self.optimizers = {
                "reconstruction": cls([{"params": enc.parameters()}, {"params": dec.parameters()}],
                                      lr=c["lr_ratio_Reconn"] * lr, weight_decay=c["weight_decay"]),
                "mutual_info": cls([{"params": enc.parameters()}, {"params": dec.parameters()}],
                                   lr=c["lr_ratio_Mutual"] * lr),
                "smoothness": cls([{"params": dec.parameters()}], lr=c["lr_ratio_Smooth"] * lr,
                                  weight_decay=c["weight_decay"]),
                "correlation": cls([{"params": enc.parameters()}], lr=c["lr_ratio_Corr"] * lr,
                                   weight_decay=c["weight_decay"]),
                "adversarial": cls([{"params": dis.parameters()}, {"params": enc.parameters()}],
                                   lr=c["lr_ratio_dis"] * lr, betas=betas_d),
            }
    return Oracle


@pytest.mark.parametrize("case,steps", [("fc_example", (1, 5)), ("fc_small", (1, 6)), ("compact_small", (1, 6))])
@pytest.mark.parametrize("name", NAMES)
def test_p2_teacher_forced_steps_with_the_rule(name, case, steps, monkeypatch):
    """``test_engine_gpu._p2`` unchanged -- the five losses to 1e-4 and every phase gradient within its bound at the
    compared steps -- with the case's config asking for ``name`` and the oracle stepping the restated rule.  Step 1
    starts from the oracle's initial state; at step 6 (five oracle steps in, moments and step counts loaded into the
    engine) RAdam makes its first rectified update.  (fc_example's epoch holds five batches of 1024 rows.)"""
    load_case = p2.load_case

    def load_case_with_the_rule(c):
        g, cfg, spec, aux = load_case(c)
        return g, dict(cfg, optimizer_name=name), spec, aux
    monkeypatch.setattr(p2, "load_case", load_case_with_the_rule)
    monkeypatch.setattr(ref_train, "OracleTrainer", _oracle_with(name))
    p2._p2(case, steps, use_graph=False)


def test_engine_applies_the_reference_table():
    """Learning rates, betas and weight decay of the five optimizers; 0 where the reference passes no weight decay
    (the class default), AdaBound's base_lr = the lr at construction."""
    g, cfg, spec, aux = p2.load_case("fc_small")
    for name in NAMES:
        c = dict(cfg, optimizer_name=name, weight_decay=0.02)
        eng = p2.build_engine(c, 1, spec, aux)
        lr = c["lr_base"]
        want = {"reconstruction": (c["lr_ratio_Reconn"], 0.02), "mutual_info": (c["lr_ratio_Mutual"], 0.0),
                "smoothness": (c["lr_ratio_Smooth"], 0.02), "correlation": (c["lr_ratio_Corr"], 0.02),
                "adversarial": (c["lr_ratio_dis"], 0.0)}
        for key, (ratio, wd) in want.items():
            o = eng.opts[key]
            betas = (c["dis_beta"] * 0.9, c["dis_beta"] * 0.009 + 0.99) if key == "adversarial" else (0.9, 0.999)
            assert o.rule == RULES[name]
            assert o.hyper.cpu().tolist() == [ratio * lr, betas[0], betas[1], 1e-8, wd, ratio * lr, 0.1, 1e-3], key
        o = eng.opts["smoothness"]
        o.lr *= 0.1
        o.push()
        assert float(o.hyper[0]) == 0.1 * o.base_lr and float(o.hyper[5]) == o.base_lr


# ---------------------------------------------------------------------------------------------------- trials
@pytest.mark.parametrize("ae_form", ["FC", "compact"])
@pytest.mark.parametrize("name", NAMES)
def test_trial_batch_with_the_rule_is_bitwise_the_trials_alone(name, ae_form):
    """Four trials at 256 rows stepped by ONE launch sequence (``TrialBatch``: the optimizer kernels' batched forms,
    gridDim.z = 4) over 8 steps -- eager, captured and replayed -- hold bit for bit the weights, moments, BatchNorm
    statistics and losses of each trial stepped alone.  No ``BatchingRefused``."""
    from rankaae_amd.trial_batch import TrialBatch
    with open(os.path.join(os.path.dirname(__file__), "golden",
                           "ref_fc_small.json" if ae_form == "FC" else "ref_compact_small.json")) as f:
        cfg = dict(json.load(f)["config"])
    T, bs = 4, 256
    cfg.update(optimizer_name=name, batch_size=bs)
    spec, aux, _ = make_spectra(1600, 256, cfg["n_aux"], seed=8)
    n_train = ref_train.split_rows(len(spec))[0]
    per_epoch = n_train // bs

    def make(t, stream=None):
        torch.manual_seed(200 + t)
        cls = pm.AE_CLS_DICT[cfg["ae_form"]]
        enc = cls["encoder"](nstyle=cfg["nstyle"], dropout_rate=cfg["dropout_rate"], dim_in=cfg["dim_in"],
                             n_layers=cfg["n_layers"])
        dec = cls["decoder"](nstyle=cfg["nstyle"], dropout_rate=cfg["dropout_rate"],
                             last_layer_activation=cfg["decoder_activation"], dim_out=cfg["dim_out"],
                             n_layers=cfg["n_layers"])
        dis = pm.DiscriminatorFC(nstyle=cfg["nstyle"], dropout_rate=cfg["dis_dropout_rate"], noise=cfg["dis_noise"],
                                 layers=cfg["FC_discriminator_layers"])
        eng = StepEngine(enc, dec, dis, cfg, DEV, rng_mode="philox", seed=700 + t, use_graph=True, stream=stream)
        eng.set_data(spec[:n_train], aux[:n_train])
        return eng

    def state(e):
        torch.cuda.synchronize()
        return ([e.arena.P.clone()] + [b_.clone() for mod in (e.enc_mod, e.dec_mod) for b_ in mod.buffers()] +
                [o.m.clone() for o in e.opts.values()] + [o.v.clone() for o in e.opts.values()], e.losses())

    def perm(t, ep):
        return torch.randperm(n_train, generator=torch.Generator().manual_seed(1000 * t + ep))

    def run(trials, step):          # trials: {trial index: engine}
        for s in range(8):
            if s % per_epoch == 0:
                for t, e in trials.items():
                    e.set_epoch(perm(t, s // per_epoch), 0.3)
            step()
    alone = []
    for t in range(T):
        e = make(t)
        run({t: e}, lambda: e.step(bs))
        alone.append(state(e))
    shared = TrialBatch.shared_stream(DEV)
    engs = [make(t, shared) for t in range(T)]
    batch = TrialBatch(engs)
    run(dict(enumerate(engs)), lambda: batch.step(bs))
    assert batch.programs[(bs, True)][1] is not None
    for t, e in enumerate(engs):
        got = state(e)
        for a, b in zip(alone[t][0], got[0]):
            assert torch.equal(a, b), f"{name} {ae_form}: trial {t} differs from the same trial alone"
        assert alone[t][1] == got[1]
    assert int(engs[0].steps_dev[0]) == 8 and all(np.isfinite(list(alone[0][1].values())))
    batch.release()


# ---------------------------------------------------------------------------------------------------- trainer
@pytest.mark.parametrize("case", ["fc_small", "compact_small"])
def test_trainer_two_epochs_with_each_rule(case, tmp_path):
    from rankaae_amd.logger import create_logger
    from rankaae_amd.parameter import Parameters
    from rankaae_amd.trainer import Trainer
    with open(os.path.join(os.path.dirname(__file__), "golden", f"ref_{case}.json")) as f:
        g = json.load(f)
    spec, aux, grid = make_spectra(g["n_rows"], g["n_points"], g["config"]["n_aux"], seed=g["data_seed"])
    csv = tmp_path / "data.csv"
    write_csv(str(csv), spec, aux, grid)
    weights = {}
    for name in ("AdamW", "RAdam", "AdaBound"):
        wd = tmp_path / name
        wd.mkdir()
        cfg = dict(g["config"], optimizer_name=name, rng_mode="philox", seed=5, max_epoch=2)
        log = create_logger(f"losses_{case}_{name}", str(wd / "losses.csv"), simple_fmt=True)
        try:
            torch.manual_seed(g["model_seed"])
            tr = Trainer.from_data(str(csv), igpu=0, verbose=False, work_dir=str(wd),
                                   config_parameters=Parameters(cfg), loss_logger=log)
            metrics = tr.train()
        finally:
            for h in list(log.handlers):
                h.close()
                log.removeHandler(h)
        assert len(metrics) == 5 and all(np.isfinite(metrics)), (name, metrics)
        rows = (wd / "losses.csv").read_text().splitlines()
        assert rows[0].startswith("Epoch,Train_D") and len(rows) >= 2, rows
        for row in rows[1:]:
            vals = [float(x) for x in row.split(",\t")[1:-1]]
            assert len(vals) == 12 and all(np.isfinite(vals)), (name, row)
        model = torch.load(str(wd / "final.pt"), map_location="cpu", weights_only=False)
        assert set(model) == {"Encoder", "Decoder", "Style Discriminator"}
        weights[name] = torch.cat([p.detach().reshape(-1) for key in ("Encoder", "Decoder", "Style Discriminator")
                                   for p in model[key].parameters()])
        assert torch.isfinite(weights[name]).all()
    for name in ("RAdam", "AdaBound"):      # the rule is active: same seeds and data, other weights
        assert not torch.equal(weights[name], weights["AdamW"]), name
    assert not torch.equal(weights["RAdam"], weights["AdaBound"])
