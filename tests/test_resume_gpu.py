"""Checkpoint / resume (config keys ``checkpoint_every`` / ``resume``) on the GPU: a run that is stopped, or abandoned,
and continued by a FRESH ``Trainer`` from the trial's resume file ends bit for bit where the uninterrupted run ends --
parameters, BatchNorm buffers, optimizer state, metrics, ``losses.csv``.  Every comparison is exact: the resumed run
executes the same kernels on the same bits.

Sizes: 200 synthetic rows (140 training rows: four batches of 32 and a ragged one of 12), 256-point spectra,
``nstyle: 3``, ``n_aux: 2``, 6 epochs, the smoothness phase ends after epoch 2, ``sch_patience: 0`` with
``sch_factor: 0.5`` so that the learning rates are cut on both sides of the checkpoint (asserted)."""
import logging
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

from rankaae_amd import resume as rf
from rankaae_amd.synthetic import make_spectra

if torch.cuda.is_available():
    from rankaae_amd import model as pm
    from rankaae_amd.engine import OPT_NAMES, StepEngine
    from rankaae_amd.parameter import Parameters
    from rankaae_amd.trainer import Trainer, train_trials_batched

CFG = dict(trials=1, timeout=10, verbose=False, max_epoch=6, batch_size=32, gradient_reversal=True, alpha_flat_step=739,
           alpha_limit=0.7172, decoder_activation="Softplus", dis_beta=1.1, dis_dropout_rate=0.056, dis_noise=0.56,
           gen_beta=1.1, n_aux=2, nstyle=3, ae_form="FC", dim_in=256, dim_out=256, n_layers=3, FC_discriminator_layers=3,
           use_cnn_discriminator=False, dropout_rate=0.04, sch_factor=0.5, sch_patience=0, lr_base=0.001,
           lr_ratio_Corr=10, lr_ratio_Mutual=1, lr_ratio_Reconn=10, lr_ratio_Smooth=1, lr_ratio_dis=1, lr_ratio_gen=10,
           optimizer_name="AdamW", spec_noise=0.02, use_flex_spec_target=True, weight_decay=0.01, kendall_activation=True,
           epoch_stop_smooth=3)
SEED = {"FC": 11, "compact": 11}        # (the schedule test asserts what a seed has to give)
CKPT_EPOCH = 3                          # checkpoint_every: 2 writes after epochs 1, 3 and 5
_counter = [0]


def _data():
    spec, aux, _ = make_spectra(200, 256, 2, seed=5)
    return spec, aux


def _cfg(ae_form, **kw):
    return {**CFG, "ae_form": ae_form, "n_layers": 3 if ae_form == "FC" else 5, **kw}


class _Trial:
    """A Trainer on the synthetic data with a private host generator and a ``losses.csv`` logger that appends."""

    def __init__(self, wd, cfg, seed, stream=None):
        os.makedirs(wd, exist_ok=True)
        _counter[0] += 1
        self.log = logging.getLogger(f"resume_gpu_{_counter[0]}")
        self.log.setLevel(logging.DEBUG)
        self.log.propagate = False
        self.handler = logging.FileHandler(os.path.join(wd, "losses.csv"))
        self.handler.setFormatter(logging.Formatter("%(message)s"))
        self.log.addHandler(self.handler)
        quiet = logging.getLogger("resume_gpu_quiet")
        quiet.addHandler(logging.NullHandler())
        quiet.propagate = False
        gen = torch.Generator().manual_seed(seed)
        torch.manual_seed(seed)                 # the networks' initial weights come from the global generator
        self.wd = str(wd)
        self.trainer = Trainer.from_data(None, igpu=0, verbose=False, work_dir=self.wd, config_parameters=Parameters(cfg),
                                         logger=quiet, loss_logger=self.log, arrays=_data(), host_rng=gen,
                                         engine_stream=stream)

    def optimizers(self):
        eng = self.trainer.engine
        torch.cuda.synchronize()
        steps = eng.steps_dev.cpu()
        return {n: (o.lr, o.base_lr, o.m.cpu(), o.v.cpu(), int(steps[o.index])) for n, o in eng.opts.items()}

    def close(self):
        self.trainer.engine.release()
        self.log.removeHandler(self.handler)
        self.handler.close()

    def outcome(self, metrics):
        """What the run left behind, on the host; releases the engine."""
        out = {"metrics": metrics, "optimizers": self.optimizers(), "final": _final(self.wd),
               "losses": open(os.path.join(self.wd, "losses.csv"), "rb").read()}
        self.close()
        return out


def _final(wd):
    mods = torch.load(os.path.join(wd, "final.pt"), weights_only=False)
    return {f"{key}.{name}": t.cpu() for key, mod in mods.items() for name, t in mod.state_dict().items()}


def _assert_same_outcome(got, want):
    assert got["final"].keys() == want["final"].keys()
    assert any(k.endswith("num_batches_tracked") for k in want["final"]) and any(k.endswith("running_var") for k in want["final"])
    for k, t in want["final"].items():
        assert torch.equal(got["final"][k], t), k
    assert got["metrics"] == want["metrics"] and all(type(m) is float for m in got["metrics"])
    for n in OPT_NAMES:
        lr, base_lr, m, v, step = want["optimizers"][n]
        glr, gbase, gm, gv, gstep = got["optimizers"][n]
        assert (glr, gbase, gstep) == (lr, base_lr, step), n
        assert torch.equal(gm, m) and torch.equal(gv, v), n
    assert got["losses"] == want["losses"]


_uninterrupted = {}


def _run_a(ae_form, optimizer, tmp_path_factory):
    """The uninterrupted run (``checkpoint_every: 2``), once per configuration; shared, never changed."""
    key = (ae_form, optimizer)
    if key not in _uninterrupted:
        wd = tmp_path_factory.mktemp(f"a_{ae_form}_{optimizer}")
        a = _Trial(wd, _cfg(ae_form, optimizer_name=optimizer, checkpoint_every=2), SEED[ae_form])
        lrs = []
        metrics = a.trainer.train(lambda epoch, m: lrs.append([o.lr for o in a.trainer.engine.opts.values()]))
        st = torch.load(os.path.join(a.wd, rf.NAME), weights_only=True)
        out = a.outcome(metrics)
        out.update(lrs=lrs, last_file=st, files=sorted(os.listdir(a.wd)))
        _uninterrupted[key] = out
    return _uninterrupted[key]


class _Abandon(Exception):
    pass


@pytest.mark.parametrize("ae_form", ["FC", "compact"])
def test_schedule_is_exercised_on_both_sides_of_the_checkpoint(ae_form, tmp_path_factory):
    """Restored scheduler state matters only if the learning rates are cut before AND after the checkpoint."""
    a = _run_a(ae_form, "AdamW", tmp_path_factory)
    lrs = [[1e-3 * CFG[k] for k in ("lr_ratio_dis", "lr_ratio_Corr", "lr_ratio_Reconn", "lr_ratio_Mutual", "lr_ratio_Smooth")]] + a["lrs"]
    assert len(lrs) == 7
    cut = [e for e in range(6) if lrs[e + 1] != lrs[e]]            # epochs after which the schedulers cut
    print(f"\n{ae_form}: learning-rate cuts after epochs {cut}")
    assert any(e <= CKPT_EPOCH for e in cut), cut
    assert any(e > CKPT_EPOCH for e in cut), cut
    # the last file of a finished run says so, and holds the final metrics
    assert a["last_file"]["finished"] is True and a["last_file"]["epoch"] == 5 and a["last_file"]["error"] is None
    assert a["last_file"]["metrics"] == a["metrics"]
    assert rf.NAME in a["files"] and rf.PREV_NAME in a["files"] and rf.TMP_NAME not in a["files"]


@pytest.mark.parametrize("ae_form,optimizer", [("FC", "AdamW"), ("compact", "AdamW"), ("FC", "AdaBound")])
def test_stopped_run_continues_bit_for_bit(ae_form, optimizer, tmp_path, tmp_path_factory):
    """B is asked to stop during epoch 3 (``request_stop`` from the callback of epoch 2): ``train`` raises at that epoch's
    boundary and leaves the stop-time file; a fresh Trainer with ``resume: true`` ends where the uninterrupted run ends."""
    want = _run_a(ae_form, optimizer, tmp_path_factory)
    cfg = _cfg(ae_form, optimizer_name=optimizer, checkpoint_every=2)
    b = _Trial(tmp_path, cfg, SEED[ae_form])
    with pytest.raises(Exception, match="Training Overtime!"):
        b.trainer.train(lambda epoch, m: b.trainer.request_stop() if epoch == CKPT_EPOCH - 1 else None)
    b.close()
    st = torch.load(tmp_path / rf.NAME, weights_only=True)
    assert st["epoch"] == CKPT_EPOCH and st["tail_pending"] is True and st["finished"] is False     # the stop-time write
    assert torch.load(tmp_path / rf.PREV_NAME, weights_only=True)["epoch"] == 1
    assert int(st["engine"]["nan_flags"].abs().sum()) == 0
    del b
    c = _Trial(tmp_path, {**cfg, "resume": True}, SEED[ae_form] + 1000)     # other initial weights: all of it is restored
    seen = []
    metrics = c.trainer.train(lambda epoch, m: seen.append(epoch))
    assert seen == [3, 4, 5]                    # epoch 3's callback, which the stop pre-empted, then the remaining epochs
    _assert_same_outcome(c.outcome(metrics), want)


@pytest.mark.parametrize("ae_form", ["FC", "compact"])
def test_abandoned_run_resumes_from_the_periodic_file(ae_form, tmp_path, tmp_path_factory):
    """B dies after epoch 4 with no stop-time write: the file of epoch 3 stands, the resumed run redoes epochs 4 and 5;
    a ``losses.csv`` row from beyond the checkpoint is cut off."""
    want = _run_a(ae_form, "AdamW", tmp_path_factory)
    cfg = _cfg(ae_form, checkpoint_every=2)
    b = _Trial(tmp_path, cfg, SEED[ae_form])

    def die(epoch, m):
        if epoch == 4:
            raise _Abandon()
    with pytest.raises(_Abandon):
        b.trainer.train(die)
    b.close()
    del b
    st = torch.load(tmp_path / rf.NAME, weights_only=True)
    assert st["epoch"] == CKPT_EPOCH and st["tail_pending"] is False
    with open(tmp_path / "losses.csv", "ab") as f:
        f.write(b"10,\t9.000000,\t9.000000,\t\n")
    c = _Trial(tmp_path, {**cfg, "resume": True}, SEED[ae_form])
    seen = []
    metrics = c.trainer.train(lambda epoch, m: seen.append(epoch))
    assert seen == [4, 5]
    got = c.outcome(metrics)
    assert b"9.000000" not in got["losses"]
    _assert_same_outcome(got, want)


def test_fingerprint_mismatch_refuses_to_resume(tmp_path):
    b = _Trial(tmp_path, _cfg("FC", checkpoint_every=1, max_epoch=1), SEED["FC"])
    b.trainer.train()
    b.close()
    c = _Trial(tmp_path, _cfg("FC", checkpoint_every=1, max_epoch=1, resume=True, lr_ratio_Corr=5), SEED["FC"])
    with pytest.raises(ValueError, match="cfg.lr_ratio_Corr"):
        c.trainer.train()
    c.close()


_batched = {}


def _group(base, cfg, tag):
    stream = torch.cuda.Stream()
    return [_Trial(os.path.join(base, f"{tag}_{k}"), cfg, 40 + k, stream=stream) for k in range(2)]


def _run_batched_a(ae_form, tmp_path_factory):
    if ae_form not in _batched:
        base = str(tmp_path_factory.mktemp(f"batched_{ae_form}"))
        group = _group(base, _cfg(ae_form, checkpoint_every=2), "a")
        metrics = train_trials_batched([t.trainer for t in group])
        _batched[ae_form] = [t.outcome(m) for t, m in zip(group, metrics)]
    return _batched[ae_form]


@pytest.mark.parametrize("ae_form,swap", [("FC", False), ("FC", True), ("compact", True)])
def test_batched_group_resumes_from_one_epoch(ae_form, swap, tmp_path, tmp_path_factory):
    """Two trials in lockstep, stopped during epoch 3 and resumed as a group.  ``swap``: trial 1's newest file is
    replaced by its older generation -- the group then resumes from the older epoch both offer, and ends the same."""
    want = _run_batched_a(ae_form, tmp_path_factory)
    cfg = _cfg(ae_form, checkpoint_every=2)
    group = _group(str(tmp_path), cfg, "b")
    stop = lambda epoch, m: group[0].trainer.request_stop() if epoch == CKPT_EPOCH - 1 else None      # noqa: E731
    with pytest.raises(Exception, match="Training Overtime!"):
        train_trials_batched([t.trainer for t in group], callbacks=[stop, None])
    dirs = [t.wd for t in group]
    for t in group:
        t.close()
    del group
    assert [rf.offered_epochs(d) for d in dirs] == [[3, 1], [3, 1]]
    if swap:
        os.replace(os.path.join(dirs[1], rf.PREV_NAME), os.path.join(dirs[1], rf.NAME))
        assert rf.offered_epochs(dirs[1]) == [1, rf.FRESH]
    group = _group(str(tmp_path), {**cfg, "resume": True}, "b")
    seen = []
    metrics = train_trials_batched([t.trainer for t in group], callbacks=[lambda epoch, m: seen.append(epoch), None])
    assert seen == ([2, 3, 4, 5] if swap else [3, 4, 5])
    for t, m, w in zip(group, metrics, want):
        _assert_same_outcome(t.outcome(m), w)


def test_batched_group_without_a_common_epoch_raises(tmp_path):
    """Trial 1 dies one file behind trial 0; with trial 0's older generation deleted the two offer no common epoch."""
    cfg = _cfg("FC", checkpoint_every=1, max_epoch=4)
    group = _group(str(tmp_path), cfg, "c")

    def die(epoch, m):
        if epoch == 2:
            raise _Abandon()
    with pytest.raises(_Abandon):
        train_trials_batched([t.trainer for t in group], callbacks=[None, die])
    dirs = [t.wd for t in group]
    for t in group:
        t.close()
    del group
    assert [rf.offered_epochs(d) for d in dirs] == [[2, 1], [1, 0]]
    os.remove(os.path.join(dirs[0], rf.PREV_NAME))
    group = _group(str(tmp_path), {**cfg, "resume": True}, "c")
    try:
        with pytest.raises(ValueError, match="no common epoch"):
            train_trials_batched([t.trainer for t in group])
    finally:
        for t in group:
            t.close()


def _modules(cfg, seed):
    torch.manual_seed(seed)
    cls = pm.AE_CLS_DICT[cfg["ae_form"]]
    enc = cls["encoder"](nstyle=cfg["nstyle"], dropout_rate=cfg["dropout_rate"], dim_in=256, n_layers=cfg["n_layers"])
    dec = cls["decoder"](nstyle=cfg["nstyle"], dropout_rate=cfg["dropout_rate"], last_layer_activation="Softplus",
                         dim_out=256, n_layers=cfg["n_layers"])
    dis = pm.DiscriminatorFC(nstyle=cfg["nstyle"], dropout_rate=cfg["dis_dropout_rate"], noise=cfg["dis_noise"], layers=3)
    return enc, dec, dis


@pytest.mark.parametrize("ae_form", ["FC", "compact"])
def test_engine_state_round_trip(ae_form):
    """``load_state(first.state())`` makes a differently seeded engine the first one, word for word: both then take the
    same two steps (the first has captured its graph by then, the second emits eagerly and captures)."""
    cfg = _cfg(ae_form)
    dev = torch.device("cuda:0")
    spec, aux = _data()
    engines = [StepEngine(*_modules(cfg, s), cfg, dev, rng_mode="philox", seed=100 + s) for s in (1, 2)]
    g = torch.Generator().manual_seed(3)
    perms = [torch.randperm(140, generator=g) for _ in range(2)]
    for e in engines:
        e.set_data(spec[:140], aux[:140])
    first, second = engines
    first.set_epoch(perms[0], 0.3)
    for _ in range(3):
        first.step(32)

    def words(e):
        torch.cuda.synchronize()
        return ([e.arena.P.cpu(), e.steps_dev.cpu(), e.rng_state.cpu(), e.loss_out.cpu(), e.nan_flags.cpu()] +
                [t.cpu() for o in e.opts.values() for t in (o.m, o.v, o.hyper)] +
                [b_.cpu() for mod in (e.enc_mod, e.dec_mod, e.dis_mod) for b_ in mod.buffers()])
    assert not torch.equal(first.arena.P.cpu(), second.arena.P.cpu())
    state = first.state()
    second.load_state(state)
    assert second.seed == first.seed and second.bn_counts and \
        list(second.bn_counts.values()) == [first.bn_counts[id(bn)] for bn in first.enc.bn_modules + first.dec.bn_modules]
    for e in engines:
        e.set_epoch(perms[1], 0.4)
        for _ in range(2):
            e.step(32)
    for a, b in zip(words(first), words(second)):
        assert a.shape == b.shape and torch.equal(a, b)
    assert int(first.steps_dev[0]) == 5
    with pytest.raises(AssertionError, match="load_state"):
        second.load_state(state)
    for e in engines:
        e.release()


@pytest.mark.parametrize("ae_form", ["FC", "compact"])
def test_defaults_write_nothing_and_checkpoints_do_not_perturb(ae_form, tmp_path):
    plain = _Trial(tmp_path / "plain", _cfg(ae_form, max_epoch=2), SEED[ae_form])
    m_plain = plain.trainer.train()
    assert [n for n in os.listdir(plain.wd) if n.startswith("resume")] == []
    want = plain.outcome(m_plain)
    ck = _Trial(tmp_path / "ck", _cfg(ae_form, max_epoch=2, checkpoint_every=1), SEED[ae_form])
    m_ck = ck.trainer.train()
    assert sorted(n for n in os.listdir(ck.wd) if n.startswith("resume")) == sorted([rf.NAME, rf.PREV_NAME])
    _assert_same_outcome(ck.outcome(m_ck), want)
