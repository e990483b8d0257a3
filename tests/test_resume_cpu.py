"""Checkpoint / resume (config keys ``checkpoint_every`` / ``resume``): the host side -- key validation, the scheduler's
state, the fingerprint, the two-generation file protocol, the epoch a batched group resumes from, ``train_sc`` skipping
finished trials and the ``losses.csv`` clean-up.  No GPU."""
import logging
import os

import pytest
import torch

from rankaae_amd import resume as rf
from rankaae_amd.parameter import Parameters, checkpoint_every_of, resume_on
from rankaae_amd.trainer import AnomalyError, PlateauScheduler, Trainer

CFG = dict(gradient_reversal=True, use_cnn_discriminator=False, optimizer_name="AdamW", lr_base=0.001, ae_form="FC",
           nstyle=3, n_aux=2, dim_in=256, dim_out=256, n_layers=3, FC_discriminator_layers=3, batch_size=32,
           max_epoch=6, epoch_stop_smooth=3, alpha_flat_step=739, alpha_limit=0.7, dropout_rate=0.04,
           dis_dropout_rate=0.05, lr_ratio_Corr=10, lr_ratio_dis=1, weight_decay=0.01, dis_beta=1.1)


class _Opt:
    def __init__(self, lr):
        self.lr, self.pushed = lr, 0

    def push(self):
        self.pushed += 1


def test_plateau_scheduler_state_round_trip():
    seq = [5.0, 4.0, 4.5, 4.6, 3.0, 3.1, 3.2, 3.3, 2.0, 2.5, 2.6, 1.0]
    cut_at = 6
    twin_opt = _Opt(1.0)
    twin = PlateauScheduler(twin_opt, 0.5, 1)
    lrs = []
    for m in seq:
        twin.step(m)
        lrs.append(twin_opt.lr)
    assert any(a != b for a, b in zip([1.0] + lrs[:cut_at - 1], lrs[:cut_at])), "no cut before the save point"
    assert any(a != b for a, b in zip(lrs[cut_at - 1:], lrs[cut_at:])), "no cut after the save point"

    first_opt = _Opt(1.0)
    first = PlateauScheduler(first_opt, 0.5, 1)
    for m in seq[:cut_at]:
        first.step(m)
    saved = first.state_dict()
    assert all(isinstance(v, (int, float)) for v in saved.values())
    second_opt = _Opt(first_opt.lr)                     # (the lr itself travels with the engine's state)
    second = PlateauScheduler(second_opt, 0.9, 7)       # constructed differently: the loaded state decides
    second.load_state_dict(saved)
    assert second.state_dict() == saved
    got = []
    for m in seq[cut_at:]:
        second.step(m)
        got.append(second_opt.lr)
    assert got == lrs[cut_at:]
    assert second.state_dict() == twin.state_dict()


@pytest.mark.parametrize("key,value", [("checkpoint_every", -1), ("checkpoint_every", 2.0), ("checkpoint_every", "2"),
                                       ("checkpoint_every", True), ("resume", "true"), ("resume", "false"),
                                       ("resume", 1), ("resume", None)])
def test_bad_key_values_raise_and_name_the_key(key, value):
    with pytest.raises(ValueError, match=key):
        (checkpoint_every_of if key == "checkpoint_every" else resume_on)({key: value})
    with pytest.raises(ValueError, match=key):          # ... and Trainer refuses them before it touches anything
        Trainer(None, None, None, None, None, None, config_parameters=Parameters({**CFG, key: value}))


def test_key_defaults_and_good_values():
    assert checkpoint_every_of({}) == 0 and resume_on({}) is False
    assert checkpoint_every_of({"checkpoint_every": 25}) == 25 and resume_on({"resume": True}) is True
    assert checkpoint_every_of(Parameters({"checkpoint_every": 3})) == 3


@pytest.mark.parametrize("extra", [{"checkpoint_every": 2}, {"resume": True}])
def test_data_parallel_and_parity_mode_are_refused(extra, monkeypatch):
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(ValueError, match="checkpoint_every / resume: single-process runs only"):
        Trainer(None, None, None, None, None, None, config_parameters=Parameters({**CFG, **extra}))
    monkeypatch.setenv("WORLD_SIZE", "1")
    with pytest.raises(ValueError, match="checkpoint_every / resume: single-process runs only"):
        Trainer(None, None, None, None, None, None, config_parameters=Parameters({**CFG, **extra, "rng_mode": "host"}))


def test_fingerprint_mismatch_names_the_differing_entries():
    spec = torch.arange(12.0, dtype=torch.float64).reshape(3, 4).numpy()
    saved = rf.fingerprint(CFG, 1, 4096, 3, 1, spec)
    assert saved["spectra.sum"] == 66.0 and saved["spectra.sum_sq"] == 506.0 and saved["arena.n"] == 4096
    for k in ("cfg.alpha_limit", "cfg.lr_ratio_Corr", "cfg.dis_dropout_rate", "cfg.precision", "cfg.trial_seed"):
        assert k in saved
    rf.check_fingerprint(saved, rf.fingerprint(dict(CFG), 1, 4096, 3, 1, spec.copy()))       # equal: nothing raised
    spec2 = spec.copy()
    spec2[0, 0] = 1.0
    now = rf.fingerprint({**CFG, "nstyle": 4, "lr_ratio_Corr": 5, "trial_seed": 7}, 4, 4096, 3, 1, spec2)
    with pytest.raises(ValueError) as err:
        rf.check_fingerprint(saved, now)
    msg = str(err.value)
    for k in ("cfg.nstyle", "cfg.lr_ratio_Corr", "cfg.trial_seed", "tile_rows_mult", "spectra.sum", "spectra.sum_sq"):
        assert k in msg
    for k in ("cfg.batch_size", "arena.n", "rows.train", "cfg.alpha_limit"):
        assert k not in msg


def _state(epoch, **kw):
    return {"version": rf.FORMAT_VERSION, "finished": False, "error": None, "epoch": epoch, "metrics": [0.5, 1.0 * epoch],
            "checkpoint_every": 2, "tail_pending": False,
            "payload": torch.full((4,), float(epoch)), **kw}


def test_two_generations_survive_a_failure_between_the_replaces(tmp_path, monkeypatch):
    wd = str(tmp_path)
    rf.write_resume(wd, _state(1))
    assert sorted(os.listdir(wd)) == [rf.NAME]
    rf.write_resume(wd, _state(3))
    assert sorted(os.listdir(wd)) == sorted([rf.NAME, rf.PREV_NAME])
    assert [int(s["epoch"]) for _, s in rf.generations(wd)] == [3, 1]
    assert rf.offered_epochs(wd) == [3, 1]

    real, calls = os.replace, []

    def failing(src, dst):
        calls.append((os.path.basename(src), os.path.basename(dst)))
        if len(calls) == 2:
            raise OSError("killed between the two replaces")
        return real(src, dst)
    monkeypatch.setattr(rf.os, "replace", failing)
    with pytest.raises(OSError):
        rf.write_resume(wd, _state(5))
    monkeypatch.setattr(rf.os, "replace", real)
    assert calls == [(rf.NAME, rf.PREV_NAME), (rf.TMP_NAME, rf.NAME)]
    assert not os.path.exists(os.path.join(wd, rf.NAME))
    gens = rf.generations(wd)                           # a complete file remains: the one that was current
    assert [int(s["epoch"]) for _, s in gens] == [3]
    assert torch.equal(gens[0][1]["payload"], torch.full((4,), 3.0))
    # a kill in the middle of torch.save leaves a cut-short tmp file and both generations untouched
    with open(os.path.join(wd, rf.TMP_NAME), "wb") as f:
        f.write(b"PK\x03\x04 cut short")
    assert rf.load_resume(os.path.join(wd, rf.TMP_NAME)) is None
    rf.write_resume(wd, _state(7))
    assert [int(s["epoch"]) for _, s in rf.generations(wd)] == [7, 3]   # (resume.pt was missing: prev stays what it was)


def test_resume_file_loads_with_weights_only_and_rejects_other_versions(tmp_path):
    rf.write_resume(str(tmp_path), _state(2))
    st = torch.load(tmp_path / rf.NAME, weights_only=True)
    assert st["epoch"] == 2 and st["metrics"] == [0.5, 2.0]
    torch.save({**_state(4), "version": rf.FORMAT_VERSION + 1}, tmp_path / rf.NAME)
    assert rf.load_resume(str(tmp_path / rf.NAME)) is None


def test_group_epoch_is_the_greatest_common_one():
    assert rf.choose_group_epoch([[5, 3], [5, 3], [5, 3]]) == 5
    assert rf.choose_group_epoch([[5, 3], [3, 1]]) == 3                 # one member is a generation behind
    assert rf.choose_group_epoch([[7, 5], [5, 3], [7, 5]]) == 5
    assert rf.choose_group_epoch([[1, rf.FRESH], [rf.FRESH]]) == rf.FRESH      # killed between the first writes
    assert rf.choose_group_epoch([[9, 7]]) == 9
    with pytest.raises(ValueError, match="no common epoch"):
        rf.choose_group_epoch([[5, 3], [9, 7]])
    with pytest.raises(ValueError, match="no common epoch"):
        rf.choose_group_epoch([[5, 3], [rf.FRESH]])                       # someone deleted a trial's files


def test_offered_epochs(tmp_path):
    wd = str(tmp_path)
    assert rf.offered_epochs(wd) == [rf.FRESH]
    rf.write_resume(wd, _state(1))
    assert rf.offered_epochs(wd) == [1, rf.FRESH]
    rf.write_resume(wd, _state(3))
    assert rf.offered_epochs(wd) == [3, 1]
    assert rf.finished_state(wd) is None
    rf.write_resume(wd, _state(5, finished=True))
    assert rf.finished_state(wd)["epoch"] == 5


def test_a_single_file_offers_a_fresh_start_only_if_it_is_the_first_a_run_writes(tmp_path):
    for name, state, want in (("first", _state(1), [1, rf.FRESH]), ("later", _state(5), [5]),
                              ("stop_before_first", _state(0, tail_pending=True), [0, rf.FRESH]),
                              ("stop_later", _state(4, tail_pending=True), [4])):
        wd = tmp_path / name
        wd.mkdir()
        rf.write_resume(str(wd), state)
        assert rf.offered_epochs(str(wd)) == want, name
    # a trial that lost all its files beside one that is well into its run: an error, not a restart
    with pytest.raises(ValueError, match="no common epoch"):
        rf.choose_group_epoch([rf.offered_epochs(str(tmp_path / "absent")), rf.offered_epochs(str(tmp_path / "later"))])


def test_drop_newer_leaves_the_chosen_generation_as_the_current_file(tmp_path):
    wd = str(tmp_path)
    rf.write_resume(wd, _state(1))
    rf.write_resume(wd, _state(3))
    rf.drop_newer(wd, 3)
    assert [int(s["epoch"]) for _, s in rf.generations(wd)] == [3, 1]
    rf.drop_newer(wd, 1)                    # the group resumes from the older epoch: the newer file goes
    assert sorted(os.listdir(wd)) == [rf.NAME] and rf.load_resume(os.path.join(wd, rf.NAME))["epoch"] == 1
    rf.write_resume(wd, _state(3))          # the next write point: two generations again, two epochs
    assert rf.offered_epochs(wd) == [3, 1]
    rf.drop_newer(wd, rf.FRESH)
    assert os.listdir(wd) == []


def test_train_sc_skips_a_finished_trial_without_building_it(tmp_path, monkeypatch):
    from rankaae_amd.cmd import train_sc

    def refuse(*a, **kw):
        raise AssertionError("a finished trial was constructed again")
    monkeypatch.setattr(Trainer, "from_data", classmethod(refuse))
    main_log = logging.getLogger("Main training:")
    for h in list(main_log.handlers):
        main_log.removeHandler(h)
    job1, job2 = tmp_path / "training" / "job_1", tmp_path / "training" / "job_2"
    job1.mkdir(parents=True)
    job2.mkdir(parents=True)
    metrics = [0.91, 0.02, 0.3, 0.11, 0.45]
    rf.write_resume(str(job1), _state(3))
    rf.write_resume(str(job1), {**_state(5, finished=True), "metrics": metrics})
    rf.write_resume(str(job2), {**_state(2, finished=True, error=["correlation", 17, 2]), "metrics": None})
    cfg = Parameters({**CFG, "resume": True, "checkpoint_every": 2, "trial_seed": 3})
    try:
        got, time_used = train_sc.run_training(0, str(tmp_path), cfg, False, None)
        assert got == metrics and time_used == 0.0
        err, time_used = train_sc.run_training(1, str(tmp_path), cfg, False, None)
        assert isinstance(err, AnomalyError) and (err.phase, err.step, err.epoch) == ("correlation", 17, 2)
        assert time_used == 0.0
        assert train_sc.diverged_trials([(got, 0.0), (err, 0.0)]) == [2]
    finally:
        for h in list(main_log.handlers):
            h.close()
            main_log.removeHandler(h)
    lines = (tmp_path / "main_process_message.txt").read_text().splitlines()
    assert len(lines) == 2 and "Trial 1 finished" in lines[0] and "Trial 2 diverged" in lines[1]
    # without `resume` the trial is built as always
    with pytest.raises(AssertionError, match="constructed again"):
        train_sc.run_training(0, str(tmp_path), Parameters({**CFG, "checkpoint_every": 2}), False, None)


def test_resumed_multi_trial_run_needs_trial_seed(tmp_path):
    from rankaae_amd.cmd import train_sc
    with pytest.raises(ValueError, match="trial_seed"):
        train_sc.run_trials(2, str(tmp_path), Parameters({**CFG, "resume": True}), False, None, 0, None)


def test_losses_csv_truncation(tmp_path):
    path = tmp_path / "losses.csv"
    header = "Epoch,Train_D,Val_D\n"
    rows = [f"{e:d},\t{0.1 * e:.6f},\t{0.2 * e:.6f},\t\n" for e in (0, 10, 20, 30)]
    path.write_text(header + "".join(rows) + "40,\t0.5")            # the last row cut short by the kill
    handler = logging.FileHandler(path)                              # an open append-mode handler, as train_sc has
    handler.setFormatter(logging.Formatter("%(message)s"))
    log = logging.getLogger("losses_truncation_test")
    log.setLevel(logging.DEBUG)
    log.addHandler(handler)
    try:
        rf.truncate_losses_csv(str(path), 25)
        assert path.read_text() == header + "".join(rows[:3])
        log.info("30,\tagain")                                       # appended behind the kept rows
        assert path.read_text() == header + "".join(rows[:3]) + "30,\tagain\n"
        rf.truncate_losses_csv(str(path), 20)
        assert path.read_text() == header + "".join(rows[:3])
        rf.truncate_losses_csv(str(path), 9)
        assert path.read_text() == header + rows[0]
        rf.truncate_losses_csv(str(path), rf.FRESH)
        assert path.read_text() == ""
    finally:
        log.removeHandler(handler)
        handler.close()
    rf.truncate_losses_csv(str(tmp_path / "absent.csv"), 3)          # no file: nothing to do
    assert not (tmp_path / "absent.csv").exists()
