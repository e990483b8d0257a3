"""``detect_anomaly`` without a GPU: the config key, the exceptions, and what ``train_sc`` does with a trial that
raises ``AnomalyError`` (a stubbed trainer stands in for the GPU run)."""
import logging
import os
import pickle
import types

import pytest
import yaml

from rankaae_amd.parameter import Parameters, detect_anomaly_on
from rankaae_amd.trainer import AnomalyError, TrialsDiverged


def test_detect_anomaly_key_defaults_on():
    assert detect_anomaly_on({}) is True
    assert detect_anomaly_on(Parameters({"detect_anomaly": False})) is False
    assert detect_anomaly_on(Parameters({"detect_anomaly": True})) is True
    for bad in ("yes", 1, None):
        with pytest.raises(ValueError, match="detect_anomaly"):
            detect_anomaly_on({"detect_anomaly": bad})


def test_detect_anomaly_key_from_yaml(tmp_path):
    (tmp_path / "c.yaml").write_text("detect_anomaly: false\nlr_base: 0.001\n")
    assert detect_anomaly_on(Parameters.from_yaml(str(tmp_path / "c.yaml"))) is False


def test_anomaly_error_is_the_reference_runtime_error():
    e = AnomalyError("reconstruction", 17, 2)
    assert isinstance(e, RuntimeError)
    assert "returned nan values" in str(e)
    assert "reconstruction" in str(e) and "step 17" in str(e) and "epoch 2" in str(e)
    back = pickle.loads(pickle.dumps(e))          # crosses train_sc's worker processes
    assert isinstance(back, AnomalyError) and (back.phase, back.step, back.epoch) == ("reconstruction", 17, 2)
    assert str(back) == str(e)
    d = TrialsDiverged([[1.0] * 5, None], [None, e])
    assert isinstance(d, RuntimeError) and d.errors[1] is e and d.results[0] == [1.0] * 5 and "[1]" in str(d)


class _StubTrainer:
    """``Trainer.from_data`` / ``train()`` of ``train_sc.run_training`` without a GPU: the trial whose work_dir ends
    in ``job_2`` raises ``AnomalyError``; the others write a final.pt and return metrics."""

    @classmethod
    def from_data(cls, csv_fn, work_dir=".", **kw):
        t = cls()
        t.work_dir = work_dir
        t.engine = types.SimpleNamespace(release=lambda: None)
        return t

    def train(self):
        if self.work_dir.endswith("job_2"):
            raise AnomalyError("mutual_info", 7, 0)
        open(os.path.join(self.work_dir, "final.pt"), "w").close()
        return [0.5, 0.1, 0.2, 0.3, 0.4]


def test_train_sc_logs_the_diverged_trial_and_exits_nonzero(tmp_path, monkeypatch):
    from rankaae_amd.cmd import train_sc
    cfg = {"trials": 3, "trial_mode": "processes", "data_file": "data.csv", "timeout": 1, "verbose": False}
    (tmp_path / "cfg.yaml").write_text(yaml.safe_dump(cfg))
    (tmp_path / "data.csv").write_text("")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "RANKAAE_TRIAL_WORKERS", "RANKAAE_TRIALS_PER_GPU"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setattr(train_sc, "Trainer", _StubTrainer)
    monkeypatch.setattr("sys.argv", ["train_sc", "-c", "cfg.yaml", "-w", str(tmp_path)])
    try:
        with pytest.raises(SystemExit) as ei:
            train_sc.main()
    finally:
        for name in ["Main training:"] + [f"{p}_{k}" for p in ("subtraining", "losses") for k in (1, 2, 3)]:
            lg = logging.getLogger(name)
            for h in list(lg.handlers):
                h.close()
                lg.removeHandler(h)
    assert ei.value.code not in (0, None)
    assert "Trials [2] diverged" in str(ei.value.code)
    jobs = tmp_path / "training"
    bad = (jobs / "job_2" / "messages.txt").read_text()
    assert "AnomalyError" in bad and "returned nan values" in bad and "Training finished" not in bad
    assert not (jobs / "job_2" / "final.pt").exists()
    for k in (1, 3):          # the trials after the diverged one still ran
        assert "Training finished" in (jobs / f"job_{k}" / "messages.txt").read_text()
        assert (jobs / f"job_{k}" / "final.pt").exists()
    main_log = (tmp_path / "main_process_message.txt").read_text()
    assert "Trials [2] diverged" in main_log and "START" in main_log


def test_diverged_trials_reads_the_results():
    from rankaae_amd.cmd.train_sc import diverged_trials
    ok = ([0.1] * 5, 1.0)
    assert diverged_trials([ok, ok]) == []
    assert diverged_trials([ok, (AnomalyError("adversarial", 1, 0), 2.0), ok]) == [2]
