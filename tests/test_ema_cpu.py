"""``ema_decay`` / ``report_weights`` without a GPU: the keys' validation, the resume fingerprint, and the float64
reference of the moving average against a recurrence worked out by hand."""
import numpy as np
import pytest
import torch

import ema_reference
from rankaae_amd import resume
from rankaae_amd.parameter import Parameters, ema_decay_of, report_weights_of

BAD = [0, 1, -0.1, 1.5, float("nan"), float("inf"), "0.9", True]


def test_absent_null_and_numbers_inside_the_interval_are_accepted():
    assert ema_decay_of({}) is None and ema_decay_of({"ema_decay": None}) is None
    assert ema_decay_of({"ema_decay": 0.5}) == 0.5 and ema_decay_of({"ema_decay": 0.9999}) == 0.9999
    assert isinstance(ema_decay_of({"ema_decay": np.float64(0.5)}), float)


@pytest.mark.parametrize("bad", BAD)
def test_key_refuses_what_is_not_a_number_strictly_between_0_and_1(bad):
    with pytest.raises(ValueError, match="ema_decay"):
        ema_decay_of({"ema_decay": bad})


@pytest.mark.parametrize("bad", BAD)
def test_trainer_refuses_a_bad_key_before_the_gpu(bad, monkeypatch):
    """``Trainer.__init__`` raises on the key before it builds the engine: no GPU, no networks, no loaders; and
    ``from_data``, which would reach for the GPU, is never called."""
    from rankaae_amd.trainer import Trainer

    def no_gpu(*a, **kw):
        raise AssertionError("Trainer.from_data was called")
    monkeypatch.setattr(Trainer, "from_data", no_gpu)
    cfg = Parameters({"gradient_reversal": True, "use_cnn_discriminator": False, "optimizer_name": "AdamW",
                      "ema_decay": bad})
    with pytest.raises(ValueError, match="ema_decay"):
        Trainer(None, None, None, torch.device("cpu"), None, None, verbose=False, config_parameters=cfg)


@pytest.mark.parametrize("bad", [0, 1.5, "0.9"])
def test_engine_refuses_a_bad_key_before_the_gpu(bad):
    """``StepEngine`` checks the key first: the error comes also where there is no GPU to refuse with."""
    from rankaae_amd.engine import StepEngine
    with pytest.raises(ValueError, match="ema_decay"):
        StepEngine(None, None, None, {"ema_decay": bad}, torch.device("cpu"))


def test_resume_fingerprint_carries_the_key_only_when_set():
    spec = np.ones((4, 8), dtype=np.float32)
    fp = lambda cfg: resume.fingerprint(cfg, 1, 640, 4, 2, spec)       # noqa: E731
    base = {"ae_form": "FC", "nstyle": 2}
    assert "cfg.ema_decay" not in fp(base) and "cfg.ema_decay" not in fp(dict(base, ema_decay=None))
    assert fp(base) == fp(dict(base, ema_decay=None))
    assert fp(dict(base, ema_decay=0.9))["cfg.ema_decay"] == 0.9
    assert fp(dict(base, ema_decay=0.9)) != fp(dict(base, ema_decay=0.99))
    with pytest.raises(ValueError, match="cfg.ema_decay"):
        resume.check_fingerprint(fp(dict(base, ema_decay=0.9)), fp(dict(base, ema_decay=0.99)))
    with pytest.raises(ValueError, match="cfg.ema_decay"):
        resume.check_fingerprint(fp(base), fp(dict(base, ema_decay=0.9)))


def test_report_weights_is_final_or_ema():
    assert report_weights_of({}) == "final" and report_weights_of(Parameters({})) == "final"
    assert report_weights_of({"report_weights": "final"}) == "final"
    assert report_weights_of(Parameters({"report_weights": "ema"})) == "ema"
    for bad in ("EMA", "best", "", None, True, 1):
        with pytest.raises(ValueError, match="report_weights"):
            report_weights_of({"report_weights": bad})


def test_report_refuses_a_job_without_the_average(tmp_path):
    """``load_model(..., "ema")`` names the job directory that has no ``final_ema.pt``; an unknown kind is a ValueError."""
    from rankaae_amd import report
    job = tmp_path / "job_1"
    job.mkdir()
    torch.save({"x": 1}, job / "final.pt")
    assert report.load_model(str(tmp_path), "job_1") == {"x": 1}
    with pytest.raises(FileNotFoundError, match="job_1"):
        report.load_model(str(tmp_path), "job_1", "ema")
    with pytest.raises(ValueError, match="report_weights"):
        report.load_model(str(tmp_path), "job_1", "best")
    torch.save({"x": 2}, job / "final_ema.pt")
    assert report.load_model(str(tmp_path), "job_1", "ema") == {"x": 2}


def test_reference_is_the_hand_computed_recurrence():
    """decay 0.5, four numbers, three steps: every value below is exact in binary, worked out by hand.
    ema0 = [0, 1, -2, 4]; p1 = [2, 1, 2, 0] -> [1, 1, 0, 2]; p2 = [3, -1, 4, 2] -> [2, 0, 2, 2];
    p3 = [0, 0, -2, 1] -> [1, 0, 0, 1.5]."""
    ema0 = [0.0, 1.0, -2.0, 4.0]
    ps = [[2.0, 1.0, 2.0, 0.0], [3.0, -1.0, 4.0, 2.0], [0.0, 0.0, -2.0, 1.0]]
    want = [[1.0, 1.0, 0.0, 2.0], [2.0, 0.0, 2.0, 2.0], [1.0, 0.0, 0.0, 1.5]]
    got = ema_reference.ema_run(ema0, ps, 0.5)
    assert [g.tolist() for g in got] == want and all(g.dtype == torch.float64 for g in got)
    # another decay, one step, against the formula written out: 0.75 * 4 + 0.25 * 8 = 5
    assert ema_reference.ema_step([4.0], [8.0], 0.75).tolist() == [5.0]
    # NaN in p propagates, at its position only
    out = ema_reference.ema_step([1.0, 1.0], [float("nan"), 3.0], 0.5)
    assert bool(torch.isnan(out[0])) and out[1].item() == 2.0
    assert ema_reference.step_bound([-4.0], [1.0]).tolist() == [2.0 ** -20]
