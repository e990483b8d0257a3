"""``detect_anomaly`` on the GPU: NaN gradients are found by the optimizer kernels and stop the trial, as the
reference's ``torch.autograd.set_detect_anomaly(True)`` does.

kernels  ``raae_optim_step_chk`` (``ops.optim_step(..., nan_step=)``), every rule in both kernel shapes, alone and in
         the batched form: the flag holds the first step that saw a NaN, Inf and skipped slabs are not flagged, and
         p / m / v are bit for bit those of ``raae_optim_step``.
engine   a NaN written into one phase's gradient slab at a chosen step of a captured, replayed run: ``anomaly()``
         names that phase and step.
trainer  a NaN in one training spectrum: ``AnomalyError`` in epoch 0, nothing of the epoch written; off, the run
         completes.  Finite runs are bitwise the same with the check on and off.
trials   batched trials (one diverges, the others are bitwise the trials batched without it), two data-parallel ranks,
         and ``train_sc`` in batched and threads mode.
"""
import ctypes as C
import json
import logging
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from rankaae_amd.synthetic import make_spectra, write_csv

if torch.cuda.is_available():
    import test_engine_gpu as p2
    from oracle import ref_train
    from rankaae_amd import _lib, ops
    from rankaae_amd.parameter import Parameters
    from rankaae_amd.trainer import AnomalyError, Trainer, TrialsDiverged, train_trials_batched
    DEV = torch.device("cuda:0")
    RULES = {"Adam": _lib.OPT_ADAM, "AdamW": _lib.OPT_ADAMW, "RAdam": _lib.OPT_RADAM, "AdaBound": _lib.OPT_ADABOUND}

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = float("nan")


def _bits(t):
    return t.detach().contiguous().view(torch.int32).cpu()


def _golden(case):
    with open(os.path.join(ROOT, "tests", "golden", f"ref_{case}.json")) as f:
        return json.load(f)


def _quiet():
    lg = logging.getLogger("anomaly_quiet")
    if not lg.handlers:
        lg.addHandler(logging.NullHandler())
    lg.propagate = False
    return lg


# ---------------------------------------------------------------------------------------------------- kernels
class _Problem:
    """One update range: 24 segments of 64 elements, segment 5 without slabs, the others with 1 .. max_nslab slabs
    (segment 0 with max_nslab); a fresh set of gradient slabs per step with the planted values of ``plant``."""

    def __init__(self, max_nslab, seed):
        g = torch.Generator().manual_seed(seed)
        self.g, self.S, self.n = g, max_nslab, 64 * 24
        counts = torch.randint(1, max_nslab + 1, (24,), generator=g)
        counts[0], counts[5], counts[7] = max_nslab, 0, 1
        self.counts = counts
        self.seg = counts.to(torch.int16).to(DEV)
        self.p0 = torch.randn(self.n, generator=g)

    def slabs(self, step, poison):
        s = torch.randn(self.S, self.n, generator=self.g)
        if poison:
            if step == 1:
                s[0, 64 * 1 + 9] = float("inf")        # Inf: not flagged (its NaN reaches the gradient next step)
                s[0, 64 * 5 + 2] = NAN                 # a segment without slabs: skipped
                s[1, 64 * 7 + 4] = NAN                 # slab 1 of a one-slab segment: not part of the gradient
            if step == 3:
                s[min(2, int(self.counts[11]) - 1), 64 * 11 + 33] = NAN
            if step == 5:                              # a later NaN: the first step stays
                s[0, 64 * 20 + 1] = NAN
        return s.to(DEV)


def _hyper():
    return torch.tensor([0.01, 0.9, 0.999, 1e-8, 0.01, 0.01, 0.1, 1e-3], dtype=torch.float64, device=DEV)


def _state(p0):
    return [p0.to(DEV), torch.zeros_like(p0, device=DEV), torch.zeros_like(p0, device=DEV)]


@pytest.mark.parametrize("max_nslab", [16, 40])
@pytest.mark.parametrize("name", ["Adam", "AdamW", "RAdam", "AdaBound"])
def test_checked_update_flags_the_first_nan_step(name, max_nslab):
    """Six steps of the checked and the unchecked update on the same gradients (one thread per element at
    max_nslab 16, eight lanes per element at 40): the flag is 0 through steps 1-2 (an Inf, a NaN in a segment without
    slabs, a NaN in a slab beyond the segment's count), 3 from the NaN of step 3 on, also after step 5's NaN; p, m, v
    are bitwise equal after every step -- NaN bit patterns included."""
    pr = _Problem(max_nslab, seed=3)
    hyper, step = _hyper(), torch.zeros(1, dtype=torch.int32, device=DEV)
    plain, chk = _state(pr.p0), _state(pr.p0)
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    for t in range(1, 7):
        slabs = pr.slabs(t, poison=True)
        step.add_(1)
        ops.optim_step(*plain, slabs, pr.n, pr.seg, pr.n, RULES[name], hyper, step, max_nslab)
        ops.optim_step(*chk, slabs, pr.n, pr.seg, pr.n, RULES[name], hyper, step, max_nslab, nan_step=flag)
        torch.cuda.synchronize()
        assert int(flag) == (0 if t < 3 else 3), (name, max_nslab, t, int(flag))
        for a, b, what in zip(plain, chk, "pmv"):
            assert torch.equal(_bits(a), _bits(b)), f"{name} max_nslab {max_nslab} step {t}: {what} differs"
    assert not torch.isfinite(chk[0].cpu()).all(), "the planted values did reach the update"


@pytest.mark.parametrize("max_nslab", [16, 40])
@pytest.mark.parametrize("name", ["Adam", "AdamW", "RAdam", "AdaBound"])
def test_checked_update_batched_form(name, max_nslab):
    """The checked ``_m`` forms through the recorder (raae_record_* / raae_multi_*, gridDim.z = 2): each trial's
    argument block carries its own flag word.  Trial 1 gets the planted NaNs, trial 0 finite gradients: flags 0 and
    3, and both trials bitwise the unchecked single-trial update."""
    lib = _lib.load()
    probs = [_Problem(max_nslab, seed=10), _Problem(max_nslab, seed=10)]
    hyper = _hyper()
    steps = [torch.zeros(1, dtype=torch.int32, device=DEV) for _ in range(2)]
    plain = [_state(pr.p0) for pr in probs]
    chk = [_state(pr.p0) for pr in probs]
    flags = [torch.zeros(1, dtype=torch.int32, device=DEV) for _ in range(2)]
    slab_bufs = [torch.zeros(max_nslab, probs[0].n, device=DEV) for _ in range(2)]
    # the program: one recorded launch per trial (the recording also runs it: the buffers are restored after)
    saved = [[t.clone() for t in chk[i] + [flags[i]]] for i in range(2)]
    handles = (C.c_void_p * 2)()
    for i in range(2):
        assert lib.raae_record_begin() == 0
        ops.optim_step(*chk[i], slab_bufs[i], probs[i].n, probs[i].seg, probs[i].n, RULES[name], hyper, steps[i],
                       max_nslab, nan_step=flags[i])
        h, cnt = C.c_void_p(), C.c_int(0)
        assert lib.raae_record_end(C.byref(h), C.byref(cnt)) == 0 and cnt.value == 1
        handles[i] = h.value
    prog = C.c_void_p()
    rc = lib.raae_multi_build(handles, 2, C.byref(prog))
    for h in handles:
        lib.raae_record_free(C.c_void_p(h))
    assert rc == 0
    try:
        for i in range(2):
            for dst, src in zip(chk[i] + [flags[i]], saved[i]):
                dst.copy_(src)
        for t in range(1, 7):
            for i in range(2):
                slab_bufs[i].copy_(probs[i].slabs(t, poison=(i == 1)))
                steps[i].add_(1)
                ops.optim_step(*plain[i], slab_bufs[i], probs[i].n, probs[i].seg, probs[i].n, RULES[name], hyper,
                               steps[i], max_nslab)
            assert lib.raae_multi_launch(prog, C.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0
            torch.cuda.synchronize()
            assert int(flags[0]) == 0 and int(flags[1]) == (0 if t < 3 else 3), (t, flags)
            for i in range(2):
                for a, b, what in zip(plain[i], chk[i], "pmv"):
                    assert torch.equal(_bits(a), _bits(b)), f"{name} {max_nslab} trial {i} step {t}: {what} differs"
    finally:
        lib.raae_multi_free(prog)


def test_checked_update_rejects_a_missing_flag():
    t = torch.zeros(64, device=DEV)
    rc = _lib.load().raae_optim_step_chk(t.data_ptr(), t.data_ptr(), t.data_ptr(), t.data_ptr(), 64,
                                         torch.ones(1, dtype=torch.int16, device=DEV).data_ptr(), 64, _lib.OPT_ADAM,
                                         _hyper().data_ptr(), torch.ones(1, dtype=torch.int32, device=DEV).data_ptr(),
                                         1, None, None)
    assert rc == -1


# ---------------------------------------------------------------------------------------------------- engine
@pytest.mark.parametrize("case,target,at", [("fc_small", "correlation", 5), ("compact_small", "smoothness", 3)])
def test_engine_anomaly_names_the_phase_and_step(case, target, at):
    """A NaN written into the gradient slab of ``target`` before its update of step ``at`` -- a replay of the captured
    step (step 1 eager, step 2 captured).  The later phases of that step and of the next ones see NaN too: ``anomaly()``
    answers the earliest step, and the first phase of that step."""
    g, cfg, spec, aux = p2.load_case(case)
    eng = p2.build_engine(dict(cfg), g["model_seed"], spec, aux, use_graph=True, rng_mode="philox")
    assert eng.detect_anomaly
    calls = {}

    def hook(name, P):
        calls[name] = calls.get(name, 0) + 1
        if name == target and calls[name] == at:
            o = eng.opts[name]
            seg = P.seg[name][o.lo // 64:o.hi // 64].cpu()
            j = int(torch.nonzero(seg > 0)[0]) * 64 + 5
            eng.G[0, o.lo + j] = NAN
    eng.phase_hook = hook
    n_train = ref_train.split_rows(len(spec))[0]
    b = cfg["batch_size"]
    eng.set_epoch(torch.randperm(n_train, generator=torch.Generator().manual_seed(4)), 0.3)
    for s in range(1, 8):
        eng.step(b)
        if s == at - 1:
            eng.losses()
            assert eng.anomaly() is None
    assert isinstance(eng.plans[b].graphs[True], list), "steps 2-7 ran as replays of the captured step"
    eng.losses()
    assert eng.anomaly() == (target, at)
    flags = eng.nan_flags.tolist()
    assert flags[["adversarial", "correlation", "reconstruction", "mutual_info", "smoothness"].index(target)] == at


# ---------------------------------------------------------------------------------------------------- trainer
def _trainer(case, wd, arrays, seed_model, **over):
    g = _golden(case)
    cfg = dict(g["config"], rng_mode="philox", seed=5, max_epoch=2)
    cfg.update(over)
    torch.manual_seed(seed_model)
    return Trainer.from_data(None, igpu=0, verbose=False, work_dir=str(wd), config_parameters=Parameters(cfg),
                             logger=_quiet(), loss_logger=_quiet(), arrays=arrays)


def _poisoned(case):
    g = _golden(case)
    spec, aux, _ = make_spectra(g["n_rows"], g["n_points"], g["config"]["n_aux"], seed=g["data_seed"])
    bad = spec.copy()
    bad[3, 100] = np.nan          # a training row: the split is contiguous, the first 70 % train
    return g, (spec, aux), (bad, aux)


@pytest.mark.parametrize("case", ["fc_small", "compact_small"])
def test_trainer_raises_on_a_nan_spectrum(case, tmp_path):
    from rankaae_amd.logger import create_logger
    g, _, bad = _poisoned(case)
    wd = tmp_path / "on"
    wd.mkdir()
    log = create_logger(f"anomaly_losses_{case}", str(wd / "losses.csv"), simple_fmt=True)
    try:
        torch.manual_seed(g["model_seed"])
        cfg = dict(g["config"], rng_mode="philox", seed=5, max_epoch=2)
        tr = Trainer.from_data(None, igpu=0, verbose=False, work_dir=str(wd), config_parameters=Parameters(cfg),
                               logger=_quiet(), loss_logger=log, arrays=bad)
        with pytest.raises(AnomalyError, match="returned nan values") as ei:
            tr.train()
    finally:
        for h in list(log.handlers):
            h.close()
            log.removeHandler(h)
    assert ei.value.epoch == 0 and ei.value.phase is not None and ei.value.step >= 1
    assert isinstance(ei.value, RuntimeError)
    assert not (wd / "final.pt").exists() and not (wd / "best.pt").exists()
    assert not list((wd / "checkpoints").glob("*.pt"))
    rows = (wd / "losses.csv").read_text().splitlines()
    assert len(rows) == 1 and rows[0].startswith("Epoch,Train_D"), rows
    # the same run with the check off trains to the end, as before the check existed
    off = tmp_path / "off"
    off.mkdir()
    tr = _trainer(case, off, bad, g["model_seed"], detect_anomaly=False)
    assert not tr.engine.detect_anomaly
    tr.train()
    assert (off / "final.pt").exists()


@pytest.mark.parametrize("case,name,use_graph", [("fc_small", "AdamW", True), ("fc_small", "AdamW", False),
                                                 ("compact_small", "RAdam", True), ("compact_small", "AdaBound", False)])
def test_finite_runs_are_unchanged_by_the_check(case, name, use_graph, tmp_path):
    """Two epochs with the check on and off: weights, optimizer moments, BatchNorm statistics and metrics bitwise
    equal (eager emission and graph replay)."""
    g, good, _ = _poisoned(case)
    out = []
    for detect in (True, False):
        wd = tmp_path / str(detect)
        wd.mkdir()
        tr = _trainer(case, wd, good, g["model_seed"], optimizer_name=name, use_graph=use_graph, detect_anomaly=detect)
        metrics = tr.train()
        e = tr.engine
        torch.cuda.synchronize()
        out.append(([e.arena.P.cpu()] + [t.cpu() for o in e.opts.values() for t in (o.m, o.v)] +
                    [b_.cpu() for mod in (e.enc_mod, e.dec_mod) for b_ in mod.buffers()], metrics, e.losses()))
        assert e.anomaly() is None and e.nan_flags.tolist() == [0] * 5
    for a, b in zip(out[0][0], out[1][0]):
        assert torch.equal(a, b)
    assert out[0][1] == out[1][1] and out[0][2] == out[1][2]


# ---------------------------------------------------------------------------------------------------- trials
@pytest.mark.parametrize("case", ["fc_small", "compact_small"])
def test_batched_trials_one_diverges(case, tmp_path):
    """Four trials in lockstep (``train_trials_batched``), trial 1 with a NaN training spectrum: it reports
    ``AnomalyError``; trials 0, 2, 3 finish with bitwise the weights and metrics of the same three trials batched
    without it, and write their files."""
    g, good, bad = _poisoned(case)
    cfg = dict(g["config"], rng_mode="philox", max_epoch=2)

    def make(ks, poisoned, tag):
        stream = torch.cuda.Stream(device=DEV)
        trs = []
        for k in ks:
            gen = torch.Generator().manual_seed(300 + k)
            torch.manual_seed(gen.initial_seed())
            wd = tmp_path / f"{tag}_{k}"
            wd.mkdir()
            trs.append(Trainer.from_data(None, igpu=0, verbose=False, work_dir=str(wd), config_parameters=Parameters(cfg),
                                         logger=_quiet(), loss_logger=_quiet(), arrays=bad if k == poisoned else good,
                                         host_rng=gen, engine_stream=stream))
        return trs
    four = make([0, 1, 2, 3], 1, "four")
    with pytest.raises(TrialsDiverged) as ei:
        train_trials_batched(four)
    res, err = ei.value.results, ei.value.errors
    assert isinstance(err[1], AnomalyError) and err[1].epoch == 0 and res[1] is None
    assert all(err[i] is None and len(res[i]) == 5 for i in (0, 2, 3)), (res, err)
    assert not (tmp_path / "four_1" / "final.pt").exists()
    assert all((tmp_path / f"four_{k}" / "final.pt").exists() for k in (0, 2, 3))
    three = make([0, 2, 3], None, "three")
    res3 = train_trials_batched(three)
    torch.cuda.synchronize()
    for j, i in enumerate((0, 2, 3)):
        assert torch.equal(four[i].engine.arena.P.cpu(), three[j].engine.arena.P.cpu()), f"trial {i}"
        assert res[i] == res3[j]


def _free_port():
    import socket
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        return sk.getsockname()[1]


def _dp_nan_worker(rank, world, port, work_dir, case):
    import time
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK="0", RANKAAE_DP_BACKEND="gloo")
    import torch.distributed as dist
    import test_engine_gpu as T
    from rankaae_amd.parameter import Parameters
    from rankaae_amd.trainer import AnomalyError, Trainer
    g, cfg, spec, aux = T.load_case(case)
    cfg = dict(cfg, max_epoch=20, batch_size=32, seed=5)
    spec = spec.copy()
    spec[3, 100] = np.nan        # the same data on both ranks: row 3 lands in one rank's shard of its global batch
    torch.manual_seed(g["model_seed"])

    class Log:
        def info(self, msg):
            pass
    tr = Trainer.from_data(None, igpu=0, verbose=False, work_dir=os.path.join(work_dir, str(rank)),
                           config_parameters=Parameters(cfg), logger=Log(), loss_logger=Log(), arrays=(spec, aux))
    t0 = time.time()
    try:
        tr.train()
        raised = None
    except AnomalyError as e:
        raised = (e.phase, e.step, e.epoch)
    elapsed = time.time() - t0
    box = [None] * world
    dist.all_gather_object(box, raised)
    assert box[0] is not None and box[0] == box[1], box
    assert box[0][2] < 20 and elapsed < 120, (box, elapsed)
    assert tr.engine.graph_ar is None
    dist.barrier()
    dist.destroy_process_group()


def test_data_parallel_ranks_raise_together(tmp_path):
    """Two gloo ranks on the one GPU, a NaN spectrum in the training split: the all-reduced gradient carries it to both
    ranks, and both raise ``AnomalyError`` with the same phase, step and epoch (none is left in a collective)."""
    import torch.multiprocessing as mp
    mp.spawn(_dp_nan_worker, args=(2, _free_port(), str(tmp_path), "fc_small"), nprocs=2, join=True)


_RUNNER = '''
import sys
import torch
from rankaae_amd.cmd import train_sc
from rankaae_amd.trainer import Trainer

_from_data = Trainer.from_data.__func__


def from_data(cls, *a, **kw):
    """trial 2 trains on a NaN spectrum (the engine's resident copy of its training split)"""
    tr = _from_data(cls, *a, **kw)
    if str(kw.get("work_dir", "")).endswith("job_2"):
        torch.cuda.synchronize()
        tr.engine.train_spec[3, 100] = float("nan")
        torch.cuda.synchronize()
    return tr


Trainer.from_data = classmethod(from_data)
sys.argv = ["train_sc"] + sys.argv[1:]
train_sc.main()
'''


@pytest.mark.parametrize("mode", ["batched", "threads"])
def test_train_sc_reports_the_diverged_trial(mode, tmp_path):
    """``train_sc`` with three trials, trial 2 on a NaN spectrum: trial 2's messages.txt holds the error and no
    "Training finished", trials 1 and 3 finish and write final.pt, main_process_message.txt names trial 2, and the
    command exits non-zero."""
    import yaml
    g = _golden("fc_small")
    spec, aux, grid = make_spectra(g["n_rows"], g["n_points"], g["config"]["n_aux"], seed=g["data_seed"])
    cfg = dict(g["config"])
    cfg.update(max_epoch=2, data_file="data.csv", verbose=False, timeout=1, trial_mode=mode, trials=3,
               trials_per_gpu=3, trial_seed=40)
    write_csv(str(tmp_path / "data.csv"), spec, aux, grid)
    with open(tmp_path / "cfg.yaml", "w") as f:
        yaml.safe_dump(cfg, f)
    (tmp_path / "runner.py").write_text(_RUNNER)
    env = dict(os.environ, PYTHONPATH=ROOT)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "RANKAAE_TRIAL_WORKERS", "RANKAAE_TRIALS_PER_GPU"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, str(tmp_path / "runner.py"), "-c", "cfg.yaml", "-w", str(tmp_path)],
                       env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode != 0, r.stderr[-3000:]
    assert "Trials [2] diverged" in r.stderr, r.stderr[-3000:]
    msg = (tmp_path / "training" / "job_2" / "messages.txt").read_text()
    assert "AnomalyError" in msg and "returned nan values" in msg and "Training finished" not in msg, msg
    assert not (tmp_path / "training" / "job_2" / "final.pt").exists()
    for k in (1, 3):
        job = tmp_path / "training" / f"job_{k}"
        assert "Training finished" in (job / "messages.txt").read_text()
        assert (job / "final.pt").exists()
    main_log = (tmp_path / "main_process_message.txt").read_text()
    assert "Trials [2] diverged" in main_log, main_log
