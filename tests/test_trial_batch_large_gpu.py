"""Batched trials of the conv networks at 1024 rows and up (``rankaae_amd.trial_batch.TrialBatch``).

From ``RAAE_BIG_ROWS`` (1024) rows the fused block kernels run their large-batch (``BIG``) instances; each has a
batched form ``KERNEL_m<KIND, true>`` that runs the same body with one trial per grid plane.  So a batched trial at
these sizes is bit for bit the trial stepped alone, and ``train_sc``'s batched mode (``tile_rows_mult: 1`` from 1024
rows) is bit for bit its thread mode."""
import json
import os
import re

import pytest
import torch

pytestmark = pytest.mark.gpu

from rankaae_amd.synthetic import make_spectra, write_csv

if torch.cuda.is_available():
    from rankaae_amd import model as pm
    from rankaae_amd.engine import StepEngine
    from oracle import ref_train
    DEV = torch.device("cuda:0")

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")


def _case_cfg(**over):
    with open(os.path.join(GOLDEN, "ref_compact_small.json")) as f:
        cfg = dict(json.load(f)["config"])
    cfg.update(ae_form="compact", tile_rows_mult=1, **over)
    return cfg


# (config, rows, data seed): the inline cases of tests/test_engine_gpu.py at large batches
CASES = {
    # first BIG size, serial chain (branches start at overlap_min_batch = 1536 rows)
    "compact_b1024": (_case_cfg(batch_size=1024), 1600, 6),
    # above overlap_min_batch: the engine's step is branched (side streams), the batch replays it on one stream
    "compact_b4096@2048": (_case_cfg(batch_size=2048), 6000, 4),
    # nstyle 5: the first decoder block (5 -> 8 channels) has no specialised shape, its GENERIC (KIND -1) instances run
    "compact_nstyle5@1024": (_case_cfg(nstyle=5, n_aux=3, batch_size=1024), 1600, 2),
}


def _make(cfg, t, stream=None):
    torch.manual_seed(100 + t)
    cls = pm.AE_CLS_DICT[cfg["ae_form"]]
    enc = cls["encoder"](nstyle=cfg["nstyle"], dropout_rate=cfg["dropout_rate"], dim_in=cfg["dim_in"],
                         n_layers=cfg["n_layers"])
    dec = cls["decoder"](nstyle=cfg["nstyle"], dropout_rate=cfg["dropout_rate"],
                         last_layer_activation=cfg["decoder_activation"], dim_out=cfg["dim_out"], n_layers=cfg["n_layers"])
    dis = pm.DiscriminatorFC(nstyle=cfg["nstyle"], dropout_rate=cfg["dis_dropout_rate"], noise=cfg["dis_noise"],
                             layers=cfg["FC_discriminator_layers"])
    return StepEngine(enc, dec, dis, cfg, DEV, rng_mode="philox", seed=500 + t, use_graph=True, stream=stream)


def _state(e):
    torch.cuda.synchronize()
    return ([e.arena.P.clone()] + [b_.clone() for mod in (e.enc_mod, e.dec_mod) for b_ in mod.buffers()] +
            [o.m.clone() for o in e.opts.values()] + [o.v.clone() for o in e.opts.values()], e.losses())


@pytest.mark.parametrize("case,T", [("compact_b1024", 3), ("compact_b4096@2048", 2), ("compact_nstyle5@1024", 2)])
def test_trial_batch_large_batch_is_bitwise_the_trials_alone(case, T):
    """T trials at 1024+ rows stepped by ONE launch sequence (every kernel with gridDim.z = T, the large-batch
    instances included): full batches (eager first step, captured graph, replays) and a ragged batch below 1024 rows
    (a second program, with the launch-bound instances) over two or more epochs, then validations of 1100 and 2100
    rows (eager, captured, replayed) -- every trial's weights, Adam moments, BatchNorm statistics, losses, validation
    styles and style metrics are BIT FOR BIT those of the same trial stepped alone."""
    from rankaae_amd.trial_batch import TrialBatch
    cfg, rows, data_seed = CASES[case]
    spec, aux, _ = make_spectra(rows, 256, cfg["n_aux"], seed=data_seed)
    bs = cfg["batch_size"]
    n_train, n_val = ref_train.split_rows(len(spec))[:2]
    full = n_train // bs
    ragged = n_train - full * bs
    assert full >= 1 and 2 <= ragged < 1024
    epochs = max(2, -(-3 // full))          # the full-batch shape: eager, captured and replayed at least once
    vs = torch.tensor(spec[n_train:n_train + n_val], dtype=torch.float32, device=DEV)
    va = torch.tensor(aux[n_train:n_train + n_val], dtype=torch.float32, device=DEV)
    splits = []
    for n in (1100, 2100):
        reps = -(-n // n_val)
        splits.append((vs.repeat(reps, 1)[:n].contiguous(), va.repeat(reps, 1)[:n].contiguous()))

    def perm(t, ep):
        return torch.randperm(n_train, generator=torch.Generator().manual_seed(1000 * t + ep))

    def make(t, stream=None):
        e = _make(cfg, t, stream)
        e.set_data(spec[:n_train], aux[:n_train])
        return e
    alone = []
    for t in range(T):
        e = make(t)
        for ep in range(epochs):
            e.set_epoch(perm(t, ep), 0.3)
            for _ in range(full):
                e.step(bs)
            e.step(ragged)
        vals = []
        for x, y in splits:
            for _ in range(3):                     # eager, captured, replayed
                z, vl = e.validate(x, y)
                vals.append((z.clone(), vl, [m.copy() for m in e.val_style_metrics()]))
        alone.append(_state(e) + (vals,))
        e.release()
        del e
    shared = TrialBatch.shared_stream(DEV)
    engs = [make(t, shared) for t in range(T)]
    batch = TrialBatch(engs)
    for ep in range(epochs):
        for t, e in enumerate(engs):
            e.set_epoch(perm(t, ep), 0.3)
        for _ in range(full):
            batch.step(bs)
        batch.step(ragged)
    assert batch.programs[(bs, True)][1] is not None and batch.launches_per_step(bs) > 50
    assert batch.programs[(ragged, True)][0] is not None
    for t, e in enumerate(engs):
        got = _state(e)
        for i, (a, b) in enumerate(zip(alone[t][0], got[0])):
            assert torch.equal(a, b), f"trial {t}: state tensor {i} differs from the same trial alone"
        assert alone[t][1] == got[1], (t, alone[t][1], got[1])
    for rep in range(6):
        x, y = splits[rep // 3]
        res = batch.validate([x] * T, [y] * T)
        key = ("val", x.shape[0], tuple(x.data_ptr() for _ in range(T)))
        assert batch.programs[key][0] is not None, "the validation was not batched"
        for t, e in enumerate(engs):
            z0, vl0, met0 = alone[t][2][rep]
            assert torch.equal(res[t][0], z0) and res[t][1] == vl0, (t, rep, res[t][1], vl0)
            W, rho = e.val_style_metrics()
            assert (W == met0[0]).all() and (rho == met0[1]).all()
    batch.release()
    for e in engs:
        e.release()


def test_per_layer_conv_kernels_are_refused_by_name():
    """``fused_blocks: false`` runs the per-layer conv kernels, which have no batched form: the recorder refuses the
    first step with ``BatchingRefused`` and names the first such kernel."""
    from rankaae_amd.trial_batch import BatchingRefused, TrialBatch
    cfg = _case_cfg(batch_size=256, fused_blocks=False)
    spec, aux, _ = make_spectra(600, 256, cfg["n_aux"], seed=6)
    n_train = ref_train.split_rows(len(spec))[0]
    shared = TrialBatch.shared_stream(DEV)
    engs = [_make(cfg, t, shared) for t in range(2)]
    for t, e in enumerate(engs):
        e.set_data(spec[:n_train], aux[:n_train])
        e.set_epoch(torch.randperm(n_train, generator=torch.Generator().manual_seed(t)), 0.3)
    batch = TrialBatch(engs)
    with pytest.raises(BatchingRefused) as info:
        batch.step(256)
    assert re.search(r"(conv_(fwd|bwd)|lenlin_|sum3_|grad_materialize)\w*_kernel", info.value.kernel), info.value.kernel
    assert info.value.kernel in str(info.value)
    assert not batch.programs
    batch.release()
    for e in engs:
        e.release()


def _run_train_sc(wd, cfg, spec, aux, grid):
    import subprocess
    import sys
    import yaml
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PYTHONPATH=root)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "RANKAAE_TRIAL_WORKERS", "RANKAAE_TRIALS_PER_GPU"):
        env.pop(k, None)
    wd.mkdir()
    write_csv(str(wd / "data.csv"), spec, aux, grid)
    with open(wd / "cfg.yaml", "w") as f:
        yaml.safe_dump(cfg, f)
    return subprocess.run([sys.executable, "-m", "rankaae_amd.cmd.train_sc", "-c", "cfg.yaml", "-w", str(wd)],
                          env=env, capture_output=True, text=True, timeout=900)


def test_train_sc_batched_conv_trials_at_1024_rows_equal_threads(tmp_path):
    """``train_sc`` with the conv networks at ``batch_size: 1024``: ``trial_mode: batched`` runs (it used to raise
    ValueError), and both trials end with BITWISE the weights and ``losses.csv`` of the same configuration under
    ``trial_mode: threads``; ``auto`` batches them without a refusal.  7000 spectra: the reference's data size, whose
    1050-row validation split runs the large-batch instances too."""
    with open(os.path.join(GOLDEN, "ref_compact_small.json")) as f:
        base = dict(json.load(f)["config"])
    spec, aux, grid = make_spectra(7000, 256, base["n_aux"], seed=8)
    out = {}
    for mode in ("batched", "threads", "auto"):
        cfg = dict(base)
        cfg.update(ae_form="compact", batch_size=1024, max_epoch=3, data_file="data.csv", verbose=False, timeout=1,
                   trial_mode=mode, trials=2, trial_seed=11)
        wd = tmp_path / mode
        r = _run_train_sc(wd, cfg, spec, aux, grid)
        assert r.returncode == 0, r.stderr[-3000:]
        log = (wd / "main_process_message.txt").read_text() + r.stderr
        assert "batched launches refused" not in log, log[-3000:]
        for k in (1, 2):
            job = wd / "training" / f"job_{k}"
            assert "Training finished" in (job / "messages.txt").read_text()
            out[(mode, k)] = (torch.load(job / "final.pt", map_location="cpu", weights_only=False),
                              (job / "losses.csv").read_text())
    for mode in ("batched", "auto"):
        for k in (1, 2):
            a, b = out[(mode, k)], out[("threads", k)]
            assert a[1] == b[1], (mode, k, a[1], b[1])
            for key in ("Encoder", "Decoder", "Style Discriminator"):
                sa, sb = a[0][key].state_dict(), b[0][key].state_dict()
                assert sa.keys() == sb.keys()
                for name in sa:
                    assert torch.equal(sa[name], sb[name]), (mode, k, key, name)
    c, d = out[("batched", 1)][0]["Encoder"].state_dict(), out[("batched", 2)][0]["Encoder"].state_dict()
    assert any(not torch.equal(c[n], d[n]) for n in c)
