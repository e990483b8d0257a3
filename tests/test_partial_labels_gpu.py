"""Missing descriptors (NaN AUX cells) on the GPU: the masked rank loss (``raae_rank_loss_masked_fwd_bwd``) against the
float64 restatement of its definition (``partial_label_reference``, pinned on the CPU by ``test_partial_labels_cpu.py``)
and against the unmasked kernel on compacted batches; the masked selection scores (``raae_select_scores_masked``)
against the unmasked kernel on each descriptor's labelled rows; training, batched trials and the report end to end on
data with 30 % of the cells missing; and the fully labelled path, which must not notice any of it.

Tolerances are the ones the unmasked kernels are already held to: the rank loss to 1e-5 relative (+ 1e-7) and its
gradient to 1e-5 relative (+ 1e-9), as ``tests/test_ops_gpu.py::test_rank_loss`` against the oracle; the selection scores
to one unit of the fourth decimal, as ``tests/test_report_gpu.py`` against ``tests/golden/selection_ref.json``."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from partial_label_reference import compact, masked_rank_loss
from rankaae_amd.synthetic import make_spectra, selection_inputs

if torch.cuda.is_available():
    from rankaae_amd import model as pm, ops, report
    from rankaae_amd.engine import StepEngine
    DEV = torch.device("cuda:0")

STEP = 1e-4 + 1e-9          # tests/test_report_gpu.py
TILE = 256                  # RANK_TJ, the pair pass's tile of j rows (raae_loss.hip)


# ------------------------------------------------------------------------------------------------ rank loss
def _rank_case(name):
    """``(d [B, K] with NaN, z [B, ld], K)``; column min(1, K - 1) holds 4 / 5 / 6: ties."""
    B, K = {"b5": (5, 1), "b7": (7, 5), "tile": (TILE + 1, 2), "blocked": (1100, 5)}[name]
    g = np.random.default_rng(B * 31 + K)
    d = g.standard_normal((B, K)).astype(np.float32)
    d[:, min(1, K - 1)] = g.integers(4, 7, size=B)
    z = g.standard_normal((B, K + 1)).astype(np.float32)
    if name == "b5":
        d[[0, 2, 3], 0] = np.nan                                   # 2 rows labelled
    elif name == "b7":
        d[[1, 5], 0] = np.nan
        d[[0, 1, 2, 6], 1] = np.nan                                # 3 labelled, of the tied column
        d[:, 2] = np.nan                                           # m = 0
        d[np.arange(7) != 4, 3] = np.nan                           # m = 1
        d[3, 4] = np.nan
    elif name == "tile":
        # one more row than the tile: labelled and unlabelled rows on both sides of the boundary, its two neighbours included
        d[[0, 7, 100, TILE - 2, TILE], 0] = np.nan                 # rows TILE - 1 (labelled) | TILE (not)
        d[[3, 50, TILE - 1], 1] = np.nan                           # rows TILE - 1 (not) | TILE (labelled)
    else:
        # > 1024 rows: four rows per thread and several column blocks (another grid and another partial layout)
        d[g.random((B, K)) < 0.3] = np.nan
        d[:, 3] = np.nan
    return d, z, K


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)


def _masked(d, z, K, act, grad=True):
    B, ld = z.shape
    work = torch.empty(ops.rank_loss_masked_work_bytes(B, K), dtype=torch.uint8, device=DEV)
    loss = torch.full((1,), 9.0, device=DEV)
    dz = torch.full((B, ld), 7.0, device=DEV) if grad else None
    ops.rank_loss_masked_fwd_bwd(_dev(d), K, _dev(z), ld, B, K, act, work, loss, dz)
    return float(loss), (dz.cpu().double().numpy() if grad else None)


def _unmasked(d, z, K, act):
    B, ld = z.shape
    work = torch.empty(ops.rank_loss_work_bytes(B, K), dtype=torch.uint8, device=DEV)
    loss = torch.full((1,), 9.0, device=DEV)
    dz = torch.full((B, ld), 7.0, device=DEV)
    ops.rank_loss_fwd_bwd(_dev(d), K, _dev(z), ld, B, K, act, work, loss, dz)
    return float(loss), dz.cpu().double().numpy()


def _close(got, want, what):
    err, tol = np.abs(got - want), 1e-9 + 1e-5 * np.abs(want)
    print(f"{what}: max |err| {err.max():.3e}, max err / tol {np.max(err / tol):.3f}")
    assert np.all(err <= tol), what


_REFS = {}


def _reference(name, act):
    """The float64 reference of a case, computed once."""
    if (name, act) not in _REFS:
        d, z, K = _rank_case(name)
        _REFS[name, act] = masked_rank_loss(d, z[:, :K], act)
    return _REFS[name, act]


@pytest.mark.parametrize("act", [False, True])
@pytest.mark.parametrize("name", ["b5", "b7", "tile", "blocked"])
def test_masked_rank_loss_is_the_float64_definition(name, act):
    d, z, K = _rank_case(name)
    lref, gref = _reference(name, act)
    loss, dz = _masked(d, z, K, act)
    print(f"{name} activate={act}: loss {loss!r} reference {lref!r}")
    assert abs(loss - lref) <= 1e-5 * abs(lref) + 1e-7, (loss, lref)
    assert not np.isnan(dz).any() and not np.isnan(loss)
    assert np.all(dz[:, :K][~np.isfinite(d)] == 0.0), "a row without a label has a gradient"
    assert np.all(dz[:, K:] == 0.0)
    _close(dz[:, :K], gref, f"{name} dz")
    loss_v, _ = _masked(d, z, K, act, grad=False)                  # validation form
    assert loss_v == loss


@pytest.mark.parametrize("act", [False, True])
@pytest.mark.parametrize("name,B", [("b5", 5), ("odd", 23), ("tile", TILE + 1)])
def test_masked_is_the_unmasked_kernel_on_the_compacted_batch(name, B, act):
    """``n_aux = 1``: the existing kernel (pinned to the reference) on the labelled rows, its gradient scattered back."""
    g = np.random.default_rng(B)
    d = g.integers(4, 9, size=(B, 1)).astype(np.float32) if name == "odd" else g.standard_normal((B, 1)).astype(np.float32)
    z = g.standard_normal((B, 1)).astype(np.float32)
    gone = {"b5": [0, 2, 3], "odd": [0, 4, 5, 11, 22], "tile": [0, 9, TILE - 1, TILE - 40]}[name]
    d[gone, 0] = np.nan
    loss, dz = _masked(d, z, 1, act)
    rows, dc, zc = compact(d, z)
    loss_c, dz_c = _unmasked(dc, zc, 1, act)
    want = np.zeros_like(dz)
    want[rows] = dz_c
    print(f"{name} activate={act}: masked {loss!r} compacted {loss_c!r}")
    assert abs(loss - loss_c) <= 1e-5 * abs(loss_c) + 1e-7
    _close(dz, want, f"{name} dz")
    assert np.all(dz[gone] == 0.0)


@pytest.mark.parametrize("B,K,act", [(36, 5, True), (TILE + 1, 1, False), (1100, 5, True)])
def test_masked_on_a_fully_labelled_batch_is_the_unmasked_kernel(B, K, act):
    g = np.random.default_rng(B + K)
    d = g.standard_normal((B, K)).astype(np.float32)
    d[:, min(1, K - 1)] = g.integers(4, 7, size=B)
    z = g.standard_normal((B, K + 1)).astype(np.float32)
    loss, dz = _masked(d, z, K, act)
    loss_u, dz_u = _unmasked(d, z, K, act)
    print(f"B={B}: masked {loss!r} unmasked {loss_u!r}")
    assert abs(loss - loss_u) <= 1e-5 * abs(loss_u) + 1e-7
    _close(dz, dz_u, "dz")


def test_masked_rank_loss_replays_bitwise_and_batches():
    """Captured into a graph and replayed, and as grid plane 1 of a two-trial launch: the bits of the eager call."""
    import ctypes as C
    from rankaae_amd import _lib
    lib = _lib.load()
    cases = [_rank_case("b7"), _rank_case("b7")]
    cases[1] = (np.roll(cases[1][0], 2, axis=0), cases[1][1] * 0.5, cases[1][2])
    stream = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(stream):
        bufs, eager = [], []
        for d, z, K in cases:
            B, ld = z.shape
            bufs.append((_dev(d), _dev(z), torch.empty(ops.rank_loss_masked_work_bytes(B, K), dtype=torch.uint8, device=DEV),
                         torch.zeros(1, device=DEV), torch.zeros(B, ld, device=DEV)))

        def call(i):
            dd, zz, work, loss, dz = bufs[i]
            ops.rank_loss_masked_fwd_bwd(dd, 5, zz, 6, 7, 5, True, work, loss, dz)
        handles = []
        for i in range(2):
            assert lib.raae_record_begin() == 0
            call(i)
            h, n = C.c_void_p(), C.c_int(0)
            assert lib.raae_record_end(C.byref(h), C.byref(n)) == 0 and n.value == 2
            handles.append(h)
            eager.append((bufs[i][3].clone(), bufs[i][4].clone()))
        torch.cuda.synchronize()
        prog = C.c_void_p()
        assert lib.raae_multi_build((C.c_void_p * 2)(*[h.value for h in handles]), 2, C.byref(prog)) == 0
        for h in handles:
            lib.raae_record_free(h)
        g = ops.Graph()
        g.begin()
        assert lib.raae_multi_launch(prog, C.c_void_p(stream.cuda_stream)) == 0
        g.end()
        for _ in range(2):
            for b in bufs:
                b[3].zero_(), b[4].fill_(3.0)
            g.launch()
            for i in range(2):
                assert torch.equal(bufs[i][3], eager[i][0]) and torch.equal(bufs[i][4], eager[i][1])
        torch.cuda.synchronize()
        del g
        lib.raae_multi_free(prog)


# ------------------------------------------------------------------------------------------------ selection scores
def _selection_case():
    """n = 40, k = 6, n_aux = 5, a quarter of the descriptor cells missing."""
    (z, aux, si, so), = selection_inputs(77, 1, 40, 6, 5, 32)
    gone = np.random.default_rng(5).random(aux.shape) < 0.25
    assert 40 <= gone.sum() <= 60 and (~gone).sum(axis=0).min() >= 20
    masked = aux.copy()
    masked[gone] = np.nan
    return z, aux, masked, si, so


def _slice(block, k):
    return block[report.SEL_HEAD + report.SEL_STRIDE * k:report.SEL_HEAD + report.SEL_STRIDE * (k + 1)]


def test_masked_selection_scores_are_the_unmasked_ones_on_each_descriptors_rows():
    z, aux, masked, si, so = _selection_case()
    block = report.score_arrays(z, masked, si, so)
    assert np.all(np.isfinite(block))
    for k in range(5):
        rows = np.flatnonzero(np.isfinite(masked[:, k]))
        # the existing kernel on the rows labelled for k (the other columns, whose slices are not read, fully labelled)
        want = _slice(report.score_arrays(z[rows], aux[rows], si[rows], so[rows]), k)
        got = _slice(block, k)
        print(f"descriptor {k}: {len(rows)} rows, max |diff| {np.abs(got - want).max():.3e}")
        assert np.all(np.abs(got - want) <= STEP), (k, got, want)
        if k == 1:
            assert got[0] == 1.0 and np.array_equal(got[2:6], want[2:6]), "thresholds are compared exactly"
            assert np.array_equal(got[6:15], want[6:15]), "confusion counts are integers"
    # reconstruction error and inter-style correlation use all rows: the unmasked call's bits
    head = report.score_arrays(z, aux, si, so)[:report.SEL_HEAD]
    assert block[:report.SEL_HEAD].tobytes() == head.tobytes()
    # the rounded result dict, as the report forms it
    res = report.result_from_block(block, 5, report.labelled_counts(masked))
    assert all(res["Style-descriptor Corr"][k] is not None for k in range(5))


def test_masked_selection_scores_thin_descriptor_and_batched_form():
    z, aux, masked, si, so = _selection_case()
    thin = masked.copy()
    thin[2:, 4] = np.nan                                           # two labelled rows: no score
    thin[:, 1] = np.nan                                            # the coordination number not labelled at all
    block = report.score_arrays(z, thin, si, so)
    assert np.all(_slice(block, 4) == 0.0) and np.all(_slice(block, 1) == 0.0) and np.all(np.isfinite(block))
    res = report.result_from_block(block, 5, report.labelled_counts(thin))
    assert res["Style-descriptor Corr"][4] is None and res["Style-descriptor Corr"][1] is None
    assert report.score_matrix({"a": res})[1][0].tolist()[3] == 0 and report.score_matrix({"a": res})[1][0].tolist()[6] == 0
    assert _slice(block, 0).tobytes() == _slice(report.score_arrays(z, masked, si, so), 0).tobytes()
    # one model per grid plane: the bits of the model alone
    both = report.score_arrays_batched([(z, masked, si, so), (z * 0.5, thin, si, so)])
    assert both[0].tobytes() == report.score_arrays(z, masked, si, so).tobytes()
    assert both[1].tobytes() == report.score_arrays(z * 0.5, thin, si, so).tobytes()


# ------------------------------------------------------------------------------------------------ end to end
def _case(case, frac=0.3):
    with open(os.path.join(os.path.dirname(__file__), "golden", f"ref_{case}.json")) as f:
        g = json.load(f)
    cfg = dict(g["config"])
    spec, aux, _ = make_spectra(g["n_rows"], g["n_points"], cfg["n_aux"], seed=g["data_seed"])
    if frac:
        aux = aux.copy()
        aux[np.random.default_rng(11).random(aux.shape) < frac] = np.nan
    return g, cfg, spec, aux


class _Log:
    def __init__(self):
        self.lines = []

    def info(self, msg):
        self.lines.append(msg)


def _train(cfg, spec, aux, work_dir, model_seed):
    from rankaae_amd.parameter import Parameters
    from rankaae_amd.trainer import Trainer
    os.makedirs(work_dir, exist_ok=True)
    torch.manual_seed(model_seed)
    log, losses = _Log(), _Log()
    tr = Trainer.from_data(None, igpu=0, verbose=False, work_dir=str(work_dir), config_parameters=Parameters(cfg),
                           logger=log, loss_logger=losses, arrays=(spec, aux))
    metrics = tr.train()               # AnomalyError (detect_anomaly) would surface here
    return tr, metrics, log.lines, losses.lines


@pytest.mark.parametrize("case", ["fc_small", "compact_small"])
def test_training_and_report_on_partially_labelled_data(case, tmp_path):
    from rankaae_amd.dataloader import get_dataloaders
    g, cfg, spec, aux = _case(case)
    assert 0.25 < np.isnan(aux).mean() < 0.35
    cfg.update(rng_mode="philox", seed=5, max_epoch=2, detect_anomaly=True)
    jobs = tmp_path / "training"
    tr, metrics, messages, losses = _train(cfg, spec, aux, jobs / "job_1", g["model_seed"])
    assert tr.engine.aux_missing and len(metrics) == 5 and all(np.isfinite(metrics)), metrics
    assert sum("labelled fraction per descriptor" in m for m in messages) == 1
    rows = [r for r in losses[1:]]
    assert rows and losses[0].startswith("Epoch,")
    for r in rows:
        vals = [float(v) for v in r.replace("\t", "").split(",") if v.strip()]
        assert len(vals) == 13 and all(np.isfinite(vals)), r
    assert vals[5] != 0.0 and vals[6] != 0.0                        # Train_Aux, Val_Aux: the masked rank loss
    # one seed, two runs: the same bits
    _train(cfg, spec, aux, tmp_path / "again", g["model_seed"])
    a = torch.load(jobs / "job_1" / "final.pt", map_location="cpu", weights_only=False)
    b = torch.load(tmp_path / "again" / "final.pt", map_location="cpu", weights_only=False)
    for key in a:
        sa, sb = a[key].state_dict(), b[key].state_dict()
        assert list(sa) == list(sb) and all(torch.equal(sa[n], sb[n]) for n in sa), key
    # a second trial, and the report ranks the two on the (partially labelled) validation split
    _train(dict(cfg, seed=6), spec, aux, jobs / "job_2", g["model_seed"] + 1)
    test_ds = get_dataloaders(None, cfg["batch_size"], n_aux=cfg["n_aux"], arrays=(spec, aux))[1].dataset
    assert np.isnan(test_ds.aux).any()
    info = {}
    results = report.evaluate_all_models(str(jobs), test_ds, info=info)
    assert info["mode"] == "batched"
    results, ranked = report.sort_all_models(results, sort_score=report.sorting_algorithm, ascending=False)
    assert sorted(map(str, ranked)) == ["job_1", "job_2"] and sorted(r["Rank"] for r in results.values()) == [0, 1]
    for r in results.values():
        assert np.isfinite(r["Score"]) and np.isfinite(r["Inter-style Corr"])
        for k, c in r["Style-descriptor Corr"].items():
            assert c is not None and np.isfinite(c["F1 score"] if k == 1 else c["Spearman"]), (k, c)
    # the batched replay gives what one model gives alone
    alone = report.evaluate_model(test_ds, report.load_model(str(jobs), "job_1"))
    assert alone["Style-descriptor Corr"] == results["job_1"]["Style-descriptor Corr"]


@pytest.mark.parametrize("case", ["fc_small", "compact_small"])
def test_trial_in_a_batch_of_three_is_bitwise_the_trial_alone(case):
    """The pattern of ``tests/test_engine_gpu.py``'s batched-trials test, on data with missing descriptors."""
    from oracle import ref_train
    from rankaae_amd.trial_batch import TrialBatch
    g, cfg, spec, aux = _case(case)
    cfg = dict(cfg, detect_anomaly=True)
    T, bs = 3, cfg["batch_size"]
    n_train, n_val = ref_train.split_rows(len(spec))[:2]
    ragged = n_train - 3 * bs if 2 <= n_train - 3 * bs < bs else bs // 2

    def make(t, stream=None):
        torch.manual_seed(100 + t)
        cls = pm.AE_CLS_DICT[cfg["ae_form"]]
        enc = cls["encoder"](nstyle=cfg["nstyle"], dropout_rate=cfg["dropout_rate"], dim_in=cfg["dim_in"], n_layers=cfg["n_layers"])
        dec = cls["decoder"](nstyle=cfg["nstyle"], dropout_rate=cfg["dropout_rate"], last_layer_activation=cfg["decoder_activation"],
                             dim_out=cfg["dim_out"], n_layers=cfg["n_layers"])
        dis = pm.DiscriminatorFC(nstyle=cfg["nstyle"], dropout_rate=cfg["dis_dropout_rate"], noise=cfg["dis_noise"],
                                 layers=cfg["FC_discriminator_layers"])
        eng = StepEngine(enc, dec, dis, cfg, DEV, rng_mode="philox", seed=500 + t, use_graph=True, stream=stream)
        eng.set_data(spec[:n_train], aux[:n_train])
        assert eng.aux_missing
        return eng

    def state(e):
        torch.cuda.synchronize()
        return ([e.arena.P.clone()] + [b_.clone() for mod in (e.enc_mod, e.dec_mod) for b_ in mod.buffers()] +
                [o.m.clone() for o in e.opts.values()] + [o.v.clone() for o in e.opts.values()], e.losses())
    vs = torch.tensor(spec[n_train:n_train + n_val], dtype=torch.float32, device=DEV)
    va = torch.tensor(aux[n_train:n_train + n_val], dtype=torch.float32, device=DEV)
    assert torch.isnan(va).any()

    def perm(t, ep):
        return torch.randperm(n_train, generator=torch.Generator().manual_seed(1000 * t + ep))
    alone = []
    for t in range(T):
        e = make(t)
        for ep in range(2):
            e.set_epoch(perm(t, ep), 0.3)
            for _ in range(3):
                e.step(bs)
            e.step(ragged)
        vals = []
        for _ in range(3):                         # eager, captured, replayed
            z, vl = e.validate(vs, va)
            vals.append((z.clone(), vl))
        alone.append(state(e) + (vals,))
        assert e.anomaly() is None and all(np.isfinite(v) for v in alone[-1][1].values()), alone[-1][1]
    shared = TrialBatch.shared_stream(DEV)
    engs = [make(t, shared) for t in range(T)]
    batch = TrialBatch(engs)
    for ep in range(2):
        for t, e in enumerate(engs):
            e.set_epoch(perm(t, ep), 0.3)
        for _ in range(3):
            batch.step(bs)
        batch.step(ragged)
    assert batch.programs[(bs, True)][1] is not None
    for t, e in enumerate(engs):
        got = state(e)
        for a, b in zip(alone[t][0], got[0]):
            assert torch.equal(a, b), f"trial {t} differs from the same trial alone"
        assert alone[t][1] == got[1]
    for rep in range(3):
        res = batch.validate([vs] * T, [va] * T)
        for t in range(T):
            z0, vl0 = alone[t][2][rep]
            assert torch.equal(res[t][0], z0) and res[t][1] == vl0, (t, rep, res[t][1], vl0)
            assert np.isfinite(vl0["kendall"])
    batch.release()


# ------------------------------------------------------------------------------------------------ the unchanged path
def _entry_points(monkeypatch, fn):
    """The ``ops`` entry points ``fn()`` goes through, in order (every launch of the engine is an ``ops`` call)."""
    import types
    log = []
    for name, f in list(vars(ops).items()):
        if isinstance(f, types.FunctionType) and not name.startswith("_") and f.__module__ == ops.__name__:
            monkeypatch.setattr(ops, name, (lambda n, f_: lambda *a, **k: (log.append(n), f_(*a, **k))[1])(name, f))
    try:
        fn()
    finally:
        monkeypatch.undo()
    return log


@pytest.mark.parametrize("case", ["fc_small", "compact_small"])
def test_fully_labelled_data_launches_no_masked_kernel(case, monkeypatch):
    from oracle import ref_train
    logs = {}
    for frac in (0.0, 0.3):
        g, cfg, spec, aux = _case(case, frac)
        n_train, n_val = ref_train.split_rows(len(spec))[:2]
        torch.manual_seed(3)
        cls = pm.AE_CLS_DICT[cfg["ae_form"]]
        enc = cls["encoder"](nstyle=cfg["nstyle"], dropout_rate=cfg["dropout_rate"], dim_in=cfg["dim_in"], n_layers=cfg["n_layers"])
        dec = cls["decoder"](nstyle=cfg["nstyle"], dropout_rate=cfg["dropout_rate"], last_layer_activation=cfg["decoder_activation"],
                             dim_out=cfg["dim_out"], n_layers=cfg["n_layers"])
        dis = pm.DiscriminatorFC(nstyle=cfg["nstyle"], dropout_rate=cfg["dis_dropout_rate"], noise=cfg["dis_noise"],
                                 layers=cfg["FC_discriminator_layers"])
        eng = StepEngine(enc, dec, dis, cfg, DEV, rng_mode="philox", seed=1, use_graph=False)
        vs = torch.tensor(spec[n_train:n_train + n_val], dtype=torch.float32, device=DEV)
        va = torch.tensor(aux[n_train:n_train + n_val], dtype=torch.float32, device=DEV)

        def run():
            eng.set_data(spec[:n_train], aux[:n_train])
            eng.set_epoch(torch.arange(n_train), 0.3)
            eng.step(cfg["batch_size"])
            eng.validate(vs, va)
        logs[frac] = _entry_points(monkeypatch, run)
        torch.cuda.synchronize()
        assert eng.aux_missing == bool(frac)
    full, part = logs[0.0], logs[0.3]
    assert not [n for n in full if "masked" in n] and full.count("rank_loss_fwd_bwd") == 2      # the step and the validation
    assert part.count("rank_loss_masked_fwd_bwd") == 2 and "rank_loss_fwd_bwd" not in part
    # nothing else moved: the two sequences differ in those two calls alone
    assert [n.replace("_masked", "") for n in part] == full
    # and the report's scorer on a fully labelled split is the unmasked one
    g, cfg, spec, aux = _case(case, 0.0)
    assert not report.SelectionScorer(40, 6, 5, 32, DEV, masked=report.has_missing(aux)).masked
