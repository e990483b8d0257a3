"""``raae_kendall_tau`` and the ``rank_metrics`` key on the GPU.

The kernel against the brute-force numpy reference (tests/kendall_reference.py, itself pinned to scipy): the six pair
counts exactly, tau within 1e-12 (both sides form it from the same integers in the same double operations; the bound is
the one the reference holds against scipy), NaN where the reference is NaN.  The pair pass tiles 256 rows, so the row
counts are 1, 2, 3 (one partial tile), 255, 256, 257 (a full tile, one row over), 513 (three row tiles: diagonal and
off-diagonal tiles, the cyclic deal of an odd tile count) and 1024 (four row tiles: an even count, whose half-way offset
belongs to the lower row tiles alone).  At all of those every workgroup meets ONE column tile: the column splits are as
many as a row tile has offsets.  A workgroup goes round its column-tile loop again -- the stride over the offsets, the
LDS tile and the wave counts staged anew behind the barrier -- only from 3072 rows on, so the large shapes are 4097 x 1
(17 row tiles, the splits capped at 8: offsets 0 and 8 in one workgroup), 3072 x 16 (12 row tiles, 6 splits; the lower
row tiles reach offset 6, the upper ones stop at 5) and 4096 x 16 (16 row tiles, 4 splits: two or three column tiles in
every workgroup); ``_deal`` reads the split count back from the library and the tests assert those loop counts.  Then
the engine, the trainer, the batched trials and resume.
"""
import ctypes as C
import json
import logging
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import kendall_reference as kr
from rankaae_amd.synthetic import make_spectra

if torch.cuda.is_available():
    from rankaae_amd import _lib, model as pm, ops
    from rankaae_amd.engine import StepEngine
    from rankaae_amd.metrics import KendallTau
    from rankaae_amd.parameter import Parameters
    from rankaae_amd.trainer import Trainer, train_trials_batched
    from oracle import ref_train
    DEV = torch.device("cuda:0")

TILE = 256


def _deal(n, n_aux):
    """``(T, S, most, least)``: row tiles, column splits per row tile (read back from the size of the work buffer: 48
    bytes per workgroup and descriptor), and the most and the fewest column tiles one workgroup meets."""
    T = -(-n // TILE)
    S, rest = divmod(ops.kendall_tau_work_bytes(n, n_aux), 48 * T * n_aux)
    assert rest == 0 and S >= 1
    H = T // 2
    loops = [len(range(s, (H if (T % 2 or ti < H) else H - 1) + 1, S)) for ti in range(T) for s in range(S)]
    return T, S, max(loops), min(loops)


def _run(d, z, n_aux):
    kt = KendallTau(d.shape[0], n_aux, DEV)
    kt.launch(torch.from_numpy(d).to(DEV), torch.from_numpy(z).to(DEV))
    return kt.read()


# ------------------------------------------------------------------------------------------------ the kernel
@pytest.mark.parametrize("n_aux", [1, 5, 16])
@pytest.mark.parametrize("n", [1, 2, 3, TILE - 1, TILE, TILE + 1, 2 * TILE + 1, 4 * TILE])
def test_kernel_matches_reference(n, n_aux):
    # (16 columns hold all nine kinds of data; fewer columns start at another kind for every n)
    d, z = kr.make_matrix(n, n_aux, seed=100 + n, shift=n % len(kr.KINDS))
    tau, counts = _run(d, z, n_aux)
    want_tau, want_counts = kr.kendall_reference(d, z, n_aux)
    kr.assert_matches(tau, counts, want_tau, want_counts, what=f"n {n}, n_aux {n_aux}")


@pytest.mark.parametrize("n,n_aux,deal", [(16 * TILE + 1, 1, (17, 8, 2, 1)), (12 * TILE, 16, (12, 6, 2, 1)),
                                          (16 * TILE, 16, (16, 4, 3, 2))])
def test_kernel_matches_reference_where_a_workgroup_meets_several_column_tiles(n, n_aux, deal):
    """The shapes at which a workgroup restages its LDS tile: ``deal`` = (row tiles, column splits, the most and the
    fewest column tiles per workgroup), asserted so that a change of the split rule cannot quietly empty the test."""
    assert _deal(n, n_aux) == deal
    d, z = kr.make_matrix(n, n_aux, seed=7 + n, shift=n_aux)
    tau, counts = _run(d, z, n_aux)
    want_tau, want_counts = kr.kendall_reference(d, z, n_aux)
    kr.assert_matches(tau, counts, want_tau, want_counts, what=f"n {n}, n_aux {n_aux}")


def test_small_shapes_meet_one_column_tile_per_workgroup():
    """What the module docstring says of the small shapes, held against the library."""
    for n in (TILE - 1, TILE, TILE + 1, 2 * TILE + 1, 4 * TILE):
        for n_aux in (1, 5, 16):
            assert _deal(n, n_aux)[2] == 1, (n, n_aux)
    assert _deal(4 * TILE, 1)[:2] == (4, 3)
    assert _deal(15000, 5)[:3] == (59, 4, 8)            # the measured shape of DESIGN.md


@pytest.mark.parametrize("kind", kr.KINDS)
def test_kernel_matches_reference_per_kind(kind):
    n = 2 * TILE + 1
    d, z = kr.make_column(kind, n, seed=9)
    tau, counts = _run(d[:, None].copy(), z[:, None].copy(), 1)
    want_tau, want_counts = kr.kendall_reference(d[:, None], z[:, None], 1)
    kr.assert_matches(tau, counts, want_tau, want_counts, what=kind)
    if kind == "ulp_1e-38":         # neighbours one ulp apart at 1e-38 are ordered under any denormal mode
        assert counts[0, kr.TX] == counts[0, kr.TY] == counts[0, kr.TXY] == 0
        assert counts[0, kr.C] + counts[0, kr.D] == n * (n - 1) // 2
    if kind == "signed_zeros":      # +0.0 and -0.0 are ties
        assert counts[0, kr.TXY] > 0 and not np.isnan(tau[0])
    if kind in ("one_labelled", "constant"):
        assert np.isnan(tau[0])


def test_padding_columns_are_never_read_as_data():
    n, n_aux = 2 * TILE + 1, 5
    d, z = kr.make_matrix(n, n_aux, seed=4, ldd=7, ldz=6, shift=1)
    assert np.isnan(d[:, n_aux:]).all() and np.isnan(z[:, n_aux:]).all()
    tau, counts = _run(d, z, n_aux)
    want_tau, want_counts = kr.kendall_reference(d, z, n_aux)
    kr.assert_matches(tau, counts, want_tau, want_counts)
    d2, z2 = kr.make_matrix(n, n_aux, seed=4, shift=1)
    tau2, counts2 = _run(d2, z2, n_aux)
    assert tau.tobytes() == tau2.tobytes() and counts.tobytes() == counts2.tobytes()


def test_bad_arguments_are_refused_before_a_launch():
    lib = _lib.load()
    t = torch.zeros(64, device=DEV)
    w, c, tau = (torch.zeros(4096, dtype=dt, device=DEV) for dt in (torch.uint8, torch.int64, torch.float64))
    p = lambda x: C.c_void_p(x.data_ptr())      # noqa: E731
    good = dict(ldd=2, ldz=2, n=8, n_aux=2)
    for bad in (dict(n=0), dict(n_aux=0), dict(n_aux=17, ldd=17, ldz=17), dict(ldd=1), dict(ldz=1)):
        a = {**good, **bad}
        assert lib.raae_kendall_tau(p(t), a["ldd"], p(t), a["ldz"], a["n"], a["n_aux"], p(w), p(c), p(tau), None) == -1, bad
    assert lib.raae_kendall_tau(None, 2, p(t), 2, 8, 2, p(w), p(c), p(tau), None) == -1
    # the work buffer grows with the number of row tiles, not with its square
    assert ops.kendall_tau_work_bytes(150_000, 5) < 1 << 20
    assert ops.kendall_tau_work_bytes(1_200_000, 5) <= 8 * ops.kendall_tau_work_bytes(150_000, 5) + 4096


def test_two_launches_give_the_same_bytes():
    n, n_aux = 2 * TILE + 1, 5
    d, z = kr.make_matrix(n, n_aux, seed=21, shift=3)
    kt = KendallTau(n, n_aux, DEV)
    dd, zz = torch.from_numpy(d).to(DEV), torch.from_numpy(z).to(DEV)
    kt.launch(dd, zz)
    tau, counts = kt.read()
    kt.tau.fill_(7.0)
    kt.counts.fill_(-1)
    kt.work.fill_(0xAB)             # stale partials must not matter: every workgroup writes its own
    kt.launch(dd, zz)
    tau2, counts2 = kt.read()
    assert tau.tobytes() == tau2.tobytes() and counts.tobytes() == counts2.tobytes()


def test_three_trials_in_one_program_get_the_bytes_they_get_alone():
    lib = _lib.load()
    # 16 row tiles (an even count), 8 column splits: split 0 of the lower row tiles meets offsets 0 and 8
    n, n_aux, T = 16 * TILE, 5, 3
    assert _deal(n, n_aux) == (16, 8, 2, 1)
    data = [kr.make_matrix(n, n_aux, seed=300 + t, ldz=6, shift=t) for t in range(T)]
    alone = [_run(d, z, n_aux) for d, z in data]
    assert alone[0][1].tobytes() != alone[1][1].tobytes()
    kr.assert_matches(*alone[2], *kr.kendall_reference(*data[2], n_aux), what="trial 2 alone")
    kts = [KendallTau(n, n_aux, DEV) for _ in range(T)]
    dev = [(torch.from_numpy(d).to(DEV), torch.from_numpy(z).to(DEV)) for d, z in data]
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    handles = (C.c_void_p * T)()
    with torch.cuda.stream(stream):
        for t in range(T):
            assert lib.raae_record_begin() == 0
            try:
                kts[t].launch(*dev[t])
            finally:
                h, count = C.c_void_p(), C.c_int(0)
                rc = lib.raae_record_end(C.byref(h), C.byref(count))
            assert rc == 0 and count.value == 2, (rc, count.value)        # both launches have the batched form
            handles[t] = h
        stream.synchronize()
        for kt in kts:
            kt.tau.fill_(7.0)
            kt.counts.fill_(-1)
        prog = C.c_void_p()
        rc = lib.raae_multi_build(handles, T, C.byref(prog))
        for h in handles:
            lib.raae_record_free(C.c_void_p(h))
        assert rc == 0
        assert lib.raae_multi_launch(prog, C.c_void_p(stream.cuda_stream)) == 0
        stream.synchronize()
        lib.raae_multi_free(prog)
    for t in range(T):
        tau, counts = kts[t].read()
        assert tau.tobytes() == alone[t][0].tobytes() and counts.tobytes() == alone[t][1].tobytes(), f"plane {t}"


# ------------------------------------------------------------------------------------------------ the engine
def _case(case, frac=0.0):
    with open(os.path.join(os.path.dirname(__file__), "golden", f"ref_{case}.json")) as f:
        g = json.load(f)
    cfg = dict(g["config"])
    spec, aux, _ = make_spectra(g["n_rows"], g["n_points"], cfg["n_aux"], seed=g["data_seed"])
    if frac:
        aux = aux.copy()
        aux[np.random.default_rng(11).random(aux.shape) < frac] = np.nan
    return g, cfg, spec, aux


def _engine(cfg, seed, spec, aux, stream=None):
    torch.manual_seed(seed)
    cls = pm.AE_CLS_DICT[cfg["ae_form"]]
    enc = cls["encoder"](nstyle=cfg["nstyle"], dropout_rate=cfg["dropout_rate"], dim_in=cfg["dim_in"], n_layers=cfg["n_layers"])
    dec = cls["decoder"](nstyle=cfg["nstyle"], dropout_rate=cfg["dropout_rate"], last_layer_activation=cfg["decoder_activation"],
                         dim_out=cfg["dim_out"], n_layers=cfg["n_layers"])
    dis = pm.DiscriminatorFC(nstyle=cfg["nstyle"], dropout_rate=cfg["dis_dropout_rate"], noise=cfg["dis_noise"],
                             layers=cfg["FC_discriminator_layers"])
    eng = StepEngine(enc, dec, dis, cfg, DEV, rng_mode="philox", seed=seed, use_graph=True, stream=stream)
    n_train = ref_train.split_rows(len(spec))[0]
    eng.set_data(spec[:n_train], aux[:n_train])
    eng.set_epoch(torch.randperm(n_train, generator=torch.Generator().manual_seed(seed)), 0.3)
    eng.step(cfg["batch_size"])
    return eng


@pytest.mark.parametrize("case,frac", [("fc_small", 0.0), ("compact_small", 0.0), ("fc_small", 0.3)])
def test_validate_with_the_key_changes_nothing_and_reports_the_reference(case, frac):
    g, cfg, spec, aux = _case(case, frac)
    n_train, n_val = ref_train.split_rows(len(spec))[:2]
    vs = torch.tensor(spec[n_train:n_train + n_val], dtype=torch.float32, device=DEV)
    va = torch.tensor(aux[n_train:n_train + n_val], dtype=torch.float32, device=DEV)
    assert bool(torch.isnan(va).any()) == bool(frac)
    off = _engine(dict(cfg), g["model_seed"], spec, aux)
    on = _engine(dict(cfg, rank_metrics=True), g["model_seed"], spec, aux)
    assert on.aux_missing == bool(frac)
    with pytest.raises(RuntimeError, match="rank_metrics"):
        off.val_rank_metrics()
    for call in range(3):               # eager, captured, replayed
        z0, vl0 = off.validate(vs, va)
        z1, vl1 = on.validate(vs, va)
        assert torch.equal(z0, z1) and vl0 == vl1, (call, vl0, vl1)
        assert all(np.array_equal(a, b) for a, b in zip(off.val_style_metrics(), on.val_style_metrics()))
        if call in (0, 2):
            tau, counts = on.val_rank_metrics()
            want_tau, want_counts = kr.kendall_reference(va.cpu().numpy(), z1.cpu().numpy(), cfg["n_aux"])
            kr.assert_matches(tau, counts, want_tau, want_counts, what=f"{case} call {call}")
            assert np.isfinite(tau).all() and (counts[:, kr.M] <= n_val).all()
            assert (counts[:, kr.M] < n_val).any() == bool(frac)
    assert on._val_plan.graph is not None


# ------------------------------------------------------------------------------------------------ the trainer
CFG = dict(trials=1, timeout=10, verbose=False, max_epoch=3, batch_size=32, gradient_reversal=True, alpha_flat_step=739,
           alpha_limit=0.7172, decoder_activation="Softplus", dis_beta=1.1, dis_dropout_rate=0.056, dis_noise=0.56,
           gen_beta=1.1, n_aux=2, nstyle=3, ae_form="FC", dim_in=256, dim_out=256, n_layers=3, FC_discriminator_layers=3,
           use_cnn_discriminator=False, dropout_rate=0.04, sch_factor=0.5, sch_patience=0, lr_base=0.001,
           lr_ratio_Corr=10, lr_ratio_Mutual=1, lr_ratio_Reconn=10, lr_ratio_Smooth=1, lr_ratio_dis=1, lr_ratio_gen=10,
           optimizer_name="AdamW", spec_noise=0.02, use_flex_spec_target=True, weight_decay=0.01, kendall_activation=True,
           epoch_stop_smooth=2, ema_decay=0.9)
_counter = [0]


def _data():
    spec, aux, _ = make_spectra(200, 256, 2, seed=5)
    aux = aux.copy()
    aux[::7, 1] = np.nan                # a few missing labels of the second descriptor, in every split
    return spec, aux


class _Messages:
    def __init__(self):
        self.lines = []

    def info(self, msg):
        self.lines.append(msg)


class _Trial:
    """A Trainer on the synthetic data with a private host generator, a ``losses.csv`` that appends, and a tap on the
    engine's ``validate`` that keeps every epoch's styles."""

    def __init__(self, wd, cfg, seed, stream=None):
        os.makedirs(wd, exist_ok=True)
        _counter[0] += 1
        self.log = logging.getLogger(f"kendall_gpu_{_counter[0]}")
        self.log.setLevel(logging.DEBUG)
        self.log.propagate = False
        self.handler = logging.FileHandler(os.path.join(wd, "losses.csv"))
        self.handler.setFormatter(logging.Formatter("%(message)s"))
        self.log.addHandler(self.handler)
        self.messages = _Messages()
        torch.manual_seed(seed)
        self.wd = str(wd)
        self.trainer = Trainer.from_data(None, igpu=0, verbose=False, work_dir=self.wd, config_parameters=Parameters(cfg),
                                         logger=self.messages, loss_logger=self.log, arrays=_data(),
                                         host_rng=torch.Generator().manual_seed(seed), engine_stream=stream)
        self.styles = []
        eng, inner = self.trainer.engine, self.trainer.engine.validate

        def validate(spec, aux, **kw):
            z, vl = inner(spec, aux, **kw)
            if vl is not None:          # (not the emit phase of a batched validation)
                self.styles.append((aux.cpu().numpy(), z.cpu().numpy()))
            return z, vl
        eng.validate = validate

    def finish(self):
        self.trainer.engine.release()
        self.log.removeHandler(self.handler)
        self.handler.close()
        out = {name: open(os.path.join(self.wd, name), "rb").read() for name in ("losses.csv", "rank_metrics.csv")
               if os.path.exists(os.path.join(self.wd, name))}
        mods = torch.load(os.path.join(self.wd, "final.pt"), weights_only=False)
        out["final"] = {f"{key}.{name}": t.cpu() for key, mod in mods.items() for name, t in mod.state_dict().items()}
        return out


_runs = {}


def _alone(seed, tmp_path_factory, **over):
    """One uninterrupted run per (seed, options); shared, never changed."""
    key = (seed, tuple(sorted(over.items())))
    if key not in _runs:
        t = _Trial(tmp_path_factory.mktemp("alone"), {**CFG, **over}, seed)
        metrics = t.trainer.train()
        _runs[key] = dict(t.finish(), metrics=metrics, styles=t.styles, messages=t.messages.lines)
    return _runs[key]


def _rows(blob):
    lines = blob.decode().split("\n")
    assert lines[-1] == ""              # every row ends with a newline
    return lines[0], lines[1:-1]


def test_trainer_writes_one_row_per_epoch_and_nothing_else_changes(tmp_path_factory):
    on = _alone(11, tmp_path_factory, rank_metrics=True)
    off = _alone(11, tmp_path_factory)
    assert "rank_metrics.csv" not in off and not any("rank_metrics" in m or "rank metrics" in m for m in off["messages"])
    header, rows = _rows(on["rank_metrics.csv"])
    assert header == "Epoch,Tau_0,Tau_1,Labelled_0,Labelled_1" and len(rows) == 3
    # three epochs and the averaged-weights validation behind them (`ema_decay`), which writes no row
    assert len(on["styles"]) == 4
    n_val = on["styles"][0][0].shape[0]
    for epoch, row in enumerate(rows):
        aux, z = on["styles"][epoch]
        tau, counts = kr.kendall_reference(aux, z, 2)
        want = ",".join([f"{epoch:d}"] + [f"{t:.6f}" for t in tau] + [f"{int(m):d}" for m in counts[:, kr.M]])
        assert row == want, (epoch, row, want)
        assert counts[0, kr.M] == n_val and 2 <= counts[1, kr.M] < n_val and np.isfinite(tau).all()
    assert on["messages"].count("rank_metrics: Kendall tau-b of every descriptor's style on the validation split, "
                                "every epoch") == 1
    ema = [m for m in on["messages"] if m.startswith("EMA rank metrics:")]
    aux, z = on["styles"][3]
    assert len(ema) == 1 and all(f"{t:.6f}" in ema[0] for t in kr.kendall_reference(aux, z, 2)[0])
    # the run itself is the run without the key
    assert on["losses.csv"] == off["losses.csv"] and on["metrics"] == off["metrics"]
    assert on["final"].keys() == off["final"].keys()
    for k, t in off["final"].items():
        assert torch.equal(on["final"][k], t), k


def test_batched_trials_write_the_files_they_write_alone(tmp_path, tmp_path_factory, monkeypatch):
    from rankaae_amd.trial_batch import TrialBatch
    want = [_alone(seed, tmp_path_factory, rank_metrics=True) for seed in (11, 12)]
    assert want[0]["rank_metrics.csv"] != want[1]["rank_metrics.csv"]
    programs, inner = [], TrialBatch.validate

    def validate(self, specs, auxs):
        out = inner(self, specs, auxs)
        programs.extend(p[0] is not None for key, p in self.programs.items() if key[0] == "val")
        return out
    monkeypatch.setattr(TrialBatch, "validate", validate)
    stream = torch.cuda.Stream()
    group = [_Trial(tmp_path / f"b_{k}", {**CFG, "rank_metrics": True}, 11 + k, stream=stream) for k in range(2)]
    metrics = train_trials_batched([t.trainer for t in group])
    assert programs and all(programs)           # the validation with the key is one batched program: nothing refused
    for t, m, w in zip(group, metrics, want):
        got = t.finish()
        assert got["rank_metrics.csv"] == w["rank_metrics.csv"] and got["losses.csv"] == w["losses.csv"] and m == w["metrics"]
    # trials that disagree on the key are refused, like the neighbouring options
    mixed = [_Trial(tmp_path / f"c_{k}", {**CFG, "rank_metrics": k == 0}, 11 + k, stream=stream) for k in range(2)]
    with pytest.raises(ValueError, match="rank_metrics"):
        train_trials_batched([t.trainer for t in mixed])
    for t in mixed:
        t.trainer.engine.release()
        t.log.removeHandler(t.handler)
        t.handler.close()


def test_resumed_run_leaves_the_uninterrupted_file(tmp_path, tmp_path_factory):
    over = dict(rank_metrics=True, max_epoch=4, checkpoint_every=1)
    want = _alone(11, tmp_path_factory, **over)
    assert len(_rows(want["rank_metrics.csv"])[1]) == 4
    b = _Trial(tmp_path, {**CFG, **over}, 11)
    with pytest.raises(Exception, match="Training Overtime!"):
        b.trainer.train(lambda epoch, m: b.trainer.request_stop() if epoch == 1 else None)      # stops after epoch 2
    b.trainer.engine.release()
    b.log.removeHandler(b.handler)
    b.handler.close()
    stopped = open(tmp_path / "rank_metrics.csv", "rb").read()
    assert len(_rows(stopped)[1]) == 3 and want["rank_metrics.csv"].startswith(stopped)
    with open(tmp_path / "rank_metrics.csv", "ab") as f:
        f.write(b"9,0.500000,0.500000,1,1\n")        # a row from beyond the resume file is cut off
    c = _Trial(tmp_path, {**CFG, **over, "resume": True}, 1011)
    metrics = c.trainer.train()
    got = c.finish()
    assert got["rank_metrics.csv"] == want["rank_metrics.csv"]
    assert got["losses.csv"] == want["losses.csv"] and metrics == want["metrics"]
    # a resumed run that first turns the key on starts its file at the resumed epoch
    d = _Trial(tmp_path / "late", {**CFG, "max_epoch": 4, "checkpoint_every": 1}, 11)
    with pytest.raises(Exception, match="Training Overtime!"):
        d.trainer.train(lambda epoch, m: d.trainer.request_stop() if epoch == 1 else None)
    d.trainer.engine.release()
    d.log.removeHandler(d.handler)
    d.handler.close()
    assert not os.path.exists(tmp_path / "late" / "rank_metrics.csv")
    e = _Trial(tmp_path / "late", {**CFG, **over, "resume": True}, 11)
    e.trainer.train()
    header, rows = _rows(e.finish()["rank_metrics.csv"])
    assert header.startswith("Epoch,Tau_0") and rows == _rows(want["rank_metrics.csv"])[1][3:]
