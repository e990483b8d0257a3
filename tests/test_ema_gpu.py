"""``ema_decay`` on the GPU: the kernel (``raae_ema_step``) against float64, its refusals and its batched form; the
engine's average over eager, captured and replayed steps; ``ema_weights()``; batched trials; ``Trainer`` / ``train_sc``
(``final_ema.pt``, the ``EMA weights:`` line); resume, bit for bit; ``generate_report`` with ``report_weights``."""
import copy
import ctypes as C
import json
import logging
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

import ema_reference
from rankaae_amd.synthetic import make_spectra, write_csv

if torch.cuda.is_available():
    from rankaae_amd import _lib, model as pm, ops
    from rankaae_amd.engine import StepEngine
    from rankaae_amd.parameter import Parameters
    DEV = torch.device("cuda:0")

LOSS_KEYS = ("adversarial", "kendall", "recon", "mutual_info", "smooth")


# ------------------------------------------------------------------------------------------------ 1. the kernel
SIZES = [1, 3, 255, 256, 257, 65541]     # 65541: above the grid cap (64 workgroups x 256 threads x 4), and 65541 % 4 == 1
DECAYS = [0.5, 0.999, 0.9999]
OFFSETS = [(0, 0), (1, 1), (0, 1), (1, 0)]      # floats into the allocation: (0, 0) is the float4 body, the rest scalar
GUARD = 4                                 # guard floats on each side (16 bytes: offset 0 stays 16-byte aligned)
FILL = -777.25
_data_cache = {}


def _values(n, nan_at):
    """(ema0, p) on the host: standard normals scaled by 1e-3, 1 or 1e3 per element, about one exact zero in eight, and
    one NaN in ``p`` (``nan_at``; None: none).  Made once per case, shared, never changed."""
    if (n, nan_at) not in _data_cache:
        g = torch.Generator().manual_seed(1000 + n)
        out = []
        for _ in range(2):
            v = torch.randn(n, generator=g) * torch.tensor([1e-3, 1.0, 1e3])[torch.randint(0, 3, (n,), generator=g)]
            v[torch.rand(n, generator=g) < 0.125] = 0.0
            out.append(v)
        if nan_at is not None:
            out[1][nan_at] = float("nan")
        _data_cache[(n, nan_at)] = tuple(out)
    return _data_cache[(n, nan_at)]


def _guarded(values, off):
    """``values`` at ``GUARD + off`` floats into a fresh device allocation filled with ``FILL``: (buffer, view)."""
    n = values.numel()
    buf = torch.full((GUARD + off + n + GUARD,), FILL, device=DEV)
    view = buf[GUARD + off:GUARD + off + n]
    view.copy_(values)
    assert view.data_ptr() % 16 == (4 * off) % 16
    return buf, view


def _guards_intact(buf, off, n):
    lo, hi = buf[:GUARD + off], buf[GUARD + off + n:]
    want = int(torch.tensor([FILL]).view(torch.int32)[0])
    return bool((lo.view(torch.int32) == want).all()) and bool((hi.view(torch.int32) == want).all())


@pytest.mark.parametrize("decay", DECAYS)
@pytest.mark.parametrize("n", SIZES)
def test_kernel_matches_float64(n, decay):
    """Per element ``|out - ref64| <= 2^-22 * max(|ema|, |p|)`` (``ema_reference.step_bound``: derived, not tuned); the
    NaN of ``p`` arrives in ``out`` at its position and nowhere else; nothing outside ``[0, n)`` changes; a captured and
    replayed call is bitwise the eager one -- at every alignment of the two pointers."""
    cases = [n // 2] + ([None] if n == 1 else [])        # (n == 1: also without the NaN, so that a number is checked)
    for nan_at in cases:
        ema0, p = _values(n, nan_at)
        ref = ema_reference.ema_step(ema0, p, decay)
        bound = ema_reference.step_bound(ema0, torch.nan_to_num(p, nan=0.0))
        for off_e, off_p in OFFSETS:
            ebuf, e = _guarded(ema0, off_e)
            pbuf, pv = _guarded(p, off_p)
            p_before = pbuf.clone()
            ops.ema_step(e, pv, n, decay)
            torch.cuda.synchronize()
            out = e.cpu()
            nan = torch.isnan(out)
            want_nan = torch.zeros(n, dtype=torch.bool)
            if nan_at is not None:
                want_nan[nan_at] = True
            assert torch.equal(nan, want_nan), (n, decay, off_e, off_p, nan.nonzero().flatten().tolist()[:5])
            err = (out.double() - ref).abs()[~want_nan]
            excess = err - bound[~want_nan]
            if excess.numel():
                print(f"n {n} decay {decay} offsets {off_e},{off_p}: max |err| / bound "
                      f"{float((err / bound[~want_nan].clamp_min(1e-300)).max()):.3f}")
                assert float(excess.max()) <= 0.0, (n, decay, off_e, off_p, float(excess.max()), int(excess.argmax()))
            assert _guards_intact(ebuf, off_e, n) and torch.equal(pbuf.view(torch.int32), p_before.view(torch.int32))
            # captured, then replayed once: the eager result, bit for bit
            ebuf2, e2 = _guarded(ema0, off_e)
            stream = torch.cuda.Stream()
            stream.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(stream):
                g = ops.Graph()
                g.begin()
                ops.ema_step(e2, pv, n, decay)
                g.end()
                g.launch()
            stream.synchronize()
            assert torch.equal(ebuf2.view(torch.int32), ebuf.view(torch.int32)), (n, decay, off_e, off_p)
            del g


def test_vector_and_scalar_bodies_give_the_same_bits():
    ema0, p = _values(65541, None)
    outs = []
    for off_e, off_p in OFFSETS:
        _, e = _guarded(ema0, off_e)
        _, pv = _guarded(p, off_p)
        ops.ema_step(e, pv, 65541, 0.999)
        outs.append(e.clone())
    for o in outs[1:]:
        assert torch.equal(o.view(torch.int32), outs[0].view(torch.int32))


# ------------------------------------------------------------------------------------------------ 2. refusals
@pytest.mark.parametrize("case", ["ema_null", "p_null", "n_zero", "decay_negative", "decay_one", "decay_nan"])
def test_kernel_refuses_bad_arguments_and_writes_nothing(case):
    ema0, p = _values(257, None)
    ebuf, e = _guarded(ema0, 0)
    pbuf, pv = _guarded(p, 0)
    before = (ebuf.clone(), pbuf.clone())
    args = {"ema_null": (None, pv, 257, 0.9), "p_null": (e, None, 257, 0.9), "n_zero": (e, pv, 0, 0.9),
            "decay_negative": (e, pv, 257, -0.1), "decay_one": (e, pv, 257, 1.0),
            "decay_nan": (e, pv, 257, float("nan"))}[case]
    a, b, n, decay = args
    rc = _lib.load().raae_ema_step(ops._ptr(a), ops._ptr(b), n, decay, ops._stream())
    torch.cuda.synchronize()
    assert rc == -1, rc                                     # RAAE_EINVAL
    assert torch.equal(ebuf.view(torch.int32), before[0].view(torch.int32))
    assert torch.equal(pbuf.view(torch.int32), before[1].view(torch.int32))
    if a is not None and b is not None:
        with pytest.raises(_lib.HipCallError):
            ops.ema_step(a, b, n, decay)


# ------------------------------------------------------------------------------------------------ 3. batched form
def test_batched_planes_are_bitwise_the_single_calls():
    """Three planes, n = 257, decays 0.5 / 0.9 / 0.999, through the recorder and one ``gridDim.z = 3`` launch.  The
    recorder logs launches while they run, so every plane is stepped twice (recording, then the batched launch): the
    single calls are made twice too."""
    lib = _lib.load()
    n, decays = 257, [0.5, 0.9, 0.999]
    planes, single = [], []
    for t, d in enumerate(decays):
        g = torch.Generator().manual_seed(70 + t)
        e0, p = torch.randn(n, generator=g), torch.randn(n, generator=g)
        planes.append((_guarded(e0, 0), _guarded(p, 0)))
        (_, e), (_, pv) = _guarded(e0, 0), _guarded(p, 0)
        ops.ema_step(e, pv, n, d)
        ops.ema_step(e, pv, n, d)
        single.append(e.clone())
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    handles = (C.c_void_p * 3)()
    with torch.cuda.stream(stream):
        for t, d in enumerate(decays):
            assert lib.raae_record_begin() == 0
            try:
                ops.ema_step(planes[t][0][1], planes[t][1][1], n, d)
            finally:
                h, count = C.c_void_p(), C.c_int(0)
                rc = lib.raae_record_end(C.byref(h), C.byref(count))
            assert rc == 0 and count.value == 1
            handles[t] = h
        stream.synchronize()
        prog = C.c_void_p()
        rc = lib.raae_multi_build(handles, 3, C.byref(prog))
        for h in handles:
            lib.raae_record_free(C.c_void_p(h))
        assert rc == 0
        assert lib.raae_multi_launch(prog, C.c_void_p(stream.cuda_stream)) == 0
        stream.synchronize()
        lib.raae_multi_free(prog)
    for t in range(3):
        (ebuf, e), _ = planes[t]
        assert torch.equal(e.view(torch.int32), single[t].view(torch.int32)), f"plane {t}"
        assert _guards_intact(ebuf, 0, n)
    assert not torch.equal(single[0], single[1])


# ------------------------------------------------------------------------------------------------ the engine
def _case_cfg(ae_form, **over):
    case = "fc_small" if ae_form == "FC" else "compact_small"
    with open(os.path.join(os.path.dirname(__file__), "golden", f"ref_{case}.json")) as f:
        return dict(json.load(f)["config"], batch_size=32, **over)


def _modules(cfg, seed):
    torch.manual_seed(seed)
    cls = pm.AE_CLS_DICT[cfg["ae_form"]]
    enc = cls["encoder"](nstyle=cfg["nstyle"], dropout_rate=cfg["dropout_rate"], dim_in=cfg["dim_in"], n_layers=cfg["n_layers"])
    dec = cls["decoder"](nstyle=cfg["nstyle"], dropout_rate=cfg["dropout_rate"],
                         last_layer_activation=cfg["decoder_activation"], dim_out=cfg["dim_out"], n_layers=cfg["n_layers"])
    dis = pm.DiscriminatorFC(nstyle=cfg["nstyle"], dropout_rate=cfg["dis_dropout_rate"], noise=cfg["dis_noise"],
                             layers=cfg["FC_discriminator_layers"])
    return enc, dec, dis


def _engine(cfg, seed, spec, aux, use_graph=True, stream=None):
    eng = StepEngine(*_modules(cfg, seed), cfg, DEV, rng_mode="philox", seed=700 + seed, use_graph=use_graph, stream=stream)
    eng.set_data(spec, aux)
    return eng


def _perm(n, seed):
    return torch.randperm(n, generator=torch.Generator().manual_seed(seed))


def _count_launches(eng, b):
    """Launches of one more step of ``eng``, as the recorder counts them (the step runs)."""
    lib = _lib.load()
    with torch.cuda.stream(eng.stream):
        P = eng._pre_step(b, True)
        assert lib.raae_record_begin() == 0
        try:
            eng.emit_step(P, True, record=False)
        finally:
            h, count = C.c_void_p(), C.c_int(0)
            rc = lib.raae_record_end(C.byref(h), C.byref(count))
        assert rc == 0
        lib.raae_record_free(h)
    torch.cuda.synchronize()
    return count.value


_trained = {}


def _six_steps(ae_form):
    """96 spectra, batch 32, ``use_graph``, ``ema_decay: 0.9``: six steps (one eager, one captured, four replays; two
    epochs of three) of the engine with the key and of its twin without, the parameters read back after every step.
    Run once per network, shared, never changed."""
    if ae_form not in _trained:
        cfg = _case_cfg(ae_form)
        spec, aux, _ = make_spectra(96, cfg["dim_in"], cfg["n_aux"], seed=4)
        eng = _engine(dict(cfg, ema_decay=0.9), 21, spec, aux)
        twin = _engine(cfg, 21, spec, aux)
        torch.cuda.synchronize()
        ema0 = eng.ema_P.cpu().clone()
        assert torch.equal(ema0, eng.arena.P.detach().cpu())
        snaps, emas = [], []
        for e in (eng, twin):
            for epoch in range(2):
                e.set_epoch(_perm(96, 30 + epoch), 0.3)
                for _ in range(3):
                    e.step(32)
                    if e is eng:
                        torch.cuda.synchronize()
                        snaps.append(eng.arena.P.detach().cpu().clone())
                        emas.append(eng.ema_P.cpu().clone())
        torch.cuda.synchronize()
        _trained[ae_form] = dict(cfg=cfg, spec=spec, aux=aux, eng=eng, twin=twin, ema0=ema0, snaps=snaps, emas=emas,
                                 losses=(eng.losses(), twin.losses()))
    return _trained[ae_form]


@pytest.mark.parametrize("ae_form", ["FC", "compact"])
def test_engine_average_follows_the_float64_recurrence(ae_form):
    """After step k: ``|ema_P - ref| <= k * 2^-22 * M`` per element, ``M`` the largest magnitude the element has had
    (initial value and every snapshot): one step's bound (``ema_reference.step_bound``) accumulates under a contraction
    (``decay < 1``), and every average is a convex combination of those values."""
    t = _six_steps(ae_form)
    refs = ema_reference.ema_run(t["ema0"], t["snaps"], 0.9)
    big = t["ema0"].double().abs()
    assert len(refs) == 6
    for k, (ref, snap, got) in enumerate(zip(refs, t["snaps"], t["emas"]), start=1):
        big = torch.maximum(big, snap.double().abs())
        err = (got.double() - ref).abs()
        bound = k * 2.0 ** -22 * big
        print(f"{ae_form} step {k}: max |err| {float(err.max()):.3e}, max err / bound "
              f"{float((err / bound.clamp_min(1e-300)).max()):.3f}, moved {float((got - t['ema0']).abs().max()):.3e}")
        assert float((err - bound).max()) <= 0.0, (k, int((err - bound).argmax()))
    assert not torch.equal(t["emas"][-1], t["snaps"][-1]) and not torch.equal(t["emas"][-1], t["ema0"])


@pytest.mark.parametrize("ae_form", ["FC", "compact"])
def test_average_does_not_perturb_training_and_costs_one_launch(ae_form):
    t = _six_steps(ae_form)
    eng, twin = t["eng"], t["twin"]
    assert getattr(twin, "ema_P", None) is None and eng.ema_P is not None
    assert torch.equal(eng.arena.P.detach(), twin.arena.P.detach())
    a, b = t["losses"]
    assert all(a[k] == b[k] for k in LOSS_KEYS), (a, b)
    if "launches" not in t:
        counts = []
        for e in (eng, twin):
            e.set_epoch(_perm(96, 40), 0.3)
            counts.append(_count_launches(e, 32))
        t["launches"] = counts
    with_key, without = t["launches"]
    print(f"{ae_form}: {with_key} launches per step with ema_decay, {without} without")
    assert with_key == without + 1


# ------------------------------------------------------------------------------------------------ 5. ema_weights()
def _rows_forward_of_average(t):
    """``reconstruct`` of the first 8 rows by a FRESH engine (no key) whose modules are copies of the live ones with the
    parameters set to ``ema_P``."""
    eng = t["eng"]
    torch.cuda.synchronize()
    ema = eng.ema_P.cpu()
    mods = []
    for live in (eng.enc_mod, eng.dec_mod, eng.dis_mod):
        m = copy.deepcopy(live)
        for p_new, p_live in zip(m.parameters(), live.parameters()):
            o = eng.arena.off(p_live)
            p_new.data = ema[o:o + p_live.numel()].view(p_live.shape).clone()
        mods.append(m.cpu())
    fresh = StepEngine(*mods, t["cfg"], DEV, rng_mode="philox", seed=1, use_graph=False)
    rows = torch.as_tensor(t["spec"][:8], dtype=torch.float32).to(DEV)
    z, out = fresh.reconstruct(rows)
    torch.cuda.synchronize()
    fresh.release()
    return rows, z, out


@pytest.mark.parametrize("ae_form", ["FC", "compact"])
def test_ema_weights_puts_the_average_in_place_and_restores(ae_form):
    t = _six_steps(ae_form)
    eng = t["eng"]
    rows, z_want, out_want = _rows_forward_of_average(t)
    torch.cuda.synchronize()
    before = eng.arena.P.detach().clone()
    z_live, out_live = eng.reconstruct(rows)
    with eng.ema_weights():
        assert torch.equal(eng.arena.P.detach(), eng.ema_P)
        z, out = eng.reconstruct(rows)
        torch.cuda.synchronize()
    assert torch.equal(z, z_want) and torch.equal(out, out_want)
    assert not torch.equal(out, out_live)
    torch.cuda.synchronize()
    assert torch.equal(eng.arena.P.detach(), before)

    class Boom(Exception):
        pass
    with pytest.raises(Boom):
        with eng.ema_weights():
            raise Boom()
    torch.cuda.synchronize()
    assert torch.equal(eng.arena.P.detach(), before)
    z_again, out_again = eng.reconstruct(rows)
    assert torch.equal(out_again, out_live) and torch.equal(z_again, z_live)
    with pytest.raises(RuntimeError, match="ema_decay"):
        with t["twin"].ema_weights():
            pass


# ------------------------------------------------------------------------------------------------ 6. TrialBatch
def test_trial_batch_with_different_decays_is_bitwise_the_trials_alone():
    from rankaae_amd.trial_batch import TrialBatch
    cfg = _case_cfg("FC")
    spec, aux, _ = make_spectra(160, cfg["dim_in"], cfg["n_aux"], seed=6)
    decays, steps = [0.9, 0.99], 4
    alone = []
    for t, d in enumerate(decays):
        e = _engine(dict(cfg, ema_decay=d), 200 + t, spec, aux)
        e.set_epoch(_perm(160, 50 + t), 0.3)
        for _ in range(steps):
            e.step(32)
        torch.cuda.synchronize()
        alone.append((e.arena.P.detach().clone(), e.ema_P.clone()))
        e.release()
    shared = TrialBatch.shared_stream(DEV)
    engs = [_engine(dict(cfg, ema_decay=d), 200 + t, spec, aux, stream=shared) for t, d in enumerate(decays)]
    batch = TrialBatch(engs)                     # (a refused step would raise BatchingRefused below)
    for t, e in enumerate(engs):
        e.set_epoch(_perm(160, 50 + t), 0.3)
    for _ in range(steps):
        batch.step(32)
    torch.cuda.synchronize()
    assert batch.programs[(32, True)][1] is not None
    for t, e in enumerate(engs):
        assert torch.equal(e.arena.P.detach(), alone[t][0]), f"trial {t}: parameters"
        assert torch.equal(e.ema_P, alone[t][1]), f"trial {t}: average"
        assert not torch.equal(e.ema_P, e.arena.P.detach())
    batch.release()
    for e in engs:
        e.release()


def test_trial_batch_refuses_one_engine_with_the_key_and_one_without():
    from rankaae_amd.trial_batch import TrialBatch
    cfg = _case_cfg("FC")
    spec, aux, _ = make_spectra(96, cfg["dim_in"], cfg["n_aux"], seed=6)
    shared = TrialBatch.shared_stream(DEV)
    a = _engine(dict(cfg, ema_decay=0.9), 1, spec, aux, stream=shared)
    b = _engine(cfg, 2, spec, aux, stream=shared)
    with pytest.raises(ValueError, match="ema_decay"):
        TrialBatch([a, b])


def test_engine_state_carries_the_average_and_refuses_the_other_configuration():
    t = _six_steps("FC")
    state = t["eng"].state()
    assert torch.equal(state["ema"], t["eng"].ema_P.cpu()) and state["ema"].dtype == torch.float32
    assert "ema" not in t["twin"].state()
    cfg = t["cfg"]
    fresh = _engine(dict(cfg, ema_decay=0.9), 99, t["spec"], t["aux"])
    fresh.load_state(state)
    torch.cuda.synchronize()
    assert torch.equal(fresh.ema_P.cpu(), state["ema"]) and torch.equal(fresh.arena.P.detach().cpu(), state["arena"])
    plain = _engine(cfg, 99, t["spec"], t["aux"])
    with pytest.raises(ValueError, match="another configuration"):
        plain.load_state(state)
    with pytest.raises(ValueError, match="another configuration"):
        _engine(dict(cfg, ema_decay=0.9), 98, t["spec"], t["aux"]).load_state(t["twin"].state())


# ------------------------------------------------------------------------------------------------ 7. Trainer / train_sc
def _sc_cfg(**over):
    import test_resume_gpu as R
    return {**R.CFG, "max_epoch": 2, "checkpoint_every": 1, "data_file": "data.csv", "output_name": "report", "top_n": 1,
            "n_sampling": 20, **over}


def _state_dicts(path):
    mods = torch.load(path, map_location="cpu", weights_only=False)
    return mods, {f"{key}.{name}": t for key, mod in mods.items() for name, t in mod.state_dict().items()}


_sc = {}


def _sc_runs(tmp_path_factory):
    """``train_sc``'s ``run_training`` (one trial, two epochs, 96 spectra, batch 32) twice from the same seed: with
    ``ema_decay: 0.9`` and without.  Run once, shared, never changed."""
    if not _sc:
        import yaml
        from rankaae_amd.cmd import train_sc
        spec, aux, grid = make_spectra(96, 256, 2, seed=9)
        for name, over in (("with", {"ema_decay": 0.9}), ("without", {})):
            wd = tmp_path_factory.mktemp(f"ema_sc_{name}")
            cfg = _sc_cfg(**over)
            write_csv(str(wd / "data.csv"), spec, aux, grid)
            with open(wd / "cfg.yaml", "w") as f:
                yaml.safe_dump(cfg, f)
            torch.manual_seed(77)
            metrics, _ = train_sc.run_training(0, str(wd), Parameters(cfg), False, str(wd / "data.csv"))
            for lg in (logging.getLogger("subtraining_1"), logging.getLogger("losses_1")):
                for h in list(lg.handlers):         # the next run's trial 1 opens its own files
                    h.close()
                    lg.removeHandler(h)
            _sc[name] = dict(wd=wd, job=wd / "training" / "job_1", metrics=metrics, cfg=cfg)
    return _sc


def test_trainer_writes_final_ema_and_logs_one_line(tmp_path_factory):
    from rankaae_amd import resume as rf
    runs = _sc_runs(tmp_path_factory)
    job = runs["with"]["job"]
    mods, ema_sd = _state_dicts(job / "final_ema.pt")
    live_mods, live_sd = _state_dicts(job / "final.pt")
    assert list(mods) == ["Encoder", "Decoder", "Style Discriminator"] == list(live_mods)
    assert [type(m) for m in mods.values()] == [type(m) for m in live_mods.values()]
    assert all(type(m).__module__ == "rankaae_amd.model" for m in mods.values())
    # the parameters are the engine's average (its last state, in the finished resume file) in arena order:
    # discriminator, encoder, decoder, every tensor at a multiple of 64 floats
    st = torch.load(job / rf.NAME, weights_only=True)
    assert st["finished"] is True
    ema, arena, off = st["engine"]["ema"], st["engine"]["arena"], 0
    for key in ("Style Discriminator", "Encoder", "Decoder"):
        for (name, p), (_, q) in zip(mods[key].named_parameters(), live_mods[key].named_parameters()):
            assert torch.equal(p.detach().reshape(-1), ema[off:off + p.numel()]), (key, name)
            assert torch.equal(q.detach().reshape(-1), arena[off:off + p.numel()]), (key, name)
            off += (p.numel() + 63) // 64 * 64
    assert off == ema.numel() and not torch.equal(ema, arena)
    # the buffers are the live modules'
    names = {f"{key}.{n}" for key, m in mods.items() for n, _ in m.named_buffers()}
    assert names and any(n.endswith("running_var") for n in names)
    for n in names:
        assert torch.equal(ema_sd[n], live_sd[n]), n
    lines = [ln for ln in (job / "messages.txt").read_text().splitlines() if "EMA weights:" in ln]
    assert len(lines) == 1 and all(k in lines[0] for k in LOSS_KEYS)
    assert lines[0].split(":  ", 1)[1].startswith("EMA weights:")        # (after the logger's time stamp and level)


def test_final_pt_is_the_file_of_the_run_without_the_key(tmp_path_factory):
    runs = _sc_runs(tmp_path_factory)
    _, a = _state_dicts(runs["with"]["job"] / "final.pt")
    _, b = _state_dicts(runs["without"]["job"] / "final.pt")
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(a[k], b[k]), k
    assert runs["with"]["metrics"] == runs["without"]["metrics"]
    assert (runs["with"]["job"] / "losses.csv").read_bytes() == (runs["without"]["job"] / "losses.csv").read_bytes()
    job = runs["without"]["job"]
    assert not (job / "final_ema.pt").exists() and "EMA weights:" not in (job / "messages.txt").read_text()


# ------------------------------------------------------------------------------------------------ 8. resume
class _Abandon(Exception):
    pass


def _both_finals(wd):
    return {name: _state_dicts(os.path.join(wd, name))[1] for name in ("final.pt", "final_ema.pt")}


def _assert_same_files(got, want):
    for name in ("final.pt", "final_ema.pt"):
        assert got[name].keys() == want[name].keys()
        for k, v in want[name].items():
            assert torch.equal(got[name][k], v), (name, k)


def test_resumed_run_ends_where_the_uninterrupted_one_does(tmp_path):
    """One trial on its own stream with its own host generator (what ``trial_mode: threads`` runs per trial): four
    epochs straight against two epochs, a kill in epoch 2's callback (the file of epoch 1 stands), then ``resume``."""
    import test_resume_gpu as R
    cfg = R._cfg("FC", max_epoch=4, checkpoint_every=1, ema_decay=0.9)
    a = R._Trial(tmp_path / "a", cfg, R.SEED["FC"])
    a.trainer.train()
    a.close()
    want = _both_finals(tmp_path / "a")
    b = R._Trial(tmp_path / "b", cfg, R.SEED["FC"])

    def die(epoch, m):
        if epoch == 2:
            raise _Abandon()
    with pytest.raises(_Abandon):
        b.trainer.train(die)
    b.close()
    st = torch.load(tmp_path / "b" / R.rf.NAME, weights_only=True)
    assert st["epoch"] == 1 and "ema" in st["engine"] and st["fingerprint"]["cfg.ema_decay"] == 0.9
    assert not (tmp_path / "b" / "final_ema.pt").exists()
    c = R._Trial(tmp_path / "b", {**cfg, "resume": True}, R.SEED["FC"] + 1000)
    seen = []
    c.trainer.train(lambda epoch, m: seen.append(epoch))
    c.close()
    assert seen == [2, 3]
    _assert_same_files(_both_finals(tmp_path / "b"), want)
    d = R._Trial(tmp_path / "b", {**cfg, "resume": True, "ema_decay": 0.99}, R.SEED["FC"])
    with pytest.raises(ValueError, match="cfg.ema_decay"):
        d.trainer.train()
    d.close()


def test_resumed_batched_group_ends_where_the_uninterrupted_one_does(tmp_path):
    import test_resume_gpu as R
    from rankaae_amd.trainer import train_trials_batched
    cfg = R._cfg("FC", max_epoch=4, checkpoint_every=1, ema_decay=0.9)
    group = R._group(str(tmp_path), cfg, "a")
    train_trials_batched([t.trainer for t in group])
    want = [_both_finals(t.wd) for t in group]
    for t in group:
        t.close()
    group = R._group(str(tmp_path), cfg, "b")

    def die(epoch, m):
        if epoch == 2:
            raise _Abandon()
    with pytest.raises(_Abandon):
        train_trials_batched([t.trainer for t in group], callbacks=[die, None])
    dirs = [t.wd for t in group]
    for t in group:
        t.close()
    del group
    assert [R.rf.offered_epochs(d) for d in dirs] == [[1, 0], [1, 0]]
    group = R._group(str(tmp_path), {**cfg, "resume": True}, "b")
    train_trials_batched([t.trainer for t in group])
    for t, w in zip(group, want):
        _assert_same_files(_both_finals(t.wd), w)
        t.close()
    a, b = want[0]["final_ema.pt"], want[1]["final_ema.pt"]
    assert any(not torch.equal(a[k], b[k]) for k in a), "the two trials of the group are different trainings"


# ------------------------------------------------------------------------------------------------ 9. report
def test_generate_report_evaluates_either_file(tmp_path_factory):
    import yaml
    from rankaae_amd import report
    from rankaae_amd.cmd import generate_report
    runs = _sc_runs(tmp_path_factory)
    wd, cfg = runs["with"]["wd"], runs["with"]["cfg"]
    results = {}
    for kind in ("ema", "final"):
        with open(wd / f"report_{kind}.yaml", "w") as f:
            yaml.safe_dump({**cfg, "report_weights": kind, "output_name": f"report_{kind}"}, f)
        generate_report.main(["-c", f"report_{kind}.yaml", "-w", str(wd)])
        results[kind] = report.load_evaluations(str(wd / f"report_{kind}_model_evaluation.pkl"))
        assert list(results[kind]) == ["job_1"]
    a, b = results["ema"]["job_1"], results["final"]["job_1"]
    print(f"reconstruction error: final.pt {b['Reconstruct Err']}, final_ema.pt {a['Reconstruct Err']}")
    assert a["Reconstruct Err"] != b["Reconstruct Err"]
    wd2 = runs["without"]["wd"]
    with open(wd2 / "report_ema.yaml", "w") as f:
        yaml.safe_dump({**runs["without"]["cfg"], "report_weights": "ema"}, f)
    with pytest.raises(FileNotFoundError, match="job_1"):
        generate_report.main(["-c", "report_ema.yaml", "-w", str(wd2)])
    with open(wd2 / "report_bad.yaml", "w") as f:
        yaml.safe_dump({**runs["without"]["cfg"], "report_weights": "best"}, f)
    with pytest.raises(ValueError, match="report_weights"):
        generate_report.main(["-c", "report_bad.yaml", "-w", str(wd2)])
