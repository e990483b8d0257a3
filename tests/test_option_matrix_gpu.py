"""The training step with every option on at once (configuration ``C`` of ``option_matrix_reference``): clipping, the
moving average, both augmentations, one of three optimizer rules, the anomaly check and NaN labels -- each option's own
file switches on that option alone.

1. every option still does, in ``C``, what its own float64 reference says (batch, rank loss, every update, average);
2. taking one option out of ``C`` changes only what that option does, bit for bit;
3. eager, captured and replayed steps agree bit for bit, and ``C`` costs the launches its options' own tests count;
4. two trials with ``C`` in one ``TrialBatch`` are the trials alone;
5. ``state()`` / ``load_state()`` carry ``C`` over an epoch boundary;
6. two data-parallel ranks with global pairs;
7. a NaN spectrum met in ``C``.

No tolerance is new: each is the one of the option's own test (named where it is used)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import ema_reference
import option_matrix_reference as om
from partial_label_reference import masked_rank_loss
from rankaae_amd.synthetic import make_spectra

if torch.cuda.is_available():
    import test_grad_clip_gpu as G
    import test_partial_labels_dp_gpu as D
    import test_partial_labels_gpu as PL
    import test_spec_broaden_gpu as B
    import test_spec_shift_gpu as S
    from rankaae_amd.engine import OPT_NAMES
    DEV = torch.device("cuda:0")

FORMS = {"FC": "fc_small", "compact": "compact_small"}


def _perm(n, seed):
    return torch.randperm(n, generator=torch.Generator().manual_seed(seed))


def _rows64(ae_form, **over):
    """``C`` on 700 spectra (489 train), 64 rows, NaN labels: ``(cfg, spec, aux with gaps, aux as drawn)``."""
    cfg = om.combined(G._case_cfg(FORMS[ae_form], batch_size=64), **over)
    spec, aux, _ = make_spectra(700, 256, cfg["n_aux"], seed=3)
    return cfg, spec, om.with_missing_labels(aux), aux


def _rows256(ae_form, **over):
    """``C`` at the 256-row schedule: the 1600 spectra (1120 train) of ``test_grad_clip_gpu._rows256``, NaN labels."""
    cfg, spec, aux = G._rows256(ae_form)
    return om.combined(cfg, **over), spec, om.with_missing_labels(aux), aux


def _outcome(e):
    """Everything the bitwise tests compare: state (arena, BatchNorm buffers, moments), losses, counts of clipped steps,
    ``{norm, scale}`` and the average (None where the engine has not got the key)."""
    losses = e.losses()
    return dict(state=G._state(e), losses=losses, counts=e.clipped_steps(),
                stats=e.clip_stats.cpu().clone() if e.grad_clip is not None else None,
                ema=e.ema_P.cpu().clone() if e.ema_decay is not None else None)


def _same(a, b, what, but=()):
    for x, y in zip(a["state"], b["state"]):
        assert torch.equal(x, y), f"{what}: state"
    assert a["losses"] == b["losses"], (what, a["losses"], b["losses"])
    for k in ("counts", "stats", "ema"):
        if k in but:
            continue
        same = (a[k] == b[k]) if k == "counts" else torch.equal(S._bits(a[k]), S._bits(b[k]))
        assert same, f"{what}: {k}"


def _run(cfg, seed, spec, aux, steps, use_graph=True, perm_seed=3):
    eng, n_train = G._engine(cfg, seed, spec, aux, use_graph=use_graph)
    eng.set_epoch(_perm(n_train, perm_seed), 0.3)
    for _ in range(steps):
        eng.step(cfg["batch_size"])
    out = _outcome(eng)
    out["anomaly"] = eng.anomaly()
    eng.release()
    return out


# ------------------------------------------------------------------------------------------------ 1. float64 references
CASES = [("AdamW", True, None), ("AdamW", False, 2), ("RAdam", True, 2), ("RAdam", False, None),
         ("AdaBound", True, None), ("AdaBound", False, None)]


@pytest.mark.parametrize("rule,detect,plain_step", CASES)
@pytest.mark.parametrize("ae_form", ["FC", "compact"])
def test_every_option_follows_its_float64_reference(ae_form, rule, detect, plain_step):
    """Three eager steps of ``C`` (``plain_step``: that step runs without the smoothness phase, so its last update is
    phase D's), hooks on every update.  Per step: the batch against ``broaden_reference`` (bound:
    ``test_spec_broaden_gpu.test_engine_batch_is_the_reference_applied_to_the_gathered_rows``), the gathered ``aux`` bit
    for bit; the kendall loss against ``masked_rank_loss`` of the styles of phase B (``test_partial_labels_gpu``: 1e-5
    relative + 1e-7); every update teacher-forced through ``clip_reference`` with the rule's own state
    (``test_grad_clip_gpu``: 2e-6 relative + 2e-7, norm and scale 2^-23); the average against ``ema_reference.ema_run``
    over the snapshots behind each step's last update (``test_ema_gpu``: k single-step bounds after step k).  Both
    forms of the update with a scale (checked with ``detect``, unchecked without) are reached for every rule."""
    cfg, spec, aux, _ = _rows64(ae_form, optimizer_name=rule, detect_anomaly=detect, pair_unused_forwards=False)
    eng, n_train = G._engine(cfg, 5, spec, aux, use_graph=False)
    assert (eng.grad_clip, eng.ema_decay, eng.spec_shift, eng.spec_broaden) == (om.CLIP, om.EMA, om.SHIFT, om.BROADEN)
    assert eng.aux_missing and eng.detect_anomaly == detect and eng.fused_begin and eng.rng_mode == "philox"
    perm = _perm(n_train, 1)
    assert om.every_batch_has_a_gap(aux[:n_train], perm.numpy(), 64, 3)
    K, noise = cfg["n_aux"], float(cfg["spec_noise"])
    table, before, bad, worst = {}, {}, [], {}
    want_counts = {n: 0 for n in OPT_NAMES}
    steps = [dict() for _ in range(3)]
    now = {"k": 0, "last": None}

    def note(what, value):
        worst[what] = max(worst.get(what, -np.inf), value)

    def pre(name, P):
        o, st = eng.opts[name], steps[now["k"]]
        seg = P.seg[name][o.lo // 64:o.hi // 64].long().repeat_interleave(64)
        grad = G._slab_sum(eng.G[:, o.lo:o.hi], seg, P.max_slab[name] > 16)
        before[name] = (eng.arena.P[o.lo:o.hi].detach().cpu().clone(), o.m.cpu().clone(), o.v.cpu().clone(), (seg > 0).cpu(),
                        grad.cpu())
        if name == "adversarial":           # the step's first update: the batch every phase of the step reads
            st["spec"], st["aux"] = P.spec.cpu().clone(), P.aux.cpu().clone()
        if name == "correlation":           # phase B's styles and loss, before later phases reuse the buffers
            st["styles"], st["kendall"] = P.enc.out.detach().cpu().double().numpy().copy(), float(eng.loss_out[1])

    def post(name, P):
        o = eng.opts[name]
        p0, m0, v0, keep, grad = before[name]
        flat = eng.G_flat[o.lo:o.hi].cpu()
        p1, m1, v1 = eng.arena.P[o.lo:o.hi].detach().cpu(), o.m.cpu(), o.v.cpu()
        stats = eng.clip_stats[o.index].cpu().tolist()
        if name == now["last"]:             # behind the step's last update: what the average is about to take
            steps[now["k"]]["snap"] = eng.arena.P.detach().cpu().clone()
        try:
            assert torch.equal(flat[keep], grad[keep]), "the flat gradient is not the captured slabs in the update's order"
            par, m, v, norm, scale = om.teacher_forced_update(table, name, rule, o.hyper.cpu().tolist(), p0[keep], m0[keep],
                                                              v0[keep], grad[keep], om.CLIP)
            want_counts[name] += scale < 1.0
            assert abs(stats[0] - norm) <= om.STAT_RTOL * norm and abs(stats[1] - scale) <= om.STAT_RTOL * scale, (norm, scale, stats)
            assert torch.equal(p1[~keep], p0[~keep]) and torch.equal(m1[~keep], m0[~keep])
            for what, got, want in (("params", p1, par), ("exp_avg", m1, m), ("exp_avg_sq", v1, v)):
                x = om.update_ratio(got[keep], want)
                note(f"{what} err / tol", x)
                assert x <= 1.0, f"{what}: {x:.3f} of the tolerance 2e-6 relative + 2e-7"
        except AssertionError as e:
            bad.append(f"step {now['k'] + 1} {name}: {e}")
    eng.phase_hook, eng.post_phase_hook = pre, post
    eng.set_epoch(perm, 0.3)
    torch.cuda.synchronize()
    ema0 = eng.ema_P.cpu().clone()
    assert torch.equal(ema0, eng.arena.P.detach().cpu())
    emas = []
    for k in range(3):
        smooth = plain_step != k + 1
        now["k"], now["last"] = k, "smoothness" if smooth else "mutual_info"
        eng.step(64, smooth=smooth)
        torch.cuda.synchronize()
        emas.append(eng.ema_P.cpu().clone())
        assert int(eng.rng_state[0].item()) == k + 1
    losses = eng.losses()
    # -- the batch and the rank loss
    data, labels = eng.train_spec.cpu(), eng.train_aux.cpu()
    zeros = torch.zeros(64, eng.L, device=DEV)
    for k, st in enumerate(steps, start=1):
        idx = perm[64 * (k - 1):64 * k]
        rows = data[idx].numpy()
        term = B._head_at(eng, k, zeros, noise)[2].cpu().double().numpy()
        got = st["spec"].numpy()
        ref = om.batch(rows, eng.seed, k, om.BROADEN, om.SHIFT, term)
        tol = om.batch_bound(rows, eng.seed, k, om.BROADEN, om.SHIFT, got, term)
        err = np.abs(got.astype(np.float64) - ref)
        note("batch err / bound", float((err / tol).max()))
        if not np.all(err <= tol):
            bad.append(f"step {k}: batch: max |err| {err.max():.3e}, err / bound {(err / tol).max():.3f}")
        if not float(np.abs(got - (rows + term)).max()) > 1e-3:
            bad.append(f"step {k}: the rows were not augmented")
        if not torch.equal(S._bits(st["aux"]), S._bits(labels[idx])) or not bool(torch.isnan(st["aux"]).any()):
            bad.append(f"step {k}: the gathered aux rows are not the data set's, NaN cells included")
        lref, _ = masked_rank_loss(st["aux"].numpy(), st["styles"][:, :K], cfg["kendall_activation"])
        note("kendall err / tol", abs(st["kendall"] - lref) / (om.RANK_RTOL * abs(lref) + om.RANK_ATOL))
        if not abs(st["kendall"] - lref) <= om.RANK_RTOL * abs(lref) + om.RANK_ATOL:
            bad.append(f"step {k}: kendall {st['kendall']!r}, reference {lref!r}")
    assert losses["kendall"] == steps[-1]["kendall"]
    # -- the average
    refs = ema_reference.ema_run(ema0, [st["snap"] for st in steps], om.EMA)
    big = ema0.double().abs()
    for k, (ref, st, got) in enumerate(zip(refs, steps, emas), start=1):
        big = torch.maximum(big, st["snap"].double().abs())
        err, bound = (got.double() - ref).abs(), k * ema_reference.step_bound(big, big)
        note("ema err / bound", float((err / bound.clamp_min(1e-300)).max()))
        if float((err - bound).max()) > 0:
            bad.append(f"step {k}: average: max excess {float((err - bound).max()):.3e} at {int((err - bound).argmax())}")
        if k == 3 and not torch.equal(st["snap"], eng.arena.P.detach().cpu()):
            bad.append("the last snapshot is not the arena the step left")
    assert not torch.equal(emas[-1], ema0)
    print(f"{ae_form} {rule} detect={detect} plain step {plain_step}: " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))
    assert not bad, "\n".join(bad)
    # -- clipping happened, and the counters say what the reference's scales say
    counts = eng.clipped_steps()
    assert counts == [want_counts[n] for n in OPT_NAMES] and sum(counts) > 0, (counts, want_counts)
    assert len(table) == 5
    assert eng.anomaly() is None
    eng.release()


# ------------------------------------------------------------------------------------------------ 2. one option out
@pytest.mark.parametrize("use_graph", [False, True])
@pytest.mark.parametrize("ae_form", ["FC", "compact"])
def test_taking_one_option_out_changes_only_what_it_does(ae_form, use_graph, monkeypatch):
    cfg, spec, aux, full = _rows256(ae_form)
    c = _run(cfg, 3, spec, aux, 3, use_graph)
    assert sum(c["counts"]) > 0 and c["anomaly"] is None and not torch.equal(c["ema"], c["state"][0].cpu())
    # the average
    out = _run(om.combined(cfg, ema_decay=...), 3, spec, aux, 3, use_graph)
    assert out["ema"] is None
    _same(c, out, "without ema_decay", but=("ema",))
    # clipping that never clips
    never = _run(om.combined(cfg, grad_clip_norm=1e30), 3, spec, aux, 3, use_graph)
    out = _run(om.combined(cfg, grad_clip_norm=...), 3, spec, aux, 3, use_graph)
    assert never["counts"] == [0] * 5 and never["stats"][:, 1].tolist() == [1.0] * 5 and out["counts"] is None
    _same(never, out, "grad_clip_norm 1e30 / absent", but=("counts", "stats"))
    assert not torch.equal(never["state"][0], c["state"][0])
    # the anomaly check
    _same(c, _run(om.combined(cfg, detect_anomaly=False), 3, spec, aux, 3, use_graph), "detect_anomaly off")
    # fully labelled data: the unmasked kernels, nothing else moved
    logs, runs = {}, {}
    for name, labels in (("full", full), ("part", aux)):
        eng, n_train = G._engine(cfg, 3, spec, labels, use_graph=False)
        assert eng.aux_missing == (name == "part")

        def go():
            eng.set_epoch(_perm(n_train, 3), 0.3)
            for _ in range(3):
                eng.step(256)
        logs[name] = PL._entry_points(monkeypatch, go)
        runs[name] = _outcome(eng)
        eng.release()
    assert not [n for n in logs["full"] if "masked" in n] and logs["full"].count("rank_loss_fwd_bwd") == 3
    assert logs["part"].count("rank_loss_masked_fwd_bwd") == 3 and "rank_loss_fwd_bwd" not in logs["part"]
    assert [n.replace("_masked", "") for n in logs["part"]] == logs["full"]
    _same(runs["full"], _run(cfg, 3, spec, full, 3, use_graph), "fully labelled")
    _same(runs["part"], c, "the logged run")


# ------------------------------------------------------------------------------------------------ 3. capture and replay
@pytest.mark.parametrize("ae_form", ["FC", "compact"])
def test_eager_captured_and_replayed_steps_agree_and_cost_their_options_launches(ae_form):
    cfg, spec, aux, _ = _rows256(ae_form)
    eager = _run(cfg, 4, spec, aux, 4, use_graph=False)
    graph = _run(cfg, 4, spec, aux, 4, use_graph=True)
    _same(eager, graph, "eager / captured and replayed")
    assert sum(eager["counts"]) > 0
    # launches: tests/test_ema_gpu.py counts one for the average, tests/test_spec_broaden_gpu.py one for the augmentation
    # (both keys together); the plain step here is C's without those keys
    EMA_LAUNCHES = AUGMENT_LAUNCHES = 1
    n = {}
    for name, over in (("C", {}), ("no average", dict(ema_decay=...)), ("no augmentation", dict(spec_shift=..., spec_broaden=...)),
                       ("neither", dict(ema_decay=..., spec_shift=..., spec_broaden=...))):
        eng, n_train = G._engine(om.combined(cfg, **over), 4, spec, aux, use_graph=True)
        eng.set_epoch(_perm(n_train, 3), 0.3)
        eng.step(256)
        n[name] = S._count_launches(eng, 256)
        eng.release()
    print(f"{ae_form}: launches per 256-row step {n}")
    assert n["C"] == n["neither"] + EMA_LAUNCHES + AUGMENT_LAUNCHES
    assert n["no average"] == n["neither"] + AUGMENT_LAUNCHES and n["no augmentation"] == n["neither"] + EMA_LAUNCHES


# ------------------------------------------------------------------------------------------------ 4. TrialBatch
@pytest.mark.parametrize("ae_form", ["FC", "compact"])
def test_trial_batch_with_everything_on_is_bitwise_the_trials_alone(ae_form):
    from rankaae_amd.trial_batch import TrialBatch
    cfg, spec, aux, _ = _rows256(ae_form)
    keys = [dict(ema_decay=om.EMA, spec_broaden=om.BROADEN, spec_shift=om.SHIFT),
            dict(ema_decay=0.99, spec_broaden=0.4, spec_shift=0.5)]
    T, bs, steps = 2, 256, 4
    alone = []
    for t in range(T):
        e, n_train = G._engine(om.combined(cfg, **keys[t]), 200 + t, spec, aux)
        e.set_epoch(_perm(n_train, 50 + t), 0.3)
        for _ in range(steps):
            e.step(bs)
        alone.append(_outcome(e))
        e.release()
    shared = TrialBatch.shared_stream(DEV)
    engs = [G._engine(om.combined(cfg, **keys[t]), 200 + t, spec, aux, stream=shared)[0] for t in range(T)]
    batch = TrialBatch(engs)
    for t, e in enumerate(engs):
        e.set_epoch(_perm(n_train, 50 + t), 0.3)
    for _ in range(steps):
        batch.step(bs)
    assert batch.programs[(bs, True)][1] is not None
    for t, e in enumerate(engs):
        _same(alone[t], _outcome(e), f"trial {t}")
    assert not torch.equal(alone[0]["stats"], alone[1]["stats"]), "each trial has its own scale"
    assert not torch.equal(alone[0]["ema"], alone[1]["ema"]), "each trial has its own average"
    assert sum(alone[0]["counts"]) > 0 and sum(alone[1]["counts"]) > 0
    batch.release()
    for e in engs:
        e.release()


# ------------------------------------------------------------------------------------------------ 5. state round trip
@pytest.mark.parametrize("ae_form", ["FC", "compact"])
def test_state_round_trip_carries_everything(ae_form):
    """An epoch of 2 steps, ``state()``, a fresh engine (other weights, other seed) that loads it, then an epoch of 2
    steps on both: bit for bit.  (``state()`` is taken between epochs: the row cursor and the epoch's loss accumulator
    are ``set_epoch``'s.)  An engine without ``grad_clip_norm`` or without ``ema_decay`` refuses the state, as in
    ``tests/test_ema_gpu.py``; the augmentation keys travel in the resume file's fingerprint
    (``test_option_matrix_cpu.py``)."""
    cfg, spec, aux, _ = _rows64(ae_form)
    first, n_train = G._engine(cfg, 7, spec, aux)
    first.set_epoch(_perm(n_train, 1), 0.3)
    for _ in range(2):
        first.step(64)
    first.losses()
    state = first.state()
    assert "clip_counts" in state and "ema" in state and sum(state["clip_counts"].tolist()) > 0
    second, _ = G._engine(cfg, 99, spec, aux)
    second.load_state(state)
    for e in (first, second):
        e.set_epoch(_perm(n_train, 2), 0.3)
        for _ in range(2):
            e.step(64)
    a, b = _outcome(first), _outcome(second)
    _same(a, b, "resumed")
    assert sum(a["counts"]) > sum(state["clip_counts"].tolist()) and not torch.equal(a["ema"], state["ema"])
    for key in ("grad_clip_norm", "ema_decay"):
        other, _ = G._engine(om.combined(cfg, **{key: ...}), 98, spec, aux)
        with pytest.raises(ValueError, match="another configuration"):
            other.load_state(state)
        other.release()
    first.release()
    second.release()


# ------------------------------------------------------------------------------------------------ 6. two ranks
def _two_rank_worker(rank, world, port):
    dist = D._begin(rank, world, port)
    cfg, spec, aux, _ = _rows64("FC", rank_loss_pairs="global")
    b = cfg["batch_size"] // world
    cfg["batch_size"] = b
    eng, n_train = G._engine(cfg, 5 + rank, spec, aux, use_graph=True, world_size=world, rank=rank)
    assert eng.aux_missing and eng.rank_pairs_global and eng.ema_decay == om.EMA and eng.spec_broaden == om.BROADEN
    K, seen = cfg["n_aux"], []

    def hook(name, P):
        if name == "correlation":           # phase B's gathered batch and loss, before later phases reuse the buffers
            seen.append((P.aux_all.cpu().numpy().copy(), P.z_all.cpu().numpy().copy(), float(eng.loss_out[1])))
    eng.phase_hook = hook
    eng.set_epoch(_perm(n_train, 2), 0.3, start=rank * b, stride=world * b)
    for _ in range(3):
        eng.step(b)
    torch.cuda.synchronize()
    eng.losses()
    assert len(seen) == 3
    for d, z, loss in seen:
        assert d.shape == (world * b, K) and np.isnan(d).any() and not np.isnan(d).all(axis=0).any()
        lref, _ = masked_rank_loss(d, z[:, :K], cfg["kendall_activation"])
        print(f"rank {rank}: kendall {loss!r} reference {lref!r}")
        assert abs(loss - lref) <= om.RANK_RTOL * abs(lref) + om.RANK_ATOL, (loss, lref)
    mine = (eng.arena.P.detach().cpu(), [o.m.cpu() for o in eng.opts.values()], [o.v.cpu() for o in eng.opts.values()],
            eng.ema_P.cpu(), eng.clip_stats.cpu(), eng.clipped_steps(), np.float32(seen[-1][2]).tobytes())
    box = [None] * world
    dist.all_gather_object(box, mine)
    for other in box[1:]:
        assert torch.equal(box[0][0], other[0]), "ranks hold different parameters"
        assert all(torch.equal(x, y) for x, y in zip(box[0][1] + box[0][2], other[1] + other[2])), "different moments"
        assert torch.equal(box[0][3], other[3]), "ranks hold different averages"
        assert torch.equal(box[0][4], other[4]) and box[0][5] == other[5], "different {norm, scale} or counts"
        assert box[0][6] == other[6], "the ranks' losses differ"
    assert sum(box[0][5]) > 0 and not torch.equal(box[0][3], box[0][0])
    D._end(dist)


def test_two_ranks_with_everything_on_stay_alike():
    """Two gloo ranks on the one GPU (fresh child processes, killed after ``WORKER_SECONDS``), ``C`` with global pairs on
    the NaN-labelled data, 3 steps: identical arena, moments, average, ``{norm, scale}`` and counts; the kendall loss of
    every step is ``masked_rank_loss`` of the gathered batch."""
    D._spawn(_two_rank_worker)


# ------------------------------------------------------------------------------------------------ 7. a NaN met in C
@pytest.mark.parametrize("ae_form", ["FC", "compact"])
def test_nan_spectrum_is_named_and_not_counted_as_a_clipped_step(ae_form):
    """One NaN in a training row that step 2 gathers: phase A's gradient is the first to hold it, so ``anomaly()`` answers
    ``("adversarial", 2)``; every norm from there on is NaN and no update counts as clipped; the same run on the clean row
    reports nothing and goes on counting."""
    cfg, spec, aux, _ = _rows64(ae_form)
    n_train = G.ref_train.split_rows(len(spec))[0]
    perm = _perm(n_train, 1)
    bad = spec.copy()
    bad[int(perm[64 + 5]), 100] = np.nan
    assert int(perm[64 + 5]) not in perm[:64].tolist()
    out = {}
    for name, rows in (("clean", spec), ("nan", bad)):
        eng, _ = G._engine(cfg, 5, rows, aux)
        eng.set_epoch(perm, 0.3)
        counts = []
        for _ in range(3):
            eng.step(64)
            counts.append(eng.clipped_steps())
        eng.losses()
        out[name] = (counts, eng.anomaly(), eng.nan_flags.tolist())
        eng.release()
    print(out)
    assert out["clean"][1] is None and out["clean"][2] == [0] * 5
    assert out["nan"][1] == ("adversarial", 2) and out["nan"][2][0] == 2
    assert out["nan"][0][0] == out["clean"][0][0] and sum(out["clean"][0][0]) > 0
    assert out["nan"][0][2] == out["clean"][0][0], "a NaN norm was counted as a clipped step"
    assert sum(out["clean"][0][2]) > sum(out["clean"][0][0])
