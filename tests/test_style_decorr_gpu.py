"""``style_decorr`` on the GPU: the kernel (``raae_style_decorr_fwd_bwd``) against the float64 reference within bounds
that come from the number formats, its statistics block, determinism, refusals and batched form; the engine's phase B
with and without the key (hooked, captured, eager); batched trials; ``Trainer`` with resume; the one-rank data-parallel
rehearsal."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import decorr_reference as dr
import test_spec_shift_gpu as S
from rankaae_amd.synthetic import make_spectra

if torch.cuda.is_available():
    from rankaae_amd import _lib, ops
    DEV = torch.device("cuda:0")

ROWS = [1, 2, 3, 63, 64, 65, 257, 1027, 4099]
COLS = [1, 2, 5, 6, 16, 64]               # 64 with at most 257 rows
GUARD = 8                                 # guard elements on each side of dz and stats; 64 guard bytes around work
FILL = -777.25
D_TOL = 1e-10                             # |D - ref| <= D_TOL * max(1, |ref|): see test_kernel_matches_the_reference
_refs = {}


def _launches(b, k):
    return 1 if k == 1 or b * k <= 4096 else 2


def _ref(b, k):
    """Mixed Gaussian styles of one shape with their float64 penalty and gradient: computed once, shared, never changed."""
    if (b, k) not in _refs:
        z = dr.mixed_gaussian(b, k, seed=1000 * b + k)
        _refs[(b, k)] = (z, dr.penalty(z), dr.gradient(z))
    return _refs[(b, k)]


def _prefill(b, ld, seed):
    """Random non-zero fp32 values of magnitudes from 1e-3 to 1.  With the larger weight of the kernel test the added
    term (0.01 to 0.3) is then as large as the prefill or larger, and an ulp of the sum is 1e-7 of it or less: the
    bound holds the gradient itself to seven digits.  No smaller: where the gradient is mathematically zero (two rows:
    every correlation is +-1) the double evaluation still leaves an ABSOLUTE residue of up to about
    w * k * 2^-53 * sum_j |M_ij| |x_j| <= 300 * 1e-15 * 4 / min s_i = 8e-12 for these inputs, which an ulp of the
    smallest prefill (6e-11) has to cover because 1e-9 of a zero gradient covers nothing."""
    rng = np.random.default_rng(seed)
    v = rng.choice([-1.0, 1.0], size=(b, ld)) * 10.0 ** rng.uniform(-3.0, 0.0, size=(b, ld))
    return v.astype(np.float32)


class _Call:
    """Guarded device buffers of one ``(z, ld)``: ``z`` with NaN in its padding columns, ``dz`` prefilled (padding
    included), ``work`` and ``stats``."""

    def __init__(self, z, ld, seed=0):
        self.b, self.k, self.ld = z.shape[0], z.shape[1], ld
        b, k = self.b, self.k
        zp = np.full((b, ld), np.nan, dtype=np.float32)
        zp[:, :k] = z
        self.z = torch.from_numpy(zp).to(DEV).reshape(-1)
        self.pre = _prefill(b, ld, seed)
        self.n = b * ld
        self.dz_buf = torch.full((GUARD + self.n + GUARD,), FILL, device=DEV)
        self.dz = self.dz_buf[GUARD:GUARD + self.n]
        self.wb = ops.style_decorr_work_bytes(b, k)
        self.work_buf = torch.full((64 + self.wb + 64,), 0xA5, dtype=torch.uint8, device=DEV)
        self.work = self.work_buf[64:64 + self.wb]
        self.stats_buf = torch.full((GUARD + 3 + GUARD,), FILL, dtype=torch.float64, device=DEV)
        self.stats = self.stats_buf[GUARD:GUARD + 3]
        self.reset()

    def reset(self):
        self.dz.copy_(torch.from_numpy(self.pre).reshape(-1))
        self.stats.zero_()

    def run(self, w):
        ops.style_decorr(self.z, self.ld, self.b, self.k, w, self.work, self.stats, self.dz, self.ld)
        torch.cuda.synchronize()
        return self.dz.cpu().numpy().reshape(self.b, self.ld).copy(), self.stats.cpu().numpy().copy()

    def guards_intact(self):
        dz, st, wk = self.dz_buf.cpu(), self.stats_buf.cpu(), self.work_buf.cpu()
        return (bool((dz[:GUARD] == FILL).all()) and bool((dz[GUARD + self.n:] == FILL).all()) and
                bool((st[:GUARD] == FILL).all()) and bool((st[GUARD + 3:] == FILL).all()) and
                bool((wk[:64] == 0xA5).all()) and bool((wk[64 + self.wb:] == 0xA5).all()))


def _check(call, got, stats, w, d_ref, g_ref):
    """The two bounds; returns the largest share of each that was used."""
    b, k = call.b, call.k
    d_share = abs(stats[0] - d_ref) / (D_TOL * max(1.0, abs(d_ref)))
    assert d_share <= 1.0, (b, k, stats[0], d_ref)
    add = w * g_ref
    want = (call.pre[:, :k].astype(np.float64) + add).astype(np.float32)
    tol = np.spacing(np.abs(want)).astype(np.float64) + 1e-9 * np.abs(add)
    err = np.abs(got[:, :k].astype(np.float64) - want.astype(np.float64))
    share = float((err / tol).max())
    assert share <= 1.0, (b, k, call.ld, w, float(err.max()), int(err.argmax()))
    assert np.array_equal(got[:, k:].view(np.int32), call.pre[:, k:].view(np.int32))      # the padding of dz
    assert call.guards_intact()
    return d_share, share


# ------------------------------------------------------------------------------------------------ 1. the kernel
@pytest.mark.parametrize("b", ROWS)
def test_kernel_matches_the_float64_reference(b):
    """Both bounds come from the formats, not from the kernel.  ``D``: double sums over at most 4099 terms carry about
    5e-13 of relative error; 1e-10 leaves room for sums that are not centred first, which the inputs' mean / deviation
    ratio (at most 10) would amplify by at most 100.  ``dz``: one fp32 rounding of the exact sum -- an ulp of the wanted
    value -- plus 1e-9 of the added term for the double arithmetic behind it.  With w = 300 the added term is as large
    as the prefill (``_prefill``), so the ulp holds the gradient itself to seven digits; an fp32 statistic of these
    inputs (means of up to ten deviations) is good to five at best."""
    worst_d = worst = 0.0
    for k in COLS:
        if k == 64 and b > 257:
            continue
        z, d_ref, g_ref = _ref(b, k)
        for ld in (k, k + 3):
            call = _Call(z, ld, seed=b + ld)
            for w in (0.5, 300.0):
                call.reset()
                got, stats = call.run(w)
                d_share, share = _check(call, got, stats, w, d_ref, g_ref)
                worst_d, worst = max(worst_d, d_share), max(worst, share)
                if b > 1 and k > 1:         # (two rows: every correlation is +-1, D = 1 and the gradient vanishes)
                    assert stats[0] > 0.0 and (b == 2 or not np.array_equal(got[:, :k], call.pre[:, :k]))
                else:                                   # D = 0 and dz untouched, bit for bit
                    assert stats[0] == 0.0 and np.array_equal(got.view(np.int32), call.pre.view(np.int32))
            print(f"b {b} k {k} ld {ld} ({_launches(b, k)} launch(es)): D {stats[0]:.6f}, |D - ref| / bound {d_share:.2e}, "
                  f"max dz err / bound {share:.3f}")
    print(f"b {b}: worst share of the D bound {worst_d:.2e}, of the dz bound {worst:.3f}")


@pytest.mark.parametrize("b,k", [(65, 5), (1027, 5)])
def test_crafted_columns(b, k):
    """A constant column (no gradient: its dz keeps its bits), two identical columns, and an all-zero z (D = 0, nothing
    written, nothing that is not finite) -- in the one-launch and the two-launch form."""
    z = _ref(b, k)[0].copy()
    z[:, 1] = np.float32(0.3)
    z[:, 4] = z[:, 0]
    for zz in (z, np.zeros((b, k), dtype=np.float32)):
        call = _Call(zz, k + 3, seed=7)
        got, stats = call.run(0.5)
        assert np.isfinite(stats).all() and np.isfinite(got).all()
        d_share, share = _check(call, got, stats, 0.5, dr.penalty(zz), dr.gradient(zz))
        assert np.array_equal(got[:, 1].view(np.int32), call.pre[:, 1].view(np.int32))
        print(f"b {b} k {k}: D {stats[0]:.6f}, D share {d_share:.2e}, dz share {share:.3f}")
    assert stats[0] == 0.0 and np.array_equal(got.view(np.int32), call.pre.view(np.int32))


@pytest.mark.parametrize("b,k", [(64, 6), (1027, 6)])
def test_statistics_accumulate_zero_weight_and_repeats(b, k):
    z, d_ref, _ = _ref(b, k)
    call = _Call(z, k, seed=3)
    first, s1 = call.run(0.5)
    _, s2 = call.run(0.5)
    _, s3 = call.run(0.5)
    assert s1[0] == s2[0] == s3[0] and s1[2] == 1.0 and s2[2] == 2.0 and s3[2] == 3.0
    assert s2[1] == s1[0] + s1[0] and s3[1] == (s1[0] + s1[0]) + s1[0]
    # a repeated call on the same input gives the same bits
    call.reset()
    again, s4 = call.run(0.5)
    assert np.array_equal(again.view(np.int32), first.view(np.int32)) and s4[0] == s1[0] and s4[2] == 1.0
    # w = 0 is legal: the statistics are written, dz keeps its bits
    call.reset()
    zero, s5 = call.run(0.0)
    assert np.array_equal(zero.view(np.int32), call.pre.view(np.int32)) and s5[0] == s1[0] and s5[2] == 1.0
    assert call.guards_intact()


@pytest.mark.parametrize("case", ["k_65", "k_0", "ldz_small", "lddz_small", "w_nan", "w_inf", "b_0"])
def test_kernel_refuses_bad_arguments_before_a_launch(case):
    lib = _lib.load()
    b, k = 64, 6
    call = _Call(_ref(b, k)[0], 70)                        # (room for a k of up to 65 had the call gone through)
    args = dict(ldz=70, b=b, k=k, w=0.5, lddz=70)
    args.update({"k_65": dict(k=65), "k_0": dict(k=0), "ldz_small": dict(ldz=5), "lddz_small": dict(lddz=5),
                 "w_nan": dict(w=float("nan")), "w_inf": dict(w=float("inf")), "b_0": dict(b=0)}[case])
    assert lib.raae_record_begin() == 0
    try:
        rc = lib.raae_style_decorr_fwd_bwd(C.c_void_p(call.z.data_ptr()), args["ldz"], args["b"], args["k"], args["w"],
                                           C.c_void_p(call.work.data_ptr()), C.c_void_p(call.stats.data_ptr()),
                                           C.c_void_p(call.dz.data_ptr()), args["lddz"],
                                           C.c_void_p(torch.cuda.current_stream().cuda_stream))
    finally:
        h, count = C.c_void_p(), C.c_int(-1)
        assert lib.raae_record_end(C.byref(h), C.byref(count)) == 0
        lib.raae_record_free(h)
    torch.cuda.synchronize()
    assert rc == -1 and count.value == 0                   # RAAE_EINVAL, and the recorder saw no launch
    assert np.array_equal(call.dz.cpu().numpy().view(np.int32), call.pre.reshape(-1).view(np.int32))
    assert not call.stats.cpu().numpy().any() and call.guards_intact()
    if case in ("k_65", "k_0", "b_0"):
        assert ops.style_decorr_work_bytes(args["b"], args["k"]) == 0


# ------------------------------------------------------------------------------------------------ 2. batched form
@pytest.mark.parametrize("b,k", [(65, 6), (1027, 6)])
def test_batched_planes_are_bitwise_the_single_calls(b, k):
    """Three recorded trials of one shape with their own weight and styles, replayed as one ``gridDim.z = 3`` program."""
    lib = _lib.load()
    ws = [0.5, 2.0, 0.125]
    calls = [_Call(dr.mixed_gaussian(b, k, seed=40 + t), k + 3, seed=50 + t) for t in range(3)]
    single = [c.run(w) for c, w in zip(calls, ws)]
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    handles = (C.c_void_p * 3)()
    with torch.cuda.stream(stream):
        for t, (c, w) in enumerate(zip(calls, ws)):
            c.reset()
            assert lib.raae_record_begin() == 0
            try:
                ops.style_decorr(c.z, c.ld, b, k, w, c.work, c.stats, c.dz, c.ld)
            finally:
                h, count = C.c_void_p(), C.c_int(0)
                rc = lib.raae_record_end(C.byref(h), C.byref(count))
            assert rc == 0 and count.value == _launches(b, k)
            handles[t] = h
        stream.synchronize()
        for c in calls:
            c.reset()
            c.work_buf.fill_(0xA5)
        prog = C.c_void_p()
        rc = lib.raae_multi_build(handles, 3, C.byref(prog))
        for h in handles:
            lib.raae_record_free(C.c_void_p(h))
        assert rc == 0
        assert lib.raae_multi_launch(prog, C.c_void_p(stream.cuda_stream)) == 0
        stream.synchronize()
        lib.raae_multi_free(prog)
    for t, c in enumerate(calls):
        got, stats = c.dz.cpu().numpy().reshape(b, c.ld), c.stats.cpu().numpy()
        assert np.array_equal(got.view(np.int32), single[t][0].view(np.int32)), f"plane {t}"
        assert np.array_equal(stats, single[t][1]) and stats[2] == 1.0 and c.guards_intact(), f"plane {t}"
    assert single[0][1][0] != single[1][1][0]


# ------------------------------------------------------------------------------------------------ 3. the engine
W = 0.5
_stepped = {}


def _hooked(cfg, spec, aux):
    """Three steps of an engine with a phase hook at "correlation": phase B's styles, the gradient the encoder's backward
    pass was given, and the loss slots of phases A and B at that point."""
    eng = S._engine(cfg, 21, spec, aux)
    seen = []

    def hook(name, P):
        if name == "correlation":
            torch.cuda.synchronize()
            seen.append((P.enc.styles.cpu().clone(), P.dstyles.cpu().clone(), eng.loss_out[:2].cpu().clone()))
    eng.phase_hook = hook
    eng.set_epoch(S._perm(192, 30), 0.3)
    for _ in range(3):
        eng.step(64)
    torch.cuda.synchronize()
    return eng, seen


def _plain(cfg, spec, aux, use_graph=True):
    eng = S._engine(cfg, 21, spec, aux, use_graph=use_graph)
    eng.set_epoch(S._perm(192, 30), 0.3)
    for _ in range(3):
        eng.step(64)
    torch.cuda.synchronize()
    return dict(eng=eng, P=eng.arena.P.detach().cpu().clone(), losses=eng.losses())


def _three_steps(ae_form):
    """192 spectra, 64 rows, three steps from the same weights and seed: hooked engines without and with the key; the key
    ``null`` and absent (captured); the key set, captured and eager.  Run once per network, shared, never changed."""
    if ae_form not in _stepped:
        cfg = S._case_cfg(ae_form)
        spec, aux, _ = make_spectra(192, cfg["dim_in"], cfg["n_aux"], seed=4)
        on = dict(cfg, style_decorr=W)
        t = dict(cfg=cfg, hook_off=_hooked(cfg, spec, aux), hook_on=_hooked(on, spec, aux),
                 null=_plain(dict(cfg, style_decorr=None), spec, aux), absent=_plain(cfg, spec, aux),
                 graph=_plain(on, spec, aux), eager=_plain(on, spec, aux, use_graph=False))
        t["stats"] = t["hook_on"][0].style_decorr_stats(reset=False)
        _stepped[ae_form] = t
    return _stepped[ae_form]


@pytest.mark.parametrize("ae_form", ["FC", "compact"])
def test_phase_b_gradient_gains_the_weighted_reference_gradient(ae_form):
    """First step, same weights: phase A is untouched, so both engines see the same phase-B styles, bit for bit, and the
    same adversarial and rank loss slots (``D`` enters no loss; the later phases' slots follow phase B's update, which
    the key changes, so they cannot be compared).  ``dstyles`` with the key is ``dstyles`` without it plus
    ``0.5 * g_ref(styles)``, within one fp32 ulp plus 1e-9 of the added term."""
    t = _three_steps(ae_form)
    (z0, d0, l0), (z1, d1, l1) = t["hook_off"][1][0], t["hook_on"][1][0]
    assert torch.equal(S._bits(z0), S._bits(z1)) and torch.equal(S._bits(l0), S._bits(l1))
    add = W * dr.gradient(z1.numpy())
    want = (d0.numpy().astype(np.float64) + add).astype(np.float32)
    tol = np.spacing(np.abs(want)).astype(np.float64) + 1e-9 * np.abs(add)
    err = np.abs(d1.numpy().astype(np.float64) - want.astype(np.float64))
    print(f"{ae_form}: max |w g| {np.abs(add).max():.3e}, max |dstyles| {np.abs(want).max():.3e}, "
          f"max err / bound {(err / tol).max():.3f}")
    assert np.all(err <= tol) and np.abs(add).max() > 0.0
    assert not torch.equal(d0, d1)


@pytest.mark.parametrize("ae_form", ["FC", "compact"])
def test_statistics_are_the_mean_penalty_of_the_steps(ae_form):
    t = _three_steps(ae_form)
    eng, seen = t["hook_on"]
    ds = [dr.penalty(z.numpy()) for z, _, _ in seen]
    mean, steps = t["stats"]
    print(f"{ae_form}: D of the three steps {ds}, engine mean {mean!r}")
    assert steps == 3 and abs(mean - sum(ds) / 3.0) <= D_TOL
    with pytest.raises(RuntimeError, match="style_decorr"):
        t["absent"]["eng"].style_decorr_stats()


@pytest.mark.parametrize("ae_form", ["FC", "compact"])
def test_key_absent_or_null_is_the_engine_that_never_heard_of_it(ae_form):
    t = _three_steps(ae_form)
    a, b = t["null"], t["absent"]
    assert a["eng"].style_decorr is None and b["eng"].style_decorr is None and a["eng"].decorr_stats is None
    assert torch.equal(S._bits(a["P"]), S._bits(b["P"]))
    assert all(a["losses"][k] == b["losses"][k] for k in S.LOSS_KEYS)


@pytest.mark.parametrize("ae_form", ["FC", "compact"])
def test_captured_steps_are_bitwise_the_eager_ones_and_cost_one_launch(ae_form):
    t = _three_steps(ae_form)
    a, b = t["graph"], t["eager"]
    assert a["eng"].plans[64].graphs[True] is not None and b["eng"].plans[64].graphs[True] is None
    assert torch.equal(S._bits(a["P"]), S._bits(b["P"]))
    assert all(a["losses"][k] == b["losses"][k] for k in S.LOSS_KEYS)
    assert all(np.isfinite(a["losses"][k]) for k in S.LOSS_KEYS)
    assert not torch.equal(a["P"], t["absent"]["P"])                         # the key changes the training
    if "launches" not in t:
        counts = []
        for name in ("graph", "absent"):
            e = t[name]["eng"]
            e.set_epoch(S._perm(192, 40), 0.3)
            counts.append(S._count_launches(e, 64))
        t["launches"] = counts
    with_key, without = t["launches"]
    print(f"{ae_form}: {with_key} launches per step with style_decorr, {without} without")
    # without the key: the count the step had before the key existed (DESIGN.md section 9 records it for the parent
    # commits: 97 for the dense networks, 136 for the conv networks at 64 rows); with it, one more
    assert without == {"FC": 97, "compact": 136}[ae_form] and with_key == without + 1


@pytest.mark.parametrize("over", [dict(fused_blocks=False), dict(overlap_min_batch=32)],
                         ids=["per_layer", "branched"])
def test_other_step_forms_capture_the_launch_too(over):
    """The conv network without its fused blocks, and the branched graph (side streams from 32 rows on): captured and
    eager steps with the key agree bit for bit, and the penalty ran in every step."""
    cfg = dict(S._case_cfg("compact"), style_decorr=W, **over)
    spec, aux, _ = make_spectra(192, cfg["dim_in"], cfg["n_aux"], seed=4)
    a, b = _plain(cfg, spec, aux), _plain(cfg, spec, aux, use_graph=False)
    assert torch.equal(S._bits(a["P"]), S._bits(b["P"]))
    for run in (a, b):
        mean, steps = run["eng"].style_decorr_stats()
        assert steps == 3 and 0.0 < mean < 1.0
        run["eng"].release()


# ------------------------------------------------------------------------------------------------ 4. TrialBatch
def test_trial_batch_with_different_weights_is_bitwise_the_trials_alone():
    from rankaae_amd.trial_batch import TrialBatch
    cfg = dict(S._case_cfg("FC"), batch_size=32)
    spec, aux, _ = make_spectra(160, cfg["dim_in"], cfg["n_aux"], seed=6)
    ws, steps = [0.5, 3.0], 3
    alone = []
    for t, w in enumerate(ws):
        e = S._engine(dict(cfg, style_decorr=w), 200 + t, spec, aux)
        e.set_epoch(S._perm(160, 50 + t), 0.3)
        for _ in range(steps):
            e.step(32)
        torch.cuda.synchronize()
        alone.append((e.arena.P.detach().clone(), e.style_decorr_stats()))
        e.release()
    shared = TrialBatch.shared_stream(DEV)
    engs = [S._engine(dict(cfg, style_decorr=w), 200 + t, spec, aux, stream=shared) for t, w in enumerate(ws)]
    batch = TrialBatch(engs)                     # (a refused step would raise BatchingRefused below)
    for t, e in enumerate(engs):
        e.set_epoch(S._perm(160, 50 + t), 0.3)
    for _ in range(steps):
        batch.step(32)
    torch.cuda.synchronize()
    assert batch.programs[(32, True)][1] is not None
    for t, e in enumerate(engs):
        assert torch.equal(S._bits(e.arena.P.detach()), S._bits(alone[t][0])), f"trial {t}: parameters"
        assert e.style_decorr_stats() == alone[t][1] and alone[t][1][1] == steps, f"trial {t}: statistics"
    assert not torch.equal(alone[0][0], alone[1][0])
    batch.release()
    for e in engs:
        e.release()


# ------------------------------------------------------------------------------------------------ 5. Trainer
def test_trainer_logs_the_penalty_and_leaves_the_loss_file_alone(tmp_path):
    """Two epochs, ``compact``, 64 rows (140 training rows: two batches of 64 and a ragged one of 12), with the key and
    without it from the same seed."""
    import test_resume_gpu as R
    messages, losses, metrics = {}, {}, {}
    for name, over in (("with", {"style_decorr": 0.5}), ("without", {})):
        cfg = R._cfg("compact", max_epoch=2, batch_size=64, **over)
        t = R._Trial(tmp_path / name, cfg, R.SEED["compact"])
        log, handler = S._messages_logger(t.wd, f"decorr_{name}")
        t.trainer.logger = log
        metrics[name] = t.trainer.train()
        handler.close()
        log.removeHandler(handler)
        messages[name] = open(os.path.join(t.wd, "messages.txt")).read().splitlines()
        losses[name] = open(os.path.join(t.wd, "losses.csv")).read().splitlines()
        t.close()
    lines = [ln for ln in messages["with"] if "style_decorr" in ln]
    assert len(lines) == 3 and "style_decorr: w = 0.5" in lines[0]
    for epoch in (0, 1):
        head, _, rest = lines[1 + epoch].partition(f"Epoch {epoch}: style_decorr: mean D = ")
        value, _, tail = rest.partition(" over ")
        assert rest and 0.0 < float(value) < 1.0 and tail == "3 steps", lines[1 + epoch]
    assert not any("style_decorr" in ln for ln in messages["without"])
    assert losses["with"][0] == losses["without"][0] and len(losses["with"]) == len(losses["without"])
    assert [len(r.split(",")) for r in losses["with"]] == [len(r.split(",")) for r in losses["without"]]
    assert all(np.isfinite(m) for m in metrics["with"])
    # two epochs prove nothing about it: printed, not asserted
    print(f"validation max |inter-style correlation| after two epochs: {metrics['with'][3]:.4f} with style_decorr, "
          f"{metrics['without'][3]:.4f} without")


class _Abandon(Exception):
    pass


def test_resumed_run_ends_where_the_uninterrupted_one_does(tmp_path):
    """Three epochs straight against a kill in epoch 2's callback (the file of epoch 1 stands), then ``resume``."""
    import test_resume_gpu as R
    cfg = R._cfg("FC", max_epoch=3, checkpoint_every=1, batch_size=64, style_decorr=0.5)
    a = R._Trial(tmp_path / "a", cfg, R.SEED["FC"])
    a.trainer.train()
    a.close()
    want = R._final(tmp_path / "a")
    b = R._Trial(tmp_path / "b", cfg, R.SEED["FC"])

    def die(epoch, m):
        if epoch == 2:
            raise _Abandon()
    with pytest.raises(_Abandon):
        b.trainer.train(die)
    b.close()
    st = torch.load(tmp_path / "b" / R.rf.NAME, weights_only=True)
    assert st["epoch"] == 1 and st["fingerprint"]["cfg.style_decorr"] == 0.5
    c = R._Trial(tmp_path / "b", {**cfg, "resume": True}, R.SEED["FC"] + 1000)
    seen = []
    c.trainer.train(lambda epoch, m: seen.append(epoch))
    c.close()
    assert seen == [2]
    got = R._final(tmp_path / "b")
    assert got.keys() == want.keys()
    for k, v in want.items():
        assert torch.equal(got[k], v), k
    d = R._Trial(tmp_path / "b", {**cfg, "resume": True, "style_decorr": 1.0}, R.SEED["FC"])
    with pytest.raises(ValueError, match="cfg.style_decorr"):
        d.trainer.train()
    d.close()


# ------------------------------------------------------------------------------------------------ 6. data parallel
def test_dp_path_one_rank_equals_plain():
    """The data-parallel code path over a one-rank RCCL group (``tests/test_dp_gpu.py``): each rank penalises its own
    rows and there is no collective for it, so the engine told ``world_size=2`` is bitwise the plain engine."""
    import torch.distributed as dist
    from rankaae_amd.engine import StepEngine
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29647")
    if not dist.is_initialized():
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda:0"))
    try:
        cfg = dict(S._case_cfg("FC"), style_decorr=W)
        spec, aux, _ = make_spectra(192, cfg["dim_in"], cfg["n_aux"], seed=4)
        results = []
        for world in (1, 2):
            eng = StepEngine(*S._modules(cfg, 21), cfg, DEV, rng_mode="philox", seed=9, use_graph=True, world_size=world,
                             rank=0)
            eng.set_data(spec, aux)
            eng.set_epoch(S._perm(192, 30), 0.3)
            for _ in range(3):
                eng.step(64)
            torch.cuda.synchronize()
            results.append((eng.arena.P.detach().clone(), eng.losses(), eng.style_decorr_stats()))
            eng.close()
    finally:
        dist.destroy_process_group()
    assert torch.equal(S._bits(results[0][0]), S._bits(results[1][0]))
    assert results[0][1] == results[1][1] and results[0][2] == results[1][2] and results[0][2][1] == 3


def _global_pairs_worker(rank, world, port):
    """One rank of two (gloo, ``tests/test_partial_labels_dp_gpu.py``'s start-up): the same first step without the key and
    with it, from the same weights and seed, ``rank_loss_pairs: global``."""
    import test_partial_labels_dp_gpu as D
    dist = D._begin(rank, world, port)
    seen = {}
    for name, over in (("off", {}), ("on", {"style_decorr": W})):
        g, cfg, spec, aux, n_train, _ = D._data(world, frac=0, **over)
        eng = D._engine(g, cfg, spec, aux, n_train, rank, world, use_graph=False)
        assert eng.rank_pairs_global and eng.world_size == 2 and not eng.aux_missing

        def hook(phase, P, name=name):
            if phase == "correlation":
                seen[name] = (P.enc.styles.cpu().clone(), P.dstyles.cpu().clone())
        eng.phase_hook = hook
        eng.step(cfg["batch_size"])
        torch.cuda.synchronize()
        if name == "on":
            mean, steps = eng.style_decorr_stats()
            assert steps == 1 and abs(mean - dr.penalty(seen["on"][0].numpy())) <= D_TOL       # this rank's rows alone
        eng.close()
    (z0, d0), (z1, d1) = seen["off"], seen["on"]
    assert torch.equal(S._bits(z0), S._bits(z1))
    add = W * dr.gradient(z1.numpy())                   # the local styles' penalty, NOT times the world size
    want = (d0.numpy().astype(np.float64) + add).astype(np.float32)
    tol = np.spacing(np.abs(want)).astype(np.float64) + 1e-9 * np.abs(add)
    err = np.abs(d1.numpy().astype(np.float64) - want.astype(np.float64))
    scaled = np.abs(d1.numpy().astype(np.float64) - (d0.numpy().astype(np.float64) + world * add))
    print(f"rank {rank}: max |w g| {np.abs(add).max():.3e}, max err / bound {(err / tol).max():.3f}; against the term "
          f"times W: {(scaled / tol).max():.3e} bounds")
    assert np.all(err <= tol)
    assert (scaled / tol).max() > 1e3                   # (the test tells the two apart)
    D._end(dist)


def test_global_pairs_add_the_term_unscaled():
    """Two gloo ranks on the one GPU, ``rank_loss_pairs: global``: the rank loss's gradient carries the factor ``W`` of
    the averaged gradients, the decorrelation term does not -- ``dstyles`` with the key is ``dstyles`` without it plus
    ``w * g_ref`` of the rank's OWN styles, within the kernel's bound."""
    import test_partial_labels_dp_gpu as D
    D._spawn(_global_pairs_worker)
