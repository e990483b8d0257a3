"""``rank_loss_form: logistic`` on the GPU: the kernel (``raae_rank_logistic_fwd_bwd``) against the float64 reference
within bounds that come from the number formats (``rank_logistic_reference``), against the linear kernel where the
sigmoid is exactly one half, its determinism, batched form and refusals; the engine's phase B with and without the keys
(hooked, captured, eager); batched trials; ``Trainer`` with resume; the one-rank data-parallel rehearsal."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import rank_logistic_reference as rl
import test_spec_shift_gpu as S
from rankaae_amd.synthetic import make_spectra

if torch.cuda.is_available():
    from rankaae_amd import _lib, ops
    DEV = torch.device("cuda:0")

ROWS = [2, 3, 8, 9, 33, 255, 256, 257, 1027, 4099]
TEMPS = [0.05, 1.0, 20.0]
GUARD = 8                                 # guard elements on each side of dz and loss; 64 guard bytes around work
FILL = -777.25
_refs = {}


def _n_aux_of(B):
    """16 descriptors up to 257 rows, 4099 rows with 5 only."""
    return [5] if B > 1027 else [1, 3, 5, 6] if B > 257 else [1, 3, 5, 6, 16]


def _ref(B, n_aux, T):
    """The inputs of one shape and their float64 evaluation at the fp32 value of ``T``: computed once, shared, never
    changed."""
    if (B, n_aux) not in _refs:
        _refs[(B, n_aux)] = rl.make_inputs(B, n_aux, n_aux + 1, n_aux + 2, seed=1000 * B + n_aux)
    d, z = _refs[(B, n_aux)]
    if (B, n_aux, T) not in _refs:
        _refs[(B, n_aux, T)] = rl.evaluate(d, z, n_aux, rl.temperature_f32(T))
    return d, z, _refs[(B, n_aux, T)]


class _Call:
    """Guarded device buffers of one ``(d, z)``: ``dz [B, lddz]``, ``loss`` and ``work`` with guards around them."""

    def __init__(self, d, z, n_aux, lddz=None):
        self.B, self.n_aux, self.ldd, self.ldz = d.shape[0], n_aux, d.shape[1], z.shape[1]
        self.lddz = n_aux + 3 if lddz is None else lddz
        self.d, self.z = torch.from_numpy(d).to(DEV), torch.from_numpy(z).to(DEV)
        self.n = self.B * self.lddz
        self.dz_buf = torch.empty(GUARD + self.n + GUARD, device=DEV)
        self.dz = self.dz_buf[GUARD:GUARD + self.n]
        self.loss_buf = torch.empty(GUARD + 1 + GUARD, device=DEV)
        self.loss = self.loss_buf[GUARD:GUARD + 1]
        self.wb = ops.rank_logistic_work_bytes(self.B, n_aux)
        self.work_buf = torch.empty(64 + self.wb + 64, dtype=torch.uint8, device=DEV)
        self.work = self.work_buf[64:64 + self.wb]
        self.reset()

    def reset(self):
        self.dz_buf.fill_(FILL)
        self.loss_buf.fill_(FILL)
        self.work_buf.fill_(0xA5)

    def launch(self, T):
        ops.rank_logistic_fwd_bwd(self.d, self.ldd, self.z, self.ldz, self.B, self.n_aux, T, self.work, self.loss, self.dz,
                                  self.lddz)

    def read(self):
        torch.cuda.synchronize()
        return self.dz.cpu().numpy().reshape(self.B, self.lddz).copy(), float(self.loss.cpu()[0])

    def run(self, T):
        self.launch(T)
        return self.read()

    def guards_intact(self):
        dz, ls, wk = self.dz_buf.cpu(), self.loss_buf.cpu(), self.work_buf.cpu()
        return (bool((dz[:GUARD] == FILL).all()) and bool((dz[GUARD + self.n:] == FILL).all()) and
                bool((ls[:GUARD] == FILL).all()) and bool((ls[GUARD + 1:] == FILL).all()) and
                bool((wk[:64] == 0xA5).all()) and bool((wk[64 + self.wb:] == 0xA5).all()))

    def untouched(self):
        return (self.guards_intact() and bool((self.dz.cpu() == FILL).all()) and bool((self.loss.cpu() == FILL).all()) and
                bool((self.work.cpu() == 0xA5).all()))


def _check(ref, B, d, got, loss):
    """The two bounds and the exact zeros; returns the largest share of each bound that was used."""
    n_aux = ref["n_aux"]
    dz_bound, loss_bound = rl.bounds(ref, B)
    assert np.isfinite(got).all() and np.isfinite(loss)
    err = np.abs(got[:, :n_aux].astype(np.float64) - ref["dz"])
    share = float((err / dz_bound).max())
    loss_share = abs(loss - ref["loss"]) / loss_bound
    assert share <= 1.0, (B, n_aux, ref["T"], float(err.max()), int(err.argmax()))
    assert loss_share <= 1.0, (B, n_aux, ref["T"], loss, ref["loss"], loss_bound)
    assert (got[:, n_aux:] == 0.0).all()                                     # the padding of dz
    assert (got[:, :n_aux][~np.isfinite(d[:, :n_aux])] == 0.0).all()         # rows without a label for k
    assert loss >= 0.0
    return share, loss_share


# ------------------------------------------------------------------------------------------------ 1. the kernel
@pytest.mark.parametrize("T", TEMPS)
@pytest.mark.parametrize("B", ROWS)
def test_kernel_matches_the_float64_reference(B, T):
    """``|dz - ref| <= f 2^-24 (E + J A) + spacing(ref)`` per element and the same for the loss on its own sums
    (``rank_logistic_reference``): the bounds follow from the formats and the documented error of ``expf`` and
    ``log1pf``, not from the kernel.  ``ldd = n_aux + 1``, ``ldz = n_aux + 2`` with NaN in the padding of ``z``,
    ``lddz = n_aux + 3``.  The largest shares seen on an MI355X are recorded in DESIGN.md section 2."""
    worst = worst_loss = 0.0
    for n_aux in _n_aux_of(B):
        d, z, ref = _ref(B, n_aux, T)
        call = _Call(d, z, n_aux)
        got, loss = call.run(T)
        share, loss_share = _check(ref, B, d, got, loss)
        assert call.guards_intact()
        worst, worst_loss = max(worst, share), max(worst_loss, loss_share)
        if B >= 33 and n_aux >= 2:
            assert ref["m"][n_aux - 1] == 1 and not got[:, n_aux - 1].any()      # one labelled row: no pair
    print(f"B {B} T {T}: largest share of the dz bound {worst:.3f}, of the loss bound {worst_loss:.3f}")


# ------------------------------------------------------------------------------------------------ 2. the linear kernel
@pytest.mark.parametrize("B", [257, 1027])
def test_huge_temperature_is_half_the_linear_gradient(B):
    """``T = 2^40`` on fully labelled data: ``sigma`` is one half on every pair, so ``dz`` is half of
    ``raae_rank_loss_fwd_bwd``'s with ``activate = 0`` (which drops pairs of equal styles: the styles here are distinct)."""
    n_aux = 5
    rng = np.random.default_rng(B)
    d = (np.round(rng.standard_normal((B, n_aux)) * 4.0) / 4.0).astype(np.float32)
    z = rng.standard_normal((B, n_aux)).astype(np.float32)
    assert all(np.unique(z[:, k]).size == B for k in range(n_aux))
    call = _Call(d, z, n_aux, lddz=n_aux)
    got, loss = call.run(2.0 ** 40)
    work = torch.empty(ops.rank_loss_work_bytes(B, n_aux), dtype=torch.uint8, device=DEV)
    lin, lin_loss = torch.full((B, n_aux), FILL, device=DEV), torch.zeros(1, device=DEV)
    ops.rank_loss_fwd_bwd(call.d, n_aux, call.z, n_aux, B, n_aux, False, work, lin_loss, lin)
    torch.cuda.synchronize()
    want = 0.5 * lin.cpu().numpy().astype(np.float64)
    err = np.abs(got.astype(np.float64) - want)
    print(f"B {B}: max |dz - lin / 2| in ulps {(err / np.spacing(np.abs(want).astype(np.float32))).max():.2f}")
    assert np.abs(want).max() > 0.0 and (err <= 2.0 * np.spacing(np.abs(want).astype(np.float32))).all()
    assert call.guards_intact()


# ------------------------------------------------------------------------------------------------ 3. replay, batched, refusals
@pytest.mark.parametrize("B,n_aux", [(257, 3), (1027, 6), (4099, 5)])
def test_two_calls_give_the_same_bits(B, n_aux):
    d, z, _ = _ref(B, n_aux, 1.0)
    call = _Call(d, z, n_aux)
    first, l1 = call.run(1.0)
    call.reset()
    again, l2 = call.run(1.0)
    assert np.array_equal(first.view(np.int32), again.view(np.int32)) and l1 == l2 and call.guards_intact()


@pytest.mark.parametrize("B,n_aux", [(65, 3), (1027, 6)])
def test_batched_planes_are_bitwise_the_single_calls(B, n_aux):
    """Three recorded trials of one shape with their own temperature and data, replayed as one ``gridDim.z = 3``
    program."""
    lib = _lib.load()
    calls = [_Call(*rl.make_inputs(B, n_aux, n_aux + 1, n_aux + 2, seed=40 + t), n_aux) for t in range(3)]
    single = [c.run(T) for c, T in zip(calls, TEMPS)]
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    handles = (C.c_void_p * 3)()
    with torch.cuda.stream(stream):
        for t, (c, T) in enumerate(zip(calls, TEMPS)):
            assert lib.raae_record_begin() == 0
            try:
                c.launch(T)
            finally:
                h, count = C.c_void_p(), C.c_int(0)
                rc = lib.raae_record_end(C.byref(h), C.byref(count))
            assert rc == 0 and count.value == 2                  # (at most two launches, each with a batched form)
            handles[t] = h
        stream.synchronize()
        for c in calls:
            c.reset()
        prog = C.c_void_p()
        rc = lib.raae_multi_build(handles, 3, C.byref(prog))
        for h in handles:
            lib.raae_record_free(C.c_void_p(h))
        assert rc == 0
        assert lib.raae_multi_launch(prog, C.c_void_p(stream.cuda_stream)) == 0
        stream.synchronize()
        lib.raae_multi_free(prog)
    for t, c in enumerate(calls):
        got, loss = c.read()
        assert np.array_equal(got.view(np.int32), single[t][0].view(np.int32)) and loss == single[t][1], f"plane {t}"
        assert c.guards_intact(), f"plane {t}"
    assert single[0][1] != single[1][1]


@pytest.mark.parametrize("case", ["B_1", "n_aux_0", "n_aux_17", "ldd_small", "ldz_small", "lddz_small", "d_null", "z_null",
                                  "work_null", "loss_null", "dz_null", "T_0", "T_negative", "T_nan", "T_inf", "T_tiny"])
def test_kernel_refuses_bad_arguments_before_a_launch(case):
    lib = _lib.load()
    B, n_aux = 64, 6
    d, z = rl.make_inputs(B, 16, 20, 20, seed=3)                # (room for 17 descriptors had the call gone through)
    call = _Call(d, z, 16, lddz=20)
    a = dict(d=call.d.data_ptr(), ldd=20, z=call.z.data_ptr(), ldz=20, B=B, n_aux=n_aux, T=1.0, work=call.work.data_ptr(),
             loss=call.loss.data_ptr(), dz=call.dz.data_ptr(), lddz=20)
    a.update({"B_1": dict(B=1), "n_aux_0": dict(n_aux=0), "n_aux_17": dict(n_aux=17), "ldd_small": dict(ldd=5),
              "ldz_small": dict(ldz=5), "lddz_small": dict(lddz=5), "d_null": dict(d=None), "z_null": dict(z=None),
              "work_null": dict(work=None), "loss_null": dict(loss=None), "dz_null": dict(dz=None), "T_0": dict(T=0.0),
              "T_negative": dict(T=-1.0), "T_nan": dict(T=float("nan")), "T_inf": dict(T=float("inf")),
              "T_tiny": dict(T=1e-60)}[case])
    assert lib.raae_record_begin() == 0
    try:
        rc = lib.raae_rank_logistic_fwd_bwd(C.c_void_p(a["d"]), a["ldd"], C.c_void_p(a["z"]), a["ldz"], a["B"], a["n_aux"],
                                            a["T"], C.c_void_p(a["work"]), C.c_void_p(a["loss"]), C.c_void_p(a["dz"]),
                                            a["lddz"], C.c_void_p(torch.cuda.current_stream().cuda_stream))
    finally:
        h, count = C.c_void_p(), C.c_int(-1)
        assert lib.raae_record_end(C.byref(h), C.byref(count)) == 0
        lib.raae_record_free(h)
    torch.cuda.synchronize()
    assert rc == -1 and count.value == 0                         # RAAE_EINVAL, and the recorder saw no launch
    assert call.untouched()
    if case in ("B_1", "n_aux_0", "n_aux_17"):
        assert ops.rank_logistic_work_bytes(a["B"], a["n_aux"]) == 0


# ------------------------------------------------------------------------------------------------ 4. the engine
T_ENG = 0.5
STEPS = (64, 64, 32)                      # 160 rows: two batches of 64 and a ragged one
_stepped = {}


def _run(cfg, spec, aux, use_graph=True, hook=False):
    eng = S._engine(cfg, 21, spec, aux, use_graph=use_graph)
    seen = []
    if hook:
        def on_phase(name, P):
            if name == "correlation":
                torch.cuda.synchronize()
                seen.append((P.aux.cpu().clone(), P.enc.styles.cpu().clone(), P.dstyles.cpu().clone(),
                             float(eng.loss_out[1].cpu())))
        eng.phase_hook = on_phase
    eng.set_epoch(S._perm(160, 30), 0.3)
    for b in STEPS:
        eng.step(b)
    torch.cuda.synchronize()
    return dict(eng=eng, seen=seen, P=eng.arena.P.detach().cpu().clone(), losses=eng.losses())


def _three_steps(ae_form):
    """160 spectra, steps of 64, 64 and 32 rows from the same weights and seed: the keys absent (twice) and ``linear``;
    ``logistic`` hooked, captured and eager.  Run once per network, shared, never changed."""
    if ae_form not in _stepped:
        cfg = S._case_cfg(ae_form)
        spec, aux, _ = make_spectra(160, cfg["dim_in"], cfg["n_aux"], seed=4)
        on = dict(cfg, rank_loss_form="logistic", rank_temperature=T_ENG)
        _stepped[ae_form] = dict(cfg=cfg, on=on, spec=spec, aux=aux, absent=_run(cfg, spec, aux), absent2=_run(cfg, spec, aux),
                                 linear=_run(dict(cfg, rank_loss_form="linear"), spec, aux),
                                 hook=_run(on, spec, aux, hook=True), graph=_run(on, spec, aux),
                                 eager=_run(on, spec, aux, use_graph=False))
    return _stepped[ae_form]


@pytest.mark.parametrize("ae_form", ["FC", "compact"])
def test_keys_absent_is_the_engine_that_never_heard_of_them(ae_form):
    t = _three_steps(ae_form)
    a, b, c = t["absent"], t["absent2"], t["linear"]
    assert a["eng"].rank_loss_form == "linear" and a["eng"].rank_temperature is None
    for other in (b, c):
        assert torch.equal(S._bits(a["P"]), S._bits(other["P"]))
        assert all(a["losses"][k] == other["losses"][k] for k in S.LOSS_KEYS)
    if "launches" not in t:
        counts = []
        for name in ("absent", "graph"):
            e = t[name]["eng"]
            e.set_epoch(S._perm(160, 40), 0.3)
            counts.append(S._count_launches(e, 64))
        t["launches"] = counts
    without, with_key = t["launches"]
    print(f"{ae_form}: {without} launches per step without the keys, {with_key} with rank_loss_form: logistic")
    # without the keys: the count of the parent commit (97 for the dense networks, 136 for the
    # conv networks at 64 rows); the logistic form is two launches in the place of the linear form's two
    assert without == {"FC": 97, "compact": 136}[ae_form] and with_key == without


@pytest.mark.parametrize("ae_form", ["FC", "compact"])
def test_phase_b_is_the_reference_within_the_kernel_bounds(ae_form):
    """Every step, the ragged one included: the gradient the encoder's backward pass is given and the rank-loss slot
    are the float64 reference of the step's own descriptors and styles, within the bounds of the kernel test."""
    t = _three_steps(ae_form)
    n_aux = t["cfg"]["n_aux"]
    assert len(t["hook"]["seen"]) == 3
    for (aux, z, dz, loss), b in zip(t["hook"]["seen"], STEPS):
        assert aux.shape[0] == z.shape[0] == dz.shape[0] == b
        ref = rl.evaluate(aux.numpy(), z.numpy(), n_aux, rl.temperature_f32(T_ENG))
        share, loss_share = _check(ref, b, aux.numpy(), dz.numpy(), loss)
        print(f"{ae_form} rows {b}: loss {loss:.6f}, share of the dz bound {share:.3f}, of the loss bound {loss_share:.3f}")
        assert np.abs(ref["dz"]).max() > 0.0
    assert not torch.equal(t["hook"]["P"], t["absent"]["P"])                  # the key changes the training


@pytest.mark.parametrize("ae_form", ["FC", "compact"])
def test_captured_steps_are_bitwise_the_eager_and_the_hooked_ones(ae_form):
    t = _three_steps(ae_form)
    a, b, c = t["graph"], t["eager"], t["hook"]
    assert a["eng"].plans[64].graphs[True] is not None and b["eng"].plans[64].graphs[True] is None
    for other in (b, c):
        assert torch.equal(S._bits(a["P"]), S._bits(other["P"]))
        assert all(a["losses"][k] == other["losses"][k] for k in S.LOSS_KEYS)
    assert all(np.isfinite(a["losses"][k]) for k in S.LOSS_KEYS) and a["losses"]["kendall"] > 0.0


@pytest.mark.parametrize("ae_form", ["FC", "compact"])
def test_it_runs_with_decorrelation_missing_labels_and_clipping(ae_form):
    t = _three_steps(ae_form)
    cfg = dict(t["on"], style_decorr=0.5, grad_clip_norm=0.05)
    aux = np.array(t["aux"], copy=True)
    aux[::3, 0] = float("nan")
    aux[5, :] = float("nan")
    a, b = _run(cfg, t["spec"], aux, hook=True), _run(cfg, t["spec"], aux, use_graph=False)
    assert a["eng"].aux_missing and torch.equal(S._bits(a["P"]), S._bits(b["P"]))
    assert all(a["losses"][k] == b["losses"][k] and np.isfinite(a["losses"][k]) for k in S.LOSS_KEYS)
    assert torch.isfinite(a["P"]).all() and a["eng"].style_decorr_stats()[1] == 3
    assert len(a["eng"].clipped_steps()) > 0
    for aux_b, z, dz, loss in a["seen"]:               # (dstyles carries the decorrelation term too: finite is the claim)
        assert torch.isnan(aux_b).any() and torch.isfinite(dz).all() and np.isfinite(loss) and loss > 0.0
    for run in (a, b):
        run["eng"].release()


@pytest.mark.parametrize("ae_form", ["FC", "compact"])
def test_validation_is_the_linear_engines(ae_form):
    """The validation pass does not follow the form: from the same weights a ``logistic`` engine and a ``linear`` one
    give the same validation losses, bit for bit, eager and captured."""
    t = _three_steps(ae_form)
    vs, va, _ = make_spectra(96, t["cfg"]["dim_in"], t["cfg"]["n_aux"], seed=8)
    vs, va = torch.as_tensor(vs, dtype=torch.float32, device=DEV), torch.as_tensor(va, dtype=torch.float32, device=DEV)
    out = []
    for cfg in (t["on"], t["cfg"]):
        eng = S._engine(cfg, 21, t["spec"], t["aux"])
        out.append([eng.validate(vs, va)[1] for _ in range(3)])
        torch.cuda.synchronize()
        eng.release()
    assert out[0] == out[1] and out[0][0] == out[0][2] and np.isfinite(out[0][0]["kendall"])


# ------------------------------------------------------------------------------------------------ 5. TrialBatch
def test_trial_batch_with_different_temperatures_is_bitwise_the_trials_alone():
    from rankaae_amd.trial_batch import TrialBatch
    cfg = dict(S._case_cfg("FC"), batch_size=32, rank_loss_form="logistic")
    spec, aux, _ = make_spectra(160, cfg["dim_in"], cfg["n_aux"], seed=6)
    steps = 3
    alone = []
    for t, T in enumerate(TEMPS):
        e = S._engine(dict(cfg, rank_temperature=T), 200 + t, spec, aux)
        e.set_epoch(S._perm(160, 50 + t), 0.3)
        for _ in range(steps):
            e.step(32)
        torch.cuda.synchronize()
        alone.append((e.arena.P.detach().clone(), e.losses()))
        e.release()
    shared = TrialBatch.shared_stream(DEV)
    engs = [S._engine(dict(cfg, rank_temperature=T), 200 + t, spec, aux, stream=shared) for t, T in enumerate(TEMPS)]
    batch = TrialBatch(engs)                     # (a refused step would raise BatchingRefused below)
    for t, e in enumerate(engs):
        e.set_epoch(S._perm(160, 50 + t), 0.3)
    for _ in range(steps):
        batch.step(32)
    torch.cuda.synchronize()
    assert batch.programs[(32, True)][1] is not None
    for t, e in enumerate(engs):
        assert torch.equal(S._bits(e.arena.P.detach()), S._bits(alone[t][0])), f"trial {t}: parameters"
        assert e.losses() == alone[t][1], f"trial {t}: losses"
    assert not torch.equal(alone[0][0], alone[1][0])
    batch.release()
    for e in engs:
        e.release()


# ------------------------------------------------------------------------------------------------ 6. Trainer
class _Abandon(Exception):
    pass


def test_resumed_run_ends_where_the_uninterrupted_one_does_and_logs_the_form(tmp_path):
    """Three epochs straight against a kill in epoch 2's callback (the file of epoch 1 stands), then ``resume``; a
    changed temperature is refused; ``messages.txt`` names the form and says what becomes of ``kendall_activation``."""
    import test_resume_gpu as R
    cfg = R._cfg("FC", max_epoch=3, checkpoint_every=1, batch_size=64, rank_loss_form="logistic", rank_temperature=0.5)
    a = R._Trial(tmp_path / "a", cfg, R.SEED["FC"])
    log, handler = S._messages_logger(a.wd, "rank_logistic_a")
    a.trainer.logger = log
    a.trainer.train()
    handler.close()
    log.removeHandler(handler)
    a.close()
    lines = [ln for ln in open(os.path.join(a.wd, "messages.txt")).read().splitlines() if "rank_loss_form" in ln]
    assert len(lines) == 2 and "rank_loss_form: logistic, rank_temperature T = 0.5" in lines[0]
    assert "kendall_activation is not applied" in lines[1]
    want = R._final(tmp_path / "a")
    b = R._Trial(tmp_path / "b", cfg, R.SEED["FC"])

    def die(epoch, m):
        if epoch == 2:
            raise _Abandon()
    with pytest.raises(_Abandon):
        b.trainer.train(die)
    b.close()
    st = torch.load(tmp_path / "b" / R.rf.NAME, weights_only=True)
    assert st["epoch"] == 1 and st["fingerprint"]["cfg.rank_temperature"] == 0.5
    assert st["fingerprint"]["cfg.rank_loss_form"] == "logistic"
    c = R._Trial(tmp_path / "b", {**cfg, "resume": True}, R.SEED["FC"] + 1000)
    seen = []
    c.trainer.train(lambda epoch, m: seen.append(epoch))
    c.close()
    assert seen == [2]
    got = R._final(tmp_path / "b")
    assert got.keys() == want.keys()
    for k, v in want.items():
        assert torch.equal(got[k], v), k
    d = R._Trial(tmp_path / "b", {**cfg, "resume": True, "rank_temperature": 1.0}, R.SEED["FC"])
    with pytest.raises(ValueError, match="cfg.rank_temperature"):
        d.trainer.train()
    d.close()


# ------------------------------------------------------------------------------------------------ 7. data parallel
def test_dp_path_one_rank_equals_plain():
    """The data-parallel code path over a one-rank RCCL group (``tests/test_dp_gpu.py``): with local pairs every rank
    runs the same kernel on its own rows and there is no collective for it, so the engine told ``world_size=2`` is
    bitwise the plain engine."""
    import torch.distributed as dist
    from rankaae_amd.engine import StepEngine
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29648")
    if not dist.is_initialized():
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda:0"))
    try:
        cfg = dict(S._case_cfg("FC"), rank_loss_form="logistic", rank_temperature=T_ENG)
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
            results.append((eng.arena.P.detach().clone(), eng.losses()))
            eng.close()
    finally:
        dist.destroy_process_group()
    assert torch.equal(S._bits(results[0][0]), S._bits(results[1][0]))
    assert results[0][1] == results[1][1] and np.isfinite(results[0][1]["kendall"])
