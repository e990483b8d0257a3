"""``spec_shift`` on the GPU: the kernel (``raae_spec_augment``) against the float64 reference of the draw, with and
without the spectral noise, its ``max_shift = 0`` form against the step head bit for bit, its two bodies, its refusals
and its batched form; the engine's augmented batch (eager, captured, recorded); batched trials; ``Trainer``; resume."""
import ctypes as C
import json
import logging
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import augment_reference as ar
from rankaae_amd.synthetic import make_spectra

if torch.cuda.is_available():
    from rankaae_amd import _lib, model as pm, ops
    from rankaae_amd.engine import StepEngine
    DEV = torch.device("cuda:0")

LOSS_KEYS = ("adversarial", "kendall", "recon", "mutual_info", "smooth")
U = 2.0 ** -24                            # unit roundoff of fp32
SHAPES = [(2, 4), (3, 7), (5, 256), (64, 256), (3, 510)]      # (3, 7), (3, 510): the scalar body; (64, 256): 16 workgroups
NOISE = 0.03
GUARD = 4                                 # guard floats on each side of an output (16 bytes: the view stays aligned)
FILL = -777.25
CURSOR0 = 2                               # the head advances it by B: the batch is idx[2 : 2 + B], inside the permutation
_cases = {}


def _shifts(L):
    return [0.5, 2.75, 4.0, float(L)]     # s = L: every sample of a row is clamped to one of its ends


class _Case:
    """``B + 5`` rows of N(0, 1) plus a ramp, a permuted ``idx`` and the state the step head publishes from
    ``{counter0, seed}`` with the cursor at ``CURSOR0``.  Made once per shape, shared, never changed."""

    def __init__(self, B, L, seed=None, counter0=None):
        self.B, self.L, self.N = B, L, B + 5
        self.seed = (1000003 * B + L) if seed is None else seed
        self.counter0 = (7 * B + L) if counter0 is None else counter0
        g = torch.Generator().manual_seed(100000 * B + L)
        self.data = torch.randn(self.N, L, generator=g) + torch.linspace(0.0, 4.0, L)[None, :]
        self.idx = torch.randperm(self.N, generator=g)
        self.rows = self.data[self.idx[CURSOR0:CURSOR0 + B]]             # what the step gathers
        self.spec, self.idx_dev = self.data.to(DEV), self.idx.to(DEV)
        self.zeros = torch.zeros_like(self.spec)
        self.aux = torch.zeros(self.N, 1, device=DEV)
        self._noise = {}

    def head(self, spec, noise):
        """One ``raae_step_begin`` from the case's initial state: ``(rng_state, cursor, spec_out)`` as it leaves them."""
        state = torch.tensor([self.counter0, self.seed, 0], dtype=torch.int64, device=DEV)
        cursor = torch.tensor([CURSOR0], dtype=torch.int32, device=DEV)
        steps, ticket = torch.zeros(8, dtype=torch.int32, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
        out, aux_out = torch.full((self.B, self.L), FILL, device=DEV), torch.empty(self.B, 1, device=DEV)
        ops.step_begin(steps, 5, 0b11111, state, cursor, self.B, ticket, spec, self.aux, self.idx_dev, self.B, self.L, 1,
                       noise, None, 0, out, aux_out)
        torch.cuda.synchronize()
        assert int(state[0]) == self.counter0 + 1 and int(cursor[0]) == CURSOR0 + self.B <= self.N
        return state, cursor, out

    def noise_term(self, sigma):
        """``z * sigma`` of every element, from the head's own draws: its output on an all-zero data set."""
        if sigma not in self._noise:
            self._noise[sigma] = self.head(self.zeros, sigma)[2].cpu()
        return self._noise[sigma]

    def augment(self, state, cursor, s, noise, off=0):
        """``raae_spec_augment`` into a guarded output ``off`` floats past a 16-byte boundary: (buffer, view)."""
        n = self.B * self.L
        buf = torch.full((GUARD + off + n + GUARD,), FILL, device=DEV)
        view = buf[GUARD + off:GUARD + off + n]
        assert view.data_ptr() % 16 == (4 * off) % 16
        ops.spec_augment(self.spec, self.idx_dev, cursor, state, self.B, self.L, s, noise, 0, view)
        torch.cuda.synchronize()
        return buf, view


def _case(B, L):
    if (B, L) not in _cases:
        _cases[(B, L)] = _Case(B, L)
    return _cases[(B, L)]


def _guards_intact(buf, off, n):
    want = int(torch.tensor([FILL]).view(torch.int32)[0])
    lo, hi = buf[:GUARD + off], buf[GUARD + off + n:]
    return bool((lo.view(torch.int32) == want).all()) and bool((hi.view(torch.int32) == want).all())


def _bits(t):
    return t.contiguous().view(torch.int32)


# ------------------------------------------------------------------------------------------------ 1, 2. the kernel
@pytest.mark.parametrize("noise", [0.0, NOISE])
@pytest.mark.parametrize("B,L", SHAPES)
def test_kernel_matches_the_float64_reference(B, L, noise):
    """Noise off: ``|out - ref| <= 4 * 2^-24 * max|in|``: the reference reproduces ``delta``, ``i0`` and ``f`` exactly,
    the kernel then makes three fp32 roundings on values bounded by ``2 max|in|``.  Noise on: the reference plus the
    head's own ``z * sigma`` (its output on an all-zero data set at the same state), to within that plus one ulp of the
    result.  The data set, ``idx``, the cursor and the random state are not written, nor anything around the output."""
    c = _case(B, L)
    state, cursor, plain = c.head(c.spec, 0.0)
    assert torch.equal(plain.cpu(), c.rows)                                  # (the head gathered the rows meant)
    before = (c.spec.clone(), c.idx_dev.clone(), state.clone(), cursor.clone())
    big = float(c.rows.abs().max())
    term = c.noise_term(noise).double().numpy() if noise else 0.0
    for s in _shifts(L):
        delta = ar.deltas(B, c.seed, c.counter0 + 1, s)
        ref = ar.shift_rows_by(c.rows.numpy(), delta) + term
        buf, view = c.augment(state, cursor, s, noise)
        got = view.cpu().view(B, L).numpy()
        tol = 4.0 * U * big + (np.spacing(np.abs(got)).astype(np.float64) if noise else 0.0)
        err = np.abs(got.astype(np.float64) - ref)
        print(f"B {B} L {L} s {s} noise {noise}: max |err| {err.max():.3e}, max err / tol {(err / tol).max():.3f}, "
              f"delta in [{delta.min():.3f}, {delta.max():.3f}]")
        assert np.all(err <= tol), (s, float(err.max()), int(err.argmax()))
        assert _guards_intact(buf, 0, B * L)
        if not noise:                         # a row shifted by L - 1 or more is one of its own end values throughout
            for b in np.nonzero(np.abs(delta) >= L - 1)[0]:
                assert np.all(got[b] == c.rows.numpy()[b, 0 if delta[b] < 0 else -1]), (s, b)
        if not noise and s <= 4.0:
            assert not np.array_equal(got, c.rows.numpy())                   # (something was shifted)
    for now, was in zip((c.spec, c.idx_dev, state, cursor), before):
        assert torch.equal(now, was)


# ------------------------------------------------------------------------------------------------ 3. max_shift = 0
@pytest.mark.parametrize("noise", [0.0, NOISE])
@pytest.mark.parametrize("B,L", [(2, 4), (3, 7), (5, 256), (3, 510)])
def test_zero_shift_is_bitwise_the_step_head(B, L, noise):
    """Pins the noise numbering, the counter and the cursor convention: the same state, the same bits -- a ``-0.0``
    sample included."""
    c = _case(B, L)
    spec = c.spec.clone()
    spec[c.idx[CURSOR0], 1] = -0.0
    spec[c.idx[CURSOR0 + 1], L - 1] = -0.0
    state, cursor, want = c.head(spec, noise)
    buf = torch.full((GUARD + B * L + GUARD,), FILL, device=DEV)
    view = buf[GUARD:GUARD + B * L]
    ops.spec_augment(spec, c.idx_dev, cursor, state, B, L, 0.0, noise, 0, view)
    torch.cuda.synchronize()
    assert torch.equal(_bits(view), _bits(want).view(-1))
    assert _guards_intact(buf, 0, B * L)
    if noise:
        assert not torch.equal(want.cpu(), spec.cpu()[c.idx[CURSOR0:CURSOR0 + B]])


# ------------------------------------------------------------------------------------------------ 4. the two bodies
@pytest.mark.parametrize("noise", [0.0, NOISE])
def test_vector_and_scalar_bodies_give_the_same_bits(noise):
    """``L = 8``: an output on a 16-byte boundary takes the ``float4`` body, the same rows into a view one, two and
    three floats past one take the scalar body."""
    c = _Case(5, 8)
    state, cursor, _ = c.head(c.spec, 0.0)
    for s in (0.0, 0.5, 2.75):
        outs = []
        for off in (0, 1, 2, 3):
            buf, view = c.augment(state, cursor, s, noise, off)
            assert _guards_intact(buf, off, 40)
            outs.append(view.clone())
        for o in outs[1:]:
            assert torch.equal(_bits(o), _bits(outs[0])), s


# ------------------------------------------------------------------------------------------------ 5. refusals
BAD_ARGS = ["spec_null", "idx_null", "cursor_null", "state_null", "out_null", "B_zero", "L_one", "shift_negative",
            "shift_nan", "shift_inf", "noise_nan", "goff_odd"]


@pytest.mark.parametrize("case", BAD_ARGS)
def test_kernel_refuses_bad_arguments_and_writes_nothing(case):
    c = _case(3, 7)
    state, cursor, _ = c.head(c.spec, 0.0)
    out = torch.full((GUARD + 21 + GUARD,), FILL, device=DEV)
    a = dict(spec=c.spec, idx=c.idx_dev, cursor=cursor, state=state, B=3, L=7, s=1.0, noise=0.0, goff=0, out=out[GUARD:GUARD + 21])
    a.update({"spec_null": dict(spec=None), "idx_null": dict(idx=None), "cursor_null": dict(cursor=None),
              "state_null": dict(state=None), "out_null": dict(out=None), "B_zero": dict(B=0), "L_one": dict(L=1),
              "shift_negative": dict(s=-0.5), "shift_nan": dict(s=float("nan")), "shift_inf": dict(s=float("inf")),
              "noise_nan": dict(noise=float("nan")), "goff_odd": dict(goff=2)}[case])
    before = (out.clone(), state.clone(), cursor.clone())
    rc = _lib.load().raae_spec_augment(ops._ptr(a["spec"]), ops._ptr(a["idx"], torch.int64), ops._ptr(a["cursor"], torch.int32),
                                       ops._ptr(a["state"], torch.int64), a["B"], a["L"], a["s"], a["noise"], a["goff"],
                                       ops._ptr(a["out"]), ops._stream())
    torch.cuda.synchronize()
    assert rc == -1, rc                                     # RAAE_EINVAL
    assert torch.equal(_bits(out), _bits(before[0])) and torch.equal(state, before[1]) and torch.equal(cursor, before[2])
    if all(a[k] is not None for k in ("spec", "idx", "cursor", "state", "out")):
        with pytest.raises(_lib.HipCallError):
            ops.spec_augment(a["spec"], a["idx"], a["cursor"], a["state"], a["B"], a["L"], a["s"], a["noise"], a["goff"], a["out"])


# ------------------------------------------------------------------------------------------------ 6. batched form
def test_batched_planes_are_bitwise_the_single_calls():
    """Three planes with their own data, largest shift, seed and counter through the recorder and one
    ``gridDim.z = 3`` launch (the kernel changes no state, so a plane can be launched again)."""
    lib = _lib.load()
    B, L, shifts = 5, 256, [0.5, 2.75, 4.0]
    planes, single = [], []
    for t, s in enumerate(shifts):
        c = _Case(B, L, seed=900 + 17 * t, counter0=3 + 5 * t)
        state, cursor, _ = c.head(c.spec, 0.0)
        single.append(c.augment(state, cursor, s, NOISE)[1].clone())
        planes.append((c, state, cursor, torch.full((GUARD + B * L + GUARD,), FILL, device=DEV)))
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    handles = (C.c_void_p * 3)()
    with torch.cuda.stream(stream):
        for t, s in enumerate(shifts):
            c, state, cursor, buf = planes[t]
            assert lib.raae_record_begin() == 0
            try:
                ops.spec_augment(c.spec, c.idx_dev, cursor, state, B, L, s, NOISE, 0, buf[GUARD:GUARD + B * L])
            finally:
                h, count = C.c_void_p(), C.c_int(0)
                rc = lib.raae_record_end(C.byref(h), C.byref(count))
            assert rc == 0 and count.value == 1
            handles[t] = h
        stream.synchronize()
        for _, _, _, buf in planes:
            buf.fill_(FILL)
        prog = C.c_void_p()
        rc = lib.raae_multi_build(handles, 3, C.byref(prog))
        for h in handles:
            lib.raae_record_free(C.c_void_p(h))
        assert rc == 0
        assert lib.raae_multi_launch(prog, C.c_void_p(stream.cuda_stream)) == 0
        stream.synchronize()
        lib.raae_multi_free(prog)
    for t in range(3):
        buf = planes[t][3]
        assert torch.equal(_bits(buf[GUARD:GUARD + B * L]), _bits(single[t])), f"plane {t}"
        assert _guards_intact(buf, 0, B * L)
    assert not torch.equal(single[0], single[1])


# ------------------------------------------------------------------------------------------------ 7. the engine
def _case_cfg(ae_form, **over):
    case = "fc_small" if ae_form == "FC" else "compact_small"
    with open(os.path.join(os.path.dirname(__file__), "golden", f"ref_{case}.json")) as f:
        return dict(json.load(f)["config"], batch_size=64, **over)


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


SHIFT = 2.75
_trained = {}


def _three_steps(ae_form):
    """192 spectra, 64 rows, three steps of four engines from the same weights and seed: ``spec_shift`` with the
    captured graph (one eager step, one captured, one replay) and without it (all eager), no key, and the key ``null``.
    The batch of every step is read back.  Run once per network, shared, never changed."""
    if ae_form not in _trained:
        cfg = _case_cfg(ae_form)
        spec, aux, _ = make_spectra(192, cfg["dim_in"], cfg["n_aux"], seed=4)
        runs = {}
        for name, c, graph in (("graph", dict(cfg, spec_shift=SHIFT), True), ("eager", dict(cfg, spec_shift=SHIFT), False),
                               ("absent", cfg, True), ("null", dict(cfg, spec_shift=None), True)):
            eng = _engine(c, 21, spec, aux, use_graph=graph)
            perm = _perm(192, 30)
            eng.set_epoch(perm, 0.3)
            batches = []
            for _ in range(3):
                eng.step(64)
                torch.cuda.synchronize()
                batches.append(eng.plans[64].spec.cpu().clone())
            runs[name] = dict(eng=eng, perm=perm, batches=batches, P=eng.arena.P.detach().cpu().clone(), losses=eng.losses())
        _trained[ae_form] = dict(cfg=cfg, **runs)
    return _trained[ae_form]


@pytest.mark.parametrize("ae_form", ["FC", "compact"])
def test_engine_batch_is_the_reference_applied_to_the_gathered_rows(ae_form):
    """After every step the encoder input is the float64 reference of the step's own rows, shifts drawn from the
    engine's seed and counter, plus the head's noise term at that state: within ``4 * 2^-24 * max|in|`` plus one ulp."""
    t = _three_steps(ae_form)
    run, cfg = t["graph"], t["cfg"]
    eng = run["eng"]
    sigma, L = float(cfg["spec_noise"]), cfg["dim_in"]
    data = eng.train_spec.cpu()
    goff = -eng.plans[64].noise - 1
    assert sigma > 0 and goff >= 0 and int(eng.rng_state[0].item()) == 3
    zeros, aux0 = torch.zeros(64, L, device=DEV), torch.zeros(64, 1, device=DEV)
    for k, got in enumerate(run["batches"], start=1):
        rows = data[run["perm"][64 * (k - 1):64 * k]]
        # the head's own draws at the state of step k: a data set of zeros, counter k - 1 -> k
        state = torch.tensor([k - 1, eng.seed, 0], dtype=torch.int64, device=DEV)
        cursor = torch.zeros(1, dtype=torch.int32, device=DEV)
        out = torch.empty(64, L, device=DEV)
        ops.step_begin(torch.zeros(8, dtype=torch.int32, device=DEV), 5, 0, state, cursor, 64,
                       torch.zeros(1, dtype=torch.int32, device=DEV), zeros, aux0,
                       torch.arange(64, dtype=torch.int64, device=DEV), 64, L, 1, sigma, None, goff, out, torch.empty(64, 1, device=DEV))
        torch.cuda.synchronize()
        ref = ar.shift_rows(rows.numpy(), eng.seed, k, SHIFT) + out.cpu().double().numpy()
        g = got.numpy()
        tol = 4.0 * U * float(rows.abs().max()) + np.spacing(np.abs(g)).astype(np.float64)
        err = np.abs(g.astype(np.float64) - ref)
        print(f"{ae_form} step {k}: max |err| {err.max():.3e}, max err / tol {(err / tol).max():.3f}")
        assert np.all(err <= tol), (k, float(err.max()), int(err.argmax()))
        assert float(np.abs(g - rows.numpy()).max()) > 10 * sigma            # (the rows were shifted, not only noised)


@pytest.mark.parametrize("ae_form", ["FC", "compact"])
def test_captured_steps_are_bitwise_the_eager_ones_and_cost_one_launch(ae_form):
    t = _three_steps(ae_form)
    a, b = t["graph"], t["eager"]
    for k in range(3):
        assert torch.equal(_bits(a["batches"][k]), _bits(b["batches"][k])), k
    assert torch.equal(_bits(a["P"]), _bits(b["P"]))
    assert all(a["losses"][k] == b["losses"][k] for k in LOSS_KEYS), (a["losses"], b["losses"])
    assert all(np.isfinite(a["losses"][k]) for k in LOSS_KEYS)
    assert not torch.equal(a["P"], t["absent"]["P"])                         # the key changes the training
    if "launches" not in t:
        counts = []
        for name in ("graph", "absent"):
            e = t[name]["eng"]
            e.set_epoch(_perm(192, 40), 0.3)
            counts.append(_count_launches(e, 64))
        t["launches"] = counts
    with_key, without = t["launches"]
    print(f"{ae_form}: {with_key} launches per step with spec_shift, {without} without")
    assert with_key == without + 1


@pytest.mark.parametrize("ae_form", ["FC", "compact"])
def test_key_absent_or_null_is_the_engine_that_never_heard_of_it(ae_form):
    t = _three_steps(ae_form)
    a, b = t["null"], t["absent"]
    assert a["eng"].spec_shift is None and b["eng"].spec_shift is None and t["graph"]["eng"].spec_shift == SHIFT
    assert torch.equal(_bits(a["P"]), _bits(b["P"]))
    assert all(a["losses"][k] == b["losses"][k] for k in LOSS_KEYS)
    for k in range(3):
        assert torch.equal(_bits(a["batches"][k]), _bits(b["batches"][k]))


# ------------------------------------------------------------------------------------------------ 8. TrialBatch
def test_trial_batch_with_different_shifts_is_bitwise_the_trials_alone():
    from rankaae_amd.trial_batch import TrialBatch
    cfg = dict(_case_cfg("FC"), batch_size=32)
    spec, aux, _ = make_spectra(160, cfg["dim_in"], cfg["n_aux"], seed=6)
    shifts, steps = [0.5, 2.75], 4
    alone = []
    for t, s in enumerate(shifts):
        e = _engine(dict(cfg, spec_shift=s), 200 + t, spec, aux)
        e.set_epoch(_perm(160, 50 + t), 0.3)
        for _ in range(steps):
            e.step(32)
        torch.cuda.synchronize()
        alone.append((e.arena.P.detach().clone(), e.plans[32].spec.clone()))
        e.release()
    shared = TrialBatch.shared_stream(DEV)
    engs = [_engine(dict(cfg, spec_shift=s), 200 + t, spec, aux, stream=shared) for t, s in enumerate(shifts)]
    batch = TrialBatch(engs)                     # (a refused step would raise BatchingRefused below)
    for t, e in enumerate(engs):
        e.set_epoch(_perm(160, 50 + t), 0.3)
    for _ in range(steps):
        batch.step(32)
    torch.cuda.synchronize()
    assert batch.programs[(32, True)][1] is not None
    for t, e in enumerate(engs):
        assert torch.equal(_bits(e.arena.P.detach()), _bits(alone[t][0])), f"trial {t}: parameters"
        assert torch.equal(_bits(e.plans[32].spec), _bits(alone[t][1])), f"trial {t}: batch"
    batch.release()
    for e in engs:
        e.release()


def test_trial_batch_refuses_one_engine_with_the_key_and_one_without():
    from rankaae_amd.trial_batch import TrialBatch
    cfg = dict(_case_cfg("FC"), batch_size=32)
    spec, aux, _ = make_spectra(96, cfg["dim_in"], cfg["n_aux"], seed=6)
    shared = TrialBatch.shared_stream(DEV)
    a = _engine(dict(cfg, spec_shift=1.0), 1, spec, aux, stream=shared)
    b = _engine(cfg, 2, spec, aux, stream=shared)
    with pytest.raises(ValueError, match="spec_shift"):
        TrialBatch([a, b])
    a.release()
    b.release()


# ------------------------------------------------------------------------------------------------ 9. Trainer
def _messages_logger(wd, tag):
    log = logging.getLogger(f"spec_shift_gpu_{tag}")
    log.setLevel(logging.DEBUG)
    log.propagate = False
    handler = logging.FileHandler(os.path.join(wd, "messages.txt"))
    handler.setFormatter(logging.Formatter("%(asctime)s %(levelname)s:  %(message)s"))
    log.addHandler(handler)
    return log, handler


def test_trainer_shifts_the_training_steps_and_never_the_validation(tmp_path):
    """Two epochs, ``compact``, 64 rows (140 training rows: two batches of 64 and a ragged one of 12), with the key
    and without it from the same seed."""
    import test_resume_gpu as R
    finals, messages = {}, {}
    for name, over in (("with", {"spec_shift": 2.0}), ("without", {})):
        cfg = R._cfg("compact", max_epoch=2, batch_size=64, **over)
        t = R._Trial(tmp_path / name, cfg, R.SEED["compact"])
        log, handler = _messages_logger(t.wd, name)
        t.trainer.logger = log
        seen = {}

        def check(epoch, metrics, t=t, seen=seen):
            if epoch == 0:
                # the validation the trainer just ran, against the engine's own on the split as it is
                _, vl = t.trainer.engine.validate(*t.trainer._val_split)
                seen["direct"], seen["metrics"] = vl, list(metrics)
        metrics = t.trainer.train(check)
        handler.close()
        log.removeHandler(handler)
        assert all(np.isfinite(m) for m in metrics)
        assert seen["metrics"][1] == seen["direct"]["recon"] and seen["metrics"][4] == seen["direct"]["kendall"]
        row = open(os.path.join(t.wd, "losses.csv")).read().splitlines()[1].replace("\t", "").split(",")
        assert int(row[0]) == 0 and all(np.isfinite(float(v)) for v in row[1:13])
        for col, key in ((2, "adversarial"), (6, "kendall"), (8, "recon"), (10, "smooth"), (12, "mutual_info")):
            assert row[col] == f"{seen['direct'][key]:.6f}", (name, key)
        finals[name] = R._final(t.wd)
        messages[name] = open(os.path.join(t.wd, "messages.txt")).read()
        t.close()
    lines = [ln for ln in messages["with"].splitlines() if "spec_shift" in ln]
    assert len(lines) == 1 and lines[0].endswith("spec_shift: rows shifted by up to ±2 grid points")
    assert "spec_shift" not in messages["without"]
    a, b = finals["with"], finals["without"]
    assert a.keys() == b.keys() and all(bool(torch.isfinite(v.double()).all()) for v in a.values())
    assert any(not torch.equal(a[k], b[k]) for k in a)


# ------------------------------------------------------------------------------------------------ 10. resume
class _Abandon(Exception):
    pass


def test_resumed_run_ends_where_the_uninterrupted_one_does(tmp_path):
    """Three epochs straight against a kill in epoch 2's callback (the file of epoch 1 stands), then ``resume``."""
    import test_resume_gpu as R
    cfg = R._cfg("FC", max_epoch=3, checkpoint_every=1, batch_size=64, spec_shift=2.0)
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
    assert st["epoch"] == 1 and st["fingerprint"]["cfg.spec_shift"] == 2.0
    c = R._Trial(tmp_path / "b", {**cfg, "resume": True}, R.SEED["FC"] + 1000)
    seen = []
    c.trainer.train(lambda epoch, m: seen.append(epoch))
    c.close()
    assert seen == [2]
    got = R._final(tmp_path / "b")
    assert got.keys() == want.keys()
    for k, v in want.items():
        assert torch.equal(got[k], v), k
    d = R._Trial(tmp_path / "b", {**cfg, "resume": True, "spec_shift": 2.5}, R.SEED["FC"])
    with pytest.raises(ValueError, match="cfg.spec_shift"):
        d.trainer.train()
    d.close()
