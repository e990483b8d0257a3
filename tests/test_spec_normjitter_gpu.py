"""``spec_gain`` and ``spec_tilt`` on the GPU: the kernel (``raae_spec_augment3``) against the fp32 emulation of its
gain and tilt stage (``normjitter_reference``), bit for bit -- alone, behind ``raae_spec_augment2``'s broadening and
shift, and under the noise term -- each key alone, its refusals and its batched form; the engine's augmented batch
(eager, captured, recorded) and its launch counts; validation; batched trials; ``Trainer``; resume; data parallel."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import normjitter_reference as nj
import test_spec_broaden_gpu as BR
import test_spec_shift_gpu as S
from rankaae_amd.synthetic import make_spectra

if torch.cuda.is_available():
    from rankaae_amd import _lib, ops
    DEV = torch.device("cuda:0")

LOSS_KEYS = S.LOSS_KEYS
# (1, 5): L no multiple of 4, the scalar tail of a quad; (2, 1): the degenerate ramp; (1025, 8): more rows than the
# 1024 workgroups, the row loop runs twice for row 0
SHAPES = [(3, 256), (1, 5), (2, 1), (1025, 8)]
GAIN, TILT, NOISE = 0.3, 0.7, 0.03
GUARD, FILL, CURSOR0 = S.GUARD, S.FILL, S.CURSOR0
_cases = {}


class _Case(BR._Case):
    """``test_spec_broaden_gpu._Case`` (the head, the state, the spiked rows, ``raae_spec_augment2``) with the new
    entry point."""

    def augment3(self, state, cursor, sg, s, a, t, noise, goff=0, spec=None):
        n = self.B * self.L
        buf = torch.full((GUARD + n + GUARD,), FILL, device=DEV)
        view = buf[GUARD:GUARD + n]
        ops.spec_augment3(self.spec if spec is None else spec, self.idx_dev, cursor, state, self.B, self.L, sg, s, a, t,
                          noise, goff, view)
        torch.cuda.synchronize()
        return buf, view

    def numbered_noise(self, sigma, goff):
        """``z * sigma`` of elements ``goff .. goff + B L - 1`` of the Gaussian numbering at the case's state, from the
        head's own draws: one row of ``B L + 4`` zeros written at the multiple of 4 below ``goff``."""
        n, lo = self.B * self.L, goff % 4
        state = torch.tensor([self.counter0, self.seed, 0], dtype=torch.int64, device=DEV)
        cursor = torch.tensor([0], dtype=torch.int32, device=DEV)
        steps, ticket = torch.zeros(8, dtype=torch.int32, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
        out = torch.full((1, n + 4), FILL, device=DEV)
        ops.step_begin(steps, 5, 0b11111, state, cursor, 1, ticket, torch.zeros(1, n + 4, device=DEV),
                       torch.zeros(1, 1, device=DEV), torch.zeros(1, dtype=torch.int64, device=DEV), 1, n + 4, 1, sigma,
                       None, goff - lo, out, torch.empty(1, 1, device=DEV))
        torch.cuda.synchronize()
        return out.view(-1)[lo:lo + n].cpu().view(self.B, self.L)


def _case(B, L):
    if (B, L) not in _cases:
        _cases[(B, L)] = _Case(B, L)
    return _cases[(B, L)]


def _stage(c, x, a, t):
    """The emulated stage at the case's seed and advanced counter on the fp32 rows ``x`` (a CPU tensor)."""
    return nj.stage32(x.view(c.B, c.L).numpy(), c.seed, c.counter0 + 1, a, t)


def _same_bits(got, want):
    return np.array_equal(np.ascontiguousarray(got).view(np.int32), np.ascontiguousarray(want).view(np.int32))


# ------------------------------------------------------------------------------------------------ 1. the kernel
@pytest.mark.parametrize("B,L", SHAPES)
def test_gain_and_tilt_alone_are_bitwise_the_emulation_of_the_gathered_rows(B, L):
    """``max_sigma = max_shift = spec_noise = 0``: the output is the fp32 emulation of the stage applied to the rows the
    step gathers, bit for bit.  The data set, ``idx``, the cursor and the random state are not written, nor anything
    around the output."""
    c = _case(B, L)
    state, cursor, plain = c.head(c.spec, 0.0)
    assert torch.equal(plain.cpu(), c.rows)
    before = (c.spec.clone(), c.idx_dev.clone(), state.clone(), cursor.clone())
    for a, t in ((GAIN, TILT), (0.05, 0.02), (0.999, 250.0)):
        buf, view = c.augment3(state, cursor, 0.0, 0.0, a, t, 0.0)
        got = view.cpu().view(B, L).numpy()
        want = _stage(c, c.rows, a, t)
        diff = np.abs(got.astype(np.float64) - want.astype(np.float64)).max()
        print(f"B {B} L {L} a {a} t {t}: max |out - emulation| {diff:.3e}; max |out - rows| {np.abs(got - c.rows.numpy()).max():.3e}")
        assert _same_bits(got, want), (a, t, diff)
        assert S._guards_intact(buf, 0, B * L)
        assert not np.array_equal(got, c.rows.numpy())
    for now, was in zip((c.spec, c.idx_dev, state, cursor), before):
        assert torch.equal(now, was)


@pytest.mark.parametrize("B,L,sg,s", [(3, 256, 2.5, 2.75), (3, 256, 21.3, 0.5), (1, 5, 0.4, 2.75), (1025, 8, 2.5, 2.75),
                                      (3, 256, 0.0, 2.75), (3, 256, 2.5, 0.0)])
def test_stage_composes_behind_raae_spec_augment2_bit_for_bit(B, L, sg, s):
    """Broadening and shift on, ``spec_noise = 0``: the output is the emulated stage applied to what
    ``raae_spec_augment2`` writes for the same state and arguments, bit for bit.  ``max_sigma = 21.3``: ``R = 64``."""
    c = _case(B, L)
    state, cursor, _ = c.head(c.spec, 0.0)
    if sg == 21.3:
        assert BR.br.radius(sg) == 64
    base = c.augment2(state, cursor, sg, s, 0.0)[1].cpu()
    assert not torch.equal(base.view(B, L), c.rows)                          # (something was broadened or shifted)
    buf, view = c.augment3(state, cursor, sg, s, GAIN, TILT, 0.0)
    got, want = view.cpu().view(B, L).numpy(), _stage(c, base, GAIN, TILT)
    assert _same_bits(got, want), float(np.abs(got.astype(np.float64) - want).max())
    assert S._guards_intact(buf, 0, B * L)


def test_one_sample_rows():
    """``L = 1`` (which ``raae_spec_augment2`` refuses): every shifted position is the one sample and the ramp is 0, so
    with the shift on the output is ``fl(g_b x)``, the emulation of the gathered rows, bit for bit.  Broadened, the one
    sample is ``x`` only up to the roundings of its weighted sum and division (``broaden_reference.error_bound``),
    which the gain scales by ``g_b < 1 + a``; the product ``g_b x`` rounds once on either side: an ulp of the result."""
    c = _case(2, 1)
    state, cursor, _ = c.head(c.spec, 0.0)
    seed, ctr = c.seed, c.counter0 + 1
    want = _stage(c, c.rows, GAIN, TILT)
    got = c.augment3(state, cursor, 0.0, 2.75, GAIN, TILT, 0.0)[1].cpu().view(2, 1).numpy()
    assert _same_bits(got, want)
    assert _same_bits(got, (c.rows.numpy() * nj.gains(2, seed, ctr, GAIN)[:, None]).astype(np.float32))
    got = c.augment3(state, cursor, 2.5, 2.75, GAIN, TILT, 0.0)[1].cpu().view(2, 1).numpy()
    bound = BR.br.error_bound(c.rows.numpy(), BR.br.sigmas(2, seed, ctr, 2.5), BR.br.radius(2.5), BR.ar.deltas(2, seed, ctr, 2.75))
    err = np.abs(got.astype(np.float64) - want.astype(np.float64))
    print(f"L 1, broadened: max |err| {err.max():.3e}, max err / bound {(err / ((1.0 + GAIN) * bound + np.spacing(np.abs(got)))).max():.3f}")
    assert np.all(err <= (1.0 + GAIN) * bound + np.spacing(np.abs(got)))


@pytest.mark.parametrize("B,L,sg,s,goff", [(3, 256, 2.5, 2.75, 0), (3, 256, 0.0, 0.0, 8), (1, 5, 0.4, 2.75, 0),
                                           (1025, 8, 2.5, 2.75, 4), (3, 256, 2.5, 2.75, 6), (1, 5, 0.0, 0.0, 3),
                                           (2, 1, 0.0, 0.0, 1)])
def test_noise_is_added_to_the_emulated_stage_as_raae_spec_augment2_adds_it(B, L, sg, s, goff):
    """With ``spec_noise`` on the output is (the emulated stage of the noiseless ``raae_spec_augment2`` output) plus the
    noise term ``z * spec_noise`` of the element's place ``noise_goff + b L + l`` in the step's Gaussian numbering.
    The existing model of that term for ``raae_spec_augment2`` (``test_spec_broaden_gpu._noise_tol``) is a BOUND, not
    bit-exact: the term is known as the head's rounded ``fl(z sigma)`` on an all-zero data set, while the kernels add
    the unrounded product in one fused operation; so this test uses that bound -- one rounding of the sum (an ulp of
    the result at most) and one of the product -- on top of a noiseless part that is exact.  ``noise_goff`` 6, 3 and 1
    are no multiples of 4: a row's quads then start inside a Philox block."""
    c = _case(B, L)
    state, cursor, _ = c.head(c.spec, 0.0)
    if goff == 0:
        assert torch.equal(S._bits(c.numbered_noise(NOISE, 0)), S._bits(c.noise_term(NOISE)))      # (the helper's numbering)
    term = c.numbered_noise(NOISE, goff).double().numpy()
    base = c.augment2(state, cursor, sg, s, 0.0)[1].cpu() if L > 1 else c.rows.contiguous()
    clean = _stage(c, base, GAIN, TILT).astype(np.float64)
    buf, view = c.augment3(state, cursor, sg, s, GAIN, TILT, NOISE, goff=goff)
    got = view.cpu().view(B, L).numpy()
    err, tol = np.abs(got.astype(np.float64) - (clean + term)), BR._noise_tol(got, term)
    print(f"B {B} L {L} max_sigma {sg} max_shift {s} noise_goff {goff}: max |err| {err.max():.3e}, max err / bound "
          f"{(err / tol).max():.3f}, max |noise term| {np.abs(term).max():.3e}")
    assert np.all(err <= tol), (float(err.max()), int(err.argmax()))
    assert S._guards_intact(buf, 0, B * L)
    assert np.abs(term).max() > 10.0 * tol.max()                             # (a term of the wrong element would show)
    if goff:
        other = c.numbered_noise(NOISE, goff - 1).double().numpy()
        assert np.abs(got.astype(np.float64) - (clean + other)).max() > 10.0 * tol.max()


@pytest.mark.parametrize("B,L", [(3, 256), (1, 5)])
def test_each_key_alone_leaves_the_other_stage_out(B, L):
    """``max_tilt = 0``: the output is ``fl(g_b x)``; ``max_gain = 0``: ``fl(x + fl(c_b r_l))``; both 0: ``x`` -- up to
    the sign of a zero (``-0 + +0 = +0``), so values are compared with ``==`` there, and ``x`` is
    ``raae_spec_augment2``'s output for the same state and arguments."""
    c = _case(B, L)
    spec = c.spec.clone()
    spec[c.idx[CURSOR0], 1] = -0.0
    state, cursor, _ = c.head(spec, 0.0)
    seed, ctr = c.seed, c.counter0 + 1
    for sg, s in ((0.0, 0.0), (2.5, 2.75)):
        x = c.augment2(state, cursor, sg, s, 0.0, spec=spec)[1].cpu().view(B, L).numpy()
        run = lambda a, t: c.augment3(state, cursor, sg, s, a, t, 0.0, spec=spec)[1].cpu().view(B, L).numpy()     # noqa: E731
        none, gain, tilt = run(0.0, 0.0), run(GAIN, 0.0), run(0.0, TILT)
        assert np.array_equal(none, x)
        p = (nj.tilts(B, seed, ctr, TILT)[:, None] * nj.ramp(L)[None, :]).astype(np.float32)
        assert np.array_equal(gain, (x * nj.gains(B, seed, ctr, GAIN)[:, None]).astype(np.float32))
        assert np.array_equal(tilt, (x + p).astype(np.float32))
        assert not np.array_equal(gain, x) and not np.array_equal(tilt, x)
        if sg == 0.0:
            assert x[0, 1] == 0.0 and np.signbit(x[0, 1]) and none[0, 1] == 0.0 and gain[0, 1] == 0.0


@pytest.mark.parametrize("noise", [0.0, NOISE])
def test_graph_replay_is_bitwise_the_eager_call(noise):
    c = _case(3, 256)
    state, cursor, _ = c.head(c.spec, 0.0)
    stream = torch.cuda.Stream(device=DEV)
    stream.wait_stream(torch.cuda.current_stream(DEV))
    out = torch.full((3 * 256,), FILL, device=DEV)
    args = (c.spec, c.idx_dev, cursor, state, 3, 256, 2.5, 2.75, GAIN, TILT, noise, 0, out)
    with torch.cuda.stream(stream):
        ops.spec_augment3(*args)
        eager = out.clone()
        out.fill_(FILL)
        g = ops.Graph()
        g.begin()
        try:
            ops.spec_augment3(*args)
        finally:
            g.end()
        for i in range(2):
            out.fill_(FILL)
            g.launch()
            stream.synchronize()
            assert torch.equal(S._bits(out), S._bits(eager)), f"replay {i}"
    torch.cuda.current_stream(DEV).wait_stream(stream)
    assert not bool((eager == FILL).any())


def test_output_does_not_depend_on_the_grid():
    """The first rows of a launch with 1025 rows (1024 workgroups, grid-stride) are bitwise those of launches with 3
    and with 40 rows (3 and 40 workgroups): a row's draws depend on its own position alone."""
    c = _case(1025, 8)
    state, cursor, _ = c.head(c.spec, 0.0)
    full = c.augment3(state, cursor, 2.5, 2.75, GAIN, TILT, NOISE)[1].view(1025, 8).clone()
    for Bs in (3, 40):
        cur = torch.tensor([CURSOR0 + Bs], dtype=torch.int32, device=DEV)      # as the head of a Bs-row step leaves it
        out = torch.full((Bs * 8,), FILL, device=DEV)
        ops.spec_augment3(c.spec, c.idx_dev, cur, state, Bs, 8, 2.5, 2.75, GAIN, TILT, NOISE, 0, out)
        torch.cuda.synchronize()
        assert torch.equal(S._bits(out.view(Bs, 8)), S._bits(full[:Bs])), Bs


# ------------------------------------------------------------------------------------------------ 2. refusals
BAD_ARGS = {"spec_null": dict(spec=None), "idx_null": dict(idx=None), "cursor_null": dict(cursor=None),
            "state_null": dict(state=None), "out_null": dict(out=None), "B_zero": dict(B=0), "B_negative": dict(B=-3),
            "B_over_2^29": dict(B=2 ** 29 + 1), "L_zero": dict(L=0), "L_8193": dict(L=8193),
            "sigma_negative": dict(sg=-0.5), "sigma_nan": dict(sg=float("nan")), "sigma_inf": dict(sg=float("inf")),
            "sigma_21.5": dict(sg=21.5), "sigma_1e10": dict(sg=1e10), "sigma_3e38": dict(sg=3e38),
            "shift_negative": dict(s=-0.5), "shift_nan": dict(s=float("nan")), "shift_inf": dict(s=float("inf")),
            "gain_negative": dict(a=-0.1), "gain_one": dict(a=1.0), "gain_one_in_fp32": dict(a=1.0 - 1e-12),
            "gain_two": dict(a=2.0), "gain_nan": dict(a=float("nan")), "gain_inf": dict(a=float("inf")),
            "tilt_negative": dict(t=-0.1), "tilt_nan": dict(t=float("nan")), "tilt_inf": dict(t=float("inf")),
            "tilt_1e39": dict(t=1e39), "noise_nan": dict(noise=float("nan")), "goff_minus_4": dict(goff=-4)}


@pytest.mark.parametrize("case", list(BAD_ARGS))
def test_kernel_refuses_bad_arguments_before_a_launch(case):
    """``RAAE_EINVAL``, the recorder sees no launch, nothing is written.  Every pointer passed is either NULL (refused
    before it is read) or a live buffer of the right size for ``B = 3``, ``L = 7``."""
    lib = _lib.load()
    c = _case(3, 7)
    state, cursor, _ = c.head(c.spec, 0.0)
    out = torch.full((GUARD + 21 + GUARD,), FILL, device=DEV)
    a = dict(spec=c.spec, idx=c.idx_dev, cursor=cursor, state=state, B=3, L=7, sg=1.0, s=1.0, a=GAIN, t=TILT, noise=0.0,
             goff=0, out=out[GUARD:GUARD + 21])
    a.update(BAD_ARGS[case])
    before = (out.clone(), state.clone(), cursor.clone())
    torch.cuda.synchronize()
    assert lib.raae_record_begin() == 0
    try:
        rc = lib.raae_spec_augment3(ops._ptr(a["spec"]), ops._ptr(a["idx"], torch.int64), ops._ptr(a["cursor"], torch.int32),
                                    ops._ptr(a["state"], torch.int64), a["B"], a["L"], a["sg"], a["s"], a["a"], a["t"],
                                    a["noise"], a["goff"], ops._ptr(a["out"]), ops._stream())
    finally:
        h, count = C.c_void_p(), C.c_int(-1)
        assert lib.raae_record_end(C.byref(h), C.byref(count)) == 0
        lib.raae_record_free(h)
    torch.cuda.synchronize()
    assert rc == -1 and count.value == 0                    # RAAE_EINVAL, and the recorder saw no launch
    assert torch.equal(S._bits(out), S._bits(before[0])) and torch.equal(state, before[1]) and torch.equal(cursor, before[2])
    if all(a[k] is not None for k in ("spec", "idx", "cursor", "state", "out")):
        with pytest.raises(_lib.HipCallError):
            ops.spec_augment3(a["spec"], a["idx"], a["cursor"], a["state"], a["B"], a["L"], a["sg"], a["s"], a["a"], a["t"],
                              a["noise"], a["goff"], a["out"])


# ------------------------------------------------------------------------------------------------ 3. batched form
def test_batched_planes_are_bitwise_the_single_calls():
    """Two planes with their own data, seed, counter and ``(a, t, s, sigma)`` through the recorder and one
    ``gridDim.z = 2`` launch."""
    lib = _lib.load()
    B, L = 3, 256
    values = [dict(a=0.05, t=0.02, s=2.75, sg=0.4), dict(a=0.6, t=3.0, s=0.5, sg=2.5)]
    planes, single = [], []
    for t, v in enumerate(values):
        c = _Case(B, L, seed=900 + 17 * t, counter0=3 + 5 * t)
        state, cursor, _ = c.head(c.spec, 0.0)
        single.append(c.augment3(state, cursor, v["sg"], v["s"], v["a"], v["t"], NOISE)[1].clone())
        planes.append((c, state, cursor, torch.full((GUARD + B * L + GUARD,), FILL, device=DEV)))
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    handles = (C.c_void_p * 2)()
    with torch.cuda.stream(stream):
        for t, v in enumerate(values):
            c, state, cursor, buf = planes[t]
            assert lib.raae_record_begin() == 0
            try:
                ops.spec_augment3(c.spec, c.idx_dev, cursor, state, B, L, v["sg"], v["s"], v["a"], v["t"], NOISE, 0,
                                  buf[GUARD:GUARD + B * L])
            finally:
                h, count = C.c_void_p(), C.c_int(0)
                rc = lib.raae_record_end(C.byref(h), C.byref(count))
            assert rc == 0 and count.value == 1
            handles[t] = h
        stream.synchronize()
        for _, _, _, buf in planes:
            buf.fill_(FILL)
        prog = C.c_void_p()
        rc = lib.raae_multi_build(handles, 2, C.byref(prog))
        for h in handles:
            lib.raae_record_free(C.c_void_p(h))
        assert rc == 0
        assert lib.raae_multi_launch(prog, C.c_void_p(stream.cuda_stream)) == 0
        stream.synchronize()
        lib.raae_multi_free(prog)
    for t in range(2):
        buf = planes[t][3]
        assert torch.equal(S._bits(buf[GUARD:GUARD + B * L]), S._bits(single[t])), f"plane {t}"
        assert S._guards_intact(buf, 0, B * L)
    assert not torch.equal(single[0], single[1])


# ------------------------------------------------------------------------------------------------ 4. the engine
BROADEN, SHIFT = 2.5, 2.75
NORM = dict(spec_gain=GAIN, spec_tilt=TILT)
ALL = dict(NORM, spec_broaden=BROADEN, spec_shift=SHIFT)
RUNS = (("norm", NORM, True), ("norm_eager", NORM, False), ("all", ALL, True), ("all_eager", ALL, False),
        ("both", dict(spec_broaden=BROADEN, spec_shift=SHIFT), True), ("shift", dict(spec_shift=SHIFT), True),
        ("shift_gain", dict(spec_shift=SHIFT, spec_gain=GAIN), True), ("absent", {}, True),
        ("null", dict(spec_gain=None, spec_tilt=None), True))
_trained = {}


def _three_steps(ae_form):
    """96 spectra, 32 rows, three steps of engines from the same weights and seed: both keys alone and with
    ``spec_broaden`` and ``spec_shift``, each with the captured graph and all eager; the older keys without the new
    ones; no key; both keys ``null``.  The batch of every step is read back.  Run once per network, shared, never
    changed."""
    if ae_form not in _trained:
        cfg = dict(S._case_cfg(ae_form), batch_size=32)
        spec, aux, _ = make_spectra(96, cfg["dim_in"], cfg["n_aux"], seed=4)
        runs = {}
        for name, over, graph in RUNS:
            eng = S._engine(dict(cfg, **over), 21, spec, aux, use_graph=graph)
            perm = S._perm(96, 30)
            eng.set_epoch(perm, 0.3)
            batches = []
            for _ in range(3):
                eng.step(32)
                torch.cuda.synchronize()
                batches.append(eng.plans[32].spec.cpu().clone())
            runs[name] = dict(eng=eng, perm=perm, batches=batches, P=eng.arena.P.detach().cpu().clone(), losses=eng.losses())
        _trained[ae_form] = dict(cfg=cfg, **runs)
    return _trained[ae_form]


@pytest.mark.parametrize("keys", ["norm", "all"])
@pytest.mark.parametrize("ae_form", ["FC", "compact"])
def test_engine_batch_is_the_reference_applied_to_the_gathered_rows(ae_form, keys):
    """After every step ``P.spec`` is the emulated stage -- gains and tilts drawn from the engine's seed and counter --
    of the step's own rows as ``raae_spec_augment2`` broadens and shifts them at that state (by nothing without those
    keys: the gathered rows, checked), plus the head's noise term at that state within the noise term's bound."""
    t = _three_steps(ae_form)
    run, cfg = t[keys], t["cfg"]
    eng = run["eng"]
    noise, L = float(cfg["spec_noise"]), cfg["dim_in"]
    sg, s = (BROADEN, SHIFT) if keys == "all" else (0.0, 0.0)
    assert noise > 0 and eng.spec_gain == GAIN and eng.spec_tilt == TILT
    data = eng.train_spec.cpu()
    zeros = torch.zeros(32, L, device=DEV)
    perm_now = eng.perm.clone()
    eng.perm.copy_(run["perm"].to(DEV))
    try:
        for k, got in enumerate(run["batches"], start=1):
            rows = data[run["perm"][32 * (k - 1):32 * k]]
            term = BR._head_at(eng, k, zeros, noise, b=32)[2].cpu().double().numpy()
            state, cursor, _, goff = BR._head_at(eng, k, eng.train_spec, 0.0, b=32, cursor0=32 * (k - 1))
            base = torch.empty(32, L, device=DEV)
            ops.spec_augment2(eng.train_spec, eng.perm, cursor, state, 32, L, sg, s, 0.0, goff, base)
            torch.cuda.synchronize()
            if keys == "norm":
                assert torch.equal(S._bits(base.cpu()), S._bits(rows))
            clean = nj.stage32(base.cpu().numpy(), eng.seed, k, GAIN, TILT).astype(np.float64)
            g = got.numpy()
            err, tol = np.abs(g.astype(np.float64) - (clean + term)), BR._noise_tol(g, term)
            print(f"{ae_form} {keys} step {k}: max |err| {err.max():.3e}, max err / tol {(err / tol).max():.3f}")
            assert np.all(err <= tol), (k, float(err.max()), int(err.argmax()))
            assert float(np.abs(g - (base.cpu().numpy() + term)).max()) > 1e-2       # (scaled and tilted, not only noised)
    finally:
        eng.perm.copy_(perm_now)
        torch.cuda.synchronize()


@pytest.mark.parametrize("ae_form", ["FC", "compact"])
def test_captured_steps_are_bitwise_the_eager_ones_and_cost_at_most_one_launch(ae_form):
    t = _three_steps(ae_form)
    for name in ("norm", "all"):
        a, b = t[name], t[name + "_eager"]
        for k in range(3):
            assert torch.equal(S._bits(a["batches"][k]), S._bits(b["batches"][k])), (name, k)
        assert torch.equal(S._bits(a["P"]), S._bits(b["P"])), name
        assert all(a["losses"][k] == b["losses"][k] for k in LOSS_KEYS), (name, a["losses"], b["losses"])
        assert all(np.isfinite(a["losses"][k]) for k in LOSS_KEYS)
        assert not torch.equal(a["P"], t["absent"]["P"])                     # the keys change the training
    assert not torch.equal(t["norm"]["P"], t["all"]["P"]) and not torch.equal(t["both"]["P"], t["all"]["P"])
    assert not torch.equal(t["shift"]["P"], t["shift_gain"]["P"])
    if "launches" not in t:
        counts = {}
        for name, _, graph in RUNS:
            if graph:
                e = t[name]["eng"]
                e.set_epoch(S._perm(96, 40), 0.3)
                counts[name] = S._count_launches(e, 32)
        t["launches"] = counts
    n = t["launches"]
    print(f"{ae_form}: launches per step {n}")
    assert n["norm"] == n["absent"] + 1                     # one launch behind the head
    assert n["all"] == n["both"] == n["absent"] + 1         # it REPLACES raae_spec_augment2 ...
    assert n["shift_gain"] == n["shift"] == n["absent"] + 1   # ... and raae_spec_augment
    assert n["null"] == n["absent"]


@pytest.mark.parametrize("ae_form", ["FC", "compact"])
def test_keys_absent_or_null_is_the_engine_that_never_heard_of_them(ae_form):
    t = _three_steps(ae_form)
    a, b = t["null"], t["absent"]
    for run in (a, b, t["both"], t["shift"]):
        assert run["eng"].spec_gain is None and run["eng"].spec_tilt is None
    assert t["shift_gain"]["eng"].spec_tilt is None and t["shift_gain"]["eng"].spec_gain == GAIN
    assert torch.equal(S._bits(a["P"]), S._bits(b["P"]))
    assert all(a["losses"][k] == b["losses"][k] for k in LOSS_KEYS)
    for k in range(3):
        assert torch.equal(S._bits(a["batches"][k]), S._bits(b["batches"][k]))


@pytest.mark.parametrize("ae_form", ["FC", "compact"])
def test_validation_reconstruction_and_the_averaged_weights_never_jitter(ae_form):
    """An engine with all four keys (and ``ema_decay``) takes three steps; its state is loaded into an engine without
    the augmentation keys.  ``validate``, ``reconstruct`` and the validation under ``ema_weights()`` are bitwise the
    same on both, and the validation split is not written."""
    cfg = dict(S._case_cfg(ae_form), batch_size=32, ema_decay=0.9)
    spec, aux, _ = make_spectra(128, cfg["dim_in"], cfg["n_aux"], seed=4)
    a = S._engine(dict(cfg, **ALL), 21, spec[:96], aux[:96])
    a.set_epoch(S._perm(96, 30), 0.3)
    for _ in range(3):
        a.step(32)
    torch.cuda.synchronize()
    b = S._engine(cfg, 22, spec[:96], aux[:96])
    b.load_state(a.state())
    vs = torch.as_tensor(spec[96:], dtype=torch.float32).to(DEV)
    va = torch.as_tensor(aux[96:], dtype=torch.float32).to(DEV)
    before = vs.clone()
    outs = []
    for e in (a, b):
        z, vl = e.validate(vs, va)
        z = z.clone()                                       # (the plan's buffer: the next validation writes it again)
        zr, rec = (t.clone() for t in e.reconstruct(vs[:8]))
        with e.ema_weights():
            ze, vle = e.validate(vs, va)
            ze = ze.clone()
        torch.cuda.synchronize()
        outs.append((z, vl, zr, rec, ze, vle))
    assert torch.equal(S._bits(vs), S._bits(before))
    (z0, vl0, zr0, rec0, ze0, vle0), (z1, vl1, zr1, rec1, ze1, vle1) = outs
    assert torch.equal(S._bits(z0), S._bits(z1)) and vl0 == vl1
    assert torch.equal(S._bits(zr0), S._bits(zr1)) and torch.equal(S._bits(rec0), S._bits(rec1))
    assert torch.equal(S._bits(ze0), S._bits(ze1)) and vle0 == vle1
    assert not torch.equal(z0, ze0)                                          # (the average is another set of weights)
    a.release()
    b.release()


# ------------------------------------------------------------------------------------------------ 5. TrialBatch
def test_trial_batch_with_different_values_is_bitwise_the_trials_alone():
    from rankaae_amd.trial_batch import TrialBatch
    cfg = dict(S._case_cfg("FC"), batch_size=32)
    spec, aux, _ = make_spectra(160, cfg["dim_in"], cfg["n_aux"], seed=6)
    keys = [dict(spec_gain=0.05, spec_tilt=0.02, spec_shift=0.5), dict(spec_gain=0.6, spec_tilt=3.0, spec_shift=2.75),
            dict(spec_gain=0.3, spec_tilt=0.7, spec_shift=1.5)]
    steps = 4
    alone = []
    for t, kw in enumerate(keys):
        e = S._engine(dict(cfg, **kw), 200 + t, spec, aux)
        e.set_epoch(S._perm(160, 50 + t), 0.3)
        for _ in range(steps):
            e.step(32)
        torch.cuda.synchronize()
        alone.append((e.arena.P.detach().clone(), e.plans[32].spec.clone()))
        e.release()
    shared = TrialBatch.shared_stream(DEV)
    engs = [S._engine(dict(cfg, **kw), 200 + t, spec, aux, stream=shared) for t, kw in enumerate(keys)]
    batch = TrialBatch(engs)
    for t, e in enumerate(engs):
        e.set_epoch(S._perm(160, 50 + t), 0.3)
    for _ in range(steps):
        batch.step(32)
    torch.cuda.synchronize()
    assert batch.programs[(32, True)][1] is not None
    for t, e in enumerate(engs):
        assert torch.equal(S._bits(e.arena.P.detach()), S._bits(alone[t][0])), f"trial {t}: parameters"
        assert torch.equal(S._bits(e.plans[32].spec), S._bits(alone[t][1])), f"trial {t}: batch"
    assert not torch.equal(alone[0][1], alone[1][1])
    batch.release()
    for e in engs:
        e.release()


@pytest.mark.parametrize("key", ["spec_gain", "spec_tilt"])
def test_trial_batch_refuses_one_engine_with_a_key_and_one_without(key):
    from rankaae_amd.trial_batch import TrialBatch
    cfg = dict(S._case_cfg("FC"), batch_size=32)
    spec, aux, _ = make_spectra(96, cfg["dim_in"], cfg["n_aux"], seed=6)
    shared = TrialBatch.shared_stream(DEV)
    a = S._engine(dict(cfg, **{key: 0.25}), 1, spec, aux, stream=shared)
    b = S._engine(cfg, 2, spec, aux, stream=shared)
    with pytest.raises(ValueError, match=f"must agree on whether {key} is set"):
        TrialBatch([a, b])
    a.release()
    b.release()


# ------------------------------------------------------------------------------------------------ 6. Trainer, resume
def test_trainer_logs_each_key_once_and_trains_on_other_batches(tmp_path):
    """One epoch, FC, 64 rows, with the keys and without them from the same seed."""
    import test_resume_gpu as R
    finals, messages = {}, {}
    for name, over in (("with", {"spec_gain": 0.05, "spec_tilt": 0.02}), ("without", {})):
        cfg = R._cfg("FC", max_epoch=1, batch_size=64, **over)
        t = R._Trial(tmp_path / name, cfg, R.SEED["FC"])
        log, handler = S._messages_logger(t.wd, "normjitter_" + name)
        t.trainer.logger = log
        metrics = t.trainer.train()
        handler.close()
        log.removeHandler(handler)
        assert all(np.isfinite(m) for m in metrics)
        finals[name] = R._final(t.wd)
        messages[name] = open(os.path.join(t.wd, "messages.txt")).read()
        t.close()
    gain = [ln for ln in messages["with"].splitlines() if "spec_gain" in ln]
    tilt = [ln for ln in messages["with"].splitlines() if "spec_tilt" in ln]
    assert len(gain) == 1 and gain[0].endswith("spec_gain: rows scaled by a factor in [1 − 0.05, 1 + 0.05)")
    assert len(tilt) == 1 and tilt[0].endswith("spec_tilt: rows tilted by a ramp of up to ±0.02 at the ends")
    assert "spec_gain" not in messages["without"] and "spec_tilt" not in messages["without"]
    a, b = finals["with"], finals["without"]
    assert a.keys() == b.keys() and all(bool(torch.isfinite(v.double()).all()) for v in a.values())
    assert any(not torch.equal(a[k], b[k]) for k in a)


class _Abandon(Exception):
    pass


def test_resumed_run_ends_where_the_uninterrupted_one_does(tmp_path):
    """Three epochs straight against a kill in epoch 2's callback (the file of epoch 1 stands), then ``resume``."""
    import test_resume_gpu as R
    cfg = R._cfg("FC", max_epoch=3, checkpoint_every=1, batch_size=64, spec_gain=0.05, spec_tilt=0.02, spec_shift=1.5)
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
    assert st["epoch"] == 1 and st["fingerprint"]["cfg.spec_gain"] == 0.05 and st["fingerprint"]["cfg.spec_tilt"] == 0.02
    c = R._Trial(tmp_path / "b", {**cfg, "resume": True}, R.SEED["FC"] + 1000)
    seen = []
    c.trainer.train(lambda epoch, m: seen.append(epoch))
    c.close()
    assert seen == [2]
    got = R._final(tmp_path / "b")
    assert got.keys() == want.keys()
    for k, v in want.items():
        assert torch.equal(got[k], v), k
    for key, value in (("spec_gain", 0.06), ("spec_tilt", 0.03)):
        d = R._Trial(tmp_path / "b", {**cfg, "resume": True, key: value}, R.SEED["FC"])
        with pytest.raises(ValueError, match="cfg." + key):
            d.trainer.train()
        d.close()


# ------------------------------------------------------------------------------------------------ 7. data parallel
def test_dp_path_one_rank_equals_plain():
    """The data-parallel code path over a one-rank RCCL group (``tests/test_dp_gpu.py``): each rank draws for its own
    rows and there is no collective for it, so the engine told ``world_size=2`` is bitwise the plain engine."""
    import torch.distributed as dist
    from rankaae_amd.engine import StepEngine
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29653")
    if not dist.is_initialized():
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda:0"))
    try:
        cfg = dict(S._case_cfg("FC"), batch_size=32, **ALL)
        spec, aux, _ = make_spectra(96, cfg["dim_in"], cfg["n_aux"], seed=4)
        results = []
        for world in (1, 2):
            eng = StepEngine(*S._modules(cfg, 21), cfg, DEV, rng_mode="philox", seed=9, use_graph=True, world_size=world,
                             rank=0)
            eng.set_data(spec, aux)
            eng.set_epoch(S._perm(96, 30), 0.3)
            for _ in range(3):
                eng.step(32)
            torch.cuda.synchronize()
            results.append((eng.arena.P.detach().clone(), eng.losses(), eng.plans[32].spec.clone()))
            eng.close()
    finally:
        dist.destroy_process_group()
    assert torch.equal(S._bits(results[0][0]), S._bits(results[1][0])) and results[0][1] == results[1][1]
    assert torch.equal(S._bits(results[0][2]), S._bits(results[1][2]))
