"""``spec_broaden`` on the GPU: the kernel (``raae_spec_augment2``) against the float64 reference within the derived
bound (and the bound against three wrong references, on the CPU), its bitwise identities with ``raae_spec_augment``
and the step head, determinism, its refusals and its batched form; the engine's augmented batch (eager, captured,
recorded) alone and with ``spec_shift``; batched trials; ``Trainer``; resume."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import augment_reference as ar
import broaden_reference as br
import test_spec_shift_gpu as S
from rankaae_amd.synthetic import make_spectra

if torch.cuda.is_available():
    from rankaae_amd import _lib, ops
    DEV = torch.device("cuda:0")

LOSS_KEYS = S.LOSS_KEYS
U = 2.0 ** -24
SMALL = [(1, 2), (2, 4), (3, 7), (5, 256), (3, 510)]
SHAPES = SMALL + [(1030, 8), (2, 8192)]   # (1030, 8): more rows than workgroups; (2, 8192): the largest LDS image (> 64 KiB)
SIGMAS = [0.4, 2.5, 21.0]                 # R = 2, 8, 63; (2, 4) with 2.5 and 21.0: R > L, every tap is clamped
SHIFTS = [0.0, 2.75]
NOISE = 0.03
GUARD, FILL, CURSOR0 = S.GUARD, S.FILL, S.CURSOR0
_cases = {}


def _rows(B, L):
    """``B + 5`` rows of N(0, 1) plus a ramp with a few large spikes (one at an end of a row), and a permuted ``idx``:
    made on the CPU, so that the checks of the bound itself need no GPU."""
    g = torch.Generator().manual_seed(100000 * B + L)
    N = B + 5
    data = torch.randn(N, L, generator=g) + torch.linspace(0.0, 4.0, L)[None, :]
    for r in range(N):
        for p in torch.randint(0, L, (2,), generator=g).tolist():
            data[r, p] += 40.0 * (1.0 if (r + p) % 2 else -1.0)
    data[0, 0] += 25.0
    data[N - 1, L - 1] -= 25.0
    return data, torch.randperm(N, generator=g)


class _Case(S._Case):
    """``test_spec_shift_gpu._Case`` (the head, the noise term, the state) on the spiked rows, with the new entry point."""

    def __init__(self, B, L, seed=None, counter0=None, data=None):
        super().__init__(B, L, seed, counter0)
        if data is None:
            self.data, self.idx = _rows(B, L)
        else:
            self.data = data
        self.rows = self.data[self.idx[CURSOR0:CURSOR0 + B]]
        self.spec, self.idx_dev = self.data.to(DEV), self.idx.to(DEV)

    def augment2(self, state, cursor, sg, s, noise, spec=None, B=None):
        B = self.B if B is None else B
        n = B * self.L
        buf = torch.full((GUARD + n + GUARD,), FILL, device=DEV)
        view = buf[GUARD:GUARD + n]
        ops.spec_augment2(self.spec if spec is None else spec, self.idx_dev, cursor, state, B, self.L, sg, s, noise, 0, view)
        torch.cuda.synchronize()
        return buf, view


def _case(B, L):
    if (B, L) not in _cases:
        _cases[(B, L)] = _Case(B, L)
    return _cases[(B, L)]


def _seed_counter(B, L):
    return 1000003 * B + L, 7 * B + L + 1            # (what ``_Case`` starts from, the counter as the head advances it)


def _reference(rows, B, L, sg, s):
    seed, counter = _seed_counter(B, L)
    sigma, delta, R = br.sigmas(B, seed, counter, sg), ar.deltas(B, seed, counter, s), br.radius(sg)
    ref = ar.shift_rows_by(br.broaden_rows_by(rows, sigma, R), delta)
    return ref, br.error_bound(rows, sigma, R, delta), sigma, delta, R


def _noise_tol(got, term):
    """The noise is added as the head adds it: one rounding of the sum (at most an ulp of the result) and, against the
    reference's ``fl(z sigma)``, one of the product."""
    return np.spacing(np.abs(got)).astype(np.float64) + U * np.abs(term)


# ------------------------------------------------------------------------------------------------ 1. the kernel
@pytest.mark.parametrize("noise", [0.0, NOISE])
@pytest.mark.parametrize("B,L", SHAPES)
def test_kernel_matches_the_float64_reference_within_the_derived_bound(B, L, noise):
    """``|out - ref| <= broaden_reference.error_bound`` per element ("Resolution augmentation: the
    error bound"; nothing in it comes from the kernel's output), plus the noise term's two roundings with the noise on.
    The data set, ``idx``, the cursor and the random state are not written, nor anything around the output."""
    c = _case(B, L)
    state, cursor, plain = c.head(c.spec, 0.0)
    assert torch.equal(plain.cpu(), c.rows)
    before = (c.spec.clone(), c.idx_dev.clone(), state.clone(), cursor.clone())
    rows = c.rows.numpy()
    term = c.noise_term(noise).double().numpy() if noise else 0.0
    worst = 0.0
    for sg in SIGMAS:
        for s in SHIFTS:
            ref, bound, sigma, delta, R = _reference(rows, B, L, sg, s)
            buf, view = c.augment2(state, cursor, sg, s, noise)
            got = view.cpu().view(B, L).numpy()
            tol = bound + (_noise_tol(got, term) if noise else 0.0)
            err = np.abs(got.astype(np.float64) - (ref + term))
            ratio = float((err / np.maximum(tol, 1e-300)).max())
            worst = max(worst, ratio)
            print(f"B {B} L {L} max_sigma {sg} (R {R}) max_shift {s} noise {noise}: max |err| {err.max():.3e}, "
                  f"max err / bound {ratio:.3f}, sigma in [{sigma.min():.3f}, {sigma.max():.3f}]")
            assert np.all(err <= tol), (sg, s, float(err.max()), int(err.argmax()), ratio)
            assert S._guards_intact(buf, 0, B * L)
            if not noise and s == 0.0 and sigma.max() > 0.3:
                assert not np.array_equal(got, rows)                         # (something was broadened)
    print(f"B {B} L {L} noise {noise}: largest err / bound {worst:.3f}")
    for now, was in zip((c.spec, c.idx_dev, state, cursor), before):
        assert torch.equal(now, was)


def _can_show(sigma, R):
    """Where each of the three mistakes CAN show, decided from the rows' widths alone (never from a kernel's output).
    A mistake that moves a share ``m`` of an output's normalised weight from one sample to another changes the output
    by ``m |x - x'|``; the bound is about ``2 n u`` times the weighted ``|x|`` (fused sum and ``W``, ``n = 2 R + 1``).
    On spiked rows ``|x - x'|`` reaches the weighted ``|x|``, so ``m > 100 n u`` leaves a factor of 5 over the 10 x
    bound that is asserted.

    * one tap dropped at either end: ``m = 2 w_R / W`` of the widest row;
    * zero-padded edges: at an end sample the nearest tap beyond the row weighs ``w_1 / W``;
    * the next row's sigma: the nearest tap's share ``w_1 / W`` differs between the two widths by more than ``100 n u``
      for some neighbouring pair (one row has no neighbour)."""
    n, thr = 2 * R + 1, 100.0 * (2 * R + 1) * U
    share = lambda sg, j: 0.0 if sg == 0 else float(br.weights(sg, R)[R + j] / br.weights(sg, R).sum())     # noqa: E731
    w1 = np.array([share(sg, 1) for sg in sigma])
    return {"R - 1": 2.0 * max(share(sg, R) for sg in sigma) > thr,
            "zero-padded": float(w1.max()) > thr,
            "sigma of the next row": len(sigma) > 1 and float(np.abs(w1 - np.roll(w1, -1)).max()) > thr}


@pytest.mark.parametrize("s", SHIFTS)
@pytest.mark.parametrize("sg", SIGMAS)
def test_bound_separates_three_wrong_references(sg, s):
    """On the CPU, for the inputs of the test above (every shape of the issue's list): a reference with one tap dropped
    at either end (``R - 1``), one with row b given row b + 1's sigma, and one with zero-padded edges each differ from
    the true reference by more than 10 x the bound -- on EVERY shape where the mistake can show (``_can_show``: the
    outermost tap of rows whose own sigma is small weighs less than a rounding, and one row has no neighbour to take a
    sigma from), and somewhere among the shapes in any case.  The bound is too tight for a kernel with one of these
    mistakes, on any of these shapes, to pass."""
    worst = {"R - 1": 0.0, "sigma of the next row": 0.0, "zero-padded": 0.0}
    for B, L in SHAPES[:-1]:
        data, idx = _rows(B, L)
        rows = data[idx[CURSOR0:CURSOR0 + B]].numpy()
        ref, bound, sigma, delta, R = _reference(rows, B, L, sg, s)
        wrong = {"R - 1": br.broaden_rows_by(rows, sigma, R - 1),
                 "sigma of the next row": br.broaden_rows_by(rows, np.roll(sigma, -1), R),
                 "zero-padded": br.broaden_rows_by(rows, sigma, R, pad="constant")}
        shows = _can_show(sigma, R)
        for name, g in wrong.items():
            ratio = float((np.abs(ar.shift_rows_by(g, delta) - ref) / bound).max())
            print(f"B {B} L {L} max_sigma {sg} max_shift {s}: {name}: max |difference| / bound {ratio:.1f}"
                  f"{'' if shows[name] else ' (cannot show here)'}")
            worst[name] = max(worst[name], ratio)
            if shows[name]:
                assert ratio > 10.0, (B, L, name, ratio)
    assert all(r > 10.0 for r in worst.values()), worst


# ------------------------------------------------------------------------------------------------ 2. bitwise identities
@pytest.mark.parametrize("noise", [0.0, NOISE])
@pytest.mark.parametrize("B,L", SMALL)
def test_zero_sigma_is_bitwise_raae_spec_augment_and_the_step_head(B, L, noise):
    """``max_sigma = 0``: every row is passed through, so the launch is ``raae_spec_augment`` with the same
    ``max_shift``, noise and state, bit for bit, and with ``max_shift = 0`` as well the head's ``spec_out`` -- a
    ``-0.0`` sample included."""
    c = _case(B, L)
    spec = c.spec.clone()
    spec[c.idx[CURSOR0], 1] = -0.0
    spec[c.idx[CURSOR0 + B - 1], L - 1] = -0.0
    state, cursor, head_out = c.head(spec, noise)
    for s in SHIFTS:
        want = torch.full((B * L,), FILL, device=DEV)
        ops.spec_augment(spec, c.idx_dev, cursor, state, B, L, s, noise, 0, want)
        buf, view = c.augment2(state, cursor, 0.0, s, noise, spec=spec)
        assert torch.equal(S._bits(view), S._bits(want)), s
        assert S._guards_intact(buf, 0, B * L)
        if s == 0.0:
            assert torch.equal(S._bits(view), S._bits(head_out).view(-1))
            if not noise:
                assert bool(torch.signbit(view.view(B, L)[0, 1])) and float(view.view(B, L)[0, 1]) == 0.0


ZERO_ROWS, ZERO_COUNTERS, ZERO_SEED = 4096, 12000, 711


def _find_zero_draw():
    """The first ``(counter, b)`` with ``v_b = 0`` among ``ZERO_ROWS`` rows of counters ``1 .. ZERO_COUNTERS`` (49 M
    draws of 24 bits: one is expected every 16.8 M), or None."""
    for counter in range(1, ZERO_COUNTERS + 1):
        hit = np.nonzero(br.unit_draws(ZERO_ROWS, ZERO_SEED, counter) == 0)[0]
        if hit.size:
            return counter, int(hit[0])
    return None


def test_row_whose_sigma_is_zero_keeps_its_bits():
    """A row with ``v_b = 0`` among broadened rows (searched with the reference on the CPU; if the bounded search finds
    none, the case is constructed through ``max_sigma = 0``, where every ``sigma_b`` is 0): the output row is the
    input row, ``-0.0`` included, while its neighbours are broadened."""
    found = _find_zero_draw()
    L = 8
    if found is None:
        counter, b0, B, sg = 5, 1, 4, 0.0
        print("no v_b == 0 in the bounded search: constructed through max_sigma = 0")
    else:
        counter, b0 = found
        B, sg = b0 + 2, 2.5
        print(f"v_b == 0 at seed {ZERO_SEED}, counter {counter}, row {b0}")
    c = _Case(B, L, seed=ZERO_SEED, counter0=counter - 1)
    spec = c.spec.clone()
    spec[c.idx[CURSOR0 + b0], 3] = -0.0
    state, cursor, _ = c.head(spec, 0.0)
    sigma = br.sigmas(B, ZERO_SEED, counter, sg)
    assert sigma[b0] == 0.0
    buf, view = c.augment2(state, cursor, sg, 0.0, 0.0, spec=spec)
    got, rows = view.view(B, L), spec[c.idx_dev[CURSOR0:CURSOR0 + B]]
    assert torch.equal(S._bits(got[b0]), S._bits(rows[b0])) and bool(torch.signbit(got[b0, 3]))
    assert S._guards_intact(buf, 0, B * L)
    if found is not None:
        other = int(np.argmax(sigma))
        assert sigma[other] > 1.0 and not torch.equal(got[other], rows[other])


# ------------------------------------------------------------------------------------------------ 3. determinism, geometry
@pytest.mark.parametrize("noise", [0.0, NOISE])
def test_graph_replay_is_bitwise_the_eager_call(noise):
    c = _case(5, 256)
    state, cursor, _ = c.head(c.spec, 0.0)
    stream = torch.cuda.Stream(device=DEV)
    stream.wait_stream(torch.cuda.current_stream(DEV))
    out = torch.full((5 * 256,), FILL, device=DEV)
    with torch.cuda.stream(stream):
        ops.spec_augment2(c.spec, c.idx_dev, cursor, state, 5, 256, 2.5, 2.75, noise, 0, out)
        eager = out.clone()
        out.fill_(FILL)
        g = ops.Graph()
        g.begin()
        try:
            ops.spec_augment2(c.spec, c.idx_dev, cursor, state, 5, 256, 2.5, 2.75, noise, 0, out)
        finally:
            g.end()
        for i in range(2):
            out.fill_(FILL)
            g.launch()
            stream.synchronize()
            assert torch.equal(S._bits(out), S._bits(eager)), f"replay {i}"
    torch.cuda.current_stream(DEV).wait_stream(stream)
    assert not bool((eager == FILL).any())


def test_output_depends_on_the_rows_own_position_only():
    """One spectrum at every batch position (every ``idx`` entry names it): row b of the output is the reference at
    ``sigma_b``, ``delta_b`` of ITS b, the rows differ from one another, and the first rows of a launch with 1030 rows
    (grid-stride, 1024 workgroups) are bitwise those of launches with 3 and with 40 rows."""
    L, sg, s = 8, 2.5, 2.75
    c = _Case(1030, L)
    same = c.spec[c.idx[CURSOR0]].clone().expand(c.N, L).contiguous()
    state, cursor, _ = c.head(same, 0.0)
    full = c.augment2(state, cursor, sg, s, 0.0, spec=same)[1].view(1030, L).clone()
    rows = same[:1030].cpu().numpy()
    ref, bound, sigma, delta, R = _reference(rows, 1030, L, sg, s)
    assert np.all(np.abs(full.cpu().numpy().astype(np.float64) - ref) <= bound)
    assert len(np.unique(full.cpu().numpy(), axis=0)) > 1000
    for Bs in (3, 40):
        cur = torch.tensor([CURSOR0 + Bs], dtype=torch.int32, device=DEV)      # as the head of a Bs-row step leaves it
        part = c.augment2(state, cur, sg, s, 0.0, spec=same, B=Bs)[1].view(Bs, L)
        assert torch.equal(S._bits(part), S._bits(full[:Bs])), Bs


@pytest.mark.parametrize("sg", SIGMAS)
def test_constant_rows_come_back_constant_within_the_bound(sg):
    B, L, value = 64, 40, 1.625
    c = _Case(B, L, data=torch.full((B + 5, L), value))
    state, cursor, _ = c.head(c.spec, 0.0)
    got = c.augment2(state, cursor, sg, 0.0, 0.0)[1].cpu().view(B, L).numpy()
    ref, bound, sigma, _, R = _reference(c.rows.numpy(), B, L, sg, 0.0)
    assert np.all(np.abs(ref - value) <= (2 * R + 2) * 2.0 ** -53 * value) and sigma.max() > 0.9 * sg     # (float64's own sums)
    err = np.abs(got.astype(np.float64) - ref)
    print(f"max_sigma {sg}: max |out - c| {err.max():.3e}, max err / bound {(err / bound).max():.3f}")
    assert np.all(err <= bound)


# ------------------------------------------------------------------------------------------------ 4. refusals
BAD_ARGS = {"spec_null": dict(spec=None), "idx_null": dict(idx=None), "cursor_null": dict(cursor=None),
            "state_null": dict(state=None), "out_null": dict(out=None), "B_zero": dict(B=0), "L_one": dict(L=1),
            "L_8193": dict(L=8193), "sigma_negative": dict(sg=-0.5), "sigma_nan": dict(sg=float("nan")),
            "sigma_inf": dict(sg=float("inf")), "sigma_21.5": dict(sg=21.5),
            # large finite values: 3 s is beyond every int (715827883: just), or Inf in fp32 (3e38), or s itself is (1e300)
            "sigma_715827883": dict(sg=715827883.0), "sigma_1e10": dict(sg=1e10), "sigma_3e38": dict(sg=3e38),
            "sigma_1e300": dict(sg=1e300), "shift_negative": dict(s=-0.5),
            "shift_nan": dict(s=float("nan")), "shift_inf": dict(s=float("inf")), "noise_nan": dict(noise=float("nan")),
            "goff_2": dict(goff=2), "goff_minus_4": dict(goff=-4)}


@pytest.mark.parametrize("case", list(BAD_ARGS))
def test_kernel_refuses_bad_arguments_and_writes_nothing(case):
    c = _case(3, 7)
    state, cursor, _ = c.head(c.spec, 0.0)
    out = torch.full((GUARD + 21 + GUARD,), FILL, device=DEV)
    a = dict(spec=c.spec, idx=c.idx_dev, cursor=cursor, state=state, B=3, L=7, sg=1.0, s=1.0, noise=0.0, goff=0,
             out=out[GUARD:GUARD + 21])
    a.update(BAD_ARGS[case])
    before = (out.clone(), state.clone(), cursor.clone())
    rc = _lib.load().raae_spec_augment2(ops._ptr(a["spec"]), ops._ptr(a["idx"], torch.int64), ops._ptr(a["cursor"], torch.int32),
                                        ops._ptr(a["state"], torch.int64), a["B"], a["L"], a["sg"], a["s"], a["noise"],
                                        a["goff"], ops._ptr(a["out"]), ops._stream())
    torch.cuda.synchronize()
    assert rc == -1, rc                                     # RAAE_EINVAL
    assert torch.equal(S._bits(out), S._bits(before[0])) and torch.equal(state, before[1]) and torch.equal(cursor, before[2])
    if all(a[k] is not None for k in ("spec", "idx", "cursor", "state", "out")):
        with pytest.raises(_lib.HipCallError):
            ops.spec_augment2(a["spec"], a["idx"], a["cursor"], a["state"], a["B"], a["L"], a["sg"], a["s"], a["noise"],
                              a["goff"], a["out"])


# ------------------------------------------------------------------------------------------------ 5. batched form
def test_batched_planes_are_bitwise_the_single_calls():
    """Three planes with their own data, largest sigma (so their own radius: 2, 8, 63), largest shift, seed and counter
    through the recorder and one ``gridDim.z = 3`` launch."""
    lib = _lib.load()
    B, L, widths, shifts = 5, 256, [0.4, 2.5, 21.0], [2.75, 0.0, 0.5]
    planes, single = [], []
    for t in range(3):
        c = _Case(B, L, seed=900 + 17 * t, counter0=3 + 5 * t)
        state, cursor, _ = c.head(c.spec, 0.0)
        single.append(c.augment2(state, cursor, widths[t], shifts[t], NOISE)[1].clone())
        planes.append((c, state, cursor, torch.full((GUARD + B * L + GUARD,), FILL, device=DEV)))
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    handles = (C.c_void_p * 3)()
    with torch.cuda.stream(stream):
        for t in range(3):
            c, state, cursor, buf = planes[t]
            assert lib.raae_record_begin() == 0
            try:
                ops.spec_augment2(c.spec, c.idx_dev, cursor, state, B, L, widths[t], shifts[t], NOISE, 0, buf[GUARD:GUARD + B * L])
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
        assert torch.equal(S._bits(buf[GUARD:GUARD + B * L]), S._bits(single[t])), f"plane {t}"
        assert S._guards_intact(buf, 0, B * L)
    assert not torch.equal(single[0], single[1])


# ------------------------------------------------------------------------------------------------ 6. the engine
BROADEN, SHIFT = 2.5, 2.75
_trained = {}


def _three_steps(ae_form):
    """192 spectra, 64 rows, three steps of engines from the same weights and seed: ``spec_broaden`` alone and with
    ``spec_shift``, each with the captured graph and all eager; ``spec_shift`` alone; no key; the key ``null``.  The
    batch of every step is read back.  Run once per network, shared, never changed."""
    if ae_form not in _trained:
        cfg = S._case_cfg(ae_form)
        spec, aux, _ = make_spectra(192, cfg["dim_in"], cfg["n_aux"], seed=4)
        both = dict(cfg, spec_broaden=BROADEN, spec_shift=SHIFT)
        runs = {}
        for name, c, graph in (("broaden", dict(cfg, spec_broaden=BROADEN), True), ("broaden_eager", dict(cfg, spec_broaden=BROADEN), False),
                               ("both", both, True), ("both_eager", both, False), ("shift", dict(cfg, spec_shift=SHIFT), True),
                               ("absent", cfg, True), ("null", dict(cfg, spec_broaden=None), True)):
            eng = S._engine(c, 21, spec, aux, use_graph=graph)
            perm = S._perm(192, 30)
            eng.set_epoch(perm, 0.3)
            batches = []
            for _ in range(3):
                eng.step(64)
                torch.cuda.synchronize()
                batches.append(eng.plans[64].spec.cpu().clone())
            runs[name] = dict(eng=eng, perm=perm, batches=batches, P=eng.arena.P.detach().cpu().clone(), losses=eng.losses())
        _trained[ae_form] = dict(cfg=cfg, **runs)
    return _trained[ae_form]


def _head_at(eng, k, spec, noise, b=64, cursor0=None):
    """The step head at the state of the engine's step k (counter k - 1 -> k) on ``spec`` with ``idx`` the identity or
    the engine's permutation: ``(state, cursor, spec_out)``."""
    L = eng.L
    goff = -eng.plans[b].noise - 1
    assert goff >= 0
    state = torch.tensor([k - 1, eng.seed, 0], dtype=torch.int64, device=DEV)
    cursor = torch.tensor([0 if cursor0 is None else cursor0], dtype=torch.int32, device=DEV)
    idx = torch.arange(len(spec), dtype=torch.int64, device=DEV) if cursor0 is None else eng.perm
    out = torch.empty(b, L, device=DEV)
    ops.step_begin(torch.zeros(8, dtype=torch.int32, device=DEV), 5, 0, state, cursor, b,
                   torch.zeros(1, dtype=torch.int32, device=DEV), spec, torch.zeros(len(spec), 1, device=DEV),
                   idx, b, L, 1, noise, None, goff, out, torch.empty(b, 1, device=DEV))
    torch.cuda.synchronize()
    return state, cursor, out, goff


@pytest.mark.parametrize("keys", ["broaden", "both"])
@pytest.mark.parametrize("ae_form", ["FC", "compact"])
def test_engine_batch_is_the_reference_applied_to_the_gathered_rows(ae_form, keys):
    """After every step the encoder input is the float64 reference of the step's own rows, widths and shifts drawn from
    the engine's seed and counter, plus the head's noise term at that state: within the bound of the kernel test."""
    t = _three_steps(ae_form)
    run, cfg = t[keys], t["cfg"]
    eng = run["eng"]
    noise, L = float(cfg["spec_noise"]), cfg["dim_in"]
    s = SHIFT if keys == "both" else 0.0
    assert noise > 0 and eng.spec_broaden == BROADEN
    data = eng.train_spec.cpu()
    zeros = torch.zeros(64, L, device=DEV)
    for k, got in enumerate(run["batches"], start=1):
        rows = data[run["perm"][64 * (k - 1):64 * k]].numpy()
        term = _head_at(eng, k, zeros, noise)[2].cpu().double().numpy()
        sigma, delta = br.sigmas(64, eng.seed, k, BROADEN), ar.deltas(64, eng.seed, k, s)
        ref = br.augment(rows, eng.seed, k, BROADEN, s) + term
        g = got.numpy()
        tol = br.error_bound(rows, sigma, br.radius(BROADEN), delta) + _noise_tol(g, term)
        err = np.abs(g.astype(np.float64) - ref)
        print(f"{ae_form} {keys} step {k}: max |err| {err.max():.3e}, max err / tol {(err / tol).max():.3f}")
        assert np.all(err <= tol), (k, float(err.max()), int(err.argmax()))
        assert float(np.abs(g - (rows + term)).max()) > 1e-3                 # (the rows were broadened, not only noised)


@pytest.mark.parametrize("ae_form", ["FC", "compact"])
def test_captured_steps_are_bitwise_the_eager_ones_and_cost_one_launch(ae_form):
    t = _three_steps(ae_form)
    for name in ("broaden", "both"):
        a, b = t[name], t[name + "_eager"]
        for k in range(3):
            assert torch.equal(S._bits(a["batches"][k]), S._bits(b["batches"][k])), (name, k)
        assert torch.equal(S._bits(a["P"]), S._bits(b["P"])), name
        assert all(a["losses"][k] == b["losses"][k] for k in LOSS_KEYS), (name, a["losses"], b["losses"])
        assert all(np.isfinite(a["losses"][k]) for k in LOSS_KEYS)
        assert not torch.equal(a["P"], t["absent"]["P"])                     # the key changes the training
    assert not torch.equal(t["broaden"]["P"], t["both"]["P"]) and not torch.equal(t["shift"]["P"], t["both"]["P"])
    if "launches" not in t:
        counts = {}
        for name in ("broaden", "both", "shift", "absent", "null"):
            e = t[name]["eng"]
            e.set_epoch(S._perm(192, 40), 0.3)
            counts[name] = S._count_launches(e, 64)
        t["launches"] = counts
    n = t["launches"]
    print(f"{ae_form}: launches per step {n}")
    assert n["broaden"] == n["absent"] + 1 and n["both"] == n["absent"] + 1
    assert n["shift"] == n["absent"] + 1 and n["null"] == n["absent"]


@pytest.mark.parametrize("ae_form", ["FC", "compact"])
def test_key_absent_or_null_is_the_engine_that_never_heard_of_it(ae_form):
    t = _three_steps(ae_form)
    a, b = t["null"], t["absent"]
    assert a["eng"].spec_broaden is None and b["eng"].spec_broaden is None and t["shift"]["eng"].spec_broaden is None
    assert torch.equal(S._bits(a["P"]), S._bits(b["P"]))
    assert all(a["losses"][k] == b["losses"][k] for k in LOSS_KEYS)
    for k in range(3):
        assert torch.equal(S._bits(a["batches"][k]), S._bits(b["batches"][k]))


@pytest.mark.parametrize("ae_form", ["FC", "compact"])
def test_spec_shift_alone_is_still_raae_spec_augment(ae_form):
    """With only ``spec_shift`` set the step's batch is bit for bit what ``raae_spec_augment`` writes for the engine's
    rows, seed and counter (and the step has the launches it had: the count is in the test above)."""
    t = _three_steps(ae_form)
    run, cfg = t["shift"], t["cfg"]
    eng = run["eng"]
    noise = float(cfg["spec_noise"])
    perm_now = eng.perm.clone()
    eng.perm.copy_(run["perm"].to(DEV))
    try:
        for k, got in enumerate(run["batches"], start=1):
            state, cursor, _, goff = _head_at(eng, k, eng.train_spec, 0.0, cursor0=64 * (k - 1))
            want = torch.empty(64, eng.L, device=DEV)
            ops.spec_augment(eng.train_spec, eng.perm, cursor, state, 64, eng.L, SHIFT, noise, goff, want)
            torch.cuda.synchronize()
            assert torch.equal(S._bits(got), S._bits(want.cpu())), k
    finally:
        eng.perm.copy_(perm_now)
        torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 7. TrialBatch
def test_trial_batch_with_different_widths_is_bitwise_the_trials_alone():
    from rankaae_amd.trial_batch import TrialBatch
    cfg = dict(S._case_cfg("FC"), batch_size=32)
    spec, aux, _ = make_spectra(160, cfg["dim_in"], cfg["n_aux"], seed=6)
    keys, steps = [dict(spec_broaden=0.4), dict(spec_broaden=2.5, spec_shift=2.75)], 4
    keys[0]["spec_shift"] = 0.5                   # (the trials must agree on whether spec_shift is set, too)
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


def test_trial_batch_refuses_one_engine_with_the_key_and_one_without():
    from rankaae_amd.trial_batch import TrialBatch
    cfg = dict(S._case_cfg("FC"), batch_size=32)
    spec, aux, _ = make_spectra(96, cfg["dim_in"], cfg["n_aux"], seed=6)
    shared = TrialBatch.shared_stream(DEV)
    a = S._engine(dict(cfg, spec_broaden=1.0), 1, spec, aux, stream=shared)
    b = S._engine(cfg, 2, spec, aux, stream=shared)
    with pytest.raises(ValueError, match="must agree on whether spec_broaden is set"):
        TrialBatch([a, b])
    a.release()
    b.release()


# ------------------------------------------------------------------------------------------------ 8. Trainer
def test_trainer_broadens_the_training_steps_and_never_the_validation(tmp_path):
    """Two epochs, FC, 64 rows (140 training rows: two batches of 64 and a ragged one of 12), with the key and without
    it from the same seed.  At the end of an epoch the batch of its last step is the reference applied to the rows the
    cursor names; the validation the trainer ran is the engine's own on the split as it is."""
    import test_resume_gpu as R
    finals, messages = {}, {}
    for name, over in (("with", {"spec_broaden": 2.0}), ("without", {})):
        cfg = R._cfg("FC", max_epoch=2, batch_size=64, **over)
        t = R._Trial(tmp_path / name, cfg, R.SEED["FC"])
        log, handler = S._messages_logger(t.wd, "broaden_" + name)
        t.trainer.logger = log
        seen = {}

        def check(epoch, metrics, t=t, seen=seen, name=name, cfg=cfg):
            if epoch != 0:
                return
            eng = t.trainer.engine
            val_spec = t.trainer._val_split[0]
            before = val_spec.clone()
            _, vl = eng.validate(*t.trainer._val_split)
            seen["direct"], seen["metrics"] = vl, list(metrics)
            assert torch.equal(S._bits(val_spec), S._bits(before))           # the split itself, bit for bit
            n, cur, k = len(eng.train_spec), int(eng.cursor.item()), int(eng.rng_state[0].item())
            b = n % 64 or 64
            assert cur == n and k == -(-n // 64) and b in eng.plans
            rows = eng.train_spec[eng.perm[cur - b:cur]].cpu().numpy()
            term = _head_at(eng, k, torch.zeros(b, eng.L, device=DEV), float(cfg["spec_noise"]), b=b)[2].cpu().double().numpy()
            got = eng.plans[b].spec.cpu().numpy()
            plain = np.abs(got - (rows + term)).max()
            if name == "with":
                sigma, delta = br.sigmas(b, eng.seed, k, 2.0), ar.deltas(b, eng.seed, k, 0.0)
                tol = br.error_bound(rows, sigma, br.radius(2.0), delta) + _noise_tol(got, term)
                assert np.all(np.abs(got - (br.augment(rows, eng.seed, k, 2.0, 0.0) + term)) <= tol)
                assert plain > 1e-3                                          # not the plain gather plus its noise
            else:
                assert plain <= 2.0 * np.spacing(np.abs(got)).max()
        metrics = t.trainer.train(check)
        handler.close()
        log.removeHandler(handler)
        assert all(np.isfinite(m) for m in metrics) and "direct" in seen
        assert seen["metrics"][1] == seen["direct"]["recon"] and seen["metrics"][4] == seen["direct"]["kendall"]
        finals[name] = R._final(t.wd)
        messages[name] = open(os.path.join(t.wd, "messages.txt")).read()
        t.close()
    lines = [ln for ln in messages["with"].splitlines() if "spec_broaden" in ln]
    assert len(lines) == 1 and lines[0].endswith("spec_broaden: rows broadened by a Gaussian of up to σ = 2 grid points")
    assert "spec_broaden" not in messages["without"]
    a, b = finals["with"], finals["without"]
    assert a.keys() == b.keys() and all(bool(torch.isfinite(v.double()).all()) for v in a.values())
    assert any(not torch.equal(a[k], b[k]) for k in a)


class _Abandon(Exception):
    pass


def test_resumed_run_ends_where_the_uninterrupted_one_does(tmp_path):
    """Three epochs straight against a kill in epoch 2's callback (the file of epoch 1 stands), then ``resume``."""
    import test_resume_gpu as R
    cfg = R._cfg("FC", max_epoch=3, checkpoint_every=1, batch_size=64, spec_broaden=2.0, spec_shift=1.5)
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
    assert st["epoch"] == 1 and st["fingerprint"]["cfg.spec_broaden"] == 2.0
    c = R._Trial(tmp_path / "b", {**cfg, "resume": True}, R.SEED["FC"] + 1000)
    seen = []
    c.trainer.train(lambda epoch, m: seen.append(epoch))
    c.close()
    assert seen == [2]
    got = R._final(tmp_path / "b")
    assert got.keys() == want.keys()
    for k, v in want.items():
        assert torch.equal(got[k], v), k
    d = R._Trial(tmp_path / "b", {**cfg, "resume": True, "spec_broaden": 2.5}, R.SEED["FC"])
    with pytest.raises(ValueError, match="cfg.spec_broaden"):
        d.trainer.train()
    d.close()
