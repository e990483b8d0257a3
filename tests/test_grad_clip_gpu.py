"""``grad_clip_norm`` on the GPU: the norm kernel (``raae_grad_norm``), the updates with a scale
(``raae_optim_step_clip``), and the clipped step of ``StepEngine`` -- teacher-forced against ``clip_reference``, never
clipping, eager / captured / replayed, batched trials, two data-parallel ranks, resume."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import clip_reference
from rankaae_amd.synthetic import make_spectra

if torch.cuda.is_available():
    from oracle import ref_train
    from rankaae_amd import _lib, model as pm, ops
    from rankaae_amd.engine import OPT_NAMES, StepEngine
    DEV = torch.device("cuda:0")
    RULES = {"Adam": _lib.OPT_ADAM, "AdamW": _lib.OPT_ADAMW, "RAdam": _lib.OPT_RADAM, "AdaBound": _lib.OPT_ADABOUND}

# Every optimizer clips on each of the first 3 steps: the CPU oracle (oracle.ref_train.OracleTrainer, fc_small and
# compact_small, 3 steps) has its smallest per-optimizer gradient norm at 0.0448 (fc_small, smoothness, step 3).
CLIP = 0.02


def _close(a, b, rtol, atol, what):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    err = (a - b).abs() - (atol + rtol * b.abs())
    print(f"{what}: max |diff| {float((a - b).abs().max()):.3e}, excess over the bound {float(err.max()):.3e}")
    assert float(err.max()) <= 0, f"{what}: max excess {float(err.max()):.3e} at {int(err.argmax())}"


# ------------------------------------------------------------------------------------------------ 1. the norm kernel
NORM_SIZES = [64, 192, 64 * 257]        # one workgroup; one; 65 narrow workgroups / 256 wide ones in a grid-stride loop
# slab counts per 64-element segment, cycled over the range; a maximum above 16 takes the 8-lanes-per-element form
SLAB_CASES = {"one": [1], "two": [2], "mixed": [3, 0, 1, 5, 0, 2], "mixed_wide": [20, 0, 1, 17, 3, 0], "extreme": [2]}
_norm_cache = {}


def _norm_case(n, case):
    """Slabs, segment table and the float64 reference norm; computed once per case, shared, never changed."""
    if (n, case) not in _norm_cache:
        g = torch.Generator().manual_seed(n + len(case))
        counts = (SLAB_CASES[case] * (n // 64))[:n // 64]
        max_slab = max(counts)
        slabs = torch.randn(max_slab, n, generator=g)
        if case == "extreme":           # magnitudes 1e-20 and 1e18 side by side (per element, both slabs alike)
            slabs = slabs * torch.where(torch.rand(n, generator=g) < 0.5, torch.tensor(1e-20), torch.tensor(1e18))
        per_el = torch.tensor(counts).repeat_interleave(64)
        live = torch.arange(max_slab)[:, None] < per_el[None, :]
        ref = float(torch.sqrt(((slabs.double() * live).sum(0) ** 2).sum()))
        _norm_cache[(n, case)] = (slabs.to(DEV), torch.tensor(counts, dtype=torch.int16, device=DEV), max_slab, ref)
    return _norm_cache[(n, case)]


def _grad_norm(slabs, seg, n, max_slab, max_norm, counter=None):
    partial = torch.zeros(ops.GRAD_NORM_PARTS, dtype=torch.float64, device=DEV)
    ticket = torch.zeros(1, dtype=torch.int32, device=DEV)
    out = torch.full((2,), -1.0, device=DEV)
    counter = torch.zeros(1, dtype=torch.int32, device=DEV) if counter is None else counter
    outs = []
    for _ in range(2):                  # twice on the same scratch: the ticket resets itself
        ops.grad_norm(slabs, slabs.shape[1], seg, n, max_slab, max_norm, partial, ticket, out, counter)
        outs.append(out.clone())
    torch.cuda.synchronize()
    assert int(ticket) == 0
    assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32)), "two launches, two results"
    return outs[0].cpu(), int(counter)


@pytest.mark.parametrize("case", list(SLAB_CASES))
@pytest.mark.parametrize("n", NORM_SIZES)
def test_norm_kernel_matches_float64(n, case):
    """The fp32 slab sum is the only rounding the kernel has that the float64 reference lacks: at most max_slab * 2^-23
    relative (the float the norm is stored as adds 2^-24, inside the same bound); asserted at twice that."""
    slabs, seg, max_slab, ref = _norm_case(n, case)
    bound = 2.0 * max_slab * 2.0 ** -23
    out, count = _grad_norm(slabs, seg, n, max_slab, 0.5 * ref)         # clips: both launches count
    rel = abs(float(out[0]) - ref) / ref
    print(f"n {n} {case}: norm {float(out[0])!r} reference {ref!r} relative error {rel:.3e} bound {bound:.3e}")
    assert rel <= bound
    want_scale = 0.5 * ref / (ref + 1e-6)
    assert abs(float(out[1]) - want_scale) <= bound * want_scale and count == 2
    out, count = _grad_norm(slabs, seg, n, max_slab, 2.0 * ref)         # does not clip
    assert float(out[1]) == 1.0 and count == 0 and abs(float(out[0]) - ref) / ref <= bound


@pytest.mark.parametrize("case", ["two", "mixed_wide"])
def test_norm_kernel_nan_gives_nan_and_does_not_count(case):
    slabs, seg, max_slab, ref = _norm_case(192, case)
    slabs = slabs.clone()
    slabs[0, 130] = float("nan")         # (segment 2 has slabs in both cases)
    out, count = _grad_norm(slabs, seg, 192, max_slab, 0.5 * ref)
    assert torch.isnan(out).all() and count == 0


def test_norm_kernel_refuses_bad_arguments():
    slabs, seg, max_slab, ref = _norm_case(64, "one")
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(_lib.HipCallError):
            _grad_norm(slabs, seg, 64, max_slab, bad)


# ------------------------------------------------------------------------------------------------ 2. update with a scale
def _hyper(wd):
    return dict(lr=0.01, betas=(0.9, 0.999), eps=1e-8, weight_decay=wd)


@pytest.mark.parametrize("chk", [False, True])
@pytest.mark.parametrize("rule", ["Adam", "AdamW", "RAdam", "AdaBound"])
def test_update_with_a_fixed_scale(rule, chk):
    """n = 192, three slabs, scale 0.25, two steps from zero moments, against ``clip_reference`` on the fp32 slab sum at
    the tolerance of tests/test_optimizers_gpu.py (2e-6 relative + 2e-7); a segment without slabs stays untouched; the
    NaN flag stays 0.  And the same call without a scale is bit for bit the entry without one."""
    g = torch.Generator().manual_seed(17)
    n, nslab, wd = 192, 3, 0.01
    p0 = torch.randn(n, generator=g)
    seg = torch.tensor([3, 0, 3], dtype=torch.int16, device=DEV)
    keep = torch.tensor([1, 0, 1]).repeat_interleave(64) > 0
    hyper = torch.tensor([0.01, 0.9, 0.999, 1e-8, wd, 0.01, 0.1, 1e-3], dtype=torch.float64, device=DEV)
    scale = torch.tensor([0.25], device=DEV)
    ref = [p0[keep].double().clone()]
    opt = clip_reference.make_optimizer(rule, ref, **_hyper(wd))
    state = {k: [p0.to(DEV), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)] for k in ("clip", "null", "old")}
    step = torch.zeros(1, dtype=torch.int32, device=DEV)
    flags = {k: torch.zeros(1, dtype=torch.int32, device=DEV) for k in state}
    for it in range(2):
        slabs = torch.randn(nslab, n, generator=g)
        clip_reference.clipped_step(opt, ref, [((slabs[0] + slabs[1]) + slabs[2])[keep]], scale=0.25)
        step.add_(1)
        sl = slabs.to(DEV)
        for k, sc in (("clip", scale), ("null", None)):
            p, m, v = state[k]
            ops.optim_step_clip(p, m, v, sl, n, seg, n, RULES[rule], hyper, step, max_nslab=3,
                                nan_step=flags[k] if chk else None, scale=sc)
        p, m, v = state["old"]
        ops.optim_step(p, m, v, sl, n, seg, n, RULES[rule], hyper, step, max_nslab=3, nan_step=flags["old"] if chk else None)
    torch.cuda.synchronize()
    for a, b in zip(state["null"], state["old"]):
        assert torch.equal(a, b), "no scale: the entry without one"
    p, m, v = (t.cpu() for t in state["clip"])
    assert torch.equal(p[~keep], p0[~keep]) and not m[~keep].any() and not v[~keep].any()
    _close(p[keep], ref[0], 2e-6, 2e-7, f"{rule} params")
    _close(m[keep], opt.state[ref[0]]["exp_avg"], 2e-6, 2e-7, f"{rule} exp_avg")
    _close(v[keep], opt.state[ref[0]]["exp_avg_sq"], 2e-6, 2e-7, f"{rule} exp_avg_sq")
    assert not torch.equal(state["clip"][1], state["old"][1]), "the moments see the scaled gradient"
    assert all(int(f) == 0 for f in flags.values())
    if chk:     # a NaN gradient stays NaN and raises the flag exactly as without a scale
        sl = torch.randn(nslab, n, generator=g).to(DEV)
        sl[1, 130] = float("nan")
        step.add_(1)
        p, m, v = state["clip"]
        ops.optim_step_clip(p, m, v, sl, n, seg, n, RULES[rule], hyper, step, max_nslab=3, nan_step=flags["clip"], scale=scale)
        assert int(flags["clip"]) == 3 and bool(torch.isnan(p[130])) and int(torch.isnan(p).sum()) == 1


@pytest.mark.parametrize("rule", ["Adam", "AdamW", "RAdam", "AdaBound"])
@pytest.mark.parametrize("hint", [3, 40])
def test_scale_of_one_is_bitwise_the_update_without(rule, hint):
    """Both kernel forms (one thread per element, 8 lanes per element), weight decay on: *scale == 1.0f changes no bit."""
    g = torch.Generator().manual_seed(23)
    n, nslab = 64 * 5, 3
    seg = torch.full((n // 64,), nslab, dtype=torch.int16, device=DEV)
    hyper = torch.tensor([0.01, 0.9, 0.999, 1e-8, 0.01, 0.01, 0.1, 1e-3], dtype=torch.float64, device=DEV)
    one = torch.ones(1, device=DEV)
    step = torch.full((1,), 7, dtype=torch.int32, device=DEV)
    p0, m0, v0 = torch.randn(n, generator=g), torch.randn(n, generator=g) * 0.1, torch.rand(n, generator=g)
    sl = torch.randn(nslab, n, generator=g).to(DEV)
    a, b = [t.to(DEV) for t in (p0, m0, v0)], [t.to(DEV) for t in (p0, m0, v0)]
    ops.optim_step_clip(*a, sl, n, seg, n, RULES[rule], hyper, step, max_nslab=hint, scale=one)
    ops.optim_step(*b, sl, n, seg, n, RULES[rule], hyper, step, max_nslab=hint)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


# ------------------------------------------------------------------------------------------------ the engine
def _case_cfg(case, **over):
    with open(os.path.join(os.path.dirname(__file__), "golden", f"ref_{case}.json")) as f:
        return dict(json.load(f)["config"], **over)


def _engine(cfg, seed, spec, aux, use_graph=True, stream=None, **kw):
    torch.manual_seed(seed)
    cls = pm.AE_CLS_DICT[cfg["ae_form"]]
    enc = cls["encoder"](nstyle=cfg["nstyle"], dropout_rate=cfg["dropout_rate"], dim_in=cfg["dim_in"], n_layers=cfg["n_layers"])
    dec = cls["decoder"](nstyle=cfg["nstyle"], dropout_rate=cfg["dropout_rate"],
                         last_layer_activation=cfg["decoder_activation"], dim_out=cfg["dim_out"], n_layers=cfg["n_layers"])
    dis = pm.DiscriminatorFC(nstyle=cfg["nstyle"], dropout_rate=cfg["dis_dropout_rate"], noise=cfg["dis_noise"],
                             layers=cfg["FC_discriminator_layers"])
    eng = StepEngine(enc, dec, dis, cfg, DEV, rng_mode="philox", seed=700 + seed, use_graph=use_graph, stream=stream, **kw)
    n_train = ref_train.split_rows(len(spec))[0]
    eng.set_data(spec[:n_train], aux[:n_train])
    return eng, n_train


def _state(e):
    torch.cuda.synchronize()
    return ([e.arena.P.clone()] + [b_.clone() for mod in (e.enc_mod, e.dec_mod) for b_ in mod.buffers()] +
            [o.m.clone() for o in e.opts.values()] + [o.v.clone() for o in e.opts.values()])


def _run(cfg, seed, spec, aux, steps, use_graph=True):
    eng, n_train = _engine(cfg, seed, spec, aux, use_graph=use_graph)
    eng.set_epoch(torch.randperm(n_train, generator=torch.Generator().manual_seed(seed)), 0.3)
    for _ in range(steps):
        eng.step(cfg["batch_size"])
    out = (_state(eng), eng.losses(), eng.clipped_steps(),
           eng.clip_stats.cpu() if eng.grad_clip is not None else None)
    eng.release()
    return out


def _slab_sum(G, seg, wide):
    """The fp32 sum of the slabs ``G`` [S][n] (``seg``: slabs per element) in the order the update kernel of the
    range's slab hint sums them: one after the other up to 16 slabs, the 8-chunk tree above (``wide``)."""
    zero = torch.zeros_like(G[0])
    top = int(seg.max())
    if not wide:
        g = zero.clone()
        for r in range(top):
            g = g + torch.where(seg > r, G[r], zero)
        return g
    ch = []
    for c in range(8):                                  # chunk c: slabs c, c + 8, ... in order
        g = zero.clone()
        for r in range(c, top, 8):
            g = g + torch.where(seg > r, G[r], zero)
        ch.append(g)
    return ((ch[0] + ch[1]) + (ch[2] + ch[3])) + ((ch[4] + ch[5]) + (ch[6] + ch[7]))     # the xor-shuffle tree


@pytest.mark.parametrize("case", ["fc_small", "compact_small"])
def test_teacher_forced_steps_match_the_clipped_reference(case):
    """Three steps of the smallest FC and compact configurations with every optimizer clipping on every step.  Per
    phase: the gradient the update is about to consume (``phase_hook``) and the parameters and moments before it go
    through ``clip_reference`` in float64; the engine's parameters and moments after the update (``post_phase_hook``)
    must agree at the tolerance of the update test, the scale the device computed with the reference's, and every
    counter ends at 3.  (Without the feature the key is ignored: no scale, no counters.)"""
    cfg = _case_cfg(case, grad_clip_norm=CLIP, pair_unused_forwards=False)
    spec, aux, _ = make_spectra(700, 256, cfg["n_aux"], seed=3)
    eng, n_train = _engine(cfg, 5, spec, aux, use_graph=False)
    assert eng.grad_clip == CLIP
    rule = cfg["optimizer_name"]
    refs, refs_seq, before, bad, scales, direct = {}, {}, {}, [], {n: [] for n in OPT_NAMES}, {}
    # The reference gets the slabs captured by `phase_hook`, summed in fp32 HERE in the order the update kernel of the
    # range's slab hint sums them (`_slab_sum`: one after the other up to 16 slabs, the 8-chunk tree above) -- no buffer
    # the code under test wrote; that sum must then be, bit for bit, the flat gradient the update consumed.  Summed one
    # after the other instead (`phase_gradient`), ill-conditioned sums -- conv biases and PReLU slopes over 64+ slabs --
    # come out differently enough to move Adam's ratio m / sqrt(v): observed on compact_small with that order, excess of
    # the parameters over the 2e-6 / 2e-7 tolerance, largest of the three steps: reconstruction 3.94e-4, correlation 3.30e-4,
    # adversarial 6.23e-6, mutual_info 1.56e-6 (smoothness and all of fc_small, whose ranges sum in slab order anyway,
    # inside it).  The
    # figure is printed on every run ("captured gradient summed in slab order").

    def pre(name, P):
        o = eng.opts[name]
        seg = P.seg[name][o.lo // 64:o.hi // 64].long().repeat_interleave(64)
        grad = _slab_sum(eng.G[:, o.lo:o.hi], seg, P.max_slab[name] > 16)
        before[name] = (eng.phase_gradient(P, name).cpu(), eng.arena.P[o.lo:o.hi].detach().cpu().clone(), o.m.cpu().clone(),
                        o.v.cpu().clone(), (seg > 0).cpu(), grad.cpu())

    def post(name, P):
        o = eng.opts[name]
        seq, p0, m0, v0, keep, grad = before[name]
        flat = eng.G_flat[o.lo:o.hi].cpu()
        assert torch.equal(flat[keep], grad[keep]), f"{name}: the flat gradient is not the captured slabs in the update's order"

        def reference(table, g):
            if name not in table:
                lr, b1, b2, eps, wd = o.hyper.cpu().tolist()[:5]
                par = [p0[keep].double().clone()]
                table[name] = (par, clip_reference.make_optimizer(rule, par, lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd))
            par, opt = table[name]
            par[0].copy_(p0[keep].double())                 # teacher forcing: the engine's state before the update
            if opt.state[par[0]]:
                opt.state[par[0]]["exp_avg"].copy_(m0[keep].double())
                opt.state[par[0]]["exp_avg_sq"].copy_(v0[keep].double())
            return (par, opt) + clip_reference.clipped_step(opt, par, [g[keep]], CLIP)
        par, opt, norm, scale = reference(refs, grad)
        par_seq = reference(refs_seq, seq)[0]               # (measured only: see the comment above)
        stats = eng.clip_stats[o.index].cpu().tolist()
        scales[name].append((norm, scale, stats))
        p1, m1, v1 = eng.arena.P[o.lo:o.hi].detach().cpu(), o.m.cpu(), o.v.cpu()
        d = (p1[keep].double() - par_seq[0]).abs() - (2e-7 + 2e-6 * par_seq[0].abs())
        direct[name] = max(direct.get(name, -1.0), float(d.max()))
        try:
            # norm and scale: float64 on the same fp32 gradient on both sides; the device stores each as a float (2^-24
            # relative, the scale formed from the float64 norm) -- asserted at 2^-23
            assert scale < 1.0 and abs(stats[0] - norm) <= 2.0 ** -23 * norm and abs(stats[1] - scale) <= 2.0 ** -23 * scale, (norm, scale, stats)
            assert torch.equal(p1[~keep], p0[~keep])
            _close(p1[keep], par[0], 2e-6, 2e-7, f"{case} {name} params")
            _close(m1[keep], opt.state[par[0]]["exp_avg"], 2e-6, 2e-7, f"{case} {name} exp_avg")
            _close(v1[keep], opt.state[par[0]]["exp_avg_sq"], 2e-6, 2e-7, f"{case} {name} exp_avg_sq")
        except AssertionError as e:
            bad.append(f"{name}: {e}")
    eng.phase_hook, eng.post_phase_hook = pre, post
    eng.set_epoch(torch.randperm(n_train, generator=torch.Generator().manual_seed(1)), 0.3)
    for _ in range(3):
        eng.step(cfg["batch_size"])
    torch.cuda.synchronize()
    eng.losses()
    print({n: [f"{s[0]:.4g}" for s in v] for n, v in scales.items()})
    print(f"{case}: captured gradient summed in slab order, excess of the parameters over the tolerance: "
          + ", ".join(f"{n} {x:.3e}" for n, x in direct.items()))
    assert not bad, "\n".join(bad)
    assert all(len(v) == 3 for v in scales.values())
    assert eng.clipped_steps() == [3] * 5
    eng.release()


def _rows256(ae_form, **over):
    cfg = _case_cfg("fc_small" if ae_form == "FC" else "compact_small", batch_size=256, **over)
    spec, aux, _ = make_spectra(1600, 256, cfg["n_aux"], seed=8)
    return cfg, spec, aux


@pytest.mark.parametrize("ae_form", ["FC", "compact"])
def test_never_clipping_is_bitwise_the_step_without_the_key(ae_form):
    """``grad_clip_norm: 1e30``: every scale is exactly 1, and after 3 steps at 256 rows (eager, captured, replayed) the
    weights, moments and BatchNorm statistics are bit for bit those of the run without the key; no step counted."""
    cfg, spec, aux = _rows256(ae_form)
    plain = _run(cfg, 3, spec, aux, 3)
    clip = _run(dict(cfg, grad_clip_norm=1e30), 3, spec, aux, 3)
    assert plain[2] is None and clip[2] == [0] * 5
    assert clip[3][:, 1].tolist() == [1.0] * 5 and all(x > 0 for x in clip[3][:, 0].tolist())
    for a, b in zip(plain[0], clip[0]):
        assert torch.equal(a, b)
    assert plain[1] == clip[1]


@pytest.mark.parametrize("ae_form", ["FC", "compact"])
def test_eager_captured_and_replayed_clipped_steps_agree(ae_form):
    """Four clipped steps through the captured graph (eager emission, capture, two replays) against four eager ones."""
    cfg, spec, aux = _rows256(ae_form, grad_clip_norm=CLIP)
    eager = _run(cfg, 4, spec, aux, 4, use_graph=False)
    graph = _run(cfg, 4, spec, aux, 4, use_graph=True)
    for a, b in zip(eager[0], graph[0]):
        assert torch.equal(a, b)
    assert eager[1] == graph[1] and eager[2] == graph[2] and torch.equal(eager[3], graph[3])
    assert sum(eager[2]) > 0, eager[2]


@pytest.mark.parametrize("ae_form", ["FC", "compact"])
def test_trial_batch_with_clipping_is_bitwise_the_trials_alone(ae_form):
    """Two trials in one launch sequence (gridDim.z = 2), each with its own scale: bit for bit the trials alone."""
    from rankaae_amd.trial_batch import TrialBatch
    cfg, spec, aux = _rows256(ae_form, grad_clip_norm=CLIP)
    T, bs, steps = 2, 256, 4

    def perm(t, n_train):
        return torch.randperm(n_train, generator=torch.Generator().manual_seed(50 + t))
    alone = []
    for t in range(T):
        e, n_train = _engine(cfg, 200 + t, spec, aux)
        e.set_epoch(perm(t, n_train), 0.3)
        for _ in range(steps):
            e.step(bs)
        alone.append((_state(e), e.losses(), e.clipped_steps(), e.clip_stats.cpu()))
        e.release()
    shared = TrialBatch.shared_stream(DEV)
    engs = [_engine(cfg, 200 + t, spec, aux, stream=shared)[0] for t in range(T)]
    batch = TrialBatch(engs)
    for t, e in enumerate(engs):
        e.set_epoch(perm(t, n_train), 0.3)
    for _ in range(steps):
        batch.step(bs)
    assert batch.programs[(bs, True)][1] is not None
    for t, e in enumerate(engs):
        for a, b in zip(alone[t][0], _state(e)):
            assert torch.equal(a, b), f"trial {t}"
        assert alone[t][1] == e.losses() and alone[t][2] == e.clipped_steps() and torch.equal(alone[t][3], e.clip_stats.cpu())
    assert not torch.equal(alone[0][3], alone[1][3]), "each trial has its own scale"
    assert sum(alone[0][2]) > 0
    batch.release()


def test_trial_batch_refuses_mixed_keys():
    from rankaae_amd.trial_batch import TrialBatch
    cfg, spec, aux = _rows256("FC")
    shared = TrialBatch.shared_stream(DEV)
    a = _engine(dict(cfg, grad_clip_norm=CLIP), 1, spec, aux, stream=shared)[0]
    b = _engine(cfg, 2, spec, aux, stream=shared)[0]
    c = _engine(dict(cfg, grad_clip_norm=2 * CLIP), 3, spec, aux, stream=shared)[0]
    for pair in ([a, b], [a, c]):
        with pytest.raises(ValueError, match="grad_clip_norm"):
            TrialBatch(pair)


def test_engine_refuses_a_bad_key_before_it_allocates():
    cfg, spec, aux = _rows256("FC")
    with pytest.raises(ValueError, match="grad_clip_norm"):
        _engine(dict(cfg, grad_clip_norm=-1.0), 1, spec, aux)


def test_bf16_storage_clips_too():
    """``precision: bf16`` keeps the updates fp32: the clipped step runs, clips and stays finite."""
    cfg = _case_cfg("fc_small", precision="bf16", grad_clip_norm=CLIP)
    spec, aux, _ = make_spectra(700, 256, cfg["n_aux"], seed=3)
    state, losses, counts, stats = _run(cfg, 2, spec, aux, 3)
    assert counts == [3] * 5 and torch.isfinite(state[0]).all() and all(np.isfinite(list(losses.values())))
    assert (stats[:, 1] < 1).all()


# ------------------------------------------------------------------------------------------------ 7. data parallel
def _free_port():
    import socket
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        return sk.getsockname()[1]


def _two_rank_clip_worker(rank, world, port):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    cfg = _case_cfg("fc_small", grad_clip_norm=CLIP)
    b = cfg["batch_size"] // world
    cfg["batch_size"] = b
    spec, aux, _ = make_spectra(700, 256, cfg["n_aux"], seed=3)
    torch.manual_seed(5 + rank)                 # (different initial weights: rank 0's are broadcast)
    eng, n_train = _engine(cfg, 5 + rank, spec, aux, use_graph=True, world_size=world, rank=rank)
    eng.set_epoch(torch.randperm(n_train, generator=torch.Generator().manual_seed(2)), 0.3, start=rank * b, stride=world * b)
    per_step = []
    for _ in range(2):
        eng.step(b)
        torch.cuda.synchronize()
        per_step.append(eng.clip_stats.cpu().clone())
    eng.losses()
    box = [None] * world
    dist.all_gather_object(box, (eng.arena.P.detach().cpu(), per_step, eng.clipped_steps(),
                                 [o.m.cpu() for o in eng.opts.values()]))
    for other in box[1:]:
        assert torch.equal(box[0][0], other[0]), "ranks hold different parameters"
        assert all(torch.equal(x, y) for x, y in zip(box[0][1], other[1])), "ranks computed different {norm, scale}"
        assert box[0][2] == other[2] and all(torch.equal(x, y) for x, y in zip(box[0][3], other[3]))
    assert box[0][2] == [2] * 5, box[0][2]
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_clip_alike():
    """Two gloo ranks on the one GPU (fresh child processes): the norm is taken of the rank-averaged gradient, so after
    2 clipped steps both ranks hold identical parameters, moments, {norm, scale} and counters."""
    import torch.multiprocessing as mp
    mp.spawn(_two_rank_clip_worker, args=(2, _free_port()), nprocs=2, join=True)


# ------------------------------------------------------------------------------------------------ 8. resume
class _Abandon(Exception):
    pass


def test_resumed_clipped_run_is_the_uninterrupted_one(tmp_path):
    """Two epochs with ``grad_clip_norm``; the second run dies in epoch 1's callback, a third resumes from the file of
    epoch 0 and ends bit for bit where the uninterrupted run ends -- the counters of clipped steps included."""
    import test_resume_gpu as R
    from rankaae_amd import resume as rf
    cfg = R._cfg("FC", max_epoch=2, checkpoint_every=1, grad_clip_norm=CLIP)
    a = R._Trial(tmp_path / "a", cfg, R.SEED["FC"])
    metrics = a.trainer.train()
    want_counts = a.trainer.engine.clipped_steps()
    want = a.outcome(metrics)
    b = R._Trial(tmp_path / "b", cfg, R.SEED["FC"])

    def die(epoch, m):
        if epoch == 1:
            raise _Abandon()
    with pytest.raises(_Abandon):
        b.trainer.train(die)
    b.close()
    st = torch.load(tmp_path / "b" / rf.NAME, weights_only=True)
    assert st["epoch"] == 0 and "clip_counts" in st["engine"]
    first = st["engine"]["clip_counts"].tolist()
    c = R._Trial(tmp_path / "b", {**cfg, "resume": True}, R.SEED["FC"] + 1000)
    seen = []
    metrics = c.trainer.train(lambda epoch, m: seen.append(epoch))
    got_counts = c.trainer.engine.clipped_steps()
    assert seen == [1]
    R._assert_same_outcome(c.outcome(metrics), want)
    print(f"clipped steps after epoch 0 {first}, after epoch 1 {got_counts}")
    assert got_counts == want_counts and sum(first) > 0 and sum(got_counts) > sum(first)
    d = R._Trial(tmp_path / "b", {**cfg, "resume": True, "grad_clip_norm": 2 * CLIP}, R.SEED["FC"])
    with pytest.raises(ValueError, match="grad_clip_norm"):
        d.trainer.train()
    d.close()
