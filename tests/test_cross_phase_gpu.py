"""The 256-row step across a phase boundary (config key ``pair_across_phases``): the decoder backward that ends the
mutual-information phase carries the encoder's half of that phase's Adam update and the encoder forward of the
smoothness phase in its launches (``raae_co_launch``).  Every body runs on the operands and with the grid-relative
indices it has alone, so nothing may move by a bit: all comparisons here are ``torch.equal`` / ``==``."""
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

from rankaae_amd.synthetic import make_spectra

if torch.cuda.is_available():
    from rankaae_amd import model as pm
    from rankaae_amd.engine import StepEngine
    from oracle import ref_train
    DEV = torch.device("cuda:0")


def _case(case):
    """``compact``: the benchmark's configuration and batch (bench.BASE_CFG, 256 rows); ``compact_small``: the golden
    case of the neighbouring suites."""
    if case == "compact":
        from bench import BASE_CFG
        cfg = dict(BASE_CFG)
        spec, aux, _ = make_spectra(2100, cfg["dim_in"], cfg["n_aux"], seed=0)
        return cfg, spec, aux
    with open(os.path.join(os.path.dirname(__file__), "golden", f"ref_{case}.json")) as f:
        g = json.load(f)
    cfg = g["config"]
    spec, aux, _ = make_spectra(g["n_rows"], g["n_points"], cfg["n_aux"], seed=g["data_seed"])
    return cfg, spec, aux


def _engine(cfg, seed, spec, aux, use_graph, stream=None):
    torch.manual_seed(seed)
    cls = pm.AE_CLS_DICT[cfg["ae_form"]]
    enc = cls["encoder"](nstyle=cfg["nstyle"], dropout_rate=cfg["dropout_rate"], dim_in=cfg["dim_in"], n_layers=cfg["n_layers"])
    dec = cls["decoder"](nstyle=cfg["nstyle"], dropout_rate=cfg["dropout_rate"], last_layer_activation=cfg["decoder_activation"],
                         dim_out=cfg["dim_out"], n_layers=cfg["n_layers"])
    dis = pm.DiscriminatorFC(nstyle=cfg["nstyle"], dropout_rate=cfg["dis_dropout_rate"], noise=cfg["dis_noise"],
                             layers=cfg["FC_discriminator_layers"])
    eng = StepEngine(enc, dec, dis, cfg, DEV, rng_mode="philox", seed=seed, use_graph=use_graph, stream=stream)
    n_train = ref_train.split_rows(len(spec))[0]
    eng.set_data(spec[:n_train], aux[:n_train])
    return eng, n_train


def _state(e):
    torch.cuda.synchronize()
    return ([e.arena.P.clone()] + [b_.clone() for mod in (e.enc_mod, e.dec_mod) for b_ in mod.buffers()] +
            [o.m.clone() for o in e.opts.values()] + [o.v.clone() for o in e.opts.values()])


def _schedule(bs, n_train):
    """(rows, smooth) of an epoch: eager emission, capture + launch, replays, a step without the smoothness phase
    (its own graph), and a ragged last batch."""
    ragged = n_train - 5 * bs if 2 <= n_train - 5 * bs < bs else bs // 2 + 3
    return [(bs, True), (bs, True), (bs, True), (bs, False), (bs, True), (ragged, True)]


@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("extra", [{}, {"detect_anomaly": False}, {"detect_anomaly": True}, {"optimizer_name": "RAdam"}],
                         ids=["default", "unchecked", "checked", "radam"])
@pytest.mark.parametrize("case", ["compact", "compact_small"])
def test_pairing_across_phases_changes_nothing(case, extra, use_graph):
    """``pair_across_phases`` on against off, device RNG: over two epochs of six steps each -- eager emission, capture +
    launch, replays, a step with ``smooth=False`` and a ragged last batch -- the five losses of every step, every
    parameter, Adam moment and BatchNorm running statistic are bit for bit the same.  With the checked and the
    unchecked updates, and with RAdam, whose update has no body in the conv kernels' translation unit and runs as a
    launch of its own between the paired ones."""
    cfg, spec, aux = _case(case)
    out = []
    for cross in (False, True):
        eng, n_train = _engine(dict(cfg, pair_across_phases=cross, **extra), 77, spec, aux, use_graph)
        losses = []
        for ep in range(2):
            eng.set_epoch(torch.randperm(n_train, generator=torch.Generator().manual_seed(ep)), 0.3)
            for rows, smooth in _schedule(cfg["batch_size"], n_train):
                eng.step(rows, smooth=smooth)
                losses.append(eng.losses())
        out.append((losses, _state(eng)))
        eng.release()
    assert out[0][0] == out[1][0]
    assert len(out[0][1]) == len(out[1][1]) and all(torch.equal(x, y) for x, y in zip(out[0][1], out[1][1]))


def test_trial_batch_across_phases_and_launch_count():
    """Three trials of the benchmark's shape stepped as one ``TrialBatch`` with ``pair_across_phases`` on: the batch is
    not refused (every new launch has its batched ``_m`` form) and every trial is bit for bit the trial stepped alone
    with the key off.  Launch count of the 256-row step: 148 with the key off, 142 with it on -- six fewer: the
    encoder's Adam half and the six block kernels of the smoothness phase's encoder forward ride in seven launches of
    the decoder backward, and the split update adds one launch (``dense_fwd`` and ``style_bn_fwd`` of the encoder's
    tail live in other translation units and stay launches of their own)."""
    from rankaae_amd.trial_batch import TrialBatch
    cfg, spec, aux = _case("compact")
    bs, T = cfg["batch_size"], 3

    def perm(t, ep, n):
        return torch.randperm(n, generator=torch.Generator().manual_seed(1000 * t + ep))
    alone = []
    for t in range(T):
        e, n_train = _engine(dict(cfg, pair_across_phases=False), 500 + t, spec, aux, True)
        for ep in range(2):
            e.set_epoch(perm(t, ep, n_train), 0.3)
            for rows, smooth in _schedule(bs, n_train):
                e.step(rows, smooth=smooth)
        alone.append((_state(e), e.losses()))
        e.release()
    counts = {}
    for cross in (False, True):
        shared = TrialBatch.shared_stream(DEV)
        engs = [_engine(dict(cfg, pair_across_phases=cross), 500 + t, spec, aux, True, shared)[0] for t in range(T)]
        batch = TrialBatch(engs)
        for ep in range(2):
            for t, e in enumerate(engs):
                e.set_epoch(perm(t, ep, n_train), 0.3)
            for rows, smooth in _schedule(bs, n_train):
                batch.step(rows, smooth=smooth)          # (raises BatchingRefused if a launch has no batched form)
        counts[cross] = batch.launches_per_step(bs)
        for t, e in enumerate(engs):
            st, losses = _state(e), e.losses()
            assert losses == alone[t][1], (cross, t)
            assert all(torch.equal(x, y) for x, y in zip(st, alone[t][0])), (cross, t)
        batch.release()
    print("launches per 256-row step: key off", counts[False], "key on", counts[True])
    assert counts[False] > 0 and counts[False] - counts[True] >= 6, counts
