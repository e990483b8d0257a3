"""The 256-row step across the A/B and C/D phase boundaries (config key ``pair_across_phases``: ``True``, ``False`` or a
list of ``"AB"``, ``"CD"``, ``"DE"``).  A/B: the decoder forward whose output the reference discards rides in the
launches of the adversarial phase's encoder backward, of the weight-gradient tasks that end it and of that phase's update;
C/D: the decoder's half of the reconstruction update and then the mutual-information phase's decoder forward ride in the
reconstruction phase's encoder backward and in the encoder's half of the update.  What is left of either decoder forward
pairs with the encoder forward that follows, its head beside the encoder's second block (``raae_co_launch``,
``raae_block_fwd_a2`` / ``_b2``).  Every body runs on the operands and with the grid-relative indices it has alone, so
nothing may move by a bit: all comparisons here are ``torch.equal`` / ``==``."""
import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from test_cross_phase_gpu import DEV, _case, _engine, _schedule, _state

KEYS = [["AB"], ["CD"], ["AB", "CD", "DE"], True]
# launches the kept pairs remove from the 256-row step of the benchmark's networks, per boundary: A/B and C/D each take
# the decoder forward's last two block kernels and its head off the chain (they find partners in the encoder forward
# that follows: 11 -> 8 launches; the riders before them and the split update add and remove none), D/E six (the
# encoder's update half and six forward block kernels ride in seven launches, the split update adds one)
REMOVED = {"AB": 3, "CD": 3, "DE": 6}


def _run(cfg, spec, aux, use_graph):
    eng, n_train = _engine(cfg, 77, spec, aux, use_graph)
    losses = []
    for ep in range(2):
        eng.set_epoch(torch.randperm(n_train, generator=torch.Generator().manual_seed(ep)), 0.3)
        for rows, smooth in _schedule(cfg["batch_size"], n_train):
            eng.step(rows, smooth=smooth)
            losses.append(eng.losses())
    st = _state(eng)
    eng.release()
    return losses, st


@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("extra", [{}, {"detect_anomaly": False}, {"detect_anomaly": True}, {"optimizer_name": "RAdam"}],
                         ids=["default", "unchecked", "checked", "radam"])
@pytest.mark.parametrize("case", ["compact", "compact_small"])
def test_crossing_ab_cd_changes_nothing(case, extra, use_graph):
    """Each of ``["AB"]``, ``["CD"]``, ``["AB", "CD", "DE"]`` and ``True`` against ``False``, device RNG: over two epochs
    of six steps each -- eager emission, capture + launch, replays, a step with ``smooth=False`` and a ragged last batch
    -- the five losses of every step, every parameter, Adam moment and BatchNorm running statistic are bit for bit the
    same.  With the checked and the unchecked updates, and with RAdam, whose update has no body in the conv kernels'
    translation unit and goes alone, before the launches that would have carried it."""
    cfg, spec, aux = _case(case)
    want = _run(dict(cfg, pair_across_phases=False, **extra), spec, aux, use_graph)
    for key in KEYS:
        got = _run(dict(cfg, pair_across_phases=key, **extra), spec, aux, use_graph)
        assert got[0] == want[0], key
        assert len(got[1]) == len(want[1]) and all(torch.equal(x, y) for x, y in zip(got[1], want[1])), key


def test_trial_batch_ab_cd_and_launch_count():
    """Three trials of the benchmark's shape stepped as one ``TrialBatch`` with the boundaries crossed: the batch is not
    refused (every new launch has its batched ``_m`` form) and every trial is bit for bit the trial stepped alone with the
    key off.  Launch count of the 256-row step: 148 with the key off; each boundary alone removes what ``REMOVED`` says,
    all three together 12 (136 launches: 6 fewer than the 142 of the D/E crossing alone)."""
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
    for name, key in (("off", False), ("AB", ["AB"]), ("CD", ["CD"]), ("DE", ["DE"]), ("on", True)):
        shared = TrialBatch.shared_stream(DEV)
        engs = [_engine(dict(cfg, pair_across_phases=key), 500 + t, spec, aux, True, shared)[0] for t in range(T)]
        batch = TrialBatch(engs)
        for ep in range(2):
            for t, e in enumerate(engs):
                e.set_epoch(perm(t, ep, n_train), 0.3)
            for rows, smooth in _schedule(bs, n_train):
                batch.step(rows, smooth=smooth)          # (raises BatchingRefused if a launch has no batched form)
        counts[name] = batch.launches_per_step(bs)
        for t, e in enumerate(engs):
            st, losses = _state(e), e.losses()
            assert losses == alone[t][1], (name, t)
            assert all(torch.equal(x, y) for x, y in zip(st, alone[t][0])), (name, t)
        batch.release()
    print("launches per 256-row step:", counts)
    assert counts["off"] > 0
    for name in ("AB", "CD", "DE"):
        assert counts["off"] - counts[name] == REMOVED[name], counts
    assert counts["off"] - counts["on"] == sum(REMOVED.values()), counts
    assert counts["DE"] - counts["on"] >= 4, counts
