"""CPU checks of ``train_sc``'s trial-mode decision: which mode ``trial_mode: auto`` picks for a configuration, and the
launch-geometry hint (``tile_rows_mult``) of the batched mode for the conv networks."""
import pytest

from rankaae_amd.cmd import train_sc
from rankaae_amd.parameter import Parameters


def _cfg(**over):
    cfg = dict(ae_form="compact", batch_size=1024, rng_mode="philox", precision="fp32", trial_mode="auto")
    cfg.update(over)
    return Parameters(cfg)


@pytest.mark.parametrize("bs", [64, 256, 1023, 1024, 1536, 2048, 4096])
def test_auto_batches_the_conv_networks_at_every_batch_size_it_wins(bs):
    want = "batched"
    if train_sc.AUTO_THREADS_FROM_ROWS is not None and bs >= train_sc.AUTO_THREADS_FROM_ROWS:
        want = "threads"
    assert train_sc.choose_trial_mode(_cfg(batch_size=bs)) == want


def test_auto_batches_conv_networks_at_1024_rows():
    assert train_sc.choose_trial_mode(_cfg()) == "batched"
    assert train_sc.choose_trial_mode(dict(ae_form="compact", batch_size=1024)) == "batched"    # the defaults


@pytest.mark.parametrize("ae_form", ["compact", "FC"])
def test_auto_falls_to_threads_where_trials_cannot_be_batched(ae_form):
    assert train_sc.choose_trial_mode(_cfg(ae_form=ae_form, rng_mode="host")) == "threads"
    assert train_sc.choose_trial_mode(_cfg(ae_form=ae_form, precision="bf16")) == "threads"
    assert train_sc.choose_trial_mode(_cfg(ae_form=ae_form, fused_blocks=False)) == "batched"   # refused at run time
    assert train_sc.choose_trial_mode(_cfg(ae_form="FC", batch_size=4096)) == "batched"


def test_explicit_modes_are_kept():
    assert train_sc.choose_trial_mode(_cfg(trial_mode="processes")) == "processes"
    assert train_sc.choose_trial_mode(_cfg(trial_mode="processes", rng_mode="host")) == "processes"
    assert train_sc.choose_trial_mode(_cfg(trial_mode="threads")) == "threads"
    # batched is accepted for the conv networks at any batch size ...
    for bs in (256, 1024, 4096):
        assert train_sc.choose_trial_mode(_cfg(trial_mode="batched", batch_size=bs)) == "batched"
    # ... but not where the engines cannot be batched
    for over in (dict(rng_mode="host"), dict(precision="bf16"), dict(fused_discriminator=False)):
        with pytest.raises(ValueError):
            train_sc.choose_trial_mode(_cfg(trial_mode="batched", **over))
    with pytest.raises(ValueError):
        train_sc.choose_trial_mode(_cfg(trial_mode="lockstep"))


def test_batched_tile_hint_is_keyed_on_the_batch_size():
    for bs in (1, 64, 256, 512, 1023):
        assert train_sc.batched_tile_rows_mult(bs) == 4
    for bs in (1024, 1536, 2048, 4096, 8192):
        assert train_sc.batched_tile_rows_mult(bs) == 1
