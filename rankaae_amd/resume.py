"""The resume file of a trial (config keys ``checkpoint_every`` / ``resume``; DESIGN.md "Checkpoint and resume"):
``<work_dir>/resume.pt``, a plain dict of tensors and Python scalars that loads with ``weights_only=True``, kept in two
generations (``resume.pt`` and ``resume.prev.pt``).  Host code only: what goes into the file is gathered by
``StepEngine.state`` and ``Trainer``; this module has the file protocol, the fingerprint of what must not change between
the two runs, the choice of the epoch a batched group resumes from, and the ``losses.csv`` clean-up."""
import os

import numpy as np
import torch

FORMAT_VERSION = 1
NAME, PREV_NAME, TMP_NAME = "resume.pt", "resume.prev.pt", "resume.pt.tmp"
FRESH = -1      # the "epoch" of a start from scratch, in lists of offered epochs

# the config keys that shape the networks, the optimizers or the step (beside every ``alpha_*`` / ``lr_ratio_*`` key and
# every dropout rate of the configuration)
FINGERPRINT_KEYS = ("ae_form", "nstyle", "n_aux", "dim_in", "dim_out", "n_layers", "FC_discriminator_layers",
                    "batch_size", "optimizer_name", "precision", "rng_mode", "max_epoch", "epoch_stop_smooth",
                    "lr_base", "weight_decay", "dis_beta", "trial_seed", "sch_factor", "sch_patience")


def write_resume(work_dir, state):
    """``torch.save`` to ``resume.pt.tmp``, then the current ``resume.pt`` becomes ``resume.prev.pt``, then the new
    file becomes ``resume.pt``: a kill at any instant leaves at least one complete file."""
    path, prev, tmp = (os.path.join(work_dir, n) for n in (NAME, PREV_NAME, TMP_NAME))
    torch.save(state, tmp)
    if os.path.exists(path):
        os.replace(path, prev)
    os.replace(tmp, path)


def load_resume(path):
    """The file's dict, or None where there is no usable file (missing, cut short, another format version)."""
    try:
        state = torch.load(path, map_location="cpu", weights_only=True)
    except Exception:      # noqa: BLE001 -- a file cut short fails in the unpickler in many ways
        return None
    if not isinstance(state, dict) or state.get("version") != FORMAT_VERSION:
        return None
    return state


def generations(work_dir):
    """The usable files of a trial, newest first: ``[(path, state)]`` (at most two)."""
    found = []
    for name in (NAME, PREV_NAME):
        path = os.path.join(work_dir, name)
        state = load_resume(path)
        if state is not None:
            found.append((path, state))
    return sorted(found, key=lambda ps: -int(ps[1]["epoch"]))


def finished_state(work_dir):
    """The newest file's dict if it says ``finished`` (trained to the end, or diverged: ``error``), else None."""
    gens = generations(work_dir)
    return gens[0][1] if gens and gens[0][1].get("finished") else None


def offered_epochs(work_dir):
    """The epochs a trial can resume from: those of its two generations.  ``FRESH`` (the start of the run) is offered
    too by a trial without any file, and by one whose only file is the first a run can write -- the periodic file of
    epoch ``checkpoint_every - 1`` or a stop-time file before it: the generation before that file is the start.  Any
    other single file offers itself alone, so that lost files end in ``choose_group_epoch``'s error."""
    gens = [s for _, s in generations(work_dir) if not s.get("finished")]
    epochs = [int(s["epoch"]) for s in gens]
    if not epochs:
        return [FRESH]
    first = int(gens[0].get("checkpoint_every") or 0) - 1
    if len(epochs) == 1 and (epochs[0] == first or (gens[0].get("tail_pending") and epochs[0] < first)):
        return epochs + [FRESH]
    return epochs


def drop_newer(work_dir, epoch):
    """Remove the generations of a trial that are newer than ``epoch`` (the one its group resumes from; ``FRESH``:
    all); the older generation, if it is the chosen one, becomes ``resume.pt``."""
    path, prev = os.path.join(work_dir, NAME), os.path.join(work_dir, PREV_NAME)
    for p in (path, prev):
        st = load_resume(p)
        if st is not None and int(st["epoch"]) > epoch:
            os.remove(p)
    if not os.path.exists(path) and load_resume(prev) is not None:
        os.replace(prev, path)


def choose_group_epoch(offers):
    """The epoch a group of lockstep trials resumes from: the greatest one that every member offers.  The members write
    their files trial after trial at the same epoch, so their newest files differ by at most one generation; no common
    epoch means files were removed, and is a ``ValueError`` (never a silent restart)."""
    common = set(offers[0]).intersection(*map(set, offers[1:])) if offers else set()
    if not common:
        raise ValueError(f"resume: the trials of the group offer no common epoch to resume from ({list(offers)}; "
                         f"{FRESH} = from scratch): resume files are missing")
    return max(common)


def fingerprint(cfg, tile_mult, arena_n, n_train, n_val, train_spec):
    """What must be the same in the run that wrote a resume file and the run that continues from it."""
    cfg = dict(cfg)
    keys = set(FINGERPRINT_KEYS) | {k for k in cfg if k.startswith("alpha_") or k.startswith("lr_ratio_") or "dropout" in k}
    fp = {f"cfg.{k}": cfg.get(k) for k in sorted(keys)}
    fp = {k: (v if isinstance(v, (bool, int, float, str, type(None))) else repr(v)) for k, v in fp.items()}
    # `grad_clip_norm` shapes the step as well; absent and null are the same run (and the same entry-less fingerprint
    # as a file written before the key existed)
    if cfg.get("grad_clip_norm") is not None:
        fp["cfg.grad_clip_norm"] = float(cfg["grad_clip_norm"])
    # `ema_decay` likewise: the resume file carries the moving average, which a run with another decay would continue
    if cfg.get("ema_decay") is not None:
        fp["cfg.ema_decay"] = float(cfg["ema_decay"])
    # `spec_shift` likewise: a run with another largest shift would continue on differently augmented batches (the
    # draws themselves need nothing: they come from the engine's random state, which travels)
    if cfg.get("spec_shift") is not None:
        fp["cfg.spec_shift"] = float(cfg["spec_shift"])
    # `spec_broaden` likewise
    if cfg.get("spec_broaden") is not None:
        fp["cfg.spec_broaden"] = float(cfg["spec_broaden"])
    # `spec_gain` and `spec_tilt` likewise
    for key in ("spec_gain", "spec_tilt"):
        if cfg.get(key) is not None:
            fp["cfg." + key] = float(cfg[key])
    # `style_decorr` likewise: a run with another weight would continue on another phase-B gradient (its per-epoch
    # statistics are reset at every epoch boundary: the file carries nothing of them)
    if cfg.get("style_decorr") is not None:
        fp["cfg.style_decorr"] = float(cfg["style_decorr"])
    # `rank_loss_form` / `rank_temperature` likewise, when set: another form or temperature is another phase-B gradient
    if cfg.get("rank_loss_form") is not None:
        fp["cfg.rank_loss_form"] = str(cfg["rank_loss_form"])
    if cfg.get("rank_temperature") is not None:
        fp["cfg.rank_temperature"] = float(cfg["rank_temperature"])
    # (`rank_metrics` stays out: it adds a file beside the run and shapes nothing of the training, so a run may be
    # resumed with the key turned on or off)
    spec = np.asarray(train_spec, dtype=np.float64)
    fp.update({"tile_rows_mult": int(tile_mult), "arena.n": int(arena_n), "rows.train": int(n_train),
               "rows.val": int(n_val), "spectra.sum": float(spec.sum()), "spectra.sum_sq": float((spec * spec).sum())})
    return fp


def check_fingerprint(saved, now, path="resume.pt"):
    """``ValueError`` listing every entry that differs."""
    diff = [f"{k}: file {saved.get(k, '<absent>')!r}, now {now.get(k, '<absent>')!r}"
            for k in sorted(set(saved) | set(now)) if k not in saved or k not in now or saved[k] != now[k]]
    if diff:
        raise ValueError(f"resume: {path} was written by a different run; differing entries: " + "; ".join(diff))


def truncate_losses_csv(path, last_epoch):
    """Cut ``losses.csv`` down to its header and the rows with ``epoch <= last_epoch`` (rows are written every 10
    epochs, and the run went on after its last resume file); ``last_epoch < 0``: to nothing.  In place, so that a log
    handler that has the file open for appending goes on behind the kept rows.  ``rank_metrics.csv`` (a row every epoch,
    the epoch first) is cut by the same rule."""
    if not os.path.isfile(path):
        return
    with open(path, "r+b") as f:
        keep = 0
        if last_epoch >= 0:
            for line in f.readlines():
                if not line.endswith(b"\n"):
                    break               # a row cut short by the kill
                first = line.split(b",", 1)[0].strip()
                try:
                    if int(first) > last_epoch:
                        break
                except ValueError:
                    pass                # the header
                keep += len(line)
        f.truncate(keep)
