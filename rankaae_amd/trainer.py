"""``Trainer`` -- drop-in for the reference's ``sc/clustering/trainer.py:33-474`` on MI355X.

Same constructor / ``from_data`` / ``train(callback)`` surface, same files written
(``losses.csv`` rows, ``final.pt`` / ``best.pt`` / ``checkpoints/`` whole-module pickles with the
reference's dict keys), same per-epoch validation, metrics, model selection and
``ReduceLROnPlateau`` schedule.  Everything from the batch loop downward (trainer.py:103-268)
runs as HIP kernels through ``rankaae_amd.engine.StepEngine``; there is no PyTorch/CPU fallback.

Build-only config keys (all optional, defaults preserve reference behaviour):
  ``rng_mode``  "philox" (device Philox tape, default) | "host" (reference-order CPU draws; parity)
  ``use_graph`` True: replay one captured hipGraph per step
  ``seed``      Philox seed (``rng_mode: philox``); default: drawn from the global torch generator, i.e. a different
                random stream for every trial of a run, as in the reference (whose trials are independent draws)
  ``detect_anomaly`` True (default, the reference's ``set_detect_anomaly(True)``): a NaN parameter gradient ends
                ``train()`` with ``AnomalyError`` at the end of its epoch, before anything of that epoch is logged or saved
  ``ema_decay`` a number in (0, 1) (default absent: off): the engine keeps a moving average of the weights; after the last
                epoch it is validated once (one ``EMA weights:`` log line) and written as ``final_ema.pt``
  ``spec_shift`` a number > 0 (default absent: off): every training step resamples each row of its batch at a random energy
                shift of up to that many grid points, on the device, before the spectral noise; validation never shifts
  ``spec_broaden`` a number s > 0 with ceil(3 s) <= 64 (default absent: off): every training step convolves each row of its
                batch with a Gaussian of a random width of up to s grid points, on the device, before the shift and the
                spectral noise; validation never broadens
  ``spec_gain`` a number a with 0 < a < 1 (default absent: off): every training step multiplies each row of its batch by a
                random factor in [1 - a, 1 + a), on the device, behind the shift and before the spectral noise (an edge
                step normalised a few per cent wrong); validation never scales
  ``spec_tilt`` a number t > 0 (default absent: off): every training step adds to each row of its batch a linear ramp of a
                random height of up to t at the ends (-c at the first sample, +c at the last, |c| <= t), on the device,
                behind the gain and before the spectral noise (a background not quite removed); validation never tilts
  ``rank_metrics`` true | false (default): every epoch's validation also forms Kendall's tau-b of each descriptor against
                its style on the device, over the validation rows labelled for it, and rank 0 appends one row to
                ``rank_metrics.csv`` (``Epoch,Tau_*,Labelled_*``); nothing else a run writes or returns changes
  ``style_decorr`` a number w > 0 (default absent: off): phase B of every training step minimises ``aux_loss + w * D``, ``D``
                the mean squared off-diagonal Pearson correlation of the styles over the batch (its exact gradient is added
                on the device); one ``messages.txt`` line per epoch with the epoch's mean ``D``; no logged loss changes
  ``rank_loss_form`` ``linear`` (default) | ``logistic``: with ``logistic`` phase B of every training step minimises the
                pairwise logistic loss ``T * softplus(-s * (z_i - z_j) / T)`` over the labelled pairs instead of the
                reference's linear one (``rank_temperature: T``, default 1.0, in style standard deviations);
                ``kendall_activation`` is not applied to it; ``Train_Aux`` is that loss, ``Val_Aux`` stays the linear one

Data parallel (the north star's replacement of the ipyparallel trial farm): started under
``torch.distributed.run`` (WORLD_SIZE > 1) every rank builds the same ``Trainer``; rank r steps rows
``[r*b, (r+1)*b)`` of each global batch of ``W*b`` rows of the SAME epoch permutation (rank 0's), the five per-phase
gradient arenas are averaged over RCCL inside the step, BatchNorm running statistics are averaged over the ranks
before each validation, the metrics list is rank 0's on every rank (so the five ReduceLROnPlateau schedules stay in
lockstep), and only rank 0 writes ``losses.csv`` / checkpoints / ``final.pt``.
"""
import copy
import logging
import gc
import os
import shutil

import numpy as np
import torch

from .dataloader import get_dataloaders
from .engine import OPT_NAMES, StepEngine
from .model import AE_CLS_DICT, DiscriminatorFC
from .parameter import (Parameters, check_optimizer, checkpoint_every_of, detect_anomaly_on, ema_decay_of,
                        grad_clip_norm_of, rank_loss_form_of, rank_metrics_on, resume_on, spec_broaden_of, spec_gain_of,
                        spec_shift_of, spec_tilt_of, style_decorr_of)
from . import resume as resume_file


class AnomalyError(RuntimeError):
    """A parameter gradient held a NaN (config key ``detect_anomaly``): the reference's anomaly mode raises
    ``RuntimeError: Function '...Backward0' returned nan values in its ...th output.`` from the backward of that step.
    Here the optimizer update of ``phase`` (``engine.OPT_NAMES``) saw it at its step count ``step`` (1-based), and
    ``Trainer.train`` raises at the end of ``epoch``, before that epoch's log row, checkpoints and schedulers."""

    def __init__(self, phase, step, epoch):
        self.phase, self.step, self.epoch = phase, step, epoch
        what = f"{phase} backward" if phase is not None else "backward on another rank"
        super().__init__(f"Function '{what}' returned nan values in its parameter gradient at optimizer step {step}, "
                         f"epoch {epoch} (detect_anomaly)")

    def __reduce__(self):           # pickles through train_sc's worker processes
        return type(self), (self.phase, self.step, self.epoch)


class TrialsDiverged(RuntimeError):
    """``train_trials_batched``: some trials of the batch raised ``AnomalyError``; the others trained to the end and
    wrote their files.  ``results[i]``: trial i's metrics (None where it diverged); ``errors[i]``: its
    ``AnomalyError`` (None where it finished)."""

    def __init__(self, results, errors):
        self.results, self.errors = results, errors
        bad = [i for i, e in enumerate(errors) if e is not None]
        super().__init__(f"trials {bad} of the batch diverged: " + "; ".join(str(errors[i]) for i in bad))


def alpha(epoch_percentage, step=800, limit=0.7):
    """Gradient-reversal ramp (reference ``sc/utils/functions.py:214-219``)."""
    return (2. / (1. + np.exp(-1.0E4 / step * epoch_percentage)) - 1) * limit


class PlateauScheduler:
    """``ReduceLROnPlateau(mode="min", threshold_mode="rel", cooldown=0, min_lr=0, eps=1e-8)`` as
    the reference configures it (trainer.py:400-408), acting on one engine optimizer."""

    def __init__(self, opt, factor, patience, threshold=0.01):
        self.opt, self.factor, self.patience, self.threshold = opt, factor, patience, threshold
        self.best, self.num_bad_epochs = float("inf"), 0

    def step(self, metric):
        metric = float(metric)
        if metric < self.best * (1.0 - self.threshold):
            self.best, self.num_bad_epochs = metric, 0
        else:
            self.num_bad_epochs += 1
        if self.num_bad_epochs > self.patience:
            new_lr = max(self.opt.lr * self.factor, 0.0)
            if self.opt.lr - new_lr > 1e-8:
                self.opt.lr = new_lr
                self.opt.push()
            self.num_bad_epochs = 0

    def state_dict(self):
        """Everything ``step`` reads except the optimizer's own ``lr`` (part of the engine's state)."""
        return {"best": float(self.best), "num_bad_epochs": int(self.num_bad_epochs), "factor": float(self.factor),
                "patience": int(self.patience), "threshold": float(self.threshold)}

    def load_state_dict(self, state):
        self.best, self.num_bad_epochs = float(state["best"]), int(state["num_bad_epochs"])
        self.factor, self.patience, self.threshold = float(state["factor"]), int(state["patience"]), float(state["threshold"])


class Trainer:
    metric_weights = [1.0, -1.0, -0.01, -1.0, -1.0]
    gau_kernel_size = 17

    def __init__(self, encoder, decoder, discriminator, device, train_loader, val_loader, verbose=True,
                 work_dir='.', tb_logdir="runs", config_parameters=Parameters({}),
                 logger=logging.getLogger("training"), loss_logger=logging.getLogger("losses"), engine_stream=None):
        self.logger, self.loss_logger = logger, loss_logger
        self.device = device
        self.encoder, self.decoder, self.discriminator = encoder, decoder, discriminator
        self.train_loader, self.val_loader = train_loader, val_loader
        self.verbose, self.work_dir, self.tb_logdir = verbose, work_dir, tb_logdir
        self.epoch_stop_smooth = 500
        # build-only key `freeze_gc` (default off for library use; `train_sc` and bench.py turn it on): after the second
        # epoch the long-lived objects of the run move to the cyclic collector's permanent generation for the rest of
        # train(), and come back out in a `finally` (process-global state: an embedding application opts in)
        self.freeze_gc = False
        self.__dict__.update(config_parameters.to_dict())
        if not self.gradient_reversal or self.use_cnn_discriminator:
            raise ValueError("only gradient_reversal: true with DiscriminatorFC is reachable in the reference "
                             "(SURVEY.md finding 4)")
        cfg = config_parameters.to_dict()
        check_optimizer(cfg)        # before anything touches the GPU
        self.grad_clip_norm = grad_clip_norm_of(cfg)
        self.ema_decay = ema_decay_of(cfg)
        self.spec_shift = spec_shift_of(cfg)
        self.spec_broaden = spec_broaden_of(cfg)
        self.spec_gain = spec_gain_of(cfg)
        self.spec_tilt = spec_tilt_of(cfg)
        self.detect_anomaly = detect_anomaly_on(cfg)
        self.rank_metrics = rank_metrics_on(cfg)
        self.style_decorr = style_decorr_of(cfg)
        self.rank_loss_form, self.rank_temperature = rank_loss_form_of(cfg, self._world_size())
        # `checkpoint_every` / `resume` (rankaae_amd/resume.py): the trial's resume file at epoch boundaries.  Refused
        # where it cannot be checked: data parallel (per-rank generator state, the private communicator's lifetime) and
        # the parity mode (its random tape is drawn from the global CPU generator in the reference's order)
        self.checkpoint_every, self.resume = checkpoint_every_of(cfg), resume_on(cfg)
        if (self.checkpoint_every or self.resume) and (self._world_size() > 1 or cfg.get("rng_mode", "philox") != "philox"):
            raise ValueError("checkpoint_every / resume: single-process runs only")
        self._restored, self._fingerprint = None, None
        self.world, self.rank, self.pg = self._data_parallel_setup(device)
        # one draw from the global generator per trial (also when `seed` is given, so that the generator's state
        # does not depend on the key): trials of one run then use different noise / dropout / latent streams
        # (the training loader's generator: the global one unless the trial was given its own -- train_sc's thread mode)
        host_rng = getattr(train_loader, "generator", None)
        drawn = int(torch.empty((), dtype=torch.int64).random_(generator=host_rng).item()) & 0x7fffffff if cfg.get("rng_mode", "philox") == "philox" else 0
        seed = int(cfg.get("seed", drawn)) + self.rank
        self.engine = StepEngine(encoder, decoder, discriminator, cfg, device,
                                 rng_mode=cfg.get("rng_mode", "philox"), seed=seed,
                                 use_graph=cfg.get("use_graph", True), world_size=self.world, rank=self.rank,
                                 process_group=self.pg, stream=engine_stream)
        ds = train_loader.dataset
        if ds.aux is None:
            raise ValueError("n_aux: 0 is not reachable in the reference (SURVEY.md finding 4)")
        # NaN descriptor cells are missing labels.  Decided once, over the training and validation splits together: any
        # such cell and the run uses the masked rank loss throughout; none and it launches what it always launched
        splits = [ds.aux, getattr(getattr(val_loader, "dataset", None), "aux", None)]
        self.aux_missing = any(a is not None and bool(np.isnan(np.asarray(a, dtype=np.float64)).any()) for a in splits)
        if self.aux_missing:
            lab = np.concatenate([~np.isnan(np.asarray(a, dtype=np.float64)) for a in splits if a is not None])
            self.logger.info("Missing descriptors (NaN AUX cells): labelled fraction per descriptor " +
                             ", ".join(f"AUX_{k}: {f:.4f}" for k, f in enumerate(lab.mean(axis=0))) +
                             "; the rank loss pairs only rows labelled for a descriptor.")
        self.engine.set_data(ds.spec, ds.aux, aux_missing=self.aux_missing)
        self.load_optimizers()
        self.load_schedulers()

    @staticmethod
    def _world_size():
        import torch.distributed as dist
        world = int(os.environ.get("WORLD_SIZE", "1"))
        if world == 1 and dist.is_available() and dist.is_initialized():
            world = dist.get_world_size()
        return world

    @staticmethod
    def _data_parallel_setup(device):
        """``(world, rank, process group)``: data parallel when started under ``torch.distributed.run``.  The process
        group is created here if the launcher's caller has not done so (backend RCCL; ``RANKAAE_DP_BACKEND=gloo``
        rehearses the path with several ranks on one GPU)."""
        import torch.distributed as dist
        world = int(os.environ.get("WORLD_SIZE", "1"))
        if world == 1 and not (dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1):
            return 1, 0, None
        if not dist.is_initialized():
            os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
            backend = os.environ.get("RANKAAE_DP_BACKEND", "nccl")
            if backend == "nccl":
                dist.init_process_group("nccl", device_id=device)
            else:
                dist.init_process_group(backend)
        return dist.get_world_size(), dist.get_rank(), None

    def load_optimizers(self):
        self.optimizers = self.engine.opts

    def load_schedulers(self):
        self.schedulers = {name: PlateauScheduler(opt, self.sch_factor, self.sch_patience)
                           for name, opt in self.optimizers.items()}

    def zerograd(self):
        """Gradients live in per-phase slabs that every backward overwrites: nothing to clear."""

    def _model_dict(self):
        """Whole-module pickles under the reference's keys (trainer.py:281-283), detached from the
        engine's arena so the file holds plain, individually-owned tensors."""
        self.engine.sync_bn_counters()
        out = {}
        for key, mod in (("Encoder", self.encoder), ("Decoder", self.decoder),
                         ("Style Discriminator", self.discriminator)):
            m = copy.deepcopy(mod)
            for p in m.parameters():
                p.data = p.data.clone()
            out[key] = m
        return out

    def train(self, callback=None):
        eng = self.engine
        try:
            # _train_epochs is a generator that hands every training step out as ("step", rows, smooth): here the
            # trial's own engine runs it; train_trials_batched runs the same request of T trials as ONE launch sequence
            gen = self._train_epochs(callback)
            try:
                req = next(gen)
                while True:
                    if req[0] == "step":
                        eng.step(req[1], smooth=req[2])
                        req = next(gen)
                    else:                                   # ("validate", spec, aux) -> (styles, losses)
                        req = gen.send(eng.validate(req[1], req[2]))
            except StopIteration as done:
                return done.value
        finally:
            # a worker process runs several trials: the next one must be able to collect this one's objects -- also when
            # the run ends in an exception (the SIGALRM "Training Overtime!", a caller's try/except around train())
            if self._gc_frozen:
                gc.unfreeze()
                self._gc_frozen = False
            # every rank reaches this point at the same place in the program: release the private RCCL communicator
            # here, not from __del__ at whatever allocation the cyclic collector happens to run
            eng.close()

    def request_stop(self, reason="Training Overtime!"):
        """Ask ``train()`` to end with ``Exception(reason)`` at the next epoch boundary -- on EVERY rank of a
        data-parallel run (the flag is OR-reduced over the ranks beside the per-epoch metrics broadcast), so that no
        rank is left waiting in a collective.  ``train_sc``'s per-trial SIGALRM calls this under data parallelism
        (reference: the handler raises at once, sc/cmd/train_sc.py:21-22; with one process that is what still happens)."""
        self._stop_reason = reason

    _stop_reason = None

    _gc_frozen = False

    # -- the trial's resume file (config keys `checkpoint_every` / `resume`; rankaae_amd/resume.py)
    def _resume_fingerprint(self):
        if self._fingerprint is None:
            eng, ds = self.engine, self.train_loader.dataset
            self._fingerprint = resume_file.fingerprint(eng.cfg, eng.tile_mult, eng.arena.n, len(ds),
                                                        len(self.val_loader.dataset), ds.spec)
        return self._fingerprint

    def _write_resume(self, epoch, metrics, best_combined_metric, best_chpt_file, tail_pending=False, finished=False,
                      error=None):
        """The state between two epochs: ``epoch`` is the last one trained and validated.  ``tail_pending``: written by
        a stop request, which ends the run before that epoch's checkpoint rule, scheduler steps and callback -- the
        resumed run does them first.  ``error``: the ``(phase, step, epoch)`` of the ``AnomalyError`` that ended the
        trial; such a file holds no state (it is full of NaN) and only says that the trial is not to be trained again."""
        state = {"version": resume_file.FORMAT_VERSION, "finished": bool(finished), "epoch": int(epoch),
                 "error": None if error is None else [error[0], int(error[1]), int(error[2])],
                 "tail_pending": bool(tail_pending), "metrics": None if metrics is None else [float(m) for m in metrics],
                 "best_combined_metric": float(best_combined_metric),
                 "best_chpt_file": None if best_chpt_file is None else os.path.basename(best_chpt_file),
                 "checkpoint_every": int(self.checkpoint_every),
                 "fingerprint": self._resume_fingerprint()}
        if error is None:
            g = getattr(self.train_loader, "generator", None)
            state.update(engine=self.engine.state(), host_rng=g.get_state() if g is not None else torch.get_rng_state(),
                         schedulers=[sch.state_dict() for sch in self.schedulers.values()])
        resume_file.write_resume(self.work_dir, state)

    def _restore(self, epoch=None):
        """``resume: true``: load the newest usable generation of the trial's resume file (``epoch``: the generation of
        that epoch -- the one a batched group agreed on; ``resume_file.FRESH``: none), check its fingerprint, and put
        back the engine, the host generator and the schedulers.  Once per trainer, before its first step.  Returns the
        file's dict, or False where the trial starts from epoch 0."""
        if self._restored is not None:
            return self._restored
        gens = resume_file.generations(self.work_dir) if self.resume else []
        if epoch is not None:
            gens = [g_ for g_ in gens if int(g_[1]["epoch"]) == epoch and not g_[1].get("finished")]
            if epoch != resume_file.FRESH and not gens:
                raise ValueError(f"resume: {self.work_dir} has no resume file of epoch {epoch}")
            if self.resume:
                # a generation newer than the epoch the group agreed on goes: kept, it would stand beside the file this
                # trial writes next, and the group's next kill could leave it without a common epoch
                resume_file.drop_newer(self.work_dir, epoch)
                gens = [g_ for g_ in resume_file.generations(self.work_dir) if int(g_[1]["epoch"]) == epoch] if gens else []
        self._restored = False
        if gens:
            path, st = gens[0]
            resume_file.check_fingerprint(st["fingerprint"], self._resume_fingerprint(), path)
            if st["error"] is None:
                self.engine.load_state(st["engine"])
                g = getattr(self.train_loader, "generator", None)
                if g is not None:
                    g.set_state(st["host_rng"])
                else:
                    torch.set_rng_state(st["host_rng"])
                for sch, sd in zip(self.schedulers.values(), st["schedulers"]):
                    sch.load_state_dict(sd)
            self.logger.info(f"Resuming from {path}: epoch {st['epoch']}" + (" (finished)" if st["finished"] else ""))
            self._restored = st
        return self._restored

    def _train_epochs(self, callback):
        from .parallel import any_rank, broadcast_from_rank0, broadcast_tensor_from_rank0, epoch_schedule
        eng = self.engine
        lead = self.rank == 0
        best_combined_metric = 10.0
        chkpt_dir = f"{self.work_dir}/checkpoints"
        st = self._restore() if self.resume else False
        if st and st["error"] is not None:      # the trial diverged in the earlier run: it does so again, untrained
            raise AnomalyError(*st["error"])
        if st and st["finished"]:
            return list(st["metrics"])
        if lead:
            os.makedirs(chkpt_dir, exist_ok=True)
        if lead and self.spec_shift is not None:
            self.logger.info(f"spec_shift: rows shifted by up to ±{self.spec_shift:g} grid points")
        if lead and self.spec_broaden is not None:
            self.logger.info(f"spec_broaden: rows broadened by a Gaussian of up to σ = {self.spec_broaden:g} grid points")
        if lead and self.spec_gain is not None:
            self.logger.info(f"spec_gain: rows scaled by a factor in [1 − {self.spec_gain:g}, 1 + {self.spec_gain:g})")
        if lead and self.spec_tilt is not None:
            self.logger.info(f"spec_tilt: rows tilted by a ramp of up to ±{self.spec_tilt:g} at the ends")
        if lead and self.style_decorr is not None:
            self.logger.info(f"style_decorr: w = {self.style_decorr:g} (phase B minimises aux_loss + w * D, D the mean "
                             "squared off-diagonal correlation of the styles over the batch)")
        if lead and self.rank_loss_form == "logistic":
            self.logger.info(f"rank_loss_form: logistic, rank_temperature T = {self.rank_temperature:g} (phase B minimises "
                             "T * softplus(-s * (z_i - z_j) / T) over the labelled pairs; Train_Aux is that loss, Val_Aux "
                             "stays the linear rank loss)")
            self.logger.info("rank_loss_form: logistic: kendall_activation is not applied to the training rank loss (the "
                             "sigmoid is the pair weight)")
        if lead and self.rank_metrics:
            self.logger.info("rank_metrics: Kendall tau-b of every descriptor's style on the validation split, every epoch")
        best_chpt_file, metrics = None, None
        if lead and self.resume:
            # rows are written every 10 epochs and the run went on after its last resume file: back to that epoch
            resume_file.truncate_losses_csv(f"{self.work_dir}/losses.csv", st["epoch"] if st else resume_file.FRESH)
        rank_csv = f"{self.work_dir}/rank_metrics.csv"
        if lead and self.rank_metrics:
            # one row per epoch, appended and closed (so flushed) every epoch.  A run from scratch starts the file; a
            # resumed one cuts it back to the epoch it resumes from and goes on behind the kept rows -- or starts it
            # there, where the earlier run did not have the key
            if self.resume:
                resume_file.truncate_losses_csv(rank_csv, st["epoch"] if st else resume_file.FRESH)
            if not self.resume or not os.path.isfile(rank_csv) or os.path.getsize(rank_csv) == 0:
                n_aux = eng.n_aux
                with open(rank_csv, "w") as f:
                    f.write(",".join(["Epoch"] + [f"Tau_{k}" for k in range(n_aux)] +
                                     [f"Labelled_{k}" for k in range(n_aux)]) + "\n")
        if lead and not st:
            self.loss_logger.info(
                "Epoch,Train_D,Val_D,Train_G,Val_G,Train_Aux,Val_Aux,Train_Recon,"
                "Val_Recon,Train_Smooth,Val_Smooth,Train_Mutual_Info,Val_Mutual_Info")
        vds = self.val_loader.dataset
        val_spec = torch.as_tensor(vds.spec, dtype=torch.float32).contiguous().to(self.device)
        val_aux = torch.as_tensor(vds.aux, dtype=torch.float32).contiguous().to(self.device)
        self._val_split = (val_spec, val_aux)       # (train_trials_batched: a diverged trial's plane still validates)
        n_train, bs = len(self.train_loader.dataset), self.train_loader.batch_size
        # single GPU: every batch of the reference's loader incl. the ragged last one; data parallel: every full
        # global batch of world * bs rows, the tail split evenly over the ranks (parallel.epoch_schedule)
        schedule = epoch_schedule(n_train, self.world, bs)
        n_batch = len(schedule)
        bn_buffers = [b_ for mod in (self.encoder, self.decoder) for name, b_ in mod.named_buffers()
                      if name.endswith("running_mean") or name.endswith("running_var")]

        def finish_epoch(epoch, metrics):
            """What follows an epoch's validation: the checkpoint rule, the scheduler steps, the callback, and the
            periodic resume file."""
            nonlocal best_combined_metric, best_chpt_file
            combined_metric = -(np.array(self.metric_weights) * np.array(metrics)).sum()
            if combined_metric > best_combined_metric:
                best_combined_metric = combined_metric
                best_chpt_file = f"{chkpt_dir}/epoch_{epoch:06d}_loss_{combined_metric:07.6g}.pt"
                if lead:
                    torch.save(self._model_dict(), best_chpt_file)
            for sch in self.schedulers.values():
                sch.step(combined_metric)
            if callback is not None:
                callback(epoch, metrics)
            if self.checkpoint_every and (epoch + 1) % self.checkpoint_every == 0:
                self._write_resume(epoch, metrics, best_combined_metric, best_chpt_file)

        first_epoch = 0
        if st:
            first_epoch, metrics = st["epoch"] + 1, st["metrics"]
            best_combined_metric = st["best_combined_metric"]
            if st["best_chpt_file"] is not None:
                best_chpt_file = f"{chkpt_dir}/{st['best_chpt_file']}"
            if st["tail_pending"]:          # a stop request ended the earlier run before this part of its last epoch
                finish_epoch(st["epoch"], metrics)
        # (the collector is held off once plans and captured graphs exist: after the second epoch of a run from
        # scratch, after the first one of a resumed run)
        freeze_epoch = 1 if first_epoch == 0 else first_epoch
        clipped_before = eng.clipped_steps()        # (None without `grad_clip_norm`; a resumed run: the restored counts)
        for epoch in range(first_epoch, self.max_epoch):
            alpha_ = alpha(epoch / self.max_epoch, self.alpha_flat_step, self.alpha_limit)
            perm = broadcast_tensor_from_rank0(self.train_loader.epoch_permutation(), self.device, self.pg)
            eng.set_epoch(perm, alpha_)
            smooth = epoch < self.epoch_stop_smooth
            prev_rows = None
            for rows, off, global_rows in schedule:
                if self.world > 1 and rows != prev_rows:      # first step of the epoch, and again at the tail
                    eng.seek(off + self.rank * rows, global_rows)
                prev_rows = rows
                yield ("step", rows, smooth)
            if epoch == freeze_epoch and self.freeze_gc and not self._gc_frozen:
                # plans, captured graphs and modules are long-lived: out of the cyclic collector's way (a full
                # collection in the middle of an epoch stalls the host for longer than the queue of launched steps lasts)
                gc.collect()
                gc.freeze()
                self._gc_frozen = True
            tl = eng.losses()
            if self.detect_anomaly:
                nan = eng.anomaly()     # read by losses(): no synchronisation of its own
                # data parallel: the gradients were all-reduced before the update, so every rank saw the NaN; the
                # agreement still makes all ranks raise here together (none is left waiting in a collective)
                if self.world > 1 and any_rank(nan is not None, self.device, self.pg) and nan is None:
                    nan = (None, 0)
                if nan is not None:
                    if self.checkpoint_every:       # a finished file: `resume` does not train this trial again
                        self._write_resume(epoch, None, best_combined_metric, best_chpt_file, finished=True,
                                           error=(nan[0], nan[1], epoch))
                    raise AnomalyError(nan[0], nan[1], epoch)
            if self.grad_clip_norm is not None:
                # (read by losses(), like the anomaly flags; the counters run over the whole training)
                clipped = eng.clipped_steps()
                steps = [n_batch if (name != "smoothness" or smooth) else 0 for name in OPT_NAMES]
                if lead:
                    self.logger.info(f"Epoch {epoch}: grad_clip_norm {self.grad_clip_norm:g}: " + ", ".join(
                        f"{name} clipped {k - k0} of {n} steps"
                        for name, k, k0, n in zip(OPT_NAMES, clipped, clipped_before, steps)))
                clipped_before = clipped
            if self.style_decorr is not None:
                # (read by losses(), like the anomaly flags; the sums start again with every epoch.  Data parallel: each
                # rank penalises its own rows, the line is rank 0's mean)
                d_mean, d_steps = eng.style_decorr_stats(reset=True)
                if lead:
                    self.logger.info(f"Epoch {epoch}: style_decorr: mean D = {d_mean:.6f} over {d_steps} steps")
            if not smooth:
                tl["smooth"] = 0.0
            if self.world > 1:
                eng.average_over_ranks(bn_buffers)
            z, vl = yield ("validate", val_spec, val_aux)
            if epoch % 10 == 0 and lead:
                self.loss_logger.info(
                    f"{epoch:d},\t"
                    f"{tl['adversarial']:.6f},\t{vl['adversarial']:.6f},\t"
                    f"{0.0:.6f},\t{0.0:.6f},\t"
                    f"{tl['kendall']:.6f},\t{vl['kendall']:.6f},\t"
                    f"{tl['recon']:.6f},\t{vl['recon']:.6f},\t"
                    f"{tl['smooth']:.6f},\t{vl['smooth']:.6f},\t"
                    f"{tl['mutual_info']:.6f},\t{vl['mutual_info']:.6f},\t")
            avg_mutual_info = tl["mi_accum"] / n_batch
            # shapiro(x).statistic per style / spearmanr(.).correlation per pair of the reference
            # (trainer.py:286-292), formed on the device by raae_style_metrics
            style_shapiro, style_rho = eng.val_style_metrics()
            style_coupling = np.max(np.fabs(style_rho))
            if lead and self.rank_metrics:
                tau, counts = eng.val_rank_metrics()
                with open(rank_csv, "a") as f:
                    f.write(",".join([f"{epoch:d}"] + [f"{t:.6f}" for t in tau] + [f"{int(m):d}" for m in counts[:, 5]]) + "\n")
            metrics = [float(np.min(style_shapiro)), vl["recon"], avg_mutual_info, float(style_coupling),
                       vl["kendall"]]
            metrics = broadcast_from_rank0(metrics, self.device, self.pg)     # no-op on one GPU
            if self.world > 1 and any_rank(self._stop_reason is not None, self.device, self.pg):
                # a rank's timeout fired: all ranks leave here together (a rank raising on its own would leave the
                # others waiting in the next step's all-reduce)
                raise Exception(self._stop_reason or "Training Overtime!")
            if self.world == 1 and self._stop_reason is not None:      # thread mode of train_sc: a timer asked for it
                if self.checkpoint_every:       # what the GPU computed so far stays: the resumed run finishes this epoch
                    self._write_resume(epoch, metrics, best_combined_metric, best_chpt_file, tail_pending=True)
                raise Exception(self._stop_reason)
            finish_epoch(epoch, metrics)
        if lead:
            torch.save(self._model_dict(), f"{self.work_dir}/final.pt")
            if best_chpt_file is not None:
                shutil.copy2(best_chpt_file, f"{self.work_dir}/best.pt")
        if self.ema_decay is not None:
            # `ema_decay`: one validation with the moving average in place of the weights, and `final_ema.pt` -- the
            # dict of `final.pt` with the averaged parameters (the BatchNorm buffers are the live modules': they are
            # not averaged).  Everything above came from the live weights; nothing below reaches the returned metrics.
            # (Data parallel: the validation holds collectives, so every rank runs it; rank 0 logs and writes.)
            with eng.ema_weights():
                _, vl = eng.validate(val_spec, val_aux)
                style_shapiro, style_rho = eng.val_style_metrics()
                if lead:
                    ema_metrics = [float(np.min(style_shapiro)), vl["recon"], vl["mutual_info"],
                                   float(np.max(np.fabs(style_rho))), vl["kendall"]]
                    self.logger.info(
                        f"EMA weights: decay {self.ema_decay:g}; validation losses " +
                        ", ".join(f"{k} {vl[k]:.6f}" for k in ("adversarial", "kendall", "recon", "mutual_info", "smooth")) +
                        "; metrics (min Shapiro W, recon, validation mutual info, max |Spearman rho|, kendall) " +
                        ", ".join(f"{m:.6f}" for m in ema_metrics))
                    if self.rank_metrics:
                        self.logger.info("EMA rank metrics: Kendall tau-b per descriptor " +
                                         ", ".join(f"{t:.6f}" for t in eng.val_rank_metrics()[0]))
                    torch.save(self._model_dict(), f"{self.work_dir}/final_ema.pt")
        if lead:
            if self.checkpoint_every and metrics is not None:
                # `resume` (train_sc) skips a trial whose file says so
                self._write_resume(self.max_epoch - 1, metrics, best_combined_metric, best_chpt_file, finished=True)
        return metrics

    @classmethod
    def from_data(cls, csv_fn, igpu=0, verbose=True, work_dir='.', train_ratio=0.7, validation_ratio=0.15,
                  test_ratio=0.15, config_parameters=Parameters({}), logger=logging.getLogger("from_data"),
                  loss_logger=logging.getLogger("losses"), arrays=None, host_rng=None, engine_stream=None):
        """``host_rng`` (build-only): a private ``torch.Generator`` for this trial's epoch permutations and device-RNG
        seed instead of the global CPU generator (several trials in one process).  ``engine_stream``: the HIP stream
        the engine works on (the trials of a ``TrialBatch`` share one)."""
        p = config_parameters
        assert p.ae_form in AE_CLS_DICT
        dl_train, dl_val, _ = get_dataloaders(csv_fn, p.batch_size, (train_ratio, validation_ratio, test_ratio),
                                              n_aux=p.n_aux, arrays=arrays, generator=host_rng)
        if not torch.cuda.is_available():
            raise RuntimeError("rankaae_amd needs an MI355X GPU: the training path has no CPU fallback "
                               "(the reference would log 'Use Slow CPU!' here)")
        if verbose:
            logger.info("Use GPU")
        device = torch.device(f"cuda:{max(igpu, 0)}")
        torch.cuda.set_device(device)
        encoder = AE_CLS_DICT[p.ae_form]["encoder"](nstyle=p.nstyle, dropout_rate=p.dropout_rate, dim_in=p.dim_in,
                                                    n_layers=p.n_layers)
        decoder = AE_CLS_DICT[p.ae_form]["decoder"](nstyle=p.nstyle, dropout_rate=p.dropout_rate,
                                                    last_layer_activation=p.decoder_activation, dim_out=p.dim_out,
                                                    n_layers=p.n_layers)
        if p.use_cnn_discriminator:
            raise ValueError("use_cnn_discriminator: true is broken in the reference (SURVEY.md finding 4)")
        discriminator = DiscriminatorFC(nstyle=p.nstyle, dropout_rate=p.dis_dropout_rate, noise=p.dis_noise,
                                        layers=p.FC_discriminator_layers)
        return cls(encoder, decoder, discriminator, device, dl_train, dl_val, verbose=verbose, work_dir=work_dir,
                   config_parameters=p, logger=logger, loss_logger=loss_logger, engine_stream=engine_stream)


def train_trials_batched(trainers, callbacks=None):
    """``train()`` of T trainers of ONE configuration in lockstep, every training step of the T trials as one launch
    sequence with ``gridDim.z = T`` (``rankaae_amd.trial_batch.TrialBatch``; dense networks).  Everything around the
    step -- epoch permutation, validation, metrics, schedulers, checkpoints, log rows -- is each trainer's own code,
    run trial after trial between the steps.  Returns the trials' metrics lists.  A trial that asks to stop
    (``request_stop``) ends the whole batch with the reference's exception: the trials advance together.  A trial whose
    ``train()`` raises ``AnomalyError`` (``detect_anomaly``) ends alone: the others go on, and once they have finished
    (and written their files) ``TrialsDiverged`` carries every trial's metrics or error."""
    from .trial_batch import TrialBatch
    callbacks = callbacks or [None] * len(trainers)
    if any(t.resume for t in trainers):
        # the trials advance together, so they resume from ONE epoch: the greatest that every member's two generations
        # of resume files offer (the engines are restored here, before the batch is built)
        if any(resume_file.finished_state(t.work_dir) is not None for t in trainers):
            raise ValueError("resume: a trial of the batch has finished (or diverged) already; leave it out of the group")
        common = resume_file.choose_group_epoch([resume_file.offered_epochs(t.work_dir) if t.resume else
                                                 [resume_file.FRESH] for t in trainers])
        for t in trainers:
            t._restore(common)
    batch = TrialBatch([t.engine for t in trainers])
    gens = [t._train_epochs(cb) for t, cb in zip(trainers, callbacks)]
    T = len(trainers)
    results, errors = [None] * T, [None] * T

    def advance(i, answer):
        try:
            return next(gens[i]) if answer is None else gens[i].send(answer)
        except StopIteration as done:
            results[i] = done.value
        except AnomalyError as exc:
            errors[i] = exc
        return None

    def advance_all(answers):
        """Every live trial one request further.  A stop request that ends one trial ends the batch; with resume files
        on, the others are asked to stop too and write theirs at this epoch before the exception goes on."""
        out, stopped = [None] * T, None
        for i in range(T):
            if reqs[i] is None:
                continue
            try:
                out[i] = advance(i, answers[i])
            except Exception as exc:      # noqa: BLE001 -- re-raised below, or here
                # only the stop exception itself (`raise Exception(reason)` of _train_epochs): a failed file write, say,
                # propagates as it is
                if type(exc) is not Exception or trainers[i]._stop_reason is None or str(exc) != str(trainers[i]._stop_reason):
                    raise
                if stopped is None:
                    if not trainers[i].checkpoint_every:
                        raise
                    stopped = exc
                    for t in trainers[i + 1:]:
                        t.request_stop(trainers[i]._stop_reason)
        if stopped is not None:
            raise stopped
        return out

    try:
        reqs = [advance(i, None) for i in range(T)]
        while True:
            live = [i for i in range(T) if reqs[i] is not None]
            if not live:
                break
            r0 = reqs[live[0]]
            finished = [i for i in range(T) if reqs[i] is None and errors[i] is None]
            if finished or any(reqs[i][0] != r0[0] or (r0[0] == "step" and reqs[i] != r0) for i in live):
                raise RuntimeError(f"the trials of a batch left lockstep: {[r and r[:1] for r in reqs]}")
            if r0[0] == "step":
                # a diverged trial's grid plane is stepped too (the batch's launch sequence covers all T planes, and
                # planes are independent); its results are never read.  Nobody starts its epochs any more: it reads
                # the first rows of its last permutation at every step
                for i in range(T):
                    if errors[i] is not None:
                        trainers[i].engine.seek(0)
                batch.step(r0[1], smooth=r0[2])
                answers = [None] * T
            else:
                # ... and validated on its own split, its answer dropped.  Its NaN weights keep every kernel of the
                # validation in bounds: the one index formed from the data, the sorted slot of style_rank_kernel
                # (raae_metrics.hip), counts comparisons that are false for NaN and stays in [0, n)
                val = [reqs[i][1:] if reqs[i] is not None else trainers[i]._val_split for i in range(T)]
                answers = batch.validate([v[0] for v in val], [v[1] for v in val])
            reqs = advance_all(answers)
        if any(e is not None for e in errors):
            raise TrialsDiverged(results, errors)
        return results
    finally:
        for g in gens:
            g.close()
        for t in trainers:
            if t._gc_frozen:
                gc.unfreeze()
                t._gc_frozen = False
            t.engine.close()
        batch.release()
