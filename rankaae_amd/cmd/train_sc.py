#!/usr/bin/env python
"""``train_sc -c <config.yaml> [-w <work_dir>]`` -- same command line, per-trial directory layout
and log files as the reference's ``sc/cmd/train_sc.py:105-157`` (``training/job_<k>/{messages.txt,
losses.csv,final.pt}``, ``main_process_message.txt``; with the config key ``ema_decay`` also ``final_ema.pt``, the moving
average of the weights, and one ``EMA weights:`` line in ``messages.txt``; with ``rank_metrics: true`` also
``rank_metrics.csv``, one row of Kendall tau-b values per epoch), with the training itself on the MI355X HIP
engine.  The ipyparallel engine farm (``train_sc.py:19-45``) becomes one worker process per visible GPU:
trial ``k`` runs on worker ``k mod n`` and worker ``w`` uses GPU ``w mod ngpus`` (``RANKAAE_TRIAL_WORKERS``
overrides ``n``).  Several trials share a GPU (config key ``trials_per_gpu``, default 4 when ``trials > 1``): a 256-row
step is one serial chain of ~10 us kernels that leaves most of the chip idle, and the chains of independent trials
overlap on it.  ``trial_mode: auto`` (default) picks ``batched`` (``choose_trial_mode``) -- the trials of a group train
in LOCKSTEP and every training step of the group is ONE launch sequence whose kernels run with ``gridDim.z = trials``
(``rankaae_amd/trial_batch.py``; dense networks 6.2x the single-trial rate at 8 trials, 10x at 16) -- for both
networks at every batch size with ``rng_mode: philox`` and fp32, and ``threads`` otherwise.  ``trial_mode: threads``:
the trials of a worker run in threads of ONE process -- one engine, HIP stream and captured graph per trial, all of
them feeding the same device; every trial draws from its own host
generator (seeded ``trial_seed + k``; ``trial_seed`` defaults to a draw from the global generator), so a trial's result
does not depend on what runs beside it (tests/test_trainer_gpu.py).  ``trial_mode: processes``: one worker process per
concurrent trial, as in round 2.  When launched under
``torch.distributed.run`` (WORLD_SIZE > 1) every trial instead trains data-parallel over RCCL: all ranks run the trials
one after the other, each trial is ONE training run (``Trainer`` shards every global batch over the ranks and averages
the gradients, rankaae_amd/trainer.py), and rank 0 alone writes the logs, checkpoints and ``final.pt``."""
import argparse
import logging
import os
import signal
import sys
import threading
import time


import numpy as np
import torch

from rankaae_amd.logger import create_logger
from rankaae_amd import resume as resume_file
from rankaae_amd.parameter import Parameters, checkpoint_every_of, resume_on
from rankaae_amd.trainer import AnomalyError, Trainer


def timeout_handler(signum, frame):
    raise Exception("Training Overtime!")


def log_diverged(logger, exc):
    """A trial whose training raised ``AnomalyError`` (``detect_anomaly``): the error line in its ``messages.txt``, and
    no "Training finished" line -- the reference's trial leaves ``run_training`` with the exception there."""
    logger.error(f"{type(exc).__name__}: {exc}")


def diverged_trials(result):
    """Trial numbers (1-based) whose result holds an ``AnomalyError`` instead of metrics."""
    return [k + 1 for k, r in enumerate(result) if isinstance(r[0], AnomalyError)]


def _main_logger(work_dir):
    """The run's ``main_process_message.txt`` logger (``main`` made it; a worker process opens the file for appending)."""
    lg = logging.getLogger("Main training:")
    return lg if lg.handlers else create_logger("Main training:", f"{work_dir}/main_process_message.txt", append=True)


def skip_finished(job_number, work_dir, train_config):
    """``resume: true``: ``(metrics, 0.0)`` of a trial whose resume file says ``finished`` -- ``(AnomalyError, 0.0)``
    where it ended in one -- with one line in ``main_process_message.txt``; None for a trial that is to be trained."""
    if not resume_on(train_config):
        return None
    st = resume_file.finished_state(f"{work_dir}/training/job_{job_number + 1}")
    if st is None:
        return None
    if _is_lead_rank():
        _main_logger(work_dir).info(f"Trial {job_number + 1} {'diverged' if st['error'] is not None else 'finished'} in "
                                    f"an earlier run (epoch {st['epoch']}, resume.pt): not trained again.")
    return (AnomalyError(*st["error"]) if st["error"] is not None else list(st["metrics"])), 0.0


def trial_loggers(job_number, trial_dir, train_config):
    """The trial's ``messages.txt`` and ``losses.csv`` loggers: started afresh, or appended to where ``resume`` is on
    and the trial has a resume file (``Trainer`` cuts ``losses.csv`` back to the epoch it resumes from)."""
    append = resume_on(train_config) and any(os.path.exists(os.path.join(trial_dir, n))
                                             for n in (resume_file.NAME, resume_file.PREV_NAME))
    return (create_logger(f"subtraining_{job_number + 1}", os.path.join(trial_dir, "messages.txt"), append=append),
            create_logger(f"losses_{job_number + 1}", os.path.join(trial_dir, "losses.csv"), append=append, simple_fmt=True))


def run_training(job_number, work_dir, train_config, verbose, data_file, timeout_hours=0,
                 logger=logging.getLogger("training"), host_rng=None, init_lock=None):
    """``host_rng`` / ``init_lock``: thread mode (several trials in this process) -- the trial's own host generator, and
    the lock under which the global generator is seeded for the construction of ITS networks.  Returns
    ``(metrics, time_used)``, or ``(AnomalyError, time_used)`` for a trial that diverged (later trials still run)."""
    done = skip_finished(job_number, work_dir, train_config)
    if done is not None:
        return done
    work_dir = f"{work_dir}/training/job_{job_number + 1}"
    os.makedirs(work_dir, exist_ok=True)
    if _is_lead_rank():
        logger, loss_logger = trial_loggers(job_number, work_dir, train_config)
    else:       # data parallel: the trial is ONE training run on all ranks, rank 0 alone keeps the logs and files
        logger = loss_logger = _null_logger()
    ngpus = torch.cuda.device_count()
    local_id = int(os.environ.get("LOCAL_RANK", os.environ.get("SLURM_LOCALID", 0)))
    igpu = local_id % ngpus if ngpus > 0 else -1
    start = time.time()
    logger.info(f"Training started for trial {job_number + 1}.")
    if host_rng is None:
        trainer = Trainer.from_data(data_file, igpu=igpu, verbose=verbose, work_dir=work_dir,
                                    config_parameters=train_config, logger=logger, loss_logger=loss_logger)
    else:
        with init_lock:      # nn.Module constructors draw their initial weights from the GLOBAL generator
            torch.manual_seed(host_rng.initial_seed())
            trainer = Trainer.from_data(data_file, igpu=igpu, verbose=verbose, work_dir=work_dir,
                                        config_parameters=train_config, logger=logger, loss_logger=loss_logger,
                                        host_rng=host_rng)
    trainer.freeze_gc = bool(train_config.get("freeze_gc", host_rng is None))   # a dedicated training process: collector held off
    timer = None
    if host_rng is not None:
        # a thread: no signals here.  A timer asks the trainer to stop; train() raises the reference's exception at the
        # next epoch boundary
        if timeout_hours > 0:
            timer = threading.Timer(float(timeout_hours) * 3600.0, trainer.request_stop, args=("Training Overtime!",))
            timer.daemon = True
            timer.start()
        try:
            metrics = trainer.train()
        except AnomalyError as exc:
            log_diverged(logger, exc)
            return exc, time.time() - start
        finally:
            if timer is not None:
                timer.cancel()
            trainer.engine.release()          # graphs, workspaces and streams back now: more trials follow in this process
        logger.info(metrics)
        time_used = time.time() - start
        logger.info(f"Training finished. Time used: {time_used:.2f}s.\n\n")
        return metrics, time_used
    if int(os.environ.get("WORLD_SIZE", "1")) > 1 or checkpoint_every_of(train_config):
        # data parallel: the rank whose alarm fires must not leave the others waiting in a collective -- it asks the
        # trainer to stop, and every rank raises the reference's exception together at the next epoch boundary.  Resume
        # files on: the same request, so that the trial's file is written at that boundary before the exception
        # (raised from the handler it would cost the epochs since the last file)
        signal.signal(signal.SIGALRM, lambda signum, frame: trainer.request_stop("Training Overtime!"))
    else:
        signal.signal(signal.SIGALRM, timeout_handler)
    # (signal.setitimer: fractional hours work too -- signal.alarm(int(...)) of the reference rounds a sub-second
    # timeout to "never"; whole seconds behave identically)
    signal.setitimer(signal.ITIMER_REAL, max(0.0, float(timeout_hours) * 3600.0))
    try:
        metrics = trainer.train()
    except AnomalyError as exc:               # data parallel: every rank raises it at the same epoch
        log_diverged(logger, exc)
        return exc, time.time() - start
    finally:
        signal.setitimer(signal.ITIMER_REAL, 0.0)
        trainer.engine.release()              # graphs, workspaces and streams back now: more trials may follow
    logger.info(metrics)
    time_used = time.time() - start
    logger.info(f"Training finished. Time used: {time_used:.2f}s.\n\n")
    return metrics, time_used


def _is_lead_rank():
    return int(os.environ.get("WORLD_SIZE", "1")) == 1 or int(os.environ.get("RANK", "0")) == 0


def _null_logger():
    lg = logging.getLogger("rankaae_amd.null")
    if not lg.handlers:
        lg.addHandler(logging.NullHandler())
    lg.propagate = False
    return lg


def assign_trials(trials, nworkers):
    """Trial numbers of each worker: round-robin, like the reference's ipyparallel ``map_sync`` over engines that
    were given GPU ``id % ngpus`` (``train_sc.py:32-41``)."""
    return [list(range(w, trials, nworkers)) for w in range(nworkers)]


def _trial_worker(worker, jobs, work_dir, config_dict, verbose, data_file, timeout, threads=1, trial_seed=None, batched=False):
    # a spawned process: nothing has touched the GPU yet; LOCAL_RANK picks it in run_training
    os.environ["LOCAL_RANK"] = str(worker)
    cfg = Parameters(config_dict)
    if batched:
        return run_trials_batched(jobs, threads, work_dir, cfg, verbose, data_file, timeout, trial_seed, auto=batched == 2)
    if threads <= 1:
        return [(k,) + tuple(run_training(k, work_dir, cfg, verbose, data_file, timeout)) for k in jobs]
    return run_trials_threaded(jobs, threads, work_dir, cfg, verbose, data_file, timeout, trial_seed)


def run_trials_batched(jobs, per_batch, work_dir, train_config, verbose, data_file, timeout, trial_seed, auto=False):
    """The trials ``jobs`` of this process, ``per_batch`` at a time, each group trained in LOCKSTEP: every training step
    of the group is one launch sequence with ``gridDim.z = trials`` (``rankaae_amd.trainer.train_trials_batched``; both
    networks).  Seeds, files and log lines per trial as in the thread mode: ``[(k, metrics, time_used)]``."""
    from rankaae_amd.trainer import TrialsDiverged, train_trials_batched
    from rankaae_amd.trial_batch import BatchingRefused
    plain_config = train_config
    if train_config.get("ae_form", None) != "FC" and train_config.get("tile_rows_mult", None) is None:
        train_config = Parameters({**train_config.to_dict(),
                                   "tile_rows_mult": batched_tile_rows_mult(train_config.get("batch_size", 0))})
    ngpus = torch.cuda.device_count()
    local_id = int(os.environ.get("LOCAL_RANK", os.environ.get("SLURM_LOCALID", 0)))
    igpu = local_id % ngpus if ngpus > 0 else -1
    out = []
    for i in range(0, len(jobs), per_batch):
        group = []
        for k in jobs[i:i + per_batch]:
            # `resume`: the finished and the diverged trials of a group are left out, the rest resume from one epoch
            # (train_trials_batched); the groups themselves stay those of the first run, whose files agree
            done = skip_finished(k, work_dir, train_config)
            if done is not None:
                out.append((k,) + done)
            else:
                group.append(k)
        if not group:
            continue
        torch.cuda.set_device(max(igpu, 0))
        stream = torch.cuda.Stream()
        trainers, loggers = [], []
        start = time.time()
        for k in group:
            wd = f"{work_dir}/training/job_{k + 1}"
            os.makedirs(wd, exist_ok=True)
            logger, loss_logger = trial_loggers(k, wd, train_config)
            logger.info(f"Training started for trial {k + 1}.")
            g = torch.Generator()
            g.manual_seed(int(trial_seed) + k)
            torch.manual_seed(g.initial_seed())          # the networks' initial weights come from the global generator
            trainers.append(Trainer.from_data(data_file, igpu=igpu, verbose=verbose, work_dir=wd,
                                              config_parameters=train_config, logger=logger, loss_logger=loss_logger,
                                              host_rng=g, engine_stream=stream))
            loggers.append(logger)
        timer = None
        if timeout > 0:
            timer = threading.Timer(float(timeout) * 3600.0, lambda: [t.request_stop("Training Overtime!") for t in trainers])
            timer.daemon = True
            timer.start()
        refused = None
        errors = [None] * len(group)
        try:
            metrics = train_trials_batched(trainers)
        except TrialsDiverged as exc:
            # some trials of the group diverged (AnomalyError); the others trained to the end and wrote their files
            metrics, errors = exc.results, exc.errors
        except BatchingRefused as exc:
            # the first step of this configuration meets a kernel without the batched form (the per-layer conv kernels
            # of `fused_blocks: false`): `trial_mode: batched` says so; `auto` trains the group in threads instead, from
            # the start.  Anything else -- another HIP error, the reference's ValueError on a one-row last batch --
            # is the training's own failure and propagates in both modes
            if not auto:
                raise
            if resume_on(train_config):
                # the first run trained this configuration in threads (other tile_rows_mult for the conv networks, logs
                # begun there): it is resumed where it ran
                raise ValueError(f"resume: batched launches are refused for this configuration (kernel {exc.kernel}); "
                                 "resume it with trial_mode: threads") from exc
            refused = exc
        finally:
            if timer is not None:
                timer.cancel()
            for t in trainers:
                t.engine.release()
        if refused is not None:
            logging.getLogger("Main").warning(f"trial_mode auto: batched launches refused (kernel {refused.kernel}); "
                                              f"trials {[k + 1 for k in group]} run in threads")
            for k, lg in zip(group, loggers):
                for h in list(lg.handlers):
                    h.close()
                    lg.removeHandler(h)
                for name in ("messages.txt", "losses.csv"):      # the threaded rerun starts the trial's logs afresh
                    open(os.path.join(f"{work_dir}/training/job_{k + 1}", name), "w").close()
            del trainers
            out += run_trials_threaded(group, min(4, len(group)), work_dir, plain_config, verbose, data_file, timeout, trial_seed)
            continue
        time_used = time.time() - start
        for k, m, err, logger in zip(group, metrics, errors, loggers):
            if err is not None:
                log_diverged(logger, err)
                out.append((k, err, time_used))
                continue
            logger.info(m)
            logger.info(f"Training finished. Time used: {time_used:.2f}s.\n\n")
            out.append((k, m, time_used))
    return out


def run_trials_threaded(jobs, threads, work_dir, train_config, verbose, data_file, timeout, trial_seed):
    """The trials ``jobs`` of this process, ``threads`` at a time, each in a thread with its own engine / stream / graph
    and its own host generator (seed ``trial_seed + k``): ``[(k, metrics, time_used)]``."""
    from concurrent.futures import ThreadPoolExecutor
    if train_config.get("rng_mode", "philox") != "philox":
        raise ValueError("trial_mode: threads needs rng_mode: philox (the parity mode draws every random number of "
                         "every trial from the one global CPU generator: use trial_mode: processes)")
    init_lock = threading.Lock()

    def one(k):
        g = torch.Generator()
        g.manual_seed(int(trial_seed) + k)
        return (k,) + tuple(run_training(k, work_dir, train_config, verbose, data_file, timeout, host_rng=g,
                                         init_lock=init_lock))
    with ThreadPoolExecutor(max_workers=threads) as ex:
        return list(ex.map(one, jobs))


def batched_tile_rows_mult(batch_size):
    """``tile_rows_mult`` of ``trial_mode: batched`` for the conv networks (where the configuration leaves it unset).
    Below ``RAAE_BIG_ROWS`` (1024) rows 4: every trial's launches sized as its share of a 4x larger batch
    (raae_tile_hint; +33 % at 8 trials of 256 rows, +48 % at 16).  From 1024 rows on 1: there the launches already
    have the sample groups that 4 gives at 256 rows, and a batched trial is then bit for bit the same trial run under
    ``trial_mode: threads`` (tile_rows_mult 1 too), so ``auto`` choosing either changes no result.  Keyed on the mode
    and the batch size, never on the group size: a trial's result is the same whatever runs beside it."""
    return 4 if int(batch_size) < 1024 else 1


# `auto` keeps the conv networks' trials in threads from this batch size up.  None: batched wins at every size measured.
# 8 conv trials on one MI355X, aggregate steps/s, batched against 8 engines on their own streams:
# 1024 rows 1004 / 929 (1.08x), 2048 rows 620 / 404 (1.54x), 4096 rows 393 / 283 (1.39x).
AUTO_THREADS_FROM_ROWS = None


def choose_trial_mode(cfg):
    """The trial mode ``run_trials`` uses for the configuration ``cfg`` (a ``Parameters`` or a dict):
    ``"batched"``, ``"threads"`` or ``"processes"``.  ``trial_mode: auto`` picks ``batched`` where the trials can be
    batched (``rng_mode: philox``, ``precision: fp32``, the fused step head and discriminator; for the conv networks up
    to ``AUTO_THREADS_FROM_ROWS``), ``threads`` otherwise; ``batched`` on a configuration that cannot be batched
    raises ``ValueError``."""
    mode = str(cfg.get("trial_mode", "auto"))
    if mode not in ("auto", "batched", "threads", "processes"):
        raise ValueError(f"trial_mode must be 'auto', 'batched', 'threads' or 'processes', not {mode!r}")
    can_batch = (cfg.get("rng_mode", "philox") == "philox" and cfg.get("precision", "fp32") == "fp32" and
                 bool(cfg.get("fused_step_begin", True)) and bool(cfg.get("fused_discriminator", True)))
    if mode == "batched" and not can_batch:
        raise ValueError("trial_mode: batched needs rng_mode: philox, precision: fp32, fused_step_begin and "
                         "fused_discriminator (use trial_mode: threads)")
    if mode != "auto":
        return mode
    dense = cfg.get("ae_form", None) == "FC"
    wins = dense or AUTO_THREADS_FROM_ROWS is None or int(cfg.get("batch_size", 0)) < AUTO_THREADS_FROM_ROWS
    return "batched" if can_batch and wins else "threads"


def run_trials(trials, work_dir, train_config, verbose, data_file, timeout, logger):
    """All trials; returns ``[(metrics, time_used)]`` in trial order and the number of worker processes."""
    world = int(os.environ.get("WORLD_SIZE", "1"))
    nworkers = 1
    if resume_on(train_config) and trials > 1 and train_config.get("trial_seed", None) is None:
        raise ValueError("resume: a run of several trials needs trial_seed, so that trial k is rebuilt from the seed "
                         "it had when its resume file was written")
    philox = train_config.get("rng_mode", "philox") == "philox"
    auto = str(train_config.get("trial_mode", "auto")) == "auto"
    # one launch sequence for all trials of a group where the step's kernels have the batched form
    mode = choose_trial_mode(train_config)
    batched = (2 if auto else 1) if mode == "batched" else 0
    if batched:
        mode = "threads"          # same process / seed plumbing below; the worker trains its group in lockstep instead
    seeded = train_config.get("trial_seed", None) is not None
    if world == 1 and (trials > 1 or seeded) and mode == "threads" and philox:
        # one worker process per GPU; inside it `trials_per_gpu` trials at a time: in threads, or (dense networks) as
        # one batched launch sequence -- eight trials of a 256-row dense step still fit the chip side by side
        per_gpu = int(os.environ.get("RANKAAE_TRIALS_PER_GPU", train_config.get("trials_per_gpu", 8 if batched else 4)))
        ngpu = max(1, torch.cuda.device_count())
        nproc = max(1, min(int(os.environ.get("RANKAAE_TRIAL_WORKERS", ngpu)), trials))
        threads = max(1, min(per_gpu, -(-trials // nproc)))
        seed = train_config.get("trial_seed", None)
        if seed is None:
            seed = int(torch.empty((), dtype=torch.int64).random_().item()) & 0x3fffffff
        if nproc == 1:
            if batched:
                done = sorted(run_trials_batched(list(range(trials)), threads, work_dir, train_config, verbose, data_file,
                                                 timeout, seed, auto=batched == 2))
            else:
                done = sorted(run_trials_threaded(list(range(trials)), threads, work_dir, train_config, verbose, data_file,
                                                  timeout, seed))
            return [(m, t) for _, m, t in done], threads
        import multiprocessing as mp
        with mp.get_context("spawn").Pool(nproc) as pool:
            parts = pool.starmap(_trial_worker, [(w, jobs, work_dir, train_config.to_dict(), verbose, data_file, timeout,
                                                  threads, seed, batched) for w, jobs in enumerate(assign_trials(trials, nproc))])
        done = sorted(r for part in parts for r in part)
        return [(m, t) for _, m, t in done], nproc * threads
    if world == 1 and trials > 1:
        # device_count() does not initialise the GPU, so the workers can still be spawned after it
        # `trials_per_gpu` (config key, or RANKAAE_TRIALS_PER_GPU): worker processes that share one GPU.  At batches
        # below 2048 rows a trial's step is one serial chain of small kernels, and such chains of different
        # processes overlap on the chip: measured on one MI355X at B=256, conv networks: 727 steps/s alone,
        # 2 x 657, 4 x 509 (2035 in total), 6 workers 2225 in total.
        per_gpu = int(os.environ.get("RANKAAE_TRIALS_PER_GPU", train_config.get("trials_per_gpu", 1)))
        nworkers = int(os.environ.get("RANKAAE_TRIAL_WORKERS", torch.cuda.device_count() * max(1, per_gpu)))
        nworkers = max(1, min(nworkers, trials))
    if nworkers == 1:
        return [run_training(k, work_dir, train_config, verbose, data_file, timeout, logger) for k in range(trials)], 1
    import multiprocessing as mp
    with mp.get_context("spawn").Pool(nworkers) as pool:
        parts = pool.starmap(_trial_worker, [(w, jobs, work_dir, train_config.to_dict(), verbose, data_file, timeout)
                                             for w, jobs in enumerate(assign_trials(trials, nworkers))])
    done = sorted(r for part in parts for r in part)
    return [(m, t) for _, m, t in done], nworkers


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("-c", "--config", type=str, required=True, help="Config for training parameter in YAML format")
    parser.add_argument("-w", "--work_dir", type=str, default=".", help="Working directory to write the output files")
    args = parser.parse_args()
    work_dir = os.path.abspath(os.path.expanduser(args.work_dir))
    train_config = Parameters.from_yaml(os.path.join(work_dir, args.config))
    assert os.path.exists(work_dir)
    verbose = train_config.get("verbose", False)
    trials = train_config.get("trials", 1)
    data_file = os.path.join(work_dir, train_config.get("data_file", None))
    timeout = train_config.get("timeout", 10)
    logger = create_logger("Main training:", f"{work_dir}/main_process_message.txt", append=True) if _is_lead_rank() \
        else _null_logger()
    logger.info("START")
    start = time.time()
    result, nworkers = run_trials(trials, work_dir, train_config, verbose, data_file, timeout, logger)
    logger.info("Running with {} process(es).".format(max(nworkers, int(os.environ.get("WORLD_SIZE", "1")))))
    time_trials = np.array([r[1] for r in result])
    logger.info(f"Time used for each trial: {time_trials.mean():.2f} +/- {time_trials.std():.2f}s.\n" +
                " ".join([f"{t:.2f}s" for t in time_trials]))
    end = time.time()
    logger.info(f"Total time used: {end - start:.2f}s for {trials} trails ({(end - start) / trials:.2f} each on average).")
    failed = diverged_trials(result)
    if failed:
        # the reference's map_sync raises once its tasks are done: the other trials have written their files
        msg = f"Trials {failed} diverged: NaN gradients (detect_anomaly); see their messages.txt."
        logger.error(msg)
        sys.exit(msg)
    logger.info("END\n\n")


if __name__ == "__main__":
    main()
