"""Aggregate training-step rate of T independent conv-network trials on one GPU at batch sizes ``bench.py``'s trials
leg does not cover: T engines on their own streams stepped round-robin from one host thread (what ``train_sc``'s
thread mode runs) against ONE ``TrialBatch`` launch sequence with ``gridDim.z = T`` (its batched mode).

    python tools/trial_batch_rate.py --batch 2048,4096 --rows 7000,100000 --trials 1,8,16 --reps 3

Every (batch, rows, T) point is measured ``--reps`` times, threads and batched alternating; one JSON line per point
with the aggregate five-phase steps/s of each repetition and the batched / threads ratio of the medians.
"""
import argparse
import gc
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bench import BASE_CFG, build_models            # noqa: E402
from rankaae_amd.dataloader import split_counts     # noqa: E402
from rankaae_amd.engine import StepEngine           # noqa: E402
from rankaae_amd.synthetic import make_spectra      # noqa: E402
from rankaae_amd.trial_batch import TrialBatch      # noqa: E402


def rate(mode, T, b, cfg, dev, spec, aux, seconds):
    n_train = split_counts(len(spec))[0]
    full = n_train // b
    stream = TrialBatch.shared_stream(dev) if mode == "batched" else None
    engs = []
    for t in range(T):
        enc, dec, dis = build_models(cfg, 1234 + t)
        e = StepEngine(enc, dec, dis, cfg, dev, rng_mode="philox", seed=99 + t, use_graph=True, stream=stream)
        e.set_data(spec[:n_train], aux[:n_train])
        engs.append(e)
    batch = TrialBatch(engs) if mode == "batched" else None
    gen = torch.Generator().manual_seed(7)
    i = 0

    def one_round():
        nonlocal i
        if i % full == 0:
            for e in engs:
                e.set_epoch(torch.randperm(n_train, generator=gen), 0.7172)
        if batch is not None:
            batch.step(b, smooth=True)
        else:
            for e in engs:
                e.step(b, smooth=True)
        i += 1
    for _ in range(3):              # eager / captured / replayed
        one_round()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(4):
        one_round()
    torch.cuda.synchronize()
    rounds = max(8, int(seconds / ((time.perf_counter() - t0) / 4)))
    t0 = time.perf_counter()
    for _ in range(rounds):
        one_round()
    if batch is None:
        for e in engs:
            e.finish()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    if batch is not None:
        batch.release()
    for e in engs:
        e.release()
    del engs, batch
    gc.collect()
    torch.cuda.empty_cache()
    return T * rounds / dt


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--batch", default="2048,4096")
    ap.add_argument("--rows", default="7000,100000", help="synthetic spectra (the train split is 70 %%)")
    ap.add_argument("--trials", default="1,8,16")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--modes", default="threads,batched")
    ap.add_argument("--seconds", type=float, default=1.5, help="timed seconds per measurement (about)")
    ap.add_argument("--tile-rows-mult", type=int, default=1, help="tile_rows_mult of both modes (train_sc: 1 from 1024 rows)")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    modes = args.modes.split(",")
    for rows in [int(x) for x in args.rows.split(",")]:
        spec, aux, _ = make_spectra(rows, BASE_CFG["dim_in"], BASE_CFG["n_aux"], seed=0)
        for b in [int(x) for x in args.batch.split(",")]:
            cfg = dict(BASE_CFG, ae_form="compact", batch_size=b, tile_rows_mult=args.tile_rows_mult)
            for T in [int(x) for x in args.trials.split(",")]:
                got = {m: [] for m in modes}
                for _ in range(args.reps):
                    for m in modes:
                        got[m].append(round(rate(m, T, b, cfg, dev, spec, aux, args.seconds), 1))
                med = {m: sorted(v)[len(v) // 2] for m, v in got.items()}
                line = {"rows": rows, "batch": b, "trials": T, "tile_rows_mult": args.tile_rows_mult,
                        "aggregate_steps_per_s": got, "median": med}
                if "threads" in med and "batched" in med:
                    line["batched_over_threads"] = round(med["batched"] / med["threads"], 3)
                print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
