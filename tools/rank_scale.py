"""Rank loss at validation scale (VERDICT task 9): raae_rank_loss_fwd_bwd timings.

``--masked``: the masked form (raae_rank_loss_masked_fwd_bwd) beside the unmasked kernel at 256 and 4096 rows,
n_aux = 5: the two alternate inside one process, seven windows each, and the minimum, median and maximum over the windows
are printed per variant -- the unmasked kernel's own spread is what a difference has to be read against.  The masked
form is timed on the same fully labelled descriptors (same pairs, same work) and with 30 % of the cells NaN."""
import sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from rankaae_amd import ops, _lib
_lib.load()
dev = torch.device("cuda:0")


def inputs(n, k):
    g = torch.Generator().manual_seed(n)
    d = torch.randn(n, k, generator=g); d[:, 1] = torch.randint(4, 7, (n,), generator=g).float()
    z = torch.randn(n, 6, generator=g)
    return d, z, g


def window(fn, s, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(s):
        e0.record(s)
        for _ in range(reps):
            fn()
        e1.record(s)
    torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / reps


def masked_against_unmasked():
    k = 5
    for n in (256, 4096):
        d, z, g = inputs(n, k)
        gaps = d.clone()
        gaps[torch.rand(n, k, generator=g) < 0.3] = float("nan")
        d, gaps, z = d.to(dev), gaps.to(dev), z.to(dev)
        work = torch.empty(ops.rank_loss_masked_work_bytes(n, k), dtype=torch.uint8, device=dev)
        assert work.numel() >= ops.rank_loss_work_bytes(n, k)
        loss = torch.zeros(1, device=dev); dz = torch.empty(n, 6, device=dev)
        variants = {
            "unmasked": lambda: ops.rank_loss_fwd_bwd(d, k, z, 6, n, k, True, work, loss, dz),
            "masked, fully labelled": lambda: ops.rank_loss_masked_fwd_bwd(d, k, z, 6, n, k, True, work, loss, dz),
            "masked, 30 % NaN": lambda: ops.rank_loss_masked_fwd_bwd(gaps, k, z, 6, n, k, True, work, loss, dz),
        }
        s = torch.cuda.Stream()
        reps = 4000 if n == 256 else 1500          # >= 0.05 s per window
        times = {name: [] for name in variants}
        for name, fn in variants.items():          # warm-up
            window(fn, s, 50)
        for _ in range(7):
            for name, fn in variants.items():
                times[name].append(window(fn, s, reps))
        for name, t in times.items():
            t = sorted(t)
            print(f"n={n:5d}  {name:24s} min {t[0]:8.2f}  median {t[len(t) // 2]:8.2f}  max {t[-1]:8.2f} us per call "
                  f"({len(t)} windows of {reps} calls)")


if "--masked" in sys.argv[1:]:
    masked_against_unmasked()
    sys.exit(0)

for n in (256, 1050, 4096, 15000, 150000):
    k = 5
    d, z, g = inputs(n, k)
    d, z = d.to(dev), z.to(dev)
    work = torch.empty(ops.rank_loss_work_bytes(n, k), dtype=torch.uint8, device=dev)
    loss = torch.zeros(1, device=dev); dz = torch.empty(n, 6, device=dev)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        for _ in range(2):
            ops.rank_loss_fwd_bwd(d, k, z, 6, n, k, True, work, loss, dz)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        reps = 20 if n <= 15000 else 3
        e0.record(s)
        for _ in range(reps):
            ops.rank_loss_fwd_bwd(d, k, z, 6, n, k, True, work, loss, dz)
        e1.record(s)
    torch.cuda.synchronize()
    us = 1e3 * e0.elapsed_time(e1) / reps
    print(f"n={n:7d}  {us:10.1f} us per call  {n * n * k / us / 1e6:8.1f} T pair-ops/s  loss {float(loss):.6f}")
