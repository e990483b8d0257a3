"""raae_kendall_tau beside the pass over the same pairs that validation already runs, raae_rank_loss_fwd_bwd with
dz = NULL, at the same shapes in one process ("Rank metrics"): 1050 and 15000 rows, n_aux = 5, one
heavily tied descriptor column.

A call is two launches of tens of microseconds, so a bracketed eager call would time the host's submission: each
variant's call is captured 20 times into one hipGraph, and a replay of that graph is timed between two events
(raae_event_record / raae_event_elapsed_ms).  The two variants alternate; 5 warm-up replays each, then the median,
minimum and maximum of 30, in microseconds per call.  One JSON line per shape."""
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rankaae_amd import ops  # noqa: E402
from rankaae_amd.metrics import KendallTau  # noqa: E402

DEV = torch.device("cuda:0")
CALLS, REPEATS, WARM = 20, 30, 5

for n in (1050, 15000):
    n_aux, ns = 5, 6
    rng = np.random.default_rng(n)
    d = rng.normal(size=(n, n_aux)).astype(np.float32)
    d[:, 1] = rng.integers(0, 5, size=n)                   # a coordination-number column: heavy ties
    z = (0.5 * np.pad(d, ((0, 0), (0, 1))) + rng.normal(size=(n, ns))).astype(np.float32)
    dd, zz = torch.from_numpy(d).to(DEV), torch.from_numpy(z).to(DEV)
    kt = KendallTau(n, n_aux, DEV)
    work = torch.empty(ops.rank_loss_work_bytes(n, n_aux), dtype=torch.uint8, device=DEV)
    loss = torch.zeros(1, device=DEV)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        fns = {"kendall_tau": lambda: kt.launch(dd, zz),
               "rank_loss_val": lambda: ops.rank_loss_fwd_bwd(dd, n_aux, zz, ns, n, n_aux, True, work, loss, None)}
        graphs = {}
        for name, fn in fns.items():
            fn()
            stream.synchronize()
            g = ops.Graph()
            g.begin()
            for _ in range(CALLS):
                fn()
            g.end()
            graphs[name] = g
        times = {name: [] for name in fns}
        e0, e1 = ops.Event(), ops.Event()
        for rep in range(WARM + REPEATS):
            for name, g in graphs.items():
                e0.record()
                g.launch()
                e1.record()
                us = 1e3 * e0.elapsed_ms(e1) / CALLS         # (elapsed_ms synchronises on the second event)
                if rep >= WARM:
                    times[name].append(us)
        stream.synchronize()
    res = {name: dict(median_us=statistics.median(t), min_us=min(t), max_us=max(t)) for name, t in times.items()}
    res["ratio"] = res["kendall_tau"]["median_us"] / res["rank_loss_val"]["median_us"]
    res["work_bytes"] = ops.kendall_tau_work_bytes(n, n_aux)
    print(json.dumps({"rows": n, "n_aux": n_aux, **res}), flush=True)
