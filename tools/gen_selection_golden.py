#!/usr/bin/env python
"""Generate ``tests/golden/selection_ref.json`` by running the REAL reference's report code on the CPU.

TEST INFRASTRUCTURE -- runs on the development machine only (the reference does not travel to the GPU machine).  It
imports ``sc.report.analysis`` and ``sc.report.generate_report`` unmodified, with empty stand-in modules for the
packages that are absent here and that the scoring never calls (``seaborn``, ``monty``, and -- pulled in by
``generate_report``'s imports of the trainer side -- ``torch_optimizer`` and ``torchvision.transforms``), in the style
of ``oracle/gen_golden.py``.  scipy, scikit-learn, numpy, matplotlib and plotly are the installed ones.  One adapter:
scikit-learn >= 1.6 returns a Python float from ``f1_score`` where the reference calls ``.tolist()`` on the result, so
the function is wrapped to return the same value as ``numpy.float64``, what the releases the reference was written
against returned.

Inputs come from ``rankaae_amd.synthetic.selection_inputs(seed, ...)`` and are NOT stored: the fixture keeps the seeds, a
SHA-256 of every input array, every job's rounded result dict as the reference returns it, and the z-scores, final
scores and rank order of ``sort_all_models(..., sort_score=sorting_algorithm, ascending=False)``.  Jobs are fed in
sorted name order.  The arrays reach the reference wrapped as constant encoder / decoder callables.

Two conditions are ASSERTED on the reference's own output, and another seed is tried if one fails, so that a test may
compare rank order exactly and values within one unit of the fourth decimal:
  * neighbouring final scores differ by at least 1e-3;
  * no reported value lies within 1e-7 of a 4-decimal rounding boundary (checked on the unrounded values, which are
    captured by wrapping ``round`` / ``np.round`` as the reference's modules see them).  1e-7 is ten times the largest
    legitimate difference between two correct evaluations (the per-spectrum MAE, an fp32 mean in scikit-learn and a
    double sum on the device: ~1e-8); every other value is double arithmetic on both sides.  A wider band cannot be
    met: a case reports ~340 values, and a band of +-2e-5 covers 40 % of every 1e-4 interval, so no seed passes (100
    seeds tried, none did).

Usage:  python tools/gen_selection_golden.py
"""
import builtins
import hashlib
import json
import os
import sys
import types

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
REFERENCE = os.environ.get("RANKAAE_REFERENCE", "/root/reference")

from rankaae_amd.synthetic import selection_inputs  # noqa: E402

CASES = [dict(name="main", n_jobs=8, n_rows=1000, nstyle=6, n_aux=5, n_points=32, four_class_job=None, top_n=5),
         dict(name="small", n_jobs=4, n_rows=300, nstyle=4, n_aux=3, n_points=16, four_class_job=2, top_n=20)]


def _install_shims():
    sys.modules.setdefault("seaborn", types.ModuleType("seaborn"))
    monty, mjson = types.ModuleType("monty"), types.ModuleType("monty.json")
    mjson.MSONable = object
    monty.json = mjson
    sys.modules.setdefault("monty", monty)
    sys.modules.setdefault("monty.json", mjson)
    to = types.ModuleType("torch_optimizer")
    to.AdaBound = to.RAdam = object
    sys.modules.setdefault("torch_optimizer", to)
    tv, tr = types.ModuleType("torchvision"), types.ModuleType("torchvision.transforms")
    tr.Compose = object
    tv.transforms = tr
    sys.modules.setdefault("torchvision", tv)
    sys.modules.setdefault("torchvision.transforms", tr)
    sys.path.insert(0, REFERENCE)


class _Const:
    """A constant network: returns its array whatever it is given (``evaluate_model`` calls ``encoder(spec_in)`` and
    ``decoder(styles)``)."""

    def __init__(self, array):
        self.t = torch.tensor(array)

    def eval(self):
        return self

    def __call__(self, x):
        return self.t


class _Ds:
    def __init__(self, spec, aux):
        self.spec, self.aux = spec, aux


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def run_case(analysis, gr, case, seed):
    """Returns the fixture entry, or None if the reference's output misses one of the two asserted conditions."""
    kw = {k: case[k] for k in ("n_jobs", "n_rows", "nstyle", "n_aux", "n_points", "four_class_job")}
    inputs = selection_inputs(seed, **kw)
    unrounded = []

    def np_round(a, decimals=0, *args, **kwargs):
        if decimals == 4:
            unrounded.extend(np.atleast_1d(np.asarray(a, dtype=np.float64)).ravel().tolist())
        return np.round(a, decimals, *args, **kwargs)

    def py_round(x, ndigits=None):
        if ndigits == 4:
            unrounded.append(float(x))
        return builtins.round(x, ndigits)

    analysis.np = types.SimpleNamespace(**{k: getattr(np, k) for k in dir(np) if not k.startswith("__")})
    analysis.np.round = np_round
    analysis.round = py_round
    f1_score = analysis.f1_score
    analysis.f1_score = lambda *a, **k: np.float64(f1_score(*a, **k))
    try:
        results, hashes = {}, {}
        for j, (z, aux, si, so) in enumerate(inputs):
            job = f"job_{j + 1}"
            assert z.dtype == np.float32 and si.dtype == np.float32 and so.dtype == np.float32 and aux.dtype == np.float64
            model = {"Encoder": _Const(z), "Decoder": _Const(so)}
            results[job] = analysis.evaluate_model(_Ds(si, aux), model)
            hashes[job] = dict(styles=sha(z), aux=sha(aux), spec_in=sha(si), spec_out=sha(so))
        cap = {}

        def sort_score(z):
            cap["z_scores"] = z.copy()
            cap["final"] = gr.sorting_algorithm(z)
            return cap["final"]
        ordered = {job: results[job] for job in sorted(results)}
        ordered, ranked_jobs, _ = analysis.sort_all_models(ordered, sort_score=sort_score, plot_score=False,
                                                           ascending=False, top_n=case["top_n"])
    finally:
        analysis.np = np
        analysis.f1_score = f1_score
        del analysis.round
    final = np.sort(cap["final"])
    if len(final) > 1 and np.min(np.diff(final)) < 1e-3:
        return None
    for v in unrounded:
        if np.isfinite(v) and abs(abs(v * 1e4 - np.floor(v * 1e4)) - 0.5) < 1e-3:     # 1e-7 in units of 1e-4
            return None
    jobs = {}
    for job, res in ordered.items():
        jobs[job] = {k: v for k, v in res.items() if k not in ("Input", "Output")}
        jobs[job]["Style-descriptor Corr"] = {str(i): v for i, v in res["Style-descriptor Corr"].items()}
    return dict(name=case["name"], seed=seed, **kw, top_n=case["top_n"], sha256=hashes, jobs=jobs,
                job_order=sorted(results), z_scores=cap["z_scores"].tolist(), final_scores=cap["final"].tolist(),
                ranked_jobs=[str(j) for j in ranked_jobs])


def main():
    _install_shims()
    import scipy
    import sklearn
    import sc.report.analysis as analysis
    import sc.report.generate_report as gr
    out = dict(generator="tools/gen_selection_golden.py", versions=dict(numpy=np.__version__, scipy=scipy.__version__,
                                                                        sklearn=sklearn.__version__), cases=[])
    for case in CASES:
        for seed in range(2024, 2124):
            entry = run_case(analysis, gr, case, seed)
            if entry is not None:
                break
            print(f"case {case['name']}: seed {seed} misses a condition, trying the next")
        else:
            raise SystemExit(f"case {case['name']}: no seed satisfies the conditions")
        print(f"case {case['name']}: seed {seed}, rank order {entry['ranked_jobs']}")
        out["cases"].append(entry)
    path = os.path.join(REPO, "tests", "golden", "selection_ref.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
