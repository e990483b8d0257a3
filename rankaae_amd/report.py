"""Model selection over the trained trials: the reference's ``sc/report/analysis.py`` (``evaluate_model``,
``evaluate_all_models``, ``sort_all_models``) and ``sc/report/generate_report.py`` (``sorting_algorithm``, the writers)
with the evaluation on the HIP engine.

Per ``training/job_*/final.pt`` the eval-mode encoder and decoder run over the validation split on the GPU and
``raae_select_scores`` forms the selection scores there (``rankaae_amd/csrc/raae_select.hip``); the host reads one
block of doubles per model and rounds it into the reference's result dict -- same keys, nesting and 4-decimal rounding.
Ranking (seven score columns, population z-scores, weights ``[-1, 0, 1, 1, 1, 1, 1]``) is a few dozen numbers and
stays in numpy, line for line the reference's.

Deviations, both deliberate:

* jobs are visited in SORTED NAME order (``job_1, job_10, job_2, ...``: plain string order); the reference iterates
  ``os.listdir``, whose order is arbitrary, and ties of the final score come out in reversed iteration order, so a
  defined order makes the ranking reproducible;
* no seaborn / monty / plotly: figures are matplotlib only and are drawn by the command, not here.
"""
import ctypes as C
import json
import os
import pickle
from collections import OrderedDict

import numpy as np
import torch

from . import _lib, ops
from ._lib import SEL_HEAD, SEL_STRIDE, check

# the thresholds of get_confusion_matrix (analysis.py:244), uploaded as they are: the kernel compares against this table
THRESH_GRID = np.linspace(-3.5, 3.5, 700)

SCORE_NAMES = ["Inter-style Corr", "Reconstuction Err", "Style_1 - CT Corr", "Style_2 - CN Corr", "Style_3 - OCN Corr",
               "Style_4 - Rstd Corr", "Style_5 - OO Corr"]

# what an engine built only to run eval forwards still has to be told (its optimizers are never stepped)
_INFERENCE_CFG = dict(lr_base=1e-3, optimizer_name="AdamW", dis_beta=1.0, lr_ratio_dis=1, lr_ratio_Corr=1,
                      lr_ratio_Reconn=1, lr_ratio_Mutual=1, lr_ratio_Smooth=1, weight_decay=0.0, batch_size=64,
                      kendall_activation=False, spec_noise=0.0, use_flex_spec_target=False, detect_anomaly=False)


# ------------------------------------------------------------------------------------------------ the device side
class SelectionScorer:
    """Device buffers of one model's ``raae_select_scores`` call.  ``launch`` enqueues the four kernels on the current
    stream (capturable, recordable); ``read`` copies the block back."""

    def __init__(self, n, k, n_aux, L, device, masked=False):
        self.n, self.k, self.n_aux, self.L = int(n), int(k), int(n_aux), int(L)
        self.masked = bool(masked)        # some descriptor cells are NaN (missing labels): the masked kernels
        self.thresh = torch.tensor(THRESH_GRID, dtype=torch.float64, device=device)
        self.work = torch.empty(ops.select_work_bytes(n, k, n_aux, self.thresh.numel(), self.masked), dtype=torch.uint8,
                                device=device)
        self.out = torch.zeros(SEL_HEAD + SEL_STRIDE * n_aux, dtype=torch.float64, device=device)

    def launch(self, styles, aux, spec_in, spec_out):
        ops.select_scores(styles, self.n, self.k, aux, self.n_aux, spec_in, spec_out, self.L, self.thresh, self.work,
                          self.out, masked=self.masked)

    def read(self):
        return self.out.cpu().numpy()


def _r4(x):
    return np.round(float(x), 4).tolist()


def has_missing(*aux):
    """Whether any descriptor cell of the given arrays is NaN, i.e. a missing label (None entries are skipped).  Asked
    once, where the data is loaded: the answer picks the masked kernels for the whole run."""
    return any(a is not None and bool(np.isnan(np.asarray(a)).any()) for a in aux)


def labelled_counts(aux):
    """Labelled (non-NaN) rows per descriptor column."""
    return (~np.isnan(np.asarray(aux, dtype=np.float64))).sum(axis=0)


def result_from_block(block, n_aux, labelled=None):
    """The reference's result dict (without ``Input`` / ``Output``) from one model's block of doubles, rounded where and
    how ``analysis.py`` rounds: Python ``round`` for the reconstruction error, the F1 score, the thresholds and the
    inter-style correlation, ``np.round`` for the rest; ``residue`` is a one-element list, as ``np.round`` of lstsq's
    residual array gives it.  ``labelled``: labelled rows per descriptor (``labelled_counts``); a descriptor with fewer
    than 3 is ``None``, which ``score_matrix`` scores like a missing descriptor."""
    block = np.asarray(block, dtype=np.float64)
    corr = {}
    for i in range(n_aux):
        o = block[SEL_HEAD + SEL_STRIDE * i:SEL_HEAD + SEL_STRIDE * (i + 1)]
        if labelled is not None and labelled[i] < 3:
            corr[i] = None
        elif i == 1:
            if o[0] == 0.0:
                corr[i] = None
                continue
            i45, i56 = int(o[2]), int(o[3])
            assert o[4] == THRESH_GRID[i45] and o[5] == THRESH_GRID[i56]
            corr[i] = {"F1 score": round(float(o[1]), 4), "CN45 Threshold": round(float(THRESH_GRID[i45]), 4),
                       "CN56 Threshold": round(float(THRESH_GRID[i56]), 4)}
        else:
            if np.isnan(o[1]):
                # a descriptor with one value on every (labelled) row: the kernel's slope is 0 / 0.  The reference's
                # linregress raises there; a NaN score must not reach the ranking
                raise ValueError(f"descriptor {i} is constant over the validation rows: cannot calculate a linear "
                                 "regression if all x values are identical")
            corr[i] = {"Spearman": _r4(o[0]),
                       "Linear": {"slope": _r4(o[1]), "intercept": _r4(o[2]), "R2": _r4(o[3])},
                       "Quadratic": {"Parameters": np.round(o[4:7], 4).tolist(), "residue": np.round(o[7:8], 4).tolist(),
                                     "R2": _r4(o[8])}}
    return {"Style-descriptor Corr": corr, "Input": None, "Output": None,
            "Reconstruct Err": [round(float(block[0]), 4), round(float(block[1]), 4)],
            "Inter-style Corr": round(float(block[2]), 4)}


def _device_inputs(styles, aux, spec_in, spec_out, device):
    f32 = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32)).to(device)      # noqa: E731
    return f32(styles), torch.as_tensor(np.ascontiguousarray(aux, dtype=np.float64)).to(device), f32(spec_in), f32(spec_out)


def score_arrays(styles, aux, spec_in, spec_out, device=None):
    """One model's unrounded block for host arrays ``styles [n, k]``, ``aux [n, n_aux]``, ``spec_in`` / ``spec_out``
    ``[n, L]`` (single-model launches).  NaN cells of ``aux`` are missing labels."""
    device = device or torch.device("cuda:0")
    z, a, si, so = _device_inputs(styles, aux, spec_in, spec_out, device)
    sc = SelectionScorer(z.shape[0], z.shape[1], a.shape[1], si.shape[1], device, masked=has_missing(aux))
    sc.launch(z, a, si, so)
    return sc.read()


class BatchedProgram:
    """J structurally identical launch sequences as ONE sequence with ``gridDim.z = J`` (``raae_record_*`` /
    ``raae_multi_*``, the machinery of ``TrialBatch``).  ``emitters[j]()`` enqueues model j's launches; they run once
    eagerly while the library logs them (that is how the recorder works), ``launch()`` then replays all J as one
    sequence.  ``BatchedProgram.build`` returns None where a launch has no batched form or the sequences differ."""

    def __init__(self, prog, J):
        self.prog, self.J = prog, J

    @classmethod
    def build(cls, emitters):
        lib = _lib.load()
        handles, ok = [], True
        for emit in emitters:
            check(lib.raae_record_begin(), "raae_record_begin")
            try:
                emit()
            finally:
                h, n = C.c_void_p(), C.c_int(0)
                rc = lib.raae_record_end(C.byref(h), C.byref(n))
            if rc != 0:
                ok = False
                break
            handles.append(h)
        prog = C.c_void_p()
        if ok:
            torch.cuda.synchronize()
            ok = lib.raae_multi_build((C.c_void_p * len(handles))(*[h.value for h in handles]), len(handles),
                                      C.byref(prog)) == 0
        for h in handles:
            lib.raae_record_free(h)
        return cls(prog, len(handles)) if ok else None

    def launch(self):
        check(_lib.load().raae_multi_launch(self.prog, ops._stream()), "raae_multi_launch")

    def count(self):
        return _lib.load().raae_multi_count(self.prog)

    def release(self):
        if self.prog is not None:
            torch.cuda.synchronize()
            _lib.load().raae_multi_free(self.prog)
            self.prog = None

    def __del__(self):
        try:
            self.release()
        except Exception:      # noqa: BLE001 -- interpreter shutdown
            pass


def score_arrays_batched(inputs, device=None):
    """Blocks of J models, ``inputs = [(styles, aux, spec_in, spec_out)]`` of one shape, scored by one
    ``gridDim.z = J`` launch sequence.  Raises if the recorder refuses (it cannot for these kernels)."""
    device = device or torch.device("cuda:0")
    dev_in = [_device_inputs(*x, device) for x in inputs]
    masked = has_missing(*[x[1] for x in inputs])
    scorers = [SelectionScorer(z.shape[0], z.shape[1], a.shape[1], si.shape[1], device, masked=masked)
               for z, a, si, _ in dev_in]
    stream = torch.cuda.Stream(device=device)
    stream.wait_stream(torch.cuda.current_stream(device))
    with torch.cuda.stream(stream):
        prog = BatchedProgram.build([(lambda s=s, x=x: s.launch(*x)) for s, x in zip(scorers, dev_in)])
        if prog is None:
            raise _lib.HipCallError("raae_select_scores: the recorder refused a batched form")
        for s in scorers:
            s.out.zero_()                 # what is read below is the batched replay's, not the recording pass's
        prog.launch()
        blocks = [s.read() for s in scorers]
    prog.release()
    return blocks


# ------------------------------------------------------------------------------------------------ models
def _ae_form(encoder):
    from .model import AE_CLS_DICT
    for form, cls in AE_CLS_DICT.items():
        if type(encoder).__name__ == cls["encoder"].__name__:
            return form
    raise TypeError(f"{type(encoder).__name__} is not one of this package's encoders ({list(AE_CLS_DICT)}): "
                    "generate_report evaluates final.pt files written by rankaae_amd's train_sc")


def engine_from_model(model, test_ds, device=None, stream=None):
    """``model``: a ``final.pt`` dict of this package's modules, a ``Trainer`` or a ``StepEngine``.  A dict becomes an
    inference-only ``StepEngine`` on ``device`` (its optimizers exist and never step)."""
    from .engine import StepEngine
    eng = getattr(model, "engine", model)
    if hasattr(eng, "reconstruct"):
        return eng
    if not isinstance(model, dict) or "Encoder" not in model or "Decoder" not in model:
        raise TypeError("evaluate_model needs a final.pt dict (Encoder / Decoder / Style Discriminator), a Trainer or "
                        "a StepEngine")
    from .model import DiscriminatorFC
    device = device or torch.device("cuda:0")
    enc, dec = model["Encoder"], model["Decoder"]
    nstyle = int(dec.nstyle)
    dis = model.get("Style Discriminator")
    if dis is None:
        dis = DiscriminatorFC(nstyle=nstyle)
    aux = getattr(test_ds, "aux", None)
    cfg = dict(_INFERENCE_CFG, ae_form=_ae_form(enc), nstyle=nstyle, n_aux=int(aux.shape[1]) if aux is not None else 0,
               dim_in=int(np.asarray(test_ds.spec).shape[1]))
    return StepEngine(enc.cpu(), dec.cpu(), dis.cpu(), cfg, device, use_graph=False, stream=stream)


class _Job:
    """One model's evaluation: engine, resident inputs, the eval-forward workspaces and the scorer."""

    def __init__(self, eng, test_ds):
        from .engine import StepPlan
        self.eng, dev = eng, eng.device
        self.spec = torch.as_tensor(np.ascontiguousarray(test_ds.spec, dtype=np.float32)).to(dev)
        self.aux = torch.as_tensor(np.ascontiguousarray(test_ds.aux, dtype=np.float64)).to(dev)
        n, L = self.spec.shape
        self.n_aux = self.aux.shape[1]
        key = ("recon", n)
        if key not in eng.plans:
            R = StepPlan()
            R.enc, R.dec = eng.enc.alloc(n), eng.dec.alloc(n)
            eng.plans[key] = R
        self.plan = eng.plans[key]
        # decided once, from the split that is scored: NaN descriptor cells are missing labels
        self.labelled = labelled_counts(test_ds.aux) if has_missing(test_ds.aux) else None
        self.scorer = SelectionScorer(n, eng.nstyle, self.n_aux, L, dev, masked=self.labelled is not None)
        self.z = self.out = None

    def emit(self):
        """Eval forwards (what ``StepEngine.reconstruct`` launches) and the score kernels, on the current stream."""
        ops.tile_hint(self.eng.tile_mult)
        self.z = self.eng.enc.forward(self.plan.enc, self.spec, None, train=False)
        self.out = self.eng.dec.forward(self.plan.dec, self.z, None, train=False)
        self.scorer.launch(self.z, self.aux, self.spec, self.out)

    def result(self):
        res = result_from_block(self.scorer.read(), self.n_aux, self.labelled)
        res["Input"] = self.spec.cpu().numpy()
        res["Output"] = self.out.cpu().numpy()
        return res


def evaluate_model(test_ds, model, device=None):
    """``analysis.evaluate_model`` (analysis.py:394-450): the result dict of one model on ``test_ds`` (anything with
    ``.spec [n, L]`` and ``.aux [n, n_aux]``)."""
    eng = engine_from_model(model, test_ds, device)
    job = _Job(eng, test_ds)
    eng.stream.wait_stream(torch.cuda.current_stream(eng.device))
    with torch.cuda.stream(eng.stream):
        job.emit()
        return job.result()


def list_jobs(jobs_dir):
    """The ``job_*`` directories that hold a ``final.pt``, in sorted name order (see the module docstring)."""
    return sorted(j for j in os.listdir(jobs_dir)
                  if j.startswith("job_") and os.path.exists(os.path.join(jobs_dir, j, "final.pt")))


def load_model(jobs_dir, job, weights="final"):
    """The model dict of ``job``: ``final.pt``, or with ``weights="ema"`` (config key ``report_weights``) the moving
    average ``final_ema.pt`` that a run with ``ema_decay`` writes -- ``FileNotFoundError`` naming the job directory
    where the run wrote none."""
    from .parameter import REPORT_WEIGHTS
    if weights not in REPORT_WEIGHTS:
        raise ValueError(f"report_weights must be 'final' or 'ema', not {weights!r}")
    path = os.path.join(jobs_dir, job, REPORT_WEIGHTS[weights])
    if weights != "final" and not os.path.exists(path):
        raise FileNotFoundError(f"report_weights: {weights}: {os.path.join(jobs_dir, job)} has no "
                                f"{REPORT_WEIGHTS[weights]} (was the run trained with ema_decay?)")
    return torch.load(path, map_location="cpu", weights_only=False)


def evaluate_all_models(jobs_dir, test_ds, device=None, batched=True, info=None, weights="final", names=None):
    """``analysis.evaluate_all_models`` (analysis.py:105-123): ``{job: result dict}`` for every ``job_*`` under
    ``jobs_dir``, in sorted name order.  With ``batched`` and jobs of one architecture, the J eval forwards and the J
    score sequences are replayed as one launch sequence with ``gridDim.z = J``; otherwise (or if the recorder refuses)
    one job after the other.  The numbers are the same either way: a grid plane runs the kernel body a model runs
    alone.  ``info``: a dict that receives ``mode`` ("batched" / "sequential") and ``launches``.  ``weights``: "final"
    (``final.pt``) or "ema" (``final_ema.pt`` of every job, ``load_model``).  ``names``: evaluate these jobs, in this
    order, instead of every job.  An ``info`` that comes in with a key ``"blocks"`` gets ``{job: block}`` there, the
    unrounded ``raae_select_scores`` blocks the results were rounded from (``rankaae_amd.apply.calibration``)."""
    device = device or torch.device("cuda:0")
    names = list_jobs(jobs_dir) if names is None else [str(j) for j in names]
    if not names:
        raise FileNotFoundError(f"no job_*/final.pt under {jobs_dir}")
    stream = torch.cuda.Stream(device=device)
    stream.wait_stream(torch.cuda.current_stream(device))
    models = [load_model(jobs_dir, j, weights) for j in names]       # (before any engine exists: a missing file raises here)
    jobs = [_Job(engine_from_model(m, test_ds, device, stream=stream), test_ds) for m in models]
    info = info if info is not None else {}
    want_blocks = "blocks" in info
    info.update(mode="sequential", launches=0)
    with torch.cuda.stream(stream):
        prog = None
        if batched and 1 < len(jobs) <= 64:
            # (the recorder logs launches while they run: the recording pass evaluates every job once, eagerly)
            prog = BatchedProgram.build([j.emit for j in jobs])
        if prog is None:
            for j in jobs:
                j.emit()
        else:
            for j in jobs:
                j.scorer.out.zero_()
            prog.launch()
            info.update(mode="batched", launches=prog.count())
        result = OrderedDict((name, j.result()) for name, j in zip(names, jobs))
        if want_blocks:
            info["blocks"] = OrderedDict((name, j.scorer.read()) for name, j in zip(names, jobs))
    if prog is not None:
        prog.release()
    for j in jobs:
        j.eng.release()
    return result


# ------------------------------------------------------------------------------------------------ ranking (host)
def sorting_algorithm(x):
    """``generate_report.sorting_algorithm`` (generate_report.py:16-45): columns of ``x`` are the z-scores of
    ``SCORE_NAMES``.  The reconstruction error's weight is 0, so its column becomes ``x ** 0 == 1``, the divisor."""
    weight = [-1, 0, 1, 1, 1, 1, 1]
    off_set = 0
    if np.sum(weight) == weight[1]:
        off_set = 1
    xx = x.copy()
    xx[:, 0] = x[:, 0] * weight[0]
    xx[:, 1] = x[:, 1] ** weight[1]
    for c in range(2, 7):
        xx[:, c] = x[:, c] * weight[c]
    return (off_set + xx[:, 0] + np.sum(xx[:, 2:], axis=1)) / xx[:, 1]


def score_matrix(result_dict):
    """``(jobs, scores [J, 7], z_scores [J, 7], mu_std [7, 2])`` as ``sort_all_models`` forms them (analysis.py:154-181):
    a missing descriptor (or the coordination number's ``None``) scores 0; population z-scores; a column without
    variation becomes 0."""
    jobs, scores = [], []
    for job, result in result_dict.items():
        jobs.append(job)
        score = [result["Inter-style Corr"], result["Reconstruct Err"][0]]
        for i in range(5):
            try:
                a = result["Style-descriptor Corr"][i]
                score.append(a["F1 score"] if i == 1 else a["Spearman"])
            except (KeyError, TypeError):
                score.append(0)
        scores.append(score)
    jobs, scores = np.array(jobs), np.array(scores, dtype=np.float64)
    mu_std = np.stack((scores.mean(axis=0), scores.std(axis=0)), axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        z_scores = (scores - mu_std[:, 0]) / mu_std[:, 1]
    z_scores[:, (mu_std[:, 1] == 0)] = 0
    return jobs, scores, z_scores, mu_std


def sort_all_models(result_dict, sort_score=None, ascending=True, top_n=None, details=None):
    """``analysis.sort_all_models`` (analysis.py:130-231) without the heat map: writes ``Rank`` and ``Score`` into the
    results and returns ``(result_dict, ranked_jobs)``.  Descending order is ``argsort()[::-1]``, so ties come out in
    reversed iteration order.  ``details``: a dict that receives the ranked score, z-score and final-score arrays
    (what the heat map shows)."""
    jobs, scores, z_scores, mu_std = score_matrix(result_dict)
    if callable(sort_score):
        final_score = sort_score(z_scores)
    elif isinstance(sort_score, int) and sort_score >= 0:
        final_score = scores[:, sort_score]
    else:
        final_score = np.arange(len(scores))
    rank = np.argsort(final_score)
    if (sort_score is not None) and (not ascending):
        rank = rank[::-1]
    ranked_jobs, ranked_final = jobs[rank], final_score[rank]
    for i, (job, score) in enumerate(zip(ranked_jobs, ranked_final)):
        result_dict[job]["Rank"] = i
        result_dict[job]["Score"] = round(float(score), 4)
    if details is not None:
        if top_n is None or top_n > len(rank):
            top_n = len(rank)
        details.update(jobs=ranked_jobs[:top_n], scores=scores[rank][:top_n], z_scores=z_scores[rank][:top_n],
                       final_scores=ranked_final[:top_n], mu_std=mu_std, score_names=SCORE_NAMES)
    return result_dict, ranked_jobs


# ------------------------------------------------------------------------------------------------ writers
def save_evaluation_result(save_dir, file_name, model_results, save_spectra=False, top_n=5):
    """``generate_report.save_evaluation_result`` (generate_report.py:179-203): ``<file_name>.json`` with the ``top_n``
    best jobs in rank order, without ``Input`` / ``Output``; with ``save_spectra`` the rank-0 model's spectra as
    ``<file_name>.in`` / ``.out``."""
    save_dict = OrderedDict()
    top_n = min(top_n, len(model_results))
    order = list(range(top_n))
    for job, result in model_results.items():
        if result["Rank"] in order:
            order[result["Rank"]] = job
    spec_in = spec_out = None
    for job in order:
        result = model_results[job]
        save_dict[job] = {k: v for k, v in result.items() if k not in ["Input", "Output"]}
        if result["Rank"] == 0 and save_spectra:
            spec_in, spec_out = result["Input"], result["Output"]
    with open(os.path.join(save_dir, file_name + ".json"), "wt") as f:
        f.write(json.dumps(save_dict))
    if spec_in is not None:
        np.savetxt(os.path.join(save_dir, file_name + ".out"), spec_out)
        np.savetxt(os.path.join(save_dir, file_name + ".in"), spec_in)


def save_model_evaluations(save_dir, file_name, result):
    with open(os.path.join(save_dir, file_name + "_model_evaluation.pkl"), "wb") as f:
        pickle.dump(result, f)


def load_evaluations(evaluation_path="./report_model_evaluations.pkl"):
    with open(evaluation_path, "rb") as f:
        return pickle.load(f)
