"""Trained trials applied to spectra they were not trained on: styles, the descriptors the styles stand for and how
far the trials agree, per spectrum.

Three steps, the per-row work on the device:

* the input rows, on their own energy grid, are resampled onto the model's (``resample_plan`` on the host, once per
  pair of grids; ``raae_resample_rows`` per row);
* the J chosen trials' eval forwards run over the rows as one ``gridDim.z = J`` sequence -- ``report.BatchedProgram``
  and the structure of ``report._Job``, the machinery that ranks the trials;
* ``raae_ensemble_stats`` combines the J answers per row: mean and sample standard deviation over the trials of every
  style and of every descriptor, the reconstruction error per trial and its mean.

A style becomes a descriptor through the fit ``raae_select_scores`` forms on the validation split (``calibration``):
``linregress`` with ``x = descriptor, y = style`` inverted, or the two coordination-number thresholds.  There is no
CPU path.
"""
import numpy as np
import torch

from . import ops, report
from ._lib import SEL_HEAD, SEL_STRIDE

KIND_NONE, KIND_LINEAR, KIND_CLASSES = 0.0, 1.0, 2.0


# ------------------------------------------------------------------------------------------------ the energy grid
def _grid(grid, name, least):
    g = np.asarray(grid, dtype=np.float64).reshape(-1)
    if len(g) < least:
        raise ValueError(f"{name}: {len(g)} points, at least {least} are needed")
    if not np.all(np.isfinite(g)):
        raise ValueError(f"{name}: not finite at index {int(np.argmax(~np.isfinite(g)))}")
    if np.any(np.diff(g) <= 0.0):
        i = int(np.argmax(np.diff(g) <= 0.0))
        raise ValueError(f"{name}: not strictly increasing at index {i + 1} ({g[i]!r} then {g[i + 1]!r})")
    return g


def resample_plan(src_grid, dst_grid):
    """``(idx int32 [L], w float32 [L], outside bool [L])`` with ``dst_grid[l]`` at ``src_grid[idx] + w * (src_grid[idx
    + 1] - src_grid[idx])``, in float64: ``0 <= idx <= Ls - 2`` and ``0 <= w <= 1``.  A point that coincides with a
    source point gets ``w = 0`` on it (the last source point: ``w = 1`` on its left neighbour), so the kernel returns
    the source value bit for bit; a point outside the source range is flagged and takes the edge value.  Both grids
    finite and strictly increasing, the source at least two points: anything else is a ``ValueError``."""
    src, dst = _grid(src_grid, "src_grid", 2), _grid(dst_grid, "dst_grid", 1)
    Ls = len(src)
    outside = (dst < src[0]) | (dst > src[-1])
    j = np.searchsorted(src, dst, side="right") - 1            # src[j] <= dst < src[j + 1]
    idx = np.clip(j, 0, Ls - 2)
    w = (dst - src[idx]) / (src[idx + 1] - src[idx])           # (dst == src[-1]: idx = Ls - 2 and w = 1 exactly)
    w = np.clip(w, 0.0, 1.0)                                   # outside points: the edge value
    return idx.astype(np.int32), w.astype(np.float32), outside


def _check_outside(outside, dst_grid, max_outside):
    n_out = int(outside.sum())
    if n_out > max_outside:
        bad = np.asarray(dst_grid, dtype=np.float64)[outside]
        raise ValueError(f"{n_out} points of the model's energy grid lie outside the input's range (first {bad[0]!r}, "
                         f"last {bad[-1]!r}); at most {max_outside} may (apply_max_outside)")


def _resample(spec, plan, device):
    idx, w, _ = plan
    spec = np.asarray(spec)
    if spec.ndim != 2:
        raise ValueError(f"spectra must be [n, Ls], not {spec.shape}")
    bad = np.argwhere(~np.isfinite(spec))
    if len(bad):
        r, c = bad[0]
        raise ValueError(f"spectrum value of data row {r}, column {c} is empty or not finite ({len(bad)} such cells)")
    src = torch.as_tensor(np.ascontiguousarray(spec, dtype=np.float32)).to(device)
    out = torch.empty(src.shape[0], len(idx), dtype=torch.float32, device=device)
    if src.shape[0]:
        ops.resample_rows(src, torch.as_tensor(idx).to(device), torch.as_tensor(w).to(device), out)
    return out


def resample(spec, src_grid, dst_grid, device=None, max_outside=0):
    """Host rows ``spec [n, Ls]`` on ``src_grid`` as a ``[n, L]`` fp32 device tensor on ``dst_grid``
    (``raae_resample_rows``: linear interpolation in fp32, source values bit for bit where the grids coincide).
    ``ValueError`` where more than ``max_outside`` points of ``dst_grid`` lie outside the source range, or a cell is
    not finite."""
    device = device or torch.device("cuda:0")
    plan = resample_plan(src_grid, dst_grid)
    if np.asarray(spec).ndim == 2 and np.asarray(spec).shape[1] != len(np.asarray(src_grid).reshape(-1)):
        raise ValueError(f"spectra have {np.asarray(spec).shape[1]} columns, src_grid {len(np.asarray(src_grid).reshape(-1))} points")
    _check_outside(plan[2], dst_grid, max_outside)
    return _resample(spec, plan, device)


# ------------------------------------------------------------------------------------------------ the calibration
def calibration(block, n_aux, labelled=None):
    """``[n_aux][4]`` float64 rows ``{kind, p0, p1, 0}`` from one model's UNROUNDED ``raae_select_scores`` block: kind 1
    with ``p0 = slope``, ``p1 = intercept`` of the descriptor's ``linregress`` (``d = (z - p1) / p0``), kind 2 with the
    CN45 and CN56 thresholds for descriptor 1 (``d = 4 + (z > p0) + (z > p1)``), kind 0 wherever
    ``report.result_from_block`` gives ``None`` (fewer than 3 labelled rows, the coordination number's ``valid == 0``)
    and where the slope is 0 or not finite: a style that does not move with the descriptor says nothing about it."""
    block = np.asarray(block, dtype=np.float64)
    calib = np.zeros((n_aux, 4), dtype=np.float64)
    for i in range(n_aux):
        o = block[SEL_HEAD + SEL_STRIDE * i:SEL_HEAD + SEL_STRIDE * (i + 1)]
        if labelled is not None and labelled[i] < 3:
            continue
        if i == 1:
            if o[0] != 0.0:
                calib[i] = [KIND_CLASSES, o[4], o[5], 0.0]
        elif np.isfinite(o[1]) and o[1] != 0.0 and np.isfinite(o[2]):
            calib[i] = [KIND_LINEAR, o[1], o[2], 0.0]
    return calib


# ------------------------------------------------------------------------------------------------ the models
class _Forward:
    """One model's eval forwards over a fixed buffer of ``rows`` input rows: ``report._Job`` without the scorer."""

    def __init__(self, eng, xbuf):
        from .engine import StepPlan
        self.eng, self.x = eng, xbuf
        key = ("recon", xbuf.shape[0])
        if key not in eng.plans:
            R = StepPlan()
            R.enc, R.dec = eng.enc.alloc(xbuf.shape[0]), eng.dec.alloc(xbuf.shape[0])
            eng.plans[key] = R
        self.plan = eng.plans[key]
        self.z = self.out = None

    def emit(self):
        ops.tile_hint(self.eng.tile_mult)
        self.z = self.eng.enc.forward(self.plan.enc, self.x, None, train=False)
        self.out = self.eng.dec.forward(self.plan.dec, self.z, None, train=False)


class _Pass:
    """The J models' forwards over ``rows`` rows and the statistics behind them: one ``gridDim.z = J`` sequence where
    the recorder takes it, else one model after the other."""

    def __init__(self, engines, rows, L, device):
        self.rows = rows
        self.x = torch.zeros(rows, L, dtype=torch.float32, device=device)
        self.fwd = [_Forward(e, self.x) for e in engines]
        self.prog = None
        if 1 < len(engines) <= 64:
            # (the recorder logs launches while they run: the recording pass runs every model once, on zeros)
            self.prog = report.BatchedProgram.build([f.emit for f in self.fwd])
        if self.prog is None:
            for f in self.fwd:
                f.emit()
        for f in self.fwd:
            assert f.z.is_contiguous() and f.out.is_contiguous()
        self.z_tab = ops.pointer_table([f.z for f in self.fwd])
        self.r_tab = ops.pointer_table([f.out for f in self.fwd])

    def run(self, x):
        self.x.copy_(x)
        if self.prog is not None:
            self.prog.launch()
        else:
            for f in self.fwd:
                f.emit()

    def release(self):
        if self.prog is not None:
            self.prog.release()


def apply_models(jobs_dir, jobs, val_ds, spec, src_grid, model_grid, device=None, weights="final", chunk_rows=16384,
                 max_outside=0, keep_recon=False, info=None):
    """The trials ``jobs`` (names of ``job_*`` directories under ``jobs_dir``) applied to the host rows ``spec [n, Ls]``
    on ``src_grid``.  ``val_ds``: the validation split the calibration is fitted on (``.spec`` on ``model_grid``,
    ``.aux``).  Returns host arrays: ``styles [J, n, k]`` and ``mae [J, n]`` per trial; ``z_mean``, ``z_std [n, k]``;
    ``d_mean``, ``d_std [n, n_aux]`` and ``d_used [n_aux]`` (how many trials have a fit for the descriptor; 0: NaN);
    ``mae_mean [n]``; ``spec [n, L]`` the resampled input; ``outside [L]``; ``jobs``; ``calib [J, n_aux, 4]``.
    ``keep_recon`` adds ``recon [J, n, L]``, the reconstructions behind ``mae``.  The rows are worked on in chunks of
    at most ``chunk_rows``; a row's numbers do not depend on the chunking.  ``info``: a dict that receives ``mode``
    ("batched": the forwards ran as one ``gridDim.z = J`` sequence; "sequential") and ``launches`` per batched pass."""
    device = device or torch.device("cuda:0")
    jobs = [str(j) for j in jobs]
    J = len(jobs)
    if not 1 <= J <= 64:
        raise ValueError(f"apply_models takes 1 to 64 jobs, not {J}")
    if int(chunk_rows) < 1:
        raise ValueError(f"chunk_rows must be >= 1, not {chunk_rows!r}")
    model_grid = np.asarray(model_grid, dtype=np.float64).reshape(-1)
    L = int(np.asarray(val_ds.spec).shape[1])
    if len(model_grid) != L:
        raise ValueError(f"model_grid has {len(model_grid)} points, the validation spectra {L}")
    # 1. the input on the model's grid
    plan = resample_plan(src_grid, model_grid)
    if np.asarray(spec).ndim == 2 and np.asarray(spec).shape[1] != len(np.asarray(src_grid).reshape(-1)):
        raise ValueError(f"spectra have {np.asarray(spec).shape[1]} columns, src_grid {len(np.asarray(src_grid).reshape(-1))} points")
    _check_outside(plan[2], model_grid, max_outside)
    x = _resample(spec, plan, device)
    n = x.shape[0]
    if n < 1:
        raise ValueError("no input rows")
    # 2. the calibration: the validation split scored by the named jobs
    scored = {"blocks": None}
    report.evaluate_all_models(jobs_dir, val_ds, device=device, info=scored, weights=weights, names=jobs)
    aux = getattr(val_ds, "aux", None)
    n_aux = int(aux.shape[1]) if aux is not None else 0
    labelled = report.labelled_counts(aux) if n_aux and report.has_missing(aux) else None
    calib = np.stack([calibration(scored["blocks"][j], n_aux, labelled) for j in jobs]).reshape(J, n_aux, 4)
    # 3. and 4. the forwards and the statistics, chunk by chunk
    stream = torch.cuda.Stream(device=device)
    stream.wait_stream(torch.cuda.current_stream(device))
    models = [report.load_model(jobs_dir, j, weights) for j in jobs]
    engines = [report.engine_from_model(m, val_ds, device, stream=stream) for m in models]
    k = int(engines[0].nstyle)
    if any(int(e.nstyle) != k for e in engines):
        raise ValueError("the jobs differ in nstyle")
    f64 = lambda *shape: torch.zeros(*shape, dtype=torch.float64, device=device)      # noqa: E731
    z_mean, z_std, mae, mae_mean = f64(n, k), f64(n, k), f64(J, n), f64(n)
    d_mean, d_std, d_used = f64(n, n_aux), f64(n, n_aux), f64(n_aux)
    calib_dev = torch.as_tensor(calib).to(device)
    styles = np.empty((J, n, k), dtype=np.float32)
    recon = np.empty((J, n, L), dtype=np.float32) if keep_recon else None
    chunk = min(int(chunk_rows), n)
    passes = {}
    with torch.cuda.stream(stream):
        for r0 in range(0, n, chunk):
            c = min(chunk, n - r0)
            if c not in passes:
                passes[c] = _Pass(engines, c, L, device)
            P = passes[c]
            P.run(x[r0:r0 + c])
            ops.ensemble_stats(P.z_tab, P.x, P.r_tab, calib_dev, J, c, k, n_aux, L, z_mean[r0:r0 + c], z_std[r0:r0 + c],
                               d_mean[r0:r0 + c], d_std[r0:r0 + c], d_used, mae[:, r0:], n, mae_mean[r0:r0 + c])
            for j, f in enumerate(P.fwd):
                styles[j, r0:r0 + c] = f.z.cpu().numpy()
                if keep_recon:
                    recon[j, r0:r0 + c] = f.out.cpu().numpy()
        host = lambda t: t.cpu().numpy()      # noqa: E731
        result = dict(styles=styles, mae=host(mae), z_mean=host(z_mean), z_std=host(z_std), d_mean=host(d_mean),
                      d_std=host(d_std), d_used=host(d_used), mae_mean=host(mae_mean), spec=host(x), outside=plan[2],
                      jobs=np.array(jobs), calib=calib)
    if info is not None:
        progs = [P.prog for P in passes.values()]
        info.update(mode="batched" if all(p is not None for p in progs) else "sequential",
                    launches=progs[0].count() if progs[0] is not None else 0)
    for P in passes.values():
        P.release()
    for e in engines:
        e.release()
    if keep_recon:
        result["recon"] = recon
    return result
