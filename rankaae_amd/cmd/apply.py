#!/usr/bin/env python
"""``python -m rankaae_amd.cmd.apply -c <config.yaml> [-w <work_dir>] -i <spectra.csv>`` -- the best trials of a
``train_sc`` run applied to spectra from elsewhere: per spectrum the styles, the descriptors the styles stand for and
how far the trials agree (``rankaae_amd.apply``).

Config keys: those of ``generate_report`` (``data_file``, ``n_aux``, ``output_name``, ``top_n``, ``gpu``,
``report_weights``, optional ``plot_job``: apply that one job, no ranking) and three of its own, all optional:
``apply_top_n`` (default ``top_n``), ``apply_max_outside`` (default 0) and ``apply_chunk_rows`` (default 16384), see
``rankaae_amd.parameter.apply_keys_of``.  The model's energy grid is the training CSV's header; the trials are ranked
as ``generate_report`` ranks them and the best ``apply_top_n`` are applied.

The input CSV: any leading columns that are not ``ENE_*`` are carried through as they are (``AUX_*`` cells included,
empty or not); the ``ENE_<eV>`` columns behind them are the spectrum on its own grid.  Files, in ``work_dir``:

* ``<output_name>_apply.csv``  the carried columns, then ``STYLE_<i>_mean``, ``STYLE_<i>_std`` per style,
  ``PRED_<i>_mean``, ``PRED_<i>_std`` per descriptor, then ``MAE_mean``
* ``<output_name>_apply.npz``  everything ``apply_models`` returns
"""
import argparse
import csv
import os

import numpy as np
import torch

from rankaae_amd import apply, report
from rankaae_amd.cmd.generate_report import validation_split
from rankaae_amd.parameter import Parameters, apply_keys_of, report_weights_of


def read_input(csv_fn):
    """``(header of the carried columns, their cells [n][c] as text, grid [Ls], spec [n, Ls] float64)``.  An empty or
    unreadable spectrum cell becomes NaN, which ``apply.resample`` refuses by row and column."""
    with open(csv_fn, newline="") as f:
        rows = [r for r in csv.reader(f) if r and not r[0].startswith("#")]
    if len(rows) < 2:
        raise ValueError(f"{csv_fn}: a header and at least one row are needed")
    header = [c.strip() for c in rows[0]]
    first = next((i for i, c in enumerate(header) if c.startswith("ENE_")), None)
    if first is None or not all(c.startswith("ENE_") for c in header[first:]):
        raise ValueError(f"{csv_fn}: the ENE_<eV> columns must be the last columns of the file")
    grid = np.array([float(c[len("ENE_"):]) for c in header[first:]])
    carried, spec = [], np.full((len(rows) - 1, len(grid)), np.nan)
    for r, row in enumerate(rows[1:]):
        if len(row) != len(header):
            raise ValueError(f"{csv_fn}: data row {r} has {len(row)} cells, the header {len(header)}")
        carried.append(row[:first])
        for c, cell in enumerate(row[first:]):
            try:
                spec[r, c] = float(cell)
            except ValueError:
                pass
    return header[:first], carried, grid, spec


def write_csv(path, carried_header, carried, out):
    k, n_aux = out["z_mean"].shape[1], out["d_mean"].shape[1]
    header = list(carried_header)
    for i in range(k):
        header += [f"STYLE_{i}_mean", f"STYLE_{i}_std"]
    for i in range(n_aux):
        header += [f"PRED_{i}_mean", f"PRED_{i}_std"]
    header.append("MAE_mean")
    with open(path, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(header)
        for r, cells in enumerate(carried):
            row = list(cells)
            for i in range(k):
                row += [repr(float(out["z_mean"][r, i])), repr(float(out["z_std"][r, i]))]
            for i in range(n_aux):
                row += [repr(float(out["d_mean"][r, i])), repr(float(out["d_std"][r, i]))]
            row.append(repr(float(out["mae_mean"][r])))
            w.writerow(row)


def main(argv=None):
    parser = argparse.ArgumentParser()
    parser.add_argument("-w", "--work_dir", type=str, default=".", help="The folder where the model and data are.")
    parser.add_argument("-c", "--config", type=str, required=True, help="Config for training parameter in YAML format")
    parser.add_argument("-i", "--input", type=str, required=True, help="CSV of the spectra to apply the models to")
    args = parser.parse_args(argv)
    work_dir = os.path.abspath(os.path.expanduser(args.work_dir))
    config = Parameters.from_yaml(os.path.join(work_dir, args.config))
    weights = report_weights_of(config)     # before anything touches the GPU
    top_n, max_outside, chunk_rows = apply_keys_of(config)
    jobs_dir = os.path.join(work_dir, "training")
    if not torch.cuda.is_available():
        raise RuntimeError("rankaae_amd.cmd.apply runs the models on the HIP engine: it needs an MI355X")
    gpu = config.get("gpu", 0)
    device = torch.device(f"cuda:{0 if isinstance(gpu, bool) else int(gpu)}")
    torch.cuda.set_device(device)

    file_name = config.get("data_file", None)
    if file_name is None:
        csvs = [f for f in os.listdir(work_dir) if f.endswith(".csv")]
        assert len(csvs) == 1, "Which data file are you going to use?"
        file_name = csvs[0]
    val_ds = validation_split(os.path.join(work_dir, file_name), config.n_aux)
    input_fn = args.input if os.path.isabs(args.input) else os.path.join(work_dir, args.input)
    carried_header, carried, grid, spec = read_input(input_fn)

    plot_job = config.get("plot_job", None)
    if plot_job is not None:
        jobs = [str(plot_job)]
    else:
        results = report.evaluate_all_models(jobs_dir, val_ds, device=device, weights=weights)
        _, ranked = report.sort_all_models(results, sort_score=report.sorting_algorithm, ascending=False)
        jobs = [str(j) for j in ranked[:top_n]]
    out = apply.apply_models(jobs_dir, jobs, val_ds, spec, grid, val_ds.grid, device=device, weights=weights,
                             chunk_rows=chunk_rows, max_outside=max_outside)
    name = config.output_name
    write_csv(os.path.join(work_dir, name + "_apply.csv"), carried_header, carried, out)
    np.savez(os.path.join(work_dir, name + "_apply.npz"), **out)
    print(f"Success: {len(carried)} spectra, jobs {', '.join(jobs)}: {name}_apply.csv and {name}_apply.npz saved!")


if __name__ == "__main__":
    main()
