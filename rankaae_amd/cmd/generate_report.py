#!/usr/bin/env python
"""``sc_generate_report -c <config.yaml> [-w <work_dir>]`` -- the reference's report step
(``sc/report/generate_report.py:218-293``) after a ``train_sc`` run: every ``training/job_*/final.pt`` is evaluated
on the validation split on the GPU, the trials are ranked and the best one is written out.

Config keys: ``data_file`` (searched in ``work_dir`` if absent), ``n_aux``, ``output_name``, ``top_n``, ``n_sampling``,
optional ``plot_job`` (skip the ranking, report that job), ``gpu`` (device index, default 0; the evaluation has no
CPU path) and ``report_weights`` (``final``, the default, or ``ema``: evaluate every ``training/job_*/final_ema.pt``, the
moving average of the weights that a run with ``ema_decay`` writes, instead of ``final.pt``; a job directory without
one is a ``FileNotFoundError``, any other value a ``ValueError``).  Files, all in ``work_dir``:

* ``<output_name>_model_evaluation.pkl``  every job's result dict (with ``Input`` / ``Output``), ``Rank`` and ``Score``
* ``<output_name>.json``                  the ``top_n`` best jobs in rank order, without the spectra
* ``<output_name>.in`` / ``.out``         ``np.savetxt`` of the best model's input and reconstructed spectra
* ``<output_name>_spec_in.txt`` / ``_spec_out.txt`` / ``_styles.txt``   ``rankaae_amd.export.Reconstruct`` of the best model
* ``<output_name>_variation.npz``         the per-style spectra sweeps behind the report's variation plots
* with matplotlib only: ``<output_name>_model_selection.png``, ``<output_name>_best_model.png`` (or
  ``<output_name>_<plot_job>.png``), ``loss_curves.png``

Unlike the reference the jobs are visited in sorted name order (``rankaae_amd.report``), and seaborn, monty and plotly
are not used: the heat map and the report figure are plain matplotlib.
"""
import argparse
import os

import numpy as np
import torch

from rankaae_amd import report
from rankaae_amd.dataloader import AuxSpectraDataset, load_csv, split_counts
from rankaae_amd.export import Reconstruct, spectra_variation
from rankaae_amd.parameter import Parameters, report_weights_of


def validation_split(csv_fn, n_aux):
    """``AuxSpectraDataset(csv, split_portion="val", n_aux=n_aux)`` of the reference: the rows ``get_dataloaders`` gives
    the validation loader."""
    spec, aux, grid, index = load_csv(csv_fn, n_aux)
    n_train, n_val, _ = split_counts(len(spec))
    rows = slice(n_train, n_train + n_val)
    return AuxSpectraDataset(spec[rows], None if aux is None else aux[rows], grid, index[rows], {"path": csv_fn})


def _pyplot():
    try:
        import matplotlib
        matplotlib.use("Agg")
        from matplotlib import pyplot as plt
        return plt
    except ImportError:
        return None


def plot_model_selection(plt, details, path):
    """The heat map of ``sort_all_models`` (analysis.py:207-229) with ``imshow`` in place of seaborn's."""
    z, scores = details["z_scores"].T, details["scores"].T
    fig, ax = plt.subplots(figsize=(max(4, z.shape[1]), z.shape[0]))
    im = ax.imshow(z, vmin=-3, vmax=3, cmap="Blues", aspect="auto")
    fig.colorbar(im, ax=ax)
    for (r, c), v in np.ndenumerate(scores):
        ax.text(c, r, f"{v:.2g}", ha="center", va="center")
    ax.set_yticks(range(z.shape[0]))
    ax.set_yticklabels([f"{name}\n{ms[0]:.3f}+-{ms[1]:.3f}" for name, ms in zip(details["score_names"], details["mu_std"])])
    ax.set_xticks(range(z.shape[1]))
    ax.set_xticklabels([f"{j}: {s:.2f}" for j, s in zip(details["jobs"], details["final_scores"])], rotation=45,
                       ha="left", va="bottom")
    ax.tick_params(labelbottom=False, labeltop=True, length=0)
    fig.savefig(path, bbox_inches="tight")
    plt.close(fig)


def plot_best_model(plt, title, result, variations, grid, styles, aux, path):
    """Style-variation sweeps on top, style against descriptor below -- the content of ``plot_report``
    (generate_report.py:48-176), not its layout."""
    k, n_aux = len(variations), aux.shape[1]
    fig, axs = plt.subplots(2, max(k, n_aux), figsize=(4 * max(k, n_aux), 8), squeeze=False)
    fig.suptitle(f"{title}\nLeast correlation: {result['Inter-style Corr']:.4f}")
    for i, (variation, spec) in enumerate(variations):
        for row in spec:
            axs[0, i].plot(grid if grid is not None and len(grid) == len(row) else np.arange(len(row)), row, lw=0.6)
        axs[0, i].set_title(f"Style {i + 1} varying from {variation[0]:.2f} to {variation[-1]:.2f}")
    for i in range(n_aux):
        axs[1, i].scatter(aux[:, i], styles[:, i], s=4.0, alpha=0.6)
        acc = result["Style-descriptor Corr"].get(i)
        if acc:
            axs[1, i].set_title(f"F1 {acc['F1 score']:.2f}" if i == 1 else f"{acc['Linear']['R2']:.2f}/{acc['Spearman']:.2f}")
    fig.savefig(path, bbox_inches="tight")
    plt.close(fig)


def plot_loss_curves(plt, losses_csv, path):
    try:
        data = np.genfromtxt(losses_csv, delimiter=",", names=True)
    except (OSError, ValueError):
        return
    if data.dtype.names is None or data.size == 0:
        return
    fig, ax = plt.subplots(figsize=(8, 5))
    for name in data.dtype.names[1:]:
        ax.plot(np.atleast_1d(data[name]), label=name)
    ax.set_xlabel("epoch")
    ax.legend(fontsize=6, ncol=2)
    fig.savefig(path, bbox_inches="tight")
    plt.close(fig)


def main(argv=None):
    parser = argparse.ArgumentParser()
    parser.add_argument("-w", "--work_dir", type=str, default=".", help="The folder where the model and data are.")
    parser.add_argument("-c", "--config", type=str, required=True, help="Config for training parameter in YAML format")
    args = parser.parse_args(argv)
    work_dir = os.path.abspath(os.path.expanduser(args.work_dir))
    config = Parameters.from_yaml(os.path.join(work_dir, args.config))
    weights = report_weights_of(config)     # before anything touches the GPU
    jobs_dir = os.path.join(work_dir, "training")
    if not torch.cuda.is_available():
        raise RuntimeError("sc_generate_report evaluates the models on the HIP engine: it needs an MI355X")
    gpu = config.get("gpu", 0)
    device = torch.device(f"cuda:{0 if isinstance(gpu, bool) else int(gpu)}")
    torch.cuda.set_device(device)

    file_name = config.get("data_file", None)
    if file_name is None:
        csvs = [f for f in os.listdir(work_dir) if f.endswith(".csv")]
        assert len(csvs) == 1, "Which data file are you going to use?"
        file_name = csvs[0]
    test_ds = validation_split(os.path.join(work_dir, file_name), config.n_aux)
    name, plt = config.output_name, _pyplot()

    plot_job = config.get("plot_job", None)
    if plot_job is not None:
        best = str(plot_job)
        png = os.path.join(work_dir, f"{name}_{best}.png")
    else:
        results = report.evaluate_all_models(jobs_dir, test_ds, device=device, weights=weights)
        details = {}
        results, ranked = report.sort_all_models(results, sort_score=report.sorting_algorithm, ascending=False,
                                                 top_n=config.top_n, details=details)
        report.save_model_evaluations(work_dir, name, results)
        if plt is not None:
            plot_model_selection(plt, details, os.path.join(work_dir, name + "_model_selection.png"))
        report.save_evaluation_result(work_dir, name, results, save_spectra=True, top_n=config.top_n)
        best = str(ranked[0])
        png = os.path.join(work_dir, f"{name}_best_model.png")

    # the best model: its own result, the latent-space export and the per-style sweeps, on one engine
    eng = report.engine_from_model(report.load_model(jobs_dir, best, weights), test_ds, device)
    result = report.evaluate_model(test_ds, eng)
    recon = Reconstruct(device=device, name=name)
    styles = recon.evaluate(test_ds, eng, path_to_save=work_dir)["styles"]
    variations = [spectra_variation(eng, i, styles, n_spec=50, n_sampling=config.get("n_sampling", 1000))
                  for i in range(eng.nstyle)]
    np.savez(os.path.join(work_dir, name + "_variation.npz"), variation=np.stack([v for v, _ in variations]),
             spectra=np.stack([s for _, s in variations]))
    eng.release()
    if plt is not None:
        plot_best_model(plt, "-".join([name, best]), result, variations, test_ds.grid, styles, np.asarray(test_ds.aux), png)
        plot_loss_curves(plt, os.path.join(jobs_dir, best, "losses.csv"), os.path.join(work_dir, "loss_curves.png"))
    print("Success: training report saved!")


if __name__ == "__main__":
    main()
