"""The report step on the GPU: ``raae_select_scores`` (``rankaae_amd/csrc/raae_select.hip``) against what the REAL
reference's ``analysis.evaluate_model`` returned for the same arrays (``tests/golden/selection_ref.json``; the inputs
are regenerated from the stored seed and checked by SHA-256), and ``train_sc`` followed by ``generate_report`` end to
end.

Tolerances: the fixture holds the reference's 4-decimal roundings, and the generator asserted that no unrounded value
lies within 1e-7 of a rounding boundary and that neighbouring final scores differ by >= 1e-3.  Values are therefore
compared within one unit of the fourth decimal (1e-4, the reference's own rounding step), the two thresholds and the
rank order exactly."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "selection_ref.json")
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEP = 1e-4 + 1e-9        # one unit of the fourth decimal (+ the representation error of the decimals compared)


def _case(name):
    from rankaae_amd.synthetic import selection_inputs
    with open(GOLDEN) as f:
        case = {c["name"]: c for c in json.load(f)["cases"]}[name]
    inputs = selection_inputs(case["seed"], case["n_jobs"], case["n_rows"], case["nstyle"], case["n_aux"],
                              case["n_points"], case["four_class_job"])
    for j, arrays in enumerate(inputs):
        want = case["sha256"][f"job_{j + 1}"]
        for key, a in zip(("styles", "aux", "spec_in", "spec_out"), arrays):
            got = hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()
            assert got == want[key], (f"regenerated input {key} of job_{j + 1} (case {name}) differs from the one the "
                                      f"fixture was made from: {got} != {want[key]} -- numpy's generator changed?")
    return case, inputs


def _compare(got, want, path=""):
    """Every leaf of the reference's dict: same keys and nesting; None where it is None; thresholds exactly; numbers
    within one unit of the fourth decimal."""
    if isinstance(want, dict):
        assert isinstance(got, dict) and set(map(str, got)) == set(want), (path, got, want)
        for k, v in want.items():
            _compare(got[k] if k in got else got[int(k)], v, f"{path}/{k}")
    elif isinstance(want, list):
        assert isinstance(got, list) and len(got) == len(want), (path, got, want)
        for i, (g, w) in enumerate(zip(got, want)):
            _compare(g, w, f"{path}[{i}]")
    elif want is None:
        assert got is None, (path, got)
    elif path.endswith("Threshold"):
        assert got == want, (path, got, want)
    else:
        assert isinstance(got, float) and abs(got - want) <= STEP, (path, got, want, abs(got - want))


def _check_blocks(case, blocks):
    from rankaae_amd import report
    results = {}
    for j, block in enumerate(blocks):
        job = f"job_{j + 1}"
        res = report.result_from_block(block, case["n_aux"])
        want = {k: v for k, v in case["jobs"][job].items() if k not in ("Rank", "Score")}
        _compare({k: v for k, v in res.items() if k not in ("Input", "Output")}, want, job)
        results[job] = res
    results, ranked = report.sort_all_models(results, sort_score=report.sorting_algorithm, ascending=False)
    assert [str(j) for j in ranked] == case["ranked_jobs"]
    for job in results:
        assert results[job]["Rank"] == case["jobs"][job]["Rank"]


@pytest.mark.parametrize("name", ["main", "small"])
def test_scores_match_the_reference_single_and_batched(name):
    from rankaae_amd import report
    case, inputs = _case(name)
    single = [report.score_arrays(*x) for x in inputs]
    _check_blocks(case, single)
    batched = report.score_arrays_batched(inputs)
    _check_blocks(case, batched)
    for j, (a, b) in enumerate(zip(single, batched)):
        assert a.tobytes() == b.tobytes(), f"job_{j + 1}: the grid plane of the batched form differs from the model alone"


def test_four_class_coordination_number_is_none():
    from rankaae_amd import report
    case, inputs = _case("small")
    j = case["four_class_job"]
    res = report.result_from_block(report.score_arrays(*inputs[j]), case["n_aux"])
    assert res["Style-descriptor Corr"][1] is None and case["jobs"][f"job_{j + 1}"]["Style-descriptor Corr"]["1"] is None
    assert res["Style-descriptor Corr"][0]["Spearman"] is not None
    assert report.score_matrix({"a": res})[1][0, 3] == 0


def test_replayed_capture_is_bitwise_the_eager_run():
    from rankaae_amd import ops, report
    case, inputs = _case("main")
    dev = torch.device("cuda:0")
    z, a, si, so = report._device_inputs(*inputs[0], dev)
    sc = report.SelectionScorer(z.shape[0], z.shape[1], a.shape[1], si.shape[1], dev)
    stream = torch.cuda.Stream(device=dev)
    stream.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(stream):
        sc.launch(z, a, si, so)
        eager = sc.read()
        g = ops.Graph()
        g.begin()
        sc.launch(z, a, si, so)
        g.end()
        for _ in range(2):
            sc.out.zero_()
            g.launch()
            assert sc.read().tobytes() == eager.tobytes()
    assert np.all(np.isfinite(eager))


def _run(args, cwd, timeout):
    env = dict(os.environ, PYTHONPATH=REPO)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, "-m"] + args, env=env, cwd=cwd, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, (args, r.stdout[-1000:], r.stderr[-3000:])
    return r


@pytest.mark.parametrize("fixture", ["ref_fc_small.json", "ref_compact_small.json"])
def test_train_then_generate_report(fixture, tmp_path):
    """``train_sc`` with ``trials: 3`` then ``generate_report`` in the same directory."""
    import yaml
    from scipy.stats import spearmanr
    from rankaae_amd import report
    from rankaae_amd.cmd.generate_report import validation_split
    from rankaae_amd.export import Reconstruct
    from rankaae_amd.synthetic import make_spectra, write_csv
    with open(os.path.join(os.path.dirname(__file__), "golden", fixture)) as f:
        g = json.load(f)
    cfg = dict(g["config"])
    cfg.update(max_epoch=3, trials=3, trial_seed=11, data_file="data.csv", verbose=False, timeout=1,
               output_name="report", top_n=2, n_sampling=20)
    spec, aux, grid = make_spectra(g["n_rows"], g["n_points"], cfg["n_aux"], seed=g["data_seed"])
    write_csv(str(tmp_path / "data.csv"), spec, aux, grid)
    with open(tmp_path / "cfg.yaml", "w") as f:
        yaml.safe_dump(cfg, f)
    _run(["rankaae_amd.cmd.train_sc", "-c", "cfg.yaml", "-w", str(tmp_path)], str(tmp_path), 500)
    r = _run(["rankaae_amd.cmd.generate_report", "-c", "cfg.yaml", "-w", str(tmp_path)], str(tmp_path), 300)
    assert "Success" in r.stdout
    for name in ("report.json", "report.in", "report.out", "report_model_evaluation.pkl", "report_spec_in.txt",
                 "report_spec_out.txt", "report_styles.txt"):
        assert (tmp_path / name).exists(), name

    results = report.load_evaluations(str(tmp_path / "report_model_evaluation.pkl"))
    assert list(results) == ["job_1", "job_2", "job_3"]
    _, ranked = report.sort_all_models({j: dict(r) for j, r in results.items()}, sort_score=report.sorting_algorithm,
                                       ascending=False)
    with open(tmp_path / "report.json") as f:
        saved = json.load(f)
    best = str(ranked[0])
    assert list(saved) == [str(j) for j in ranked[:2]] and saved[best]["Rank"] == 0

    # the latent-space export is Reconstruct on the rank-0 job's final.pt
    test_ds = validation_split(str(tmp_path / "data.csv"), cfg["n_aux"])
    eng = report.engine_from_model(report.load_model(str(tmp_path / "training"), best), test_ds)
    want = Reconstruct(name="again").evaluate(test_ds, eng)
    styles = np.loadtxt(tmp_path / "report_styles.txt")
    assert np.array_equal(styles, want["styles"].astype(np.float64))
    eng.release()

    # the saved spectra and styles re-scored with scipy / numpy on the host
    spec_in, spec_out = np.loadtxt(tmp_path / "report.in"), np.loadtxt(tmp_path / "report.out")
    mae = np.abs(spec_out - spec_in).mean(axis=1)
    res = saved[best]
    assert abs(res["Reconstruct Err"][0] - mae.mean()) <= STEP and abs(res["Reconstruct Err"][1] - mae.std()) <= STEP
    d = np.asarray(test_ds.aux)
    for i in range(cfg["n_aux"]):
        if i != 1:
            rho = spearmanr(d[:, i], styles[:, i]).correlation
            assert abs(res["Style-descriptor Corr"][str(i)]["Spearman"] - rho) <= STEP, (i, rho)
    inter = max(abs(spearmanr(styles[:, i], styles[:, -1]).correlation) for i in range(styles.shape[1] - 1))
    assert abs(res["Inter-style Corr"] - inter) <= STEP
