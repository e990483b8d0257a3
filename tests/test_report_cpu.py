"""Host side of the report step (``rankaae_amd.report``): the ranking of ``sort_all_models`` + ``sorting_algorithm`` and
the JSON writer, fed the per-job result dicts the REAL reference returned (``tests/golden/selection_ref.json``,
``tools/gen_selection_golden.py``).  No GPU."""
import copy
import json
import os

import numpy as np
import pytest

from rankaae_amd import report

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "selection_ref.json")


def _cases():
    with open(GOLDEN) as f:
        return {c["name"]: c for c in json.load(f)["cases"]}


def _results(case):
    """The fixture's dicts as ``evaluate_model`` returns them: integer descriptor keys, no Rank / Score yet."""
    out = {}
    for job in case["job_order"]:
        r = copy.deepcopy(case["jobs"][job])
        r["Style-descriptor Corr"] = {int(i): v for i, v in r["Style-descriptor Corr"].items()}
        r.pop("Rank"), r.pop("Score")
        r["Input"], r["Output"] = np.zeros((2, 3)), np.ones((2, 3))
        out[job] = r
    return out


@pytest.mark.parametrize("name", ["main", "small"])
def test_ranking_reproduces_the_reference(name):
    case = _cases()[name]
    res = _results(case)
    jobs, scores, z, mu_std = report.score_matrix(res)
    assert list(jobs) == case["job_order"]
    np.testing.assert_allclose(z, np.array(case["z_scores"]), rtol=0, atol=1e-12)
    np.testing.assert_allclose(report.sorting_algorithm(z), np.array(case["final_scores"]), rtol=0, atol=1e-12)
    res, ranked = report.sort_all_models(res, sort_score=report.sorting_algorithm, ascending=False, top_n=case["top_n"])
    assert [str(j) for j in ranked] == case["ranked_jobs"]
    for job in case["job_order"]:
        assert res[job]["Rank"] == case["jobs"][job]["Rank"], job
        assert res[job]["Score"] == case["jobs"][job]["Score"], job


def test_zero_variance_and_missing_descriptor_columns():
    case = _cases()["small"]          # n_aux = 3: descriptors 3 and 4 are missing; job_3's coordination number is None
    res = _results(case)
    assert res["job_3"]["Style-descriptor Corr"][1] is None
    jobs, scores, z, mu_std = report.score_matrix(res)
    assert np.all(scores[:, 5:] == 0) and np.all(mu_std[5:, 1] == 0)
    assert np.all(z[:, 5:] == 0) and np.all(np.isfinite(z))
    assert scores[list(jobs).index("job_3"), 3] == 0
    # every job with the same value in a column: that column's z-score is 0, not NaN
    for r in res.values():
        r["Inter-style Corr"] = 0.25
    assert np.all(report.score_matrix(res)[2][:, 0] == 0)


def test_descending_order_reverses_ties():
    case = _cases()["small"]
    res = _results(case)
    for r in res.values():
        for k, v in res["job_1"].items():
            if k not in ("Input", "Output"):
                r[k] = copy.deepcopy(v)
    _, ranked = report.sort_all_models(res, sort_score=report.sorting_algorithm, ascending=False)
    assert list(ranked) == np.array(case["job_order"])[np.argsort(np.zeros(len(res)))[::-1]].tolist()


@pytest.mark.parametrize("top_n", [3, 5, 100])
def test_json_writer_keys_order_and_top_n(tmp_path, top_n):
    case = _cases()["main"]
    res, ranked = report.sort_all_models(_results(case), sort_score=report.sorting_algorithm, ascending=False)
    report.save_evaluation_result(str(tmp_path), "report", res, save_spectra=True, top_n=top_n)
    with open(tmp_path / "report.json") as f:
        saved = json.load(f)
    keep = min(top_n, len(res))
    assert list(saved) == case["ranked_jobs"][:keep]
    for i, (job, r) in enumerate(saved.items()):
        assert set(r) == {"Style-descriptor Corr", "Reconstruct Err", "Inter-style Corr", "Rank", "Score"}
        assert r["Rank"] == i and set(r["Style-descriptor Corr"]) == {"0", "1", "2", "3", "4"}
        assert set(r["Style-descriptor Corr"]["1"]) == {"F1 score", "CN45 Threshold", "CN56 Threshold"}
        assert set(r["Style-descriptor Corr"]["0"]) == {"Spearman", "Linear", "Quadratic"}
    assert np.loadtxt(tmp_path / "report.in").shape == (2, 3) and np.all(np.loadtxt(tmp_path / "report.out") == 1)
    details = {}
    report.sort_all_models(_results(case), sort_score=report.sorting_algorithm, ascending=False, top_n=top_n, details=details)
    assert details["z_scores"].shape == (keep, 7) and list(details["jobs"]) == case["ranked_jobs"][:keep]


def test_result_from_block_layout():
    """The block -> dict conversion: keys, nesting, rounding and the None path."""
    from rankaae_amd._lib import SEL_HEAD, SEL_STRIDE
    b = np.zeros(SEL_HEAD + 3 * SEL_STRIDE)
    b[:3] = [0.012345, 0.00455, 0.33336]
    b[SEL_HEAD:SEL_HEAD + 9] = [0.91234, 1.5, -0.25, 0.81, 0.1, 0.2, 0.3, 0.04321, 0.88888]
    b[SEL_HEAD + 2 * SEL_STRIDE:SEL_HEAD + 2 * SEL_STRIDE + 9] = b[SEL_HEAD:SEL_HEAD + 9]
    r = report.result_from_block(b, 3)
    assert r["Style-descriptor Corr"][1] is None and r["Reconstruct Err"] == [0.0123, 0.0046 if round(0.00455, 4) == 0.0046 else 0.0045]
    assert r["Style-descriptor Corr"][0] == {"Spearman": 0.9123, "Linear": {"slope": 1.5, "intercept": -0.25, "R2": 0.81},
                                             "Quadratic": {"Parameters": [0.1, 0.2, 0.3], "residue": [0.0432], "R2": 0.8889}}
    o = SEL_HEAD + SEL_STRIDE
    b[o:o + 6] = [1.0, 0.97291, 304, 421, report.THRESH_GRID[304], report.THRESH_GRID[421]]
    cn = report.result_from_block(b, 3)["Style-descriptor Corr"][1]
    assert cn == {"F1 score": 0.9729, "CN45 Threshold": round(float(report.THRESH_GRID[304]), 4),
                  "CN56 Threshold": round(float(report.THRESH_GRID[421]), 4)}
