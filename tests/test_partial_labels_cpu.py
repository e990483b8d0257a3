"""Missing descriptors (NaN AUX cells) without a GPU: the CSV ingest and its cache, and the float64 restatement of the
masked rank loss (``partial_label_reference``) that the GPU tests compare the kernels with -- pinned here to the oracle's
rank loss on fully labelled batches and to itself on compacted batches."""
import numpy as np
import pytest
import torch

from partial_label_reference import compact, masked_rank_loss
from rankaae_amd.synthetic import make_spectra, write_csv


def _csv_with_gaps(path):
    """40 rows, 3 descriptors, 16 points; AUX cells of a few rows written as the empty string and as ``NaN``."""
    spec, aux, grid = make_spectra(40, 16, 3, seed=7)
    write_csv(path, spec, aux, grid)
    lines = open(path).read().split("\n")
    want = aux.copy()
    for row, col, text in ((0, 0, ""), (3, 2, "NaN"), (3, 1, ""), (17, 0, "nan"), (39, 2, "")):
        cells = lines[1 + row].split(",")
        cells[2 + col] = text
        lines[1 + row] = ",".join(cells)
        want[row, col] = np.nan
    with open(path, "w") as f:
        f.write("\n".join(lines))
    return spec, want


def test_empty_and_nan_aux_cells_parse_to_nan_and_the_cache_round_trips_them(tmp_path):
    from rankaae_amd import dataloader as dl
    csv = str(tmp_path / "d.csv")
    spec, want = _csv_with_gaps(csv)
    first = dl.load_csv(csv, 3)
    calls, orig = [], dl._parse_csv
    dl._parse_csv = lambda *k: (calls.append(1), orig(*k))[1]
    try:
        second = dl.load_csv(csv, 3)
    finally:
        dl._parse_csv = orig
    assert not calls, "the second load must come from the cache"
    for got_spec, got_aux, *_ in (first, second):
        assert got_aux.dtype == np.float64 and got_spec.dtype == np.float64
        assert np.array_equal(np.isnan(got_aux), np.isnan(want)) and np.isnan(got_aux).sum() == 5
        # (the CSV parser's decimal conversion may be an ulp off the written value)
        assert np.allclose(got_aux, want, rtol=1e-14, atol=0, equal_nan=True)
        assert np.allclose(got_spec, spec, rtol=1e-14, atol=0)
    assert np.array_equal(first[0], second[0]) and np.array_equal(first[1], second[1], equal_nan=True)
    # the splits carry them through
    train, val, test = dl.get_dataloaders(csv, 8, n_aux=3)
    assert np.isnan(train.dataset.aux).sum() == 4
    assert np.isnan(np.concatenate([val.dataset.aux, test.dataset.aux])).sum() == 1


def test_an_incomplete_spectrum_is_refused_with_row_and_column(tmp_path):
    from rankaae_amd import dataloader as dl
    csv = str(tmp_path / "d.csv")
    spec, aux, grid = make_spectra(12, 8, 2, seed=1)
    write_csv(csv, spec, aux, grid)
    lines = open(csv).read().split("\n")
    cells = lines[1 + 5].split(",")
    cells[2 + 2 + 3] = ""                     # row 5, fourth energy point
    lines[1 + 5] = ",".join(cells)
    with open(csv, "w") as f:
        f.write("\n".join(lines))
    with pytest.raises(ValueError) as err:
        dl.load_csv(csv, 2, cache=False)
    assert "mp-5" in str(err.value) and "data row 5" in str(err.value) and f"ENE_{grid[3]:.1f}" in str(err.value)


def _batch(B, K, seed, ties=True):
    g = np.random.default_rng(seed)
    d = g.standard_normal((B, K)).astype(np.float32)
    if ties:
        d[:, min(1, K - 1)] = g.integers(4, 7, size=B)
    return d, g.standard_normal((B, K)).astype(np.float32)


@pytest.mark.parametrize("B,K,act", [(36, 5, True), (36, 5, False), (7, 1, True), (50, 12, True)])
def test_helper_on_a_fully_labelled_batch_is_the_oracles_rank_loss(B, K, act):
    """Literal form (float64 inputs, so that only the restatement is compared) and the closed form with its gradient."""
    from oracle.ref_train import kendall_closed_form, kendall_constraint
    d, z = _batch(B, K, B + K)
    loss, grad = masked_rank_loss(d, z, act)
    zt = torch.tensor(z, dtype=torch.float64, requires_grad=True)
    lit = kendall_constraint(torch.tensor(d, dtype=torch.float64), zt, activate=act)
    lit.backward()
    lit = lit.detach()
    assert abs(loss - lit.item()) <= 1e-13 * max(1.0, abs(lit.item()))
    assert np.allclose(grad, zt.grad.numpy(), rtol=1e-12, atol=1e-15)
    l64, g64 = kendall_closed_form(torch.tensor(d), torch.tensor(z), activate=act)
    assert abs(loss - float(l64)) <= 1e-13 * max(1.0, abs(float(l64)))
    assert np.allclose(grad, g64.numpy(), rtol=1e-12, atol=1e-15)


@pytest.mark.parametrize("act", [False, True])
def test_helper_on_a_masked_batch_is_the_helper_on_the_compacted_batch(act):
    d, z = _batch(23, 1, 5)
    d[[0, 4, 5, 11, 22], 0] = np.nan
    loss, grad = masked_rank_loss(d, z, act)
    rows, dc, zc = compact(d, z)
    loss_c, grad_c = masked_rank_loss(dc, zc, act)
    assert len(rows) == 18 and loss == loss_c
    assert np.array_equal(grad[rows], grad_c)
    assert np.all(grad[np.isnan(d[:, 0])] == 0.0) and not np.isnan(grad).any()
    # and against the oracle on those rows
    from oracle.ref_train import kendall_closed_form
    l64, g64 = kendall_closed_form(torch.tensor(dc), torch.tensor(zc), activate=act)
    assert abs(loss - float(l64)) <= 1e-13 and np.allclose(grad[rows], g64.numpy(), rtol=1e-12, atol=1e-15)


def test_helper_columns_without_pairs_contribute_nothing():
    d, z = _batch(7, 3, 2, ties=False)
    d[:, 0] = np.nan                  # m = 0
    d[1:, 1] = np.nan                 # m = 1
    loss, grad = masked_rank_loss(d, z, True)
    l2, g2 = masked_rank_loss(d[:, 2:], z[:, 2:], True)
    assert loss == pytest.approx(l2 / 3, rel=1e-15) and np.allclose(grad[:, 2], g2[:, 0] / 3, rtol=1e-15)
    assert np.all(grad[:, :2] == 0.0)


def test_report_helpers_count_labels_and_mark_thin_descriptors():
    from rankaae_amd import report
    aux = np.ones((6, 3))
    assert not report.has_missing(aux, None)
    aux[:4, 2] = np.nan
    assert report.has_missing(None, aux) and report.labelled_counts(aux).tolist() == [6, 6, 2]
    block = np.zeros(report.SEL_HEAD + report.SEL_STRIDE * 3)
    block[report.SEL_HEAD + report.SEL_STRIDE] = 1.0          # coordination number: valid, thresholds at index 0
    block[report.SEL_HEAD + report.SEL_STRIDE + 4:report.SEL_HEAD + report.SEL_STRIDE + 6] = report.THRESH_GRID[0]
    res = report.result_from_block(block, 3, report.labelled_counts(aux))
    assert res["Style-descriptor Corr"][2] is None and res["Style-descriptor Corr"][0] is not None
    assert report.score_matrix({"a": res})[1][0, 4] == 0
