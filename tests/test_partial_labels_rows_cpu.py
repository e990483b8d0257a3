"""The float64 reference of the masked rank loss split over ranks (``partial_label_rows_reference``), without a GPU:
the totals of the ranks' row ranges, summed, and ``finish`` reproduce the whole-batch definition
(``partial_label_reference.masked_rank_loss``) for every case and split the GPU test runs the kernels on, and the
oracle's ``kendall_constraint`` on fully labelled input."""
import numpy as np
import pytest
import torch

from partial_label_reference import masked_rank_loss
from partial_label_rows_reference import SPLITS, finish, masked_rank_rows, rank_case

CASES = [(name, split) for name, splits in SPLITS.items() for split in splits]


def _ranks(d, z, split, act):
    """``(summed totals, loss per rank, stacked gradient)`` of the emulated ranks."""
    row0s = np.concatenate([[0], np.cumsum(split)[:-1]])
    parts = [masked_rank_rows(d, z, r0, n, act) for r0, n in zip(row0s, split)]
    total = parts[0].copy()
    for p in parts[1:]:
        total += p
    outs = [finish(total, d, z, r0, n, act) for r0, n in zip(row0s, split)]
    return total, parts, [o[0] for o in outs], np.concatenate([o[1] for o in outs])


@pytest.mark.parametrize("act", [False, True])
@pytest.mark.parametrize("name,split", CASES)
def test_summed_totals_and_finish_are_the_whole_batch_definition(name, split, act):
    d, z, K = rank_case(name)
    assert sum(split) == len(d)
    total, parts, losses, grad = _ranks(d, z[:, :K], split, act)
    lref, gref = masked_rank_loss(d, z[:, :K], act)
    assert len(set(losses)) == 1, "every rank forms the same loss from the same totals"
    assert abs(losses[0] - lref) <= 1e-13 * abs(lref), (losses[0], lref)
    assert np.allclose(grad, gref, rtol=1e-12, atol=0)
    assert np.all(grad[~np.isfinite(d)] == 0.0) and not np.isnan(grad).any()
    # the counts are those of the whole batch: labelled rows per descriptor, and no more pairs than they can form
    m = np.isfinite(d).sum(axis=0)
    assert np.array_equal(total[4], m) and np.all(total[0] + total[1] <= m * m - m)
    whole = masked_rank_rows(d, z[:, :K], 0, len(d), act)
    assert np.array_equal(total[[0, 1, 4]], whole[[0, 1, 4]]) and np.allclose(total[2:4], whole[2:4], rtol=1e-12, atol=0)
    if name == "b7":
        assert m.tolist() == [5, 3, 0, 1, 6]
        if split == (3, 2, 2):
            assert parts[0][4, 1] == 0 and np.all(parts[0][:4, 1] == 0), "rank 0 owns no labelled row of column 1"


@pytest.mark.parametrize("act", [False, True])
@pytest.mark.parametrize("name,split", [("b7", (3, 2, 2)), ("tile", (128, 129))])
def test_on_fully_labelled_input_it_is_the_oracles_rank_loss(name, split, act):
    from oracle.ref_train import kendall_constraint
    d, z, K = rank_case(name, labelled=True)
    assert np.isfinite(d).all()
    _, _, losses, grad = _ranks(d, z[:, :K], split, act)
    zt = torch.tensor(z[:, :K], dtype=torch.float64, requires_grad=True)
    lit = kendall_constraint(torch.tensor(d, dtype=torch.float64), zt, activate=act)
    lit.backward()
    assert abs(losses[0] - lit.item()) <= 1e-13 * abs(lit.item())
    assert np.allclose(grad, zt.grad.numpy(), rtol=1e-12, atol=1e-15)
