"""The masked rows-against-all pair (``raae_rank_rows_masked_pairs`` / ``raae_rank_rows_masked_finish``) on one GPU, the
ranks of a data-parallel run emulated: ``_pairs`` once per rank, the totals summed on the device in rank order, ``_finish``
per rank with ``scale = W``.  Held against the float64 definition on the whole batch (``partial_label_reference``, and
``partial_label_rows_reference``, which ``test_partial_labels_rows_cpu.py`` pins to it) to the tolerances of
``tests/test_partial_labels_gpu.py``: loss 1e-5 relative + 1e-7, gradient 1e-5 relative + 1e-9.

Cases: 7 rows (m = 5, 3, 0, 1, 6; in 3+2+2 a rank owns no labelled row of a column), 257 rows (NaNs on both sides of the
256-row tile; a rank of one row), 1100 rows (several column blocks; 1050 rows on a rank: four rows per thread)."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from partial_label_reference import masked_rank_loss
from partial_label_rows_reference import SPLITS, rank_case

if torch.cuda.is_available():
    from rankaae_amd import _lib, ops
    DEV = torch.device("cuda:0")

CASES = [(name, split) for name, splits in SPLITS.items() for split in splits]
RAAE_EINVAL = -1            # include/rankaae_hip.h


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)


def _row0s(split):
    return [int(v) for v in np.concatenate([[0], np.cumsum(split)[:-1]])]


class _Ranks:
    """The emulated ranks' buffers; ``masked=False``: the unmasked pair (64 totals) on the same rows."""

    def __init__(self, d, z, K, split, masked=True):
        self.K, self.split, self.masked = K, split, masked
        self.n_all, self.ld = z.shape
        self.d, self.z = _dev(d), _dev(z)
        nbytes = ops.rank_rows_masked_work_bytes if masked else ops.rank_loss_work_bytes
        self.work = [torch.empty(nbytes(n, K), dtype=torch.uint8, device=DEV) for n in split]
        self.totals = [torch.full((80 if masked else 64,), 5.0, dtype=torch.float64, device=DEV) for _ in split]
        self.total = torch.zeros_like(self.totals[0])
        self.loss = [torch.full((1,), 9.0, device=DEV) for _ in split]
        self.dz = [torch.full((n, self.ld), 7.0, device=DEV) for n in split]

    def run(self, act, grad=True):
        pairs, fin = ((ops.rank_rows_masked_pairs, ops.rank_rows_masked_finish) if self.masked else
                      (ops.rank_rows_pairs, ops.rank_rows_finish))
        for r, (row0, n) in enumerate(zip(_row0s(self.split), self.split)):
            pairs(self.d, self.K, self.z, self.ld, self.n_all, row0, n, self.K, self.work[r], self.totals[r])
        self.total.copy_(self.totals[0])
        for t in self.totals[1:]:                                   # the all-reduce: summed in rank order
            self.total += t
        for r, n in enumerate(self.split):
            fin(self.total, self.n_all, n, self.K, act, float(len(self.split)), self.work[r], self.loss[r],
                self.dz[r] if grad else None, self.ld)
        torch.cuda.synchronize()
        return self

    def loss_bits(self):
        return [t.cpu().numpy().tobytes() for t in self.loss]

    def stacked_dz(self):
        return torch.cat(self.dz).cpu().double().numpy()

    def state(self):
        return [t.cpu().numpy().tobytes() for t in self.totals + [self.total] + self.loss + self.dz]


def _close(got, want, what):
    err, tol = np.abs(got - want), 1e-9 + 1e-5 * np.abs(want)
    print(f"{what}: max |err| {err.max():.3e}, max err / tol {np.max(err / tol):.3f}")
    assert np.all(err <= tol), what


def _loss_close(got, want, what):
    print(f"{what}: loss {got!r} reference {want!r}, |err| / tol {abs(got - want) / (1e-5 * abs(want) + 1e-7):.3f}")
    assert abs(got - want) <= 1e-5 * abs(want) + 1e-7, (what, got, want)


_REFS = {}


def _reference(name, act):
    """The float64 loss and gradient of a case on the whole batch, computed once."""
    if (name, act) not in _REFS:
        d, z, K = rank_case(name)
        _REFS[name, act] = masked_rank_loss(d, z[:, :K], act)
    return _REFS[name, act]


@pytest.mark.parametrize("act", [False, True])
@pytest.mark.parametrize("name,split", CASES)
def test_emulated_ranks_form_the_float64_loss_of_the_whole_batch(name, split, act):
    d, z, K = rank_case(name)
    W = len(split)
    lref, gref = _reference(name, act)
    ranks = _Ranks(d, z, K, split).run(act)
    bits = ranks.loss_bits()
    assert all(b == bits[0] for b in bits), "the ranks' losses differ"
    loss = float(ranks.loss[0])
    _loss_close(loss, lref, f"{name} {split} activate={act}")
    # the summed counts are the whole batch's, exactly
    total = ranks.total.cpu().numpy().reshape(5, 16)
    assert np.array_equal(total[4, :K], np.isfinite(d).sum(axis=0)) and np.all(total[:, K:] == 0.0)
    dz = ranks.stacked_dz()
    assert not np.isnan(dz).any() and not np.isnan(loss)
    assert np.all(dz[:, :K][~np.isfinite(d)] == 0.0), "a row without a label has a gradient"
    assert np.all(dz[:, K:] == 0.0)
    _close(dz[:, :K] / W, gref, f"{name} {split} dz / W")
    state = ranks.state()
    # the same buffers again: the same bytes
    assert ranks.run(act).state() == state
    # validation form
    for t in ranks.loss:
        t.fill_(9.0)
    assert ranks.run(act, grad=False).loss_bits() == bits


@pytest.mark.parametrize("act", [False, True])
@pytest.mark.parametrize("name", list(SPLITS))
def test_one_rank_is_the_single_gpu_masked_kernel(name, act):
    d, z, K = rank_case(name)
    B, ld = z.shape
    ranks = _Ranks(d, z, K, (B,)).run(act)
    work = torch.empty(ops.rank_loss_masked_work_bytes(B, K), dtype=torch.uint8, device=DEV)
    loss = torch.full((1,), 9.0, device=DEV)
    dz = torch.full((B, ld), 7.0, device=DEV)
    ops.rank_loss_masked_fwd_bwd(ranks.d, K, ranks.z, ld, B, K, act, work, loss, dz)
    torch.cuda.synchronize()
    print(f"{name} activate={act}: loss bitwise {torch.equal(loss, ranks.loss[0])}, dz bitwise {torch.equal(dz, ranks.dz[0])}")
    # one finalize kernel forms both from the same reduction, coefficients and dz loop, and the counts pass through the
    # totals exactly: the same bits
    assert torch.equal(loss, ranks.loss[0]) and torch.equal(dz, ranks.dz[0])
    _loss_close(float(ranks.loss[0]), float(loss), f"{name} W=1 against rank_loss_masked_fwd_bwd")
    _close(ranks.stacked_dz(), dz.cpu().double().numpy(), f"{name} W=1 dz")


@pytest.mark.parametrize("act", [False, True])
@pytest.mark.parametrize("name,split", CASES)
def test_on_fully_labelled_input_it_is_the_unmasked_pair(name, split, act):
    d, z, K = rank_case(name, labelled=True)
    got = _Ranks(d, z, K, split).run(act)
    want = _Ranks(d, z, K, split, masked=False).run(act)
    print(f"{name} {split} activate={act}: totals bitwise {torch.equal(got.total[:64], want.total)}, "
          f"loss bitwise {got.loss_bits() == want.loss_bits()}, dz bitwise {got.state()[-len(split):] == want.state()[-len(split):]}")
    assert got.total[64:64 + K].tolist() == [float(len(d))] * K
    _loss_close(float(got.loss[0]), float(want.loss[0]), f"{name} {split} against rank_rows_finish")
    _close(got.stacked_dz(), want.stacked_dz(), f"{name} {split} dz")


def test_invalid_arguments_are_refused_without_a_launch():
    lib = _lib.load()
    d, z, K = rank_case("b7")
    ranks = _Ranks(d, z, K, (4, 3))
    p = lambda t: C.c_void_p(t.data_ptr())
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    tot, work, loss, dz = ranks.totals[0], ranks.work[0], ranks.loss[0], ranks.dz[0]
    # rows [4, 8) of 7; 17 descriptors
    assert lib.raae_rank_rows_masked_pairs(p(ranks.d), K, p(ranks.z), K + 1, 7, 4, 4, K, p(work), p(tot), st) == RAAE_EINVAL
    assert lib.raae_rank_rows_masked_pairs(p(ranks.d), 17, p(ranks.z), 17, 7, 0, 4, 17, p(work), p(tot), st) == RAAE_EINVAL
    assert lib.raae_rank_rows_masked_finish(p(tot), 7, 4, 17, 0, 1.0, p(work), p(loss), p(dz), 17, st) == RAAE_EINVAL
    assert lib.raae_rank_rows_masked_finish(p(tot), 7, 8, K, 0, 1.0, p(work), p(loss), p(dz), K + 1, st) == RAAE_EINVAL
    with pytest.raises(_lib.HipCallError):
        ops.rank_rows_masked_pairs(ranks.d, K, ranks.z, K + 1, 7, 4, 4, K, work, tot)
    torch.cuda.synchronize()
    assert torch.all(tot == 5.0) and float(loss) == 9.0 and torch.all(dz == 7.0), "a refused call wrote something"
