"""Dataset ingest with the reference's semantics (``sc/clustering/dataloader.py:8-77``):
CSV with two index columns, ``n_aux`` ``AUX_*`` columns then ``ENE_<eV>`` columns; contiguous
70/15/15 row split; float64 -> float32; an empty AUX cell is NaN, a missing label; training rows reshuffled every epoch; the last,
partial batch is kept.  Unlike the reference the CSV is parsed ONCE and the split arrays go
to the device whole -- batches are gathered there by index (``raae_gather_batch``)."""
import numpy as np
import torch


class AuxSpectraDataset:
    def __init__(self, spec, aux, grid=None, atom_index=None, metadata=None):
        self.spec, self.aux, self.grid = spec, aux, grid
        self.atom_index, self.metadata = atom_index, metadata

    def __len__(self):
        return self.spec.shape[0]

    def __getitem__(self, idx):
        aux = np.array([0.0]) if self.aux is None else self.aux[idx]
        return torch.Tensor(self.spec[idx]), torch.Tensor(aux)


class Loader:
    """Minimal stand-in for ``torch.utils.data.DataLoader``: what ``Trainer`` needs
    (``dataset``, ``batch_size``, ``len``) plus the reference's shuffle order."""

    def __init__(self, dataset, batch_size, shuffle, generator=None):
        self.dataset, self.batch_size, self.shuffle = dataset, batch_size, shuffle
        # None: the GLOBAL torch CPU generator, as the reference's DataLoader (one trial per process); a private
        # generator when several trials share a process (train_sc's thread mode: each trial its own stream)
        self.generator = generator

    def __len__(self):
        return -(-len(self.dataset) // self.batch_size)

    def epoch_permutation(self):
        """Row order of one epoch exactly as ``DataLoader(shuffle=True, num_workers=0)`` draws it
        (SURVEY.md finding 9): iterator ``_base_seed`` draw, sampler seed draw, private randperm."""
        torch.empty((), dtype=torch.int64).random_(generator=self.generator)
        if not self.shuffle:
            return torch.arange(len(self.dataset))
        seed = int(torch.empty((), dtype=torch.int64).random_(generator=self.generator).item())
        g = torch.Generator()
        g.manual_seed(seed)
        return torch.randperm(len(self.dataset), generator=g)

    def __iter__(self):
        perm = self.epoch_permutation()
        for i in range(len(self)):
            rows = perm[i * self.batch_size:(i + 1) * self.batch_size].numpy()
            aux = self.dataset.aux[rows] if self.dataset.aux is not None else np.zeros((len(rows), 1))
            yield torch.tensor(self.dataset.spec[rows], dtype=torch.float32), torch.tensor(aux, dtype=torch.float32)


def split_counts(n_rows, ratios=(0.7, 0.15, 0.15)):
    n = [int(n_rows * r) for r in ratios]
    n[-1] = int(n_rows) - sum(n[:-1])
    return n


def _parse_csv(csv_fn, n_aux):
    import pandas as pd
    df = pd.read_csv(csv_fn, index_col=[0, 1], comment="#")
    cols = df.columns.to_list()
    assert "ENE_" in cols[n_aux]
    if n_aux > 0:
        assert "ENE_" not in cols[n_aux - 1]
        assert "AUX_" in cols[0]
        assert "AUX_" in cols[n_aux - 1]
    grid = np.array([float(c.strip("ENE_")) for c in cols if c.startswith("ENE_")])
    # an empty (or "NaN") AUX cell is a missing label and stays NaN; a spectrum has to be complete
    data = df.to_numpy(dtype=np.float64)
    bad = np.argwhere(~np.isfinite(data[:, n_aux:]))
    if len(bad):
        r, c = bad[0]
        raise ValueError(f"{csv_fn}: spectrum value of row {df.index[r]} (data row {r}), column {cols[n_aux + c]} is "
                         f"empty or not finite ({len(bad)} such cells); only AUX_* cells may be missing")
    return data[:, n_aux:], (data[:, :n_aux] if n_aux > 0 else None), grid, df.index.to_list()


CACHE_SUFFIX = ".raae_cache.npz"


def load_csv(csv_fn, n_aux, cache=True):
    """Parse the reference's CSV schema (``dataloader.py:12-33``).  The reference parses the file three times
    per trial (once per split) and again in every trial of a run; here the parsed float64 arrays are kept next
    to the CSV as ``<csv>.raae_cache.npz``, keyed on the CSV's size, mtime and ``n_aux``, and a
    later trial maps them instead of parsing.  The cache is best effort: an unwritable directory, a stale or
    unreadable cache all fall back to parsing (the values are identical either way, tests/test_host_cpu.py)."""
    import json
    import os
    if not cache:
        return _parse_csv(csv_fn, n_aux)
    st = os.stat(csv_fn)
    key = [int(st.st_size), int(st.st_mtime_ns), int(n_aux)]
    cache_fn = str(csv_fn) + CACHE_SUFFIX
    try:
        with np.load(cache_fn, allow_pickle=False) as z:
            if z["key"].tolist() == key:
                index = [tuple(t) for t in json.loads(str(z["index"]))]
                return z["spec"], (z["aux"] if n_aux > 0 else None), z["grid"], index
    except (OSError, KeyError, ValueError):
        pass
    spec, aux, grid, index = _parse_csv(csv_fn, n_aux)
    try:
        tmp = f"{cache_fn}.{os.getpid()}.tmp.npz"
        np.savez(tmp, key=np.array(key, dtype=np.int64), spec=np.ascontiguousarray(spec),
                 aux=np.ascontiguousarray(aux) if aux is not None else np.zeros((0, 0)), grid=grid,
                 index=np.array(json.dumps([list(t) for t in index])))
        os.replace(tmp, cache_fn)
    except (OSError, TypeError):
        pass
    return spec, aux, grid, index


def get_dataloaders(csv_fn, batch_size, train_val_test_ratios=(0.7, 0.15, 0.15), n_aux=0, arrays=None, generator=None):
    """``arrays=(spec, aux)`` bypasses the CSV (synthetic data already in memory); ``generator``: see ``Loader``."""
    if arrays is None:
        spec, aux, grid, index = load_csv(csv_fn, n_aux)
    else:
        spec, aux = arrays
        grid, index = None, list(range(len(spec)))
    n = split_counts(len(spec), train_val_test_ratios)
    loaders, lo = [], 0
    meta = {"path": csv_fn, "train_test_val_split_ratio": train_val_test_ratios}
    for i, cnt in enumerate(n):
        ds = AuxSpectraDataset(spec[lo:lo + cnt], None if aux is None else aux[lo:lo + cnt], grid,
                               index[lo:lo + cnt], meta)
        loaders.append(Loader(ds, batch_size, shuffle=(i == 0), generator=generator))
        lo += cnt
    return loaders
