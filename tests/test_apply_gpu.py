"""``rankaae_amd.apply`` on the GPU: ``raae_resample_rows`` against ``np.interp``, ``raae_ensemble_stats`` against the
numpy reference (``tests/apply_reference.py``), ``apply_models`` end to end on freshly constructed models (nothing is
trained) and the command in a child process.

Tolerances, none of them tuned:

* resampling: one rounding of ``w`` to fp32, one of ``b - a``, one of the ``fmaf`` give ``|error| <= 5 2^-24 max(|a|,
  |b|)``; the tests allow ``2^-21 max|row|``, a factor 1.6 over that.  Coinciding and outside points are bitwise.
* means and ``mae``: double sums of at most 256 fp32 values, order-of-summation error below ``256 2^-53``: ``rtol =
  1e-12``.
* standard deviations: two-pass in double on inputs whose spread over the models is at least 1e-3 of the mean's magnitude
  (``tests/test_apply_cpu.py`` checks that of the inputs): below ``J 2^-53 1e3 ~ 1e-11`` relative, ``rtol = 1e-10``.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import apply_reference as ar

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"


# ------------------------------------------------------------------------------------------------ resampling
def _resample_dev(rows32, idx, w, ld_src=None, ld_out=None):
    from rankaae_amd import ops
    n, Ls = rows32.shape
    L = len(idx)
    src = torch.full((n, ld_src or Ls), float("nan"), dtype=torch.float32, device=DEV)
    src[:, :Ls] = torch.as_tensor(rows32)
    out = torch.full((n, ld_out or L), -7.0, dtype=torch.float32, device=DEV)
    ops.resample_rows(src[:, :Ls], torch.as_tensor(idx).to(DEV), torch.as_tensor(w).to(DEV), out[:, :L])
    torch.cuda.synchronize()
    if ld_out:
        assert torch.all(out[:, L:] == -7.0), "the kernel wrote into the padding of out"
    return out[:, :L].cpu().numpy()


def _check_resample(n, Ls, L, seed, **ld):
    from rankaae_amd import apply
    rng = np.random.default_rng(seed)
    src = np.sort(rng.uniform(100.0, 200.0, Ls))
    dst = np.sort(rng.uniform(src[0], src[-1], L))
    rows = rng.standard_normal((n, Ls)).astype(np.float32)
    idx, w, outside = apply.resample_plan(src, dst)
    assert not outside.any()
    got = _resample_dev(rows, idx, w, **ld)
    want = np.stack([np.interp(dst, src, r.astype(np.float64)) for r in rows])
    err = np.abs(got.astype(np.float64) - want).max(axis=1)
    bound = 2.0 ** -21 * np.abs(rows).max(axis=1)
    print(f"resample n={n} Ls={Ls} L={L}: max error / bound = {np.max(err / bound):.3f}")
    assert np.all(err <= bound), (n, Ls, L, err, bound)


@pytest.mark.parametrize("Ls", [2, 7, 257, 1000])
def test_resample_against_np_interp(Ls):
    for L in (1, 64, 256, 300):
        _check_resample(3, Ls, L, seed=Ls * 1000 + L)


def test_resample_many_rows_and_padded_leading_dimensions():
    _check_resample(130, 257, 300, seed=5)          # 33 row groups of four, the last one half full
    _check_resample(3, 257, 300, seed=6, ld_src=264, ld_out=320)


def test_resample_bitwise_cases():
    from rankaae_amd import apply
    rng = np.random.default_rng(11)
    Ls = 301
    src = np.cumsum(rng.uniform(0.1, 1.0, Ls)) + 7000.0
    rows = rng.standard_normal((5, Ls)).astype(np.float32)
    rows[0, 3], rows[1, 4], rows[2, -1] = np.inf, -0.0, np.float32(1e-45)      # an infinite neighbour, a signed zero, a denormal

    def run(dst):
        idx, w, outside = apply.resample_plan(src, dst)
        return torch.as_tensor(_resample_dev(rows, idx, w)), outside

    got, outside = run(src)                                                      # the identity grid
    assert not outside.any() and torch.equal(got.view(torch.int32), torch.as_tensor(rows).view(torch.int32))
    got, _ = run(src[::2])                                                       # every second point; ends on the last
    assert torch.equal(got.view(torch.int32), torch.as_tensor(rows[:, ::2].copy()).view(torch.int32))
    got, _ = run(src[290:])                                                      # a grid that ends on the last source point
    assert torch.equal(got.view(torch.int32), torch.as_tensor(rows[:, 290:].copy()).view(torch.int32))
    dst = np.concatenate([[src[0] - 5.0, src[0] - 1e-9], src[10:12], [src[-1] + 1e-9, src[-1] + 5.0]])
    got, outside = run(dst)                                                      # outside points: the edge value
    assert outside.tolist() == [True, True, False, False, True, True]
    want = np.stack([rows[:, 0], rows[:, 0], rows[:, 10], rows[:, 11], rows[:, -1], rows[:, -1]], axis=1)
    assert torch.equal(got.view(torch.int32), torch.as_tensor(want).view(torch.int32))


# ------------------------------------------------------------------------------------------------ statistics
def _stats_dev(z, spec, recon, calib):
    from rankaae_amd import ops
    J, n, k = z.shape
    n_aux, L = calib.shape[1], spec.shape[1]
    zs = [torch.as_tensor(np.ascontiguousarray(z[j])).to(DEV) for j in range(J)]
    rs = [torch.as_tensor(np.ascontiguousarray(recon[j])).to(DEV) for j in range(J)]
    f64 = lambda *s: torch.full(s, -7.0, dtype=torch.float64, device=DEV)      # noqa: E731
    out = dict(z_mean=f64(n, k), z_std=f64(n, k), d_mean=f64(n, n_aux), d_std=f64(n, n_aux), d_used=f64(n_aux),
               mae=f64(J, n), mae_mean=f64(n))
    ops.ensemble_stats(ops.pointer_table(zs), torch.as_tensor(spec).to(DEV), ops.pointer_table(rs),
                       torch.as_tensor(calib).to(DEV), J, n, k, n_aux, L, out["z_mean"], out["z_std"], out["d_mean"],
                       out["d_std"], out["d_used"], out["mae"], n, out["mae_mean"])
    torch.cuda.synchronize()
    return {key: v.cpu().numpy() for key, v in out.items()}


def _check_stats(got, want):
    for key in ("z_mean", "mae", "mae_mean", "d_mean"):
        assert got[key].shape == want[key].shape, key
        assert np.allclose(got[key], want[key], rtol=1e-12, atol=0.0, equal_nan=True), key
    for key in ("z_std", "d_std"):
        assert got[key].shape == want[key].shape, key
        assert np.allclose(got[key], want[key], rtol=1e-10, atol=0.0, equal_nan=True), key
    assert np.array_equal(got["d_used"], want["d_used"])
    assert np.array_equal(np.isnan(got["d_mean"]), np.isnan(want["d_mean"]))
    assert np.array_equal(np.isnan(got["d_std"]), np.isnan(want["d_std"]))


@pytest.mark.parametrize("J", [1, 2, 5])
def test_stats_against_the_reference(J):
    for n in (1, 67):
        for n_aux in (0, 3, 5):
            for L in (16, 256):
                z, spec, recon, calib = ar.stats_inputs(J * 100 + n + n_aux + L, J, n, 5, n_aux, L)
                got = _stats_dev(z, spec, recon, calib)
                _check_stats(got, ar.ensemble_stats(z, spec, recon, calib))
                if J == 1:
                    assert not got["z_std"].any() and not np.nan_to_num(got["d_std"]).any()


def test_stats_every_kind_and_a_descriptor_nobody_fits():
    z, spec, recon, calib = ar.stats_inputs(3, 5, 67, 5, 5, 256)
    assert {0.0, 1.0, 2.0} == set(calib[:, :, 0].ravel().tolist())              # every kind in one table
    _check_stats(_stats_dev(z, spec, recon, calib), ar.ensemble_stats(z, spec, recon, calib))
    z, spec, recon, calib = ar.stats_inputs(4, 5, 67, 5, 5, 256, kinds=2)
    assert not calib[:, 2, 0].any()
    got = _stats_dev(z, spec, recon, calib)
    _check_stats(got, ar.ensemble_stats(z, spec, recon, calib))
    assert got["d_used"].tolist() == [5.0, 5.0, 0.0, 5.0, 5.0]
    assert np.isnan(got["d_mean"][:, 2]).all() and np.isnan(got["d_std"][:, 2]).all()
    assert np.isfinite(got["d_mean"][:, [0, 1, 3, 4]]).all()


def test_stats_identical_planes_and_repeatability():
    """J identical planes: ``J x`` is exact in double for an fp32 ``x`` (24 + 3 bits), so the mean is ``x`` itself and
    every deviation 0.  The same holds for the descriptors where the prediction is exact in few bits: the classes (4, 5
    or 6), and a linear row with slope 0.5 and intercept 0.25 (``z - 0.25`` is exact in double for the styles here,
    ``|z| < 4`` on a grid of ``2^-24`` at worst; the division by 0.5 is a shift)."""
    J = 5
    z1, spec, recon1, _ = ar.stats_inputs(9, 1, 67, 5, 3, 256)
    z, recon = np.repeat(z1, J, axis=0), np.repeat(recon1, J, axis=0)
    calib = np.tile(np.array([[1.0, 0.5, 0.25, 0.0], [2.0, -0.7, 0.9, 0.0], [1.0, -0.5, 0.25, 0.0]]), (J, 1, 1))
    got = _stats_dev(z, spec, recon, calib)
    assert np.array_equal(got["z_mean"], z1[0].astype(np.float64))
    assert not got["z_std"].any() and not got["d_std"].any()
    assert np.array_equal(got["d_mean"][:, 0], (z1[0, :, 0].astype(np.float64) - 0.25) / 0.5)
    again = _stats_dev(z, spec, recon, calib)
    for key in got:
        assert got[key].tobytes() == again[key].tobytes(), key


# ------------------------------------------------------------------------------------------------ apply_models
N_IN = 67


def _write_jobs(root, form, seeds=(101, 202, 303)):
    from rankaae_amd import model as pm
    cls = pm.AE_CLS_DICT[form]
    for t, seed in enumerate(seeds):
        torch.manual_seed(seed)
        enc = cls["encoder"](nstyle=6, dropout_rate=0.04, dim_in=256, n_layers=5)
        dec = cls["decoder"](nstyle=6, dropout_rate=0.04, last_layer_activation="Softplus", dim_out=256, n_layers=5)
        dis = pm.DiscriminatorFC(nstyle=6, dropout_rate=0.056, noise=0.56, layers=3)
        os.makedirs(os.path.join(root, "training", f"job_{t + 1}"))
        torch.save({"Encoder": enc, "Decoder": dec, "Style Discriminator": dis},
                   os.path.join(root, "training", f"job_{t + 1}", "final.pt"))
    return [f"job_{t + 1}" for t in range(len(seeds))]


def _foreign(grid, spec):
    """The rows on a grid of 400 points, a slightly wider range, non-uniform spacing."""
    t = np.linspace(0.0, 1.0, 400)
    src = (grid[0] - 1.0) + (grid[-1] - grid[0] + 2.0) * (t + 0.05 * np.sin(2.0 * np.pi * t))
    return src, np.stack([np.interp(src, grid, r) for r in spec])


class _Setup:
    pass


@pytest.fixture(scope="module", params=["FC", "compact"])
def setup(request, tmp_path_factory):
    """Three freshly constructed models of one form, a synthetic validation split of 200 rows, 67 input rows, and the
    unchunked run on the model's own grid that several tests compare with."""
    from rankaae_amd import apply
    from rankaae_amd.dataloader import AuxSpectraDataset
    from rankaae_amd.synthetic import make_spectra
    s = _Setup()
    s.form, s.root = request.param, str(tmp_path_factory.mktemp("apply_" + request.param))
    s.jobs = _write_jobs(s.root, s.form)
    s.jobs_dir = os.path.join(s.root, "training")
    spec, aux, s.grid = make_spectra(200, 256, 5, seed=21)
    s.val_ds = AuxSpectraDataset(spec, aux, s.grid, list(range(200)), {})
    s.spec = make_spectra(N_IN, 256, 5, seed=22)[0]
    s.info = {}
    s.own = apply.apply_models(s.jobs_dir, s.jobs, s.val_ds, s.spec, s.grid, s.grid, keep_recon=True, info=s.info)
    return s


def _reconstruct(s, job, x):
    from rankaae_amd import report
    eng = report.engine_from_model(report.load_model(s.jobs_dir, job), s.val_ds)
    z, out = eng.reconstruct(x)
    z, out = z.cpu().numpy(), out.cpu().numpy()
    eng.release()
    return z, out


def test_apply_on_the_models_own_grid(setup):
    s, out = setup, setup.own
    print(f"apply_models {s.form}: {s.info}")
    if s.form == "FC":      # (every launch of the dense networks has the batched form)
        assert s.info["mode"] == "batched" and s.info["launches"] > 0
    x32 = s.spec.astype(np.float32)
    assert out["spec"].tobytes() == x32.tobytes() and not out["outside"].any()          # the identity resample
    assert out["styles"].shape == (3, N_IN, 6) and out["mae"].shape == (3, N_IN) and out["jobs"].tolist() == s.jobs
    x = torch.as_tensor(x32).to(DEV)
    for j, job in enumerate(s.jobs):
        z, rec = _reconstruct(s, job, x)
        assert out["styles"][j].tobytes() == z.tobytes(), f"{job}: styles differ from StepEngine.reconstruct"
        assert out["recon"][j].tobytes() == rec.tobytes(), f"{job}: reconstruction differs from StepEngine.reconstruct"
    assert out["calib"].shape == (3, 5, 4) and set(out["calib"][:, 1, 0].tolist()) <= {0.0, 2.0}
    _check_stats(out, ar.ensemble_stats(out["styles"], out["spec"], out["recon"], out["calib"]))


def test_apply_on_a_foreign_grid(setup):
    from rankaae_amd import apply
    s = setup
    src, spec_f = _foreign(s.grid, s.spec)
    out = apply.apply_models(s.jobs_dir, s.jobs, s.val_ds, spec_f, src, s.grid)
    x = apply.resample(spec_f, src, s.grid)
    assert out["spec"].tobytes() == x.cpu().numpy().tobytes() and not out["outside"].any()
    assert np.max(np.abs(out["spec"] - s.spec)) < 0.05                                   # (it is the same spectrum)
    for j, job in enumerate(s.jobs):
        assert out["styles"][j].tobytes() == _reconstruct(s, job, x)[0].tobytes(), job
    assert np.array_equal(out["calib"], s.own["calib"])


def test_apply_in_chunks_is_bitwise_the_unchunked_run(setup):
    from rankaae_amd import apply
    s = setup
    out = apply.apply_models(s.jobs_dir, s.jobs, s.val_ds, s.spec, s.grid, s.grid, chunk_rows=64, keep_recon=True)
    assert set(out) == set(s.own)
    for key in out:
        assert out[key].tobytes() == s.own[key].tobytes(), key


def test_apply_outside_points(setup):
    from rankaae_amd import apply
    s = setup
    with pytest.raises(ValueError, match="outside"):
        apply.apply_models(s.jobs_dir, s.jobs, s.val_ds, s.spec[:, :-1], s.grid[:-1], s.grid, max_outside=0)
    out = apply.apply_models(s.jobs_dir, s.jobs, s.val_ds, s.spec[:, :-1], s.grid[:-1], s.grid, max_outside=1)
    assert out["outside"].sum() == 1 and out["outside"][-1]
    assert np.array_equal(out["spec"][:, -1], out["spec"][:, -2])                        # the edge value
    with pytest.raises(ValueError, match="row 3, column 7"):
        bad = s.spec.copy()
        bad[3, 7] = np.nan
        apply.resample(bad, s.grid, s.grid)


# ------------------------------------------------------------------------------------------------ the command
def test_command(setup):
    """``python -m rankaae_amd.cmd.apply`` in a child process on the directory above."""
    import yaml
    from rankaae_amd import apply
    from rankaae_amd.cmd.generate_report import validation_split
    from rankaae_amd.synthetic import make_spectra, write_csv
    s = setup
    spec, aux, grid = make_spectra(400, 256, 5, seed=23)
    write_csv(os.path.join(s.root, "data.csv"), spec, aux, grid)
    with open(os.path.join(s.root, "cfg.yaml"), "w") as f:
        yaml.safe_dump(dict(data_file="data.csv", n_aux=5, output_name="report", top_n=3, apply_top_n=2), f)
    n = 20
    src, spec_f = _foreign(grid, s.spec[:n])
    with open(os.path.join(s.root, "beamline.csv"), "w") as f:
        f.write(",".join(["sample", "site", "AUX_0"] + [f"ENE_{e!r}" for e in src.tolist()]) + "\n")
        for r in range(n):
            f.write(",".join([f"s-{r}", str(r % 3), "" if r % 2 else repr(0.25 * r)] + [repr(float(v)) for v in spec_f[r]]) + "\n")
    env = dict(os.environ, PYTHONPATH=REPO)
    for key in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(key, None)
    r = subprocess.run([sys.executable, "-m", "rankaae_amd.cmd.apply", "-c", "cfg.yaml", "-w", s.root, "-i", "beamline.csv"],
                       env=env, cwd=s.root, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    with open(os.path.join(s.root, "report_apply.csv")) as f:
        lines = [ln.rstrip("\n").split(",") for ln in f]
    want = ["sample", "site", "AUX_0"]
    for i in range(6):
        want += [f"STYLE_{i}_mean", f"STYLE_{i}_std"]
    for i in range(5):
        want += [f"PRED_{i}_mean", f"PRED_{i}_std"]
    assert lines[0] == want + ["MAE_mean"] and len(lines) == n + 1
    for r_, cells in enumerate(lines[1:]):
        assert cells[:3] == [f"s-{r_}", str(r_ % 3), "" if r_ % 2 else repr(0.25 * r_)]
    with np.load(os.path.join(s.root, "report_apply.npz")) as z:
        saved = {key: z[key] for key in z.files}
    assert len(saved["jobs"]) == 2 and set(saved["jobs"].tolist()) <= set(s.jobs)
    assert [float(c) for c in lines[1][3:5]] == [saved["z_mean"][0, 0], saved["z_std"][0, 0]]
    assert float(lines[n][-1]) == saved["mae_mean"][n - 1]
    val_ds = validation_split(os.path.join(s.root, "data.csv"), 5)
    out = apply.apply_models(s.jobs_dir, saved["jobs"].tolist(), val_ds, spec_f, src, val_ds.grid)
    assert set(out) == set(saved)
    for key in out:
        assert np.asarray(out[key]).tobytes() == saved[key].tobytes(), key
