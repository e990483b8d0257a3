"""Every kernel of ``raae_select.hip`` (14: rank / mae / sweep / stat, the masked rank / sweep / stat, and the
one-model-per-grid-plane twin of each) and of ``raae_metrics.hip`` (5) against ``tests/select_reference.py``: one
entry-point call per test, the test's own threshold table, work buffer and output block, both filled with a sentinel byte
and followed by guard bytes.  Ranks, per-row MAEs, sweep counts, arg-max indices, thresholds and confusion counts are
read back and compared EXACTLY; each floating output within ``max(64 eps scale, 16 |ref64 - ref_hp|)`` where the second
term is the float64 restatement's own distance from its high-precision form on that case's inputs
(``select_reference.bound``; ``tests/test_select_reference_cpu.py`` asserts beforehand that the restatement alone sits
inside every bound and holds the restatement to scipy / numpy / scikit-learn).

FORM -> CASE (recomputed from the mirror by ``test_select_reference_cpu.py::test_case_table_reaches_every_form``)

  rank tile: one partial tile, exactly one, one over, two + odd tail; even / odd double2 tail   tile3 .. tile4099
  a run of equal values across index 2048 (styles and descriptors)                              tile2049, tile4099
  MAE: L = 1, 32, 63, 64, 65, 256; one, two, three rows in the last workgroup; n_aux = 1        mae_n3_L1 .. mae_n1027_L65
  problem shape: k = 2, 6, 13, 64; n_aux = 1, 2, 5, k                                           shape_k2_a2 .. shape_k64_a64
  sweeps / arg-max: n_th = 1, 255, 256, 257, 700 (the report's grid), 4097; ties; 0 / 0; 2/4 = 4/8  sw_1 .. sw_4097, sw_craft, sw_two
  classes: three, two, four (no result), below 0 and above 2, 3.5 and 4.5                       sw_*, cls_two, cls_four, cls_outside, cls_frac
  masked form of each class above; 3 and 2 labelled rows; unlabelled rows round 2048            *_m
  degenerate columns: two-valued and constant descriptor, constant style                        deg_two37, deg_two2049, deg_constdesc, deg_conststyle
  grid planes (two models, other data), graph replay                                            pl_*, cap_*
  raae_style_metrics: sm_n{n}_k{k}; constant, tiny-range, NaN column                            sm_*, smx_*
  raae_group_mean: (1, 1, 1), (3, 20, 256), (37, 7, 65), (2049, 3, 257: the grid stride)        gm_*
"""
import collections
import ctypes as C
import functools
import time
import zlib

import numpy as np
import pytest
import torch

import select_reference as sr

pytestmark = pytest.mark.gpu

SENT = 0xA5
GUARD = 256                                   # bytes behind every buffer
WORST = {}                                    # quantity class -> (largest share of its bound, case)
SLOW = {}

Case = collections.namedtuple("Case", "name n k n_aux L th cn masked deg", defaults=("three", False, None))

TILE_N = (3, 4, 37, 255, 256, 257, 1027, 2047, 2048, 2049, 4099)
MAE_NL = ((3, 1), (5, 32), (6, 63), (7, 64), (5, 256), (7, 65), (1027, 65))
SHAPES = ((2, 2), (6, 5), (13, 2), (13, 13), (64, 1), (64, 64))
SWEEP_NTH = (1, 255, 256, 257, 700, 4097)

CASES = ([Case(f"tile{n}", n, 3, 3, 8, 5) for n in TILE_N] +
         [Case(f"tile{n}_m", n, 3, 3, 8, 5, masked=True) for n in (37, 2049, 4099)] +
         [Case(f"mae_n{n}_L{L}", n, 2, 1, L, 0) for n, L in MAE_NL] +
         [Case(f"shape_k{k}_a{a}", 41, k, a, 5, 5 if a > 1 else 0) for k, a in SHAPES] +
         [Case(f"shape_k{k}_a{a}_m", 41, k, a, 5, 5, masked=True) for k, a in ((2, 2), (6, 5), (13, 13), (64, 64))] +
         [Case(f"sw_{t}", 48, 2, 2, 4, t) for t in SWEEP_NTH] +
         [Case("sw_craft", 12, 2, 2, 4, 257, cn="craft"), Case("sw_two", 48, 2, 2, 4, 257, cn="two"),
          Case("sw_257_m", 48, 2, 2, 4, 257, masked=True)] +
         [Case(f"cls_{c}", 37, 2, 2, 4, 64, cn=c) for c in ("two", "four", "outside", "frac")] +
         [Case("cls_frac_m", 37, 2, 2, 4, 64, cn="frac", masked=True), Case("cls_four_m", 37, 2, 2, 4, 64, cn="four", masked=True)] +
         [Case("deg_two37", 37, 3, 3, 4, 700, deg="two"), Case("deg_two2049", 2049, 3, 3, 4, 5, deg="two"),
          Case("deg_constdesc", 37, 3, 3, 4, 700, deg="constdesc"), Case("deg_conststyle", 37, 6, 3, 4, 700, deg="conststyle")])
BY_NAME = {c.name: c for c in CASES}
PLANES = {"pl_tile2049": "tile2049", "pl_shape_k6_a5_m": "shape_k6_a5_m", "pl_mae_n7_L65": "mae_n7_L65",
          "pl_deg_two37": "deg_two37", "pl_deg_constdesc": "deg_constdesc", "pl_deg_conststyle": "deg_conststyle"}
CAPTURES = {"cap_tile2049": "tile2049", "cap_tile2049_m": "tile2049_m"}

SM_NK = ((3, 1), (4, 2), (37, 13), (255, 2), (256, 1), (257, 13), (258, 2), (259, 1), (1027, 2), (2047, 2), (2048, 13),
         (2049, 2), (4099, 2), (41, 64))
GM_CASES = ((1, 1, 1), (3, 20, 256), (37, 7, 65), (2049, 3, 257))

CN_SETS = {"three": [4.0, 5.0, 6.0], "two": [4.0, 5.0], "four": [4.0, 5.0, 6.0, 7.0], "outside": [3.0, 5.0, 7.0],
           "frac": [3.5, 4.5, 5.2, 6.9]}
LEVELS = np.arange(-28, 29) / 8.0              # thresholds on the grid the styles are rounded to: z == th happens
THRESH_GRID = np.linspace(-3.5, 3.5, 700)     # == report.THRESH_GRID (asserted in the CPU module)


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


@functools.lru_cache(maxsize=None)
def case_data(name, variant=""):
    """``(styles f32 [n, k], aux f64 [n, n_aux], spec_in, spec_out f32 [n, L], thresholds f64)`` of a case: heavy ties in
    styles and descriptors, a run of equal values across index 2048, NaN cells where the case is masked.  ``variant``:
    other data of the same shape (the second grid plane)."""
    c = BY_NAME[name]
    g = _rng(name + variant)
    n, k, n_aux = c.n, c.k, c.n_aux
    if n < 8:
        # too few rows for ties: every descriptor a shuffled, evenly spread column (a well-conditioned fit)
        aux = np.stack([g.permutation(np.linspace(-1.0, 1.0, n)) * (1.0 + i) + 0.25 * i for i in range(n_aux)], axis=1)
    else:
        aux = g.standard_normal((n, n_aux))
        aux[:, ::2] = np.round(aux[:, ::2] * 4.0) / 4.0                  # heavy ties in every other descriptor
    z = g.standard_normal((n, k))
    for i in range(n_aux):
        z[:, i] = (1.0 if i % 3 else -1.0) * (aux[:, i] + 0.2 * aux[:, i] ** 2) + 0.5 * z[:, i]
    z[:, k - 1] += 0.3 * z[:, 0]
    z = np.round(z * 8.0) / 8.0 if n >= 8 else z                         # ties in the styles, on the threshold grid
    if n > 2048:
        z[2040:2060, 0], aux[2040:2060, 0] = z[2040, 0], aux[2040, 0]    # a run of equal values across index 2048
        z[2046:2050, k - 1] = z[2046, k - 1]
    if n_aux >= 2:
        if c.cn == "craft":
            # ascending styles; class 0 on rows 1 and 5 only: sweep 0 peaks at 2/4 (threshold behind row 1) and 4/8
            # (behind row 5), sweep 1 has class 2 on the two top rows
            z[:, 1] = -1.5 + 0.25 * np.arange(n)
            aux[:, 1] = 5.0
            aux[[1, 5], 1] = 4.0
            aux[[n - 2, n - 1], 1] = 6.0
        else:
            vals = CN_SETS[c.cn]
            aux[:, 1] = g.choice(vals, size=n)
            aux[:len(vals), 1] = vals
            z[:, 1] = np.clip(np.round(((aux[:, 1] - 5.0) * 1.1 + 0.8 * g.standard_normal(n)) * 8.0) / 8.0, -3.0, 3.0)
    if c.deg == "two":
        aux[:, 0] = (g.random(n) < 0.4).astype(np.float64)
        aux[:2, 0] = [0.0, 1.0]
    elif c.deg == "constdesc":
        aux[:, 0] = 1.25
    elif c.deg == "conststyle":
        z[:, 4] = 0.5
    if c.masked:
        keep = g.random((n, n_aux)) < 0.7
        if n > 2048:
            keep[2044:2049, :] = np.array([0, 1, 0, 1, 0], dtype=bool)[:, None]             # unlabelled on both sides of 2048
        if n_aux >= 3:
            keep[:, n_aux - 1] = False
            keep[g.choice(n, 3, replace=False), n_aux - 1] = True        # exactly three labelled rows
        if n_aux >= 5:
            keep[:, n_aux - 2] = False
            keep[g.choice(n, 2, replace=False), n_aux - 2] = True        # two: the slice is zeros
        aux = np.where(keep, aux, np.nan)
        if c.cn != "craft" and n_aux >= 2:
            rows = np.flatnonzero(keep[:, 1])[:len(CN_SETS[c.cn])]
            aux[rows, 1] = CN_SETS[c.cn][:len(rows)]
    spec_in = (0.5 + 0.5 * g.random((n, c.L))).astype(np.float32)
    # outputs at 0.3, 1 and 2.7 times the input: where the two differ by more than a factor of two the fp32 difference
    # rounds (between y / 2 and 2 y it is exact, and a difference taken in double would go unnoticed)
    spec_out = (spec_in * g.choice([0.3, 1.0, 2.7], size=(n, c.L)) + 0.05 * g.standard_normal((n, c.L))).astype(np.float32)
    if c.th == 700:
        th = THRESH_GRID.copy()
    elif c.th:
        th = g.choice(LEVELS, size=c.th) + (0.0625 if c.cn == "craft" else 0.0)
    else:
        th = np.zeros(0)
    return z.astype(np.float32), aux, spec_in, spec_out, th


@functools.lru_cache(maxsize=None)
def case_ref(name, variant="", masked=None):
    c = BY_NAME[name]
    return sr.select_ref(*case_data(name, variant), masked=c.masked if masked is None else masked)


@functools.lru_cache(maxsize=None)
def sm_data(n, k, extra=""):
    g = _rng(f"sm{n}_{k}{extra}")
    z = g.standard_normal((n, k))
    z[:, 0] += 0.5 * z[:, k - 1]
    if n > 3 and k > 1:
        z[:, 1] = np.round(z[:, 1] * 4.0) / 4.0
        z[::7, k - 1] = z[0, k - 1]
    if n > 2048:
        z[2040:2060, 0] = z[2040, 0]
    z = z.astype(np.float32)
    if extra == "const":
        z[:, 1] = -0.75
    elif extra == "tiny":
        z[:, 1] = (g.integers(0, 1000, size=n) * 1e-18).astype(np.float32)
    elif extra == "nan":
        z[5, 1] = np.nan
    return z


def gm_data(groups, per, L):
    return (_rng(f"gm{groups}_{per}_{L}").standard_normal((groups, per, L)) * 3.0 + 1.0).astype(np.float32)


# ------------------------------------------------------------------------------------------------------------- device
def _dev():
    return torch.device("cuda:0")


class Buf:
    """A device buffer of ``nbytes`` filled with the sentinel, guard bytes behind it."""

    def __init__(self, nbytes, dtype=torch.uint8):
        self.nbytes = int(nbytes)
        pad = (-self.nbytes) % 8
        self.raw = torch.full((self.nbytes + pad + GUARD,), SENT, dtype=torch.uint8, device=_dev())
        self.t = self.raw[:self.nbytes].view(dtype)

    def bytes(self):
        return self.raw.cpu().numpy()

    def guard_ok(self):
        return bool((self.raw[self.nbytes:] == SENT).all())


class SelDev:
    def __init__(self, name, variant="", masked=None):
        from rankaae_amd import ops
        self.c = c = BY_NAME[name]
        self.masked = c.masked if masked is None else masked
        z, aux, si, so, th = case_data(name, variant)
        d = _dev()
        self.z, self.aux = torch.from_numpy(z).to(d), torch.from_numpy(aux).to(d)
        self.si, self.so = torch.from_numpy(si).to(d), torch.from_numpy(so).to(d)
        self.th = torch.from_numpy(th).to(d)
        nbytes = ops.select_work_bytes(c.n, c.k, c.n_aux, len(th), self.masked)
        mirror = (sr.select_masked_work_bytes if self.masked else sr.select_work_bytes)(c.n, c.k, c.n_aux, len(th))
        assert nbytes == mirror, (nbytes, mirror)
        self.work, self.out = Buf(nbytes), Buf(8 * (sr.HEAD + sr.STRIDE * c.n_aux), torch.float64)

    def launch(self):
        from rankaae_amd import ops
        c = self.c
        ops.select_scores(self.z, c.n, c.k, self.aux, c.n_aux, self.si, self.so, c.L, self.th, self.work.t, self.out.t,
                          masked=self.masked)

    def bits(self):
        torch.cuda.synchronize()
        return self.work.bytes().tobytes(), self.out.bytes().tobytes()


def _share(cls, case, err, tol):
    s = err / tol if tol > 0 else (0.0 if err == 0 else np.inf)
    if s > WORST.get(cls, (-1.0, ""))[0]:
        WORST[cls] = (float(s), case)
    return s


def check_select(dev, ref, name):
    """Everything one call wrote, against the reference; every mismatch is collected, then asserted at once."""
    c, bad = dev.c, []
    torch.cuda.synchronize()
    wb, ob = dev.work.bytes(), dev.out.bytes()
    n_th = dev.th.numel()
    lay = sr.work_layout(c.n, c.k, c.n_aux, n_th, dev.masked)
    assert lay["bytes"] == dev.work.nbytes

    def view(key):
        off, dt, shape = lay[key]
        return wb[off:off + int(np.prod(shape)) * np.dtype(dt).itemsize].view(dt).reshape(shape)
    if not np.array_equal(view("rank_z"), ref["rank_z"]):
        bad.append(f"rank_z (rows {np.flatnonzero((view('rank_z') != ref['rank_z']).any(0))[:5]})")
    for key in ("rank_d",) + (("rank_zs",) if dev.masked else ()):
        for i in range(c.n_aux):
            if ref[key][i] is not None and not np.array_equal(view(key)[i], ref[key][i]):
                bad.append(f"{key}[{i}] (rows {np.flatnonzero(view(key)[i] != ref[key][i])[:5]})")
    mae = view("mae")[0]
    exact = sr.mae_rows(dev.si.cpu().numpy(), dev.so.cpu().numpy())[1]
    for r in range(c.n):
        tol = sr.bound(ref["mae"][r], ref["mae"][r], float(exact[r]))
        if _share("MAE row", name, abs(mae[r] - ref["mae"][r]), tol) > 1.0:
            bad.append(f"mae row {r}: {mae[r]!r} != {ref['mae'][r]!r}")
            break
    if c.n_aux >= 2 and not np.array_equal(view("sweep"), ref["sweep"]):
        bad.append(f"sweep counts (first at {np.argwhere(view('sweep') != ref['sweep'])[:3].tolist()})")
    unwritten = ~sr.written_bytes(c.n, c.k, c.n_aux, n_th, dev.masked)
    if not (wb[:lay["bytes"]][unwritten] == SENT).all():
        bad.append(f"work bytes the mirror calls unwritten were written (first at {np.flatnonzero(unwritten & (wb[:lay['bytes']] != SENT))[:3]})")
    if not dev.work.guard_ok() or not dev.out.guard_ok():
        bad.append("guard bytes")
    got = ob[:dev.out.nbytes].view(np.float64)
    for j in range(len(got)):
        want, cls = ref["block"][j], ref["cls"][j]
        d, s = divmod(j - sr.HEAD, sr.STRIDE) if j >= sr.HEAD else (-1, j)
        if cls is None:
            if got[j] == want:
                continue
            bad.append(f"slot {j} (descriptor {d}, {s}): {got[j]!r} != {want!r} exactly")
        elif d >= 0 and ref["lstsq_rank"].get(d) == 1:
            if s == 0 and not np.isnan(got[j]):
                bad.append(f"Spearman of the constant descriptor {d} is {got[j]!r}, not NaN")
        elif np.isnan(want):
            if not np.isnan(got[j]):
                bad.append(f"slot {j} ({cls}): {got[j]!r}, not NaN")
        else:
            share = _share(cls, name, abs(got[j] - want), ref["tol"][j])
            if not share <= 1.0:
                bad.append(f"slot {j} ({cls}, descriptor {d}): {got[j]!r} != {want!r}, {share:.2f} of the bound {ref['tol'][j]:.2e}")
    assert not bad, f"{name}: " + "; ".join(bad)
    return got.copy()


def _timed(name, t0, cpu):
    wall = time.perf_counter() - t0
    if wall > 1.0:
        SLOW[name] = (wall, cpu)


# ============================================================================================== raae_select_scores
@pytest.mark.parametrize("name", [c.name for c in CASES])
def test_select_scores(name):
    t0 = time.perf_counter()
    ref = case_ref(name)
    cpu = time.perf_counter() - t0
    dev = SelDev(name)
    dev.launch()
    check_select(dev, ref, name)
    _timed(name, t0, cpu)


@pytest.mark.parametrize("name", [c.name for c in CASES if c.masked])
def test_masked_head_is_bitwise_the_unmasked_head(name):
    """The head uses all rows: with the NaN cells replaced by numbers the unmasked entry point writes the same four
    doubles, bit for bit."""
    m = SelDev(name)
    m.launch()
    u = SelDev(name)
    u.masked = False
    u.aux = torch.nan_to_num(u.aux, nan=5.0)
    u.launch()
    torch.cuda.synchronize()
    a, b = m.out.bytes()[:8 * sr.HEAD], u.out.bytes()[:8 * sr.HEAD]
    assert a.tobytes() == b.tobytes(), (a.view(np.float64), b.view(np.float64))


@pytest.mark.parametrize("name", ["tile37", "tile2049", "shape_k6_a5", "sw_700", "cls_four", "deg_two37", "shape_k64_a1"])
def test_fully_labelled_through_the_masked_entry_is_bitwise_the_unmasked_block(name):
    u, m = SelDev(name), SelDev(name, masked=True)
    u.launch()
    m.launch()
    torch.cuda.synchronize()
    assert u.out.bytes().tobytes() == m.out.bytes().tobytes()
    check_select(m, case_ref(name, masked=True), name + " (masked entry)")


def _two_planes(devs):
    """Each model alone, then both as one two-plane program: the planes are bit for bit the single launches."""
    from rankaae_amd import report
    single = []
    for d in devs:
        d.launch()
        single.append(d.bits())
    for d in devs:
        d.work.raw.fill_(SENT)
        d.out.raw.fill_(SENT)
    prog = report.BatchedProgram.build([d.launch for d in devs])
    assert prog is not None, "the recorder refused a batched form"
    for d in devs:
        d.work.raw.fill_(SENT)
        d.out.raw.fill_(SENT)
    prog.launch()
    planes = [d.bits() for d in devs]
    prog.release()
    for j, (a, b) in enumerate(zip(single, planes)):
        assert a[0] == b[0], f"plane {j}: the work buffer differs from the model alone"
        assert a[1] == b[1], f"plane {j}: the block differs from the model alone"


@pytest.mark.parametrize("name", list(PLANES))
def test_select_scores_two_planes(name):
    base = PLANES[name]
    devs = [SelDev(base), SelDev(base, variant="#2")]
    assert not np.array_equal(case_data(base)[0], case_data(base, "#2")[0])
    _two_planes(devs)
    check_select(devs[0], case_ref(base), name + " plane 0")
    check_select(devs[1], case_ref(base, "#2"), name + " plane 1")


def _replay(dev):
    from rankaae_amd import ops
    stream = torch.cuda.Stream(device=_dev())
    stream.wait_stream(torch.cuda.current_stream(_dev()))
    with torch.cuda.stream(stream):
        dev.launch()
        eager = dev.bits()
        g = ops.Graph()
        g.begin()
        dev.launch()
        g.end()
        for b in (dev.work, dev.out):
            b.raw.fill_(SENT)
        g.launch()
        assert dev.bits() == eager


@pytest.mark.parametrize("name", list(CAPTURES))
def test_select_scores_replayed_capture_is_bitwise_the_eager_run(name):
    dev = SelDev(CAPTURES[name])
    _replay(dev)
    check_select(dev, case_ref(CAPTURES[name]), name)


def test_degenerate_columns_on_the_host():
    """What the host makes of the three degenerate slices: the two-valued descriptor is a finite, rounded result with a
    one-element residue; the constant descriptor raises before anything is ranked; the constant style ranks."""
    from rankaae_amd import report
    blocks = {}
    for name in ("deg_two37", "deg_constdesc", "deg_conststyle"):
        dev = SelDev(name)
        dev.launch()
        blocks[name] = check_select(dev, case_ref(name), name)
    res = report.result_from_block(blocks["deg_two37"], 3)
    q = res["Style-descriptor Corr"][0]["Quadratic"]
    assert np.all(np.isfinite(q["Parameters"])) and len(q["residue"]) == 1 and np.isfinite(q["residue"][0]) and np.isfinite(q["R2"])
    assert case_ref("deg_two37")["lstsq_rank"][0] == 2
    assert np.all(np.isfinite(report.score_matrix({"a": res, "b": report.result_from_block(blocks["deg_conststyle"], 3)})[2]))
    with pytest.raises(ValueError, match="constant"):
        report.result_from_block(blocks["deg_constdesc"], 3)
    # the constant style (column 4 of 6) is left out of the maximum: the head is the maximum over the other columns
    z = case_data("deg_conststyle")[0]
    rk = [sr.avg_rank(z[:, c]) for c in range(6)]
    others = max(abs(sr.pearson(rk[c], rk[5])) for c in (0, 1, 2, 3))
    assert np.isnan(sr.pearson(rk[4], rk[5])) and case_ref("deg_conststyle")["block"][2] == others
    assert abs(blocks["deg_conststyle"][2] - others) <= case_ref("deg_conststyle")["tol"][2]


def _sel_args(dev):
    c = dev.c
    p = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731
    return [p(dev.z), c.n, c.k, p(dev.aux), c.n_aux, p(dev.si), p(dev.so), c.L, p(dev.th), dev.th.numel(), p(dev.work.t),
            p(dev.out.t), None]


REJECT = {"n2": (1, 2), "k1": (2, 1), "k65": (2, 65), "n_aux_above_k": (4, 4), "n_aux0": (4, 0), "L0": (7, 0),
          "no_thresholds": (8, None), "n_th0": (9, 0), "n_th65536": (9, 65536), "null_styles": (0, None), "null_aux": (3, None),
          "null_spec_in": (5, None), "null_spec_out": (6, None), "null_work": (10, None), "null_out": (11, None)}


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("what", list(REJECT))
def test_select_scores_rejections(what, masked):
    """Every argument check of both entry points: the invalid-argument code, nothing launched, nothing written."""
    from rankaae_amd import _lib
    dev = SelDev("tile37", masked=masked)
    args = _sel_args(dev)
    i, v = REJECT[what]
    args[i] = v
    before = dev.bits()
    fn = getattr(_lib.load(), "raae_select_scores_masked" if masked else "raae_select_scores")
    assert fn(*args) == -1, what
    assert dev.bits() == before, f"{what}: something was written"


# ============================================================================================== raae_style_metrics
class SmDev:
    def __init__(self, z):
        from rankaae_amd.metrics import shapiro_coefficients
        self.n, self.k = z.shape
        self.zh = z
        self.z = torch.from_numpy(z).to(_dev())
        self.a_host = shapiro_coefficients(self.n)
        self.a = torch.from_numpy(self.a_host).to(_dev())
        self.work = Buf(8 * 2 * self.k * self.n, torch.float64)
        self.out = Buf(8 * (self.k + self.k * (self.k - 1) // 2), torch.float64)

    def launch(self):
        from rankaae_amd import ops
        ops.style_metrics(self.z, self.n, self.k, self.a, self.work.t, self.out.t)

    def bits(self):
        torch.cuda.synchronize()
        return self.work.bytes().tobytes(), self.out.bytes().tobytes()

    def read(self):
        torch.cuda.synchronize()
        w = self.work.bytes()[:self.work.nbytes].view(np.float64).reshape(2, self.k, self.n)
        o = self.out.bytes()[:self.out.nbytes].view(np.float64)
        return w[0], w[1], o[:self.k], o[self.k:]


def check_metrics(dev, name, skip_col=None):
    import itertools
    ref = sr.style_metrics_ref(dev.zh, dev.a_host)
    rank, srt, W, rho = dev.read()
    assert dev.work.guard_ok() and dev.out.guard_ok(), f"{name}: guard bytes"
    cols = [c for c in range(dev.k) if c != skip_col]
    for c in cols:
        assert np.array_equal(rank[c], ref["rank"][c]), f"{name}: ranks of column {c}"
        assert np.array_equal(srt[c], ref["sorted"][c]), f"{name}: sorted column {c} is not the sorted input minus the pivot"
        share = _share("W", name, abs(W[c] - ref["W"][c]), sr.bound(1.0, ref["W"][c], ref["W_hp"][c]))
        assert share <= 1.0, f"{name}: W[{c}] {W[c]!r} != {ref['W'][c]!r} ({share:.2f} of the bound)"
    for j, (p, q) in enumerate(itertools.combinations(range(dev.k), 2)):
        if skip_col in (p, q):
            continue
        if np.isnan(ref["rho"][j]):
            assert np.isnan(rho[j]), f"{name}: rho({p}, {q}) of a constant column is {rho[j]!r}, not NaN"
        else:
            share = _share("metric rho", name, abs(rho[j] - ref["rho"][j]), sr.bound(1.0, ref["rho"][j], ref["rho_hp"][j]))
            assert share <= 1.0, f"{name}: rho({p}, {q}) {rho[j]!r} != {ref['rho'][j]!r} ({share:.2f} of the bound)"
    return W, rho


@pytest.mark.parametrize("n,k", SM_NK)
def test_style_metrics(n, k):
    t0 = time.perf_counter()
    dev = SmDev(sm_data(n, k))
    dev.launch()
    check_metrics(dev, f"sm_n{n}_k{k}")
    _timed(f"sm_n{n}_k{k}", t0, 0.0)


@pytest.mark.parametrize("n", [37, 2049])
def test_style_metrics_constant_column(n):
    dev = SmDev(sm_data(n, 3, "const"))
    dev.launch()
    W, rho = check_metrics(dev, f"smx_const{n}")
    assert W[1] == 1.0 and np.isnan(rho[0]) and np.isnan(rho[2]) and not np.isnan(rho[1])


def test_style_metrics_tiny_range_column():
    z = sm_data(257, 3, "tiny")
    assert 1e-19 < float(z[:, 1].max()) - float(z[:, 1].min()) < 1e-12
    dev = SmDev(z)
    dev.launch()
    W, _ = check_metrics(dev, "smx_tiny257")
    assert W[1] < 1.0


def test_style_metrics_nan_column_stays_inside_its_column():
    """A NaN element (a diverged trial's plane keeps running this kernel): its column's W is wrong by design, every store
    stays inside the column -- the guards and the other columns' results are untouched."""
    dev = SmDev(sm_data(261, 3, "nan"))
    dev.launch()
    check_metrics(dev, "smx_nan261", skip_col=1)


def test_style_metrics_two_planes_and_capture():
    devs = [SmDev(sm_data(2049, 2)), SmDev(sm_data(2049, 2, "#2"))]
    assert not np.array_equal(devs[0].zh, devs[1].zh)
    _two_planes(devs)
    for d in devs:
        check_metrics(d, "pl_sm2049")
    _replay(devs[0])
    check_metrics(devs[0], "cap_sm2049")


@pytest.mark.parametrize("what", ["n2", "k0", "k65", "null_z", "null_a", "null_work", "null_out"])
def test_style_metrics_rejections(what):
    from rankaae_amd import _lib
    dev = SmDev(sm_data(37, 13))
    p = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731
    args = [p(dev.z), 37, 13, p(dev.a), p(dev.work.t), p(dev.out.t), None]
    i, v = {"n2": (1, 2), "k0": (2, 0), "k65": (2, 65), "null_z": (0, None), "null_a": (3, None), "null_work": (4, None),
            "null_out": (5, None)}[what]
    args[i] = v
    before = dev.bits()
    assert _lib.load().raae_style_metrics(*args) == -1, what
    assert dev.bits() == before


# ================================================================================================= raae_group_mean
@pytest.mark.parametrize("groups,per,L", GM_CASES)
def test_group_mean(groups, per, L):
    """Each output within half an fp32 ulp of the exact mean plus 2^-40 |mean|: the correctly rounded value, allowing
    for the double sum's own rounding.  Guard rows behind ``out``."""
    from rankaae_amd import ops
    t0 = time.perf_counter()
    x = gm_data(groups, per, L)
    want = sr.group_mean_exact(x, groups, per, L)
    cpu = time.perf_counter() - t0
    assert (sr.group_mean_grid(groups, L) == 2048) == (groups == 2049)
    out = Buf(4 * groups * L, torch.float32)
    ops.group_mean(torch.from_numpy(x).to(_dev()), groups, per, L, out.t)
    torch.cuda.synchronize()
    got = out.bytes()[:out.nbytes].view(np.float32).reshape(groups, L).astype(np.float64)
    tol = 0.5 * sr.ulp32(want) + 2.0 ** -40 * np.abs(want)
    err = np.abs(got - want)
    WORST["group mean, of half an fp32 ulp"] = max(WORST.get("group mean, of half an fp32 ulp", (0.0, "")),
                                                   (float((err / tol).max()), f"gm_{groups}_{per}_{L}"))
    assert (err <= tol).all(), (np.argwhere(err > tol)[:3], float((err / tol).max()))
    assert out.guard_ok()
    _timed(f"gm_{groups}_{per}_{L}", t0, cpu)


def test_group_mean_capture_and_rejections():
    from rankaae_amd import _lib, ops
    x = torch.from_numpy(gm_data(37, 7, 65)).to(_dev())

    class D:
        out = Buf(4 * 37 * 65, torch.float32)
        work = out

        def launch(self):
            ops.group_mean(x, 37, 7, 65, self.out.t)

        def bits(self):
            torch.cuda.synchronize()
            return self.out.bytes().tobytes()
    d = D()
    _replay(d)
    before = d.bits()
    d.out.raw.fill_(SENT)
    clean = d.bits()
    p = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731
    for args in ([None, 37, 7, 65, p(d.out.t), None], [p(x), 37, 7, 65, None, None], [p(x), 0, 7, 65, p(d.out.t), None],
                 [p(x), 37, 0, 65, p(d.out.t), None], [p(x), 37, 7, 0, p(d.out.t), None]):
        assert _lib.load().raae_group_mean(*args) == -1
    assert d.bits() == clean and before != clean


# =========================================================================================================== summary
def test_zz_largest_share_of_each_bound():
    """Printed last: the largest share of each bound per class with the case it occurred in, and every test above one
    second with the CPU (reference) share of its time."""
    for k in sorted(WORST):
        print(f"{k}: {WORST[k][0]:.3f} ({WORST[k][1]})")
    for k, (wall, cpu) in sorted(SLOW.items()):
        print(f"slow: {k} {wall:.1f} s, of which {cpu:.1f} s CPU reference")
    assert all(v[0] <= 1.0 for v in WORST.values())
