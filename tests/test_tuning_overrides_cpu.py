"""Holds ``test_tuning_overrides_gpu.py`` to the sources without a GPU: the override names and defaults are those the
kernel files read, every case's mirrored geometry stays inside what the rigs and the default path provide, and the
twins reached by default and under ``big_all`` together are all 80."""
import os
import re

import block_reference as br
import co_reference as co
import conv_reference as cr
import test_co_kernels_gpu as cok
import test_tuning_overrides_gpu as tu

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), os.pardir, "rankaae_amd", "csrc")


def _read(name):
    with open(os.path.join(CSRC, name)) as fh:
        return fh.read()


def overrides_in_sources():
    """{name: default} of every ``getenv`` / ``env_int`` in raae_conv.hip and raae_disc.hip."""
    conv, disc = _read("raae_conv.hip"), _read("raae_disc.hip")
    consts = {k: int(v, 0) for k, v in re.findall(r"static const int (\w+) = (\w+);", conv)}
    out = {}
    for name, dflt in re.findall(r'env_int\("(\w+)",\s*(\w+)\)', conv):
        out[name] = consts[dflt] if dflt in consts else int(dflt, 0)
    for name, again, dflt in re.findall(r'getenv\("(\w+)"\) \? atol\(getenv\("(\w+)"\)\) : (-?\d+)', conv):
        assert name == again
        out[name] = int(dflt)
    for name, dflt in re.findall(r'getenv\("(\w+)"\); return e \? atoi\(e\) : (-?\d+)', disc):
        out[name] = int(dflt)
    names = set(re.findall(r'getenv\("(\w+)"\)', conv + disc)) | set(re.findall(r'env_int\("(\w+)"', conv))
    assert names == set(out), f"a getenv this parser does not read: {sorted(names ^ set(out))}"
    return out


def test_names_and_defaults_are_the_sources():
    """A new or renamed override without an entry in the GPU module fails here."""
    src = overrides_in_sources()
    assert src == tu.DEFAULTS, f"sources {src}, module {tu.DEFAULTS}"
    assert tuple(tu.DEFAULTS[k] for k in tu.MASK_NAMES) == co.BIG_MASK
    assert [n.rsplit("_MASK_", 1)[1] for n in tu.MASK_NAMES] == list(cok.MASK_ENV)
    d = tu.mirror("disc_mfma_on")
    assert d["pick"] == dict(small_floats=2200, small_mult=8, small_div=256) and d["wgrad_grid"] == 128 and d["wgrad_S"] == 0
    assert "36 * 1024" in _read("raae_conv.hip") and "kTileBudget = 10 * 1024" in _read("raae_conv.hip")
    used = set()
    for name, (env, limit) in tu.SETS.items():
        assert env and set(env) <= set(tu.DEFAULTS) and 0 < limit <= 120, name
        assert any(str(tu.DEFAULTS[k]) != v and hex(tu.DEFAULTS[k]) != v for k, v in env.items()), f"{name} sets only defaults"
        used |= set(env)
    assert used == set(tu.DEFAULTS), f"overrides without a set: {sorted(set(tu.DEFAULTS) - used)}"


def test_mirror_values():
    assert tu.mirror("big_all")["big_mask"] == (0xff,) * 5 and tu.mirror("big_none")["big_mask"] == (0,) * 5
    assert tu.mirror("disc_mfma_on")["disc_force"] == 1 and tu.mirror("disc_mfma_off")["disc_force"] == 0
    assert (tu.mirror("wgrad_small")["wgrad_grid"], tu.mirror("wgrad_small")["wgrad_S"]) == (16, 1)
    assert (tu.mirror("wgrad_wide")["wgrad_grid"], tu.mirror("wgrad_wide")["wgrad_S"]) == (256, 3)
    assert tu.mirror("pick_one")["pick"] == dict(small_floats=0, small_mult=8, small_div=256)
    assert tu.mirror("pick_many")["pick"] == dict(small_floats=2200, small_mult=2, small_div=64)


def test_geometry_mirror_at_the_defaults():
    """The figures the block module's docstrings state for the default path."""
    mir = tu.mirror("disc_mfma_on")
    g = tu.geometry("dec3", 4099, mir)
    assert [g[k]["S"] for k in ("fwd_a", "fwd_b", "bwd_b", "bwd_a")] == [8, 8, 8, 3]       # (phase A: 10240 // 3144 floats)
    assert [g[k]["groups"] for k in ("fwd_a", "fwd_b", "bwd_b", "bwd_a")] == [513, 513, 513, 1367]
    assert all(g[k]["rows"] == 512 for k in ("fwd_a", "fwd_b", "bwd_b", "bwd_a"))
    assert all(t["rows"] <= 128 for t in g["wgrad"]) and len(g["wgrad"]) == 4
    assert len(tu.geometry("enc0", 37, mir)["wgrad"]) == 6 and len(tu.geometry("dec2", 37, mir)["wgrad"]) == 5
    d = tu.block_dims("dec0")
    assert (d["Cin"], d["Cout"], d["Lin"], d["L1"], d["Lout"], d["E"]) == (6, 8, 1, 2, 8, 1)
    assert tu.strip_ok(tu.block_dims("dec3")["cv1"]) and not tu.strip_ok(tu.block_dims("enc1")["cv1"])


def test_every_case_stays_inside_the_rigs_and_the_tile_budget():
    """For every block case of every set: S and the counts a launch returns lie in 1..512 (the rigs' buffers hold 512
    rows), the staged tile is at most kTileBudget (40 KB), and the whole dynamic LDS -- the tile plus the weights the
    kernel keeps beside it, which kTileBudget does not count -- is at most the largest the default path uses in the
    block module's own cases: 42528 bytes (phase A backward of dec3 at 4099 rows, a 9432-float tile and 1200 weights)."""
    base = tu.mirror("disc_mfma_on")
    default_lds = max(v["lds"] for n in list(br.TABLE_SHAPES) + ["gen_c"] for rows in (37, 1027, 4099)
                      for g in [tu.geometry(n, rows, base)] for v in [g[k] for k in ("fwd_a", "fwd_b", "bwd_b", "bwd_a")] + g["wgrad"])
    assert default_lds == 42528
    seen = 0
    for name in tu.SETS:
        mir = tu.mirror(name)
        for case, runner, args in tu.cases(name):
            if runner not in ("forced", "chained", "first", "running", "eval", "planes"):
                continue
            shape, rows = (args[1], args[2]) if runner == "planes" else (args[0], args[1])
            g = tu.geometry(shape, rows, mir)
            for k, v in list((k, g[k]) for k in ("fwd_a", "fwd_b", "bwd_b", "bwd_a")) + [("wgrad", t) for t in g["wgrad"]]:
                assert 1 <= v["S"] <= rows and 1 <= v["rows"] <= cr.MAX_PARTS, (name, case, k, v)
                assert v["groups"] == cr.cdiv(rows, v["S"]), (name, case, k, v)
                assert v["tile"] <= cr.TILE_BUDGET, (name, case, k, v)
                assert v["lds"] <= default_lds, (name, case, k, v)
            seen += 1
    assert seen > 100


def test_the_geometry_sets_move_the_geometry():
    """Each geometry set changes S or the grid of some case against the default (else it pins nothing new), and the
    forced weight-gradient S applies only from 1024 rows."""
    base = tu.mirror("disc_mfma_on")
    for name in tu.GEOMETRY_SETS:
        mir = tu.mirror(name)
        moved = [(n, rows) for n in list(br.TABLE_SHAPES) + ["gen_c"] for rows in (37, 1027)
                 if tu.geometry(n, rows, mir) != tu.geometry(n, rows, base)]
        assert moved, name
        print(name, "moves", moved)
    wide, small = tu.mirror("wgrad_wide"), tu.mirror("wgrad_small")
    assert {t["S"] for t in tu.geometry("dec3", 1027, wide)["wgrad"]} == {3}
    assert {t["S"] for t in tu.geometry("dec3", 1027, small)["wgrad"]} == {1}
    assert all(t["S"] == 1 for t in tu.geometry("dec3", 37, wide)["wgrad"])
    assert all(t["rows"] <= 16 for t in tu.geometry("dec3", 1027, small)["wgrad"])


def test_cases_of_the_sets():
    """FORM -> CASE: the 18 BIG instances and their twins under ``big_all``; with the default twins all 80."""
    a = tu.cases("big_all")
    mask = (0xff,) * 5
    new = {(k, n) for k in co.FAMILY for n in br.TABLE_SHAPES if co.use_big(1027, k, n, mask) and not co.use_big(1027, k, n)}
    assert len(new) == 18 and {n for _, n in new} == set(tu.NEW_BIG)
    assert {(args[0], args[1]) for _, r, args in a if r == "planes"} == new
    for n in tu.NEW_BIG:
        names = {c for c, _, _ in a}
        assert {f"forced:{n}@1027", f"forced:{n}@1027,bn", f"forced:{n}@4099,bn", f"chained:{n}@1027"} <= names
    # the 16-byte sub-paths of dec0 and enc2 (Lout = 8) need S * Lout >= 256: not at 1027 or 4099 rows, at QUAD_ROWS yes,
    # in every row-writing kernel, with a partial last group and (enc2) more groups than workgroups
    mir = tu.mirror("big_all")
    assert tu.mirror("big_all")["pick"] == tu.mirror("disc_mfma_on")["pick"]
    assert dict(tu.QUAD_ROWS) == {"dec0": 8195, "enc2": 16387}
    for n, rows in tu.QUAD_ROWS:
        assert tu.block_dims(n)["Lout"] == 8 and f"forced:{n}@{rows},bn" in {c for c, _, _ in a}
        for small in (1027, 4099):
            assert all(tu.geometry(n, small, mir)[k]["S"] * 8 < 256 for k in ("fwd_a", "fwd_b", "bwd_b", "bwd_a"))
        g = tu.geometry(n, rows, mir)
        assert all(g[k]["S"] * 8 >= 256 and rows % g[k]["S"] == 3 for k in ("fwd_a", "fwd_b", "bwd_b", "bwd_a")), g
    assert [tu.geometry("dec0", 8195, mir)[k]["groups"] for k in ("fwd_a", "fwd_b", "bwd_b", "bwd_a")] == [257] * 4
    assert [tu.geometry("enc2", 16387, mir)[k]["groups"] for k in ("fwd_a", "fwd_b", "bwd_b", "bwd_a")] == [513, 257, 513, 513]
    assert tu.geometry("dec0", 8193, mir)["bwd_b"]["S"] == 32 and tu.geometry("dec0", 8192, mir)["bwd_b"]["S"] == 16
    assert tu.geometry("enc2", 7937, mir)["fwd_b"]["S"] == 32 and tu.geometry("enc2", 16384, mir)["bwd_a"]["S"] == 32
    default = {(k, co.K_SHAPE[co.shape_k(n)], co.use_big(rows, k, n)) for k, n, rows in cok.BLOCK_PLANE_CASES}
    reached = default | {(k, n, True) for k, n in new}
    assert reached == co.block_twins(mask) and len(reached) == 80
    b = tu.cases("big_none")
    assert {args[0] for _, r, args in b if r == "forced"} == {"enc0", "dec2", "dec3", "gen_c"}
    moved = tu.moved_pairs((0,) * 5)
    assert [i for i, want in moved] == [0, 1, 3, 5, 13, 14, 15, 16] and all(want == i for i, want in moved)
    assert [args[0] for _, r, args in b if r == "pair"] == [i for i, _ in moved]
    assert [i for i, want in tu.moved_pairs(mask)] == [7, 8, 9, 11] and all(want is None for _, want in tu.moved_pairs(mask))
    assert tu.geometry("dec3", 4099, tu.mirror("big_none"))["fwd_a"]["groups"] == 513
    on, off = tu.cases("disc_mfma_on"), tu.cases("disc_mfma_off")
    assert len(on) == 6 and len(off) == 3 and all(c.startswith("disc:dm_") for c, _, _ in off)
    for name in tu.GEOMETRY_SETS:
        g = tu.cases(name)
        assert len(g) == 18 and sum(r == "chained" for _, r, _ in g) == 2
    assert len({(s, c) for s, c in tu.ALL}) == len(tu.ALL)
    table = tu.__doc__.split("FORM -> CASE")[1]
    for name in tu.SETS:
        assert re.search(r"\b" + name + r"\b", table), name
