"""Pins ``co_reference`` (the mirror of ``co_pair`` that ``test_co_kernels_gpu.py`` takes its launch counts from) without
a GPU: row for row to the ``RAAE_CO(`` lines of ``rankaae_amd/csrc/raae_conv.hip``, to the answers recorded in
``CO_TABLE`` of ``test_block_kernels_gpu.py``, and the GPU module's FORM -> CASE table to the mirror."""
import os
import re

import co_reference as co
import test_block_kernels_gpu as blocks
import test_co_kernels_gpu as gpu

SOURCE = os.path.join(os.path.dirname(os.path.abspath(__file__)), os.pardir, "rankaae_amd", "csrc", "raae_conv.hip")
KINDS = {"RAAE_CO_FWD_A": "a", "RAAE_CO_FWD_B": "b", "RAAE_CO_BWD_A": "bwd_a", "RAAE_CO_BWD_B_WGRAD": "bwd_b+wgrad",
         "kCoBwdB": "bwd_b", "RAAE_CO_ADAM": "adam", "RAAE_CO_WGRAD": "wgrad", "RAAE_CO_HEAD_FWD": "head"}
# kind -> (body tag, field of CoSide)
BODY = {"a": ("CoFwdA", "fa"), "b": ("CoFwdB", "fb"), "bwd_a": ("CoBwdA", "ba"), "bwd_b+wgrad": ("CoBwdBW", "bw"),
        "bwd_b": ("CoBwdB", "bb"), "adam": ("CoAdam", "ad"), "wgrad": ("CoWgrad", "wg"), "head": ("CoHeadFwd", "hf")}


def _side(var, kind_name, cond, templ, field):
    """One side of a ``RAAE_CO(`` line -> (mirror kind, mirror condition); the template must carry the condition."""
    kind = KINDS[kind_name]
    tag, targs = re.fullmatch(r"(\w+)<(.*)>", templ).groups()
    targs = [t.strip() for t in targs.split("COMMA")]
    assert (tag, field) == BODY[kind], (templ, field, kind)
    if kind == "adam":
        m = re.fullmatch(rf"{var}\.wide && (!?){var}\.chk", cond)
        assert m, cond
        chk = m.group(1) == ""
        assert targs == ["true" if chk else "false"], (cond, templ)
        return "adam", (True, chk)
    if cond == "true":
        assert targs == ["-1"], (cond, templ)
        return kind, "any"
    names = ["k", "kw"] if kind == "bwd_b+wgrad" else ["k"]
    m = re.fullmatch(" && ".join(rf"{var}\.{n} == (-?\d+)" for n in names), cond)
    assert m, (cond, "does not read", names, "of", var)
    nums = list(m.groups())
    assert nums == targs, f"`{cond}` with `{templ}`: the template arguments are not the numbers of the condition"
    if kind == "head":
        return "head", int(nums[0])
    if kind == "bwd_b+wgrad":
        return "bwd_b", tuple(co.K_SHAPE[int(n)] for n in nums)
    return kind, co.K_SHAPE[int(nums[0])]


def parse(text):
    body = text[text.index("#define RAAE_CO("):text.index("#undef RAAE_CO")]
    rows = []
    for line in body.splitlines()[1:]:
        line = line.strip()
        if not line.startswith("RAAE_CO("):
            continue
        f = [s.strip() for s in line[len("RAAE_CO("):line.rindex(")")].split(",")]
        assert len(f) == 9, line
        assert f[0] in ("plain", "entry"), line
        rows.append((f[0],) + _side("x", *f[1:5]) + _side("y", *f[5:9]))
    return rows


def test_mirror_is_the_table_of_the_kernel_file():
    """Every ``RAAE_CO(`` line, in order (the first match wins): gate, kinds, conditions; in every row the template
    arguments carry the numbers of the conditions and the body tag and argument field belong to the kind."""
    with open(SOURCE) as fh:
        rows = parse(fh.read())
    assert len(rows) == len(co.CO_ROWS) == 35 and co.N_PLAIN == 18
    for i, (got, want) in enumerate(zip(rows, co.CO_ROWS)):
        assert got == want, f"row {i}: the kernel file has {got}, the mirror {want}"
    assert [r[0] for r in co.CO_ROWS] == ["plain"] * 18 + ["entry"] * 17


def test_parser_notices_mismatched_template_arguments():
    line = "#define RAAE_CO(\n    RAAE_CO(plain, RAAE_CO_BWD_A, x.k == 5, CoBwdA<6>, ba, RAAE_CO_FWD_B, y.k == 0, CoFwdB<0>, fb)\n#undef RAAE_CO"
    try:
        parse(line)
    except AssertionError as e:
        assert "template arguments" in str(e)
    else:
        raise AssertionError("a row whose template names another shape than its condition was accepted")
    assert parse(line.replace("CoBwdA<6>", "CoBwdA<5>")) == [("plain", "bwd_a", "dec2", "b", "enc0")]


def test_mirror_reproduces_the_recorded_answers():
    """Both columns of ``CO_TABLE`` (256 and 1027 rows; read off the build before the forward pairs joined the table)."""
    for x, y, at256, at1027 in blocks.CO_TABLE:
        assert int(co.instance(x, y, 256, False) is not None) == at256, (x, y, 256)
        assert int(co.instance(x, y, 1027, False) is not None) == at1027, (x, y, 1027)
    for i in range(18):
        assert co.instance(*blocks.CO_TABLE[i][:2], 256, False) == i, "the first 18 recorded pairs are the plain rows, in order"
    survive = [i for i in range(18) if co.instance(*co.row_sides(i), 1027, False) is not None]
    assert survive == [7, 8, 9, 11]


def test_gate_edges():
    sides = lambda i: co.row_sides(i)
    assert co.instance(*sides(3), 1023, False) == 3 and co.instance(*sides(3), 1024, False) is None
    assert co.instance(*sides(3), (1023, 1024), False) is None and co.instance(*sides(3), (1024, 2), False) is None
    assert co.instance(*sides(17), 1023, False) == 17 and co.instance(*sides(17), 1024, False) is None      # head: `large`
    assert co.instance(("a", "enc1"), ("head", 4, False), 37, False) is None and co.instance(("a", "enc1"), ("head", 8), 37, False) is None
    assert co.instance(*sides(2), 1024, False) is None                                                     # bwd_b + wgrad: `large`
    assert co.instance(("bwd_a", "dec3"), ("adam", 16, True), 37, False) is None and co.instance(("bwd_a", "dec3"), ("adam", 17, True), 37, False) == 0
    assert co.instance(*sides(18), 4099, True) == 18 and co.instance(*sides(18), 37, False) is None         # entry rows: ungated
    assert co.instance(("bwd_b", "dec3"), ("wgrad", "gen_b"), 37, True) == 33, "any generic task list beside dec3 is row 33"
    assert co.instance(("bwd_b", "enc0"), ("wgrad", "dec3"), 37, True) == 34
    assert co.instance(*sides(3), 1027, False, big_mask=(0, 0, 0, 0, 0)) == 3
    assert co.single_is_big(("a", "enc0"), 1027) and not co.single_is_big(("a", "enc1"), 1027)
    assert co.single_is_big(("bwd_a", "dec1"), 1027) and not co.single_is_big(("bwd_b", "dec1"), 1027)
    assert not co.single_is_big(("bwd_b", "dec2", "dec3"), 1027) and co.single_is_big(("wgrad", "head_task"), 1027)
    assert len(co.block_twins()) == 5 * 8 + 3 * 4 + 2 * 5


def test_every_row_and_every_twin_has_a_case():
    """FORM -> CASE recomputed from the mirror.  Every row: a value case at each row count the module promises, where
    the mirror selects exactly that row, and a two-plane case; every selectable ``KERNEL_m<KIND, BIG>`` twin of the
    block kernels: a two-plane case.  Every case's expectation is the mirror's."""
    for c in gpu.ALL_CASES:
        assert c.want == co.instance(c.x, c.y, c.rows, c.via != "co"), c.name
    values = [c for c in gpu.VALUE_CASES if not c.opt]
    for i, row in enumerate(co.CO_ROWS):
        hits = {c.rows[0] for c in values if c.row == i and c.want == i}
        want = set(gpu.PLAIN_ROWS) | ({1027} if i in (7, 8, 9, 11) else set()) if row[0] == "plain" else {37, 256, 1027}
        assert hits == want, f"row {i} {row}: value cases select it at {sorted(hits)}, wanted {sorted(want)}"
        if row[0] == "plain":
            two = [c for c in values if c.row == i and c.rows[0] == 1027]
            assert len(two) == 1 and (two[0].want is None) == (i not in (7, 8, 9, 11)), f"row {i} at 1027 rows"
        assert any(c.rows == (37, 40) for c in values if c.row == i), f"row {i}: no case with different grids"
        assert [c for c in gpu.PLANE_CASES if c.row == i and c.want == i], f"row {i} {row}: no two-plane case"
    special = {c.name: c for c in gpu.VALUE_CASES if c.opt}
    assert special["cap_bwd_a_adam"].want in (0, 1) and special["cap_adam_fwd_b"].want in (15, 16)
    assert all(special[n].x[1] == gpu.CAPPED or special[n].y[1] == gpu.CAPPED for n in ("cap_bwd_a_adam", "cap_adam_fwd_b"))
    assert {special[f"head_{n}"].opt["act"] for n in gpu.HEAD_ACTS} == {0, 3, 4} and all(special[f"head_{n}"].want == 17 for n in gpu.HEAD_ACTS)
    assert special["e18@4099"].want == 18 and special["e22@4099"].want == 22 and special["e18@4099"].y[1] == "dec3"
    assert special["head_unal"].want is None and special["head8"].want is None
    def xk(cases):
        rows = [co.CO_ROWS[c.row] for c in cases]
        return {k + ("+wgrad" if k == "bwd_b" and isinstance(cond, tuple) else "") for gate, k, cond, _, _ in rows if gate == "plain"}
    assert xk(gpu.GRAPH_CASES) == xk(gpu.TILE_CASES) == {"bwd_a", "bwd_b+wgrad", "wgrad", "adam", "a"}
    assert sum(co.CO_ROWS[c.row][0] == "entry" for c in gpu.TILE_CASES) == 2
    assert {37, 1023} <= set(gpu.PLAIN_ROWS), "different grids, and the last row count below the gate"
    assert all(c.want == c.row and c.rows == (256, 256) for c in gpu.TILE_CASES) and all(c.want == c.row for c in gpu.GRAPH_CASES)
    have = {(k, co.K_SHAPE[co.shape_k(n)], co.use_big(rows, k, n)) for k, n, rows in gpu.BLOCK_PLANE_CASES}
    missing = co.block_twins() - have
    assert not missing, f"block-kernel twins without a two-plane case: {sorted(missing)}"
    assert have == co.block_twins()
