"""The table of two-body launches (``co_pair`` of ``rankaae_amd/csrc/raae_conv.hip``) restated as data, with the gate
``co_prep`` computes in front of it.  ``test_co_reference_cpu.py`` holds it row for row to the ``RAAE_CO(`` lines of the
kernel file and to the answers recorded in ``CO_TABLE`` of ``test_block_kernels_gpu.py``; ``test_co_kernels_gpu.py``
takes from it how many launches a pair must be.  Not a conftest: tests import it.

A SIDE is written as the tests already write it (``CO_TABLE``):

  ("a" | "b" | "bwd_a" | "wgrad", shape)    a block kernel on a block shape, ``enc0 .. dec3`` (k = 0 .. 6) or a generic
                                            one (``gen_*`` / "generic", k = -1)
  ("bwd_b", shape)                          backward phase B alone: a side of ``raae_block_bwd_b_wgrad`` only
  ("bwd_b", shape, shape of the tasks)      RAAE_CO_BWD_B_WGRAD: phase B with the next block's weight-gradient tasks
  ("adam", max_nslab, checked)              an Adam / AdamW update; the wide (8-lane) kernel above 16 slabs
  ("head", channels[, out aligned])         the decoder's head conv

A ROW is (gate, x kind, x condition, y kind, y condition): the condition of a block side is its shape name, of
RAAE_CO_BWD_B_WGRAD the two names, of an update (wide, checked), of the head its channel count; "any" = ``true``.
The first matching row wins.
"""
SHAPE_K = {"enc0": 0, "enc1": 1, "enc2": 2, "dec0": 3, "dec1": 4, "dec2": 5, "dec3": 6}
K_SHAPE = {k: n for n, k in SHAPE_K.items()}
K_SHAPE[-1] = "generic"
BIG_ROWS = 1024
FAMILY = {"a": 0, "b": 1, "bwd_b": 2, "bwd_a": 3, "wgrad": 4}                 # kFamFwdA .. kFamWgrad
BIG_MASK = (0xe1, 0xe1, 0xe1, 0xf1, 0xf1)                                      # kBigMask: bit k = shape k, bit 7 = generic
WIDE_ABOVE = 16                                                                # s.wide = max_nslab > 16

CO_ROWS = [
    ("plain", "bwd_a", "dec3", "adam", (True, True)),
    ("plain", "bwd_a", "dec3", "adam", (True, False)),
    ("plain", "bwd_b", ("dec2", "dec3"), "a", "enc0"),
    ("plain", "bwd_a", "dec2", "b", "enc0"),
    ("plain", "bwd_b", ("dec1", "dec2"), "a", "enc1"),
    ("plain", "bwd_a", "dec1", "b", "enc1"),
    ("plain", "bwd_b", ("dec0", "dec1"), "a", "enc2"),
    ("plain", "bwd_a", "dec0", "b", "enc2"),
    ("plain", "bwd_a", "enc2", "adam", (True, True)),
    ("plain", "bwd_a", "enc2", "adam", (True, False)),
    ("plain", "bwd_b", ("enc1", "enc2"), "a", "dec0"),
    ("plain", "bwd_a", "enc1", "b", "dec0"),
    ("plain", "bwd_b", ("enc0", "enc1"), "a", "dec1"),
    ("plain", "bwd_a", "enc0", "b", "dec1"),
    ("plain", "wgrad", "enc0", "a", "dec2"),
    ("plain", "adam", (True, True), "b", "dec2"),
    ("plain", "adam", (True, False), "b", "dec2"),
    ("plain", "a", "enc1", "head", 4),
    ("entry", "a", "enc0", "a", "dec3"),
    ("entry", "a", "enc0", "a", "dec0"),
    ("entry", "a", "enc1", "a", "dec1"),
    ("entry", "a", "enc2", "a", "dec2"),
    ("entry", "b", "enc0", "b", "dec3"),
    ("entry", "b", "enc0", "b", "dec0"),
    ("entry", "b", "enc1", "b", "dec1"),
    ("entry", "b", "enc2", "b", "dec2"),
    ("entry", "bwd_b", "enc0", "wgrad", "enc1"),
    ("entry", "bwd_b", "enc1", "wgrad", "enc2"),
    ("entry", "bwd_b", "dec0", "wgrad", "dec1"),
    ("entry", "bwd_b", "dec1", "wgrad", "dec2"),
    ("entry", "bwd_b", "dec2", "wgrad", "dec3"),
    ("entry", "bwd_b", "enc2", "wgrad", "dec0"),
    ("entry", "bwd_b", "dec3", "wgrad", "enc0"),
    ("entry", "bwd_b", "dec3", "wgrad", "generic"),
    ("entry", "bwd_b", "any", "wgrad", "any"),
]
N_PLAIN = sum(1 for r in CO_ROWS if r[0] == "plain")


def shape_k(name):
    return SHAPE_K.get(name, -1)


def use_big(rows, kind, shape, big_mask=BIG_MASK):
    """Whether the block kernel ``kind`` runs its large-batch (BIG) instance alone on ``shape`` at ``rows`` rows."""
    k = shape_k(shape)
    return rows >= BIG_ROWS and bool((big_mask[FAMILY[kind]] >> (7 if k < 0 else k)) & 1)


def side(spec, rows, big_mask=BIG_MASK):
    """``co_prep``'s view of a side: (kind, condition value, big, large).  A head whose shape or output alignment the
    head kernel does not take has no channel count (``None``) and is never ``large``."""
    kind = spec[0]
    if kind == "adam":
        return kind, (spec[1] > WIDE_ABOVE, bool(spec[2])), False, False
    if kind == "head":
        ok = spec[1] in (4, 8) and (len(spec) < 3 or bool(spec[2]))
        return kind, (spec[1] if ok else None), False, ok and rows >= BIG_ROWS
    if kind == "bwd_b" and len(spec) == 3:
        return kind, (K_SHAPE[shape_k(spec[1])], K_SHAPE[shape_k(spec[2])]), False, rows >= BIG_ROWS
    return kind, K_SHAPE[shape_k(spec[1])], use_big(rows, kind, spec[1], big_mask), False


def _matches(kind, cond, skind, sval):
    if kind != skind or isinstance(cond, tuple) != isinstance(sval, tuple):
        return False             # (phase B alone and RAAE_CO_BWD_B_WGRAD are different kinds of the kernel file)
    return cond == "any" or cond == sval


def instance(x, y, rows, entry, big_mask=BIG_MASK):
    """The index of the row of ``CO_ROWS`` that runs the pair as ONE launch, or ``None`` (two launches, x first).
    ``rows``: the row count of both sides, or (x rows, y rows); ``entry``: through ``raae_block_fwd_a2`` / ``_b2`` /
    ``_bwd_b_wgrad`` rather than ``raae_co_launch``."""
    rx, ry = rows if isinstance(rows, tuple) else (rows, rows)
    kx, vx, bx, lx = side(x, rx, big_mask)
    ky, vy, by, ly = side(y, ry, big_mask)
    gates = {"plain": not (bx or lx or by or ly), "entry": bool(entry)}
    for i, (gate, rkx, cx, rky, cy) in enumerate(CO_ROWS):
        if gates[gate] and _matches(rkx, cx, kx, vx) and _matches(rky, cy, ky, vy):
            return i
    return None


def single_is_big(spec, rows, big_mask=BIG_MASK):
    """Whether the side's OWN entry point runs a BIG instance at ``rows`` rows.  RAAE_CO_BWD_B_WGRAD alone is the pair
    ``raae_block_bwd_b_wgrad`` launches, an ``entry`` row: plain bodies at every row count."""
    if spec[0] in ("adam", "head") or (spec[0] == "bwd_b" and len(spec) == 3):
        return False
    return use_big(rows, spec[0], spec[1], big_mask)


def row_sides(i, max_nslab=40):
    """Row ``i`` as the (x, y) side tuples of ``CO_TABLE``; "any" becomes the generic shape ``gen_c`` / ``gen_b`` and
    "generic" the lone head-conv task (``head_task``)."""
    _, kx, cx, ky, cy = CO_ROWS[i]

    def one(kind, cond, generic):
        if kind == "adam":
            return (kind, max_nslab, cond[1])
        if kind == "head":
            return (kind, cond)
        if isinstance(cond, tuple):
            return (kind,) + cond
        return (kind, {"any": generic, "generic": "head_task"}.get(cond, cond))
    return one(kx, cx, "gen_c"), one(ky, cy, "gen_b")


# every KERNEL_m<KIND, BIG> twin of the five block kernels that the default dispatch can select
def block_twins(big_mask=BIG_MASK):
    """{(kind, shape name, big)}: the plain twin of every table shape and of the generic instance, and the BIG twin
    wherever ``big_mask`` sends 1024 rows and more to it (such a shape still runs its plain one below 1024 rows)."""
    out = set()
    for kind in FAMILY:
        for name in list(SHAPE_K) + ["generic"]:
            out.add((kind, name, False))
            if use_big(BIG_ROWS, kind, name, big_mask):
                out.add((kind, name, True))
    return out
