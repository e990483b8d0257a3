"""The kernel instances and launch geometries that only the tuning overrides select (``RAAE_BIG_MASK_*``,
``RAAE_DISC_MFMA``, ``RAAE_WGRAD_GRID``, ``RAAE_WGRAD_S``, ``RAAE_PICK_SMALL``, ``RAAE_PICK_MULT``, ``RAAE_PICK_DIV``) against the
float64 references, bounds and runners of the modules that pin the default dispatch: ``test_block_kernels_gpu.py``,
``test_co_kernels_gpu.py`` and ``test_loss_kernels_gpu.py``.  No tolerance is new and none is widened.

Every override is read once when the library loads, so each OVERRIDE SET runs in a child process of its own
(``override_child.py``) that is started with the set in its environment, runs every case of the set and writes
``{case: {"ok", "message", "shares"}}`` as JSON.  One child per set and session, one at a time (with this process at
most two hold the GPU); the parametrised tests below read the cached result, so a failure names its case.  A child that
ends on a signal, on an exit status other than 0 (all cases ran; failed assertions are in the JSON) or on its time limit
sets ``BROKEN``: every later test of the module fails at once and no further child is started.  Nothing is retried.

SETS gives each set's environment once; ``mirror`` parses the same strings the way the library does (``strtol(., 0)``
for the masks and the weight-gradient knobs, ``atol`` / ``atoi`` for the others) into the arguments of the Python
mirrors (``co_reference`` for the masks, ``conv_reference.pick_S`` for the group sizes, ``loss_reference.disc_instance``
for the discriminator), and ``geometry`` restates the launch geometry of the five block kernels
(``prep_block_*`` of csrc/raae_conv.hip).  ``test_tuning_overrides_cpu.py`` holds names, defaults and conditions to the
sources without a GPU.

FORM -> CASE
  big_all       all five masks 0xff.  The 18 BIG instances the default mask leaves out (enc1, enc2, dec0 everywhere, dec1
                in fwd_a / fwd_b / bwd_b): forced:{shape}@1027 (gy without and behind a BatchNorm), forced:{shape}@4099,
                chained:{shape}@1027, first / running / eval:{enc1, dec1}@1027; forced:dec0@8195 and forced:enc2@16387
                (S = 32: the 16-byte sub-paths of the two shapes with ``Lout`` = 8); their ``_m`` twins planes:{kind}_{shape};
                the control forced:{enc0, dec2, dec3}@1027; pair_table (the library's own word that the mask was read)
  big_none      all five masks 0.  The plain instances at 1027 rows through their own entry points:
                forced:{enc0, dec2, dec3, gen_c}@1027, forced:dec3@4099 (513 groups on 512 workgroups); pair_table;
                pair:p{i}@1027 for every plain row whose answer moved to one launch
  disc_mfma_on  the matrix-core discriminator on partial tiles and tiny batches: disc:dv_*; planes:disc_dv_40_23_6
  disc_mfma_off the VALU discriminator past 256 tiles (its workgroups loop): disc:dm_*
  wgrad_small, wgrad_wide, pick_one, pick_many
                other samples per group / workgroups per task: forced:{seven table shapes, gen_c}@{37, 1027},
                chained:{dec3, enc1}@1027; the returned row and slab counts equal ``geometry``'s
"""
import json
import os
import subprocess
import sys
import tempfile
import time

import pytest

import block_reference as br
import co_reference as co
import conv_reference as cr

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
CHILD = os.path.join(HERE, "override_child.py")

# name -> default, as the sources read them (test_tuning_overrides_cpu.py parses the sources)
MASK_NAMES = tuple("RAAE_BIG_MASK_" + n for n in ("FWD_A", "FWD_B", "BWD_B", "BWD_A", "WGRAD"))
DEFAULTS = dict(zip(MASK_NAMES, co.BIG_MASK), RAAE_WGRAD_GRID=128, RAAE_WGRAD_S=0, RAAE_PICK_SMALL=2200, RAAE_PICK_MULT=8,
                RAAE_PICK_DIV=256, RAAE_DISC_MFMA=-1)

# set -> (environment, time limit of its child in seconds).  The limits are about 3x the measured run of each child on
# an MI355X inside the whole suite (big_all 9.7 s; big_none 6.5-7.3 s; the two discriminator
# sets 2.4 s; the four geometry sets 4.8-5.2 s; about 2.5 s of each is the import of torch and the library, most of the
# rest the float64 references on the CPU), not below 12 s.  All eight children together: 41.1 s.
SETS = {
    "big_all": (dict.fromkeys(MASK_NAMES, "0xff"), 30),
    "big_none": (dict.fromkeys(MASK_NAMES, "0"), 25),
    "disc_mfma_on": ({"RAAE_DISC_MFMA": "1"}, 12),
    "disc_mfma_off": ({"RAAE_DISC_MFMA": "0"}, 12),
    "wgrad_small": ({"RAAE_WGRAD_GRID": "16", "RAAE_WGRAD_S": "1"}, 18),
    "wgrad_wide": ({"RAAE_WGRAD_GRID": "256", "RAAE_WGRAD_S": "3"}, 18),
    "pick_one": ({"RAAE_PICK_SMALL": "0"}, 18),
    "pick_many": ({"RAAE_PICK_DIV": "64", "RAAE_PICK_MULT": "2"}, 18),
}
GEOMETRY_SETS = ("wgrad_small", "wgrad_wide", "pick_one", "pick_many")
NEW_BIG = ("enc1", "enc2", "dec0", "dec1")
# The 16-byte sub-paths of the BIG instances (``vec1``, ``vecA``, the quad ``fwd_b``) need ``S * Lout >= 256``: 32 samples
# per group for dec0 and enc2 (``Lout`` = 8).  With the default ``RAAE_PICK_*`` the host reaches that from 8193 rows (dec0), from
# 7937 (``fwd_b`` of enc2) and by 16384 rows (the other kernels of enc2); at 1027 and 4099 rows they have S = 5 and 16 and
# run the scalar forms.  dec0 at 8195 rows: S = 32 in all four kernels, 257 groups, the last of 3 rows; enc2 at 16387
# rows: S = 32 (64 in ``fwd_b``), 513 groups on 512 workgroups, the last of 3 rows (test_tuning_overrides_cpu.py holds this).
QUAD_ROWS = (("dec0", 8195), ("enc2", 16387))


def mirror(name):
    """The set's environment as the arguments of the mirrors."""
    v = dict(DEFAULTS)
    for k, s in SETS[name][0].items():
        assert k in DEFAULTS, k
        v[k] = int(s, 0) if k.startswith(("RAAE_BIG_MASK_", "RAAE_WGRAD_")) else int(s)
    return dict(big_mask=tuple(v[k] for k in MASK_NAMES), wgrad_grid=v["RAAE_WGRAD_GRID"], wgrad_S=v["RAAE_WGRAD_S"],
                pick=dict(small_floats=v["RAAE_PICK_SMALL"], small_mult=v["RAAE_PICK_MULT"], small_div=v["RAAE_PICK_DIV"]),
                disc_force=v["RAAE_DISC_MFMA"])


# ----------------------------------------------------------------------------------------------- geometry, mirrored
def _conv(m, Lin):
    if m is None:
        return None
    tr = m.__class__.__name__ == "ConvTranspose1d"
    return cr.Conv(m.in_channels, Lin, m.out_channels, m.kernel_size[0], m.stride[0], 0 if tr else m.padding[0],
                   (not tr) and m.padding_mode == "replicate", m.groups, tr)


def block_dims(name):
    """The static description of block ``name`` (``nets_conv.Block``) without the device."""
    m, Lin = br.make_block(name)
    cv1 = _conv(m.conv1, Lin)
    cv2 = _conv(m.conv2, cv1.Lout)
    return dict(Cin=cv1.Cin, Cout=cv1.Cout, Lin=Lin, L1=cv1.Lout, Lout=cv2.Lout, E=m.fc1.out_features, cv1=cv1, cv2=cv2,
                cvs=_conv(m.conv_short, Lin), cve=_conv(m.conv_excit, cv2.Lout), table=name in br.TABLE_SHAPES)


def strip_ok(cv):
    return (not cv.transposed and cv.stride == 1 and cv.groups == 1 and cv.K % 2 == 1 and 3 <= cv.K <= 15 and
            cv.pad == (cv.K - 1) // 2 and cv.Lin == cv.Lout and cv.Lin % 4 == 0 and cv.Lin >= 64)


def _halo(cv):
    return 0 if cv.transposed else (8 if strip_ok(cv) else cv.pad)


def geometry(name, B, mir):
    """kernel -> dict(S, groups, rows = what the launch returns, tile = staged floats, lds = dynamic LDS bytes) for the
    four row-writing block kernels, and "wgrad" -> one such dict per task (``rows`` = its slabs), in the order of
    ``Rig.wgrad_tasks``.  Aligned tensors, ``raae_tile_hint(1)``."""
    d = block_dims(name)
    Cin, Cout, Lin, L1, Lout, E = (d[k] for k in ("Cin", "Cout", "Lin", "L1", "Lout", "E"))
    cv1, cv2, cvs, cve = d["cv1"], d["cv2"], d["cvs"], d["cve"]
    nw = lambda cv: cr.conv_nw(cv) if cv is not None else 0
    pick = lambda per, outs, min_out=256: cr.pick_S(per, outs, B, cr.TILE_BUDGET, min_out, **mir["pick"])

    def one(per, outs, weights):
        S = pick(per, outs)
        groups = cr.cdiv(B, S)
        return dict(S=S, groups=groups, rows=min(groups, cr.MAX_PARTS), tile=S * per, lds=4 * (S * per + weights))
    out = {}
    h = _halo(cv1)
    out["fwd_a"] = one(Cin * (Lin + 2 * h) + Cin * E, max(Cout * L1, Cout * Lout, Cin * Lout),
                       nw(cv1) + nw(cvs) + E * Lin + Lout * E)
    out["fwd_b"] = one(Cout * (L1 + 2 * _halo(cv2)) + (Cin * Lout if cve else 0), Cout * Lout, nw(cv2) + nw(cve))
    gm = 8 if d["table"] and strip_ok(cv2) else 0
    out["bwd_b"] = one(Cout * (Lout + 2 * gm) + (Cout * Lout if cve else 0), max(Cout * Lout, Cout * L1), nw(cv2) + nw(cve))
    gm = 8 if d["table"] and strip_ok(cv1) and cvs is None else 0
    out["bwd_a"] = one(Cout * (L1 + 2 * gm) + Cout * Lout + Cin * Lout + Cin * E, max(Cin * Lin, Cout * L1, Cout * Lout, Cin * Lout),
                       nw(cv1) + nw(cvs) + E * Lin + Lout * E)
    task_grid = max(mir["wgrad_grid"], 16)

    def task(per, S):
        if mir["wgrad_S"] > 0 and B >= cr.BIG_ROWS:
            S = max(1, min(mir["wgrad_S"], (36 * 1024) // per))
        S = min(S, cr.cdiv(B, task_grid))
        groups = cr.cdiv(B, S)
        return dict(S=S, groups=groups, rows=min(groups, task_grid), tile=S * per, lds=4 * S * per)
    tasks = []
    for cv in [cv2, cv1] + ([cve] if cve else []) + ([cvs] if cvs else []):
        per = cv.Cout * cv.Lout + cv.Cin * (cv.Lin + 2 * (0 if cv.transposed else cv.pad))
        tasks.append(task(per, pick(per, cv.Lin if cv.transposed else cv.Lout)))
    for C_, E_, L_ in ((Cin, Lout, E), (Cin, E, Lin)):                  # fc2, fc1
        per = C_ * E_ + C_ * L_
        tasks.append(task(per, pick(per, C_, 64)))
    out["wgrad"] = tasks
    return out


# ------------------------------------------------------------------------------------------------------- case tables
def _forced(n, rows, bn):
    return (f"forced:{n}@{rows}" + (",bn" if bn else ""), "forced", (n, rows, bn))


def moved_pairs(mask):
    """The plain rows of the table whose answer at 1027 rows is another under ``mask`` than under the default:
    [(row, answer under the mask)]."""
    out = []
    for i in range(co.N_PLAIN):
        x, y = co.row_sides(i)
        a, b = co.instance(x, y, 1027, False), co.instance(x, y, 1027, False, mask)
        if (a is None) != (b is None):
            out.append((i, b))
    return out


def cases(name):
    """[(case name, runner, arguments)] of a set, in the order the child runs them."""
    mir = mirror(name)
    if name == "big_all":
        out = []
        for n in NEW_BIG:
            out += [_forced(n, 1027, False), _forced(n, 1027, True), _forced(n, 4099, True), (f"chained:{n}@1027", "chained", (n, 1027, False))]
        out += [_forced(n, rows, True) for n, rows in QUAD_ROWS]
        out += [_forced(n, 1027, True) for n in ("enc0", "dec2", "dec3")]
        for n in ("enc1", "dec1"):
            out += [(f"first:{n}@1027", "first", (n, 1027)), (f"running:{n}@1027", "running", (n, 1027)), (f"eval:{n}@1027", "eval", (n, 1027))]
        out += [(f"planes:{k}_{n}", "planes", (k, n, 1027)) for k in co.FAMILY for n in br.TABLE_SHAPES
                if co.use_big(1027, k, n, mir["big_mask"]) and not co.use_big(1027, k, n)]
        return out + [("pair_table", "pair_table", ())]
    if name == "big_none":
        out = [_forced(n, 1027, True) for n in ("enc0", "dec2", "dec3", "gen_c")] + [_forced("dec3", 4099, True)]
        out.append(("pair_table", "pair_table", ()))
        return out + [(f"pair:p{i}@1027", "pair", (i,)) for i, want in moved_pairs(mir["big_mask"]) if want is not None]
    if name == "disc_mfma_on":
        return [(f"disc:{n}", "disc", (n,)) for n in ("dv_1_1_1", "dv_16_16_16", "dv_40_23_6", "dv_17_15_13_bare", "dv_1000_1047_6")] + \
               [("planes:disc_dv_40_23_6", "planes_disc", ("dv_40_23_6",))]
    if name == "disc_mfma_off":
        return [(f"disc:{n}", "disc", (n,)) for n in ("dm_1000_1048_6", "dm_1_2047_16", "dm_2056_2057_3")]
    assert name in GEOMETRY_SETS
    return [_forced(n, rows, True) for n in list(br.TABLE_SHAPES) + ["gen_c"] for rows in (37, 1027)] + \
           [(f"chained:{n}@1027", "chained", (n, 1027, False)) for n in ("dec3", "enc1")]


ALL = [(s, c[0]) for s in SETS for c in cases(s)]

# ------------------------------------------------------------------------------------------------------- the children
RESULTS = {}                     # set -> {case: {"ok", "message", "shares"}}
WALL = {}
BROKEN = []                      # why no further child is started


def run_set(name):
    if name in RESULTS:
        return RESULTS[name]
    assert not BROKEN, f"no child is started any more: {BROKEN[0]}"
    env, limit = SETS[name]
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "result.json")
        t0 = time.perf_counter()
        try:
            p = subprocess.run([sys.executable, CHILD, name, out], env={**os.environ, **env}, timeout=limit, capture_output=True)
        except subprocess.TimeoutExpired as e:
            print((e.stdout or b"").decode(errors="replace")[-20000:])
            BROKEN.append(f"the child of {name} passed its time limit of {limit} s")
            raise AssertionError(BROKEN[0])
        WALL[name] = time.perf_counter() - t0
        print(p.stdout.decode(errors="replace"))
        if p.returncode != 0 or not os.path.exists(out):
            print(p.stderr.decode(errors="replace")[-20000:])
            BROKEN.append(f"the child of {name} ended with status {p.returncode}")
            raise AssertionError(BROKEN[0])
        with open(out) as fh:
            RESULTS[name] = json.load(fh)
    print(f"WALL {name}: {WALL[name]:.1f} s")
    return RESULTS[name]


@pytest.mark.parametrize("name,case", ALL, ids=[f"{s}-{c}" for s, c in ALL])
def test_override_case(name, case):
    res = run_set(name)
    assert case in res, f"the child of {name} did not report {case}"
    assert res[case]["ok"], res[case]["message"]


def test_the_mask_was_read():
    """Under ``big_all`` and under ``big_none`` at least one answer of the pair table differs from the default column,
    and the library's answers are the mirror's (asserted by the pair_table cases): the child reports which moved."""
    for name in ("big_all", "big_none"):
        moved = run_set(name)["pair_table"].get("moved", [])
        print(f"MOVED {name}: {moved}")
        assert moved, f"{name}: no answer of the pair table differs from the default"


def test_zz_shares_and_times():
    """Printed last: the largest share of each bound per quantity class and set, and the children's wall times."""
    for name, res in RESULTS.items():
        worst = {}
        for r in res.values():
            for k, v in r.get("shares", {}).items():
                worst[k] = max(worst.get(k, 0.0), v)
        for k in sorted(worst):
            print(f"SHARE {name} {k}: {worst[k]:.3f}")
            assert worst[k] <= 1.0 or "arbiter" in k, (name, k, worst[k])
    for name, w in WALL.items():
        print(f"WALL {name}: {w:.1f} s of {SETS[name][1]} s")
    print(f"WALL all children: {sum(WALL.values()):.1f} s")
