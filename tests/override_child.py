"""Child process of ``test_tuning_overrides_gpu.py``: ``python override_child.py SET RESULT.json``.

Started with the override set SET in its environment, it loads the library (which reads the overrides, once), runs every
case of the set through the module-level runners of ``test_block_kernels_gpu``, ``test_co_kernels_gpu`` and
``test_loss_kernels_gpu`` -- their references, bounds and assertions, nothing of its own -- catches ``AssertionError`` per
case and writes ``{case: {"ok", "message", "shares"}}``.  The ``ERR`` / ``CMP`` lines of the runners stay on stdout;
``shares`` is the largest share of each bound per quantity class, read off those lines.  Exit status 0 means every case
ran; anything else (an exception that is no failed assertion, a signal) is the parent's to report.  A plain script: not
collected by pytest, not a conftest."""
import contextlib
import io
import json
import os
import re
import sys
import time
import traceback

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.dirname(HERE), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

LINE = re.compile(r"^(ERR|CMP) (.+?): max err .*?([0-9.]+|inf|nan) of the bound(.*)$")


def _class(kind, prefix, rest):
    """The quantity class of a printed comparison: those of ``test_co_kernels_gpu.Rep`` (block quantities) or the
    loss module's own ``[kind]``."""
    if kind == "CMP":
        m = re.search(r"\[(.+)\]", rest)
        return m.group(1) if m else "loss"
    tok = prefix.split(" ")
    what = " ".join(tok[2:] if tok[0] in ("forced", "chained", "eval") else [t for t in tok[1:] if t != "(singles)"])
    return ("running statistics" if "running" in what else "forward sums" if what.startswith("stats") else
            "backward sums" if what.startswith("pairs") else "parameter gradients" if what.startswith("d ") else
            "data gradients" if what.startswith("d") else "forward tensors")


def shares_of(text):
    out = {}
    for line in text.splitlines():
        m = LINE.match(line)
        if not m:
            continue
        kind, prefix, ratio, rest = m.groups()
        v = float(ratio)
        cls = _class(kind, prefix, rest)
        if kind == "ERR" and v > 1.0 and "arbiter" in rest and rest.rstrip().endswith("ok"):
            cls += " (through the fp32 arbiter)"
        out[cls] = max(out.get(cls, 0.0), v)
    return out


def main(name, result_path):
    import test_tuning_overrides_gpu as tu
    env = tu.SETS[name][0]
    # the overrides of this set, and no other, are in the environment BEFORE the library is loaded
    assert all(os.environ.get(k) == v for k, v in env.items()), f"{name}: its overrides are not in the environment"
    others = [k for k in tu.DEFAULTS if k in os.environ and k not in env]
    assert not others, f"{name}: other overrides are set: {others}"
    from rankaae_amd import _lib
    assert _lib._lib is None, "the library was loaded before the overrides were checked"
    _lib.load()
    import torch
    assert torch.cuda.is_available()
    import co_reference as co
    import test_block_kernels_gpu as blocks
    import test_co_kernels_gpu as cok
    import test_loss_kernels_gpu as tk
    from rankaae_amd import ops
    mir = tu.mirror(name)
    mask = mir["big_mask"]
    cok.MASK[0] = mask
    extra = {}

    def forced(n, rows, bn):
        slabs = {}
        counts = blocks.run_teacher_forced(n, rows, gy_bn=bn, slabs_out=slabs)
        geo = tu.geometry(n, rows, mir)
        want = {k: geo[k]["rows"] for k in counts}
        assert counts == want, f"returned row counts {counts}, the mirror gives {want}"
        want = tuple(t["rows"] for t in geo["wgrad"])
        assert slabs["wgrad"] == want, f"weight-gradient slab counts {slabs['wgrad']}, the mirror gives {want}"
        print(f"GEOMETRY {n}@{rows}: " + ", ".join(f"{k} S={geo[k]['S']} rows={geo[k]['rows']}" for k in counts) +
              f", wgrad S={[t['S'] for t in geo['wgrad']]} slabs={list(want)}")

    def planes(kind, n, rows):
        assert co.use_big(rows, kind, n, mask)
        cok._two_planes(f"blk_{kind}_{n}@{rows}", lambda seed: (cok.BlockSide(kind, n, rows, seed),), lambda s: s[0].single())

    def pair_table():
        got, want, rigs, moved = [], [], {}, []
        for row in blocks.CO_TABLE:
            (kx, ax), (ky, ay) = blocks._side(row[0], 1027, rigs), blocks._side(row[1], 1027, rigs)
            got.append(int(ops.co_pairable(kx, ax, ky, ay)))
            want.append(int(co.instance(row[0], row[1], 1027, False, big_mask=mask) is not None))
            print(f"PAIR 1027 rows: {row[0]} + {row[1]}: {got[-1]} (mirror {want[-1]}, default {row[3]})")
            if got[-1] != row[3]:
                moved.append(f"{row[0]} + {row[1]}: {row[3]} -> {got[-1]}")
        extra["moved"] = moved
        assert got == want, f"raae_co_instance {got}, the mirror under {mask} gives {want}"

    def pair(i):
        x, y = co.row_sides(i, cok.WIDE)
        want = co.instance(x, y, (1027, 1027), False, big_mask=mask)
        assert want == i
        c = cok.Case(f"p{i}@1027", "value", i, x, y, (1027, 1027), "co", want, {})
        cok._run_pair(c)

    def disc(n):
        # the library does not say which form it launched (nslab is the same for both): that the forced form ran is
        # shown by the hand mutation check recorded in DESIGN.md, not here
        _, extra["nslab"] = tk.run_disc_fused(n, force=mir["disc_force"])

    def planes_disc(n):
        rep = tk.Report("pl_" + n)
        made = [tk._plane_disc(n)(i) for i in range(2)]
        tk._two_planes(rep, [m[0] for m in made], [m[1] for m in made])
        rep.done()

    run = dict(forced=forced, chained=lambda n, rows, bn: blocks.run_chained(n, rows, gy_bn=bn), first=blocks.run_first_block,
               running=blocks.run_running_statistics, eval=blocks.run_eval_forward, planes=planes, pair_table=pair_table,
               pair=pair, disc=disc, planes_disc=planes_disc)
    results = {}
    t_all = time.perf_counter()
    for case, runner, args in tu.cases(name):
        buf, extra = io.StringIO(), {}
        t0 = time.perf_counter()
        try:
            with contextlib.redirect_stdout(buf):
                run[runner](*args)
            ok, msg = True, ""
        except AssertionError as e:
            ok, msg = False, f"{e}\n{traceback.format_exc(limit=4)}"
        text = buf.getvalue()
        sys.stdout.write(text)
        torch.cuda.synchronize()
        results[case] = dict(ok=ok, message=msg[-4000:], shares=shares_of(text), seconds=round(time.perf_counter() - t0, 2), **extra)
        print(f"CASE {name} {case}: {'ok' if ok else 'FAILED'} in {results[case]['seconds']} s")
    print(f"CHILD {name}: {len(results)} cases in {time.perf_counter() - t_all:.1f} s")
    with open(result_path, "w") as fh:
        json.dump(results, fh)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
