"""Missing descriptors (NaN AUX cells) under data parallelism: two real ranks (two fresh processes on the one GPU over
gloo, started as ``tests/test_dp_gpu.py`` starts its ranks) train with ``rank_loss_pairs: global`` and validate with the
sharded rank loss on the ``fc_small`` fixture with 30 % of its AUX cells NaN.  The rank loss is held against the float64
definition on the gathered batch (``partial_label_reference.masked_rank_loss``) to the tolerances of
``tests/test_partial_labels_gpu.py`` (loss 1e-5 relative + 1e-7, gradient 1e-5 relative + 1e-9); the captured step
against the eager one bit for bit; and the paths that must not change are read off the engine's sequence of entry points."""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

WORKER_SECONDS = 240        # a worker that has not finished by then is killed (SIGALRM) and the test fails


def _free_port():
    import socket
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        return sk.getsockname()[1]


def _begin(rank, world, port):
    import datetime
    import signal
    import torch.distributed as dist
    signal.alarm(WORKER_SECONDS)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=WORKER_SECONDS))
    torch.set_num_threads(1)
    return dist


def _end(dist):
    torch.cuda.synchronize()
    dist.barrier()
    dist.destroy_process_group()


def _data(world, frac=0.3, **over):
    """The fixture with ``frac`` of the AUX cells NaN (fixed seed); its batch is the GLOBAL batch here."""
    import numpy as np
    import test_engine_gpu as T
    from oracle import ref_train
    g, cfg, spec, aux = T.load_case("fc_small")
    if frac:
        aux = aux.copy()
        aux[np.random.default_rng(11).random(aux.shape) < frac] = np.nan
    cfg = dict(cfg, rank_loss_pairs="global", **over)
    cfg["batch_size"] = cfg["batch_size"] // world
    n_train, n_val, _ = ref_train.split_rows(len(spec))
    return g, cfg, spec, aux, n_train, n_val


def _engine(g, cfg, spec, aux, n_train, rank, world, use_graph):
    import test_engine_gpu as T
    from rankaae_amd import model as pm
    from rankaae_amd.engine import StepEngine
    torch.manual_seed(g["model_seed"])
    cls = pm.AE_CLS_DICT[cfg["ae_form"]]
    enc = cls["encoder"](nstyle=cfg["nstyle"], dropout_rate=cfg["dropout_rate"], dim_in=cfg["dim_in"], n_layers=cfg["n_layers"])
    dec = cls["decoder"](nstyle=cfg["nstyle"], dropout_rate=cfg["dropout_rate"], last_layer_activation=cfg["decoder_activation"],
                         dim_out=cfg["dim_out"], n_layers=cfg["n_layers"])
    dis = pm.DiscriminatorFC(nstyle=cfg["nstyle"], dropout_rate=cfg["dis_dropout_rate"], noise=cfg["dis_noise"],
                             layers=cfg["FC_discriminator_layers"])
    eng = StepEngine(enc, dec, dis, cfg, T.DEV, rng_mode="philox", seed=21, use_graph=use_graph, world_size=world, rank=rank)
    eng.set_data(spec[:n_train], aux[:n_train])             # the parent commit refuses this with a ValueError
    b = cfg["batch_size"]
    eng.set_epoch(torch.randperm(n_train, generator=torch.Generator().manual_seed(11)), 0.3, start=rank * b, stride=world * b)
    return eng


def _entry_points(ops, fn):
    """The ``ops`` entry points ``fn()`` goes through, in order (``test_partial_labels_gpu._entry_points``, here in a
    child process of its own)."""
    import types
    log, saved = [], {}
    for name, f in list(vars(ops).items()):
        if isinstance(f, types.FunctionType) and not name.startswith("_") and f.__module__ == ops.__name__:
            saved[name] = f
            setattr(ops, name, (lambda n, f_: lambda *a, **k: (log.append(n), f_(*a, **k))[1])(name, f))
    try:
        fn()
    finally:
        for name, f in saved.items():
            setattr(ops, name, f)
    return [n for n in log if not n.endswith("_bytes")]       # launches only: buffer-size queries launch nothing


def _spawn(worker, *args):
    import torch.multiprocessing as mp
    mp.spawn(worker, args=(2, _free_port()) + args, nprocs=2, join=True)


# ------------------------------------------------------------------------------------------------ eager step
def _eager_worker(rank, world, port):
    import numpy as np
    from partial_label_reference import masked_rank_loss
    dist = _begin(rank, world, port)
    g, cfg, spec, aux, n_train, _ = _data(world)
    eng = _engine(g, cfg, spec, aux, n_train, rank, world, use_graph=False)
    assert eng.aux_missing and eng.rank_pairs_global
    b, K, seen = cfg["batch_size"], cfg["n_aux"], {}

    def hook(name, P):
        if name == "correlation":       # phase B's buffers before later phases reuse them
            seen.update(aux_all=P.aux_all.cpu().numpy(), z_all=P.z_all.cpu().numpy(), dstyles=P.dstyles.cpu().double().numpy(),
                        loss=float(eng.loss_out[1]))
    eng.phase_hook = hook
    eng.step(b)
    torch.cuda.synchronize()
    d, z = seen["aux_all"], seen["z_all"]
    assert d.shape == (world * b, K) and 0.2 < np.isnan(d).mean() < 0.4
    lref, gref = masked_rank_loss(d, z[:, :K], cfg["kendall_activation"])
    loss = seen["loss"]
    print(f"rank {rank}: loss {loss!r} reference {lref!r}")
    assert loss == eng.losses()["kendall"]
    assert abs(loss - lref) <= 1e-5 * abs(lref) + 1e-7, (loss, lref)
    box = [None] * world
    dist.all_gather_object(box, np.float32(loss).tobytes())
    assert box[0] == box[1], "the ranks' losses differ"
    got, want = seen["dstyles"][:, :K], world * gref[rank * b:(rank + 1) * b]
    err, tol = np.abs(got - want), 1e-9 + 1e-5 * np.abs(want)
    print(f"rank {rank}: dstyles max |err| {err.max():.3e}, max err / tol {np.max(err / tol):.3f}")
    assert np.all(err <= tol)
    mine = d[rank * b:(rank + 1) * b]
    assert np.all(got[~np.isfinite(mine)] == 0.0) and np.all(seen["dstyles"][:, K:] == 0.0) and not np.isnan(seen["dstyles"]).any()
    _end(dist)


def test_global_pairs_step_is_the_float64_loss_of_the_gathered_batch():
    _spawn(_eager_worker)


# ------------------------------------------------------------------------------------------------ captured step
def _graph_worker(rank, world, port, in_graph):
    dist = _begin(rank, world, port)
    g, cfg, spec, aux, n_train, _ = _data(world, in_graph_allreduce=in_graph)
    b, out = cfg["batch_size"], []
    for use_graph in (False, True):
        eng = _engine(g, cfg, spec, aux, n_train, rank, world, use_graph)
        losses = []
        for _ in range(3):              # graph mode: eager emission, capture, replay
            eng.step(b)
            losses.append(eng.losses())
        torch.cuda.synchronize()
        out.append((losses, eng.arena.P.clone()))
        if use_graph:
            items = eng.plans[b].graphs[True]
            assert items is not None
            cuts = sum(1 for it in items if not hasattr(it, "launch"))
            if eng.graph_ar is None:
                # the graph is cut at the collectives: five gradient means, and the rank loss's two gathers and its sum
                assert cuts == 8, (cuts, len(items))
            else:
                assert cuts == 0 and len(items) == 1
        eng.close()
    assert out[0][0] == out[1][0], (out[0][0], out[1][0])
    assert torch.equal(out[0][1], out[1][1]), "captured and eager steps end at different parameters"
    assert all(v == v for step in out[1][0] for v in step.values())
    _end(dist)


@pytest.mark.parametrize("in_graph", [True, False])
def test_captured_global_pairs_step_is_bitwise_the_eager_one(in_graph):
    _spawn(_graph_worker, in_graph)


# ------------------------------------------------------------------------------------------------ validation
def _validation_worker(rank, world, port):
    import numpy as np
    from partial_label_reference import masked_rank_loss
    from rankaae_amd import ops
    dist = _begin(rank, world, port)
    g, cfg, spec, aux, n_train, n_val = _data(world)
    eng = _engine(g, cfg, spec, aux, n_train, rank, world, use_graph=False)
    import test_engine_gpu as T
    nv = n_val - (1 - n_val % 2)          # an odd number of rows: the two shards differ in size
    vs = torch.tensor(spec[n_train:n_train + nv], dtype=torch.float32, device=T.DEV)
    va = torch.tensor(aux[n_train:n_train + nv], dtype=torch.float32, device=T.DEV)
    assert torch.isnan(va).any()
    K, vals, logs = cfg["n_aux"], {}, {}
    for shard in (False, True):
        eng.cfg["shard_validation"] = shard

        def run():
            z, losses = eng.validate(vs, va)
            vals[shard] = (z.cpu().double().numpy(), losses["kendall"])
        logs[shard] = _entry_points(ops, run)
    assert np.array_equal(vals[False][0], vals[True][0])
    lref, _ = masked_rank_loss(va.cpu().numpy(), vals[True][0][:, :K], cfg["kendall_activation"])
    rep, sh = vals[False][1], vals[True][1]
    print(f"rank {rank}: Val_Aux sharded {sh!r} replicated {rep!r} reference {lref!r}")
    assert abs(sh - rep) <= 1e-5 * abs(rep) + 1e-7
    assert abs(sh - lref) <= 1e-5 * abs(lref) + 1e-7 and abs(rep - lref) <= 1e-5 * abs(lref) + 1e-7
    box = [None] * world
    dist.all_gather_object(box, sh)
    assert box[0] == box[1], "the ranks' sharded validation losses differ"
    assert logs[True].count("rank_rows_masked_pairs") == 1 and logs[True].count("rank_rows_masked_finish") == 1
    assert "rank_loss_masked_fwd_bwd" not in logs[True]
    assert logs[False].count("rank_loss_masked_fwd_bwd") == 1 and not [n for n in logs[False] if n.startswith("rank_rows")]
    _end(dist)


def test_sharded_validation_on_missing_labels_equals_replicated():
    _spawn(_validation_worker)


# ------------------------------------------------------------------------------------------------ unchanged paths
def _paths_worker(rank, world, port):
    from rankaae_amd import ops
    dist = _begin(rank, world, port)
    logs = {}
    for frac, pairs in ((0.0, "global"), (0.3, "local"), (0.3, "global")):
        g, cfg, spec, aux, n_train, _ = _data(world, frac)
        cfg["rank_loss_pairs"] = pairs
        eng = _engine(g, cfg, spec, aux, n_train, rank, world, use_graph=False)
        assert eng.aux_missing == bool(frac)
        logs[frac, pairs] = _entry_points(ops, lambda: eng.step(cfg["batch_size"]))
        torch.cuda.synchronize()
    full = logs[0.0, "global"]
    assert not [n for n in full if "masked" in n]
    assert [n for n in full if n.startswith("rank_")] == ["rank_rows_pairs", "rank_rows_finish"]
    local = logs[0.3, "local"]
    assert [n for n in local if n.startswith("rank_")] == ["rank_loss_masked_fwd_bwd"]
    # masked data with global pairs: the fully labelled sequence with the masked pair in place of the unmasked one
    assert [n.replace("_masked", "") for n in logs[0.3, "global"]] == full
    assert [n for n in logs[0.3, "global"] if n.startswith("rank_")] == ["rank_rows_masked_pairs", "rank_rows_masked_finish"]
    _end(dist)


def test_fully_labelled_and_local_pairs_launch_what_they_launched():
    _spawn(_paths_worker)
