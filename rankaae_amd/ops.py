"""Thin Python wrappers over the C ABI: torch tensors in (device memory + current stream
only -- PyTorch is plumbing here), HIP kernels underneath.  No fallback paths.
"""
import ctypes as C

import torch

from . import _lib
from ._lib import BnT, check


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t, dtype=torch.float32):
    if t is None:
        return None
    if isinstance(t, int):
        return C.c_void_p(t)
    assert t.is_cuda and t.is_contiguous(), "device, contiguous tensors only"
    if dtype is not None:
        assert t.dtype == dtype, (t.dtype, dtype)
    return C.c_void_p(t.data_ptr())


def make_bn(partials=None, nparts=0, count=0.0, running_mean=None, running_var=None, momentum=0.1, eps=1e-5,
            update_running=False):
    """Build a ``raae_bn_t``.  ``partials=None`` selects eval mode (running statistics)."""
    bn = BnT()
    bn.partials = partials.data_ptr() if partials is not None else None
    bn.nparts = int(nparts)
    bn.count = float(count)
    bn.running_mean = running_mean.data_ptr() if running_mean is not None else None
    bn.running_var = running_var.data_ptr() if running_var is not None else None
    bn.momentum = float(momentum)
    bn.eps = float(eps)
    bn.update_running = 1 if update_running else 0
    return bn


def _bnp(bn):
    return C.byref(bn) if bn is not None else None


def dense_fwd(x, B, K, in_kind, slope, bn, mask, w, bias, N, z, out_kind, out_slope=None, out_partials=None):
    def launch():
        n = C.c_int(0)
        check(_lib.load().raae_dense_fwd(_ptr(x), B, K, in_kind, _ptr(slope), _bnp(bn), _ptr(mask), _ptr(w), _ptr(bias),
                                         N, _ptr(z), out_kind, _ptr(out_slope), _ptr(out_partials, torch.float64),
                                         C.byref(n), _stream()), "raae_dense_fwd")
        return n.value
    return _probed("dense_fwd_kernel", 4 * (B * K * (2 if mask is not None else 1) + N * K + N + B * N), launch)


def make_gen(gen):
    """``raae_maskgen_t`` from ``(state tensor [counter, seed, keys], slot offset, keep)`` or None (disabled): the
    step's hash keys live in the third 8-byte word of the engine's state; threshold and multiplier are formed here
    exactly as ``raae_rng_fill`` forms them from the float keep probability."""
    import numpy as np
    g = _lib.MaskGenT()
    if gen is not None:
        state, off, keep = gen
        assert state.dtype == torch.int64 and state.is_cuda and state.numel() >= 3 and 0 <= off < 2 ** 32 and 0.0 < keep <= 1.0
        k32 = np.float32(keep)
        g.keys, g.offset = state.data_ptr() + 16, int(off)
        g.thr = min(0xFFFFFFFF, int(float(k32) * 4294967296.0))
        g.inv = float(np.float32(1.0) / k32)
    return g


def dense_fwd_args(x, B, K, in_kind, slope, bn, mask, w, bias, N, z, out_kind, out_slope=None, out_partials=None,
                   storage=0, mask_scale=1.0, gen=None):
    """``raae_dense_fwd_t`` holding the arguments of ``dense_fwd`` (for ``dense_fwd_pair``).  ``storage``: RAAE_ST_*
    bits -- which of x / mask / z are bf16 tensors.  ``gen``: the layer's dropout multipliers are generated in the
    kernel (``make_gen``) instead of read from ``mask``; ``mask_scale``: what a bf16 {0, 1} mask is multiplied by."""
    a = _lib.DenseFwdT()
    a.storage = int(storage)
    a.mask_scale = float(mask_scale)
    a.gen = make_gen(gen)
    assert mask is None or gen is None
    a.x, a.B, a.K, a.in_kind, a.slope = _ptr(x, None), B, K, in_kind, _ptr(slope)
    a.has_bn = 0 if bn is None else 1
    if bn is not None:
        a.bn = bn
    a.mask, a.w, a.bias, a.N, a.z = _ptr(mask, None), _ptr(w), _ptr(bias), N, _ptr(z, None)
    a.out_kind, a.out_slope, a.out_partials = out_kind, _ptr(out_slope), _ptr(out_partials, torch.float64)
    for t, bit in ((x, _lib.ST_X), (mask, _lib.ST_MASK), (z, _lib.ST_Z)):      # the dtype of each tensor must match its bit
        assert t is None or t.dtype == (torch.bfloat16 if storage & bit else torch.float32), (t.dtype, storage, bit)
    return a


def dense_fwd_bytes(a):
    """Algorithmic bytes of a fused dense layer: input (and its dropout mask) read once, weights and bias once,
    output written once."""
    bx, bm, bz = (2 if a.storage & 1 else 4), (2 if a.storage & 2 else 4), (2 if a.storage & 4 else 4)
    # (dropout multipliers generated in the kernel are not bytes: only a mask TENSOR counts)
    return a.B * a.K * (bx + (bm if a.mask else 0)) + 4 * (a.N * a.K + a.N) + bz * a.B * a.N


def dense_fwd_struct(a):
    """``dense_fwd`` from a ``raae_dense_fwd_t``."""
    def launch():
        n = C.c_int(0)
        check(_lib.load().raae_dense_fwd_s(C.byref(a), C.byref(n), _stream()), "raae_dense_fwd_s")
        return n.value
    return _probed("dense_fwd_kernel", dense_fwd_bytes(a), launch)


def dense_fwd_pair(p, q):
    """Two independent dense layers in one launch; returns both partial-row counts."""
    def launch():
        n1, n2 = C.c_int(0), C.c_int(0)
        check(_lib.load().raae_dense_fwd2(C.byref(p), C.byref(q), C.byref(n1), C.byref(n2), _stream()), "raae_dense_fwd2")
        return n1.value, n2.value
    return _probed("dense_fwd2_kernel", dense_fwd_bytes(p) + dense_fwd_bytes(q), launch)


def disc_fused(z_real, styles, noise, sigma, mask1, mask2, layers, alpha, n_real, n_fake, ns, gslab, slab_stride,
               dstyles, partial, ticket, loss):
    """The adversarial branch in one launch (``raae_disc_fused``); ``layers``: the three dense layers of the
    discriminator (``w``, ``b``, ``prelu``); returns the slab count of the parameter gradients."""
    l1, l2, l3 = layers
    a = _lib.DiscFusedT()
    a.z_real, a.styles, a.noise, a.sigma = z_real.data_ptr(), styles.data_ptr(), _p(noise), float(sigma)
    a.mask1, a.mask2 = _p(mask1), _p(mask2)
    a.w1, a.b1, a.s1 = l1.w.data_ptr(), l1.b.data_ptr(), l1.prelu.weight.data_ptr()
    a.w2, a.b2, a.s2 = l2.w.data_ptr(), l2.b.data_ptr(), l2.prelu.weight.data_ptr()
    a.w3, a.b3, a.alpha = l3.w.data_ptr(), l3.b.data_ptr(), alpha.data_ptr()
    a.n_real, a.n_fake, a.ns, a.hidden = n_real, n_fake, ns, l1.N
    a.dw1, a.db1, a.ds1 = gslab(l1.w).data_ptr(), gslab(l1.b).data_ptr(), gslab(l1.prelu.weight).data_ptr()
    a.dw2, a.db2, a.ds2 = gslab(l2.w).data_ptr(), gslab(l2.b).data_ptr(), gslab(l2.prelu.weight).data_ptr()
    a.dw3, a.db3 = gslab(l3.w).data_ptr(), gslab(l3.b).data_ptr()
    a.slab_stride = slab_stride
    a.dstyles, a.partial, a.ticket, a.loss = dstyles.data_ptr(), partial.data_ptr(), ticket.data_ptr(), loss.data_ptr()
    def launch():
        n = C.c_int(0)
        check(_lib.load().raae_disc_fused(C.byref(a), C.byref(n), _stream()), "raae_disc_fused")
        return n.value
    rows = n_real + n_fake
    nmask = (1 if mask1 is not None else 0) + (1 if mask2 is not None else 0)
    # z_real / styles (+ noise) read, masks read, dstyles written, weights read + one gradient slab written per workgroup
    nbytes = 4 * (rows * ns * (2 if noise is not None else 1) + rows * l1.N * nmask + n_fake * ns +
                  2 * (l1.w.numel() + l2.w.numel() + l3.w.numel() + 3 * l1.N + 1))
    return _probed("disc_fused_kernel", nbytes, launch)


def dense_bwd(g, g_kind, g_partials, g_nparts, zout, out_slope, out_bn, B, N, x, K, in_kind, slope, bn, mask, w,
              dw, db, dslope, slab_stride, dx=None, dx_partials=None, storage=0, mask_scale=1.0, gen=None):
    for t, bit in ((x, _lib.ST_X), (mask, _lib.ST_MASK), (zout, _lib.ST_Z)):
        assert t is None or t.dtype == (torch.bfloat16 if storage & bit else torch.float32), (t.dtype, storage, bit)
    assert mask is None or gen is None
    a = _lib.DenseBwdT()
    a.g, a.g_kind, a.g_partials, a.g_nparts = _p(g), g_kind, _p(g_partials), int(g_nparts)
    a.zout, a.out_slope = _p(zout), _p(out_slope)
    a.has_out_bn = 0 if out_bn is None else 1
    if out_bn is not None:
        a.out_bn = out_bn
    a.B, a.N, a.x, a.K, a.in_kind, a.slope = B, N, _p(x), K, in_kind, _p(slope)
    a.has_bn = 0 if bn is None else 1
    if bn is not None:
        a.bn = bn
    a.mask, a.w, a.dw, a.db, a.dslope, a.slab_stride = _p(mask), _p(w), _p(dw), _p(db), _p(dslope), slab_stride
    a.dx, a.dx_partials, a.storage, a.mask_scale = _p(dx), _p(dx_partials), int(storage), float(mask_scale)
    a.gen = make_gen(gen)

    def launch():
        n = C.c_int(0)
        check(_lib.load().raae_dense_bwd_s(C.byref(a), C.byref(n), _stream()), "raae_dense_bwd_s")
        return n.value
    # output gradient and raw output read, input (+ mask tensor) read, input gradient written, weights read, one slab written
    nbytes = 4 * (B * N * (2 if zout is not None else 1) + B * K * (2 if mask is not None else 1) +
                  (B * K if dx is not None else 0) + 2 * N * K + 2 * N)
    return _probed("dense_bwd_kernel", nbytes, launch)


def tile_hint(mult):
    """Thread-local launch-geometry hint of the conv-network entry points (``raae_tile_hint``)."""
    check(_lib.load().raae_tile_hint(int(mult)), "raae_tile_hint")


def style_bn_fwd(z, B, Cc, bn, styles):
    check(_lib.load().raae_style_bn_fwd(_ptr(z), B, Cc, _bnp(bn), _ptr(styles), _stream()), "raae_style_bn_fwd")


def style_bn_bwd(dstyles, styles, B, Cc, bn, dz, scale=1.0):
    check(_lib.load().raae_style_bn_bwd(_ptr(dstyles), _ptr(styles), B, Cc, _bnp(bn), scale, _ptr(dz), _stream()),
          "raae_style_bn_bwd")


def rank_loss_work_bytes(B, n_aux):
    return int(_lib.load().raae_rank_loss_work_bytes(B, n_aux))


def rank_loss_fwd_bwd(d, ldd, z, ldz, B, n_aux, activate, work, loss, dz):
    def launch():
        check(_lib.load().raae_rank_loss_fwd_bwd(_ptr(d), ldd, _ptr(z), ldz, B, n_aux, 1 if activate else 0,
                                                 _ptr(work, None), _ptr(loss), _ptr(dz), _stream()),
              "raae_rank_loss_fwd_bwd")
    _probed("rank_pairs_kernel", 4 * B * n_aux * 3, launch)      # O(B) bytes for B^2 n_aux pair operations: VALU-bound


def rank_loss_masked_work_bytes(B, n_aux):
    return int(_lib.load().raae_rank_loss_masked_work_bytes(B, n_aux))


def rank_loss_masked_fwd_bwd(d, ldd, z, ldz, B, n_aux, activate, work, loss, dz):
    """The rank loss where NaN cells of ``d`` are missing labels (``raae_rank_loss_masked_fwd_bwd``)."""
    def launch():
        check(_lib.load().raae_rank_loss_masked_fwd_bwd(_ptr(d), ldd, _ptr(z), ldz, B, n_aux, 1 if activate else 0,
                                                        _ptr(work, None), _ptr(loss), _ptr(dz), _stream()),
              "raae_rank_loss_masked_fwd_bwd")
    _probed("rank_pairs_masked_kernel", 4 * B * n_aux * 3, launch)


def rank_logistic_work_bytes(B, n_aux):
    return int(_lib.load().raae_rank_logistic_work_bytes(B, n_aux))


def rank_logistic_fwd_bwd(d, ldd, z, ldz, B, n_aux, temperature, work, loss, dz, lddz):
    """The pairwise logistic rank loss (``raae_rank_logistic_fwd_bwd``): ``loss[0]`` and ``dz [B, lddz]`` (overwritten)
    from the descriptors ``d`` (NaN cells are missing labels) and the styles ``z``; ``work`` a byte buffer of
    ``rank_logistic_work_bytes``.  Two launches; no host synchronisation."""
    def launch():
        check(_lib.load().raae_rank_logistic_fwd_bwd(_ptr(d), ldd, _ptr(z), ldz, B, n_aux, float(temperature),
                                                     _ptr(work, None), _ptr(loss), _ptr(dz), lddz, _stream()),
              "raae_rank_logistic_fwd_bwd")
    _probed("rank_logistic_kernel", 4 * B * n_aux * 3, launch)


def rank_rows_pairs(d_all, ldd, z_all, ldz, n_all, row0, nrows, n_aux, work, totals):
    check(_lib.load().raae_rank_rows_pairs(_ptr(d_all), ldd, _ptr(z_all), ldz, n_all, row0, nrows, n_aux, _ptr(work, None),
                                           _ptr(totals, torch.float64), _stream()), "raae_rank_rows_pairs")


def rank_rows_finish(totals, n_all, nrows, n_aux, activate, scale, work, loss, dz, ldz):
    check(_lib.load().raae_rank_rows_finish(_ptr(totals, torch.float64), n_all, nrows, n_aux, 1 if activate else 0,
                                            float(scale), _ptr(work, None), _ptr(loss), _ptr(dz), ldz, _stream()),
          "raae_rank_rows_finish")


def rank_rows_masked_work_bytes(nrows, n_aux):
    return int(_lib.load().raae_rank_rows_masked_work_bytes(nrows, n_aux))


def rank_rows_masked_pairs(d_all, ldd, z_all, ldz, n_all, row0, nrows, n_aux, work, totals):
    """``rank_rows_pairs`` where NaN cells of ``d_all`` are missing labels; ``totals``: 80 doubles, the fifth block of 16
    the labelled rows per descriptor among this rank's rows."""
    assert totals.numel() >= 80
    check(_lib.load().raae_rank_rows_masked_pairs(_ptr(d_all), ldd, _ptr(z_all), ldz, n_all, row0, nrows, n_aux,
                                                  _ptr(work, None), _ptr(totals, torch.float64), _stream()),
          "raae_rank_rows_masked_pairs")


def rank_rows_masked_finish(totals, n_all, nrows, n_aux, activate, scale, work, loss, dz, ldz):
    assert totals.numel() >= 80
    check(_lib.load().raae_rank_rows_masked_finish(_ptr(totals, torch.float64), n_all, nrows, n_aux, 1 if activate else 0,
                                                   float(scale), _ptr(work, None), _ptr(loss), _ptr(dz), ldz, _stream()),
          "raae_rank_rows_masked_finish")


def style_metrics(z, n, k, a_coef, work, out):
    check(_lib.load().raae_style_metrics(_ptr(z), n, k, _ptr(a_coef, torch.float64), _ptr(work, torch.float64),
                                         _ptr(out, torch.float64), _stream()), "raae_style_metrics")


def kendall_tau_work_bytes(n, n_aux):
    return int(_lib.load().raae_kendall_tau_work_bytes(n, n_aux))


def kendall_tau(d, ldd, z, ldz, n, n_aux, work, counts, tau):
    """Kendall's tau-b of style column k against descriptor column k (``raae_kendall_tau``): ``counts`` int64
    ``[n_aux, 6]``, ``tau`` float64 ``[n_aux]``, ``work`` a byte buffer of ``kendall_tau_work_bytes``."""
    assert d.numel() >= (n - 1) * ldd + n_aux and z.numel() >= (n - 1) * ldz + n_aux
    assert counts.numel() >= 6 * n_aux and tau.numel() >= n_aux
    assert work.numel() * work.element_size() >= kendall_tau_work_bytes(n, n_aux) > 0
    check(_lib.load().raae_kendall_tau(_ptr(d), ldd, _ptr(z), ldz, n, n_aux, _ptr(work, None), _ptr(counts, torch.int64),
                                       _ptr(tau, torch.float64), _stream()), "raae_kendall_tau")


def style_decorr_work_bytes(b, k):
    return int(_lib.load().raae_style_decorr_work_bytes(b, k))


def style_decorr(z, ldz, b, k, w, work, stats, dz, lddz):
    """The decorrelation penalty of the styles ``z [b, >= k]`` (``raae_style_decorr_fwd_bwd``): ``dz += w * dD/dz`` in
    place, ``stats`` float64 ``[3]`` = {D, running sum of D, calls}, ``work`` a byte buffer of
    ``style_decorr_work_bytes``.  One launch where ``b * k <= 4096``, two otherwise; no host synchronisation."""
    assert z.numel() >= (b - 1) * ldz + k and dz.numel() >= (b - 1) * lddz + k and stats.numel() >= 3
    assert work.numel() * work.element_size() >= style_decorr_work_bytes(b, k) > 0
    check(_lib.load().raae_style_decorr_fwd_bwd(_ptr(z), ldz, b, k, float(w), _ptr(work, None), _ptr(stats, torch.float64),
                                                _ptr(dz), lddz, _stream()), "raae_style_decorr_fwd_bwd")


def group_mean(x, groups, per, L, out):
    check(_lib.load().raae_group_mean(_ptr(x), groups, per, L, _ptr(out), _stream()), "raae_group_mean")


def select_work_bytes(n, k, n_aux, n_thresh, masked=False):
    fn = _lib.load().raae_select_masked_work_bytes if masked else _lib.load().raae_select_work_bytes
    return int(fn(n, k, n_aux, n_thresh))


def select_scores(styles, n, k, aux, n_aux, spec_in, spec_out, L, thresh, work, out, masked=False):
    """Model-selection scores of one model (``raae_select_scores``): ``aux`` and ``thresh`` float64, ``out`` float64
    ``[SEL_HEAD + SEL_STRIDE * n_aux]``, ``work`` a byte buffer of ``select_work_bytes``.  ``masked``: NaN cells of
    ``aux`` are missing labels (``raae_select_scores_masked``; ``work`` sized with ``masked=True``)."""
    assert out.numel() >= _lib.SEL_HEAD + _lib.SEL_STRIDE * n_aux
    assert work.numel() * work.element_size() >= select_work_bytes(n, k, n_aux, thresh.numel(), masked)
    assert styles.numel() == n * k and aux.numel() == n * n_aux and spec_in.numel() == n * L and spec_out.numel() == n * L
    name = "raae_select_scores_masked" if masked else "raae_select_scores"
    check(getattr(_lib.load(), name)(_ptr(styles), n, k, _ptr(aux, torch.float64), n_aux, _ptr(spec_in),
                                     _ptr(spec_out), L, _ptr(thresh, torch.float64), thresh.numel(), _ptr(work, None),
                                     _ptr(out, torch.float64), _stream()), name)


def resample_rows(src, idx, w, out):
    """``raae_resample_rows``: ``src [n, Ls]`` fp32 rows (a row stride >= Ls is taken as the leading dimension) onto
    ``out [n, L]`` by the plan ``idx [L]`` int32, ``w [L]`` fp32 (``rankaae_amd.apply.resample_plan``)."""
    assert src.is_cuda and out.is_cuda and src.dtype == out.dtype == torch.float32 and src.dim() == out.dim() == 2
    assert src.stride(1) == 1 and out.stride(1) == 1 and src.shape[0] == out.shape[0]
    n, Ls = src.shape
    L = out.shape[1]
    assert idx.numel() == L and w.numel() == L
    ld_src = src.stride(0) if n > 1 else max(src.stride(0), Ls)
    ld_out = out.stride(0) if n > 1 else max(out.stride(0), L)
    check(_lib.load().raae_resample_rows(C.c_void_p(src.data_ptr()), n, Ls, ld_src, _ptr(idx, torch.int32), _ptr(w), L,
                                         C.c_void_p(out.data_ptr()), ld_out, _stream()), "raae_resample_rows")


def pointer_table(tensors):
    """A device array of the tensors' device addresses (``const float* const*`` of ``raae_ensemble_stats``).  The
    caller keeps the tensors alive."""
    return torch.tensor([t.data_ptr() for t in tensors], dtype=torch.int64).to(tensors[0].device)


def ensemble_stats(z_tab, spec, recon_tab, calib, J, n, k, n_aux, L, z_mean, z_std, d_mean, d_std, d_used, mae, ld_mae,
                   mae_mean):
    """``raae_ensemble_stats`` over ``n`` rows: ``z_tab`` / ``recon_tab`` are ``pointer_table`` s of the J models'
    contiguous ``[n, k]`` styles and ``[n, L]`` reconstructions, ``calib [J, n_aux, 4]`` float64; the outputs are
    float64 (``mae`` may be a view into ``[J, ld_mae]`` at a row offset)."""
    assert z_tab.numel() == J and recon_tab.numel() == J and spec.numel() == n * L
    assert z_mean.numel() >= n * k and z_std.numel() >= n * k and mae_mean.numel() >= n
    if n_aux:
        assert calib.numel() == J * n_aux * 4 and d_mean.numel() >= n * n_aux and d_std.numel() >= n * n_aux
        assert d_used.numel() == n_aux
    f64 = lambda t: _ptr(t, torch.float64) if n_aux else None      # noqa: E731
    check(_lib.load().raae_ensemble_stats(_ptr(z_tab, torch.int64), _ptr(spec), _ptr(recon_tab, torch.int64), f64(calib),
                                          J, n, k, n_aux, L, _ptr(z_mean, torch.float64), _ptr(z_std, torch.float64),
                                          f64(d_mean), f64(d_std), f64(d_used), C.c_void_p(mae.data_ptr()), ld_mae,
                                          _ptr(mae_mean, torch.float64), _stream()), "raae_ensemble_stats")


def _fin(fin):
    """``fin = (scale, out, slot, acc_slot, ticket)``: the loss is finished inside the kernel (``raae_loss_fin_t``);
    None: the partials are left for ``loss_finalize``."""
    if fin is None:
        return None
    scale, out, slot, acc_slot, ticket = fin
    f = _lib.LossFinT()
    f.scale, f.out, f.slot, f.acc_slot, f.ticket = float(scale), out.data_ptr(), slot, acc_slot, ticket.data_ptr()
    return C.byref(f)


def recon_loss_fwd_bwd(spec_in, spec_out, B, L, scale, partial, dout, fin=None):
    n = C.c_int(0)
    check(_lib.load().raae_recon_loss_fwd_bwd(_ptr(spec_in), _ptr(spec_out), B, L, 1 if scale else 0,
                                              _ptr(partial, torch.float64), C.byref(n), _ptr(dout), _fin(fin), _stream()),
          "raae_recon_loss_fwd_bwd")
    return n.value


def smooth_loss_fwd_bwd(x, B, L, taps, partial, dx, fin=None):
    n = C.c_int(0)
    arr = (C.c_float * len(taps))(*[float(t) for t in taps])
    check(_lib.load().raae_smooth_loss_fwd_bwd(_ptr(x), B, L, arr, len(taps), _ptr(partial, torch.float64),
                                               C.byref(n), _ptr(dx), _fin(fin), _stream()), "raae_smooth_loss_fwd_bwd")
    return n.value


def mse_fwd_bwd(a, b, n_el, partial, da, fin=None):
    n = C.c_int(0)
    check(_lib.load().raae_mse_fwd_bwd(_ptr(a), _ptr(b), n_el, _ptr(partial, torch.float64), C.byref(n), _ptr(da),
                                       _fin(fin), _stream()), "raae_mse_fwd_bwd")
    return n.value


def bce_pair_fwd_bwd(logits, n_real, n_fake, loss, dlogits):
    check(_lib.load().raae_bce_pair_fwd_bwd(_ptr(logits), n_real, n_fake, _ptr(loss), _ptr(dlogits), _stream()),
          "raae_bce_pair_fwd_bwd")


def disc_input(z_real, styles, noise, sigma, n_real, n_fake, Cc, out):
    check(_lib.load().raae_disc_input(_ptr(z_real), _ptr(styles), _ptr(noise), sigma, n_real, n_fake, Cc, _ptr(out),
                                      _stream()), "raae_disc_input")


def scale_by_dev(src, dev_scale, sign, n, dst):
    check(_lib.load().raae_scale_by_dev(_ptr(src), _ptr(dev_scale), sign, n, _ptr(dst), _stream()),
          "raae_scale_by_dev")


def loss_finalize(partial, n, scale, out, slot, acc_slot=-1):
    check(_lib.load().raae_loss_finalize(_ptr(partial, torch.float64), n, scale, _ptr(out), slot, acc_slot,
                                         _stream()), "raae_loss_finalize")


def gather_batch(spec, aux, idx, cursor, noise, spec_noise, B, L, n_aux, spec_out, aux_out):
    check(_lib.load().raae_gather_batch(_ptr(spec), _ptr(aux), _ptr(idx, torch.int64), _ptr(cursor, torch.int32),
                                        _ptr(noise), spec_noise, B, L, n_aux, _ptr(spec_out), _ptr(aux_out),
                                        _stream()), "raae_gather_batch")


def adam_step(p, m, v, g_slabs, slab_stride, seg_nslab, n, hyper, step, decoupled, max_nslab=512):
    def launch():
        check(_lib.load().raae_adam_step(_ptr(p), _ptr(m), _ptr(v), _ptr(g_slabs), slab_stride,
                                         _ptr(seg_nslab, torch.int16), n, _ptr(hyper, torch.float64),
                                         _ptr(step, torch.int32), 1 if decoupled else 0, int(max_nslab), _stream()),
              "raae_adam_step")
    _probed("adam_kernel", 28 * n, launch)       # p, m, v read + written, one gradient read (28 B / parameter)


OPT_RULE_NAMES = {_lib.OPT_ADAM: "Adam", _lib.OPT_ADAMW: "AdamW", _lib.OPT_RADAM: "RAdam", _lib.OPT_ADABOUND: "AdaBound"}


def optim_step(p, m, v, g_slabs, slab_stride, seg_nslab, n, rule, hyper, step, max_nslab=512, nan_step=None):
    """``raae_optim_step``: one step of update rule ``rule`` (``_lib.OPT_*``); ``hyper`` is the device block
    {lr, beta1, beta2, eps, weight_decay, base_lr, final_lr, gamma} (the Adam rules read the first five).
    ``nan_step`` (a device int32 word): the same update with the NaN check of ``raae_optim_step_chk`` -- the word
    receives the step count of the first step whose gradient held a NaN, and stays 0 until then."""
    if rule not in OPT_RULE_NAMES:
        raise ValueError(f"unknown optimizer rule {rule!r}")
    if hyper.numel() < (5 if rule in (_lib.OPT_ADAM, _lib.OPT_ADAMW) else 8):       # what the kernel reads
        raise ValueError(f"{OPT_RULE_NAMES[rule]}: hyper holds {hyper.numel()} values, the rule reads 8")
    family = "adam_kernel" if rule in (_lib.OPT_ADAM, _lib.OPT_ADAMW) else "optim_kernel"
    if nan_step is not None:
        def launch_chk():
            check(_lib.load().raae_optim_step_chk(_ptr(p), _ptr(m), _ptr(v), _ptr(g_slabs), slab_stride,
                                                  _ptr(seg_nslab, torch.int16), n, int(rule), _ptr(hyper, torch.float64),
                                                  _ptr(step, torch.int32), int(max_nslab), _ptr(nan_step, torch.int32),
                                                  _stream()), "raae_optim_step_chk")
        _probed(family, 28 * n, launch_chk, tag=OPT_RULE_NAMES[rule])
        return

    def launch():
        check(_lib.load().raae_optim_step(_ptr(p), _ptr(m), _ptr(v), _ptr(g_slabs), slab_stride,
                                          _ptr(seg_nslab, torch.int16), n, int(rule), _ptr(hyper, torch.float64),
                                          _ptr(step, torch.int32), int(max_nslab), _stream()),
              "raae_optim_step")
    _probed(family, 28 * n, launch, tag=OPT_RULE_NAMES[rule])


def optim_step_clip(p, m, v, g_slabs, slab_stride, seg_nslab, n, rule, hyper, step, max_nslab=512, nan_step=None,
                    scale=None):
    """``raae_optim_step_clip``: ``optim_step`` with the gradient multiplied by the device float ``scale[0]`` (the clip
    scale ``grad_norm`` leaves) before weight decay and the moments.  ``scale=None``: exactly ``optim_step``."""
    if rule not in OPT_RULE_NAMES:
        raise ValueError(f"unknown optimizer rule {rule!r}")
    if hyper.numel() < (5 if rule in (_lib.OPT_ADAM, _lib.OPT_ADAMW) else 8):       # what the kernel reads
        raise ValueError(f"{OPT_RULE_NAMES[rule]}: hyper holds {hyper.numel()} values, the rule reads 8")
    family = "adam_kernel" if rule in (_lib.OPT_ADAM, _lib.OPT_ADAMW) else "optim_kernel"

    def launch():
        check(_lib.load().raae_optim_step_clip(_ptr(p), _ptr(m), _ptr(v), _ptr(g_slabs), slab_stride,
                                               _ptr(seg_nslab, torch.int16), n, int(rule), _ptr(hyper, torch.float64),
                                               _ptr(step, torch.int32), int(max_nslab),
                                               _ptr(nan_step, torch.int32) if nan_step is not None else None,
                                               _ptr(scale) if scale is not None else None, _stream()),
              "raae_optim_step_clip")
    _probed(family, 28 * n, launch, tag=OPT_RULE_NAMES[rule])


GRAD_NORM_PARTS = 256       # RAAE_GRAD_NORM_PARTS


def grad_norm(g_slabs, slab_stride, seg_nslab, n, max_nslab, max_norm, partial, ticket, out, clipped):
    """``raae_grad_norm``: ``out`` (2 floats) = {L2 norm of the slab-summed gradient, min(1, max_norm / (norm + 1e-6))};
    ``clipped`` (int32 word) += 1 when the scale is below 1.  ``partial``: ``GRAD_NORM_PARTS`` doubles, ``ticket``: an
    int32 word that is zero before the first launch (the launch leaves it zero)."""
    if partial.numel() < GRAD_NORM_PARTS or out.numel() < 2:
        raise ValueError("grad_norm: partial holds GRAD_NORM_PARTS doubles, out two floats")
    check(_lib.load().raae_grad_norm(_ptr(g_slabs), slab_stride, _ptr(seg_nslab, torch.int16), n, int(max_nslab),
                                     float(max_norm), _ptr(partial, torch.float64), _ptr(ticket, torch.int32), _ptr(out),
                                     _ptr(clipped, torch.int32), _stream()), "raae_grad_norm")


def ema_step(ema, p, n, decay):
    """``raae_ema_step``: ``ema[i] = fmaf(d, ema[i], (1 - d) * p[i])`` for ``i < n`` in fp32, ``d = decay`` with
    ``0 <= decay < 1`` (config key ``ema_decay``).  One element-wise launch; bitwise reproducible."""
    check(_lib.load().raae_ema_step(_ptr(ema), _ptr(p), int(n), float(decay), _stream()), "raae_ema_step")


SPEC_SHIFT_OFF = 0x80000000     # hash index of row 0's shift draw: beyond every dropout element of a step (< 2^31)


def spec_augment(spec, idx, cursor, rng_state, B, L, max_shift, spec_noise, noise_goff, spec_out):
    """``raae_spec_augment`` (config key ``spec_shift``): behind ``step_begin`` on the same state, ``spec_out[b]`` = row
    ``idx[cursor - B + b]`` of ``spec`` resampled at ``l + delta_b`` (linear, replicated edges; ``delta_b`` uniform in
    ``[-max_shift, max_shift)`` from the step's hash keys) plus the head's spectral noise.  One element-wise launch."""
    assert rng_state.dtype == torch.int64 and rng_state.numel() >= 3 and cursor.dtype == torch.int32
    check(_lib.load().raae_spec_augment(_ptr(spec), _ptr(idx, torch.int64), _ptr(cursor, torch.int32), _ptr(rng_state, torch.int64),
                                        int(B), int(L), float(max_shift), float(spec_noise), int(noise_goff),
                                        _ptr(spec_out), _stream()), "raae_spec_augment")


SPEC_BROADEN_OFF = 0xC0000000   # hash index of row 0's width draw: beyond every shift draw (SPEC_SHIFT_OFF + b, b < 2^30)


def spec_augment2(spec, idx, cursor, rng_state, B, L, max_sigma, max_shift, spec_noise, noise_goff, spec_out):
    """``raae_spec_augment2`` (config key ``spec_broaden``): ``spec_augment`` with row b convolved, in front of its shift,
    with a normalised Gaussian of its own width ``sigma_b``, uniform in ``[0, max_sigma)`` grid points, from the step's
    hash keys (replicated edges, radius ``ceil(3 max_sigma) <= 64``).  One launch, one workgroup per row, the row in
    LDS; ``max_sigma = 0`` is ``spec_augment`` bit for bit."""
    assert rng_state.dtype == torch.int64 and rng_state.numel() >= 3 and cursor.dtype == torch.int32
    check(_lib.load().raae_spec_augment2(_ptr(spec), _ptr(idx, torch.int64), _ptr(cursor, torch.int32), _ptr(rng_state, torch.int64),
                                         int(B), int(L), float(max_sigma), float(max_shift), float(spec_noise),
                                         int(noise_goff), _ptr(spec_out), _stream()), "raae_spec_augment2")


SPEC_GAIN_OFF = 0xA0000000      # hash index of row 0's gain draw: between the shift draws and the broaden draws (b < 2^29)
SPEC_TILT_OFF = 0xE0000000      # hash index of row 0's tilt draw: beyond every broaden draw; ends at 2^32 - 1 (b < 2^29)
SPEC_NORM_BMAX = 2 ** 29        # the most rows raae_spec_augment3 takes: above it the four ranges of draws would meet


def spec_augment3(spec, idx, cursor, rng_state, B, L, max_sigma, max_shift, max_gain, max_tilt, spec_noise, noise_goff,
                  spec_out):
    """``raae_spec_augment3`` (config keys ``spec_gain``, ``spec_tilt``): ``spec_augment2`` with row b, behind its
    broadening and its shift and before the noise, multiplied by ``g_b = 1 + (2 u_b - 1) max_gain`` and tilted by
    ``c_b r_l``, ``c_b = (2 u'_b - 1) max_tilt``, ``r_l = (2 l - (L - 1)) / (L - 1)``; both draws from the step's hash
    keys.  One launch, ``spec_augment2``'s geometry; any of the four values may be 0."""
    assert rng_state.dtype == torch.int64 and rng_state.numel() >= 3 and cursor.dtype == torch.int32
    check(_lib.load().raae_spec_augment3(_ptr(spec), _ptr(idx, torch.int64), _ptr(cursor, torch.int32), _ptr(rng_state, torch.int64),
                                         int(B), int(L), float(max_sigma), float(max_shift), float(max_gain), float(max_tilt),
                                         float(spec_noise), int(noise_goff), _ptr(spec_out), _stream()), "raae_spec_augment3")


def slab_reduce(g_slabs, slab_stride, seg_nslab, n, out, max_nslab=512):
    check(_lib.load().raae_slab_reduce(_ptr(g_slabs), slab_stride, _ptr(seg_nslab, torch.int16), n, _ptr(out),
                                       int(max_nslab), _stream()), "raae_slab_reduce")


def step_tick(steps, n, mask, rng_counter, cursor, cursor_inc):
    check(_lib.load().raae_step_tick(_ptr(steps, torch.int32), n, mask, _ptr(rng_counter, torch.int64),
                                     _ptr(cursor, torch.int32), cursor_inc, _stream()), "raae_step_tick")


def step_begin(steps, nsteps, mask, rng_state, cursor, stride, ticket, spec, aux, idx, B, L, n_aux, spec_noise, noise_tape,
               noise_goff, spec_out, aux_out, tape=None):
    """Tick + tape fill + batch gather in one launch (``raae_step_begin``).  ``noise_tape``: the noise slot of a
    host-filled tape (parity mode) or None (generated in the kernel at position ``noise_goff`` of the Gaussian
    numbering); ``tape``: an engine ``Tape`` whose resident slots are filled here (None / no slots: no fill)."""
    a = _lib.StepBeginT()
    a.steps, a.nsteps, a.step_mask, a.rng_state = _p(steps), int(nsteps), int(mask), _p(rng_state)
    a.cursor, a.stride, a.ticket = _p(cursor), int(stride), _p(ticket)
    a.spec, a.aux, a.idx, a.B, a.L, a.n_aux = _p(spec), _p(aux), _p(idx), B, L, n_aux
    a.spec_noise, a.noise_tape, a.noise_goff = float(spec_noise), _p(noise_tape), int(noise_goff)
    a.spec_out, a.aux_out = _p(spec_out), _p(aux_out)
    if tape is not None and len(tape.segs) > 0:
        a.tape, a.seg_desc, a.seg_scale, a.nseg, a.total = _p(tape.buf), _p(tape.seg_desc), _p(tape.seg_scale), len(tape.segs), tape.total
    assert steps.dtype == torch.int32 and rng_state.dtype == torch.int64 and cursor.dtype == torch.int32 and idx.dtype == torch.int64
    check(_lib.load().raae_step_begin(C.byref(a), _stream()), "raae_step_begin")


def rng_fill(tape, seg_desc, seg_scale, nseg, total, seed, counter):
    check(_lib.load().raae_rng_fill(_ptr(tape), _ptr(seg_desc, torch.int32), _ptr(seg_scale), nseg, total,
                                    C.c_ulonglong(seed), _ptr(counter, torch.int64), _stream()), "raae_rng_fill")


class Graph:
    """A captured HIP graph of one training step (hipStreamBeginCapture / hipGraphLaunch)."""

    active = 0      # captures in progress in this process (any engine, any thread): StepEngine.close() must not run inside one
    _lock = __import__("threading").Lock()

    def __init__(self):
        self.handle = C.c_void_p()

    def begin(self):
        check(_lib.load().raae_graph_begin(_stream()), "raae_graph_begin")
        with Graph._lock:
            Graph.active += 1

    def end(self):
        with Graph._lock:
            Graph.active -= 1
        check(_lib.load().raae_graph_end(_stream(), C.byref(self.handle)), "raae_graph_end")

    def launch(self):
        check(_lib.load().raae_graph_launch(self.handle, _stream()), "raae_graph_launch")

    def __del__(self):
        try:
            if self.handle:
                _lib.load().raae_graph_destroy(self.handle)
        except Exception:
            pass


class Event:
    def __init__(self):
        self.h = C.c_void_p()
        check(_lib.load().raae_event_create(C.byref(self.h)), "raae_event_create")

    def record(self):
        check(_lib.load().raae_event_record(self.h, _stream()), "raae_event_record")

    def elapsed_ms(self, stop):
        ms = C.c_float(0)
        check(_lib.load().raae_event_elapsed_ms(self.h, stop.h, C.byref(ms)), "raae_event_elapsed_ms")
        return ms.value


# ------------------------------------------------------------------ roofline probe (bench.py)
class Probe:
    """While ``ops.PROBE`` holds one of these, every kernel launch that goes through a probed wrapper is followed
    by ``reps`` identical launches captured into a small hipGraph and replayed between two HIP events recorded on the
    stream the kernel is launched on (a single bracketed eager launch would measure the host's submission latency,
    tens of microseconds, not the kernel).  ``records[family] = [(event0, event1, algorithmic bytes)]``."""

    def __init__(self, reps=10, detail=False):
        self.reps, self.records, self.graphs, self.busy, self.detail = reps, {}, [], False, detail

    def summary(self):
        """``{family: dict(launches, avg_us, bytes)}`` -- call after a device synchronisation."""
        out = {}
        for fam, recs in self.records.items():
            us = [1e3 * a.elapsed_ms(z) / self.reps for a, z, _ in recs]
            out[fam] = {"launches": len(recs), "avg_us": sum(us) / len(us), "total_us": sum(us),
                        "bytes": sum(n for *_, n in recs) / len(recs)}
        return out


PROBE = None


def _probed(family, nbytes, launch, tag=None):
    out = launch()
    pr = PROBE
    if pr is None or pr.busy:
        return out
    if pr.detail and tag is not None:
        family = f"{family}[{tag}]"
    pr.busy = True
    try:
        g = Graph()
        g.begin()
        for _ in range(pr.reps):
            launch()
        g.end()
        e0, e1 = Event(), Event()
        # ALONE means alone: drain every stream first -- replays of a weight-gradient launch on a side stream were still
        # running beside the next main-stream kernel's replays (its "alone" time then doubled or not, depending on timing)
        torch.cuda.synchronize()
        e0.record()
        g.launch()
        e1.record()
        pr.graphs.append(g)
        pr.records.setdefault(family, []).append((e0, e1, int(nbytes)))
    finally:
        pr.busy = False
    return out


def _ktag(k):
    return f"{k.Cin}x{k.Lin}->{k.Cout}x{k.Lout}"


def block_bytes(kernel, k, B, mask=False, need_dx=True, input_bn=True):
    """ALGORITHMIC bytes of one launch of a fused residual-block kernel (SURVEY.md 8d's rule: every tensor the
    kernel must read or write counted once, fp32, weights once, no extra passes): ``k`` is the block's static
    shape (nets_conv.Block).  Per sample, with X [Cin,Lin], T1 [Cout,L1], everything else [C,Lout]:
      fwd_a  reads X (+ dropout mask)              writes T1, Sh (conv_short), E1, E2
      fwd_b  reads T1, E2, Sh | X                  writes T2, E3 (conv_excit), Y
      bwd_b  reads gY (+ Y behind a BatchNorm), T2, Sh, E3 | E2, T1 (, E2)      writes dT2, dSh, dEx, dBn2 (, dBnE)
      bwd_a  reads dBn2, T1, dSh, dBnE + E2 | dE2, E1 (, mask, X)               writes dT1 (, dE2), dE1, dR
    """
    ci_lin, co_l1, co_lo, ci_lo, ci_e = k.Cin * k.Lin, k.Cout * k.L1, k.Cout * k.Lout, k.Cin * k.Lout, k.Cin * k.E
    short, excit = k.cvs is not None, k.cve is not None
    nw = lambda mod: 0 if mod is None else mod.weight.numel() + (0 if mod.bias is None else mod.bias.numel())
    m = k.m
    if kernel == "fwd_a":
        per = ci_lin * (2 if mask else 1) + co_l1 + (co_lo if short else 0) + ci_e + ci_lo
        w = nw(m.conv1) + nw(m.conv_short) + nw(m.fc1) + nw(m.fc2)
    elif kernel == "fwd_b":
        per = co_l1 + ci_lo + (co_lo if short else ci_lin) + co_lo * (3 if excit else 2)
        w = nw(m.conv2) + nw(m.conv_excit)
    elif kernel == "bwd_b":
        per = co_lo * (2 if input_bn else 1) + co_lo * (3 if short else 2) + co_l1 + (ci_lo if excit else 0) + \
            3 * co_lo + co_l1 + (ci_lo if excit else 0)
        w = nw(m.conv2) + nw(m.conv_excit)
    elif kernel == "bwd_a":
        per = 2 * co_l1 + co_lo + (2 * ci_lo if excit else ci_lo) + ci_e + (ci_lin if mask else 0) + \
            co_l1 + (ci_lo if excit else 0) + ci_e + ((ci_lin * (2 if input_bn else 1)) if need_dx else 0)
        w = nw(m.conv1) + nw(m.conv_short) + nw(m.fc1) + nw(m.fc2)
    else:
        raise ValueError(kernel)
    return 4 * (B * per + w)


# ------------------------------------------------------------------ conv-network ops
def make_view(raw, slope=None, bn=None, mask=None):
    v = _lib.ViewT()
    v.raw = raw.data_ptr()
    v.slope = slope.data_ptr() if slope is not None else None
    if bn is not None:
        v.bn = bn
        v.has_bn = 1
    else:
        v.has_bn = 0
    v.mask = mask.data_ptr() if mask is not None else None
    v._keep = (raw, slope, mask)
    return v


def make_grad(g, raw=None, slope=None, bn=None, g_partials=None, g_nparts=0, u=None, act=0):
    s = _lib.GradT()
    s.g = g.data_ptr()
    s.g_partials = g_partials.data_ptr() if g_partials is not None else None
    s.g_nparts = int(g_nparts)
    s.u = u.data_ptr() if u is not None else None
    if bn is not None:
        s.bn = bn
        s.has_bn = 1
    else:
        s.has_bn = 0
    s.raw = raw.data_ptr() if raw is not None else None
    s.slope = slope.data_ptr() if slope is not None else None
    s.act = int(act)
    s._keep = (g, raw, slope, u, g_partials)
    return s


def make_conv(Cin, Lin, Cout, Lout, K, stride, pad, pad_replicate, groups, transposed):
    c = _lib.ConvT()
    c.Cin, c.Lin, c.Cout, c.Lout, c.K, c.stride, c.pad = Cin, Lin, Cout, Lout, K, stride, pad
    c.pad_replicate, c.groups, c.transposed = int(pad_replicate), groups, int(transposed)
    return c


def conv_bytes(cv, B, extra_in=0, extra_out=0):
    """``4 B (Cin Lin + Cout Lout) + 4 (weights + bias)`` per Conv1d call; ``extra_*``: further whole
    input- / output-sized tensors the call must touch (a mask, the raw output behind an activation gradient, ...)."""
    return 4 * B * (cv.Cin * cv.Lin * (1 + extra_in) + cv.Cout * cv.Lout * (1 + extra_out)) + \
        4 * (cv.Cout * (cv.Cin // cv.groups) * cv.K + cv.Cout)


def conv_fwd(view, B, cv, w, bias, out, stats_kind=0, out_slope=None, out_partials=None, act=0):
    def launch():
        n = C.c_int(0)
        check(_lib.load().raae_conv_fwd(C.byref(view), B, C.byref(cv), _ptr(w), _ptr(bias), _ptr(out), stats_kind,
                                        _ptr(out_slope), _ptr(out_partials, torch.float64), C.byref(n), act, _stream()),
              "raae_conv_fwd")
        return n.value
    return _probed("conv_fwd (per-layer)", conv_bytes(cv, B, extra_in=1 if view.mask else 0), launch)


def conv_bwd_data(go, B, cv, w, view, din, accumulate, din_partials=None):
    def launch():
        n = C.c_int(0)
        check(_lib.load().raae_conv_bwd_data(C.byref(go), B, C.byref(cv), _ptr(w), C.byref(view), _ptr(din),
                                             1 if accumulate else 0, _ptr(din_partials, torch.float64), C.byref(n),
                                             _stream()), "raae_conv_bwd_data")
        return n.value
    return _probed("conv_bwd_data (per-layer)", conv_bytes(cv, B, extra_in=1 if din_partials is not None else 0,
                                                           extra_out=1 if go.raw else 0), launch)


def head_bwd_supported(go, B, cv, view):
    return bool(_lib.load().raae_head_bwd_supported(C.byref(go), B, C.byref(cv), C.byref(view)))


def head_bwd(go, B, cv, w, view, din, din_partials, dw, dbias, slab_stride):
    """The decoder head's backward in one pass (``raae_head_bwd``): returns (partial rows of din, slabs of dw/dbias)."""
    def launch():
        n, ns = C.c_int(0), C.c_int(0)
        check(_lib.load().raae_head_bwd(C.byref(go), B, C.byref(cv), _ptr(w), C.byref(view), _ptr(din),
                                        _ptr(din_partials, torch.float64), C.byref(n), _ptr(dw), _ptr(dbias), slab_stride,
                                        C.byref(ns), _stream()), "raae_head_bwd")
        return n.value, ns.value
    # reads g, out and the C input rows, writes the C gradient rows
    return _probed("head_bwd", 4 * B * cv.Lin * (2 * cv.Cin + 2) + 4 * (cv.Cin + 1), launch)


def conv_bwd_weight(go, B, cv, view, dw, dbias, dslope, slab_stride):
    def launch():
        n = C.c_int(0)
        check(_lib.load().raae_conv_bwd_weight(C.byref(go), B, C.byref(cv), C.byref(view), _ptr(dw), _ptr(dbias),
                                               _ptr(dslope), slab_stride, C.byref(n), _stream()), "raae_conv_bwd_weight")
        return n.value
    return _probed("conv_bwd_weight (per-layer)", conv_bytes(cv, B, extra_out=1 if go.raw else 0), launch)


def lenlin_fwd(view, B, Cc, Lin, w, bias, E, out, stats_kind=0, out_slope=None, out_partials=None):
    n = C.c_int(0)
    check(_lib.load().raae_lenlin_fwd(C.byref(view), B, Cc, Lin, _ptr(w), _ptr(bias), E, _ptr(out), stats_kind,
                                      _ptr(out_slope), _ptr(out_partials, torch.float64), C.byref(n), _stream()),
          "raae_lenlin_fwd")
    return n.value


def lenlin_bwd_data(go, B, Cc, E, w, view, Lin, din, accumulate, din_partials=None):
    n = C.c_int(0)
    check(_lib.load().raae_lenlin_bwd_data(C.byref(go), B, Cc, E, _ptr(w), C.byref(view), Lin, _ptr(din),
                                           1 if accumulate else 0, _ptr(din_partials, torch.float64), C.byref(n),
                                           _stream()), "raae_lenlin_bwd_data")
    return n.value


def lenlin_bwd_weight(go, B, Cc, E, view, Lin, dw, dbias, dslope, slab_stride):
    n = C.c_int(0)
    check(_lib.load().raae_lenlin_bwd_weight(C.byref(go), B, Cc, E, C.byref(view), Lin, _ptr(dw), _ptr(dbias),
                                             _ptr(dslope), slab_stride, C.byref(n), _stream()),
          "raae_lenlin_bwd_weight")
    return n.value


def sum3_fwd(va, vb, vc, B, Cc, L, y, out_partials=None):
    n = C.c_int(0)
    check(_lib.load().raae_sum3_fwd(C.byref(va), C.byref(vb), C.byref(vc), B, Cc, L, _ptr(y),
                                    _ptr(out_partials, torch.float64), C.byref(n), _stream()), "raae_sum3_fwd")
    return n.value


def grad_materialize(go, B, Cc, L, draw, accumulate=False, dslope=None, slab_stride=0):
    n = C.c_int(0)
    check(_lib.load().raae_grad_materialize(C.byref(go), B, Cc, L, _ptr(draw), 1 if accumulate else 0, _ptr(dslope),
                                            slab_stride, C.byref(n), _stream()), "raae_grad_materialize")
    return n.value


def _p(t):
    return t.data_ptr() if t is not None else None


def block_fwd_a_args(view_in, mask, B, k, m, T1, Sh, E1, E2, pT1, pE2):
    """``raae_block_fwd_a_t`` of a residual block (``k``: nets_conv.Block, ``m``: its nn.Module)."""
    a = _lib.BlockFwdAT()
    a.inp, a.mask, a.B = view_in, _p(mask), B
    a.Cin, a.Cout, a.Lin, a.L1, a.Lout, a.E = k.Cin, k.Cout, k.Lin, k.L1, k.Lout, k.E
    a.cv1 = k.cv1
    a.has_short = 1 if k.cvs is not None else 0
    if k.cvs is not None:
        a.cvs = k.cvs
        a.ws, a.bs = _p(m.conv_short.weight), _p(m.conv_short.bias)
    a.w1, a.b1, a.slope1 = _p(m.conv1.weight), _p(m.conv1.bias), _p(m.relu1.weight)
    a.wf1, a.bf1, a.se1 = _p(m.fc1.weight), _p(m.fc1.bias), _p(m.relu_excit_1.weight)
    a.wf2, a.bf2, a.se2 = _p(m.fc2.weight), _p(m.fc2.bias), _p(m.relu_excit_2.weight)
    a.T1, a.Sh, a.E1, a.E2, a.pT1, a.pE2 = _p(T1), _p(Sh), _p(E1), _p(E2), _p(pT1), _p(pE2)
    a.nbytes = block_bytes("fwd_a", k, B, mask=mask is not None)
    a.tag = _ktag(k)
    return a


def block_fwd_a(a):
    """Fused forward phase A of a residual block; returns the number of partial-statistic rows written."""
    def launch():
        n = C.c_int(0)
        check(_lib.load().raae_block_fwd_a(C.byref(a), C.byref(n), _stream()), "raae_block_fwd_a")
        return n.value
    return _probed("block_fwd_a_kernel", a.nbytes, launch, a.tag)


def block_fwd_pair(kind, x, y):
    """Phase ``kind`` ("a" / "b") of two independent blocks in one launch; returns both row counts."""
    def launch():
        n1, n2 = C.c_int(0), C.c_int(0)
        fn = _lib.load().raae_block_fwd_a2 if kind == "a" else _lib.load().raae_block_fwd_b2
        check(fn(C.byref(x), C.byref(y), C.byref(n1), C.byref(n2), _stream()), f"raae_block_fwd_{kind}2")
        return n1.value, n2.value
    return _probed(f"block_fwd_{kind}2_kernel", x.nbytes + y.nbytes, launch)


def block_fwd_b_args(vT1, vE2, vR, B, k, m, Sh, T2, E3, Y, pY):
    a = _lib.BlockFwdBT()
    a.vT1, a.vE2 = vT1, vE2
    if vR is not None:
        a.vR = vR
    a.B, a.Cin, a.Cout, a.L1, a.Lout = B, k.Cin, k.Cout, k.L1, k.Lout
    a.cv2 = k.cv2
    a.has_short = 1 if k.cvs is not None else 0
    a.has_excit = 1 if k.cve is not None else 0
    if k.cve is not None:
        a.cve = k.cve
        a.we, a.be, a.se3 = _p(m.conv_excit.weight), _p(m.conv_excit.bias), _p(m.relu_excit_3.weight)
    if k.cvs is not None:
        a.Sh, a.ss = _p(Sh), _p(m.relu_short.weight)
    a.w2, a.b2, a.slope2 = _p(m.conv2.weight), _p(m.conv2.bias), _p(m.relu2.weight)
    a.T2, a.E3, a.Y, a.pY = _p(T2), _p(E3), _p(Y), _p(pY)
    a.nbytes = block_bytes("fwd_b", k, B)
    a.tag = _ktag(k)
    return a


def block_fwd_b(a):
    def launch():
        n = C.c_int(0)
        check(_lib.load().raae_block_fwd_b(C.byref(a), C.byref(n), _stream()), "raae_block_fwd_b")
        return n.value
    return _probed("block_fwd_b_kernel", a.nbytes, launch, a.tag)


def block_bwd_b_args(gy, vT1, vE2, B, k, m, w, slab_stride, gslab, wgrad=None):
    """``raae_block_bwd_b_t`` of fused backward phase B (``w``: the block's workspace, ``gslab(p)``: slab-0 view of
    parameter p); ``wgrad``: the following block's weight-gradient tasks, which ride in the same launch."""
    a = _lib.BlockBwdBT()
    a.gy, a.vT1 = gy, vT1
    if vE2 is not None:
        a.vE2 = vE2
    a.B, a.Cin, a.Cout, a.L1, a.Lout = B, k.Cin, k.Cout, k.L1, k.Lout
    a.cv2 = k.cv2
    a.has_short = 1 if k.cvs is not None else 0
    a.has_excit = 1 if k.cve is not None else 0
    a.w2, a.slope2, a.T2 = _p(m.conv2.weight), _p(m.relu2.weight), _p(w.T2)
    if k.cvs is not None:
        a.ss, a.Sh, a.dslope_s = _p(m.relu_short.weight), _p(w.Sh), _p(gslab(m.relu_short.weight))
    if k.cve is not None:
        a.cve = k.cve
        a.we, a.se, a.Ex = _p(m.conv_excit.weight), _p(m.relu_excit_3.weight), _p(w.E3)
        a.dslope_e = _p(gslab(m.relu_excit_3.weight))
        a.dBnE, a.pdBnE = _p(w.dBnE), _p(w.pdBnE)
    else:
        a.se, a.Ex = _p(m.relu_excit_2.weight), _p(w.E2)
        a.dslope_e = _p(gslab(m.relu_excit_2.weight))
    a.dT2, a.dSh, a.dEx, a.dBn2, a.pdBn2 = _p(w.dT2), _p(w.dSh), _p(w.dEx), _p(w.dBn2), _p(w.pdBn2)
    a.dslope2 = _p(gslab(m.relu2.weight))
    a.slab_stride = slab_stride
    a.nbytes = block_bytes("bwd_b", k, B, input_bn=bool(gy.has_bn))
    a.wgrad, a.tag = wgrad, _ktag(k)
    a.keep = (gy, vT1, vE2)         # (what the struct's pointers refer to stays alive as long as the struct)
    return a


def block_bwd_b_launch(a):
    """Launch a ``block_bwd_b_args`` block; returns the partial-row count, with weight-gradient tasks
    ``(rows, [slabs per task])``."""
    wgrad, nbytes = a.wgrad, a.nbytes
    if wgrad is not None:          # the following block's weight-gradient tasks ride in the same launch
        def launch2():
            n, ns = C.c_int(0), (C.c_int * 6)()
            check(_lib.load().raae_block_bwd_b_wgrad(C.byref(a), C.byref(wgrad), C.byref(n), ns, _stream()),
                  "raae_block_bwd_b_wgrad")
            return n.value, list(ns)[:wgrad.n_conv + wgrad.n_lin]
        return _probed("block_bwd_b_wgrad_kernel", nbytes + wgrad.nbytes, launch2, a.tag)

    def launch():
        n = C.c_int(0)
        check(_lib.load().raae_block_bwd_b(C.byref(a), C.byref(n), _stream()), "raae_block_bwd_b")
        return n.value
    return _probed("block_bwd_b_kernel", nbytes, launch, a.tag)


def block_bwd_b(gy, vT1, vE2, B, k, m, w, slab_stride, gslab, wgrad=None):
    """Fused backward phase B, launched."""
    return block_bwd_b_launch(block_bwd_b_args(gy, vT1, vE2, B, k, m, w, slab_stride, gslab, wgrad))


def block_bwd_a_args(g1, ge, view_in, mask, B, k, m, w, dE2, dR, pdR, slab_stride, gslab):
    a = _lib.BlockBwdAT()
    a.g1 = g1
    if ge is not None:
        a.ge = ge
    a.inp, a.mask = view_in, _p(mask)
    a.B, a.Cin, a.Cout, a.Lin, a.L1, a.Lout, a.E = B, k.Cin, k.Cout, k.Lin, k.L1, k.Lout, k.E
    a.cv1 = k.cv1
    a.has_short = 1 if k.cvs is not None else 0
    a.has_excit = 1 if k.cve is not None else 0
    if k.cvs is not None:
        a.cvs = k.cvs
        a.ws = _p(m.conv_short.weight)
    a.w1, a.wf1, a.wf2, a.se1 = _p(m.conv1.weight), _p(m.fc1.weight), _p(m.fc2.weight), _p(m.relu_excit_1.weight)
    a.E1, a.dSh, a.dT1, a.dE2, a.dE1, a.dR, a.pdR = _p(w.E1), _p(w.dSh), _p(w.dT1), _p(dE2), _p(w.dE1), _p(dR), _p(pdR)
    a.dslope1 = _p(gslab(m.relu1.weight))
    a.dslope_e1 = _p(gslab(m.relu_excit_1.weight))
    if k.cve is not None:
        a.dslope_e2 = _p(gslab(m.relu_excit_2.weight))
    a.slab_stride = slab_stride

    a.nbytes = block_bytes("bwd_a", k, B, mask=mask is not None, need_dx=dR is not None, input_bn=pdR is not None)
    a.tag = _ktag(k)
    a.keep = (g1, ge, view_in)
    return a


def block_bwd_a_launch(a):
    def launch():
        n = C.c_int(0)
        check(_lib.load().raae_block_bwd_a(C.byref(a), C.byref(n), _stream()), "raae_block_bwd_a")
        return n.value
    return _probed("block_bwd_a_kernel", a.nbytes, launch, a.tag)


def block_bwd_a(g1, ge, view_in, mask, B, k, m, w, dE2, dR, pdR, slab_stride, gslab):
    return block_bwd_a_launch(block_bwd_a_args(g1, ge, view_in, mask, B, k, m, w, dE2, dR, pdR, slab_stride, gslab))


def adam_part_args(p, m, v, g_slabs, slab_stride, seg_nslab, n, rule, hyper, step, max_nslab, nan_step=None):
    """``raae_co_adam_t``: an Adam / AdamW update (of a slice of an optimizer's range) as a body of ``co_launch``."""
    a = _lib.CoAdamT()
    a.p, a.m, a.v, a.g_slabs, a.slab_stride = _ptr(p), _ptr(m), _ptr(v), _ptr(g_slabs), slab_stride
    a.seg_nslab, a.n, a.rule = _ptr(seg_nslab, torch.int16), n, int(rule)
    a.hyper, a.step, a.max_nslab = _ptr(hyper, torch.float64), _ptr(step, torch.int32), int(max_nslab)
    a.nan_step = _ptr(nan_step, torch.int32) if nan_step is not None else None
    a.nbytes = 28 * n
    return a


def conv_fwd_item(view, B, cv, w, bias, out, act):
    """The decoder's head (``conv_fwd`` without statistics) as an item of a generator of launches: called, it launches
    what ``conv_fwd`` launches; ``co_args`` (``raae_co_conv_fwd_t``) lets it ride in another launch (``co_launch``)."""
    def launch():
        return conv_fwd(view, B, cv, w, bias, out, 0, None, None, act)
    launch.co_args = _lib.CoConvFwdT(C.pointer(view), B, C.pointer(cv), _ptr(w), _ptr(bias), _ptr(out), act)
    launch.co_args.nbytes = conv_bytes(cv, B)
    launch.keep = (view, cv)
    return launch


# what a generator of launches (nets_conv.forward_steps / backward_steps, the engine's Adam updates; schedule.py) yields:
# ("a" | "b" | "head" | "bwd_a" | "bwd_b" | "wgrad" | "adam", argument block)
_CO_KIND = {"a": _lib.CO_FWD_A, "b": _lib.CO_FWD_B, "bwd_a": _lib.CO_BWD_A}


def launch_item(kind, a):
    """One yielded launch on its own; returns what the generator expects back."""
    if kind == "a":
        return block_fwd_a(a)
    if kind == "b":
        return block_fwd_b(a)
    if kind == "bwd_a":
        return block_bwd_a_launch(a)
    if kind == "bwd_b":
        return block_bwd_b_launch(a)
    if kind == "wgrad":
        return block_wgrad(a.B, None, None, a.slab_stride, args=a)
    if kind in ("adam", "head"):
        return a()            # (the engine's own launch: any rule, checked or not; the head: conv_fwd)
    raise ValueError(kind)


def _co_side(kind, a):
    """One side of ``raae_co_launch``: (RAAE_CO_* kind, argument block, algorithmic bytes, name, slab-count array)."""
    if kind == "bwd_b":
        ns = (C.c_int * 6)()
        return (_lib.CO_BWD_B_WGRAD, _lib.CoBwdBWgradT(C.pointer(a), C.pointer(a.wgrad), C.cast(ns, C.POINTER(C.c_int))),
                a.nbytes + a.wgrad.nbytes, "bwd_b_wgrad", ns)
    if kind == "wgrad":
        ns = (C.c_int * 6)()
        return _lib.CO_WGRAD, _lib.CoWgradT(C.pointer(a), C.cast(ns, C.POINTER(C.c_int))), a.nbytes, "wgrad", ns
    if kind == "adam":
        return _lib.CO_ADAM, a.co_args, a.co_args.nbytes, "adam", None
    if kind == "head":
        return _lib.CO_HEAD_FWD, a.co_args, a.co_args.nbytes, "head", None
    return _CO_KIND[kind], a, a.nbytes, ("fwd_" + kind if kind in ("a", "b") else kind), None


def co_pairable(kx, ax, ky, ay):
    """Whether ``co_launch`` runs the two yielded launches as ONE (x: the host, a backward launch, the weight-gradient
    tasks or the update that end a backward pass, or an encoder forward block; y: the rider): the library has an
    instance for the pair (``raae_co_instance``).  Without one the host goes alone and the rider waits."""
    if not ((kx in ("bwd_a", "wgrad", "adam", "a") or (kx == "bwd_b" and ax.wgrad is not None)) and
            ky in ("a", "b", "adam", "head")):
        return False
    if (kx == "adam" and getattr(ax, "co_args", None) is None) or (ky == "adam" and getattr(ay, "co_args", None) is None):
        return False
    cx, px, _, _, _ = _co_side(kx, ax)
    cy, py, _, _, _ = _co_side(ky, ay)
    rc = _lib.load().raae_co_instance(cx, C.cast(C.pointer(px), C.c_void_p), cy, C.cast(C.pointer(py), C.c_void_p))
    if rc < 0:
        check(rc, "raae_co_instance")
    return rc == 1


def co_launch(kx, ax, ky, ay):
    """Two independent launches as one (``raae_co_launch``); returns what each would have returned alone."""
    cx, px, nbx, namex, ns = _co_side(kx, ax)
    cy, py, nby, namey, _ = _co_side(ky, ay)

    def launch():
        n1, n2 = C.c_int(0), C.c_int(0)
        check(_lib.load().raae_co_launch(cx, C.cast(C.pointer(px), C.c_void_p), cy, C.cast(C.pointer(py), C.c_void_p),
                                         C.byref(n1), C.byref(n2), _stream()), "raae_co_launch")
        if kx == "bwd_b":
            rx = (n1.value, list(ns)[:ax.wgrad.n_conv + ax.wgrad.n_lin])
        elif kx == "wgrad":
            rx = list(ns)[:ax.n_conv + ax.n_lin]
        else:
            rx = None if kx == "adam" else n1.value
        return rx, (None if ky in ("adam", "head") else n2.value)
    return _probed(f"co_kernel[{namex}+{namey}]", nbx + nby, launch)


def block_wgrad_args(B, conv_tasks, lin_tasks, slab_stride):
    """The ``raae_block_wgrad_t`` of ``block_wgrad`` (to be launched later, e.g. inside ``block_bwd_b(wgrad=...)``)."""
    a = _lib.BlockWgradT()
    a.n_conv, a.n_lin, a.B, a.slab_stride = len(conv_tasks), len(lin_tasks), B, slab_stride
    for i, (go, cv, view, dw, db) in enumerate(conv_tasks):
        a.conv[i].go, a.conv[i].cv, a.conv[i].inp = go, cv, view
        a.conv[i].dw, a.conv[i].dbias = dw.data_ptr(), db.data_ptr()
    for i, (go, Cc, E, Lin, view, dw, db) in enumerate(lin_tasks):
        a.lin[i].go, a.lin[i].C, a.lin[i].E, a.lin[i].Lin, a.lin[i].inp = go, Cc, E, Lin, view
        a.lin[i].dw, a.lin[i].dbias = dw.data_ptr(), db.data_ptr()
    # algorithmic bytes: every DISTINCT tensor the launch must read counted once (the block input is the
    # operand of up to three tasks -- conv1, conv_short, fc1 -- and is one tensor; VERDICT r2: 74 MB for the last
    # decoder block at 4096 rows, not the 101 MB of the per-task sum) + one slab of weight and bias gradients per task
    uniq = {}
    for go, cv, view, _, _ in conv_tasks:
        uniq[go.g] = 4 * B * cv.Cout * cv.Lout
        uniq[view.raw] = 4 * B * cv.Cin * cv.Lin
        if view.mask:
            uniq[view.mask] = 4 * B * cv.Cin * cv.Lin
    for go, Cc, E, Lin, view, _, _ in lin_tasks:
        uniq[go.g] = 4 * B * Cc * E
        uniq[view.raw] = 4 * B * Cc * Lin
        if view.mask:
            uniq[view.mask] = 4 * B * Cc * Lin
    a.nbytes = sum(uniq.values()) + \
        sum(4 * (cv.Cout * (cv.Cin // cv.groups) * cv.K + cv.Cout) for _, cv, _, _, _ in conv_tasks) + \
        sum(4 * (E * Lin + E) for _, Cc, E, Lin, _, _, _ in lin_tasks)
    if conv_tasks:
        cv = conv_tasks[0][1]
        a.tag = f"{len(conv_tasks)}conv+{len(lin_tasks)}lin {cv.Cin}x{cv.Lin}->{cv.Cout}x{cv.Lout}"
    return a


def block_wgrad(B, conv_tasks, lin_tasks, slab_stride, args=None):
    """``conv_tasks``: [(grad, conv_desc, view, dw, dbias)], ``lin_tasks``: [(grad, C, E, Lin, view, dw, dbias)].
    One launch; returns the slab count per task (conv tasks first)."""
    a = args if args is not None else block_wgrad_args(B, conv_tasks, lin_tasks, slab_stride)

    def launch():
        ns = (C.c_int * 6)()
        check(_lib.load().raae_block_wgrad(C.byref(a), ns, _stream()), "raae_block_wgrad")
        return list(ns)[:a.n_conv + a.n_lin]
    return _probed("wgrad_multi_kernel", a.nbytes, launch, getattr(a, "tag", None))
