"""Every kernel form of the dense (``FC``) layers -- ``raae_dense_fwd_s``, ``raae_dense_bwd_s``, ``raae_dense_fwd2``
(``csrc/raae_dense.hip``) -- against the float64 reference of ``dense_reference``, one launch at a time, bf16
storage and in-kernel dropout multipliers included.

* TEACHER-FORCED: a kernel receives the reference's tensors as its stored inputs, rounded to the storage type (fp32,
  or the bf16 grid where a ``RAAE_ST_*`` bit says so), and float64 partial rows as its input statistics.  Kernel and
  reference read the same values, no PReLU branch can differ and no element is excused.
* HYGIENE, every case: the returned row / slab count lies in 1..RAAE_MAX_PARTS (and is what ``pick_grid`` gives);
  partial rows and slabs beyond it, the unused columns of a slab, and four guard floats after every written tensor
  keep a sentinel; a second identical launch is bitwise equal; running statistics move only when asked.
* bf16 COMPARISON RULE (``ST_Z``): per element ``|got - z64| <= ulp_bf16(z64) / 2 + (2e-5 |z64| + 2e-5)`` -- the
  kernel may land on the neighbouring bf16 value only where fp32 arithmetic is within rounding error of a tie;
  truncation or a bias fails it -- AND at most 1 % of the elements differ from ``round_bf16(z64)``
  (``test_dense_reference_cpu.py`` measures plain fp32 ``F.linear`` at these shapes: under a quarter of that).  A
  softplus output is rounded twice (z, then softplus(z) at the store): the first rounding reaches the stored value
  through a slope <= 1, so its bound carries ``ulp_bf16(z64) / 2`` more.  The emitted ``{sum, sumsq}`` must describe
  the kernel's OWN stored tensor (upcast exactly, statistics recomputed in float64) to 1e-6 of sum |v| and sum v^2:
  one fp32 PReLU product (6e-8) is the only rounding in between; the fp32 cases meet the same check.
* Tolerances otherwise are those ``test_dense_chain_fwd_bwd`` / ``test_block_kernels_gpu.py`` apply: forward tensors
  2e-5 relative + 2e-5; dx 5e-4 + 5e-5; dW / db / dslope 5e-4 + 5e-5 * mean|g| * sqrt(B); dx partial sums 1e-4
  relative + max(1e-3, 5e-5 sqrt(B)); running statistics 1e-4 + 1e-6.  At 2051 rows a parameter gradient may instead
  lie within 3x the distance of fp32 CPU autograd of the same layer from float64, plus the same floor.

INSTANCE -> CASE.  ``fwd_instance`` / ``bwd_instance`` below mirror the dispatch (``prep_dense_fwd`` /
``launch_dense_fwd``, the end of ``raae_dense_bwd_s``); every case names the instance it expects and the table test
fails if the mirror disagrees or an instance is left without a case.  ``ST`` instances run whenever ``storage != 0``.

  forward <KQ, RT, ST>; KQ from K (<= 16: 4, <= 64: 16, <= 256: 64, else 128), RT = 4 from 2048 rows.  <128, 4> is
  not compiled and not dispatched (a 64-row tile of 512 columns does not fit the registers): K = 512 runs RT = 1 at
  every batch.
    <4,1>    f_k6_raw f_k13_bn f_k6_softplus f_k13_relu f_k13_pd     <4,1,ST>    s_m_k13 s_z_relu
    <16,1>   f_k64_bn f_k64_eval f_disc f_k64_pd_softplus f_k64_pd_relu   <16,1,ST>   s_z_k64 s_xmz_k64 s_xm_k64 s_z_softplus
    <64,1>   f_k256_none f_k256_eval f_k256_train                   <64,1,ST>   s_x_k256
    <128,1>  f_k512 f_k512_pd f_k512_big                            <128,1,ST>  s_z_k512
    <4,4>    f_rt4_k6                                               <4,4,ST>    s_z_rt4_k6
    <16,4>   f_rt4_k64                                              <16,4,ST>   s_xmz_rt4_k64
    <64,4>   f_rt4_k256                                             <64,4,ST>   s_xmz_rt4_k256
  paired forward: <64,4> p_256_6; <16,16> p_64_64; the two-launch fallback p_other (K 64 beside K 256) and p_storage.
  backward <TPW, KT4, ST>, from tiles = ceil(N/16) * ceil(kw/16), tpw = ceil(tiles/4), kt4 = ceil(ceil(kw/16)/4),
  kw = 128 for a first layer (IN_NONE, N <= 64, K = 256 | 512), else K:
    <1,1>    b_11 b_11_k13                <1,1,ST>    bs_11_m bs_z_softplus
    <4,1>    b_41 b_41_prelu b_41_big     <4,1,ST>    bs_41_xmz bs_41_z bs_z_relu
    <8,2>    b_82 b_82_nodx b_82_n70 b_82_big   <8,2,ST>    bs_82_z
    <16,1>   b_161 b_161_nodx             <16,1,ST>   bs_161_xm bs_z_softplus_wide
    <16,4>   b_164 b_164_bn               <16,4,ST>   bs_164_x
    <32,1>   b_321 b_321_nodx             <32,1,ST>   bs_321_xm bs_z_softplus_512
    <32,8>   b_328 b_328_relu             <32,8,ST>   bs_328_xmz
  <16,4> and <32,8> are selected by no case of ``test_ops_gpu.py`` (its layers give <1,1>, <4,1>, <8,2>, <16,1>,
  <32,1>); the dispatch reaches both: <16,4> with dx and 5..16 input tiles that are not a first-layer slice (N = 64,
  K = 256 behind a PReLU), <32,8> with dx and K = 512 behind a PReLU.

A FINDING kept here: the narrow (N <= 64) and the 32-tile staging loop of ``dense_bwd_body`` read ``zout`` as fp32 for
``G_SOFTPLUS`` / ``G_RELU`` even with ``RAAE_ST_Z`` (only the 16-tile wide path honoured the bit); ``bs_z_softplus``,
``bs_z_relu`` and ``bs_z_softplus_512`` are its cases.  The engine never combines the two (its last layer is fp32).

The ``_m`` (trial-batched) forms stay with the trial-batch suites, which hold them bitwise to the launches pinned here.
"""
import collections
import ctypes as C
import functools
import zlib

import numpy as np
import pytest
import torch

import dense_reference as dr
from dense_reference import (IN_NONE, IN_PRELU_BN_DROP, IN_PRELU_DROP, OUT_RAW, OUT_STATS_PRELU, OUT_STATS_RAW,
                             OUT_SOFTPLUS, OUT_RELU, G_DIRECT, G_SOFTPLUS, G_PRELU_BN, G_PRELU, G_RELU, ST_X, ST_MASK,
                             ST_Z)

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from rankaae_amd import ops, _lib
    DEV = torch.device("cuda:0")

MAXP = 512                      # RAAE_MAX_PARTS
SENT = -776.0                   # what nothing may overwrite (a bf16 value too)
FLIP_CAP = 0.01                 # share of a bf16 output that may differ from round_bf16(float64)
KEYS = (0x9E3779B1, 0x7F4A7C15)  # arbitrary hash keys written into word 2 of the generator state
BN, PD = IN_PRELU_BN_DROP, IN_PRELU_DROP
XMZ, XM = ST_X | ST_MASK | ST_Z, ST_X | ST_MASK

FwdCase = collections.namedtuple("FwdCase", "name B K N in_kind out_kind inst train mask keep storage offset update")
BwdCase = collections.namedtuple("BwdCase", "name B N K g_kind in_kind inst mask keep storage need_dx offset")


def F_(name, B, K, N, in_kind, out_kind, inst, train=True, mask=None, keep=0.9, storage=0, offset=0, update=True):
    return FwdCase(name, B, K, N, in_kind, out_kind, inst + (storage != 0,), train, mask, keep, storage, offset, update)


def B_(name, B, N, K, g_kind, in_kind, inst, mask=None, keep=0.9, storage=0, need_dx=True, offset=0):
    return BwdCase(name, B, N, K, g_kind, in_kind, inst + (storage != 0,), mask, keep, storage, need_dx, offset)


FWD_CASES = [
    # ---- fp32: every in_kind x out_kind, train and eval BatchNorm, every instance and tail
    F_("f_k6_raw", 37, 6, 64, IN_NONE, OUT_RAW, (4, 1)),
    F_("f_k6_softplus", 5, 6, 256, IN_NONE, OUT_SOFTPLUS, (4, 1)),
    F_("f_k13_relu", 37, 13, 6, IN_NONE, OUT_RELU, (4, 1)),
    F_("f_k13_bn", 37, 13, 70, BN, OUT_STATS_PRELU, (4, 1), mask="t"),
    F_("f_k13_pd", 37, 13, 13, PD, OUT_STATS_RAW, (4, 1), mask="t", keep=0.5),
    F_("f_k64_bn", 256, 64, 64, BN, OUT_STATS_PRELU, (16, 1), mask="t"),
    F_("f_k64_eval", 37, 64, 13, BN, OUT_STATS_RAW, (16, 1), train=False),
    F_("f_disc", 256, 64, 64, PD, OUT_STATS_PRELU, (16, 1), mask="t"),
    F_("f_k64_pd_softplus", 37, 64, 512, PD, OUT_SOFTPLUS, (16, 1), mask="t"),
    F_("f_k64_pd_relu", 5, 64, 6, PD, OUT_RELU, (16, 1)),
    F_("f_k256_none", 256, 256, 64, IN_NONE, OUT_STATS_PRELU, (64, 1)),
    F_("f_k256_eval", 5, 256, 6, BN, OUT_RAW, (64, 1), train=False),
    F_("f_k256_train", 37, 256, 13, BN, OUT_RELU, (64, 1), mask="t"),
    F_("f_k256_noupd", 37, 256, 1, BN, OUT_RAW, (64, 1), update=False),
    F_("f_k512", 37, 512, 64, IN_NONE, OUT_STATS_PRELU, (128, 1)),
    F_("f_k512_pd", 5, 512, 1, PD, OUT_RAW, (128, 1), mask="t"),
    F_("f_k512_big", 2051, 512, 6, IN_NONE, OUT_STATS_RAW, (128, 1)),
    F_("f_rt4_k6", 2051, 6, 64, IN_NONE, OUT_STATS_PRELU, (4, 4)),
    F_("f_rt4_k64", 2051, 64, 256, BN, OUT_SOFTPLUS, (16, 4), mask="t"),
    F_("f_rt4_k256", 2051, 256, 64, IN_NONE, OUT_STATS_PRELU, (64, 4)),
    # ---- bf16 storage: each bit alone, the engine's three combinations, every ST instance
    F_("s_z_k64", 256, 64, 64, BN, OUT_STATS_PRELU, (16, 1), mask="t", storage=ST_Z),
    F_("s_xmz_k64", 37, 64, 64, BN, OUT_STATS_PRELU, (16, 1), mask="t", storage=XMZ),
    F_("s_xm_k64", 256, 64, 512, BN, OUT_SOFTPLUS, (16, 1), mask="t", storage=XM),
    F_("s_x_k256", 37, 256, 70, PD, OUT_STATS_RAW, (64, 1), storage=ST_X),
    F_("s_m_k13", 37, 13, 64, BN, OUT_STATS_PRELU, (4, 1), mask="t", storage=ST_MASK),
    F_("s_z_k512", 37, 512, 64, IN_NONE, OUT_STATS_PRELU, (128, 1), storage=ST_Z),
    F_("s_z_rt4_k6", 2051, 6, 64, IN_NONE, OUT_STATS_PRELU, (4, 4), storage=ST_Z),
    F_("s_xmz_rt4_k64", 2051, 64, 64, BN, OUT_STATS_PRELU, (16, 4), mask="t", storage=XMZ),
    F_("s_xmz_rt4_k256", 2051, 256, 13, PD, OUT_STATS_RAW, (64, 4), mask="t", storage=XMZ),
    F_("s_z_softplus", 37, 64, 13, IN_NONE, OUT_SOFTPLUS, (16, 1), storage=ST_Z),
    F_("s_z_relu", 5, 6, 6, IN_NONE, OUT_RELU, (4, 1), storage=ST_Z),
]

# in-kernel multipliers against the same launch with a host-built tensor (bitwise)
GEN_FWD = [
    F_("g_k64", 37, 64, 64, BN, OUT_STATS_PRELU, (16, 1), mask="g", keep=0.9, offset=1000),
    F_("g_k13", 37, 13, 64, BN, OUT_STATS_PRELU, (4, 1), mask="g", keep=0.5, offset=7),
    F_("g_wrap", 37, 64, 13, PD, OUT_RAW, (16, 1), mask="g", keep=0.9, offset=2 ** 32 - 100),
    F_("g_keep1", 37, 64, 64, BN, OUT_STATS_PRELU, (16, 1), mask="g", keep=1.0, offset=3),
    F_("g_rt4", 2051, 64, 64, BN, OUT_STATS_PRELU, (16, 4), mask="g", keep=0.5, offset=2 ** 32 - 100),
    F_("g_rt4_k13", 2051, 13, 6, PD, OUT_RAW, (4, 4), mask="g", keep=0.9, offset=12),
    F_("g_bf16", 37, 64, 64, BN, OUT_STATS_PRELU, (16, 1), mask="g", keep=0.9, offset=5, storage=ST_X | ST_Z),
]

BWD_CASES = [
    B_("b_11", 37, 6, 6, G_DIRECT, IN_NONE, (1, 1)),
    B_("b_11_k13", 37, 13, 13, G_PRELU_BN, BN, (1, 1), mask="t", keep=0.5),
    B_("b_41", 256, 64, 64, G_PRELU_BN, BN, (4, 1), mask="t"),
    B_("b_41_prelu", 37, 64, 64, G_PRELU, PD, (4, 1), mask="t"),
    B_("b_41_big", 2051, 64, 64, G_PRELU_BN, BN, (4, 1), mask="t"),
    B_("b_82", 256, 64, 256, G_PRELU_BN, IN_NONE, (8, 2)),
    B_("b_82_nodx", 37, 13, 512, G_PRELU_BN, IN_NONE, (8, 2), need_dx=False),
    B_("b_82_n70", 37, 70, 64, G_PRELU_BN, BN, (8, 2)),
    B_("b_82_big", 2051, 64, 256, G_PRELU_BN, IN_NONE, (8, 2)),
    B_("b_161", 37, 256, 64, G_SOFTPLUS, BN, (16, 1), mask="t"),
    B_("b_161_nodx", 5, 64, 256, G_PRELU, PD, (16, 1), need_dx=False),
    B_("b_164", 37, 64, 256, G_PRELU_BN, PD, (16, 4), mask="t"),
    B_("b_164_bn", 256, 13, 256, G_DIRECT, BN, (16, 4), mask="t"),
    B_("b_321", 37, 512, 64, G_SOFTPLUS, BN, (32, 1), mask="t"),
    B_("b_321_nodx", 37, 64, 512, G_PRELU_BN, PD, (32, 1), need_dx=False),
    B_("b_328", 37, 64, 512, G_DIRECT, PD, (32, 8), mask="t"),
    B_("b_328_relu", 256, 13, 512, G_RELU, PD, (32, 8)),
    # ---- bf16 storage
    B_("bs_11_m", 37, 6, 13, G_PRELU_BN, BN, (1, 1), mask="t", storage=ST_MASK),
    B_("bs_41_xmz", 256, 64, 64, G_PRELU_BN, BN, (4, 1), mask="t", storage=XMZ),
    B_("bs_41_z", 37, 64, 64, G_PRELU_BN, BN, (4, 1), mask="t", storage=ST_Z),
    B_("bs_82_z", 37, 64, 256, G_PRELU_BN, IN_NONE, (8, 2), storage=ST_Z),
    B_("bs_161_xm", 37, 256, 64, G_SOFTPLUS, BN, (16, 1), mask="t", storage=XM),
    B_("bs_164_x", 37, 64, 256, G_DIRECT, PD, (16, 4), storage=ST_X),
    B_("bs_321_xm", 37, 512, 64, G_SOFTPLUS, BN, (32, 1), mask="t", storage=XM),
    B_("bs_328_xmz", 37, 64, 512, G_PRELU, PD, (32, 8), mask="t", storage=XMZ),
    B_("bs_z_softplus", 37, 13, 64, G_SOFTPLUS, BN, (1, 1), storage=ST_Z),
    B_("bs_z_relu", 37, 64, 64, G_RELU, BN, (4, 1), storage=ST_Z),
    B_("bs_z_softplus_wide", 37, 256, 64, G_SOFTPLUS, BN, (16, 1), storage=ST_Z),
    B_("bs_z_softplus_512", 37, 512, 64, G_SOFTPLUS, BN, (32, 1), storage=ST_Z),
]

GEN_BWD = [
    B_("gb_k64", 37, 64, 64, G_PRELU_BN, BN, (4, 1), mask="g", keep=0.9, offset=1000),
    B_("gb_k13", 37, 6, 13, G_DIRECT, PD, (1, 1), mask="g", keep=0.5, offset=7),
    B_("gb_wrap", 2051, 64, 64, G_PRELU_BN, BN, (4, 1), mask="g", keep=0.9, offset=2 ** 32 - 100),
    B_("gb_keep1", 37, 13, 64, G_DIRECT, BN, (1, 1), mask="g", keep=1.0, offset=2 ** 32 - 100),
]


# ------------------------------------------------------------------------------------- the dispatch, mirrored
def pick_grid(B, rt=1):
    ntiles = (B + 16 * rt - 1) // (16 * rt)
    return min(ntiles, max(64, min(MAXP, ntiles // 8)))


def fwd_instance(B, K):
    K4 = (K + 3) & ~3
    kq = 4 if K4 <= 16 else 16 if K4 <= 64 else 64 if K4 <= 256 else 128
    return kq, (4 if B >= 2048 and kq <= 64 else 1)


def bwd_instance(N, K, in_kind, need_dx):
    kw = 128 if (in_kind == IN_NONE and N <= 64 and K >= 256 and K % 128 == 0) else K
    nt, kt = (N + 15) // 16, (kw + 15) // 16
    tpw, kt4 = (nt * kt + 3) // 4, (kt + 3) // 4
    for t, k in ((1, 1), (4, 1), (8, 2), (16, 1), (16, 4), (32, 1), (32, 8)):
        if tpw <= t and (kt4 <= k or (k == 1 and t >= 16 and not need_dx)):
            return t, k
    return None


def bwd_grid(B, N, K):
    gx = pick_grid(B)
    return min(gx, 64) if N * K >= 8192 else gx


def test_case_table_reaches_every_instance():
    """The docstring's map: the mirrored dispatch gives every case the instance it names, and every forward, backward
    and storage instance the dispatch can select has a case; so has every in_kind x out_kind and every g_kind."""
    for c in FWD_CASES + GEN_FWD:
        assert fwd_instance(c.B, c.K) == c.inst[:2], c
    for c in BWD_CASES + GEN_BWD:
        assert bwd_instance(c.N, c.K, c.in_kind, c.need_dx) == c.inst[:2], c
    fwd_all = {(kq, rt, st) for kq in (4, 16, 64, 128) for rt in (1, 4) for st in (False, True)} - {(128, 4, False), (128, 4, True)}
    assert {c.inst for c in FWD_CASES} == fwd_all
    assert all(fwd_instance(B, 512)[1] == 1 for B in (2048, 2051, 1 << 20))         # <128, 4> cannot be selected
    bwd_all = {(t, k, st) for t, k in ((1, 1), (4, 1), (8, 2), (16, 1), (16, 4), (32, 1), (32, 8)) for st in (False, True)}
    assert {c.inst for c in BWD_CASES} == bwd_all
    assert {(c.in_kind, c.out_kind) for c in FWD_CASES if not c.storage} == {(i, o) for i in range(3) for o in range(5)}
    assert {c.g_kind for c in BWD_CASES if not c.storage} == set(range(5))
    assert {c.storage for c in FWD_CASES} >= {0, ST_X, ST_MASK, ST_Z, XMZ, XM}
    assert {c.storage for c in BWD_CASES} >= {0, ST_X, ST_MASK, ST_Z, XMZ, XM}
    names = [c.name for c in FWD_CASES + GEN_FWD + BWD_CASES + GEN_BWD]
    assert len(names) == len(set(names))


# ------------------------------------------------------------------------------------- case data (CPU, cached)
def _gen(name):
    return torch.Generator().manual_seed(zlib.crc32(name.encode()))


def _f32(t):
    return t.float().double()


def _common(c, g):
    """Inputs both directions share: x on its storage grid, parameters, multipliers, input statistics."""
    t = {}
    x = _f32(torch.randn(c.B, c.K, generator=g) * 1.5 + 0.2)
    t["x"] = dr.round_bf16(x) if c.storage & ST_X else x
    t["w"] = _f32(torch.randn(c.N, c.K, generator=g) / c.K ** 0.5)
    t["bias"] = _f32(torch.randn(c.N, generator=g) * 0.1)
    t["slope"] = _f32(torch.rand(c.K, generator=g) * 0.5 - 0.1)              # some negative
    t["out_slope"] = _f32(torch.rand(c.N, generator=g) * 0.5 - 0.1)
    t["flags"], t["inv"], t["mult"] = None, 1.0, None
    if c.mask is not None and c.in_kind != IN_NONE:
        thr, inv = dr.gen_params(c.keep)
        if c.mask == "g":
            flags = torch.from_numpy(dr.mask_hash(KEYS[0], KEYS[1], c.offset, thr, c.B * c.K)).view(c.B, c.K)
        else:
            flags = torch.rand(c.B, c.K, generator=g) < c.keep
        t["flags"], t["inv"] = flags.double(), float(inv)
        t["mult"] = t["flags"] * float(inv)
    t["rows"] = None
    if c.in_kind == BN:
        a = dr.prelu(t["x"], t["slope"])
        t["rows"] = dr.partial_rows([a, a * a], nrows=min(3, c.B))
    t["running"] = (_f32(torch.randn(c.K, generator=g) * 0.3), _f32(torch.rand(c.K, generator=g) + 0.5))
    return t


@functools.lru_cache(maxsize=None)
def make_fwd(c):
    t = _common(c, _gen(c.name))
    train = c.train and c.in_kind == BN
    t["ref"] = dr.fwd(t["x"], t["w"], t["bias"], in_kind=c.in_kind, slope=t["slope"],
                      rows=t["rows"] if train else None, count=c.B, running=t["running"], mult=t["mult"],
                      out_kind=c.out_kind, out_slope=t["out_slope"], storage=c.storage)
    return t


@functools.lru_cache(maxsize=None)
def make_bwd(c):
    g = _gen(c.name)
    t = _common(c, g)
    out_kind = {G_SOFTPLUS: OUT_SOFTPLUS, G_RELU: OUT_RELU}.get(c.g_kind, OUT_RAW)
    f = dr.fwd(t["x"], t["w"], t["bias"], in_kind=c.in_kind, slope=t["slope"], rows=t["rows"], count=c.B, mult=t["mult"],
               out_kind=out_kind, storage=c.storage & ST_Z)
    t["zout"] = f["stored"] if c.storage & ST_Z else _f32(f["stored"])
    t["g"] = _f32(torch.randn(c.B, c.N, generator=g))
    t["out_rows"] = t["g_rows"] = None
    if c.g_kind == G_PRELU_BN:
        a = dr.prelu(t["zout"], t["out_slope"])
        t["out_rows"] = dr.partial_rows([a, a * a], nrows=2)
        mean, rstd, _ = dr.bn_from_rows(t["out_rows"], c.B)
        t["g_rows"] = dr.partial_rows([t["g"], t["g"] * (a - mean) * rstd], nrows=min(3, c.B))
    t["ref"] = dr.bwd(t["g"], c.g_kind, t["x"], t["w"], zout=t["zout"], out_slope=t["out_slope"], out_rows=t["out_rows"],
                      g_rows=t["g_rows"], count=c.B, in_kind=c.in_kind, slope=t["slope"], rows=t["rows"], mult=t["mult"],
                      need_dx=c.need_dx)
    t["arbiter"] = None
    if c.B >= 2048:         # fp32 CPU autograd of the same layer: the arbiter of the long gradient sums
        has = c.g_kind in (G_PRELU, G_PRELU_BN)
        t["arbiter"] = dr.layer_autograd(t["g"], c.g_kind, t["x"], t["w"], t["bias"], t["out_slope"] if has else None,
                                         c.in_kind, t["slope"], t["mult"], dtype=torch.float32)[:3]
    return t


# ------------------------------------------------------------------------------------- device plumbing
class Report:
    """Collects every comparison of a case: prints the largest error per quantity as a share of its bound, asserts
    once at the end."""

    def __init__(self, case):
        self.case, self.bad = case, []

    def bound(self, what, got, want, tol, arbiter=None, atol=0.0):
        got, want = got.detach().double().cpu(), want.detach().double().cpu()
        assert got.shape == want.shape, (self.case, what, got.shape, want.shape)
        err = (got - want).abs()
        finite = bool(torch.isfinite(got).all())
        worst = float(err.max()) if finite else float("inf")
        ratio = float((err / tol).max()) if finite else float("inf")
        ok, note = finite and ratio <= 1.0, ""
        if not ok and finite and arbiter is not None:
            e_ref = float((arbiter.detach().double().cpu() - want).abs().max())
            ok = worst <= 3.0 * e_ref + atol
            note = f"  arbiter: fp32 autograd is {e_ref:.3e} from float64 -> {'ok' if ok else 'FAIL'}"
        print(f"ERR {self.case} {what}: max err {worst:.3e} (max |ref| {float(want.abs().max()):.3e}), "
              f"{ratio:.3f} of the bound{note}")
        if not ok:
            i = int(torch.nan_to_num(err / tol, nan=float("inf")).argmax())
            self.bad.append(f"{what}: max err {worst:.3e} = {ratio:.2f} x bound at flat index {i}: "
                            f"ref {float(want.flatten()[i]):.6e} got {float(got.flatten()[i]):.6e}{note}")

    def close(self, what, got, want, rtol, atol, arbiter=None):
        self.bound(what, got, want, atol + rtol * want.detach().double().cpu().abs(), arbiter, atol)

    def share(self, what, value, cap):
        print(f"ERR {self.case} {what}: {value:.5f}, {value / cap:.3f} of the bound")
        if not value <= cap:
            self.bad.append(f"{what}: {value:.5f} > {cap}")

    def check(self, cond, what):
        if not cond:
            self.bad.append(what)

    def done(self):
        assert not self.bad, f"{self.case}:\n" + "\n".join(self.bad)


class Buf:
    """A device tensor all sentinel, with four guard floats (16 bytes) behind it."""

    def __init__(self, shape, dtype=torch.float32):
        self.n = int(np.prod(shape))
        self.whole = torch.full((self.n + 16 // torch.empty(0, dtype=dtype).element_size(),), SENT, dtype=dtype, device=DEV)
        self.t = self.whole[:self.n].view(*shape)

    def guard_ok(self):
        return bool((self.whole[self.n:] == SENT).all())

    def snap(self):
        return self.whole.clone()


def _dev(t, dtype=torch.float32):
    return None if t is None else t.to(dtype).contiguous().to(DEV)


def _state():
    """The engine's {counter, seed, keys} words with arbitrary keys in word 2."""
    word = KEYS[0] | (KEYS[1] << 32)
    return torch.tensor([5, 99, word - (1 << 64) if word >= 1 << 63 else word], dtype=torch.int64, device=DEV)


def _rows_dev(rows, C_):
    """Partial rows as a producer leaves them: the first rows of a RAAE_MAX_PARTS buffer, sentinel behind."""
    buf = torch.full((MAXP, C_, 2), SENT, dtype=torch.float64, device=DEV)
    buf[:rows.shape[0]] = rows.to(DEV)
    return buf, rows.shape[0]


def _mask_args(c, t, mode):
    """(mask tensor, mask_scale, gen) of a launch.  mode: "t" fp32 {0, 1/keep} or, under ST_MASK, bf16 {0, 1} times
    mask_scale; "g": generated in the kernel."""
    if t["flags"] is None:
        return None, 1.0, None
    if mode == "g":
        return None, 1.0, (_state(), c.offset, c.keep)
    if c.storage & ST_MASK:
        return _dev(t["flags"], torch.bfloat16), t["inv"], None
    return _dev(t["mult"]), 1.0, None


class FwdRun:
    """One forward launch of a case on fresh buffers; ``mode`` overrides where the multipliers come from."""

    def __init__(self, c, t, mode=None, mask_override=None):
        self.c, self.t = c, t
        self.x = _dev(t["x"], torch.bfloat16 if c.storage & ST_X else torch.float32)
        self.w, self.bias, self.slope, self.oslope = map(_dev, (t["w"], t["bias"], t["slope"], t["out_slope"]))
        self.z = Buf((c.B, c.N), torch.bfloat16 if c.storage & ST_Z else torch.float32)
        self.parts = Buf((MAXP, c.N, 2), torch.float64)
        self.rm, self.rv = Buf((c.K,)), Buf((c.K,))
        self.reset_running()
        self.bn = None
        if c.in_kind == BN:
            if c.train:
                self.rows, n = _rows_dev(t["rows"], c.K)
                self.bn = ops.make_bn(self.rows, n, c.B, self.rm.t, self.rv.t, update_running=c.update)
            else:
                self.bn = ops.make_bn(None, 0, 0, self.rm.t, self.rv.t)
        self.mask, self.scale, self.gen = mask_override or _mask_args(c, t, mode or c.mask)
        stats = c.out_kind in (OUT_STATS_PRELU, OUT_STATS_RAW)
        self.args = ops.dense_fwd_args(self.x, c.B, c.K, c.in_kind, self.slope if c.in_kind != IN_NONE else None, self.bn,
                                       self.mask, self.w, self.bias, c.N, self.z.t, c.out_kind,
                                       self.oslope if c.out_kind == OUT_STATS_PRELU else None,
                                       self.parts.t if stats else None, storage=c.storage, mask_scale=self.scale,
                                       gen=self.gen)

    def reset_running(self):
        self.rm.t.copy_(self.t["running"][0])
        self.rv.t.copy_(self.t["running"][1])

    def launch(self):
        self.n = ops.dense_fwd_struct(self.args)
        torch.cuda.synchronize()
        return self.snaps()

    def snaps(self):
        return [b.snap() for b in (self.z, self.parts, self.rm, self.rv)]


def _same(a, b):
    return all(torch.equal(u.view(torch.uint8), v.view(torch.uint8)) for u, v in zip(a, b))


def _check_fwd(c, t, run, rep):
    ref = t["ref"]
    first = run.launch()
    n = run.n
    rep.check(1 <= n <= MAXP and n == pick_grid(c.B, c.inst[1]), f"nparts {n}, pick_grid {pick_grid(c.B, c.inst[1])}")
    got = run.z.t.double().cpu()
    fp = 2e-5 * ref["raw"].abs() + 2e-5
    if c.storage & ST_Z:
        tol = dr.ulp_bf16(ref["raw"]) / 2 + fp
        if c.out_kind == OUT_SOFTPLUS:
            tol = tol + dr.ulp_bf16(ref["z_raw"]) / 2          # the first rounding, through a slope <= 1
        rep.bound("z (bf16)", got, ref["raw"], tol)
        rep.share("bf16 flips", float((got != ref["stored"]).double().mean()), FLIP_CAP)
    else:
        rep.bound("z", got, ref["stored"], fp)
    stats = c.out_kind in (OUT_STATS_PRELU, OUT_STATS_RAW)
    rows = run.parts.t.cpu()
    if stats:
        # the statistics describe what was stored: recomputed in float64 from the kernel's own tensor
        v = dr.prelu(got, t["out_slope"]) if c.out_kind == OUT_STATS_PRELU else got
        tot = rows[:n].sum(0)
        rep.bound("sum of own z", tot[:, 0], v.sum(0), 1e-6 * v.abs().sum(0) + 1e-300)
        rep.bound("sumsq of own z", tot[:, 1], (v * v).sum(0), 1e-6 * (v * v).sum(0) + 1e-300)
        if not c.storage & ST_Z:
            rep.close("{sum, sumsq}", tot, ref["stats"], 1e-5, max(1e-3, 5e-5 * c.B ** 0.5))
    rep.check(bool((rows[n if stats else 0:] == SENT).all()), "partial rows beyond nparts (or all, without statistics) touched")
    rep.check(run.z.guard_ok() and run.parts.guard_ok() and run.rm.guard_ok() and run.rv.guard_ok(), "a guard was overwritten")
    moved = c.in_kind == BN and c.train and c.update
    if moved:
        rep.close("running_mean", run.rm.t, ref["running"][0], 1e-4, 1e-6)
        rep.close("running_var", run.rv.t, ref["running"][1], 1e-4, 1e-6)
    else:
        rep.check(torch.equal(run.rm.t.cpu().double(), t["running"][0]) and
                  torch.equal(run.rv.t.cpu().double(), t["running"][1]), "running statistics moved")
    run.reset_running()
    rep.check(_same(first, run.launch()), "second identical launch differs")
    return first


@pytest.mark.parametrize("c", FWD_CASES, ids=lambda c: c.name)
def test_forward(c):
    """(a) fp32 and (b) bf16 forward of every instance against the float64 reference, with the hygiene checks."""
    t = make_fwd(c)
    rep = Report(c.name)
    _check_fwd(c, t, FwdRun(c, t), rep)
    rep.done()


# ------------------------------------------------------------------------------------- backward
class BwdRun:
    def __init__(self, c, t, mode=None, mask_override=None):
        self.c, self.t = c, t
        r64 = lambda v: (v + 63) // 64 * 64
        self.o_db = r64(c.N * c.K)
        self.o_ds = self.o_db + r64(c.N)
        self.stride = self.o_ds + r64(c.N)
        self.x = _dev(t["x"], torch.bfloat16 if c.storage & ST_X else torch.float32)
        self.zout = _dev(t["zout"], torch.bfloat16 if c.storage & ST_Z else torch.float32)
        self.g, self.w, self.slope, self.oslope = map(_dev, (t["g"], t["w"], t["slope"], t["out_slope"]))
        self.slabs = Buf((MAXP, self.stride))
        self.dx = Buf((c.B, c.K))
        self.dxp = Buf((MAXP, c.K, 2), torch.float64)
        self.has_slope = c.g_kind in (G_PRELU, G_PRELU_BN)
        self.out_bn, self.g_rows, self.g_n = None, None, 0
        if c.g_kind == G_PRELU_BN:
            self.out_rows, n = _rows_dev(t["out_rows"], c.N)
            self.out_bn = ops.make_bn(self.out_rows, n, c.B)
            self.g_rows, self.g_n = _rows_dev(t["g_rows"], c.N)
        self.bn = None
        if c.in_kind == BN:
            self.rows, n = _rows_dev(t["rows"], c.K)
            self.bn = ops.make_bn(self.rows, n, c.B)
        self.mask, self.scale, self.gen = mask_override or _mask_args(c, t, mode or c.mask)

    def launch(self):
        c, s = self.c, self.slabs.t
        self.n = ops.dense_bwd(self.g, c.g_kind, self.g_rows, self.g_n, self.zout if c.g_kind != G_DIRECT else None,
                               self.oslope if self.has_slope else None, self.out_bn, c.B, c.N, self.x, c.K, c.in_kind,
                               self.slope if c.in_kind != IN_NONE else None, self.bn, self.mask, self.w,
                               s[0, 0:], s[0, self.o_db:], s[0, self.o_ds:] if self.has_slope else None, self.stride,
                               self.dx.t if c.need_dx else None, self.dxp.t if c.need_dx else None,
                               storage=c.storage, mask_scale=self.scale, gen=self.gen)
        torch.cuda.synchronize()
        return [b.snap() for b in (self.slabs, self.dx, self.dxp)]


def _check_bwd(c, t, run, rep):
    ref, arb = t["ref"], t["arbiter"] or (None, None, None)
    first = run.launch()
    n = run.n
    rep.check(1 <= n <= MAXP and n == bwd_grid(c.B, c.N, c.K), f"nslab {n}, expected {bwd_grid(c.B, c.N, c.K)}")
    s = run.slabs.t.cpu()
    floor = 5e-5 * float(t["g"].abs().mean()) * c.B ** 0.5
    NK = c.N * c.K
    rep.close("dW", s[:n, :NK].double().sum(0).view(c.N, c.K), ref["dw"], 5e-4, floor, arb[0])
    rep.close("db", s[:n, run.o_db:run.o_db + c.N].double().sum(0), ref["db"], 5e-4, floor, arb[1])
    used = torch.zeros(run.stride, dtype=torch.bool)
    used[:NK] = True
    used[run.o_db:run.o_db + c.N] = True
    if run.has_slope:
        rep.close("dslope", s[:n, run.o_ds:run.o_ds + c.N].double().sum(0), ref["dslope"], 5e-4, floor, arb[2])
        used[run.o_ds:run.o_ds + c.N] = True
    rep.check(bool((s[n:] == SENT).all()), "slabs beyond nslab touched")
    rep.check(bool((s[:n][:, ~used] == SENT).all()), "columns of a slab outside dW / db / dslope touched")
    rep.check(not bool((s[:n][:, used] == SENT).any()), "an element of a slab was left unwritten")
    dxp = run.dxp.t.cpu()
    if c.need_dx:
        rep.close("dx", run.dx.t, ref["dx"], 5e-4, 5e-5)
    else:
        rep.check(bool((run.dx.t == SENT).all()), "dx written without being asked for")
    if c.need_dx and c.in_kind == BN:
        tot = dxp[:n].sum(0)
        rep.close("dx partial sums", tot, ref["dx_stats"], 1e-4, max(1e-3, 5e-5 * c.B ** 0.5))
        own = run.dx.t.double().cpu()
        rep.bound("sum of own dx", tot[:, 0], own.sum(0), 1e-6 * own.abs().sum(0) + 1e-300)
        rep.check(bool((dxp[n:] == SENT).all()), "dx partial rows beyond nslab touched")
    else:
        rep.check(bool((dxp == SENT).all()), "dx partial rows written without a BatchNorm to feed")
    rep.check(run.slabs.guard_ok() and run.dx.guard_ok() and run.dxp.guard_ok(), "a guard was overwritten")
    rep.check(_same(first, run.launch()), "second identical launch differs")
    return first


@pytest.mark.parametrize("c", BWD_CASES, ids=lambda c: c.name)
def test_backward(c):
    """(a) fp32 and (b) bf16 backward of every instance and g_kind, dx given and NULL."""
    t = make_bwd(c)
    rep = Report(c.name)
    _check_bwd(c, t, BwdRun(c, t), rep)
    rep.done()


# ------------------------------------------------------------------------------------- (b) bf16 masks, consumers
def test_bf16_mask_is_the_scaled_fp32_mask():
    """A bf16 {0, 1} mask with mask_scale = s is bitwise the fp32 mask {0, s}, forward and backward (K % 4 == 0: at4,
    K = 13: at); mask_scale = 0 is read as 1."""
    rep = Report("bf16_mask")
    for K in (64, 13):
        c = F_(f"m_fwd_k{K}", 37, K, 64, BN, OUT_STATS_PRELU, fwd_instance(37, K), mask="t", keep=0.8, storage=ST_MASK)
        t = make_fwd(c)
        s = t["inv"]
        bf = FwdRun(c, t).launch()
        c0 = c._replace(storage=0, inst=c.inst[:2] + (False,))
        rep.check(_same(bf, FwdRun(c0, t).launch()), f"forward K {K}: bf16 mask x scale differs from the fp32 mask")
        flags = _dev(t["flags"], torch.bfloat16)
        one = FwdRun(c, t, mask_override=(flags, 0.0, None)).launch()
        rep.check(_same(one, FwdRun(c0, t, mask_override=(_dev(t["flags"]), 1.0, None)).launch()),
                  f"forward K {K}: mask_scale 0 is not read as 1")
        rep.check(not _same(one, bf) and abs(s - 1.25) < 1e-6, "the scale made no difference")
        b = B_(f"m_bwd_k{K}", 37, 64, K, G_PRELU_BN, BN, bwd_instance(64, K, BN, True), mask="t", keep=0.8, storage=ST_MASK)
        tb = make_bwd(b)
        b0 = b._replace(storage=0, inst=b.inst[:2] + (False,))
        bfb = BwdRun(b, tb).launch()
        rep.check(_same(bfb, BwdRun(b0, tb).launch()), f"backward K {K}: bf16 mask x scale differs from the fp32 mask")
        oneb = BwdRun(b, tb, mask_override=(_dev(tb["flags"], torch.bfloat16), 0.0, None)).launch()
        rep.check(_same(oneb, BwdRun(b0, tb, mask_override=(_dev(tb["flags"]), 1.0, None)).launch()),
                  f"backward K {K}: mask_scale 0 is not read as 1")
    rep.done()


def test_bf16_consumers_read_the_producers_tensor():
    """A bf16 producer's consumers -- the next layer's forward, both backwards -- are fed the KERNEL's own bf16 tensor
    and partial rows; their reference reads the same values, so the fp32 tolerances hold with no bf16 allowance."""
    rep = Report("bf16_chain")
    B, K, H, N = 256, 64, 64, 13
    p = F_("c_prod", B, K, H, BN, OUT_STATS_PRELU, (16, 1), mask="t", storage=ST_Z)
    tp = make_fwd(p)
    prod = FwdRun(p, tp)
    prod.launch()
    z = prod.z.t.clone()                                   # bf16, the kernel's own
    rows = prod.parts.t[:prod.n].cpu()
    # ---- the next layer's forward reads z as ST_X
    q = F_("c_cons", B, H, N, BN, OUT_STATS_RAW, (16, 1), mask="t", storage=XM)
    tq = dict(_common(q, _gen(q.name)))
    tq["x"], tq["slope"], tq["rows"] = z.double().cpu(), tp["out_slope"], rows
    tq["ref"] = dr.fwd(tq["x"], tq["w"], tq["bias"], in_kind=BN, slope=tq["slope"], rows=rows, count=B,
                       running=tq["running"], mult=tq["mult"], out_kind=OUT_STATS_RAW, storage=XM)
    _check_fwd(q, tq, FwdRun(q, tq), rep)
    # ---- its backward (x = z: ST_X), then the producer's own backward (zout = z: ST_Z)
    g = _gen("c_bwd")
    bq = B_("c_cons_bwd", B, N, H, G_DIRECT, BN, (1, 1), mask="t", storage=XM)
    tb = dict(tq, g=_f32(torch.randn(B, N, generator=g)), zout=None, arbiter=None)
    tb["ref"] = dr.bwd(tb["g"], G_DIRECT, tb["x"], tb["w"], count=B, in_kind=BN, slope=tb["slope"], rows=rows, mult=tb["mult"])
    run = BwdRun(bq, tb)
    _check_bwd(bq, tb, run, rep)
    dx, dxrows = run.dx.t.double().cpu(), run.dxp.t[:run.n].cpu()
    bp = B_("c_prod_bwd", B, H, K, G_PRELU_BN, BN, (4, 1), mask="t", storage=ST_Z)
    tpb = dict(tp, g=dx, zout=z.double().cpu(), out_rows=rows, g_rows=dxrows, arbiter=None)
    tpb["ref"] = dr.bwd(dx, G_PRELU_BN, tp["x"], tp["w"], zout=tpb["zout"], out_slope=tp["out_slope"], out_rows=rows,
                        g_rows=dxrows, count=B, in_kind=BN, slope=tp["slope"], rows=tp["rows"], mult=tp["mult"])
    _check_bwd(bp, tpb, BwdRun(bp, tpb), rep)
    rep.done()


# ------------------------------------------------------------------------------------- (c) in-kernel multipliers
@pytest.mark.parametrize("c", GEN_FWD, ids=lambda c: c.name)
def test_generated_multipliers_forward(c):
    """``gen=`` (keys in word 2 of the state, slot offset, keep) is bitwise ``mask=`` of the tensor ``mask_hash`` builds
    on the host; and both meet the reference."""
    t = make_fwd(c)
    rep = Report(c.name)
    assert c.B * c.K > 100 and 0.0 < float(t["flags"].mean()) <= 1.0
    gen = _check_fwd(c, t, FwdRun(c, t, "g"), rep)
    rep.check(_same(gen, FwdRun(c, t, "t").launch()), "generated multipliers differ from the host-built tensor")
    rep.done()


@pytest.mark.parametrize("c", GEN_BWD, ids=lambda c: c.name)
def test_generated_multipliers_backward(c):
    t = make_bwd(c)
    rep = Report(c.name)
    gen = _check_bwd(c, t, BwdRun(c, t, "g"), rep)
    rep.check(_same(gen, BwdRun(c, t, "t").launch()), "generated multipliers differ from the host-built tensor")
    rep.done()


def test_rng_fill_masks_are_the_hash():
    """``raae_rng_fill`` kind 1 ({0, 1/keep} floats) and kind 2 (bf16 {0, 1} flags, two per float) at a hash offset,
    bitwise ``mask_hash`` with the keys ``raae_step_tick`` stored for that seed and counter."""
    seed, ctr0, n1, n2, off1, off2 = 0x1234567890ABCDEF, 41, 4096 + 8, 2048, 1000, 2 ** 31 + 12344
    state = torch.tensor([ctr0, seed, 0], dtype=torch.int64, device=DEV)
    ops.step_tick(torch.zeros(1, dtype=torch.int32, device=DEV), 1, 0, state, None, 0)
    st = state.cpu().numpy().view(np.uint32)
    assert int(state[0]) == ctr0 + 1
    k1, k2 = int(st[4]), int(st[5])
    assert (k1, k2) == dr.step_keys(seed, ctr0 + 1)
    desc = torch.tensor([[0, n1, 1, off1], [n1, n2, 2, off2 - 2 ** 32]], dtype=torch.int32, device=DEV)
    scale = torch.tensor([0.9, 0.5], device=DEV)
    tape = Buf((n1 + n2,))
    ops.rng_fill(tape.t, desc, scale, 2, n1 + n2, seed, state)
    torch.cuda.synchronize()
    thr, inv = dr.gen_params(0.9)
    want1 = torch.from_numpy(dr.mask_hash(k1, k2, off1, thr, n1).astype(np.float32) * inv)
    assert torch.equal(tape.t[:n1].cpu(), want1)
    thr, _ = dr.gen_params(0.5)
    want2 = torch.from_numpy(dr.mask_hash(k1, k2, off2, thr, 2 * n2).astype(np.float32)).to(torch.bfloat16)
    assert torch.equal(tape.t[n1:].view(torch.bfloat16).cpu().view(torch.int16), want2.view(torch.int16))
    assert tape.guard_ok()


# ------------------------------------------------------------------------------------- (d) raae_dense_fwd2
PAIRS = [
    ("p_256_6", F_("p_a", 37, 256, 64, IN_NONE, OUT_STATS_PRELU, (64, 1)), F_("p_b", 256, 6, 64, IN_NONE, OUT_STATS_PRELU, (4, 1))),
    ("p_64_64", F_("p_c", 37, 64, 64, BN, OUT_STATS_PRELU, (16, 1), mask="t"), F_("p_d", 256, 64, 70, BN, OUT_STATS_RAW, (16, 1), mask="g", offset=9)),
    ("p_other", F_("p_e", 37, 64, 13, BN, OUT_SOFTPLUS, (16, 1), mask="t"), F_("p_f", 256, 256, 64, IN_NONE, OUT_STATS_PRELU, (64, 1))),
    ("p_storage", F_("p_g", 37, 64, 64, BN, OUT_STATS_PRELU, (16, 1), mask="t", storage=XMZ), F_("p_h", 256, 64, 64, BN, OUT_STATS_PRELU, (16, 1), mask="t")),
]


@pytest.mark.parametrize("name,p,q", PAIRS, ids=[x[0] for x in PAIRS])
def test_pair_is_the_two_single_launches(name, p, q):
    """``raae_dense_fwd2`` -- both fused instances, a pair without an instance and a pair with a storage bit (two
    launches inside) -- is bitwise the two ``raae_dense_fwd_s`` launches: z, partial rows, counts, running statistics."""
    tp, tq = make_fwd(p), make_fwd(q)
    rep = Report(name)
    a, b = FwdRun(p, tp), FwdRun(q, tq)
    single = a.launch() + b.launch()
    _check_fwd(p, tp, FwdRun(p, tp), rep)
    a2, b2 = FwdRun(p, tp), FwdRun(q, tq)
    n1, n2 = ops.dense_fwd_pair(a2.args, b2.args)
    torch.cuda.synchronize()
    rep.check((n1, n2) == (a.n, b.n) and 1 <= n1 <= MAXP and 1 <= n2 <= MAXP, f"counts {(n1, n2)} against {(a.n, b.n)}")
    rep.check(_same(single, a2.snaps() + b2.snaps()), "the pair differs from the two single launches")
    n1, n2 = ops.dense_fwd_pair(b2.args, a2.args)          # the other order runs no fused instance for p_256_6
    rep.check((n2, n1) == (a.n, b.n), "counts of the swapped pair")
    rep.done()


# ------------------------------------------------------------------------------------- (e) argument rejections
def _fwd_rc(args):
    n = C.c_int(-5)
    rc = _lib.load().raae_dense_fwd_s(C.byref(args), C.byref(n), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc


def test_forward_rejections_touch_nothing():
    rep = Report("fwd_einval")

    def expect(what, c, mutate=None, mode=None):
        t = make_fwd(c)
        run = FwdRun(c, t, mode)
        if mutate:
            mutate(run)
        before = run.snaps()
        rep.check(_fwd_rc(run.args) == -1, f"{what}: not RAAE_EINVAL")
        rep.check(_same(before, run.snaps()) and bool((run.z.whole == SENT).all()) and
                  bool((run.parts.whole == SENT).all()), f"{what}: an output was written")

    expect("ST_X with K % 4 != 0", F_("r_x13", 37, 13, 6, PD, OUT_STATS_RAW, (4, 1), storage=ST_X))
    expect("unknown storage bit", F_("r_bit", 37, 64, 6, BN, OUT_STATS_RAW, (16, 1)), lambda r: setattr(r.args, "storage", 8))
    gen_case = F_("r_gen", 37, 64, 6, BN, OUT_STATS_RAW, (16, 1), mask="g", offset=1)
    keep = []

    def add_mask(r):
        keep.append(_dev(make_fwd(gen_case)["mult"]))
        r.args.mask = keep[-1].data_ptr()
    expect("gen.keys together with mask", gen_case, add_mask)

    def low_inv(r):
        r.args.gen.inv = 0.5
    expect("gen.inv < 1", gen_case, low_inv)
    expect("gen.inv NaN", gen_case, lambda r: setattr(r.args.gen, "inv", float("nan")))
    rep.done()


def test_backward_rejections_touch_nothing():
    rep = Report("bwd_einval")

    def expect(what, c, mode=None, **over):
        t = make_bwd(c)
        run = BwdRun(c, t, mode)
        s = run.slabs.t
        a = _lib.DenseBwdT()
        p = lambda v: None if v is None else v.data_ptr()
        a.g, a.g_kind, a.zout, a.B, a.N = p(run.g), c.g_kind, p(run.zout), c.B, c.N
        a.x, a.K, a.in_kind, a.slope, a.has_bn, a.bn = p(run.x), c.K, c.in_kind, p(run.slope), 1, run.bn
        a.mask, a.w, a.dw, a.db, a.slab_stride = p(run.mask), p(run.w), p(s[0, 0:]), p(s[0, run.o_db:]), run.stride
        a.dx, a.dx_partials, a.storage, a.mask_scale, a.gen = p(run.dx.t), p(run.dxp.t), c.storage, 1.0, ops.make_gen(run.gen)
        for k, v in over.items():
            if k == "inv":
                a.gen.inv = v
            else:
                setattr(a, k, v)
        n = C.c_int(-5)
        rc = _lib.load().raae_dense_bwd_s(C.byref(a), C.byref(n), C.c_void_p(torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        rep.check(rc == -1, f"{what}: not RAAE_EINVAL")
        rep.check(all(bool((b.whole == SENT).all()) for b in (run.slabs, run.dx, run.dxp)), f"{what}: an output was written")
        return run

    expect("ST_X with K % 4 != 0", B_("rb_x13", 37, 6, 13, G_DIRECT, BN, (1, 1), storage=ST_X))
    expect("unknown storage bit", B_("rb_bit", 37, 6, 64, G_DIRECT, BN, (1, 1)), storage=8)
    gen_case = B_("rb_gen", 37, 6, 64, G_DIRECT, BN, (1, 1), mask="g", offset=1)
    extra = _dev(make_bwd(gen_case)["mult"])
    expect("gen.keys together with mask", gen_case, mask=extra.data_ptr())
    expect("gen.inv < 1", gen_case, inv=0.5)
    rep.done()
