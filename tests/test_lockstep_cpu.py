"""Host logic of the step's launch protocol (``rankaae_amd.schedule``: ``Pass``, ``run``, ``chain`` / ``item``, ``lockstep`` and
its sharing policies), without a GPU: generators of named launches and a stand-in for ``rankaae_amd.ops`` that knows which
pairs have an instance.  Checks the schedule DESIGN.md section 3 lists for the A/B, C/D and D/E boundaries, the dense
pair, and when each pass is primed."""
import pytest

from rankaae_amd import schedule
from rankaae_amd.engine import FCNet
from rankaae_amd.nets_conv import CompactNet
from rankaae_amd.schedule import Pass, chain, item, lockstep, share_across


class _Item:
    def __init__(self, name, wgrad=None):
        self.name, self.wgrad = name, wgrad


# host -> rider pairs with an instance (by name), as raae_co_instance answers for the 256-point networks
INSTANCES = {("bwd_a2", "adam_dec"), ("bwd_bw12", "a3"), ("bwd_a1", "b3"), ("bwd_bw01", "a4"), ("bwd_a0", "b4"),
             ("wgrad0", "a5"), ("adam", "b5"), ("adam_enc", "b5"), ("a1", "head"),
             # D/E: the decoder backward as host
             ("bwd_a6", "adam_enc"), ("bwd_bw56", "a0"), ("bwd_a5", "b0"), ("bwd_bw45", "a1"), ("bwd_a4", "b1"),
             ("bwd_bw34", "a2"), ("bwd_a3", "b2")}


class _Ops:
    def __init__(self):
        self.log = []

    def launch_item(self, kind, a):
        self.log.append(a.name)
        return 1

    def dense_fwd_struct(self, a):
        self.log.append(a.name)
        return 1

    def dense_fwd_pair(self, x, y):
        self.log.append(f"{x.name}+{y.name}")
        return 1, 1

    def co_pairable(self, kx, ax, ky, ay):
        return (ax.name, ay.name) in INSTANCES

    def co_launch(self, kx, ax, ky, ay):
        self.log.append(f"{ax.name}|{ay.name}")
        return 1, 1

    def block_fwd_pair(self, kind, x, y):
        self.log.append(f"{x.name}+{y.name}")
        return 1, 1


@pytest.fixture
def fake_ops(monkeypatch):
    o = _Ops()
    monkeypatch.setattr(schedule, "ops", o)
    return o


def _gen(items, result, log=None, before=None, after=None):
    """A pass of named launches; ``before`` / ``after``: what it launches inline before its first yield / behind its
    last one, written to ``log`` when that happens."""
    if before:
        log.append(before)
    for kind, name in items:
        yield (kind, _Item(name, wgrad=True if kind == "bwd_b" and "w" in name else None))
    if after:
        log.append(after)
    return result


def _adam(name):
    return item(lambda: ("adam", _Item(name)))


ENC_BWD = [("bwd_b", "bwd_b2"), ("bwd_a", "bwd_a2"), ("bwd_b", "bwd_bw12"), ("bwd_a", "bwd_a1"), ("bwd_b", "bwd_bw01"),
           ("bwd_a", "bwd_a0"), ("wgrad", "wgrad0")]
DEC_BWD = [("bwd_b", "bwd_bw06"), ("bwd_a", "bwd_a6"), ("bwd_b", "bwd_bw56"), ("bwd_a", "bwd_a5"), ("bwd_b", "bwd_bw45"),
           ("bwd_a", "bwd_a4"), ("bwd_b", "bwd_bw34"), ("bwd_a", "bwd_a3"), ("wgrad", "wgrad3")]
DEC_FWD = [("a", "a3"), ("b", "b3"), ("a", "a4"), ("b", "b4"), ("a", "a5"), ("b", "b5"), ("a", "a6"), ("b", "b6"),
           ("head", "head")]
ENC_FWD = [("a", "a0"), ("b", "b0"), ("a", "a1"), ("b", "b1"), ("a", "a2"), ("b", "b2")]
ENC_FC = [("dense", f"e{i}") for i in range(3)]
DEC_FC = [("dense", f"d{i}") for i in range(5)]


def test_ab_boundary_schedule(fake_ops):
    rider = Pass(_gen(DEC_FWD, "spec"))
    res, _ = lockstep(chain(Pass(_gen(ENC_BWD, None)), _adam("adam")), rider, share_across, until_host_ends=True)
    assert res is None and not rider.ended and rider.item[1].name == "a6"
    assert fake_ops.log == ["bwd_b2", "bwd_a2", "bwd_bw12|a3", "bwd_a1|b3", "bwd_bw01|a4", "bwd_a0|b4", "wgrad0|a5", "adam|b5"]
    del fake_ops.log[:]
    styles, spec = CompactNet.forward_pair(Pass(_gen(ENC_FWD, "styles")), rider)
    assert (styles, spec) == ("styles", "spec")
    assert fake_ops.log == ["a0+a6", "b0+b6", "a1|head", "b1", "a2", "b2"]


def test_cd_boundary_schedule(fake_ops):
    host = Pass(_gen([("bwd_b", "bwd_bw23")] + ENC_BWD[1:], None)).prime()
    host.launch()
    rest = Pass(_gen(DEC_FWD, "spec"))
    lockstep(chain(host, _adam("adam_enc")), chain(_adam("adam_dec"), rest), share_across, until_host_ends=True)
    assert fake_ops.log == ["bwd_bw23", "bwd_a2|adam_dec", "bwd_bw12|a3", "bwd_a1|b3", "bwd_bw01|a4", "bwd_a0|b4",
                            "wgrad0|a5", "adam_enc|b5"]
    assert not rest.ended and rest.item[1].name == "a6"


def test_de_boundary_schedule(fake_ops):
    """The encoder's half of the update and then the smoothness phase's encoder forward ride in the decoder backward,
    behind its first block launch; the encoder's tail (``lin3`` and the style BatchNorm, launched inline) goes out as
    soon as its last block has ridden, before the host's next launch; the decoder's half of the update follows."""
    log = fake_ops.log
    host = Pass(_gen(DEC_BWD, None, log, before="head_bwd")).prime()
    host.launch()
    fwd = Pass(_gen(ENC_FWD, "styles", log, after="lin3+style_bn"))
    res = lockstep(host, chain(_adam("adam_enc"), fwd), share_across)
    schedule.run(_adam("adam_dec"))
    assert res == (None, "styles") and fwd.ended and fwd.result == "styles"
    assert log == ["head_bwd", "bwd_bw06", "bwd_a6|adam_enc", "bwd_bw56|a0", "bwd_a5|b0", "bwd_bw45|a1", "bwd_a4|b1",
                   "bwd_bw34|a2", "bwd_a3|b2", "lin3+style_bn", "wgrad3", "adam_dec"]


def test_update_without_instance_goes_first_and_rider_waits(fake_ops, monkeypatch):
    """An update that cannot ride (RAdam, a narrow Adam) goes alone before the host it would have ridden in; a forward
    block without an instance waits for the next host and finishes alone behind the backward pass."""
    monkeypatch.setattr(fake_ops, "co_pairable", lambda kx, ax, ky, ay: (ax.name, ay.name) == ("bwd_bw12", "a3"))
    res, spec = lockstep(Pass(_gen(ENC_BWD[1:4], "left")), chain(_adam("adam_dec"), Pass(_gen(DEC_FWD[:3], "spec"))),
                         share_across)
    assert (res, spec) == ("left", "spec")
    assert fake_ops.log == ["adam_dec", "bwd_a2", "bwd_bw12|a3", "bwd_a1", "b3", "a4"]


def test_forward_pair_of_fresh_generators_is_unchanged(fake_ops):
    """Two fresh forward passes: block i of both in one launch, the decoder's tail and its head alone."""
    styles, spec = CompactNet.forward_pair(Pass(_gen(ENC_FWD, "styles")), Pass(_gen(DEC_FWD, "spec")))
    assert (styles, spec) == ("styles", "spec")
    assert fake_ops.log == ["a0+a3", "b0+b3", "a1+a4", "b1+b4", "a2+a5", "b2+b5", "a6", "b6", "head"]


def test_forward_pair_with_a_rider_that_has_ended(fake_ops):
    """A decoder forward that has ended beside the phase before: the encoder forward goes alone, the result is kept."""
    rider = Pass(_gen(DEC_FWD[:1], "spec"))
    schedule.run(rider)
    del fake_ops.log[:]
    assert CompactNet.forward_pair(Pass(_gen(ENC_FWD, "styles")), rider) == ("styles", "spec")
    assert fake_ops.log == ["a0", "b0", "a1", "b1", "a2", "b2"]


def test_dense_pair_and_single_pass(fake_ops):
    """The dense networks: layer i of both passes in one launch while both have layers left (the encoder's style
    BatchNorm goes out inline when its last layer has returned), the longer pass's tail alone; one pass alone."""
    log = fake_ops.log
    out = FCNet.forward_pair(Pass(_gen(ENC_FC, "styles", log, after="style_bn")), Pass(_gen(DEC_FC, "spec")))
    assert out == ("styles", "spec")
    assert log == ["e0+d0", "e1+d1", "e2+d2", "style_bn", "d3", "d4"]
    del log[:]
    assert schedule.run(Pass(_gen(ENC_FC, "styles", log, after="style_bn"))) == "styles"
    assert log == ["e0", "e1", "e2", "style_bn"]


def test_priming_order(fake_ops):
    """Nothing runs when a pass is made; ``lockstep`` primes the host before the rider, so what the backward pass
    launches inline before its first block launch goes out first; and the update chained behind the backward pass is
    built only after the host's last launch, when the pass has recorded all its slab counts."""
    log = fake_ops.log

    def update():
        log.append("build adam")
        return ("adam", _Item("adam"))
    host = chain(Pass(_gen(ENC_BWD, None, log, before="style_bn_bwd+dense_bwd")), item(update))
    rider = Pass(_gen(DEC_FWD, "spec", log, before="rider primed"))
    assert log == [] and not host.primed and not rider.primed
    res, _ = lockstep(host, rider, share_across, until_host_ends=True)
    assert res is None and host.ended and not rider.ended and rider.item[1].name == "a6"
    assert log == ["style_bn_bwd+dense_bwd", "rider primed", "bwd_b2", "bwd_a2", "bwd_bw12|a3", "bwd_a1|b3", "bwd_bw01|a4",
                   "bwd_a0|b4", "wgrad0|a5", "build adam", "adam|b5"]
