"""Host logic of the launch sharing across phase boundaries (``CompactNet.lockstep`` / ``forward_pair``,
``StepEngine._then``), without a GPU: generators of named launches and a stand-in for ``rankaae_amd.ops`` that knows which
pairs have an instance.  Checks the schedule DESIGN.md section 3 lists for the A/B and C/D boundaries."""
import pytest

from rankaae_amd import nets_conv
from rankaae_amd.engine import StepEngine
from rankaae_amd.nets_conv import CompactNet


class _Item:
    def __init__(self, name, wgrad=None):
        self.name, self.wgrad = name, wgrad


# host -> rider pairs with an instance (by name), as raae_co_instance answers for the 256-point networks
INSTANCES = {("bwd_a2", "adam_dec"), ("bwd_bw12", "a3"), ("bwd_a1", "b3"), ("bwd_bw01", "a4"), ("bwd_a0", "b4"),
             ("wgrad0", "a5"), ("adam", "b5"), ("adam_enc", "b5"), ("a1", "head")}


class _Ops:
    def __init__(self):
        self.log = []

    def launch_item(self, kind, a):
        self.log.append(a.name)
        return 1

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
    monkeypatch.setattr(nets_conv, "ops", o)
    return o


def _gen(items, result):
    for kind, name in items:
        yield (kind, _Item(name, wgrad=True if kind == "bwd_b" and "w" in name else None), 0)
    return result


ENC_BWD = [("bwd_b", "bwd_b2"), ("bwd_a", "bwd_a2"), ("bwd_b", "bwd_bw12"), ("bwd_a", "bwd_a1"), ("bwd_b", "bwd_bw01"),
           ("bwd_a", "bwd_a0"), ("wgrad", "wgrad0")]
DEC_FWD = [("a", "a3"), ("b", "b3"), ("a", "a4"), ("b", "b4"), ("a", "a5"), ("b", "b5"), ("a", "a6"), ("b", "b6"),
           ("head", "head")]
ENC_FWD = [("a", "a0"), ("b", "b0"), ("a", "a1"), ("b", "b1"), ("a", "a2"), ("b", "b2")]


def test_ab_boundary_schedule(fake_ops):
    host = StepEngine._then(_gen(ENC_BWD, None), lambda: ("adam", _Item("adam")))
    res, rider = CompactNet.lockstep(host, _gen(DEC_FWD, "spec"), finish_rider=False)
    assert res is None and rider[0] is not None and rider[1][1].name == "a6"
    assert fake_ops.log == ["bwd_b2", "bwd_a2", "bwd_bw12|a3", "bwd_a1|b3", "bwd_bw01|a4", "bwd_a0|b4", "wgrad0|a5", "adam|b5"]
    del fake_ops.log[:]
    styles, spec = CompactNet.forward_pair(_gen(ENC_FWD, "styles"), rider)
    assert (styles, spec) == ("styles", "spec")
    assert fake_ops.log == ["a0+a6", "b0+b6", "a1|head", "b1", "a2", "b2"]


def test_cd_boundary_schedule(fake_ops):
    steps = _gen([("bwd_b", "bwd_bw23")] + ENC_BWD[1:], None)
    first = next(steps)
    first = steps.send(fake_ops.launch_item(first[0], first[1]))

    def rider():
        yield ("adam", _Item("adam_dec"))
        return (yield from _gen(DEC_FWD, "spec"))
    host = StepEngine._then(steps, lambda: ("adam", _Item("adam_enc")), first)
    _, rest = CompactNet.lockstep(host, rider(), finish_rider=False)
    assert fake_ops.log == ["bwd_bw23", "bwd_a2|adam_dec", "bwd_bw12|a3", "bwd_a1|b3", "bwd_bw01|a4", "bwd_a0|b4",
                            "wgrad0|a5", "adam_enc|b5"]
    assert rest[1][1].name == "a6"


def test_update_without_instance_goes_first_and_rider_waits(fake_ops, monkeypatch):
    """An update that cannot ride (RAdam, a narrow Adam) goes alone before the host it would have ridden in; a forward
    block without an instance waits for the next host and finishes alone behind the backward pass."""
    monkeypatch.setattr(fake_ops, "co_pairable", lambda kx, ax, ky, ay: (ax.name, ay.name) == ("bwd_bw12", "a3"))

    def rider():
        yield ("adam", _Item("adam_dec"))
        return (yield from _gen(DEC_FWD[:3], "spec"))
    res, spec = CompactNet.lockstep(_gen(ENC_BWD[1:4], "left"), rider())
    assert (res, spec) == ("left", "spec")
    assert fake_ops.log == ["adam_dec", "bwd_a2", "bwd_bw12|a3", "bwd_a1", "b3", "a4"]


def test_forward_pair_of_fresh_generators_is_unchanged(fake_ops):
    """Two fresh forward passes: block i of both in one launch, the decoder's tail and its head alone."""
    styles, spec = CompactNet.forward_pair(_gen(ENC_FWD, "styles"), _gen(DEC_FWD, "spec"))
    assert (styles, spec) == ("styles", "spec")
    assert fake_ops.log == ["a0+a3", "b0+b3", "a1+a4", "b1+b4", "a2+a5", "b2+b5", "a6", "b6", "head"]
