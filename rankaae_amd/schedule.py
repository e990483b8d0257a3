"""The host-side protocol of the step's launches.

A network pass is a generator of launches (``forward_steps`` / ``backward_steps`` of ``FCNet`` / ``CompactNet``): it
yields ``(kind, args)`` where a launch may share a kernel with a launch of another pass, expects back what that launch
returns, and launches everything else inline.  ``Pass`` is a cursor over such a generator; ``run`` drives one pass alone,
``lockstep`` two of them side by side under a sharing policy (``share_dense`` / ``share_blocks`` / ``share_across``), and
``chain`` / ``item`` put passes and single launches one behind the other.

What a generator launches inline BEFORE its first yield runs when the pass is primed, so the moment of priming is part
of the launch order: nothing here primes a pass at construction, ``run`` / ``lockstep`` / ``chain`` prime it when its
turn comes (``lockstep``: the host before the rider), and a caller that needs it earlier calls ``prime`` itself.

``ops`` is read through this module's attribute, so that a test can put a stand-in there.
"""
from . import ops


class Pass:
    """Cursor over a generator of launches: ``item`` is the ``(kind, args)`` it waits at, ``ended`` whether it has
    returned, ``result`` what it returned."""

    def __init__(self, steps):
        self.steps, self.primed, self.item, self.ended, self.result = steps, False, None, False, None

    def prime(self):
        """Run the generator up to its first yield, inline launches included; a second call does nothing."""
        if not self.primed:
            self.primed = True
            self.advance(None)
        return self

    def advance(self, value):
        """Hand the generator what the launch of ``item`` returned and run it to its next yield or its end."""
        try:
            self.item = self.steps.send(value)
        except StopIteration as done:
            self.item, self.ended, self.result = None, True, done.value

    def launch(self):
        """The launch it waits at, on its own."""
        kind, args = self.item
        self.advance(ops.dense_fwd_struct(args) if kind == "dense" else ops.launch_item(kind, args))

    def rest(self):
        """What is left of the pass as a generator of launches (``chain``)."""
        self.prime()
        while not self.ended:
            self.advance((yield self.item))
        return self.result


def run(p):
    """Drive one pass alone to its end, every launch on its own; returns its result."""
    p.prime()
    while not p.ended:
        p.launch()
    return p.result


def item(make):
    """A pass of ONE launch: ``make()`` is called when the pass is primed -- an update built then sees what the pass
    chained before it has recorded -- and returns the ``(kind, args)`` to yield."""
    def steps():
        yield make()
    return Pass(steps())


def chain(*passes):
    """The passes one behind the other as one pass, each primed when its turn comes; its result is the last one's."""
    def steps():
        result = None
        for p in passes:
            result = yield from p.rest()
        return result
    return Pass(steps())


# ---- sharing policies: what the two waiting launches return if they went out as ONE launch, or None if they do not share

def share_dense(h, r):
    """Two dense layers: always one launch (raae_dense_fwd2)."""
    return ops.dense_fwd_pair(h[1], r[1])


def share_blocks(h, r):
    """Two forward passes of the conv networks, the ENCODER's as host: the same phase of a fused block in one launch
    (raae_block_fwd_a2 / _b2); the decoder's head rides in an encoder block launch that has an instance for it."""
    if h[0] == r[0]:
        return ops.block_fwd_pair(h[0], h[1], r[1])
    if r[0] == "head" and ops.co_pairable(h[0], h[1], "head", r[1]):
        return ops.co_launch(h[0], h[1], "head", r[1])
    return None


def share_across(h, r):
    """Across a phase boundary (host: a backward pass and what ends it; rider: whatever may run beside it): one launch
    where the library has an instance for the pair (``ops.co_pairable``, raae_co_launch)."""
    if ops.co_pairable(h[0], h[1], r[0], r[1]):
        return ops.co_launch(h[0], h[1], r[0], r[1])
    return None


def lockstep(host, rider, share, until_host_ends=False):
    """Two independent passes side by side: while both wait at a launch and ``share`` makes one launch of the two, they
    share it; otherwise the host's launch goes alone and the rider waits for the next one -- except an update
    (``"adam"``) that cannot ride, which goes first: the rest of the rider waits for it.  Whichever pass outlives the
    other runs the rest alone; with ``until_host_ends`` the rider stops where it is when the host has ended, to go on
    as the rider of a later ``lockstep``.  Returns the two results (the rider's is None while it has not ended)."""
    host.prime()
    rider.prime()
    while not (host.ended and (rider.ended or until_host_ends)):
        if host.ended or rider.ended:
            (rider if host.ended else host).launch()
            continue
        shared = share(host.item, rider.item)
        if shared is None:
            (rider if rider.item[0] == "adam" else host).launch()
        else:
            rider.advance(shared[1])     # (the rider first: what it launches inline next must not wait for the host's host work)
            host.advance(shared[0])
    return host.result, rider.result
