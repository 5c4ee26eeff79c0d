"""drba_amd.handoff on the CPU: stand-in streams and events that log what is asked of them, and a tensor subclass that says it
lives on the device and logs record_stream.  (The driver grid's frames say is_cuda = False, so nothing else in the CPU suite
reaches this code.)"""
import gc
import types
import weakref

import pytest
import torch

from drba_amd import handoff


class Stream:
    def __init__(self, name, log):
        self.name, self.log = name, log

    def wait_event(self, ev):
        self.log.append(("wait", self, ev))


class Event:
    def __init__(self):
        self.stream = None

    def record(self, stream):
        self.stream = stream


class DeviceTensor(torch.Tensor):
    is_cuda = property(lambda self: True)

    def record_stream(self, stream):
        LOG.append(("record", self, stream))


LOG = []


def dev(n=4):
    return torch.zeros(n).as_subclass(DeviceTensor)


@pytest.fixture
def streams(monkeypatch):
    """(P, Q): the producer's stream and the consumer's, which is the current one."""
    del LOG[:]
    p, q = Stream("P", LOG), Stream("Q", LOG)
    cuda = types.SimpleNamespace(Event=Event, current_stream=lambda device=None: q)
    monkeypatch.setattr(handoff, "torch", types.SimpleNamespace(is_tensor=torch.is_tensor, cuda=cuda))
    return p, q


def loaded():
    """A tensor carrying all three layout copies -> (tensor, [copies])."""
    t, copies = dev(), [dev(), dev(), dev()]
    t._drba_pair = copies[0]
    t._drba_x4 = (copies[1], t._version)
    t._drba_quad = (copies[2], t._version)
    return t, copies


def test_companions_are_the_tensor_and_its_three_copies():
    t, copies = loaded()
    assert [id(c) for c in handoff.companions(t)] == [id(t)] + [id(c) for c in copies]
    assert [id(c) for c in handoff.companions(copies[0])] == [id(copies[0])]


def test_collect_waits_once_and_records_everything(streams):
    p, q = streams
    t, copies = loaded()
    u, v, holder = dev(), dev(), dev()
    value = {"a": [t, (u,)], "b": v, "n": 3}
    handoff.publish(holder, "_drba_thing", value, (7, 0.5), p)
    rec = holder._drba_thing
    assert rec.value is value and rec.key == (7, 0.5) and rec.event.stream is p and rec.pred is None
    assert LOG == []
    assert handoff.peek(holder, "_drba_thing", (7, 0.5)) is rec and LOG == []
    assert handoff.collect(holder, "_drba_thing", (7, 0.5)) is value
    waits = [e for e in LOG if e[0] == "wait"]
    assert len(waits) == 1 and waits[0][1] is q and waits[0][2] is rec.event
    recorded = [e for e in LOG if e[0] == "record"]
    assert all(e[2] is q for e in recorded)
    assert sorted(id(e[1]) for e in recorded) == sorted(id(x) for x in [t, u, v] + copies)  # each exactly once


def test_key_mismatch_is_a_miss_without_a_wait(streams):
    p, _ = streams
    holder, a = dev(), dev()
    mine, other = handoff.token_of(types.SimpleNamespace()), handoff.token_of(types.SimpleNamespace())
    handoff.publish(holder, "_drba_thing", [dev()], (mine, 1.0), p, pred=a)
    for key, pred in (((other, 1.0), a), ((mine, 0.5), a), (mine, a), ((mine, 1.0), dev()), ((mine, 1.0), None)):
        assert handoff.peek(holder, "_drba_thing", key, pred) is None
        assert handoff.collect(holder, "_drba_thing", key, pred) is None
    assert handoff.collect(holder, "_drba_other", (mine, 1.0), a) is None
    assert LOG == []
    assert handoff.collect(holder, "_drba_thing", (mine, 1.0), a) is not None and LOG


def test_lookahead_take_matches_frames_by_identity_and_only_waits(streams, monkeypatch):
    from drba_amd.models import lookahead
    p, q = streams
    monkeypatch.setattr(lookahead, "torch", handoff.torch)
    a, b, value = dev(), dev(), [dev()]
    look = lookahead.Lookahead()
    for pair in ((a, dev()), (b, a)):
        look.pending = handoff.Ahead(value, handoff.event_on(p), (a, b), None)
        assert look.take(*pair) is None and look.pending is None  # a miss drops the result
    assert LOG == []
    rec = look.pending = handoff.Ahead(value, handoff.event_on(p), (a, b), None)
    assert look.take(a, b) is value and look.pending is None
    assert len(LOG) == 1 and LOG[0][0] == "wait" and LOG[0][1] is q and LOG[0][2] is rec.event  # start() told the allocator


def test_owner_tokens_are_never_reused():
    class Owner:
        pass
    tokens = []
    for _ in range(1000):  # each dropped before the next is made: id() hands the same address out again and again
        o = Owner()
        tokens.append(handoff.token_of(o))
        assert handoff.token_of(o) == tokens[-1]
        del o
    assert len(set(tokens)) == 1000


def test_pair_record_does_not_keep_the_first_frame_alive(streams):
    p, _ = streams
    a, b = dev(), dev()
    handoff.publish(b, "_drba_pairflow", (dev(), dev()), 1, p, pred=a)
    assert handoff.peek(b, "_drba_pairflow", 1, a) is not None
    ra = weakref.ref(a)
    del a
    gc.collect()
    assert ra() is None
    assert handoff.peek(b, "_drba_pairflow", 1, dev()) is None and handoff.peek(b, "_drba_pairflow", 1) is None


def test_host_tensors_store_nothing_and_touch_no_cuda_function(monkeypatch):
    class Raises:
        def __getattr__(self, name):
            raise AssertionError(f"torch.cuda.{name} used for a host tensor")
    monkeypatch.setattr(handoff, "torch", types.SimpleNamespace(is_tensor=torch.is_tensor, cuda=Raises()))
    holder = torch.zeros(4)
    assert handoff.publish(holder, "_drba_thing", [torch.ones(2)], 1) is None
    assert not hasattr(holder, "_drba_thing")
    assert handoff.peek(holder, "_drba_thing", 1) is None and handoff.collect(holder, "_drba_thing", 1) is None


def test_hand_to_waits_before_it_records(streams):
    p, q = streams
    t, copies = loaded()
    ev = handoff.event_on(p)
    assert handoff.hand_to(q, (t, [dev()]), ev) is not None
    assert LOG[0][0] == "wait" and LOG[0][1] is q and LOG[0][2] is ev
    assert [e[0] for e in LOG[1:]] == ["record"] * 5 and all(e[2] is q for e in LOG[1:])
    del LOG[:]
    handoff.hand_to(q, t)  # no event: the caller has ordered the streams
    assert [e[0] for e in LOG] == ["record"] * 4
