"""How a tensor made on one HIP stream reaches a consumer on another, with the layout copies hung on it (DESIGN.md,
"Stream hand-off").  The producer records an event behind the work; the consumer's stream waits on it, and the caching
allocator is told (record_stream) about the consumer's stream for the tensor AND every copy it carries -- a missed one lets
the allocator hand the memory to a new tensor while the other stream still reads it."""
import collections
import itertools
import weakref

import torch


def tensors(x):
    """Every tensor inside nested lists / tuples / dicts."""
    if torch.is_tensor(x):
        yield x
    elif isinstance(x, (list, tuple)):
        for y in x:
            yield from tensors(y)
    elif isinstance(x, dict):
        for y in x.values():
            yield from tensors(y)


def companions(t):
    """The tensor and every layout copy it carries: ops.pair_interleaved's, ops.to_inp / rgbx's and ops.quad_interleaved's
    (the last two are kept as (copy, version))."""
    out = [t]
    c = getattr(t, "_drba_pair", None)
    if c is not None:
        out.append(c)
    for attr in ("_drba_x4", "_drba_quad"):
        c = getattr(t, attr, None)
        if c is not None:
            out.append(c[0])
    return out


def event_on(stream):
    ev = torch.cuda.Event()
    ev.record(stream)
    return ev


def hand_to(stream, value, event=None):
    """`stream` is going to use `value` (tensors in nested lists / tuples / dicts), which was made on another stream: wait for
    `event` (recorded behind the producer's work; None: the caller has ordered the streams already), then tell the allocator."""
    if event is not None:
        stream.wait_event(event)
    seen = set()  # (a staged group names the same frames and features once per work item)
    for t in tensors(value):
        if id(t) not in seen:
            seen.add(id(t))
            for c in companions(t):
                c.record_stream(stream)
    return value


# A value produced ahead of its use, kept on a holder (the frame tensor it belongs to; the Lookahead keeps its one result,
# keyed by the frame pair, on itself): `event` was recorded behind the producer, `key` says whose it is and for what, `pred`
# is a weak reference to a second tensor the value belongs to (the pair flow's first frame: a strong one would chain every
# frame, with its features, to its successor for the length of the clip).
Ahead = collections.namedtuple("Ahead", "value event key pred")

_TOKENS = itertools.count(1)


def token_of(owner):
    """The owner's part of a key: unique in the process, unlike id(owner), which the next model built at a freed model's
    address inherits together with the old model's per-frame caches.  (Kept in the owner's __dict__: a copy.copy or deepcopy
    of an owner would share its token.)"""
    t = getattr(owner, "_handoff_token", None)
    if t is None:
        t = owner._handoff_token = next(_TOKENS)
    return t


def publish(holder, attr, value, key, stream=None, pred=None):
    """Keep `value`, whose producer is the work enqueued on `stream` so far (None: the current stream), as holder.attr
    (`holder` is a tensor).  Nothing is kept on a host tensor (there is no second stream to hand over to)."""
    if not holder.is_cuda:
        return
    ev = event_on(torch.cuda.current_stream(holder.device) if stream is None else stream)
    setattr(holder, attr, Ahead(value, ev, key, None if pred is None else weakref.ref(pred)))


def peek(holder, attr, key, pred=None):
    """Is there a value under (key, pred) on the holder?  -> its record or None; nothing waits."""
    rec = getattr(holder, attr, None)
    if rec is None or rec.key != key:
        return None
    if pred is None:  # (a predecessor that is gone matches nothing)
        return rec if rec.pred is None else None
    return rec if rec.pred is not None and rec.pred() is pred else None


def collect(holder, attr, key, pred=None):
    """The value published under (key, pred), handed to the current stream, or None."""
    rec = peek(holder, attr, key, pred)
    if rec is None:
        return None
    return hand_to(torch.cuda.current_stream(holder.device), rec.value, rec.event)
