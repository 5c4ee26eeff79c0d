"""The per-frame driver loop: reference infer.py:58-174 plus the read-ahead, the intake stream, scene tests asked for ahead
of their use and the announcement of groups of steps.  Written once: drba_amd.infer.interpolate_stream runs it over the whole
clip, drba_amd.parallel.interpolate_shard over a rank's window of it with the state the sequential run would carry in."""
import contextlib

import torch

from drba_amd import handoff
from drba_amd.models.utils import tools as _tools


class SceneCuts:
    """cut(k, a, b): is there a scene cut between source frames k and k + 1 (a, b: their network inputs)?  Every pair is tested
    once, however often the look-ahead window asks.  The library's own test can be asked for ahead of its use (submit:
    tools.SceneChecks, for frames on the device); an injected check_scene is called in place."""

    def __init__(self, enable_scdet, scdet_threshold, check_scene=None):
        self.enabled, self.thr, self.known = enable_scdet, scdet_threshold, {}
        self.ahead = _tools.SceneChecks(scdet_threshold) if (check_scene is None and enable_scdet) else None
        self.check_scene = check_scene or _tools.check_scene

    def submit(self, k, a, b):
        if self.ahead is not None and b.is_cuda:
            self.ahead.submit(k, a, b)

    def cut(self, k, a, b):
        if not self.enabled:
            return False
        if k not in self.known:
            if self.ahead is not None and a.is_cuda:
                self.known[k] = self.ahead.cut(k, a, b)
            else:
                self.known[k] = bool(self.check_scene(a, b, self.thr))
        return self.known[k]


class KeptFrames:
    """--dedup's filter over the frame source: next() hands out the network inputs of the frames that are kept, in order, None past
    the end.  Every raw frame of get(k) is converted once with to_inp and tested against the previous SOURCE frame, kept or not
    (drba_amd.dedup: mpdecimate's rule on ops.dup_stats), so the decisions do not depend on one another and are asked for `ahead`
    frames before they are needed: by the time one is read (after its own event) the host is not in lock step with the device.
    A dropped frame is never seen by the driver -- no prefetch_frame, no prefetch_pair, no scene test.  Frame 0 is kept; after
    settings.max_run drops in a row the next frame is kept untested; if fewer than two frames would be kept the last one is too.
    kept[u] is the source index of the u-th kept frame, total the number of source frames once the source has ended; on_kept(k)
    fires as frame k is kept.  check_dup(a, b) -> bool, called in place, replaces the device test (frames on the host).
    stream() -> the HIP stream to_inp and the tests run on for a frame on the device (the model's intake stream) or None: every
    frame is made there and handed to the stream current at next() (drba_amd.handoff)."""

    def __init__(self, get, to_inp, settings, check_dup=None, stream=None, on_kept=None, ahead=4):
        self.get, self.to_inp, self.set, self.check_dup, self.on_kept = get, to_inp, settings, check_dup, on_kept
        self.stream_of, self.stream, self.ahead = stream, None, max(int(ahead), 1)
        self.kept, self.total = [], None
        self._q, self._read, self._prev, self._run = [], 0, None, 0  # _q: [k, network input, pending test, event, the frame before]

    def _fill(self):
        while len(self._q) <= self.ahead and self.total is None:
            raw = self.get(self._read)
            if raw is None:
                self.total = self._read
                break
            if self._read == 0 and self.stream_of is not None:
                self.stream = self.stream_of()
            with contextlib.nullcontext() if self.stream is None else torch.cuda.stream(self.stream):
                x = self.to_inp(raw)
                test = None
                if self._prev is not None and self.check_dup is None:
                    from drba_amd import ops
                    test = ops.dup_stats_async(self._prev, x, self.set.lo)
                ev = handoff.event_on(self.stream) if self.stream is not None and x.is_cuda else None
            self._q.append([self._read, x, test, ev, self._prev])
            self._read, self._prev = self._read + 1, x

    def _repeats(self, x, test, prev):
        if self.check_dup is not None:
            return bool(self.check_dup(prev, x))
        from drba_amd import dedup, ops
        host, ev = test
        ev.synchronize()
        return dedup.is_dup(*ops.dup_stats_decode(host), hi=self.set.hi, frac=self.set.frac)

    def next(self):
        while True:
            self._fill()
            if not self._q:
                return None
            k, x, test, ev, prev = self._q.pop(0)
            self._fill()  # (is frame k the last of the source?)
            last = self.total is not None and not self._q
            if k > 0 and self._run < self.set.max_run and not (last and len(self.kept) < 2) and self._repeats(x, test, prev):
                self._run += 1
                continue
            self._run = 0
            self.kept.append(k)
            if self.on_kept is not None:
                self.on_kept(k)
            if ev is not None:
                handoff.hand_to(torch.cuda.current_stream(x.device), x, ev)
            return x


def run(model, get, pair, first, to_inp, emit, cuts, ts_of, state=(False, None), head=True, tail=True, on_step=None,
        announce_ungrouped=False, linear=True, even_of=None):
    """Drive the model from loop iteration `first` until the frame source ends.

    get(k): raw source frame k, or None past the end (not asked again after that).  pair: [I0, I1], the network inputs of
    frames `first` and `first + 1`, in a list this function empties (a frame, and the features hung on it, must go when the
    loop has moved past it; a reference held by the caller would keep it).  Every later frame is taken in here.
    to_inp(raw) -> network input; emit(frames) receives each emission (head / one iteration / tail); cuts: a SceneCuts;
    ts_of(idx) -> tools.calc_t of iteration idx.  state: (cut_left, reuse) entering iteration `first` when there is no head
    (the head is a cold start and tests the first pair itself).  on_step(idx) fires after the head (idx = first), after
    every iteration and after the tail.  announce_ungrouped: name the following iterations to a GROUP = 1 model too.
    even_of(idx) -> bool (--dedup; None: every iteration): are the two intervals of iteration idx equal?  An iteration over unequal
    ones is two pairwise steps, `reuse` is dropped as beside a cut, and no group or look-ahead is announced across it.
    linear: the `linear` of every inference_ts_drba call -- True, the reference driver's (infer.py:143); False runs the clip
    through the non-linear DistanceRatioMap (get_drm_t), which the reference's model entry point defaults to but its driver never
    asks for.

    Schedule quirks kept from the reference: calc_t is evaluated at an index one behind the centre frame
    in the loop and tail (infer.py:118,159); the left/right split uses `ts < 1` when the left pair is unusable and `ts <= 1`
    when the right pair is (infer.py:102-103,127-128 vs :135-136,160-161); after any scene cut the model's `reuse` state is
    dropped.
    """
    idx = first
    cut_left, reuse = state
    I0, I1 = pair
    pair.clear()
    on_step = on_step or (lambda i: None)

    # ---- head: frames before/around the first source frame
    if head:
        ts = ts_of(idx)
        cut_left, reuse = cuts.cut(idx, I0, I1), None
        if cut_left:
            out = [I0 for _ in ts]
        else:
            out = [I0 for _ in ts[ts < 1]]
            out.extend(model.inference_ts(I0, I1, ts[ts >= 1] - 1))
        emit(out)
        on_step(idx)

    # ---- steady state: one (I0, I1, I2) triplet per source frame.  The loop reads ahead of the reference's (same frames, same
    # order, same outputs).  A model that supports it starts the next step's coarse flow on a side stream while this step's
    # frames are synthesised (inference_ts_drba(..., lookahead=)): one frame ahead.  A model that can (RIFE: `prefetch_frame`)
    # has the encoder and the coarse flow of every frame started the moment it is read, and is told the frames and timesteps
    # of the next iterations so that it may compute several consecutive steps in one stacked pass (RIFE._drba_group, the
    # next iterations then only collect): 2 GROUP - 1 frames ahead, three at the least.
    can_look = bool(getattr(model, "supports_lookahead", False))
    prefetch = getattr(model, "prefetch_frame", None) if can_look else None
    prefetch_pair = getattr(model, "prefetch_pair", None) if prefetch is not None else None
    group = int(getattr(model, "GROUP", 1)) if prefetch is not None else 1
    depth = max(3, 2 * group - 1) if prefetch is not None else (1 if can_look else 0)

    # Frame intake on its own stream (a model that prefetches offers one: RIFE.intake_stream = its prefetch stream): to_inp, the
    # scene test of the pair the new frame closes and the frame's encoder depend on nothing but the frame, and the driver needs
    # the test's DECISION before it can announce the frame as part of a group of steps.  On the caller's stream they sat behind
    # every synthesis kernel issued so far and host and GPU ran in lock step ("Frame intake on the prefetch stream")
    intake = main = None
    if prefetch is not None and getattr(I1, "is_cuda", False) and getattr(model, "intake_stream", None) is not None:
        intake = model.intake_stream(I1.device)
        if intake is not None:
            main = torch.cuda.current_stream(I1.device)
            intake.wait_stream(main)  # the only frames made on the caller's stream: I0, I1 and what the caller's state was built from

    nxt, last, ended = first + 2, I1, False

    def read():
        """The next frame's network input (None: the source has ended), with the scene test of the pair it closes asked for
        and the model's prefetches started."""
        nonlocal nxt, last, ended
        raw = None if ended else get(nxt)
        if raw is None:
            ended = True
            return None
        with contextlib.nullcontext() if intake is None else torch.cuda.stream(intake):
            x = to_inp(raw)
            if intake is not None and x.is_cuda:
                # the frame is consumed on the caller's stream later (the model's kernels, to_out of a pass-through copy): an
                # event wait behind a queue that is far from reaching the frame
                handoff.hand_to(main, x, handoff.event_on(intake))
            cuts.submit(nxt - 1, last, x)  # asked for in this or a later iteration
            if prefetch is not None:
                prefetch(x)
                if prefetch_pair is not None:
                    prefetch_pair(last, x)
        nxt, last = nxt + 1, x
        return x

    I2 = read()
    ahead = []  # the frames after I2, oldest first
    while len(ahead) < depth and I2 is not None:
        x = read()
        if x is None:
            break
        ahead.append(x)
    while I2 is not None:
        ts = ts_of(idx)
        cut_right = cuts.cut(idx + 1, I1, I2)
        if cut_left and cut_right:
            out, reuse = [I1 for _ in ts], None
        elif cut_left:
            reuse = None
            out = [I1 for _ in ts[ts < 1]]
            out.extend(model.inference_ts(I1, I2, ts[ts >= 1] - 1))
        elif cut_right:
            reuse = None
            out = model.inference_ts(I0, I1, ts[ts <= 1])
            out.extend([I1 for _ in ts[ts > 1] - 1])
        elif even_of is not None and not even_of(idx):
            # unequal intervals: the DistanceRatioMap compares distances over two equal ones -- the two pairs on their own, as beside a cut
            reuse = None
            out = model.inference_ts(I0, I1, ts[ts <= 1])
            out.extend(model.inference_ts(I1, I2, ts[ts > 1] - 1))
        elif can_look and ahead and (even_of is None or even_of(idx + 1)):
            look = (ahead[0], ts_of(idx + 1))
            if prefetch is not None and (group > 1 or announce_ungrouped):
                # the following iterations, as far as they are DRBA steps too (no cut up to the last frame named): the model may
                # take them in one stacked pass with this one and stage the group after them
                entries, prev = [], I2
                for j, x in enumerate(ahead):
                    if cuts.cut(idx + 2 + j, prev, x) or (even_of is not None and not even_of(idx + 1 + j)):
                        break
                    entries += [x, ts_of(idx + 1 + j)]
                    prev = x
                if len(entries) >= 4:
                    look = tuple(entries)
            out, reuse = model.inference_ts_drba(I0, I1, I2, ts, reuse, linear=linear, lookahead=look)
        else:
            out, reuse = model.inference_ts_drba(I0, I1, I2, ts, reuse, linear=linear)
        emit(out)
        I0, I1, cut_left = I1, I2, cut_right
        I2 = ahead.pop(0) if ahead else (read() if depth == 0 else None)
        if depth:
            x = read()
            if x is not None:
                ahead.append(x)
        idx += 1
        on_step(idx)

    # ---- tail: the last pair
    if tail:
        ts = ts_of(idx)
        out = model.inference_ts(I0, I1, ts[ts <= 1])
        out.extend([I1 for _ in ts[ts > 1] - 1])
        emit(out)
        on_step(idx + 1)
