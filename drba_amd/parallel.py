"""Frame-level data parallelism: shard the clip across ranks, gather finished frames to the writer.

The reference has no parallelism at all; this is the scheme BASELINE.json's
north_star prescribes.  Every (I0, I1, I2) step is independent *given* the driver state that
enters it, so the source-step range is cut into contiguous chunks, one per rank (one process
per GPU, torch.distributed; backend "nccl" = RCCL over xGMI on the GPUs, "gloo" in CPU tests).
Each rank rebuilds the state the sequential driver would carry into its first step from a
halo of one extra leading frame:

    cut_left = check_scene(frame[a], frame[a+1])         (only with scene detection on)
    reuse    = swap(model.calc_flow(frame[a], frame[a+1])) if step a-1 was a DRBA step (no cut on either side) else None

which is exactly what step a-1 of the sequential run returns (reference models/rife.py:82-85,109), and then runs the
sequential driver's loop (drba_amd/driver.py) over its frames, so the sharded result equals the sequential one (on the
GPU up to which steps share a stacked pass: tests/test_gpu_parallel.py).
The only collective in the data path is the gather of finished uint8 frames to rank 0; a 1080p
frame is 6.2 MB, i.e. ~0.2 GB/s per xGMI link at 8 x 30 fps -- no ring tuning needed.
"""
import numpy as np
import torch

from drba_amd import driver
from drba_amd.models.utils import tools as _tools


def partition(n_loop_steps, world):
    """Contiguous, near-equal split of loop iterations [0, n) -> list of (first, last_exclusive) per rank."""
    base, rem = divmod(n_loop_steps, world)
    out, start = [], 0
    for r in range(world):
        n = base + (1 if r < rem else 0)
        out.append((start, start + n))
        start += n
    return out


def warm_reuse(model, Ia, Ib):
    """The `reuse` state a DRBA step on (.., Ia, Ib) hands to the next step (rife.py:82-85,109)."""
    if hasattr(model, "warm_reuse"):
        return model.warm_reuse(Ia, Ib)
    flow_ab, flow_ba, fa, fb = model.calc_flow(Ia, Ib)
    return (flow_ba, flow_ab, fb, fa)


def emission_counts(n_frames, src_fps, dst_fps, times, world):
    """Output frames per emission (head / loop iteration / tail) of every rank: [[count, ...] per rank].
    Every branch of the driver loop emits len(calc_t(idx)) frames (copies at scene cuts replace synthesised frames one
    for one, infer.py:98-103,121-143,160-162), so the counts are known to all ranks without any communication."""
    mapper = _tools.TMapper(src_fps, dst_fps, times)
    n_loop = max(n_frames - 2, 0)
    out = []
    for r, (a, b) in enumerate(partition(n_loop, world)):
        c = [len(_tools.calc_t(0, times, mapper))] if r == 0 else []
        c += [len(_tools.calc_t(k, times, mapper)) for k in range(a, b)]
        if r == world - 1 and n_frames >= 2:
            c.append(len(_tools.calc_t(n_frames - 2, times, mapper)))
        out.append(c)
    return out


def interpolate_shard(model, frames, src_fps, dst_fps, rank, world, times=-1, enable_scdet=False, scdet_threshold=0.3,
                      to_inp=None, to_out=None, check_scene=None, sink=None, linear=True):
    """Run this rank's share of the clip.  `frames` is a random-access sequence of uint8 HWC frames
    (every rank can index it; only its own range plus the halo is touched).
    Returns the list of output frames (whatever to_out returns) this rank is responsible for, in order.
    Concatenating the lists of ranks 0..world-1 gives exactly the sequential driver's output.
    `sink(list_of_frames)`, if given, receives each emission (head / one loop iteration / tail) as it is produced
    instead (StreamedGather.push: the frames travel to the writer rank while the next steps compute) and the
    function returns [].  `linear`: see drba_amd.driver.run."""
    to_inp = to_inp or _tools.to_inp
    to_out = to_out or _tools.to_out
    if dst_fps <= src_fps:
        raise ValueError(f"dst fps should be greater than src fps, but got dst_fps={dst_fps} and src_fps={src_fps}")
    n = len(frames)
    a, b = partition(max(n - 2, 0), world)[rank]
    head, tail = rank == 0, rank == world - 1
    out = []
    if a == b and not (head or tail):  # more ranks than loop iterations: nothing to do here
        return out
    size = _tools.get_valid_net_inp_size(frames[0], model.scale, div=model.pad_size)
    src_size, dst_size = size["src_size"], size["dst_size"]
    mapper = _tools.TMapper(src_fps, dst_fps, times)
    cuts = driver.SceneCuts(enable_scdet, scdet_threshold, check_scene)

    def emit(xs):
        fr = [to_out(x, src_size) for x in xs]
        if sink is not None:
            sink(fr)
        else:
            out.extend(fr)

    # ---- state entering loop iteration a, as the sequential driver would have it (rank 0 starts cold, with the head)
    pair = [to_inp(frames[a], dst_size), to_inp(frames[a + 1], dst_size)]
    cut_left, reuse = False, None
    if a > 0 and a < b:
        cut_left = cuts.cut(a, *pair)
        # iteration a-1 had (left, right) = (cut(a-1), cut(a)): a DRBA step iff both are False
        if not cut_left and not cuts.cut(a - 1, to_inp(frames[a - 1], dst_size), pair[0]):
            reuse = warm_reuse(model, *pair)

    # ---- the head (rank 0), loop iterations [a, b) and the tail (last rank): the sequential loop over the frames up to b + 1,
    # the I2 of iteration b - 1.  (announce_ungrouped: a shard has always named the following iterations to a prefetching
    # model with GROUP = 1 too, where the sequential driver names one; such a model reads the first entry alone.  Kept.)
    hi = min(b + 1, n - 1)
    driver.run(model, lambda k: frames[k] if k <= hi else None, pair, a, to_inp=lambda raw: to_inp(raw, dst_size), emit=emit,
               cuts=cuts, ts_of=lambda idx: _tools.calc_t(idx, times, mapper), state=(cut_left, reuse), head=head, tail=tail,
               announce_ungrouped=True, linear=linear)
    return out


def _default_device(group=None):
    """Where collective buffers must live: the current GPU for the nccl (= RCCL) backend, host memory for gloo."""
    import torch.distributed as dist
    if dist.get_backend(group) == "nccl":
        return torch.device("cuda", torch.cuda.current_device())
    return torch.device("cpu")


class StreamedGather:
    """The RCCL gather of finished uint8 frames to the writer rank, overlapped with the computation.

    One gather at the end of a shard leaves the xGMI links idle while the GPUs compute and the GPUs idle while the
    frames travel (8 ranks x 40 1080p frames = 2 GB into rank 0).  Here the emissions (head / loop iteration / tail)
    of a rank are grouped into rounds of `chunk` emissions; after its j-th round every rank contributes a fixed-size
    padded buffer to an ASYNCHRONOUS dist.gather (RCCL runs it on its own stream, under the next steps' kernels).  All
    sizes follow from emission_counts(), which every rank computes locally, so ranks with fewer emissions (no head /
    tail) still take part in every round and the collectives are issued in the same order everywhere.
    Device memory stays bounded: at most `in_flight` rounds keep their send / receive buffers on the GPU; older rounds
    are retired as later ones are issued -- every rank drops its send buffer, the writer copies the round's received
    frames into pinned host memory on a drain stream of its own (a 10-minute 1080p60 clip is > 200 GB of uint8 frames:
    it cannot wait on the GPU for finish()).  `on_round(j, frames_by_rank)`, if given, receives the writer's host
    frames of round j as soon as they have landed (list over ranks of lists of HWC uint8 tensors).
    finish() returns the ordered frame list on rank 0 (host tensors; None elsewhere)."""

    def __init__(self, rank, world, counts, chunk=4, device=None, group=None, frame_shape=None, in_flight=2, on_round=None):
        self.rank, self.world, self.group, self.chunk = rank, world, group, max(1, int(chunk))
        self.dev = device if device is not None else (_default_device(group) if world > 1 else None)
        self.counts = counts
        self.n_rounds = max((len(c) + self.chunk - 1) // self.chunk for c in counts) if counts else 0
        # frames rank r contributes in round j
        self.per_round = [[sum(c[j * self.chunk:(j + 1) * self.chunk]) for j in range(self.n_rounds)] for c in counts]
        self.cap = [max(self.per_round[r][j] for r in range(world)) for j in range(self.n_rounds)]
        self.pending, self.emissions, self.round = [], 0, 0
        self.handles, self.recv, self.keep = [], [], []
        self.shape = None if frame_shape is None else tuple(frame_shape)  # (H, W, 3) of an output frame, if known
        self.local = []  # world == 1: plain accumulation
        self.in_flight, self.on_round = max(1, int(in_flight)), on_round
        self.retired = 0            # rounds [0, retired) no longer hold device buffers
        self.host = []              # writer: per retired round, per rank, the received frames in host memory
        self._drain, self._landed = None, []  # writer on a GPU: the D2H stream and one event per retired round
        self.peak_device_rounds = 0  # (tests) most rounds that held device buffers at any time

    def _tensor(self, f):
        t = f if torch.is_tensor(f) else torch.from_numpy(np.ascontiguousarray(f))
        return t.to(self.dev, non_blocking=True) if self.dev is not None else t

    def _issue(self):
        """The gather of round self.round (every rank calls this the same number of times, in the same order)."""
        import torch.distributed as dist
        j = self.round
        want = self.per_round[self.rank][j]
        assert len(self.pending) == want, (self.rank, j, len(self.pending), want)
        if self.shape is None:  # ranks whose first rounds are empty learn the frame shape from rank 0
            shp = [tuple(self.pending[0].shape) if self.pending else None]
            dist.broadcast_object_list(shp, src=0, group=self.group)
            self.shape = shp[0]
        buf = torch.empty((max(self.cap[j], 1),) + self.shape, dtype=torch.uint8, device=self.dev)
        if self.pending:
            torch.stack(self.pending, out=buf[:want])
        recv = [torch.empty_like(buf) for _ in range(self.world)] if self.rank == 0 else None
        self.handles.append(dist.gather(buf, recv, dst=0, group=self.group, async_op=True))
        self.recv.append(recv)
        self.keep.append(buf)
        self.pending = []
        self.round += 1
        self.peak_device_rounds = max(self.peak_device_rounds, self.round - self.retired)
        while self.round - self.retired > self.in_flight:
            self._retire()

    def _retire(self):
        """Round self.retired leaves the device: wait for its gather, (writer) copy what it received to host memory."""
        j = self.retired
        h = self.handles[j]
        on_gpu = self.dev is not None and torch.device(self.dev).type == "cuda"
        if self.rank != 0:
            h.wait()  # (RCCL: orders the current stream behind the collective; gloo: blocks the host)
        elif not on_gpu:
            h.wait()
            self.host.append([[self.recv[j][r][k] for k in range(self.per_round[r][j])] for r in range(self.world)])
        else:
            if self._drain is None:
                self._drain = torch.cuda.Stream(device=self.dev)
            with torch.cuda.stream(self._drain):
                h.wait()  # the drain stream, not the compute stream, waits for the collective
                rows = []
                for r in range(self.world):
                    n = self.per_round[r][j]
                    src = self.recv[j][r]
                    src.record_stream(self._drain)
                    dst = torch.empty((n,) + tuple(src.shape[1:]), dtype=torch.uint8, pin_memory=True)
                    if n:
                        dst.copy_(src[:n], non_blocking=True)
                    rows.append([dst[k] for k in range(n)])
                ev = torch.cuda.Event()
                ev.record(self._drain)
            self.keep[j].record_stream(self._drain)
            self._landed.append(ev)
            self.host.append(rows)
        self.recv[j] = self.keep[j] = None  # device buffers back to the allocator
        self.retired += 1
        if self.rank == 0 and self.on_round is not None:
            if self._landed:
                self._landed[-1].synchronize()
            self.on_round(j, self.host[j])

    def push(self, frames):
        """One emission of this rank (a list of uint8 HWC frames)."""
        if self.world == 1:
            self.local.extend(frames)
            return
        self.pending.extend(self._tensor(f) for f in frames)
        self.emissions += 1
        if self.emissions % self.chunk == 0 or self.emissions == len(self.counts[self.rank]):
            self._issue()

    def finish(self):
        if self.world == 1:
            return list(self.local)
        assert self.emissions == len(self.counts[self.rank]), "every emission must be pushed before finish()"
        while self.round < self.n_rounds:  # ranks with fewer emissions: empty contributions to the remaining rounds
            self._issue()
        while self.retired < self.n_rounds:
            self._retire()
        if self.rank != 0:
            return None
        for ev in self._landed:
            ev.synchronize()
        out = []
        for r in range(self.world):
            for j in range(self.n_rounds):
                out.extend(self.host[j][r])
        return out


def gather_frames(local_frames, rank, world, device=None, group=None):
    """Gather every rank's finished uint8 frames on rank 0 (the writer), in rank order.

    One size exchange + one padded gather (torch.distributed, RCCL on GPUs).  Returns the full
    ordered list on rank 0, None elsewhere."""
    import torch.distributed as dist
    if world == 1:
        return list(local_frames)
    dev = device if device is not None else _default_device(group)
    as_t = [f if torch.is_tensor(f) else torch.from_numpy(np.ascontiguousarray(f)) for f in local_frames]
    shape = tuple(as_t[0].shape) if as_t else None
    counts = [torch.zeros(1, dtype=torch.int64, device=dev) for _ in range(world)]
    dist.all_gather(counts, torch.tensor([len(as_t)], dtype=torch.int64, device=dev), group=group)
    counts = [int(c.item()) for c in counts]
    shapes = [None] * world
    dist.all_gather_object(shapes, shape, group=group)
    shape = next(s for s in shapes if s is not None)
    nmax = max(counts)
    buf = torch.zeros((nmax,) + shape, dtype=torch.uint8, device=dev)
    if as_t:
        buf[:len(as_t)] = torch.stack([t.to(dev) for t in as_t])
    recv = [torch.empty_like(buf) for _ in range(world)] if rank == 0 else None
    dist.gather(buf, recv, dst=0, group=group)
    if rank != 0:
        return None
    out = []
    for r in range(world):
        out.extend(recv[r][k] for k in range(counts[r]))
    return out
