"""Shared pieces of the --dedup tests: the fp64 numpy reference of the duplicate statistic, the numpy rule, frames with a planted
patch, clips with planted repeats."""
import numpy as np

from drba_amd import dedup

# (c, h, w) of the statistic's GPU test: one block; whole blocks only; partial edges on both sides; w % 4 != 0 (row starts that are
# not 16-byte aligned) with one / two partial sides; a row wider than one wave's 32 pixels; more 32 x 8 strips than one workgroup takes
SHAPES = [(3, 8, 8), (3, 16, 24), (3, 9, 17), (3, 8, 19), (3, 23, 18), (3, 64, 200), (3, 136, 260), (1, 9, 17)]
LO = dedup.LO


def block_means(a, b):
    """fp64 means of |a - b| over 8 x 8 pixel blocks aligned at the origin and all channels; edge blocks by their own pixel count.
    a, b: [c, h, w] (or [1, c, h, w]) arrays -> [ceil(h / 8), ceil(w / 8)]"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    a, b = a.reshape(a.shape[-3:]), b.reshape(b.shape[-3:])
    d = np.abs(a - b)
    c, h, w = d.shape
    out = np.empty(((h + 7) // 8, (w + 7) // 8), dtype=np.float64)
    for by in range(out.shape[0]):
        for bx in range(out.shape[1]):
            out[by, bx] = d[:, by * 8:by * 8 + 8, bx * 8:bx * 8 + 8].mean()
    return out


def ref_stats(a, b, lo=LO):
    """-> (max_block, n_above, n_blocks, margin): margin is the smallest relative distance of a block mean from lo."""
    m = block_means(a, b)
    margin = float(np.min(np.abs(m - lo)) / lo) if lo > 0 else np.inf
    return float(m.max()), int((m > lo).sum()), int(m.size), margin


def np_is_dup(a, b, s=None):
    s = s or dedup.Settings()
    mx, n_above, n_blocks, _ = ref_stats(a, b, s.lo)
    return dedup.is_dup(mx, n_above, n_blocks, hi=s.hi, frac=s.frac)


def check_dup_numpy(settings=None):
    """interpolate_stream's check_dup= on torch (CPU) network inputs, by the numpy rule."""
    return lambda a, b: np_is_dup(a.detach().cpu().numpy(), b.detach().cpu().numpy(), settings)


def planted_pair(c, h, w, seed, last_block=False):
    """Two fp32 frames [1, c, h, w] in [0, 1]: b = a + small noise (block means around lo on both sides of it), plus 0.3 on one 8 x 8
    block -- the first one inside, or the last (bottom right, partial where the shape has partial edges) -> (a, b, (by, bx))"""
    rng = np.random.default_rng(seed)
    a = rng.random((1, c, h, w), dtype=np.float32) * 0.6
    amp = rng.random((1, 1, (h + 7) // 8, (w + 7) // 8), dtype=np.float32) * 4 * LO  # per-block noise amplitude: means 0 .. 2 lo
    amp = np.repeat(np.repeat(amp, 8, axis=2), 8, axis=3)[:, :, :h, :w]
    b = a + amp * rng.random((1, c, h, w), dtype=np.float32)
    nby, nbx = (h + 7) // 8, (w + 7) // 8
    by, bx = (nby - 1, nbx - 1) if last_block else (min(1, nby - 1), min(1, nbx - 1))
    b[:, :, by * 8:by * 8 + 8, bx * 8:bx * 8 + 8] += np.float32(0.3)
    return a, b.astype(np.float32), (by, bx)


def seeded_pair(c, h, w, last_block=False, need=1e-4):
    """planted_pair with the first seed whose fp64 reference keeps every block mean `need` (relative) away from lo: chosen here on
    the CPU, so the n_above comparison on the device never has to be waived."""
    for seed in range(100):
        a, b, where = planted_pair(c, h, w, 1000 + seed, last_block)
        if ref_stats(a, b)[3] > 10 * need:
            return a, b, where
    raise AssertionError(f"no seed gives a margin at {(c, h, w)}")


def repeat_clip(frames, pattern):
    """frames[i] for i in pattern, e.g. [0, 0, 1, 2, 2, 2] -> a clip on uneven holds (copies, not views)"""
    return [frames[i].copy() for i in pattern]


def moving_clip(n, h, w, seed):
    """synth.make_clip with 4 or 6 pixels of motion per frame: no pair is a repeat by the default rule (the largest block mean is
    around 40/255 against hi = 12/255; make_clip's own 1 .. 3 pixel steps of a smooth texture stay below the thresholds)."""
    from drba_amd.utils import synth
    return synth.make_clip(n, h, w, seed=seed, offsets=[5 * k + (k % 2) for k in range(n)])
