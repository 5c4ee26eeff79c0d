"""--dedup, the host side without a device: the duplicate rule and the retimed schedule (not in the reference, whose README leaves
repeated frames to a separate tool).

The rule is ffmpeg mpdecimate's with its documented defaults carried onto the [0, 1] scale: a frame repeats its predecessor in the
source when no 8 x 8 block differs by more than `hi` on average and at most `frac` of the blocks differ by more than `lo`
(drba_amd.ops.dup_stats gives the two figures).  The filter that applies it to a stream is drba_amd.driver.KeptFrames.

The schedule: the written clip has the frames of a run without --dedup at the same instants; only what each is interpolated from
changes.  Time is in source-frame units, frame 0 at 0.  The plain run writes, around source frame j, the instants (j - 1) + t for t
in calc_t(max(j - 1, 0)) -- the head is j = 0, loop iteration i is j = i + 1, the tail j = N - 1 (calc_t is evaluated one behind
the centre frame: SURVEY.md App. D).  With the kept source indices k_0 = 0 < k_1 < ... an instant T belongs to the kept iteration u
(left a = k_u, centre c = k_(u+1), right b = k_(u+2)) when (a + c) / 2 <= T < (c + b) / 2, with the timestep 1 - (c - T) / (c - a)
left of the centre and 1 + (T - c) / (b - c) from it on; what lies before (k_0 + k_1) / 2 is the head's, what lies at or after
(k_(M-2) + k_(M-1)) / 2 the tail's.  An instant is carried as (j, t) and converted only where the interval it falls into is longer
than one frame, so a step between neighbouring frames gets calc_t's own array."""
import math

import numpy as np

HI, LO, FRAC, MAX_RUN = 12.0 / 255.0, 5.0 / 255.0, 0.33, 3  # mpdecimate's hi = 64 * 12, lo = 64 * 5 (per 8 x 8 block of bytes), frac


class Settings:
    """hi / lo / frac of the rule and max_run, the most frames dropped in a row (the frame after them is kept whatever the test
    says: drawings on fours by default; without the bound a held shot that ends in motion would become one long morph)."""

    def __init__(self, hi=HI, lo=LO, frac=FRAC, max_run=MAX_RUN):
        self.hi, self.lo, self.frac, self.max_run = float(hi), float(lo), float(frac), int(max_run)
        if not (self.hi >= 0 and self.lo >= 0 and 0 <= self.frac <= 1 and self.max_run >= 0):
            raise ValueError(f"--dedup: hi and lo must be >= 0, frac in [0, 1], max >= 0; got {hi}, {lo}, {frac}, {max_run}")


def settings_of(dedup):
    """interpolate_stream's dedup=: None / False (off), True (the defaults), a Settings or a dict of its fields."""
    if dedup is None or dedup is False:
        return None
    if dedup is True:
        return Settings()
    return dedup if isinstance(dedup, Settings) else Settings(**dict(dedup))


def is_dup(max_block, n_above, n_blocks, hi=HI, frac=FRAC):
    return max_block <= hi and n_above <= frac * n_blocks


def kept_indices(dups, max_run=MAX_RUN):
    """The filter's frame rules on a whole clip: dups[k - 1] says whether source frame k repeats frame k - 1 (len(dups) + 1 frames).
    Frame 0 is kept; after max_run drops in a row the next frame is kept; if fewer than two frames would be kept the last one is too."""
    kept, run = [0], 0
    for k in range(1, len(dups) + 1):
        if dups[k - 1] and run < max_run:
            run += 1
        else:
            kept.append(k)
            run = 0
    if len(kept) < 2 and len(dups) >= 1:
        kept.append(len(dups))
    return kept


class Retimed:
    """ts_of / even_of of a --dedup run for drba_amd.driver.run.  calc(i) -> tools.calc_t of plain iteration i; kept: the list of kept
    source indices, which may still grow (step u needs k_(u+2), a frame the driver has read by then); total() -> the number of
    source frames, asked for the tail only, when the source has ended."""

    def __init__(self, calc, kept, total):
        self.calc, self.kept, self.total, self._memo, self._head_asked = calc, kept, total, {}, False

    def _instants(self, lo, hi, last):
        """(j, t) of the plain run's instants lo <= (j - 1) + t < hi, in its order; `last`: the highest slot there is."""
        j0 = 0 if lo == -math.inf else max(0, math.ceil(lo - 0.5))
        j1 = last if hi == math.inf else min(last, math.ceil(hi + 0.5) - 1)
        return [(j, t) for j in range(j0, j1 + 1) for t in self.calc(max(j - 1, 0)) if lo <= (j - 1) + t < hi]

    # what each part of the run writes, as (j, t): the instant is (j - 1) + t
    def head_instants(self):
        return self._instants(-math.inf, (self.kept[0] + self.kept[1]) / 2, self.kept[1])

    def step_instants(self, u):
        return self._instants((self.kept[u] + self.kept[u + 1]) / 2, (self.kept[u + 1] + self.kept[u + 2]) / 2, self.kept[u + 2])

    def tail_instants(self):
        return self._instants((self.kept[-2] + self.kept[-1]) / 2, math.inf, self.total() - 1)

    def _array(self, inst, values, whole_slot):
        """The timesteps as an array: calc_t's own when the step is one whole slot between neighbouring frames."""
        if whole_slot is not None:
            own = self.calc(max(whole_slot - 1, 0))
            if len(own) == len(inst) and all(j == whole_slot for j, _ in inst):
                return own
        return np.array([float(v) for v in values], dtype=np.float64)

    def head(self):
        k0, k1 = self.kept[0], self.kept[1]
        inst = self.head_instants()
        # before frame k_0: copies (any value < 1: calc_t's own, the instant lies in slot 0); from it on the way to k_1
        vals = [t if (j == k0 and (k1 - k0 == 1 or (j - 1) + t < k0)) else 1 + ((j - 1) + t - k0) / (k1 - k0) for j, t in inst]
        return self._array(inst, vals, k0 if k1 - k0 == 1 else None)

    def tail(self):
        a, c = self.kept[-2], self.kept[-1]
        inst = self.tail_instants()
        vals = []
        for j, t in inst:
            T = (j - 1) + t
            if j == c and (T >= c or c - a == 1):
                vals.append(t)  # (in slot c: t >= 1 exactly when T >= c)
            elif T > c:
                vals.append(1 + (T - c))  # after the last kept frame: a copy (any value > 1)
            else:
                vals.append(1 - (c - T) / (c - a))
        return self._array(inst, vals, c if (c - a == 1 and self.total() - 1 == c) else None)

    def step(self, u):
        a, c, b = self.kept[u], self.kept[u + 1], self.kept[u + 2]
        inst = self.step_instants(u)
        vals = []
        for j, t in inst:
            T = (j - 1) + t
            gap = c - a if T < c else b - c
            if j == c and gap == 1:
                vals.append(t)
            else:
                vals.append(1 - (c - T) / gap if T < c else 1 + (T - c) / gap)
        return self._array(inst, vals, c if (c - a == 1 and b - c == 1) else None)

    def even_of(self, u):
        """Are the two intervals of kept iteration u equal?  (The DistanceRatioMap compares distances over two equal intervals.)"""
        return self.kept[u + 1] - self.kept[u] == self.kept[u + 2] - self.kept[u + 1]

    def ts_of(self, u):
        """driver.run's ts_of for a run from a cold start: its first question is the head's, then it asks for iteration idx -- as
        often as its look-ahead likes, always with the right frame read -- and last, when the source has ended, for the tail
        (idx = M - 2: the iteration whose right frame is missing)."""
        if not self._head_asked:
            self._head_asked = True
            return self.head()
        if u + 2 >= len(self.kept):
            return self.tail()
        if u not in self._memo:
            self._memo[u] = self.step(u)
            self._memo.pop(u - 16, None)
        return self._memo[u]
