"""Shared pieces of the 16-bit frame tests (tests/test_depth16_cpu.py, tests/test_gpu_depth16.py): the CPU restatement of the
16-bit conversions, whole-clip hooks built on it, the cases of drba_frame_error_u16 and a numpy "u16" back end for
drba_amd.metrics.

There is no reference for 16-bit frames; the truth is written here from oracle.ops.resize (F.interpolate):

    to_inp16 = resize(frame.float() / maxval, dst)
    to_out16 = clamp(round(resize(x, src) * maxval), 0, maxval), NaN -> 0          (torch.round: half to even)

with `resize` = oracle.ops.resize called so that ATen runs the loop it runs on frames (see resize below).
"""
import numpy as np
import torch

from oracle import ops as oops
from tests import metric_checks as mc
from tests.op_checks import Row

# the whole-clip bar: the project's 1e-3 frame tolerance in 16-bit steps, ceil(1e-3 * 65535)
CLIP_TOL_STEPS = 66
ERR16_SIZES = (1, 17, 363, 70000)


# ------------------------------------------------------------------------------------------------------ the CPU restatement
def planar16(frame, maxval=65535):
    """uint16 [H,W,3] -> fp32 [1,3,H,W] / maxval (every uint16 is exact in fp32; the division is fp32's)"""
    x = torch.from_numpy(np.ascontiguousarray(frame).astype(np.float32).transpose(2, 0, 1).copy()).unsqueeze(0)
    return x / float(maxval)


def resize(x, size):
    """oracle.ops.resize (F.interpolate) evaluated by the loop ATen runs on FRAMES.

    ATen's CPU upsample_bilinear2d has two loops whose last bit differs (which product of a 1-D interpolation is fused into the
    fma): the generic one, which every frame-sized call takes and the project's kernels are pinned to bit for bit
    (tests/test_gpu_fullsize.py), and a channels-last style one that it picks when output H + W <= 128, or with a single thread
    when C == 3 (UpSampleKernel.cpp, _use_vectorized_kernel_cond_2d).  No frame is that small, but the shapes of these tests are
    (45 + 70, 60 + 64, 64 + 64 ...), and a plain call would compare the kernels with a loop frames never meet.  So the planes go
    in one by one (C == 1) and, where H + W <= 128, widened to k W by repeating their last column, out to k Wo, of which the first
    Wo columns are kept: k W / k Wo is the same fp32 scale, every kept column reads the taps and weights it read before (a tap
    past the last column is the clamped tap), only the loop changes.  Where ATen's choice does not change, the result equals the
    plain call's bit for bit (tests/test_depth16_cpu.py)."""
    n, c, h, w = x.shape
    ho, wo = int(size[0]), int(size[1])
    k = max(1, -(-(129 - ho) // wo))  # the smallest k with ho + k wo > 128
    planes = x.reshape(n * c, 1, h, w)
    if k > 1:
        planes = torch.cat([planes, planes[..., -1:].expand(-1, -1, -1, (k - 1) * w)], 3)
    return oops.resize(planes, (ho, k * wo))[..., :wo].reshape(n, c, ho, wo).contiguous()


def to_inp16_ref(frame, dst, maxval=65535):
    return resize(planar16(frame, maxval), tuple(dst))


def quantise16(x, maxval=65535):
    """fp32 [1,3,H,W] -> uint16 [H,W,3]: * maxval, round half to even, NaN -> 0, saturate"""
    y = torch.round(x[0] * float(maxval))
    y = torch.clamp(torch.nan_to_num(y, nan=0.0, posinf=float("inf"), neginf=float("-inf")), 0.0, float(maxval))
    return np.ascontiguousarray(y.numpy().transpose(1, 2, 0)).astype(np.uint16)


def to_out16_ref(x, src, maxval=65535, rev=False):
    out = quantise16(resize(x, tuple(src)), maxval)
    return np.ascontiguousarray(out[:, :, ::-1]) if rev else out


def cpu_hooks16(maxval=65535):
    """to_inp / to_out / check_scene for interpolate_stream on the CPU, 16 bits at both ends"""
    import oracle
    return (lambda fr, size: to_inp16_ref(fr, size, maxval)), (lambda x, size: to_out16_ref(x, size, maxval)), oracle.scdet.check_scene


def all_values_frame(maxval=65535):
    """a square frame holding each value 0 .. maxval in every channel (256 x 256 at 65535, 32 x 32 at 1023), each channel in
    another order"""
    n = maxval + 1
    side = int(round(n ** 0.5))
    assert side * side == n
    v = np.arange(n, dtype=np.uint16)
    return np.ascontiguousarray(np.stack([v, v[::-1], np.roll(v, n // 3)], 1).reshape(side, side, 3))


# ------------------------------------------------------------------------------------------------- frame differences, uint16
def err_u16_ref(a, b, N, n):
    d = np.abs(a.astype(np.int64).reshape(N, n) - b.astype(np.int64).reshape(N, n))
    return np.stack([(d * d).sum(1), d.sum(1), d.max(1), (d != 0).sum(1)], 1).astype(np.int64)


def err_u16_cases():
    """[(name, a, b, N, n, off_a, off_b)]: flat uint16 arrays of N * n samples; off_a / off_b: the SAMPLE offsets the
    implementation under test is asked to place them at (equal and different 16-byte phases)."""
    rng = np.random.default_rng(16)
    out = []
    for n in ERR16_SIZES:
        for off_a, off_b in ((0, 0), (1, 1), (3, 5)):
            a, b = rng.integers(0, 65536, 3 * n, dtype=np.uint16), rng.integers(0, 65536, 3 * n, dtype=np.uint16)
            same = rng.random(3 * n) < 0.4
            b[same] = a[same]
            out.append((f"n={n} N=3 offsets {off_a}/{off_b}", a, b, 3, n, off_a, off_b))
    z, f = np.zeros(70000, np.uint16), np.full(70000, 65535, np.uint16)
    out.append(("a=0 b=65535 n=70000: sum d^2 > 2^48", z, f, 1, 70000, 0, 0))
    out.append(("a=65535 b=0 n=70000 offsets 1/2", f, z, 1, 70000, 1, 2))
    a = rng.integers(0, 65536, 3 * 363, dtype=np.uint16)
    out.append(("identical n=363 N=3", a, a.copy(), 3, 363, 1, 1))
    return out


def check_frame_error_u16(fn):
    """fn(a, b, N, n, off_a, off_b) -> integer array [N, 4] (sum d^2, sum |d|, max |d|, differing), bit-exact against int64."""
    rows = []
    for name, a, b, N, n, oa, ob in err_u16_cases():
        got, want = np.asarray(fn(a, b, N, n, oa, ob)), err_u16_ref(a, b, N, n)
        bad = float("inf") if got.shape != want.shape else float((got.astype(np.int64) != want).sum())
        rows.append(Row("frame_error_u16", name, bad, 0.0, f"bit-exact, want[0]={want[0].tolist()}"))
    return rows


# ------------------------------------------------------------------------------------------ a numpy "u16" back end (tests only)
class NumpyBackend16(mc.NumpyBackend):
    """metric_checks.NumpyBackend with the third frame kind: uint16 HWC frames, measured with the keyword maxval.  wrap=True
    plants the defect the rows must catch: the differences taken in uint16 arithmetic, which wraps."""

    def __init__(self, wrap=False):
        super().__init__()
        self.wrap, self.maxvals = wrap, []

    def prepare(self, x):
        x = x.numpy() if torch.is_tensor(x) else np.asarray(x)
        if x.dtype == np.uint16 and x.ndim in (3, 4) and x.shape[-1] == 3:
            return x, "u16", (1 if x.ndim == 3 else x.shape[0], x.shape[-3], x.shape[-2])
        return super().prepare(x)

    def measure(self, slots, k, a, b, kind, shape, val_range, want_ssim=True, maxval=None):
        if kind != "u16":
            assert maxval is None
            return super().measure(slots, k, a, b, kind, shape, val_range, want_ssim)
        n, h, w = shape
        self.maxvals.append(maxval)
        for i in range(n):
            fa, fb = a.reshape(n, *a.shape[-3:])[i], b.reshape(n, *b.shape[-3:])[i]
            self.pairs.append((fa, fb))
            if self.wrap:
                d = (fa - fb).astype(np.int64).reshape(-1)  # uint16 - uint16 wraps modulo 65536
                row = [int((d * d).sum()), int(d.sum()), int(d.max()), int((d != 0).sum())]
            else:
                row = [int(v) for v in err_u16_ref(fa.reshape(-1), fb.reshape(-1), 1, fa.size)[0]]
            ss = float("nan")
            if want_ssim and h >= 11 and w >= 11:
                ss = mc.ssim_separable64(planar16(fa, maxval), planar16(fb, maxval), val_range or 1.0)[0]
            slots[k + i] = tuple(row) + (ss,)
