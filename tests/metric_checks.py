"""Checks of the picture metrics (metrics.hip behind drba_amd.metrics), shared by tests/test_gpu_metrics.py (the kernels) and
tests/test_metrics_cpu.py (torch / numpy stand-ins, with and without a planted defect: the rows CAN fail).

Every check takes the function under test and returns rows (name, err, tol, extra) with the pass rule `err <= tol`
(tests/op_checks.py's Row).

SSIM.  The truth is the definition of ssim_matlab (pytorch_msssim/__init__.py:83-136) evaluated in float64 with the reference's
own fp32 window widened (oracle.scdet.gaussian_window_3d(11).double(): a dense 11^3 convolution, not the separable form the
kernel uses), the range rule applied per item.  The bar is |value - truth| <= 2e-5 on every row: the value-row rule of
tests/op_checks.py at |ref| <= 1 WITHOUT its "3 x the fp32 oracle's own error" branch -- on flat content the fp32 oracle is
itself off by up to 1.4e-3, which that branch would turn into the tolerance.  The oracle's error is printed beside each row.

Frame differences.  Bytes: bit-exact against numpy int64 (err = number of differing result words, tol 0).  fp32: the sums to
1e-12 relative against numpy float64 over the finite differences, the maximum and the non-finite count exactly.
"""
import numpy as np
import torch
import torch.nn.functional as F

from drba_amd.utils import synth
from oracle import scdet as oscdet
from tests.op_checks import Row

SSIM_TOL = 2e-5
TILE_H, TILE_W = 16, 32  # metrics.hip's output tile (kTY, kTX)
SSIM_SHAPES = ((11, 11), (11, 40), (40, 11), (13, 37), (45, 70), (TILE_H + 1, TILE_W + 1), (270, 480))
ERR_SIZES = (1, 15, 16, 17, 363, 70000)


# ------------------------------------------------------------------------------------------------------------------- SSIM
def range_of(img1):
    """pytorch_msssim/__init__.py:85-97 on one item"""
    return (255.0 if float(img1.max()) > 128 else 1.0) - (-1.0 if float(img1.min()) < -0.5 else 0.0)


def blur_dense(fields):
    """[F,1,3,H,W] float64 -> the same shape: the dense 11^3 window over the volume, replicate padding 5 on all three axes"""
    w = oscdet.gaussian_window_3d(11).double()
    return F.conv3d(F.pad(fields, (5, 5, 5, 5, 5, 5), mode="replicate"), w)


def blur_dense_folded(fields):
    """blur_dense for all but the smallest frames (its conv3d takes 0.3 s per 45 x 70 pair and 4 s per 270 x 480 one): the 13 planes of the channel-padded volume are
    copies of three, so the taps that fall on one plane are added up first -- W[c][s] = sum of window[i] over the i with
    clamp(c + i - 5, 0, 2) = s -- and the volume convolution becomes a 3 -> 3 channel 11 x 11 one.  Same dense fp32 window, same
    padding; test_metrics_cpu.py holds it to blur_dense at 1e-13."""
    w = oscdet.gaussian_window_3d(11).double()[0, 0]  # [i (channel), j (y), k (x)]
    w2 = torch.zeros(3, 3, 11, 11, dtype=torch.float64)
    for c in range(3):
        for i in range(11):
            w2[c, min(max(c + i - 5, 0), 2)] += w[i]
    return F.conv2d(F.pad(fields[:, 0], (5, 5, 5, 5), mode="replicate"), w2).unsqueeze(1)


def ssim_truth(a, b, val_range=0.0, blur=None):
    """float64 [N] from fp32 [N,3,H,W] inputs: the definition with the dense 3-D window, range per item."""
    if blur is None:
        blur = blur_dense if a.shape[2] * a.shape[3] <= 2000 else blur_dense_folded
    out = []
    for i in range(a.shape[0]):
        x, y = a[i:i + 1].double().unsqueeze(1), b[i:i + 1].double().unsqueeze(1)
        L = float(val_range) if val_range else range_of(a[i])
        bl = blur(torch.cat([x, y, x * x, y * y, x * y]))  # [5,1,3,H,W]
        mu1, mu2 = bl[0], bl[1]
        s1, s2, s12 = bl[2] - mu1 * mu1, bl[3] - mu2 * mu2, bl[4] - mu1 * mu2
        C1, C2 = (0.01 * L) ** 2, (0.03 * L) ** 2
        m = ((2 * mu1 * mu2 + C1) * (2.0 * s12 + C2)) / ((mu1 * mu1 + mu2 * mu2 + C1) * (s1 + s2 + C2))
        out.append(float(m.mean()))
    return np.array(out, np.float64)


def ssim_oracle32(a, b):
    """the fp32 oracle (bit-equal to the reference), item by item"""
    return np.array([float(oscdet.ssim_matlab(a[i:i + 1], b[i:i + 1])) for i in range(a.shape[0])], np.float64)


def noise_pair(h, w, seed, lo=0.0, hi=1.0):
    g = torch.Generator().manual_seed(seed)
    a = torch.rand(1, 3, h, w, generator=g)
    b = a + 0.05 * torch.randn(1, 3, h, w, generator=g)
    return a * (hi - lo) + lo, b * (hi - lo) + lo


def synth_pair_u8(h, w, seed=31):
    f = synth.make_clip(2, h, w, seed=seed)
    return np.ascontiguousarray(f[0]), np.ascontiguousarray(f[1])


def planar(u8):
    """uint8 [H,W,3] -> fp32 [1,3,H,W] / 255 (tools.to_tensor's arithmetic, on the CPU)"""
    return torch.from_numpy(np.ascontiguousarray(u8).transpose(2, 0, 1).copy()).unsqueeze(0).float().div(255.0)


def synth_pair(h, w, seed=31):
    a, b = synth_pair_u8(h, w, seed)
    return planar(a), planar(b)


def flat_pair(h, w):
    """two flat fields, 0.93 above 0.2; b = a + 1/255 on the right half: the content blur(a a) - blur(a)^2 cancels on in fp32"""
    a = torch.full((1, 3, h, w), 0.93)
    a[:, :, h // 2:] = 0.2
    b = a.clone()
    b[..., w // 2:] += 1.0 / 255.0
    return a, b


_cases = None


def ssim_cases():
    """[(name, a, b, val_range, truth [N], oracle32 [N] or None)]: computed once, shared by every test that needs them."""
    global _cases
    if _cases is not None:
        return _cases
    out = []

    def add(name, a, b, val_range=0.0, oracle=True):
        out.append((name, a, b, val_range, ssim_truth(a, b, val_range), ssim_oracle32(a, b) if oracle else None))

    for k, (h, w) in enumerate(SSIM_SHAPES):
        add(f"{h}x{w} noise", *noise_pair(h, w, 100 + k))
        add(f"{h}x{w} synth", *synth_pair(h, w))
        add(f"{h}x{w} flat", *flat_pair(h, w))
    # the range rule per item at val_range = 0: [0, 255], [0, 1], [-1, 1] in one batch
    for h, w in ((13, 37), (45, 70)):
        parts = [noise_pair(h, w, 200, 0.0, 255.0), noise_pair(h, w, 201), noise_pair(h, w, 202, -1.0, 1.0)]
        add(f"{h}x{w} N=3 ranges 255/1/2", torch.cat([p[0] for p in parts]), torch.cat([p[1] for p in parts]))
    a, b = flat_pair(45, 70)
    add("45x70 N=2: flat x 255, noise in [0,1]", torch.cat([a * 255.0, noise_pair(45, 70, 203)[0]]), torch.cat([b * 255.0, noise_pair(45, 70, 203)[1]]))
    # explicit val_range (the oracle has no such argument)
    add("13x37 noise val_range=2", *noise_pair(13, 37, 204), val_range=2.0, oracle=False)
    add("45x70 flat val_range=255 on [0,1] data", *flat_pair(45, 70), val_range=255.0, oracle=False)
    add("33x17 synth x 255 val_range=255", *[t * 255.0 for t in synth_pair(33, 17)], val_range=255.0, oracle=False)
    _cases = out
    return out


def check_ssim(fn):
    """fn(a, b, val_range) -> N floats for fp32 [N,3,H,W] inputs (val_range 0: inferred per item)."""
    rows = []
    for name, a, b, vr, truth, ora in ssim_cases():
        got = np.asarray(fn(a, b, vr), np.float64).reshape(-1)
        err = float(np.abs(got - truth).max()) if got.shape == truth.shape and np.isfinite(got).all() else float("inf")
        floor = "" if ora is None else f"fp32_oracle_err={float(np.abs(ora - truth).max()):.2e} "
        rows.append(Row("ssim3d", name, err, SSIM_TOL, f"{floor}truth={truth.round(6).tolist()}"))
    return rows


# ------------------------------------------------------------------------------------------------------- frame differences
def err_u8_ref(a, b, N, n):
    d = np.abs(a.astype(np.int64).reshape(N, n) - b.astype(np.int64).reshape(N, n))
    return np.stack([(d * d).sum(1), d.sum(1), d.max(1), (d != 0).sum(1)], 1).astype(np.int64)


def err_u8_cases():
    """[(name, a, b, N, n, off_a, off_b)]: flat uint8 arrays of N * n bytes; off_a / off_b: the byte offsets the implementation
    under test is asked to place them at (odd addresses, equal and different 16-byte phases)."""
    rng = np.random.default_rng(7)
    out = []
    for n in ERR_SIZES:
        for off_a, off_b in ((0, 0), (1, 1), (3, 9)):
            a, b = rng.integers(0, 256, 3 * n, dtype=np.uint8), rng.integers(0, 256, 3 * n, dtype=np.uint8)
            same = rng.random(3 * n) < 0.4
            b[same] = a[same]
            out.append((f"n={n} N=3 offsets {off_a}/{off_b}", a, b, 3, n, off_a, off_b))
    z, f = np.zeros(70000, np.uint8), np.full(70000, 255, np.uint8)
    out.append(("a=0 b=255 n=70000: sum d^2 > 2^32", z, f, 1, 70000, 0, 0))
    out.append(("a=255 b=0 n=70000 offsets 1/2", f, z, 1, 70000, 1, 2))
    a = rng.integers(0, 256, 3 * 363, dtype=np.uint8)
    out.append(("identical n=363 N=3", a, a.copy(), 3, 363, 1, 1))
    return out


def check_frame_error_u8(fn):
    """fn(a, b, N, n, off_a, off_b) -> integer array [N, 4] (sum d^2, sum |d|, max |d|, differing)."""
    rows = []
    for name, a, b, N, n, oa, ob in err_u8_cases():
        got, want = np.asarray(fn(a, b, N, n, oa, ob)), err_u8_ref(a, b, N, n)
        bad = float("inf") if got.shape != want.shape else float((got.astype(np.int64) != want).sum())
        rows.append(Row("frame_error_u8", name, bad, 0.0, f"bit-exact, want[0]={want[0].tolist()}"))
    return rows


def err_f32_cases():
    rng = np.random.default_rng(11)
    out = []
    for n in (1, 1000, 70001):
        a, b = rng.standard_normal(3 * n).astype(np.float32), rng.standard_normal(3 * n).astype(np.float32)
        out.append((f"n={n} N=3", a, b, 3, n))
    a, b = rng.standard_normal(3 * 5000).astype(np.float32) * 100, rng.standard_normal(3 * 5000).astype(np.float32)
    a[7], b[5000 + 4999] = np.nan, np.inf  # one NaN in item 0, one inf in item 1
    out.append(("n=5000 N=3, one NaN, one inf", a, b, 3, 5000))
    out.append(("identical n=1000", np.full(1000, 1.5, np.float32), np.full(1000, 1.5, np.float32), 1, 1000))
    return out


def err_f32_ref(a, b, N, n):
    d = np.abs(a.astype(np.float64).reshape(N, n) - b.astype(np.float64).reshape(N, n))
    fin = np.isfinite(d)
    dz = np.where(fin, d, 0.0)
    return np.stack([(dz * dz).sum(1), dz.sum(1), dz.max(1)], 1), (~fin).sum(1)


def check_frame_error_f32(fn):
    """fn(a, b, N, n) -> (float64 [N, 3]: sum d^2, sum |d|, max |d| over the finite differences; int [N]: non-finite ones)."""
    rows = []
    for name, a, b, N, n in err_f32_cases():
        got, got_nf = fn(a, b, N, n)
        want, want_nf = err_f32_ref(a, b, N, n)
        got = np.asarray(got, np.float64)
        rel = np.abs(got[:, :2] - want[:, :2]) / np.maximum(np.abs(want[:, :2]), 1e-300)
        rel = np.where(want[:, :2] == 0, np.abs(got[:, :2]), rel)
        rows.append(Row("frame_error_f32", name + " sums", float(rel.max()), 1e-12, "relative"))
        rows.append(Row("frame_error_f32", name + " max, non-finite", float((got[:, 2] != want[:, 2]).sum() + (np.asarray(got_nf) != want_nf).sum()),
                        0.0, f"exact, nonfinite={want_nf.tolist()}"))
    return rows


# ------------------------------------------------------------------------------------------- a numpy back end for the host logic
def ssim_separable64(a, b, val_range=0.0, channel_mix=True, replicate=True):
    """The definition again, written the way the kernel is (separable passes in float64 with the fp32 1-D window widened) --
    and, with channel_mix / replicate off, the two defects the rows must catch."""
    g1 = torch.tensor([float(np.exp(-(x - 5) ** 2 / (2 * 1.5 ** 2))) for x in range(11)])
    g = (g1 / g1.sum()).double()
    out = []
    for i in range(a.shape[0]):
        x, y = a[i].double(), b[i].double()
        L = float(val_range) if val_range else range_of(a[i])

        def blur(v):  # [3,H,W]
            for axis in ((0, 1, 2) if channel_mix else (1, 2)):
                pad = [0, 0, 0, 0, 0, 0]
                pad[2 * (2 - axis)] = pad[2 * (2 - axis) + 1] = 5
                vp = F.pad(v[None, None], pad, mode="replicate" if replicate else "constant")[0, 0]
                v = sum(g[k] * vp.narrow(axis, k, v.shape[axis]) for k in range(11))
            return v

        mu1, mu2 = blur(x), blur(y)
        s1, s2, s12 = blur(x * x) - mu1 * mu1, blur(y * y) - mu2 * mu2, blur(x * y) - mu1 * mu2
        C1, C2 = (0.01 * L) ** 2, (0.03 * L) ** 2
        m = ((2 * mu1 * mu2 + C1) * (2.0 * s12 + C2)) / ((mu1 * mu1 + mu2 * mu2 + C1) * (s1 + s2 + C2))
        out.append(float(m.mean()))
    return out


class NumpyBackend:
    """drba_amd.metrics' back-end protocol on the host (tests only: the product has no CPU path).  Frames are uint8 HWC."""

    def __init__(self):
        self.pairs = []  # every pair measured, in order

    def prepare(self, x):
        x = x.numpy() if torch.is_tensor(x) else np.asarray(x)
        if x.dtype == np.uint8 and x.ndim in (3, 4) and x.shape[-1] == 3:
            return x, "u8", (1 if x.ndim == 3 else x.shape[0], x.shape[-3], x.shape[-2])
        if x.dtype == np.float32 and x.ndim == 4 and x.shape[1] == 3:
            return x, "f32", (x.shape[0], x.shape[2], x.shape[3])
        raise TypeError(f"got {x.dtype} {x.shape}")

    def slots(self, capacity):
        return [None] * int(capacity)

    def measure(self, slots, k, a, b, kind, shape, val_range, want_ssim=True):
        n, h, w = shape
        for i in range(n):
            fa = a.reshape(n, *a.shape[-3:])[i]
            fb = b.reshape(n, *b.shape[-3:])[i]
            self.pairs.append((fa, fb))
            if kind == "u8":
                e = err_u8_ref(fa.reshape(-1), fb.reshape(-1), 1, fa.size)[0]
                row = [int(v) for v in e]
                pa, pb = planar(fa), planar(fb)
            else:
                s, nf = err_f32_ref(fa.reshape(-1), fb.reshape(-1), 1, fa.size)
                row = [float(s[0, 0]), float(s[0, 1]), float(s[0, 2]), int(nf[0])]
                pa, pb = torch.from_numpy(fa)[None], torch.from_numpy(fb)[None]
            ss = ssim_separable64(pa, pb, val_range or 0.0)[0] if (want_ssim and h >= 11 and w >= 11) else float("nan")
            slots[k + i] = tuple(row) + (ss,)

    def collect(self, slots_list, counts):
        return [s[i] for s, (n, _) in zip(slots_list, counts) for i in range(n)]
